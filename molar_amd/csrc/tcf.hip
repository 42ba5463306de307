// tcf.hip - time correlation functions of vectors over a block of trajectory frames: for every tuple of atoms a vector per
// frame (an atom's own 3-vector, a bond, a plane normal), and over all time origins the first and second Legendre
// polynomial of the cosine between the vector at t and at t + tau (gmx rotacf -P 1 / 2, gmx velacc), per vector and per group
// of vectors, with the mean vector and the order parameter S^2 of every vector.  The definition is in molar_hip.h.
//
//   w_v(f)  = p[a] | sv(p[b] - p[a]) | sv(p[b] - p[a]) x sv(p[c] - p[a]),   components outside dims set to 0
//   u_v(f)  = w / sqrt((wx^2 + wy^2) + wz^2)  (UNIT)  |  w  (RAW)
//   d       = u(t) . u(t + tau),   S1_v[tau] = sum_t d,   S2_v[tau] = sum_t d^2,   t = 0, origin_stride, ... while t + tau <= F - 1
//
// Stages, all on the context's stream:
//
//   boxes (one thread per box: the f64 PeriodicBox of box9)
//   ->  vectors: a workgroup takes TCF_VECS vectors and TCF_FRAMES frames, a lane owns a vector and walks its frames: u into
//       U [V][F][3] (f64, vector-major), the chunk's partial first and second moments and its count of bad frames into the
//       workspace; indices and labels are judged here (a bad index reads atom 0)
//   ->  64 bytes read back: the status
//   ->  fold: one lane per vector adds the chunks in chunk order: mean, s2, bad_frames, the valid flag, nvalid (integer atomics)
//   ->  lags: a workgroup of one wave owns a chunk of vectors and a block of 64 R lags, a lane owns R consecutive lags (below)
//   ->  finish: the chunks in order, the scaling.
//
// No floating-point atomics: every sum has an order fixed by the launch geometry, which depends on the sizes alone.
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "boxmath.hpp"
#include "common.hpp"
#include "traj_block.hpp"

using namespace mh;

struct molar_hip_tcf_state {
    DevBuf in_frames, in_tuples, in_labels, in_boxes;                                   // host inputs staged here
    DevBuf ws;                                                                           // the workspace molar_hip_tcf_plan reports
    DevBuf out_c1, out_c2, out_c1v, out_c2v, out_mean, out_s2, out_bad;                  // results on their way to host memory
};

namespace {

typedef unsigned long long u64;

constexpr uint32_t TCF_VECS = 256;           // vectors per workgroup of the vector stage: one per lane
constexpr uint32_t TCF_FRAMES = 64;          // frames per workgroup of the vector stage, walked in order by every lane
constexpr uint32_t TCF_LANES = 64;           // lanes of a workgroup of the lag kernel: one wave
constexpr uint32_t TCF_R = 4;                // lags per lane (MOLAR_HIP_TCF_R = 1, 2 or 4 for A/B runs)
constexpr uint32_t TCF_SEG = 128;            // frames of origins per staged segment (a multiple of every R)
constexpr size_t TCF_TARGET_WGS = 8192;      // workgroups the lag kernel aims for
constexpr uint32_t TCF_MAX_CHUNK = 64;       // vectors per workgroup of the lag kernel at the most
constexpr uint32_t TCF_MOMENTS = 9;          // x, y, z, xx, yy, zz, xy, xz, yz

// flags[0]: a tuple index not below natoms; [1]: a box matrix without an inverse; [3]: a box vector of zero length;
// [5]: a label not below ngroups
constexpr uint32_t TCF_FLAG_WORDS = 16;

uint32_t lags_per_lane() {
    const char *e = std::getenv("MOLAR_HIP_TCF_R");
    if (e && (e[0] == '1' || e[0] == '2' || e[0] == '4') && e[1] == 0) return (uint32_t)(e[0] - '0');
    return TCF_R;
}

// Where everything lives in the workspace, from the sizes alone (the plan entry and the call share it).
struct Layout {
    size_t fchunks;                   // chunks of TCF_FRAMES frames
    uint32_t R, lag_block, nlb_main, tail_R, chunk, nchunks;   // the lag stage: lags per lane and per block, whole blocks, the lane width of the last block
    size_t off_flags, off_boxes, off_mom, off_bad, off_valid, off_nvalid, off_traj, off_part, bytes;
};

Layout make_layout(size_t F, size_t V, size_t G, size_t L, bool per_frame_boxes, bool want_lags, bool want_groups) {
    Layout Y{};
    Y.fchunks = (F + TCF_FRAMES - 1) / TCF_FRAMES;
    Y.R = lags_per_lane();
    Y.lag_block = TCF_LANES * Y.R;
    Y.nlb_main = (uint32_t)((L + 1) / Y.lag_block);
    const size_t rest = (L + 1) % Y.lag_block;
    Y.tail_R = rest == 0 ? 0u : rest <= TCF_LANES ? 1u : rest <= 2 * TCF_LANES ? 2u : 4u;   // the narrowest lane that holds the rest
    const size_t nlb = Y.nlb_main + (rest ? 1 : 0);
    const size_t per = V * nlb / TCF_TARGET_WGS;
    Y.chunk = (uint32_t)std::max<size_t>(1, std::min<size_t>(TCF_MAX_CHUNK, per));
    Y.nchunks = (uint32_t)((V + Y.chunk - 1) / Y.chunk);
    // the chunks never exceed this, which grows with V: the reservation never shrinks when an argument grows
    const size_t chunks_bound = std::min<size_t>(V, 2 * TCF_TARGET_WGS) + V / TCF_MAX_CHUNK + 1;
    Carve ws;
    ws.take(Y.off_flags, TCF_FLAG_WORDS * 4);
    ws.take(Y.off_boxes, (per_frame_boxes ? F : 1) * sizeof(BoxD));
    ws.take(Y.off_mom, Y.fchunks * TCF_MOMENTS * V * 8);
    ws.take(Y.off_bad, Y.fchunks * V * 4);
    ws.take(Y.off_valid, V * 4);
    ws.take(Y.off_nvalid, G * 8);
    ws.take(Y.off_traj, want_lags ? V * F * 3 * 8 : 0);
    ws.take(Y.off_part, want_lags && want_groups ? chunks_bound * G * (L + 1) * 2 * 8 : 0);
    Y.bytes = ws.bytes;
    return Y;
}

// PeriodicBox::from_matrix in double on the device (box_from_matrix of boxmath.hpp, operation by operation, its two errors
// included); 0: a box, 1: a box vector of zero length, 2: a matrix without an inverse.
__device__ int tcf_build_box(const double *m9, BoxD *out) {
    D3 col[3];
    bool ok = true;
    for (int k = 0; k < 3; ++k) {
        col[k] = D3{m9[3 * k], m9[3 * k + 1], m9[3 * k + 2]};
        if (sqrt(norm2(col[k])) == 0.0) ok = false;
    }
    for (int q = 0; q < 9; ++q) {
        out->m[q] = m9[q];
        out->inv[q] = __builtin_nan("");
    }
    out->nshift = 0;
    if (!ok) return 1;
    if (!inverse3(out->m, out->inv)) return 2;
    const bool ortho = m9[3] == 0.0 && m9[6] == 0.0 && m9[1] == 0.0 && m9[7] == 0.0 && m9[2] == 0.0 && m9[5] == 0.0;
    if (ortho) return 0;
    const D3 a = col[0], b = col[1], c = col[2], na = D3{-a.x, -a.y, -a.z};
    const double longest = fmax(fmax(fmax(sqrt(norm2((a + b) + c)), sqrt(norm2((a + b) - c))), sqrt(norm2((a - b) + c))), sqrt(norm2((na + b) + c)));
    const double half_diag = 0.5 * longest, two = 2.0 * half_diag, bound2 = two * two;
    for (int i = -1; i <= 1; ++i)
        for (int j = -1; j <= 1; ++j)
            for (int k = -1; k <= 1; ++k) {
                if (!i && !j && !k) continue;
                const double fi = (double)i, fj = (double)j, fk = (double)k;
                const D3 sft = (D3{fi * a.x, fi * a.y, fi * a.z} + D3{fj * b.x, fj * b.y, fj * b.z}) + D3{fk * c.x, fk * c.y, fk * c.z};
                if (norm2(sft) < bound2) {
                    double *dst = out->shifts + 3 * out->nshift++;
                    dst[0] = sft.x;
                    dst[1] = sft.y;
                    dst[2] = sft.z;
                }
            }
    return 0;
}

// One thread per box.
template <class Real>
__global__ void __launch_bounds__(64) tcf_box_kernel(const Real *__restrict__ boxes, size_t nbox, BoxD *__restrict__ out, uint32_t *__restrict__ flags) {
    const size_t f = (size_t)blockIdx.x * 64u + threadIdx.x;
    if (f >= nbox) return;
    double m9[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) m9[q] = (double)boxes[f * 9 + q];
    const int bad = tcf_build_box(m9, out + f);
    if (bad == 1) flags[3] = 1u;
    if (bad == 2) flags[1] = 1u;
}

__device__ __forceinline__ D3 cross3(D3 a, D3 b) { return D3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }

template <class Real>
struct VecP {
    const Real *frames;
    size_t stride, F, natoms;
    const uint64_t *tuples;
    const uint32_t *labels;       // judged here when in device memory; null: nothing to judge
    size_t V, G;
    const BoxD *boxes;            // null: no image is removed
    uint32_t box_step, pbc, dims, unit;
    uint32_t vblocks;             // workgroups along the vectors; blockIdx.x = frame chunk * vblocks + vector block
    double *traj;                 // [V][F][3], or null
    double *mom;                  // [frame chunks][TCF_MOMENTS][V]
    uint32_t *bad;                // [frame chunks][V]
};

template <class Real>
__device__ __forceinline__ D3 tcf_atom(const Real *p, uint64_t a) {
    return D3{(double)p[3 * a], (double)p[3 * a + 1], (double)p[3 * a + 2]};
}

// The vector stage.  A lane owns vector v and walks the frames of its chunk in order.  A frame is bad when a component of w
// (after the mask) is not finite or, in UNIT mode, |w|^2 is exactly 0: it is counted, stored as zeros and enters no moment.
template <class Real, int KIND>
__global__ void __launch_bounds__(TCF_VECS) tcf_vector_kernel(VecP<Real> P, uint32_t *__restrict__ flags) {
    const uint32_t chunk = blockIdx.x / P.vblocks, vb = blockIdx.x - chunk * P.vblocks;
    const size_t v = (size_t)vb * TCF_VECS + threadIdx.x;
    if (v >= P.V) return;
    uint64_t a[KIND];
    bool beyond = false;
#pragma unroll
    for (int j = 0; j < KIND; ++j) {
        const uint64_t k = P.tuples[v * KIND + j];
        const bool out = k >= P.natoms;
        beyond = beyond || out;
        a[j] = out ? 0 : k;
    }
    if (beyond) flags[0] = 1u;
    if (chunk == 0u && P.labels && P.labels[v] >= P.G) flags[5] = 1u;
    const size_t f0 = (size_t)chunk * TCF_FRAMES, f1 = f0 + TCF_FRAMES < P.F ? f0 + TCF_FRAMES : P.F;
    double m[TCF_MOMENTS];
#pragma unroll
    for (uint32_t k = 0; k < TCF_MOMENTS; ++k) m[k] = 0.0;
    uint32_t nbad = 0;
    for (size_t f = f0; f < f1; ++f) {
        const Real *p = P.frames + f * P.stride;
        D3 w = tcf_atom(p, a[0]);
        if constexpr (KIND >= 2) {
            const BoxD *box = P.boxes ? P.boxes + f * P.box_step : nullptr;
            D3 b = tcf_atom(p, a[1]) - w;
            if (box) b = shortest_vector(*box, b, P.pbc);
            if constexpr (KIND == 3) {
                D3 c = tcf_atom(p, a[2]) - w;
                if (box) c = shortest_vector(*box, c, P.pbc);
                w = cross3(b, c);
            } else {
                w = b;
            }
        }
        if (!(P.dims & 1u)) w.x = 0.0;
        if (!(P.dims & 2u)) w.y = 0.0;
        if (!(P.dims & 4u)) w.z = 0.0;
        bool ok = isfinite(w.x) && isfinite(w.y) && isfinite(w.z);
        if (P.unit) {
            const double n2 = norm2(w);
            if (n2 == 0.0) ok = false;
            const double len = sqrt(n2);
            w = D3{w.x / len, w.y / len, w.z / len};
        }
        if (!ok) {
            ++nbad;
            w = D3{0.0, 0.0, 0.0};
        } else {
            m[0] += w.x;
            m[1] += w.y;
            m[2] += w.z;
            m[3] += w.x * w.x;
            m[4] += w.y * w.y;
            m[5] += w.z * w.z;
            m[6] += w.x * w.y;
            m[7] += w.x * w.z;
            m[8] += w.y * w.z;
        }
        if (P.traj) {
            double *dst = P.traj + (v * P.F + f) * 3;
            dst[0] = w.x;
            dst[1] = w.y;
            dst[2] = w.z;
        }
    }
#pragma unroll
    for (uint32_t k = 0; k < TCF_MOMENTS; ++k) P.mom[((size_t)chunk * TCF_MOMENTS + k) * P.V + v] = m[k];
    P.bad[(size_t)chunk * P.V + v] = nbad;
}

// One lane per vector: the chunks in chunk order.  mean = S / F; s2 = 1.5 q - 0.5 with
// q = ((xx^2 + yy^2) + zz^2) + 2 ((xy^2 + xz^2) + yz^2) of the second moments over F.  A vector with a bad frame: NaN, valid 0.
template <class Real>
__global__ void __launch_bounds__(TCF_VECS) tcf_fold_kernel(const double *__restrict__ mom, const uint32_t *__restrict__ bad, size_t fchunks, size_t V, size_t F,
                                                            const uint32_t *__restrict__ labels, uint32_t *__restrict__ valid, u64 *__restrict__ nvalid,
                                                            Real *__restrict__ mean, Real *__restrict__ s2, uint32_t *__restrict__ bad_frames) {
    const size_t v = (size_t)blockIdx.x * TCF_VECS + threadIdx.x;
    if (v >= V) return;
    double m[TCF_MOMENTS];
#pragma unroll
    for (uint32_t k = 0; k < TCF_MOMENTS; ++k) m[k] = 0.0;
    uint32_t nbad = 0;
    for (size_t c = 0; c < fchunks; ++c) {
#pragma unroll
        for (uint32_t k = 0; k < TCF_MOMENTS; ++k) m[k] += mom[(c * TCF_MOMENTS + k) * V + v];
        nbad += bad[c * V + v];
    }
    const bool ok = nbad == 0u;
    const double nan = __builtin_nan(""), dF = (double)F;
#pragma unroll
    for (uint32_t k = 0; k < TCF_MOMENTS; ++k) m[k] = m[k] / dF;
    valid[v] = ok ? 1u : 0u;
    if (ok) atomicAdd(&nvalid[labels ? labels[v] : 0u], (u64)1);
    if (bad_frames) bad_frames[v] = nbad;
    if (mean) {
#pragma unroll
        for (int d = 0; d < 3; ++d) mean[v * 3 + d] = (Real)(ok ? m[d] : nan);
    }
    if (s2) {
        const double q = ((m[3] * m[3] + m[4] * m[4]) + m[5] * m[5]) + 2.0 * ((m[6] * m[6] + m[7] * m[7]) + m[8] * m[8]);
        s2[v] = (Real)(ok ? 1.5 * q - 0.5 : nan);
    }
}

struct LagQ {
    const double *traj;           // [V][F][3]
    const uint32_t *valid;        // [V]
    const uint32_t *labels;       // [V] or null
    size_t V, F, L, os, G;        // vectors, frames, largest lag, origin stride, groups
    size_t l_base;                // the first lag of this launch
    uint32_t chunk, nchunks;
    double *part;                 // [chunk][G][L + 1][2]: sums of d and d^2 over the chunk's vectors, zeroed; null: no group curve
};

typedef double tcf_d2 __attribute__((ext_vector_type(2)));
typedef double tcf_d4 __attribute__((ext_vector_type(4)));

// R consecutive doubles of LDS at an index that is a multiple of R: one wide read
template <uint32_t R>
__device__ __forceinline__ void lds_group(const double *p, double *out) {
    if constexpr (R == 4) {
        const tcf_d4 x = *reinterpret_cast<const tcf_d4 *>(p);
        out[0] = x.x;
        out[1] = x.y;
        out[2] = x.z;
        out[3] = x.w;
    } else if constexpr (R == 2) {
        const tcf_d2 x = *reinterpret_cast<const tcf_d2 *>(p);
        out[0] = x.x;
        out[1] = x.y;
    } else {
        out[0] = *p;
    }
}

// The R^2 pairs of a step: origin k against lag j meets window value k + j of the two groups lo | hi.
template <uint32_t R, bool P2>
__device__ __forceinline__ void tcf_pairs(const double (&O)[3][R], const double (&lo)[3][R], const double (&hi)[3][R], double (&s1)[R], double (&s2)[R]) {
#pragma unroll
    for (uint32_t k = 0; k < R; ++k)
#pragma unroll
        for (uint32_t j = 0; j < R; ++j) {
            const uint32_t i = k + j;
            const double wx = i < R ? lo[0][i % R] : hi[0][i % R], wy = i < R ? lo[1][i % R] : hi[1][i % R], wz = i < R ? lo[2][i % R] : hi[2][i % R];
            const double dd = fma(O[2][k], wz, fma(O[1][k], wy, O[0][k] * wx));
            s1[j] += dd;
            if (P2) s2[j] = fma(dd, dd, s2[j]);
        }
}

// Workgroup (chunk of vectors, block of 64 R lags), one wave; blockIdx.x = lag block * chunks + chunk, so that the blocks of
// short lags - the long ones - start first.  Lane l holds the lags tau_j = l0 + R l + j, j < R.  Per vector the frames of
// origins go by in segments of TCF_SEG: the window u(t0 + l0 .. + TCF_SEG + 64 R) and the origins u(t0 .. t0 + TCF_SEG) are
// staged in LDS, one array per component, zeros behind the last frame and behind the last origin of the segment: a pair that
// the definition leaves out adds an exact zero to both sums, so that no pair is predicated.  origin_stride == 1: R origins at
// a time; the lane holds the groups q = step + l and q + 1 of R window values each (one wide read per step and component,
// the second group becomes the first) and R origin values (one wide read, the same address in every lane) and forms the R^2
// dot products u(t + k) . u(t + k + tau_j) from W[k + j]: per pair 3 operations for d, one for S1, one for S2.  A larger stride: one
// origin at a time against the lane's R window values.  Either way a lag's sum runs over the origins in order, then over the
// chunk's valid vectors in index order.
template <class Real, uint32_t R, bool P2>
__global__ void __launch_bounds__(TCF_LANES) tcf_lag_kernel(LagQ Q, Real *__restrict__ c1_vec, size_t ld1, Real *__restrict__ c2_vec, size_t ld2) {
    constexpr uint32_t LB = TCF_LANES * R, WIN = TCF_SEG + LB;
    static_assert(TCF_SEG % R == 0, "whole steps of R origins");
    __shared__ __attribute__((aligned(32))) double shw[3][WIN];
    __shared__ __attribute__((aligned(32))) double sho[3][TCF_SEG];
    const uint32_t lb = blockIdx.x / Q.nchunks, ch = blockIdx.x - lb * Q.nchunks, lane = threadIdx.x;
    const size_t l0 = Q.l_base + (size_t)lb * LB, tau0 = l0 + (size_t)R * lane;
    const size_t g0 = (size_t)ch * Q.chunk, g1 = g0 + Q.chunk < Q.V ? g0 + Q.chunk : Q.V;
    const size_t tend = Q.F - l0;                                       // origins t < tend reach lag l0 (l0 <= L < F)
    double count[R];
#pragma unroll
    for (uint32_t j = 0; j < R; ++j) count[j] = tau0 + j <= Q.L ? (double)((Q.F - 1 - (tau0 + j)) / Q.os + 1) : 1.0;
    double tot1[R], tot2[R];
#pragma unroll
    for (uint32_t j = 0; j < R; ++j) tot1[j] = tot2[j] = 0.0;
    uint32_t cur = Q.labels ? Q.labels[g0] : 0u;
    auto flush = [&](uint32_t label) {
        if (!Q.part) return;
#pragma unroll
        for (uint32_t j = 0; j < R; ++j)
            if (tau0 + j <= Q.L) {
                double *dst = Q.part + ((((size_t)ch * Q.G + label) * (Q.L + 1)) + tau0 + j) * 2;
                dst[0] += tot1[j];
                if (P2) dst[1] += tot2[j];
            }
    };
    for (size_t g = g0; g < g1; ++g) {
        const uint32_t label = Q.labels ? Q.labels[g] : 0u;
        if (label != cur) {
            flush(cur);
#pragma unroll
            for (uint32_t j = 0; j < R; ++j) tot1[j] = tot2[j] = 0.0;
            cur = label;
        }
        if (!Q.valid[g]) {
#pragma unroll
            for (uint32_t j = 0; j < R; ++j)
                if (tau0 + j <= Q.L) {
                    if (c1_vec) c1_vec[g * ld1 + tau0 + j] = (Real)__builtin_nan("");
                    if (P2 && c2_vec) c2_vec[g * ld2 + tau0 + j] = (Real)__builtin_nan("");
                }
            continue;
        }
        const double *__restrict__ U = Q.traj + g * Q.F * 3;
        double s1[R], s2[R];
#pragma unroll
        for (uint32_t j = 0; j < R; ++j) s1[j] = s2[j] = 0.0;
        for (size_t t0 = 0; t0 < tend; t0 += TCF_SEG) {
            const size_t t1 = t0 + TCF_SEG < tend ? t0 + TCF_SEG : tend;
            size_t t = (t0 + Q.os - 1) / Q.os * Q.os;                   // the first origin of the segment
            if (t >= t1) continue;
            const size_t w0 = t0 + l0;
            __syncthreads();
            for (uint32_t i = lane; i < WIN; i += TCF_LANES) {
                const bool in = w0 + i < Q.F;
#pragma unroll
                for (int d = 0; d < 3; ++d) shw[d][i] = in ? U[(w0 + i) * 3 + d] : 0.0;
            }
            for (uint32_t i = lane; i < TCF_SEG; i += TCF_LANES) {
                const bool in = t0 + i < t1;
#pragma unroll
                for (int d = 0; d < 3; ++d) sho[d][i] = in ? U[(t0 + i) * 3 + d] : 0.0;
            }
            __syncthreads();
            if (Q.os == 1) {
                // two steps per turn, the two groups changing places, so that no register is copied; a step past the last
                // origin of the segment (TCF_SEG / R is even) meets zeros
                const uint32_t nsteps = (uint32_t)((t1 - t0 + 2 * R - 1) / (2 * R)) * 2u;
                double A[3][R], B[3][R], O[3][R];
#pragma unroll
                for (int d = 0; d < 3; ++d) lds_group<R>(&shw[d][R * lane], A[d]);
                for (uint32_t s = 0; s < nsteps; s += 2) {
#pragma unroll
                    for (int d = 0; d < 3; ++d) {
                        lds_group<R>(&shw[d][R * (s + lane + 1)], B[d]);
                        lds_group<R>(&sho[d][R * s], O[d]);
                    }
                    tcf_pairs<R, P2>(O, A, B, s1, s2);
#pragma unroll
                    for (int d = 0; d < 3; ++d) {
                        lds_group<R>(&shw[d][R * (s + lane + 2)], A[d]);
                        lds_group<R>(&sho[d][R * (s + 1)], O[d]);
                    }
                    tcf_pairs<R, P2>(O, B, A, s1, s2);
                }
            } else {
                for (; t < t1; t += Q.os) {
                    const uint32_t i = (uint32_t)(t - t0);
                    const double ox = sho[0][i], oy = sho[1][i], oz = sho[2][i];
#pragma unroll
                    for (uint32_t j = 0; j < R; ++j) {
                        const uint32_t w = i + R * lane + j;
                        const double dd = fma(oz, shw[2][w], fma(oy, shw[1][w], ox * shw[0][w]));
                        s1[j] += dd;
                        if (P2) s2[j] = fma(dd, dd, s2[j]);
                    }
                }
            }
        }
#pragma unroll
        for (uint32_t j = 0; j < R; ++j) {
            if (tau0 + j <= Q.L) {
                if (c1_vec) c1_vec[g * ld1 + tau0 + j] = (Real)(s1[j] / count[j]);
                if (P2 && c2_vec) c2_vec[g * ld2 + tau0 + j] = (Real)(1.5 * (s2[j] / count[j]) - 0.5);
            }
            tot1[j] += s1[j];
            if (P2) tot2[j] += s2[j];
        }
    }
    flush(cur);
}

// One thread per group and lag: the chunks in order, then the scaling by N_g n(tau); a group without a valid vector: NaN.
template <class Real>
__global__ void __launch_bounds__(256) tcf_finish_kernel(LagQ Q, const u64 *__restrict__ nvalid, Real *__restrict__ c1, Real *__restrict__ c2) {
    const size_t k = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (k >= Q.G * (Q.L + 1)) return;
    const size_t g = k / (Q.L + 1), tau = k - g * (Q.L + 1);
    double a = 0.0, b = 0.0;
    for (uint32_t ch = 0; ch < Q.nchunks; ++ch) {
        const double *src = Q.part + (((size_t)ch * Q.G + g) * (Q.L + 1) + tau) * 2;
        a += src[0];
        b += src[1];
    }
    const u64 n = nvalid[g];
    const double scale = (double)n * (double)((Q.F - 1 - tau) / Q.os + 1), nan = __builtin_nan("");
    if (c1) c1[k] = (Real)(n ? a / scale : nan);
    if (c2) c2[k] = (Real)(n ? 1.5 * (b / scale) - 0.5 : nan);
}

template <class Real, uint32_t R>
void launch_lags_r(hipStream_t st, const LagQ &Q, uint32_t nblocks, bool p2, Real *c1v, size_t ld1, Real *c2v, size_t ld2) {
    const dim3 grid(nblocks * Q.nchunks), wg(TCF_LANES);
    if (p2) hipLaunchKernelGGL((tcf_lag_kernel<Real, R, true>), grid, wg, 0, st, Q, c1v, ld1, c2v, ld2);
    else hipLaunchKernelGGL((tcf_lag_kernel<Real, R, false>), grid, wg, 0, st, Q, c1v, ld1, c2v, ld2);
}
template <class Real>
void launch_lags(hipStream_t st, uint32_t R, const LagQ &Q, uint32_t nblocks, bool p2, Real *c1v, size_t ld1, Real *c2v, size_t ld2) {
    if (R == 4) launch_lags_r<Real, 4>(st, Q, nblocks, p2, c1v, ld1, c2v, ld2);
    else if (R == 2) launch_lags_r<Real, 2>(st, Q, nblocks, p2, c1v, ld1, c2v, ld2);
    else launch_lags_r<Real, 1>(st, Q, nblocks, p2, c1v, ld1, c2v, ld2);
}

template <class T>
int walk_below(const char *who, const char *name, const T *v, size_t count, size_t bound, const char *bound_name) {
    if (v && !is_device_ptr(v))
        for (size_t k = 0; k < count; ++k)
            if (v[k] >= bound)
                return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: %s[%zu] = %llu is not below %s = %zu", who, name, k, (unsigned long long)v[k], bound_name, bound);
    return 0;
}

template <class Real>
int tcf_run(molar_hip_ctx *c, const char *who, const Real *frames, size_t F, size_t stride, size_t natoms, const uint64_t *tuples, size_t V,
            const uint32_t *labels, size_t ngroups, const Real *boxes, size_t box_stride, uint8_t pbc, const molar_hip_tcf_spec *spec, size_t max_lag,
            size_t origin_stride, Real *c1, Real *c2, Real *c1_vec, Real *c2_vec, size_t ld, uint64_t *nvalid, Real *mean, Real *s2, uint32_t *bad_frames) {
    // the arguments are judged before the context is used
    if (!c) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "null context");
    const size_t G = labels ? ngroups : 1, L = max_lag;
    if (V == 0) return fail(MOLAR_HIP_ERR_SIZES, "%s: no vectors", who);
    if (G == 0) return fail(MOLAR_HIP_ERR_SIZES, "%s: labels and ngroups = 0", who);
    if ((c1_vec || c2_vec) && ld < L + 1) return fail(MOLAR_HIP_ERR_SIZES, "%s: ld = %zu is below the %zu lags of a row", who, ld, L + 1);
    if (!spec) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: the spec is null", who);
    const uint32_t kind = spec->kind;
    if (kind < 1 || kind > 3) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: kind = %u is not 1 (atom), 2 (bond) or 3 (plane normal)", who, kind);
    if (spec->mode != MOLAR_HIP_TCF_UNIT && spec->mode != MOLAR_HIP_TCF_RAW) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: mode = %u is neither UNIT (0) nor RAW (1)", who, spec->mode);
    if (spec->dims == 0 || spec->dims > 7) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: dims = %u is not one of 1 .. 7", who, spec->dims);
    if (spec->reserved != 0) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: the reserved field of the spec is not zero", who);
    if (pbc > 7) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: pbc = %u is not a PbcDims byte", who, (unsigned)pbc);
    if (box_stride != 0 && box_stride != 9) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: box_stride = %zu is neither 0 nor 9", who, box_stride);
    if (F >= 1 && L >= F) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: max_lag = %zu is not below nframes = %zu", who, L, F);
    if (origin_stride == 0) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: origin_stride is zero", who);
    if (spec->mode == MOLAR_HIP_TCF_RAW && (c2 || c2_vec || s2)) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: c2, c2_vec and s2 are defined in UNIT mode only", who);
    if (!tuples) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: the tuples pointer is null", who);
    if (natoms == 0) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: %zu vectors out of natoms = 0", who, V);
    MH_TRY(check_stride(who, "the frame stride", F, stride, natoms));
    const bool use_box = kind >= 2 && pbc != 0;
    if (use_box && !boxes) return fail(MOLAR_HIP_ERR_NO_PBC, "%s: pbc operation without periodic box", who);
    const size_t fchunks = (F + TCF_FRAMES - 1) / TCF_FRAMES, vblocks = (V + TCF_VECS - 1) / TCF_VECS;
    if (V >= 0x7FFFFF00ull || G >= 0x7FFFFF00ull || F >= 0x7FFFFFF0ull || fchunks * vblocks >= 0x7FFFFFFFull)
        return fail(MOLAR_HIP_ERR_TOO_LARGE, "%s: more than 2^31 vectors, groups, frames or workgroups", who);
    if (F == 0) return MOLAR_HIP_OK;
    if (!frames) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: the frames pointer is null", who);
    // tuples and labels in host memory are walked here; those in device memory are judged by the vector stage, where a bad
    // index reads atom 0, and a label is an address only behind the status
    MH_TRY(check_index(who, "tuples", tuples, V * kind, natoms));
    MH_TRY(walk_below(who, "labels", labels, V, G, "ngroups"));
    MH_HIP(hipSetDevice(c->device));

    const bool want_p2 = c2 || c2_vec, want_groups = c1 || c2, want_lags = want_groups || c1_vec || c2_vec;
    const Layout Y = make_layout(F, V, G, L, use_box && box_stride == 9, want_lags, want_groups);
    if (want_lags && ((size_t)Y.nlb_main + 1) * Y.nchunks >= 0x7FFFFFFFull) return fail(MOLAR_HIP_ERR_TOO_LARGE, "%s: more than 2^31 workgroups", who);
    molar_hip_tcf_state &Z = state_of(c->tcf);
    MH_TRY(grow_exact(Z.ws, Y.bytes, who, "the workspace"));
    char *W = Z.ws.as<char>();
    uint32_t *flags = reinterpret_cast<uint32_t *>(W + Y.off_flags);
    BoxD *boxd = reinterpret_cast<BoxD *>(W + Y.off_boxes);
    double *mom_d = reinterpret_cast<double *>(W + Y.off_mom), *traj_d = reinterpret_cast<double *>(W + Y.off_traj), *part_d = reinterpret_cast<double *>(W + Y.off_part);
    uint32_t *bad_d = reinterpret_cast<uint32_t *>(W + Y.off_bad), *valid_d = reinterpret_cast<uint32_t *>(W + Y.off_valid);
    u64 *nvalid_d = reinterpret_cast<u64 *>(W + Y.off_nvalid);

    Real *c1_d, *c2_d, *c1v_d, *c2v_d, *mean_d, *s2_d;
    uint32_t *badf_d;
    MH_TRY(out_buffer(c1, G * (L + 1), Z.out_c1, who, &c1_d));
    MH_TRY(out_buffer(c2, G * (L + 1), Z.out_c2, who, &c2_d));
    MH_TRY(out_buffer(c1_vec, V * (L + 1), Z.out_c1v, who, &c1v_d));
    MH_TRY(out_buffer(c2_vec, V * (L + 1), Z.out_c2v, who, &c2v_d));
    MH_TRY(out_buffer(mean, V * 3, Z.out_mean, who, &mean_d));
    MH_TRY(out_buffer(s2, V, Z.out_s2, who, &s2_d));
    MH_TRY(out_buffer(bad_frames, V, Z.out_bad, who, &badf_d));

    VecP<Real> P{};
    const Real *boxes_dev = nullptr;
    const uint32_t *labels_dev = nullptr;
    const size_t nbox = use_box ? (box_stride ? F : 1) : 0;
    MH_TRY(to_device(c, frames, (F - 1) * stride + natoms * 3, Z.in_frames, &P.frames));
    MH_TRY(to_device(c, tuples, V * kind, Z.in_tuples, &P.tuples));
    MH_TRY(to_device(c, labels, labels ? V : 0, Z.in_labels, &labels_dev));
    MH_TRY(to_device(c, use_box ? boxes : nullptr, nbox * 9, Z.in_boxes, &boxes_dev));
    P.stride = stride;
    P.F = F;
    P.natoms = natoms;
    P.labels = is_device_ptr(labels) ? labels_dev : nullptr;
    P.V = V;
    P.G = G;
    P.boxes = use_box ? boxd : nullptr;
    P.box_step = box_stride ? 1u : 0u;
    P.pbc = pbc;
    P.dims = spec->dims;
    P.unit = spec->mode == MOLAR_HIP_TCF_UNIT ? 1u : 0u;
    P.vblocks = (uint32_t)vblocks;
    P.traj = want_lags ? traj_d : nullptr;
    P.mom = mom_d;
    P.bad = bad_d;

    MH_HIP(hipMemsetAsync(flags, 0, TCF_FLAG_WORDS * 4, c->stream));
    MH_HIP(hipMemsetAsync(nvalid_d, 0, G * 8, c->stream));
    if (use_box) hipLaunchKernelGGL(tcf_box_kernel<Real>, dim3((uint32_t)((nbox + 63) / 64)), dim3(64), 0, c->stream, boxes_dev, nbox, boxd, flags);
    const dim3 vgrid((uint32_t)(fchunks * vblocks)), vwg(TCF_VECS);
    if (kind == 1) hipLaunchKernelGGL((tcf_vector_kernel<Real, 1>), vgrid, vwg, 0, c->stream, P, flags);
    else if (kind == 2) hipLaunchKernelGGL((tcf_vector_kernel<Real, 2>), vgrid, vwg, 0, c->stream, P, flags);
    else hipLaunchKernelGGL((tcf_vector_kernel<Real, 3>), vgrid, vwg, 0, c->stream, P, flags);
    MH_HIP(hipGetLastError());
    // the one read-back: the status.  Nothing below runs, no label is used as an address and no output is touched after a bad
    // argument.
    uint32_t hf[TCF_FLAG_WORDS];
    MH_TRY(read_back(c, hf, flags, sizeof hf));
    if (hf[0]) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: a tuple index is not below natoms = %zu", who, natoms);
    if (hf[5]) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: a label is not below ngroups = %zu", who, G);
    if (hf[3]) return fail(MOLAR_HIP_ERR_ZERO_LENGTH_VECTOR, "%s: zero length box vector", who);
    if (hf[1]) return fail(MOLAR_HIP_ERR_INVERSE_FAILED, "%s: box matrix inverse failed", who);

    hipLaunchKernelGGL(tcf_fold_kernel<Real>, dim3((uint32_t)vblocks), dim3(TCF_VECS), 0, c->stream, mom_d, bad_d, fchunks, V, F, labels_dev, valid_d, nvalid_d, mean_d,
                       s2_d, badf_d);
    if (want_lags) {
        LagQ Q{};
        Q.traj = traj_d;
        Q.valid = valid_d;
        Q.labels = labels_dev;
        Q.V = V;
        Q.F = F;
        Q.L = L;
        Q.os = std::min(origin_stride, F);          // beyond F - 1 there is the origin 0 alone either way
        Q.G = G;
        Q.chunk = Y.chunk;
        Q.nchunks = Y.nchunks;
        Q.part = want_groups ? part_d : nullptr;
        if (want_groups) MH_HIP(hipMemsetAsync(part_d, 0, (size_t)Y.nchunks * G * (L + 1) * 16, c->stream));
        const size_t ld1 = c1v_d != c1_vec ? L + 1 : ld, ld2 = c2v_d != c2_vec ? L + 1 : ld;      // a staged result is dense
        if (Y.nlb_main) {
            Q.l_base = 0;
            launch_lags<Real>(c->stream, Y.R, Q, Y.nlb_main, want_p2, c1v_d, ld1, c2v_d, ld2);
        }
        if (Y.tail_R) {             // the lags behind the whole blocks: one block of the narrowest lane that holds them
            Q.l_base = (size_t)Y.nlb_main * Y.lag_block;
            launch_lags<Real>(c->stream, Y.tail_R, Q, 1u, want_p2, c1v_d, ld1, c2v_d, ld2);
        }
        if (want_groups) {
            const size_t cells = G * (L + 1);
            hipLaunchKernelGGL(tcf_finish_kernel<Real>, dim3((uint32_t)((cells + 255) / 256)), dim3(256), 0, c->stream, Q, nvalid_d, c1_d, c2_d);
        }
    }
    MH_HIP(hipGetLastError());
    bool wait = false;
    MH_TRY(copy_out(c, c1, c1_d, G * (L + 1), wait));
    MH_TRY(copy_out(c, c2, c2_d, G * (L + 1), wait));
    MH_TRY(copy_out_2d(c, c1_vec, ld, c1v_d, L + 1, V, wait));
    MH_TRY(copy_out_2d(c, c2_vec, ld, c2v_d, L + 1, V, wait));
    MH_TRY(copy_out(c, mean, mean_d, V * 3, wait));
    MH_TRY(copy_out(c, s2, s2_d, V, wait));
    MH_TRY(copy_out(c, bad_frames, badf_d, V, wait));
    if (nvalid) {
        const bool dev = is_device_ptr(nvalid);
        MH_HIP(hipMemcpyAsync(nvalid, nvalid_d, G * 8, dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c->stream));
        if (!dev) wait = true;
    }
    return finish_copies(c, wait);
}

}  // namespace

namespace mh {
void tcf_release(molar_hip_ctx *c) {
    release_state(c->tcf);
}
}  // namespace mh

extern "C" {

int molar_hip_tcf_plan(size_t nframes, size_t nvectors, size_t ngroups, size_t max_lag, int per_frame_boxes, int want_lags, int want_groups,
                       size_t *workspace_bytes, uint32_t *frame_chunk, uint32_t *vec_chunk, uint32_t *lag_block, uint32_t *lags_per_lane, uint32_t *segment,
                       uint32_t *window) {
    const Layout Y = make_layout(nframes, nvectors, ngroups ? ngroups : 1, max_lag, per_frame_boxes != 0, want_lags != 0, want_groups != 0);
    const bool none = nframes == 0 || nvectors == 0;
    if (workspace_bytes) *workspace_bytes = none ? 0 : Y.bytes;
    if (frame_chunk) *frame_chunk = TCF_FRAMES;
    if (vec_chunk) *vec_chunk = none ? 1u : Y.chunk;
    if (lag_block) *lag_block = Y.lag_block;
    if (lags_per_lane) *lags_per_lane = Y.R;
    if (segment) *segment = TCF_SEG;
    if (window) *window = TCF_SEG + Y.lag_block;
    return MOLAR_HIP_OK;
}

int molar_hip_tcf(molar_hip_ctx *c, const float *frames, size_t nframes, size_t frame_stride, size_t natoms, const uint64_t *tuples, size_t nvectors,
                  const uint32_t *labels, size_t ngroups, const float *boxes, size_t box_stride, uint8_t pbc, const molar_hip_tcf_spec *spec, size_t max_lag,
                  size_t origin_stride, float *c1, float *c2, float *c1_vec, float *c2_vec, size_t ld, uint64_t *nvalid, float *mean, float *s2,
                  uint32_t *bad_frames) {
    return tcf_run<float>(c, "tcf", frames, nframes, frame_stride, natoms, tuples, nvectors, labels, ngroups, boxes, box_stride, pbc, spec, max_lag, origin_stride,
                          c1, c2, c1_vec, c2_vec, ld, nvalid, mean, s2, bad_frames);
}

int molar_hip_tcf_f64(molar_hip_ctx *c, const double *frames, size_t nframes, size_t frame_stride, size_t natoms, const uint64_t *tuples, size_t nvectors,
                      const uint32_t *labels, size_t ngroups, const double *boxes, size_t box_stride, uint8_t pbc, const molar_hip_tcf_spec *spec,
                      size_t max_lag, size_t origin_stride, double *c1, double *c2, double *c1_vec, double *c2_vec, size_t ld, uint64_t *nvalid, double *mean,
                      double *s2, uint32_t *bad_frames) {
    return tcf_run<double>(c, "tcf_f64", frames, nframes, frame_stride, natoms, tuples, nvectors, labels, ngroups, boxes, box_stride, pbc, spec, max_lag,
                           origin_stride, c1, c2, c1_vec, c2_vec, ld, nvalid, mean, s2, bad_frames);
}

}  // extern "C"
