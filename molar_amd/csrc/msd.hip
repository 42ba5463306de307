// msd.hip - mean-squared displacement of a block of trajectory frames: the no-jump unwrap of every selected atom along time,
// the displacement of each particle (an atom, or the centre of mass of a group of atoms), the optional removal of the drift of
// a reference set, and the all-time-origins reduction over the lags.  The definition is in molar_hip.h.
//
//   u_k(0) = 0,  u_k(f) = u_k(f-1) + shortest_vector(box_f, x_k(f) - x_k(f-1), pbc)          (boxmath.hpp in double)
//   U_g(f) = sum_k w_k u_k(f) / W_g  -  D(f),   D(f) = the same over the reference set
//   msd[tau] = sum_g sum_t |U_g(t + tau) - U_g(t)|^2 / (P count[tau]),  t = 0, origin_stride, ... while t + tau <= F - 1
//
// Stages, all on the context's stream:
//
//   boxes (one thread per box: the f64 PeriodicBox of box9)
//   ->  unwrap of the reference set (as one group)  ->  its pieces in order: D [F][3]
//   ->  unwrap of the selection: one thread per selected atom walks the frames with its u in registers; per frame the atoms of a
//       workgroup meet in LDS and the first atom of each particle adds its particle's atoms in index order; writes the
//       particle-major f64 trajectories U [P][F][3] and disp.  A group of more than 256 atoms is cut into pieces of 256 (one
//       workgroup each, a fixed tree per frame); a second kernel adds the pieces in order.
//   ->  16 bytes read back: the status (an index not below natoms, a box that is none, a weight sum of zero)
//   ->  lags: a workgroup owns a chunk of particles and a block of 256 lags, one lane per lag (below)
//   ->  finish: the chunks in order, the scaling.
//
// No floating-point atomics: every sum has an order fixed by the launch geometry, which depends on the sizes alone.
#include <algorithm>
#include <cmath>
#include <vector>

#include "boxmath.hpp"
#include "common.hpp"
#include "traj_block.hpp"

using namespace mh;

struct molar_hip_msd_state {
    DevBuf in_frames, in_idx, in_mass, in_boxes, in_off, in_ref, tab;   // host inputs and the host-made tables staged here
    DevBuf ws;                                                           // the workspace molar_hip_msd_plan reports
    DevBuf out_msd, out_m4, out_mp, out_disp;                            // results of a call whose destinations are host memory
};

namespace {

constexpr uint32_t MSD_ATOMS = 256;          // selected atoms per workgroup of the unwrap kernel
constexpr uint32_t MSD_LAGS = 256;           // lags per workgroup of the lag kernel: one lane each
constexpr uint32_t MSD_SEG = 512;            // frames of origins per staged segment
constexpr uint32_t MSD_WIN = MSD_SEG + MSD_LAGS;   // frames of U(t + tau) a segment reaches
constexpr size_t MSD_TARGET_WGS = 2048;      // workgroups the lag kernel aims for
constexpr uint32_t MSD_MAX_CHUNK = 64;       // particles per workgroup at the most

// A workgroup of the unwrap kernel: selected atoms [a0, a0 + count), the particle of its first atom, and, for a piece of a
// group of more than MSD_ATOMS atoms, the slot of its sums (-1: the workgroup holds whole particles).
struct Block {
    uint32_t a0, count, g0;
    int32_t piece;
};
// A group of more than MSD_ATOMS atoms: its particle and its pieces [piece0, piece0 + npieces).
struct Big {
    uint32_t g, piece0, npieces;
};

// pieces of all large groups of n atoms together, at the most: a group of len > MSD_ATOMS atoms has ceil(len / MSD_ATOMS) < 2 len / MSD_ATOMS
inline size_t pieces_bound(size_t n) { return 2 * n / MSD_ATOMS + 1; }

// Where everything lives in the workspace, from the sizes alone (the plan entry and the call share it).
struct Layout {
    size_t F, n, P, nref, L;
    uint32_t nlb, chunk, nchunks;     // lag blocks, particles per workgroup, chunks of particles
    size_t off_flags, off_boxes, off_drift, off_piece, off_piecew, off_traj, off_part, bytes;
};

Layout make_layout(size_t F, size_t n, size_t P, size_t nref, size_t L, bool per_frame_boxes, bool want_lags) {
    Layout Y{};
    Y.F = F;
    Y.n = n;
    Y.P = P;
    Y.nref = nref;
    Y.L = L;
    Y.nlb = (uint32_t)((L + 1 + MSD_LAGS - 1) / MSD_LAGS);
    const size_t per = P * Y.nlb / MSD_TARGET_WGS;
    Y.chunk = (uint32_t)std::max<size_t>(1, std::min<size_t>(MSD_MAX_CHUNK, per));
    Y.nchunks = (uint32_t)((P + Y.chunk - 1) / Y.chunk);
    // the chunks never exceed this, which grows with P: the reservation never shrinks when an argument grows
    const size_t chunks_bound = std::min<size_t>(P, 2 * MSD_TARGET_WGS) + P / MSD_MAX_CHUNK + 1;
    Carve ws;
    ws.take(Y.off_flags, 16);
    ws.take(Y.off_boxes, (per_frame_boxes ? F : 1) * sizeof(BoxD));
    ws.take(Y.off_drift, nref ? F * 3 * 8 : 0);
    // the pieces by their bound, not by the count the offsets give: the plan entry sees sizes only, and what it reports must
    // neither differ from what the call takes nor shrink when an argument grows
    ws.take(Y.off_piece, pieces_bound(std::max(n, nref)) * F * 3 * 8);
    ws.take(Y.off_piecew, pieces_bound(std::max(n, nref)) * 8);
    ws.take(Y.off_traj, want_lags ? P * F * 3 * 8 : 0);
    ws.take(Y.off_part, want_lags ? chunks_bound * (L + 1) * 2 * 8 : 0);
    Y.bytes = ws.bytes;
    return Y;
}

// PeriodicBox::from_matrix in double on the device (box_from_matrix of boxmath.hpp, operation by operation, its two errors
// included); 0: a box, 1: a box vector of zero length, 2: a matrix without an inverse.
__device__ int build_box(const double *m9, BoxD *out) {
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

// One thread per box.  flags[1]: a box matrix without an inverse; flags[3]: a box vector of zero length.
template <class Real>
__global__ void __launch_bounds__(64) msd_box_kernel(const Real *__restrict__ boxes, size_t nbox, BoxD *__restrict__ out, uint32_t *__restrict__ flags) {
    const size_t f = (size_t)blockIdx.x * 64u + threadIdx.x;
    if (f >= nbox) return;
    double m9[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) m9[q] = (double)boxes[f * 9 + q];
    const int bad = build_box(m9, out + f);
    if (bad == 1) flags[3] = 1u;
    if (bad == 2) flags[1] = 1u;
}

template <class Real>
struct Set {
    const Real *frames;
    size_t stride, F, natoms;
    const uint64_t *idx;          // the set's atoms; null: 0 .. n-1
    const Real *mass;
    const uint64_t *off;          // CSR of its particles over the set's order; null: every atom is one
    const Block *blocks;
    const BoxD *boxes;            // null: no image is removed
    size_t box_step;              // 0: one box, 1: one per frame
    uint32_t pbc;
    const double *drift;          // [F][3] subtracted from every particle; null: none
    double *traj;                 // [P][F][3], or null
    Real *disp;                   // [F][P][3], or null
    size_t P;
    double *piece, *piecew;       // [pieces][F][3] and [pieces]: sums of w u and of w of the pieces of large groups
};

static_assert(MSD_ATOMS == 256, "the pieces of a large group are summed by tree256_sum");

// One workgroup per entry of S.blocks, one thread per atom of it.  flags[0]: an index not below natoms; flags[2]: a particle
// whose weights add up to zero.
template <class Real>
__global__ void __launch_bounds__(MSD_ATOMS) msd_unwrap_kernel(Set<Real> S, uint32_t *__restrict__ flags) {
    __shared__ double sh[3][MSD_ATOMS];
    const Block B = S.blocks[blockIdx.x];
    const uint32_t t = threadIdx.x;
    const bool live = t < B.count;
    const size_t k = (size_t)B.a0 + (live ? t : 0u);
    uint64_t a = sel_atom(S, k);
    if (a >= S.natoms) {
        flags[0] = 1u;
        a = 0;
    }
    const double w = live ? sel_weight(S, a) : 0.0;
    // the particle of this atom and, for the first atom of a particle within the workgroup, how many atoms follow
    size_t g = B.g0;
    uint32_t cnt = 0;
    bool whole = false;
    if (B.piece < 0 && live) {
        if (S.off) {
            size_t lo = B.g0, hi = B.g0 + B.count < S.P ? B.g0 + B.count : S.P;   // off[lo] <= k < off[hi]: no particle is empty
            while (hi - lo > 1) {
                const size_t mid = (lo + hi) / 2;
                if (S.off[mid] <= k) lo = mid;
                else hi = mid;
            }
            g = lo;
            if (S.off[g] == k) cnt = (uint32_t)(S.off[g + 1] - k);
        } else {
            g = k;
            cnt = 1;
        }
        whole = cnt != 0;
    }
    // the weights' sums: of each whole particle by its first atom, of a piece by the tree
    double W = 0.0;
    sh[0][t] = w;
    sh[1][t] = 0.0;
    sh[2][t] = 0.0;
    __syncthreads();
    if (B.piece >= 0) {
        tree256_sum<3>(sh);
        if (t == 0u) S.piecew[B.piece] = sh[0][0];
    } else if (whole) {
        for (uint32_t j = 0; j < cnt; ++j) W += sh[0][t + j];
        if (W == 0.0) flags[2] = 1u;
    }
    __syncthreads();

    const Real *p = S.frames + 3 * a;
    double px = (double)p[0], py = (double)p[1], pz = (double)p[2];
    double u[3] = {0.0, 0.0, 0.0};
    for (size_t f = 0; f < S.F; ++f) {
        if (f > 0) {
            const Real *q = p + f * S.stride;
            const double x = (double)q[0], y = (double)q[1], z = (double)q[2];
            D3 d{x - px, y - py, z - pz};
            if (S.boxes) d = shortest_vector(S.boxes[f * S.box_step], d, S.pbc);
            u[0] += d.x;
            u[1] += d.y;
            u[2] += d.z;
            px = x;
            py = y;
            pz = z;
        }
        sh[0][t] = w * u[0];
        sh[1][t] = w * u[1];
        sh[2][t] = w * u[2];
        __syncthreads();
        if (B.piece >= 0) {
            tree256_sum<3>(sh);
            if (t < 3u) S.piece[((size_t)B.piece * S.F + f) * 3 + t] = sh[t][0];
        } else if (whole) {
            double s[3] = {sh[0][t], sh[1][t], sh[2][t]};
            for (uint32_t j = 1; j < cnt; ++j) {
                s[0] += sh[0][t + j];
                s[1] += sh[1][t + j];
                s[2] += sh[2][t + j];
            }
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                double v = s[d] / W;
                if (S.drift) v -= S.drift[f * 3 + d];
                if (S.traj) S.traj[(g * S.F + f) * 3 + d] = v;
                if (S.disp) S.disp[(f * S.P + g) * 3 + d] = (Real)v;
            }
        }
        __syncthreads();
    }
}

// Large groups: one thread per frame and group adds the pieces in order.  flags[2] as above.
template <class Real>
__global__ void __launch_bounds__(256) msd_pieces_kernel(Set<Real> S, const Big *__restrict__ big, uint32_t *__restrict__ flags) {
    const size_t f = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (f >= S.F) return;
    const Big G = big[blockIdx.y];
    double W = 0.0, s[3] = {0.0, 0.0, 0.0};
    for (uint32_t q = 0; q < G.npieces; ++q) {
        const size_t pc = (size_t)G.piece0 + q;
        W += S.piecew[pc];
#pragma unroll
        for (int d = 0; d < 3; ++d) s[d] += S.piece[(pc * S.F + f) * 3 + d];
    }
    if (W == 0.0) flags[2] = 1u;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        double v = s[d] / W;
        if (S.drift) v -= S.drift[f * 3 + d];
        if (S.traj) S.traj[((size_t)G.g * S.F + f) * 3 + d] = v;
        if (S.disp) S.disp[(f * S.P + G.g) * 3 + d] = (Real)v;
    }
}

struct LagP {
    const double *traj;           // [P][F][3]
    size_t P, F, L, os;           // particles, frames, largest lag, origin stride
    uint32_t chunk, nchunks;
    double *part;                 // [chunk][L + 1][2]: sums of r^2 and r^4 over the chunk's particles
};

// Workgroup (chunk of particles, block of MSD_LAGS lags), blockIdx.x = lag block * chunks + chunk, so that the blocks of short lags -
// the long ones - start first.  Lane l holds lag tau = block * MSD_LAGS + l.  Per particle the frames of origins go by in
// segments of MSD_SEG: the window U(t0 + l0 .. t0 + l0 + MSD_WIN) is staged in LDS, one array per component, so that the lanes
// read consecutive doubles; U(t) is the same for the whole workgroup and comes straight from memory (scalar loads).  A lane
// adds its own r^2 and r^4 over the origins in order, then into its totals over the particles in order.
template <class Real, uint32_t DIMS>
__global__ void __launch_bounds__(MSD_LAGS) msd_lag_kernel(LagP Q, Real *__restrict__ msd_particle, size_t ld) {
    __shared__ double sh[3][MSD_WIN];
    const uint32_t lb = blockIdx.x / Q.nchunks, ch = blockIdx.x - lb * Q.nchunks;
    const size_t l0 = (size_t)lb * MSD_LAGS, tau = l0 + threadIdx.x;
    const bool mine = tau <= Q.L;
    const size_t g0 = (size_t)ch * Q.chunk, g1 = g0 + Q.chunk < Q.P ? g0 + Q.chunk : Q.P;
    const size_t tend = Q.F - l0;                                       // origins t < tend reach lag l0 (l0 <= L < F)
    const double count = mine ? (double)((Q.F - 1 - tau) / Q.os + 1) : 1.0;
    double tot2 = 0.0, tot4 = 0.0;
    for (size_t g = g0; g < g1; ++g) {
        const double *__restrict__ U = Q.traj + g * Q.F * 3;
        double s2 = 0.0, s4 = 0.0;
        for (size_t t0 = 0; t0 < tend; t0 += MSD_SEG) {
            const size_t t1 = t0 + MSD_SEG < tend ? t0 + MSD_SEG : tend;
            size_t t = (t0 + Q.os - 1) / Q.os * Q.os;                   // the first origin of the segment
            if (t >= t1) continue;
            const size_t w0 = t0 + l0, wn = Q.F - w0 < MSD_WIN ? Q.F - w0 : MSD_WIN;
            __syncthreads();
            for (size_t i = threadIdx.x; i < wn; i += MSD_LAGS) {
#pragma unroll
                for (int d = 0; d < 3; ++d)
                    if (DIMS >> d & 1u) sh[d][i] = U[(w0 + i) * 3 + d];
            }
            __syncthreads();
            // the origins every lane of the block reaches (t + l0 + MSD_LAGS - 1 < F), four at a time and without the predicate;
            // the same chain per lane as the loop below, which takes the rest
            const size_t tfull = Q.F - l0 >= MSD_LAGS ? Q.F - l0 - (MSD_LAGS - 1) : 0, t1f = t1 < tfull ? t1 : tfull;
            for (; t + 3 * Q.os < t1f; t += 4 * Q.os) {
                double r2[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const size_t tk = t + k * Q.os, i = tk - t0 + threadIdx.x;
                    r2[k] = 0.0;
#pragma unroll
                    for (int d = 0; d < 3; ++d)
                        if (DIMS >> d & 1u) {
                            const double e = sh[d][i] - U[tk * 3 + d];
                            r2[k] = fma(e, e, r2[k]);
                        }
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    s2 += r2[k];
                    s4 = fma(r2[k], r2[k], s4);
                }
            }
            for (; t < t1; t += Q.os) {
                const size_t i = t - t0 + threadIdx.x;                  // t + tau - w0
                if (t + tau < Q.F) {
                    double r2 = 0.0;
#pragma unroll
                    for (int d = 0; d < 3; ++d)
                        if (DIMS >> d & 1u) {
                            const double e = sh[d][i] - U[t * 3 + d];
                            r2 = fma(e, e, r2);
                        }
                    s2 += r2;
                    s4 = fma(r2, r2, s4);
                }
            }
        }
        if (msd_particle && mine) msd_particle[g * ld + tau] = (Real)(s2 / count);
        tot2 += s2;
        tot4 += s4;
    }
    if (mine) {
        double *dst = Q.part + ((size_t)ch * (Q.L + 1) + tau) * 2;
        dst[0] = tot2;
        dst[1] = tot4;
    }
}

// One thread per lag: the chunks in order, then the scaling by P count[tau].
template <class Real>
__global__ void __launch_bounds__(256) msd_finish_kernel(LagP Q, Real *__restrict__ msd, Real *__restrict__ m4) {
    const size_t tau = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (tau > Q.L) return;
    double a = 0.0, b = 0.0;
    for (uint32_t ch = 0; ch < Q.nchunks; ++ch) {
        const double *src = Q.part + ((size_t)ch * (Q.L + 1) + tau) * 2;
        a += src[0];
        b += src[1];
    }
    const double scale = (double)Q.P * (double)((Q.F - 1 - tau) / Q.os + 1);
    if (msd) msd[tau] = (Real)(a / scale);
    if (m4) m4[tau] = (Real)(b / scale);
}

// The workgroups of the unwrap kernel for n atoms in particles off[0..P] (null: every atom is one): whole particles packed into
// workgroups of at most MSD_ATOMS atoms in order; a group of more than MSD_ATOMS atoms in pieces of MSD_ATOMS.
void make_blocks(const uint64_t *off, size_t n, size_t P, std::vector<Block> &blocks, std::vector<Big> &big) {
    blocks.clear();
    big.clear();
    if (!off) {
        for (size_t a = 0; a < n; a += MSD_ATOMS) blocks.push_back(Block{(uint32_t)a, (uint32_t)std::min<size_t>(MSD_ATOMS, n - a), (uint32_t)a, -1});
        return;
    }
    uint32_t npieces = 0;
    size_t g = 0;
    while (g < P) {
        const size_t len = off[g + 1] - off[g];
        if (len > MSD_ATOMS) {
            const uint32_t first = npieces;
            for (size_t a = off[g]; a < off[g + 1]; a += MSD_ATOMS)
                blocks.push_back(Block{(uint32_t)a, (uint32_t)std::min<size_t>(MSD_ATOMS, off[g + 1] - a), (uint32_t)g, (int32_t)npieces++});
            big.push_back(Big{(uint32_t)g, first, npieces - first});
            ++g;
            continue;
        }
        size_t h = g;
        while (h < P && off[h + 1] - off[h] <= MSD_ATOMS && off[h + 1] - off[g] <= MSD_ATOMS) ++h;
        blocks.push_back(Block{(uint32_t)off[g], (uint32_t)(off[h] - off[g]), (uint32_t)g, -1});
        g = h;
    }
}

template <class Real, uint32_t DIMS>
void launch_lags(hipStream_t st, const LagP &Q, uint32_t nlb, Real *mp, size_t ld) {
    hipLaunchKernelGGL((msd_lag_kernel<Real, DIMS>), dim3(nlb * Q.nchunks), dim3(MSD_LAGS), 0, st, Q, mp, ld);
}

template <class Real>
int msd_run(molar_hip_ctx *c, const char *who, const Real *frames, size_t F, size_t stride, size_t natoms, const uint64_t *idx, size_t n,
            const Real *mass, const Real *boxes, size_t box_stride, uint8_t pbc, const uint64_t *group_offsets, size_t nparticles,
            const uint64_t *ref_idx, size_t nref, size_t max_lag, size_t origin_stride, uint32_t msd_dims, Real *msd, Real *m4, Real *msd_particle,
            size_t ld, Real *disp) {
    // the arguments are judged before the context is used
    if (!c) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "null context");
    const size_t P = group_offsets ? nparticles : n, L = max_lag;
    if (n == 0) return fail(MOLAR_HIP_ERR_SIZES, "%s: empty selection", who);
    if (group_offsets && P == 0) return fail(MOLAR_HIP_ERR_SIZES, "%s: no particles", who);
    if (msd_particle && ld < L + 1) return fail(MOLAR_HIP_ERR_SIZES, "%s: ld = %zu is below the %zu lags of a row", who, ld, L + 1);
    // the offsets are needed here: they decide the launch geometry
    std::vector<uint64_t> off_host;
    const uint64_t *off = group_offsets;
    if (group_offsets && is_device_ptr(group_offsets)) {
        MH_HIP(hipSetDevice(c->device));
        off_host.resize(P + 1);
        MH_HIP(hipMemcpy(off_host.data(), group_offsets, (P + 1) * 8, hipMemcpyDeviceToHost));
        off = off_host.data();
    }
    if (off) {
        if (off[0] != 0 || off[P] != n) return fail(MOLAR_HIP_ERR_SIZES, "%s: the group offsets run from %llu to %llu, not from 0 to n = %zu", who, (unsigned long long)off[0], (unsigned long long)off[P], n);
        for (size_t g = 0; g < P; ++g) {
            if (off[g + 1] < off[g]) return fail(MOLAR_HIP_ERR_SIZES, "%s: the group offsets decrease at group %zu", who, g);
            if (off[g + 1] == off[g]) return fail(MOLAR_HIP_ERR_SIZES, "%s: group %zu is empty", who, g);
        }
    }
    if (F >= 1 && L >= F) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: max_lag = %zu is not below nframes = %zu", who, L, F);
    if (origin_stride == 0) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: origin_stride is zero", who);
    if (msd_dims == 0 || msd_dims > 7) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: msd_dims = %u is not one of 1 .. 7", who, msd_dims);
    if (pbc > 7) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: pbc = %u is not a PbcDims byte", who, (unsigned)pbc);
    if (box_stride != 0 && box_stride != 9) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: box_stride = %zu is neither 0 nor 9", who, box_stride);
    if (natoms == 0) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: a selection of %zu atoms out of natoms = 0", who, n);
    MH_TRY(check_no_index(who, "n", idx, n, natoms));
    MH_TRY(check_no_index(who, "nref", ref_idx, nref, natoms));
    MH_TRY(check_stride(who, "the frame stride", F, stride, natoms));
    if (pbc != 0 && !boxes) return fail(MOLAR_HIP_ERR_NO_PBC, "%s: pbc operation without periodic box", who);
    if (n >= 0x7FFFFF00ull || nref >= 0x7FFFFF00ull || F >= 0x7FFFFFF0ull) return fail(MOLAR_HIP_ERR_TOO_LARGE, "%s: more than 2^31 atoms or frames", who);
    if (F == 0) return MOLAR_HIP_OK;
    if (!frames) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: the frames pointer is null", who);
    MH_TRY(check_index(who, "idx", idx, n, natoms));
    MH_TRY(check_index(who, "ref_idx", ref_idx, nref, natoms));
    MH_HIP(hipSetDevice(c->device));
    const bool use_box = boxes != nullptr && pbc != 0;
    const bool want_lags = msd || m4 || msd_particle;
    const Layout Y = make_layout(F, n, P, nref, L, use_box && box_stride == 9, want_lags);
    molar_hip_msd_state &Z = state_of(c->msd);
    MH_TRY(grow_exact(Z.ws, Y.bytes, who, "the workspace"));
    char *W = Z.ws.as<char>();
    auto at = [&](size_t o) { return reinterpret_cast<double *>(W + o); };
    uint32_t *flags = reinterpret_cast<uint32_t *>(W + Y.off_flags);
    BoxD *boxd = reinterpret_cast<BoxD *>(W + Y.off_boxes);

    // the tables of both unwrap launches in one staged block: [blocks of the reference set | its large group | blocks | large groups]
    std::vector<Block> rblocks, sblocks;
    std::vector<Big> rbig, sbig;
    if (nref) {                 // the reference set is one group, always in pieces: its sums go through msd_pieces_kernel
        for (size_t a = 0; a < nref; a += MSD_ATOMS) rblocks.push_back(Block{(uint32_t)a, (uint32_t)std::min<size_t>(MSD_ATOMS, nref - a), 0u, (int32_t)rblocks.size()});
        rbig.push_back(Big{0u, 0u, (uint32_t)rblocks.size()});
    }
    make_blocks(off, n, P, sblocks, sbig);
    if (sbig.size() > 65535u) return fail(MOLAR_HIP_ERR_TOO_LARGE, "%s: more than 65535 groups of more than %u atoms", who, MSD_ATOMS);
    // built in the context's pinned memory behind the 16 bytes of the status read-back, so that no return below leaves the copy
    // reading memory that is gone
    const size_t tab_bytes = (rblocks.size() + sblocks.size()) * sizeof(Block) + (rbig.size() + sbig.size()) * sizeof(Big);
    MH_TRY(ensure_pinned(c, 16 + tab_bytes));
    char *tab = static_cast<char *>(c->h_pinned) + 16;
    size_t o_rb = 0, o_sb = o_rb + rblocks.size() * sizeof(Block), o_rg = o_sb + sblocks.size() * sizeof(Block), o_sg = o_rg + rbig.size() * sizeof(Big);
    if (!rblocks.empty()) memcpy(tab + o_rb, rblocks.data(), rblocks.size() * sizeof(Block));
    memcpy(tab + o_sb, sblocks.data(), sblocks.size() * sizeof(Block));
    if (!rbig.empty()) memcpy(tab + o_rg, rbig.data(), rbig.size() * sizeof(Big));
    if (!sbig.empty()) memcpy(tab + o_sg, sbig.data(), sbig.size() * sizeof(Big));
    MH_TRY(Z.tab.reserve(tab_bytes));
    MH_HIP(hipMemcpyAsync(Z.tab.p, tab, tab_bytes, hipMemcpyHostToDevice, c->stream));
    const char *T = Z.tab.as<char>();

    Set<Real> S{};
    const Real *boxes_dev = nullptr;
    const uint64_t *ref_dev = nullptr;
    MH_TRY(to_device(c, frames, (F - 1) * stride + natoms * 3, Z.in_frames, &S.frames));
    MH_TRY(to_device(c, idx, idx ? n : 0, Z.in_idx, &S.idx));
    MH_TRY(to_device(c, mass, mass ? natoms : 0, Z.in_mass, &S.mass));
    MH_TRY(to_device(c, use_box ? boxes : nullptr, box_stride ? F * 9 : 9, Z.in_boxes, &boxes_dev));
    MH_TRY(to_device(c, group_offsets, group_offsets ? P + 1 : 0, Z.in_off, &S.off));
    MH_TRY(to_device(c, ref_idx, ref_idx ? nref : 0, Z.in_ref, &ref_dev));
    S.stride = stride;
    S.F = F;
    S.natoms = natoms;
    S.boxes = use_box ? boxd : nullptr;
    S.box_step = box_stride ? 1 : 0;
    S.pbc = pbc;
    S.piece = at(Y.off_piece);
    S.piecew = at(Y.off_piecew);
    Real *msd_dev, *m4_dev, *mp_dev, *disp_dev;
    MH_TRY(out_buffer(msd, L + 1, Z.out_msd, who, &msd_dev));
    MH_TRY(out_buffer(m4, L + 1, Z.out_m4, who, &m4_dev));
    MH_TRY(out_buffer(msd_particle, P * (L + 1), Z.out_mp, who, &mp_dev));
    MH_TRY(out_buffer(disp, F * P * 3, Z.out_disp, who, &disp_dev));
    const bool mp_host = msd_particle && mp_dev != msd_particle;

    MH_HIP(hipMemsetAsync(flags, 0, 16, c->stream));
    if (use_box) {
        const size_t nbox = box_stride ? F : 1;
        hipLaunchKernelGGL(msd_box_kernel<Real>, dim3((uint32_t)((nbox + 63) / 64)), dim3(64), 0, c->stream, boxes_dev, nbox, boxd, flags);
    }
    const uint32_t fblocks = (uint32_t)((F + 255) / 256);
    if (nref) {
        Set<Real> R = S;
        R.idx = ref_dev;
        R.off = nullptr;
        R.blocks = reinterpret_cast<const Block *>(T + o_rb);
        R.drift = nullptr;
        R.traj = at(Y.off_drift);
        R.disp = nullptr;
        R.P = 1;
        hipLaunchKernelGGL(msd_unwrap_kernel<Real>, dim3((uint32_t)rblocks.size()), dim3(MSD_ATOMS), 0, c->stream, R, flags);
        hipLaunchKernelGGL(msd_pieces_kernel<Real>, dim3(fblocks, 1), dim3(256), 0, c->stream, R, reinterpret_cast<const Big *>(T + o_rg), flags);
        S.drift = R.traj;
    }
    S.blocks = reinterpret_cast<const Block *>(T + o_sb);
    S.traj = want_lags ? at(Y.off_traj) : nullptr;
    S.disp = disp_dev;
    S.P = P;
    if (S.traj || S.disp) {
        hipLaunchKernelGGL(msd_unwrap_kernel<Real>, dim3((uint32_t)sblocks.size()), dim3(MSD_ATOMS), 0, c->stream, S, flags);
        if (!sbig.empty())
            hipLaunchKernelGGL(msd_pieces_kernel<Real>, dim3(fblocks, (uint32_t)sbig.size()), dim3(256), 0, c->stream, S, reinterpret_cast<const Big *>(T + o_sg), flags);
    }
    // the index check, the boxes and the weights' sums decide the status: 16 bytes read back before the lags are enqueued.  The
    // tables behind byte 16 of the pinned buffer may still be in flight as the source of their copy: the read-back touches bytes
    // 0 - 15 alone, and a buffer that holds the tables is not moved for 16 bytes
    uint32_t hf[4];
    MH_TRY(read_back(c, hf, flags, sizeof hf));
    if (hf[0]) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: a selection index is not below natoms = %zu", who, natoms);
    if (hf[3]) return fail(MOLAR_HIP_ERR_ZERO_LENGTH_VECTOR, "%s: zero length box vector", who);
    if (hf[1]) return fail(MOLAR_HIP_ERR_INVERSE_FAILED, "%s: box matrix inverse failed", who);
    if (hf[2]) return fail(MOLAR_HIP_ERR_ZERO_MASS, "%s: the masses of a particle or of the reference set add up to zero", who);

    if (want_lags) {
        LagP Q{};
        Q.traj = S.traj;
        Q.P = P;
        Q.F = F;
        Q.L = L;
        Q.os = std::min(origin_stride, F);          // beyond F - 1 there is the origin 0 alone either way
        Q.chunk = Y.chunk;
        Q.nchunks = Y.nchunks;
        Q.part = at(Y.off_part);
        const size_t mld = mp_host ? L + 1 : ld;
        switch (msd_dims) {
            case 1: launch_lags<Real, 1>(c->stream, Q, Y.nlb, mp_dev, mld); break;
            case 2: launch_lags<Real, 2>(c->stream, Q, Y.nlb, mp_dev, mld); break;
            case 3: launch_lags<Real, 3>(c->stream, Q, Y.nlb, mp_dev, mld); break;
            case 4: launch_lags<Real, 4>(c->stream, Q, Y.nlb, mp_dev, mld); break;
            case 5: launch_lags<Real, 5>(c->stream, Q, Y.nlb, mp_dev, mld); break;
            case 6: launch_lags<Real, 6>(c->stream, Q, Y.nlb, mp_dev, mld); break;
            default: launch_lags<Real, 7>(c->stream, Q, Y.nlb, mp_dev, mld); break;
        }
        if (msd_dev || m4_dev) hipLaunchKernelGGL(msd_finish_kernel<Real>, dim3((uint32_t)((L + 256) / 256)), dim3(256), 0, c->stream, Q, msd_dev, m4_dev);
    }
    MH_HIP(hipGetLastError());
    bool wait = false;
    MH_TRY(copy_out(c, msd, msd_dev, L + 1, wait));
    MH_TRY(copy_out(c, m4, m4_dev, L + 1, wait));
    MH_TRY(copy_out_2d(c, msd_particle, ld, mp_dev, L + 1, P, wait));
    MH_TRY(copy_out(c, disp, disp_dev, F * P * 3, wait));
    return finish_copies(c, wait);
}

}  // namespace

namespace mh {
void msd_release(molar_hip_ctx *c) {
    release_state(c->msd);
}
}  // namespace mh

extern "C" {

int molar_hip_msd_plan(size_t nframes, size_t n, size_t nparticles, size_t nref, size_t max_lag, int per_frame_boxes, int want_lags,
                       size_t *workspace_bytes, uint32_t *particle_chunk, uint32_t *lag_block) {
    const Layout Y = make_layout(nframes, n, nparticles, nref, max_lag, per_frame_boxes != 0, want_lags != 0);
    const bool none = nframes == 0 || n == 0 || nparticles == 0;
    if (workspace_bytes) *workspace_bytes = none ? 0 : Y.bytes;
    if (particle_chunk) *particle_chunk = none ? 1u : Y.chunk;
    if (lag_block) *lag_block = MSD_LAGS;
    return MOLAR_HIP_OK;
}

int molar_hip_msd(molar_hip_ctx *c, const float *frames, size_t nframes, size_t frame_stride, size_t natoms, const uint64_t *idx, size_t n,
                  const float *mass, const float *boxes, size_t box_stride, uint8_t pbc, const uint64_t *group_offsets, size_t nparticles,
                  const uint64_t *ref_idx, size_t nref, size_t max_lag, size_t origin_stride, uint32_t msd_dims, float *msd, float *m4,
                  float *msd_particle, size_t ld, float *disp) {
    return msd_run<float>(c, "msd", frames, nframes, frame_stride, natoms, idx, n, mass, boxes, box_stride, pbc, group_offsets, nparticles, ref_idx, nref,
                          max_lag, origin_stride, msd_dims, msd, m4, msd_particle, ld, disp);
}

int molar_hip_msd_f64(molar_hip_ctx *c, const double *frames, size_t nframes, size_t frame_stride, size_t natoms, const uint64_t *idx, size_t n,
                      const double *mass, const double *boxes, size_t box_stride, uint8_t pbc, const uint64_t *group_offsets, size_t nparticles,
                      const uint64_t *ref_idx, size_t nref, size_t max_lag, size_t origin_stride, uint32_t msd_dims, double *msd, double *m4,
                      double *msd_particle, size_t ld, double *disp) {
    return msd_run<double>(c, "msd_f64", frames, nframes, frame_stride, natoms, idx, n, mass, boxes, box_stride, pbc, group_offsets, nparticles, ref_idx,
                           nref, max_lag, origin_stride, msd_dims, msd, m4, msd_particle, ld, disp);
}

}  // extern "C"
