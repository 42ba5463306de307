// fluct.hip - fluctuations of a block of trajectory frames about their mean structure: the mean, the per-atom RMSF and the
// 3n x 3n positional covariance, after an optional mass-weighted fit of every frame onto a reference (frame 0, a given
// structure, or - iterated - the mean itself).  The definition is in molar_hip.h.  With z'_f,k = R_f (x_f,k - c_f) (R_f = I and
// c_f = one common origin without a fit) and o the reference's centre (or that origin):
//
//   mean_k = o + m'_k,  m'_k = (1/F) sum_f z'_f,k,   rmsf_k^2 = (1/F) sum_f |z'_f,k - m'_k|^2,
//   cov = (1/F) D^T D,  D[f][3k+d] = z'_f,k,d - m'_k,d        (two passes: the deviations are taken about the finished mean)
//
// Stages, all on the context's stream:
//
//   centres (one workgroup per frame, fixed-order f64 sums)  ->  reference (its f64 copy, centre and sum w |y|^2)
//   ->  per pass:  fit sums (nine sums w x y^T and sum w |x|^2 per frame, atoms in chunks)  ->  rotations (one lane per
//       frame: the chunks in order, Horn's quaternion by Jacobi at f64 working precision, the fit_out record)
//       ->  sums of z' (one thread per atom and split of the frames)  ->  mean (the splits in order; the next reference)
//   ->  sums of |z' - m'|^2  ->  rmsf
//   ->  pack (z' - m' in f64, fragment-major)  ->  covariance (v_mfma_f64_16x16x4_f64, K = frames, a 64 x 64 block of
//       coordinates per wave, blocks on and above the diagonal)  ->  finish (only when the frames are split over workgroups)
//
// The packed operand is [tile of 16 coordinates][frame][16 coordinates] doubles, zero for the frames that pad F to a multiple
// of four and for the coordinates that pad 3n to a multiple of 64: the A or B fragment of a wave for four consecutive frames
// is 512 contiguous bytes, lane l reads double l of them, and the A and the B fragments of any tile pair both come out of
// this one operand.  No floating-point atomics: every sum has an order fixed by the launch geometry, which depends on the
// sizes alone.
#include <algorithm>
#include <cmath>

#include "common.hpp"
#include "linalg3.hpp"
#include "traj_block.hpp"

using namespace mh;

struct molar_hip_fluct_state {
    DevBuf in_frames, in_idx, in_mass, in_ref;        // host inputs staged here
    DevBuf ws;                                        // the workspace molar_hip_fluct_plan reports
    DevBuf out_mean, out_rmsf, out_cov, out_fit;      // results of a call whose destinations are host memory
};

namespace {

constexpr uint32_t FL_TILE = 16;                     // coordinates per tile: the M and N of the MFMA
constexpr uint32_t FL_KSTEP = 4;                     // frames per MFMA
constexpr uint32_t FL_BLOCK = 4;                     // tiles per side of a wave's register block (64 x 64 coordinates)
constexpr uint32_t FL_CHUNK = 4096;                  // atoms per workgroup of the fit sums
constexpr uint32_t FL_PACK_FRAMES = 256;             // frames per workgroup of the pack kernel
constexpr size_t FL_STAT_THREADS = 524288;           // threads the sums over the frames aim for (atoms x splits)
constexpr uint32_t FL_MIN_SPLIT_STEPS = 64;          // a split of the covariance's frames is at least this many MFMA steps
constexpr uint32_t FL_MAX_SPLITS = 64;
constexpr size_t FL_TARGET_WAVES = 4096;             // blocks x splits the covariance kernel aims for
constexpr size_t FL_PART_BLOCKS = 4096;              // blocks x splits the partial covariances may take (32 KiB each)
constexpr size_t FL_PART_DOUBLES = 16 * 4 * 64;      // one block's sixteen accumulators

// Where everything lives in the workspace, from the sizes alone (the plan entry and the call share it).
struct Layout {
    size_t F, n, M;               // frames, atoms, coordinates (3 n)
    size_t Fpad;                  // frames padded to FL_KSTEP
    uint32_t T, Tp, NB;           // tiles that hold coordinates, tiles of the operand (a multiple of FL_BLOCK), blocks per side
    size_t nupper;                // blocks on and above the diagonal
    uint32_t ksteps, ksplits, kper;
    uint32_t nchunks;             // workgroups per frame of the fit sums
    uint32_t nfs, fper;           // splits of the frames in the sums of z', frames per split
    size_t off_centre, off_refd, off_refc, off_origin, off_flags, off_fitpart, off_rot, off_mprime, off_spart, off_packed, off_part, bytes;
};

Layout make_layout(size_t F, size_t n, bool want_cov) {
    Layout L{};
    L.F = F;
    L.n = n;
    L.M = 3 * n;
    L.Fpad = (F + FL_KSTEP - 1) / FL_KSTEP * FL_KSTEP;
    L.T = (uint32_t)((L.M + FL_TILE - 1) / FL_TILE);
    L.Tp = (L.T + FL_BLOCK - 1) / FL_BLOCK * FL_BLOCK;
    L.NB = L.Tp / FL_BLOCK;
    L.nupper = (size_t)L.NB * (L.NB + 1) / 2;
    L.ksteps = (uint32_t)(L.Fpad / FL_KSTEP);
    L.nchunks = (uint32_t)((n + FL_CHUNK - 1) / FL_CHUNK);
    // splits of the frames in the sums of z': enough threads to fill the device, at least eight frames each
    const size_t nn = std::max<size_t>(n, 1);
    const size_t by_frames = std::max<size_t>(1, (F + 7) / 8);
    const size_t want = std::min((FL_STAT_THREADS + nn - 1) / nn, by_frames);
    L.fper = (uint32_t)((F + want - 1) / want);
    if (L.fper == 0) L.fper = 1;
    L.nfs = F ? (uint32_t)((F + L.fper - 1) / L.fper) : 1;             // no empty split
    // splits of the frames in the covariance: as many as the frames allow (ksK), as the partial covariances' budget allows
    // and as it takes to fill the device; the bounds and the reservation below grow with the sizes, so the workspace never
    // shrinks when an argument grows
    const size_t ksK = std::min<size_t>(FL_MAX_SPLITS, std::max<size_t>(1, L.ksteps / FL_MIN_SPLIT_STEPS));
    size_t ks = 1;
    if (want_cov && L.nupper) ks = std::min({ksK, FL_PART_BLOCKS / L.nupper, (FL_TARGET_WAVES + L.nupper - 1) / L.nupper});
    const Splits sp = even_splits(L.ksteps, ks);
    L.kper = sp.kper;
    L.ksplits = sp.ksplits;
    const size_t part_blocks = std::min(ksK * L.nupper, FL_PART_BLOCKS);
    Carve ws;
    ws.take(L.off_centre, F * 4 * 8);
    ws.take(L.off_refd, L.M * 8);
    ws.take(L.off_refc, 8 * 8);
    ws.take(L.off_origin, 4 * 8);
    ws.take(L.off_flags, 16);
    ws.take(L.off_fitpart, F * L.nchunks * 10 * 8);
    ws.take(L.off_rot, F * 9 * 8);
    ws.take(L.off_mprime, L.M * 8);
    ws.take(L.off_spart, std::min(by_frames * n, FL_STAT_THREADS + n) * 3 * 8);
    ws.take(L.off_packed, want_cov ? (size_t)L.Tp * FL_TILE * L.Fpad * 8 : 0);
    ws.take(L.off_part, want_cov && ksK > 1 ? part_blocks * FL_PART_DOUBLES * 8 : 0);
    L.bytes = ws.bytes;
    return L;
}

template <class Real>
struct In {
    const Real *frames;
    size_t stride, F, natoms;
    const uint64_t *idx;
    const Real *mass;
    uint32_t n;
    __device__ __forceinline__ const Real *frame(size_t f) const { return frames + f * stride; }
};

// How a frame is brought onto the reference: z' = R_f (x - c_f) with R_f = rot + 9 f (column-major) and c_f = c + cstride f;
// rot == nullptr: no rotation, and cstride == 0 with c the common origin.
struct Pose {
    const double *rot;
    const double *c;
    size_t cstride;
};

template <class Real>
__device__ __forceinline__ void zprime(const Real *__restrict__ p, uint64_t a, const double *__restrict__ R, const double *__restrict__ c, double *z) {
    const double x0 = (double)p[3 * a] - c[0], x1 = (double)p[3 * a + 1] - c[1], x2 = (double)p[3 * a + 2] - c[2];
    if (R) {
#pragma unroll
        for (int d = 0; d < 3; ++d) z[d] = (R[d] * x0 + R[3 + d] * x1) + R[6 + d] * x2;
    } else {
        z[0] = x0;
        z[1] = x1;
        z[2] = x2;
    }
}

// The first reference in f64: the caller's packed [n][3], or the selection of frame 0.
template <class Real>
__global__ void __launch_bounds__(256) fl_ref_init_kernel(In<Real> P, const Real *__restrict__ ref, double *__restrict__ refd) {
    const size_t k = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (k >= P.n) return;
    double v[3] = {0.0, 0.0, 0.0};
    if (ref) {
#pragma unroll
        for (int d = 0; d < 3; ++d) v[d] = (double)ref[3 * k + d];
    } else {
        const uint64_t a = sel_atom(P, k);
        if (a < P.natoms)
#pragma unroll
            for (int d = 0; d < 3; ++d) v[d] = (double)P.frames[3 * a + d];
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) refd[3 * k + d] = v[d];
}

// One workgroup: refc = {c_ref (3), W, sum w |y|^2} of the reference refd, y = refd - c_ref; the sums as in tb_centre_kernel.
template <class Real>
__global__ void __launch_bounds__(256) fl_ref_centre_kernel(In<Real> P, const double *__restrict__ refd, double *__restrict__ refc) {
    __shared__ double sh[4][256];
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (uint32_t k = threadIdx.x; k < P.n; k += 256u) {
        const uint64_t a = sel_atom(P, k);
        if (a >= P.natoms) continue;
        const double w = sel_weight(P, a);
        s[0] += w * refd[3 * k];
        s[1] += w * refd[3 * k + 1];
        s[2] += w * refd[3 * k + 2];
        s[3] += w;
    }
    tree256<4>(sh, s);
    const double W = sh[3][0];
    const double c[3] = {sh[0][0] / W, sh[1][0] / W, sh[2][0] / W};
    __syncthreads();
    double g[1] = {0.0};
    for (uint32_t k = threadIdx.x; k < P.n; k += 256u) {
        const uint64_t a = sel_atom(P, k);
        if (a >= P.natoms) continue;
        const double w = sel_weight(P, a);
        const double y0 = refd[3 * k] - c[0], y1 = refd[3 * k + 1] - c[1], y2 = refd[3 * k + 2] - c[2];
        g[0] += w * ((y0 * y0 + y1 * y1) + y2 * y2);
    }
    tree256<1>(sh, g);
    if (threadIdx.x == 0u) {
        refc[0] = c[0];
        refc[1] = c[1];
        refc[2] = c[2];
        refc[3] = W;
        refc[4] = sh[0][0];
    }
}

// Workgroup (frame, chunk of FL_CHUNK atoms): S[d][e] = sum w (x - c_f)_d y_e and sum w |x - c_f|^2 of the chunk; thread t
// adds atoms t, t + 256, ... of the chunk in that order, then the fixed tree.  part is [frame][chunk][10].
template <class Real>
__global__ void __launch_bounds__(256) fl_fit_sums_kernel(In<Real> P, const double *__restrict__ centre, const double *__restrict__ refd,
                                                          const double *__restrict__ refc, uint32_t nchunks, double *__restrict__ part) {
    __shared__ double sh[10][256];
    const size_t f = blockIdx.x;
    const Real *p = P.frames + f * P.stride;
    const double c[3] = {centre[f * 4], centre[f * 4 + 1], centre[f * 4 + 2]};
    const double cr[3] = {refc[0], refc[1], refc[2]};
    const uint32_t k0 = blockIdx.y * FL_CHUNK, k1 = min(k0 + FL_CHUNK, P.n);
    double s[10];
#pragma unroll
    for (int q = 0; q < 10; ++q) s[q] = 0.0;
    for (uint32_t k = k0 + threadIdx.x; k < k1; k += 256u) {
        const uint64_t a = P.idx ? P.idx[k] : (uint64_t)k;      // (sel_atom written out: through it two scalar registers change places)
        const double w = sel_weight(P, a);
        const double x[3] = {(double)p[3 * a] - c[0], (double)p[3 * a + 1] - c[1], (double)p[3 * a + 2] - c[2]};
        const double y[3] = {refd[3 * (size_t)k] - cr[0], refd[3 * (size_t)k + 1] - cr[1], refd[3 * (size_t)k + 2] - cr[2]};
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const double wx = w * x[d];
#pragma unroll
            for (int e = 0; e < 3; ++e) s[d * 3 + e] += wx * y[e];
        }
        s[9] += w * ((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]);
    }
    tree256<10>(sh, s);
    if (threadIdx.x < 10u) part[(f * nchunks + blockIdx.y) * 10 + threadIdx.x] = sh[threadIdx.x][0];
}

// One Newton step towards the nearest orthogonal matrix, R <- R + R (I - R^T R) / 2.  The quaternion formula leaves R^T R a
// few 2^-53 from the identity; that residual is formed in doubled precision (Dot2, linalg3.hpp) so that it means something,
// and the corrected entries carry one rounding each: R^T R = I to about 2 * 2^-53.  The correction itself is a few 2^-53, far
// inside what the eigenvector determines.  R is column-major.
__device__ __forceinline__ void orthogonal_step(double *R) {
    double E[9], N[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            double s = i == j ? -1.0 : 0.0, err = 0.0;
#pragma unroll
            for (int k = 0; k < 3; ++k) dot2_step(R[i * 3 + k], R[j * 3 + k], s, err);
            E[i * 3 + j] = -(s + err);                  // (I - R^T R)(i, j)
        }
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int r = 0; r < 3; ++r) N[j * 3 + r] = R[j * 3 + r] + 0.5 * ((R[r] * E[j] + R[3 + r] * E[3 + j]) + R[6 + r] * E[6 + j]);
#pragma unroll
    for (int q = 0; q < 9; ++q) R[q] = N[q];
}

// One lane per frame: the chunks in order, the rotation (rotation_from_cov at f64 working precision: with S as laid out
// here its argument is S itself, and sum w (R x) . y is the dot product of the two arrays), the record of fit_out.
// fit == 0: R = I, t = 0, and the distance as the frames stand, sum w |x - r|^2 = Gx + Gy - 2 tr S + W |c_f - c_ref|^2.
// A frame with a non-finite selected coordinate: every number of its record and of its rotation is NaN.
template <class Real>
__global__ void __launch_bounds__(64) fl_rotation_kernel(const double *__restrict__ part, uint32_t nchunks, size_t F, const double *__restrict__ centre,
                                                         const double *__restrict__ refc, int fit, double *__restrict__ rot,
                                                         Real *__restrict__ fit_out) {
    const size_t f = (size_t)blockIdx.x * 64u + threadIdx.x;
    if (f >= F) return;
    double S[9], gx = 0.0;
#pragma unroll
    for (int q = 0; q < 9; ++q) S[q] = 0.0;
    for (uint32_t ch = 0; ch < nchunks; ++ch) {
        const double *src = part + (f * nchunks + ch) * 10;
#pragma unroll
        for (int q = 0; q < 9; ++q) S[q] += src[q];
        gx += src[9];
    }
    const double c[3] = {centre[f * 4], centre[f * 4 + 1], centre[f * 4 + 2]};
    const double cr[3] = {refc[0], refc[1], refc[2]}, W = refc[3], gy = refc[4];
    double R[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, t[3] = {0.0, 0.0, 0.0}, d2;
    bool ok = true;
    if (fit) {
        ok = rotation_from_cov(S, R, /*precise=*/true);
        orthogonal_step(R);                            // R is still the identity when there was no rotation
        double dot = 0.0;
#pragma unroll
        for (int q = 0; q < 9; ++q) dot += R[q] * S[q];
        d2 = (gx + gy) - 2.0 * dot;
#pragma unroll
        for (int d = 0; d < 3; ++d) t[d] = cr[d] - ((R[d] * c[0] + R[3 + d] * c[1]) + R[6 + d] * c[2]);
    } else {
        const double e0 = c[0] - cr[0], e1 = c[1] - cr[1], e2 = c[2] - cr[2];
        d2 = ((gx + gy) - 2.0 * ((S[0] + S[4]) + S[8])) + W * ((e0 * e0 + e1 * e1) + e2 * e2);
    }
    double rmsd = sqrt(fmax(d2, 0.0) / W);
    if (!ok || d2 != d2) {                             // fmax drops a NaN
        const double nan = __builtin_nan("");
        rmsd = nan;
#pragma unroll
        for (int q = 0; q < 9; ++q) R[q] = nan;
#pragma unroll
        for (int d = 0; d < 3; ++d) t[d] = nan;
    }
    if (fit)
#pragma unroll
        for (int q = 0; q < 9; ++q) rot[f * 9 + q] = R[q];
    if (fit_out) {
#pragma unroll
        for (int q = 0; q < 9; ++q) fit_out[f * 13 + q] = (Real)R[q];
#pragma unroll
        for (int d = 0; d < 3; ++d) fit_out[f * 13 + 9 + d] = (Real)t[d];
        fit_out[f * 13 + 12] = (Real)rmsd;
    }
}

// Workgroup (block of 256 atoms, split of the frames), blockIdx.x = split * atom blocks + atom block: one thread per selected
// atom walks the frames of the split in order.  Second == false: sum z' (three values per atom); Second == true:
// sum |z' - m'|^2 (one value).  R_f and c_f are the same for the whole workgroup.  spart is [split][n][NV].
template <class Real, bool Second>
__global__ void __launch_bounds__(256) fl_sums_kernel(In<Real> P, Pose Z, uint32_t nab, uint32_t fper, const double *__restrict__ mprime,
                                                      double *__restrict__ spart) {
    const uint32_t ab = blockIdx.x % nab, split = blockIdx.x / nab;
    const size_t k = (size_t)ab * 256u + threadIdx.x;
    if (k >= P.n) return;
    const uint64_t a = sel_atom(P, k);
    const size_t f0 = (size_t)split * fper, f1 = f0 + fper < P.F ? f0 + fper : P.F;
    double m[3] = {0.0, 0.0, 0.0}, s[3] = {0.0, 0.0, 0.0};
    if (Second) {
        m[0] = mprime[3 * k];
        m[1] = mprime[3 * k + 1];
        m[2] = mprime[3 * k + 2];
    }
    for (size_t f = f0; f < f1; ++f) {
        double z[3];
        zprime(P.frames + f * P.stride, a, Z.rot ? Z.rot + f * 9 : nullptr, Z.c + f * Z.cstride, z);
        if (Second) {
            const double d0 = z[0] - m[0], d1 = z[1] - m[1], d2 = z[2] - m[2];
            s[0] += (d0 * d0 + d1 * d1) + d2 * d2;
        } else {
            s[0] += z[0];
            s[1] += z[1];
            s[2] += z[2];
        }
    }
    if (Second) {
        spart[(size_t)split * P.n + k] = s[0];
    } else {
        double *dst = spart + ((size_t)split * P.n + k) * 3;
        dst[0] = s[0];
        dst[1] = s[1];
        dst[2] = s[2];
    }
}

// One thread per coordinate: m' = (the splits in order) / F; mean = o + m' rounded to Real; next_ref = o + m' in f64.
template <class Real>
__global__ void __launch_bounds__(256) fl_mean_kernel(const double *__restrict__ spart, uint32_t nfs, size_t M, size_t F, const double *__restrict__ o,
                                                      double *__restrict__ mprime, Real *__restrict__ mean, double *__restrict__ next_ref) {
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= M) return;
    double sum = 0.0;
    for (uint32_t s = 0; s < nfs; ++s) sum += spart[(size_t)s * M + i];
    const double m = sum / (double)F;
    mprime[i] = m;
    const double abs_m = o[i % 3] + m;
    if (mean) mean[i] = (Real)abs_m;
    if (next_ref) next_ref[i] = abs_m;
}

// One thread per atom: rmsf = sqrt((the splits in order) / F).
template <class Real>
__global__ void __launch_bounds__(256) fl_rmsf_kernel(const double *__restrict__ spart, uint32_t nfs, size_t n, size_t F, Real *__restrict__ rmsf) {
    const size_t k = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (k >= n) return;
    double sum = 0.0;
    for (uint32_t s = 0; s < nfs; ++s) sum += spart[(size_t)s * n + k];
    rmsf[k] = (Real)sqrt(sum / (double)F);
}

// Workgroup (chunk of FL_PACK_FRAMES frames, tile): thread t holds coordinate t & 15 of the tile and frames (t >> 4) + 16 j of
// the chunk, so that 16 lanes store 128 contiguous bytes.  z' - m' in f64, formed as in fl_sums_kernel; exact zeros for the
// coordinates beyond 3 n and the frames beyond F.
template <class Real>
__global__ void __launch_bounds__(256) fl_pack_kernel(In<Real> P, Pose Z, size_t M, size_t Fpad, const double *__restrict__ mprime,
                                                      double *__restrict__ packed) {
    const uint32_t cl = threadIdx.x & 15u, fl = threadIdx.x >> 4;
    const uint32_t tile = blockIdx.y;
    const size_t i = (size_t)tile * FL_TILE + cl;
    const bool live = i < M;
    const size_t k = live ? i / 3 : 0;
    const uint32_t d = (uint32_t)(i - 3 * (i / 3));
    const uint64_t a = live ? sel_atom(P, k) : 0;
    const double m = live ? mprime[i] : 0.0;
    const size_t f0 = (size_t)blockIdx.x * FL_PACK_FRAMES, f1 = f0 + FL_PACK_FRAMES < Fpad ? f0 + FL_PACK_FRAMES : Fpad;
    double *dst = packed + (size_t)tile * Fpad * FL_TILE + cl;
    for (size_t f = f0 + fl; f < f1; f += 16u) {
        double v = 0.0;
        if (live && f < P.F) {
            double z[3];
            zprime(P.frames + f * P.stride, a, Z.rot ? Z.rot + f * 9 : nullptr, Z.c + f * Z.cstride, z);
            v = (d == 0u ? z[0] : d == 1u ? z[1] : z[2]) - m;
        }
        dst[f * FL_TILE] = v;
    }
}

struct CovP {
    const double *packed;
    uint32_t NB;
    size_t tile_stride;           // Fpad * 16 doubles
    uint32_t ksteps, kper;
    double *part;                 // [split][block on or above the diagonal][tile pair][4][64], or null: finish here
};

template <class Real>
struct CovOut {
    Real *cov;
    size_t ld, M;
    double F;
};

// block (bi, bj >= bi) from its index p among the blocks on and above the diagonal, row by row: row bi holds NB - bi of them
// (a scalar loop of at most NB steps, nothing beside the K loop)
__device__ __forceinline__ void upper_block(uint32_t p, uint32_t NB, uint32_t &bi, uint32_t &bj) {
    uint32_t row = 0;
    while (p >= NB - row) {
        p -= NB - row;
        ++row;
    }
    bi = row;
    bj = row + p;
}

// One entry and its mirror image: only entries on and above the diagonal are stored, each twice, so the result is exactly
// symmetric.
template <class Real>
__device__ __forceinline__ void fl_store(const CovOut<Real> &O, size_t row, size_t col, double sum) {
    if (row >= O.M || col >= O.M || col < row) return;
    const Real v = (Real)(sum / O.F);
    O.cov[row * O.ld + col] = v;
    O.cov[col * O.ld + row] = v;
}

// One wave per workgroup (x, y): the 64 x 64 block of coordinates number x among those on and above the diagonal, split y of the frames.
// Per step of four frames the wave loads four A and four B fragments (a block on the diagonal reuses A as B and leaves out
// the tile pairs below the diagonal) and issues 16 MFMAs into 16 accumulators.  By the C layout of the instruction lane l holds,
// in register r of tile pair (i, j), the entry (row 16 i + (l >> 4) + 4 r, column 16 j + (l & 15)) of the block.
// amdgpu_waves_per_eu(2): the register budget of two waves per SIMD makes the compiler keep the sixteen accumulators in VGPRs
// (about 150 in all, three waves per SIMD); without it they go to 128 AGPRs beside 158 VGPRs in the fused form, one wave per SIMD.
template <class Real, bool Fused>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2))) fl_cov_kernel(CovP Q, CovOut<Real> O) {
    uint32_t bi, bj;
    upper_block(blockIdx.x, Q.NB, bi, bj);
    const uint32_t lane = threadIdx.x;
    const uint32_t s0 = blockIdx.y * Q.kper, s1 = min(s0 + Q.kper, Q.ksteps);
    const size_t ts = Q.tile_stride;
    const double *pa = Q.packed + (size_t)bi * FL_BLOCK * ts + lane;
    const double *pb = Q.packed + (size_t)bj * FL_BLOCK * ts + lane;
    d4 acc[FL_BLOCK][FL_BLOCK];
#pragma unroll
    for (int i = 0; i < (int)FL_BLOCK; ++i)
#pragma unroll
        for (int j = 0; j < (int)FL_BLOCK; ++j) acc[i][j] = d4{0.0, 0.0, 0.0, 0.0};
    if (bi == bj) {
        for (uint32_t s = s0; s < s1; ++s) {
            const size_t o = (size_t)s * 64u;
            double a[FL_BLOCK];
#pragma unroll
            for (int i = 0; i < (int)FL_BLOCK; ++i) a[i] = pa[i * ts + o];
#pragma unroll
            for (int i = 0; i < (int)FL_BLOCK; ++i)
#pragma unroll
                for (int j = i; j < (int)FL_BLOCK; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], a[j], acc[i][j], 0, 0, 0);
        }
    } else {
        for (uint32_t s = s0; s < s1; ++s) {
            const size_t o = (size_t)s * 64u;
            double a[FL_BLOCK], b[FL_BLOCK];
#pragma unroll
            for (int i = 0; i < (int)FL_BLOCK; ++i) a[i] = pa[i * ts + o];
#pragma unroll
            for (int j = 0; j < (int)FL_BLOCK; ++j) b[j] = pb[j * ts + o];
#pragma unroll
            for (int i = 0; i < (int)FL_BLOCK; ++i)
#pragma unroll
                for (int j = 0; j < (int)FL_BLOCK; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], acc[i][j], 0, 0, 0);
        }
    }
    if constexpr (Fused) {
#pragma unroll
        for (int i = 0; i < (int)FL_BLOCK; ++i)
#pragma unroll
            for (int j = 0; j < (int)FL_BLOCK; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    fl_store<Real>(O, mfma_c_row(((size_t)bi * FL_BLOCK + i) * FL_TILE, lane, r), mfma_c_col(((size_t)bj * FL_BLOCK + j) * FL_TILE, lane), acc[i][j][r]);
    } else {
        const size_t nupper = (size_t)Q.NB * (Q.NB + 1u) / 2u;
        double *dst = Q.part + ((size_t)blockIdx.y * nupper + blockIdx.x) * FL_PART_DOUBLES + lane;
#pragma unroll
        for (int i = 0; i < (int)FL_BLOCK; ++i)
#pragma unroll
            for (int j = 0; j < (int)FL_BLOCK; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) dst[(size_t)(((i * 4 + j) * 4 + r) * 64)] = acc[i][j][r];
    }
}

// Frames split over workgroups: one workgroup per block on or above the diagonal, thread (r, lane) adds each of its sixteen entries over
// the splits in order, scales and stores as above.
template <class Real>
__global__ void __launch_bounds__(256) fl_cov_finish_kernel(const double *__restrict__ part, uint32_t ksplits, uint32_t NB, CovOut<Real> O) {
    uint32_t bi, bj;
    upper_block(blockIdx.x, NB, bi, bj);
    const uint32_t lane = threadIdx.x & 63u, r = threadIdx.x >> 6;
    const size_t nupper = (size_t)NB * (NB + 1u) / 2u;
    const double *src = part + (size_t)blockIdx.x * FL_PART_DOUBLES + lane;
    for (uint32_t ij = 0; ij < 16u; ++ij) {
        const uint32_t i = ij >> 2, j = ij & 3u;
        // (mfma_c_row / mfma_c_col written out: through them the compiler swaps the operands of two scalar ANDs below)
        const size_t row = ((size_t)bi * FL_BLOCK + i) * FL_TILE + (lane >> 4) + 4u * r, col = ((size_t)bj * FL_BLOCK + j) * FL_TILE + (lane & 15u);
        if (row >= O.M || col >= O.M || col < row) continue;
        double sum = 0.0;
        for (uint32_t z = 0; z < ksplits; ++z) sum += src[(size_t)z * nupper * FL_PART_DOUBLES + (size_t)((ij * 4u + r) * 64u)];
        fl_store<Real>(O, row, col, sum);
    }
}

template <class Real>
int fluct_run(molar_hip_ctx *c, const char *who, const Real *frames, size_t F, size_t stride, size_t natoms, const uint64_t *idx, size_t n,
              const Real *mass, const Real *ref, int fit, int iterations, Real *mean, Real *rmsf, Real *cov, size_t ld, Real *fit_out) {
    MH_CTX(c);
    if (n == 0) return fail(MOLAR_HIP_ERR_SIZES, "%s: empty selection", who);
    if (cov && ld < 3 * n) return fail(MOLAR_HIP_ERR_SIZES, "%s: ld = %zu is below the %zu columns of the covariance", who, ld, 3 * n);
    MH_TRY(check_no_index(who, "n", idx, n, natoms));
    MH_TRY(check_stride(who, "the frame stride", F, stride, natoms));
    if (iterations < 0) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: iterations = %d is negative", who, iterations);
    if (n >= 0x2AAAAAA0ull || F >= 0x7FFFFFF0ull) return fail(MOLAR_HIP_ERR_TOO_LARGE, "%s: more than 2^31 coordinates or frames", who);
    if (F == 0) return MOLAR_HIP_OK;
    if (!frames) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: the frames pointer is null", who);
    MH_TRY(check_index(who, "idx", idx, n, natoms));
    const Layout L = make_layout(F, n, cov != nullptr);
    if (cov && L.Tp > 65535u) return fail(MOLAR_HIP_ERR_TOO_LARGE, "%s: a covariance of more than %u coordinates", who, 65532u * FL_TILE);
    if (L.nchunks > 65535u) return fail(MOLAR_HIP_ERR_TOO_LARGE, "%s: a selection of more than %u atoms", who, 65535u * FL_CHUNK);
    molar_hip_fluct_state &Z = state_of(c->fluct);
    MH_TRY(grow_exact(Z.ws, L.bytes, who, "the workspace"));
    char *W = Z.ws.as<char>();
    auto at = [&](size_t off) { return reinterpret_cast<double *>(W + off); };
    double *centre = at(L.off_centre), *refd = at(L.off_refd), *refc = at(L.off_refc), *origin = at(L.off_origin);
    uint32_t *flags = reinterpret_cast<uint32_t *>(W + L.off_flags);
    double *fitpart = at(L.off_fitpart), *rot = at(L.off_rot), *mprime = at(L.off_mprime), *spart = at(L.off_spart);
    double *packed = at(L.off_packed), *part = at(L.off_part);

    In<Real> P{};
    const Real *ref_dev = nullptr;
    MH_TRY(to_device(c, frames, (F - 1) * stride + natoms * 3, Z.in_frames, &P.frames));
    MH_TRY(to_device(c, idx, idx ? n : 0, Z.in_idx, &P.idx));
    MH_TRY(to_device(c, mass, mass ? natoms : 0, Z.in_mass, &P.mass));
    MH_TRY(to_device(c, ref, ref ? 3 * n : 0, Z.in_ref, &ref_dev));
    P.stride = stride;
    P.F = F;
    P.natoms = natoms;
    P.n = (uint32_t)n;
    Real *mean_dev, *rmsf_dev, *cov_dev, *fit_dev;
    MH_TRY(out_buffer(mean, L.M, Z.out_mean, who, &mean_dev));
    MH_TRY(out_buffer(rmsf, n, Z.out_rmsf, who, &rmsf_dev));
    MH_TRY(out_buffer(cov, L.M * L.M, Z.out_cov, who, &cov_dev));
    MH_TRY(out_buffer(fit_out, F * 13, Z.out_fit, who, &fit_dev));

    const uint32_t nblk_n = (uint32_t)((n + 255) / 256), nblk_M = (uint32_t)((L.M + 255) / 256);
    MH_HIP(hipMemsetAsync(flags, 0, 16, c->stream));
    hipLaunchKernelGGL(tb_centre_kernel<In<Real>>, dim3((uint32_t)F), dim3(256), 0, c->stream, P, centre, flags);
    if (!fit) hipLaunchKernelGGL(tb_origin_kernel<>, dim3(1), dim3(1), 0, c->stream, centre, F, origin);
    hipLaunchKernelGGL(fl_ref_init_kernel<Real>, dim3(nblk_n), dim3(256), 0, c->stream, P, ref_dev, refd);
    // the weights' sum and the index check decide the status, read back before the rest is enqueued
    MH_TRY(check_selection(c, flags, centre + 3, who, natoms));

    const int passes = fit ? 1 + iterations : 1;
    const Pose pose{fit ? rot : nullptr, fit ? centre : origin, fit ? (size_t)4 : (size_t)0};
    const double *o = fit ? refc : origin;
    const dim3 sums_grid(nblk_n * L.nfs);
    for (int pass = 0; pass < passes; ++pass) {
        const bool last = pass + 1 == passes;
        if (fit || (fit_dev && last)) {
            hipLaunchKernelGGL(fl_ref_centre_kernel<Real>, dim3(1), dim3(256), 0, c->stream, P, refd, refc);
            hipLaunchKernelGGL(fl_fit_sums_kernel<Real>, dim3((uint32_t)F, L.nchunks), dim3(256), 0, c->stream, P, centre, refd, refc, L.nchunks, fitpart);
            hipLaunchKernelGGL(fl_rotation_kernel<Real>, dim3((uint32_t)((F + 63) / 64)), dim3(64), 0, c->stream, fitpart, L.nchunks, F, centre, refc,
                               fit ? 1 : 0, rot, last ? fit_dev : (Real *)nullptr);
        }
        if (!last || mean_dev || rmsf_dev || cov_dev) {
            hipLaunchKernelGGL((fl_sums_kernel<Real, false>), sums_grid, dim3(256), 0, c->stream, P, pose, nblk_n, L.fper, mprime, spart);
            hipLaunchKernelGGL(fl_mean_kernel<Real>, dim3(nblk_M), dim3(256), 0, c->stream, spart, L.nfs, L.M, F, o, mprime, last ? mean_dev : (Real *)nullptr,
                               last ? (double *)nullptr : refd);
        }
    }
    if (rmsf_dev) {
        hipLaunchKernelGGL((fl_sums_kernel<Real, true>), sums_grid, dim3(256), 0, c->stream, P, pose, nblk_n, L.fper, mprime, spart);
        hipLaunchKernelGGL(fl_rmsf_kernel<Real>, dim3(nblk_n), dim3(256), 0, c->stream, spart, L.nfs, n, F, rmsf_dev);
    }
    const bool cov_host = cov && cov_dev != cov;
    if (cov_dev) {
        hipLaunchKernelGGL(fl_pack_kernel<Real>, dim3((uint32_t)((L.Fpad + FL_PACK_FRAMES - 1) / FL_PACK_FRAMES), L.Tp), dim3(256), 0, c->stream, P, pose, L.M,
                           L.Fpad, mprime, packed);
        CovP Q{};
        Q.packed = packed;
        Q.NB = L.NB;
        Q.tile_stride = L.Fpad * FL_TILE;
        Q.ksteps = L.ksteps;
        Q.kper = L.kper;
        CovOut<Real> O{};
        O.cov = cov_dev;
        O.ld = cov_host ? L.M : ld;
        O.M = L.M;
        O.F = (double)F;
        const dim3 grid((uint32_t)L.nupper, L.ksplits);
        if (L.ksplits == 1) {
            Q.part = nullptr;
            hipLaunchKernelGGL((fl_cov_kernel<Real, true>), grid, dim3(64), 0, c->stream, Q, O);
        } else {
            Q.part = part;
            hipLaunchKernelGGL((fl_cov_kernel<Real, false>), grid, dim3(64), 0, c->stream, Q, O);
            hipLaunchKernelGGL(fl_cov_finish_kernel<Real>, dim3((uint32_t)L.nupper), dim3(256), 0, c->stream, part, L.ksplits, L.NB, O);
        }
    }
    MH_HIP(hipGetLastError());
    bool wait = false;
    MH_TRY(copy_out(c, mean, mean_dev, L.M, wait));
    MH_TRY(copy_out(c, rmsf, rmsf_dev, n, wait));
    MH_TRY(copy_out(c, fit_out, fit_dev, F * 13, wait));
    MH_TRY(copy_out_2d(c, cov, ld, cov_dev, L.M, L.M, wait));
    return finish_copies(c, wait);
}

}  // namespace

namespace mh {
void fluct_release(molar_hip_ctx *c) {
    release_state(c->fluct);
}
}  // namespace mh

extern "C" {

int molar_hip_fluct_plan(size_t nframes, size_t n, int want_cov, size_t *workspace_bytes, uint32_t *ksplits) {
    const Layout L = make_layout(nframes, n, want_cov != 0);
    const bool none = nframes == 0 || n == 0;
    if (workspace_bytes) *workspace_bytes = none ? 0 : L.bytes;
    if (ksplits) *ksplits = none ? 1u : L.ksplits;
    return MOLAR_HIP_OK;
}

int molar_hip_fluct(molar_hip_ctx *c, const float *frames, size_t nframes, size_t frame_stride, size_t natoms, const uint64_t *idx, size_t n,
                    const float *mass, const float *ref, int fit, int iterations, float *mean, float *rmsf, float *cov, size_t ld, float *fit_out) {
    return fluct_run<float>(c, "fluct", frames, nframes, frame_stride, natoms, idx, n, mass, ref, fit, iterations, mean, rmsf, cov, ld, fit_out);
}

int molar_hip_fluct_f64(molar_hip_ctx *c, const double *frames, size_t nframes, size_t frame_stride, size_t natoms, const uint64_t *idx, size_t n,
                        const double *mass, const double *ref, int fit, int iterations, double *mean, double *rmsf, double *cov, size_t ld,
                        double *fit_out) {
    return fluct_run<double>(c, "fluct_f64", frames, nframes, frame_stride, natoms, idx, n, mass, ref, fit, iterations, mean, rmsf, cov, ld, fit_out);
}

}  // extern "C"
