// rmsd_matrix.hip - all-pairs minimum RMSD over the frames of a block (or of two blocks) as one Gram product on the f64
// matrix cores.  With x the coordinates of a frame about its weighted centre and q = sqrt(w) x,
//
//   C_ab = sum_k q_a,k q_b,k^T (3x3),  G_a = sum_k |q_a,k|^2,  rmsd_ab = sqrt(max(0, G_a + G_b - 2 lambda_max(K(C_ab))) / sum w)
//
// (K: Horn's 4x4 matrix, linalg3.hpp; without the fit tr C_ab stands in for lambda_max and every frame is taken about one
// common origin).  Three stages, all on the context's stream:
//
//   centres (one workgroup per frame, fixed-order f64 sums)  ->  pack (q in f64, fragment-major, + partial G)  ->  G
//   ->  gram (v_mfma_f64_16x16x4_f64: nine accumulators per 16 x 16 tile of frame pairs, finish fused when K is not split)
//   ->  finish (only when K is split over workgroups: partial covariances summed in the order of the splits)
//
// The packed operand of a block is [dimension][tile of 16 frames][atom k][16 frames] doubles, zero for the frames that pad
// the last tile (the tiles are padded to an even count) and for the atoms that pad n to a multiple of four: the A or B
// fragment of a wave for four consecutive atoms is 512 contiguous bytes, lane l reads double l of them.  No floating-point
// atomics: every sum has an order fixed by the launch geometry, which depends on the sizes alone.
#include <algorithm>
#include <cmath>

#include "common.hpp"
#include "linalg3.hpp"
#include "traj_block.hpp"

using namespace mh;

struct molar_hip_rmsd_matrix_state {
    DevBuf in_frames1, in_frames2, in_idx, in_mass;   // host inputs staged here
    DevBuf ws;                                       // the workspace molar_hip_rmsd_matrix_plan reports
    DevBuf out;                                      // dense result of a call whose destination is host memory
};

namespace {

constexpr uint32_t RM_TILE = 16;                     // frames per tile: the M and N of the MFMA
constexpr uint32_t RM_KSTEP = 4;                     // atoms per MFMA
constexpr uint32_t RM_ROWS = 4, RM_COLS = 2;         // tiles per workgroup: one row tile per wave, two column tiles per wave
constexpr uint32_t RM_CHUNK = 1024;                  // atoms per workgroup of the pack kernel
constexpr uint32_t RM_MIN_SPLIT_STEPS = 64;          // a K split is at least this many MFMA steps (256 atoms)
constexpr uint32_t RM_MAX_SPLITS = 256;
constexpr size_t RM_PART_TILES = 8192;               // tile pairs x splits the partial covariances may take (18 KiB each)
constexpr size_t RM_PART_BYTES = 36 * 64 * 8;        // one tile pair's nine accumulators

// Where everything lives in the workspace, from the sizes alone (the plan entry and the call share it).
struct Layout {
    size_t F1, F2;                // frames; F2 == 0: symmetric
    uint32_t T1, T2;              // tiles that hold frames
    uint32_t T1p, T2p;            // tiles of the packed operands (even)
    size_t Kpad;                  // atoms, padded to RM_KSTEP
    uint32_t ksteps, ksplits, kper;
    uint32_t nchunks;             // pack workgroups per frame tile
    size_t Ftot;                  // F1 + F2
    size_t off_packed1, off_packed2, off_centre, off_gpart, off_g, off_origin, off_flags, off_part, bytes;
};

Layout make_layout(size_t F1, size_t F2, size_t n) {
    Layout L{};
    const bool sym = F2 == 0;
    L.F1 = F1;
    L.F2 = F2;
    L.Ftot = F1 + F2;
    L.T1 = (uint32_t)((F1 + RM_TILE - 1) / RM_TILE);
    L.T2 = sym ? L.T1 : (uint32_t)((F2 + RM_TILE - 1) / RM_TILE);
    L.T1p = (L.T1 + 1u) & ~1u;
    L.T2p = (L.T2 + 1u) & ~1u;
    L.Kpad = (n + RM_KSTEP - 1) / RM_KSTEP * RM_KSTEP;
    L.ksteps = (uint32_t)(L.Kpad / RM_KSTEP);
    L.nchunks = (uint32_t)((L.Kpad + RM_CHUNK - 1) / RM_CHUNK);
    // K splits: as many as the atoms allow (ksK) and as the partial covariances' budget allows; both bounds and the
    // reservation below grow with the sizes, so the workspace never shrinks when an argument grows
    const size_t npairs = (size_t)L.T1 * L.T2p;
    const size_t ksK = std::min<size_t>(RM_MAX_SPLITS, std::max<size_t>(1, L.ksteps / RM_MIN_SPLIT_STEPS));
    const size_t ks = npairs ? std::min(ksK, RM_PART_TILES / std::max<size_t>(npairs, 1)) : 1;
    const Splits sp = even_splits(L.ksteps, ks);
    L.kper = sp.kper;
    L.ksplits = sp.ksplits;
    const size_t part_tiles = std::min(ksK * npairs, RM_PART_TILES);
    Carve ws;
    ws.take(L.off_packed1, (size_t)3 * L.T1p * RM_TILE * L.Kpad * 8);
    ws.take(L.off_packed2, sym ? 0 : (size_t)3 * L.T2p * RM_TILE * L.Kpad * 8);
    const size_t Fpad = ((size_t)L.T1p + (sym ? 0 : L.T2p)) * RM_TILE;
    ws.take(L.off_centre, L.Ftot * 4 * 8);
    ws.take(L.off_gpart, (size_t)L.nchunks * Fpad * 8);
    ws.take(L.off_g, Fpad * 8);
    ws.take(L.off_origin, 4 * 8);
    ws.take(L.off_flags, 16);
    ws.take(L.off_part, ksK > 1 ? part_tiles * RM_PART_BYTES : 0);
    L.bytes = ws.bytes;
    return L;
}

template <class Real>
struct PackIn {
    const Real *frames1, *frames2;
    size_t stride1, stride2, F1, F2;      // F2 == 0: one block
    size_t natoms;
    const uint64_t *idx;
    const Real *mass;
    uint32_t n;
    // frame f of both blocks, the second behind the first
    __device__ __forceinline__ const Real *frame(size_t f) const { return f < F1 ? frames1 + f * stride1 : frames2 + (f - F1) * stride2; }
};

// Workgroup (chunk, tile) of one block: thread t holds frame t & 15 of the tile and atoms (t >> 4) + 16 i of the chunk, so
// that 16 lanes store 128 contiguous bytes.  q = sqrt(w) (p - c) in f64 from the exact inputs; the squares of the chunk go
// to gpart[chunk][frame], added over the thread's atoms in order and then over the 16 threads of the frame in order.
template <class Real>
__global__ void __launch_bounds__(256) rm_pack_kernel(PackIn<Real> P, int block2, uint32_t Tp, size_t Kpad, const double *__restrict__ centre,
                                                      const double *__restrict__ origin, double *__restrict__ packed,
                                                      double *__restrict__ gpart, size_t gstride, size_t gbase) {
    __shared__ double sh[16][17];
    const uint32_t fl = threadIdx.x & 15u, kk = threadIdx.x >> 4;
    const uint32_t tile = blockIdx.y;
    const size_t F = block2 ? P.F2 : P.F1;
    const size_t fb = (size_t)tile * RM_TILE + fl;            // frame within its block
    const bool live = fb < F;
    const size_t f = block2 ? P.F1 + fb : fb;                 // frame among both blocks
    const Real *p = live ? P.frame(f) : nullptr;
    double c[3] = {0.0, 0.0, 0.0};
    if (live) {
        const double *src = origin ? origin : centre + f * 4;
        c[0] = src[0];
        c[1] = src[1];
        c[2] = src[2];
    }
    const size_t k0 = (size_t)blockIdx.x * RM_CHUNK, k1 = k0 + RM_CHUNK < Kpad ? k0 + RM_CHUNK : Kpad;
    const size_t plane = (size_t)Tp * Kpad * RM_TILE;         // one dimension of the operand
    double *dst = packed + ((size_t)tile * Kpad) * RM_TILE + fl;
    double g = 0.0;
    for (size_t k = k0 + kk; k < k1; k += 16u) {
        double q[3] = {0.0, 0.0, 0.0};
        if (live && k < P.n) {
            const uint64_t a = sel_atom(P, k);
            if (a < P.natoms) {
                const double sw = sqrt(P.mass ? (double)P.mass[a] : 1.0);      // (sel_weight written out: through it the kernel's scalar loads are grouped otherwise)
#pragma unroll
                for (int d = 0; d < 3; ++d) q[d] = sw * ((double)p[3 * a + d] - c[d]);
            }
        }
#pragma unroll
        for (int d = 0; d < 3; ++d) dst[d * plane + k * RM_TILE] = q[d];
        g += (q[0] * q[0] + q[1] * q[1]) + q[2] * q[2];
    }
    sh[kk][fl] = g;
    __syncthreads();
    if (kk == 0u) {
        double sum = 0.0;
#pragma unroll
        for (int i = 0; i < 16; ++i) sum += sh[i][fl];
        gpart[(size_t)blockIdx.x * gstride + gbase + (size_t)tile * RM_TILE + fl] = sum;
    }
}

// G of every (padded) frame: the chunks in order.  A frame with a non-finite selected coordinate gets NaN, which the
// finish hands on to its row and column without an eigen solve.
__global__ void __launch_bounds__(256) rm_g_kernel(const double *__restrict__ gpart, uint32_t nchunks, size_t Fpad, double *__restrict__ G) {
    const size_t f = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (f >= Fpad) return;
    double sum = 0.0;
    for (uint32_t c = 0; c < nchunks; ++c) sum += gpart[(size_t)c * Fpad + f];
    G[f] = isfinite(sum) ? sum : __builtin_nan("");
}

template <class Real>
struct FinishP {
    const double *G1, *G2;        // per frame of block 1 / of the column block (== G1 in the symmetric form)
    const double *sumw;           // centre[3] of frame 0
    Real *out;
    size_t ld, F1, F2;            // F2: columns
    int sym, fit;
};

// One entry from the nine sums S[d][e] = sum_k q_a,k,d q_b,k,e.
template <class Real>
__device__ __forceinline__ void rm_finish_pair(const FinishP<Real> &P, size_t a, size_t b, const double *S) {
    if (a >= P.F1 || b >= P.F2) return;
    if (P.sym && b < a) return;                       // the mirror image of (b, a), written with it
    const double gsum = P.G1[a] + P.G2[b];
    const bool bad = gsum != gsum;                    // a frame with a non-finite coordinate: NaN without an eigen solve
    double v = 0.0;                                   // the diagonal of the symmetric form is exact
    if (!bad && !(P.sym && a == b)) {
        double lam;
        if (P.fit) {
            double K[16];
            horn_matrix(S, K);
            lam = horn_lambda_max(K);
        } else {
            lam = (S[0] + S[4]) + S[8];
        }
        const double d2 = gsum - 2.0 * lam;
        const double r = sqrt(fmax(d2, 0.0) / P.sumw[0]);
        v = d2 != d2 ? d2 : r;                        // fmax drops a NaN
    }
    v = bad ? gsum : v;
    P.out[a * P.ld + b] = (Real)v;
    if (P.sym && a != b) P.out[b * P.ld + a] = (Real)v;
}

struct GramP {
    const double *A, *B;          // packed operands of the rows' and the columns' block
    uint32_t T1, T2, T1p, T2p;
    size_t Kpad;
    uint32_t ksteps, kper;
    int sym;
    double *part;                 // [split][row tile][column tile of T2p][9][4][64], or null: finish here
};

// Workgroup (x, y, z): column tiles 2x, 2x + 1, row tiles 4y + wave, K split z.  Per step of four atoms a wave loads three A
// and six B fragments (the four waves read the same B lines) and issues 18 MFMAs.  By the C layout of the instruction lane l
// then holds, in register r of the nine accumulators of a tile pair, the whole S of frames (row (l >> 4) + 4 r, column
// l & 15): the finish needs no shuffle.  No barrier in here: a wave without work leaves.
template <class Real, bool Fused>
__global__ void __launch_bounds__(64 * RM_ROWS) rm_gram_kernel(GramP Q, FinishP<Real> P) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t ta = blockIdx.y * RM_ROWS + wave, tb0 = blockIdx.x * RM_COLS;
    if (ta >= Q.T1) return;
    if (Q.sym && tb0 + 1u < ta) return;               // both column tiles lie below the diagonal
    const uint32_t s0 = blockIdx.z * Q.kper, s1 = min(s0 + Q.kper, Q.ksteps);
    const size_t planeA = (size_t)Q.T1p * Q.Kpad * RM_TILE, planeB = (size_t)Q.T2p * Q.Kpad * RM_TILE;
    const double *pa = Q.A + (size_t)ta * Q.Kpad * RM_TILE + lane;
    const double *pb = Q.B + (size_t)tb0 * Q.Kpad * RM_TILE + lane;
    const size_t tileB = Q.Kpad * RM_TILE;
    d4 acc[RM_COLS][3][3];
#pragma unroll
    for (int j = 0; j < (int)RM_COLS; ++j)
#pragma unroll
        for (int d = 0; d < 3; ++d)
#pragma unroll
            for (int e = 0; e < 3; ++e) acc[j][d][e] = d4{0.0, 0.0, 0.0, 0.0};
    for (uint32_t s = s0; s < s1; ++s) {
        const size_t o = (size_t)s * 64u;
        double a[3], b[RM_COLS][3];
#pragma unroll
        for (int d = 0; d < 3; ++d) a[d] = pa[d * planeA + o];
#pragma unroll
        for (int j = 0; j < (int)RM_COLS; ++j)
#pragma unroll
            for (int e = 0; e < 3; ++e) b[j][e] = pb[e * planeB + j * tileB + o];
#pragma unroll
        for (int j = 0; j < (int)RM_COLS; ++j)
#pragma unroll
            for (int d = 0; d < 3; ++d)
#pragma unroll
                for (int e = 0; e < 3; ++e) acc[j][d][e] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[d], b[j][e], acc[j][d][e], 0, 0, 0);
    }
    if constexpr (Fused) {
        // one copy of the eigen solve: the eight (column tile, register) entries of the lane are picked by selects
#pragma unroll 1
        for (uint32_t jr = 0; jr < 4u * RM_COLS; ++jr) {
            double S[9];
#pragma unroll
            for (int d = 0; d < 3; ++d)
#pragma unroll
                for (int e = 0; e < 3; ++e) {
                    double v = 0.0;
#pragma unroll
                    for (int j = 0; j < (int)RM_COLS; ++j)
#pragma unroll
                        for (int r = 0; r < 4; ++r) v = jr == (uint32_t)(j * 4 + r) ? acc[j][d][e][r] : v;
                    S[d * 3 + e] = v;
                }
            rm_finish_pair<Real>(P, mfma_c_row((size_t)ta * RM_TILE, lane, jr & 3u), mfma_c_col((size_t)(tb0 + (jr >> 2)) * RM_TILE, lane), S);
        }
    } else {
        const size_t npairs = (size_t)Q.T1 * Q.T2p;
#pragma unroll
        for (int j = 0; j < (int)RM_COLS; ++j) {
            double *dst = Q.part + (((size_t)blockIdx.z * npairs + (size_t)ta * Q.T2p + tb0 + (uint32_t)j) * 36u) * 64u + lane;
#pragma unroll
            for (int d = 0; d < 3; ++d)
#pragma unroll
                for (int e = 0; e < 3; ++e)
#pragma unroll
                    for (int r = 0; r < 4; ++r) dst[(size_t)(((d * 3 + e) * 4 + r) * 64)] = acc[j][d][e][r];
        }
    }
}

// K split over workgroups: thread (tile pair, r, lane) adds its nine sums over the splits in order and finishes as above.
// A tile pair the gram kernel left out (below the diagonal of the symmetric form) holds no entry that is written, and is
// not read.
template <class Real>
__global__ void __launch_bounds__(256) rm_finish_kernel(const double *__restrict__ part, uint32_t ksplits, uint32_t T1, uint32_t T2p, FinishP<Real> P) {
    const size_t pair = blockIdx.x;
    const uint32_t ta = (uint32_t)(pair / T2p), tb = (uint32_t)(pair % T2p);
    const uint32_t lane = threadIdx.x & 63u, r = threadIdx.x >> 6;
    const size_t a = mfma_c_row((size_t)ta * RM_TILE, lane, r), b = mfma_c_col((size_t)tb * RM_TILE, lane);
    if (a >= P.F1 || b >= P.F2 || (P.sym && b < a)) return;
    const size_t npairs = (size_t)T1 * T2p;
    double S[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) S[q] = 0.0;
    for (uint32_t z = 0; z < ksplits; ++z) {
        const double *src = part + (((size_t)z * npairs + pair) * 36u) * 64u + lane;
#pragma unroll
        for (int q = 0; q < 9; ++q) S[q] += src[(size_t)((q * 4 + (int)r) * 64)];
    }
    rm_finish_pair<Real>(P, a, b, S);
}

template <class Real>
int rmsd_matrix_run(molar_hip_ctx *c, const char *who, const Real *frames1, size_t nframes1, size_t stride1, const Real *frames2, size_t nframes2,
                    size_t stride2, size_t natoms, const uint64_t *idx, size_t n, const Real *mass, int fit, Real *out, size_t ld) {
    MH_CTX(c);
    const bool sym = frames2 == nullptr;
    const size_t F1 = nframes1, F2 = sym ? 0 : nframes2, cols = sym ? nframes1 : nframes2;
    if (n == 0) return fail(MOLAR_HIP_ERR_SIZES, "%s: empty selection", who);
    if (ld < cols) return fail(MOLAR_HIP_ERR_SIZES, "%s: ld = %zu is below the %zu columns of the result", who, ld, cols);
    MH_TRY(check_no_index(who, "n", idx, n, natoms));
    MH_TRY(check_stride(who, "a frame stride", F1, stride1, natoms));
    MH_TRY(check_stride(who, "a frame stride", F2, stride2, natoms));
    if (n >= 0x7FFFFFFCull || F1 >= 0x7FFFFFF0ull || F2 >= 0x7FFFFFF0ull) return fail(MOLAR_HIP_ERR_TOO_LARGE, "%s: more than 2^31 atoms or frames", who);
    if (F1 == 0 || cols == 0) return MOLAR_HIP_OK;
    if (!frames1 || !out) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: frames or output pointer is null", who);
    MH_TRY(check_index(who, "idx", idx, n, natoms));
    const Layout L = make_layout(F1, F2, n);
    if (L.T1p > 65535u || L.T2p > 65535u) return fail(MOLAR_HIP_ERR_TOO_LARGE, "%s: a block of more than %u frames", who, 65534u * RM_TILE);
    molar_hip_rmsd_matrix_state &Z = state_of(c->rmsdm);
    MH_TRY(grow_exact(Z.ws, L.bytes, who, "the workspace"));
    char *W = Z.ws.as<char>();
    double *packed1 = reinterpret_cast<double *>(W + L.off_packed1);
    double *packed2 = sym ? packed1 : reinterpret_cast<double *>(W + L.off_packed2);
    double *centre = reinterpret_cast<double *>(W + L.off_centre);
    double *gpart = reinterpret_cast<double *>(W + L.off_gpart);
    double *G = reinterpret_cast<double *>(W + L.off_g);
    double *origin = reinterpret_cast<double *>(W + L.off_origin);
    uint32_t *flags = reinterpret_cast<uint32_t *>(W + L.off_flags);
    double *part = reinterpret_cast<double *>(W + L.off_part);

    PackIn<Real> P{};
    MH_TRY(to_device(c, frames1, (F1 - 1) * stride1 + natoms * 3, Z.in_frames1, &P.frames1));
    if (!sym) MH_TRY(to_device(c, frames2, (F2 - 1) * stride2 + natoms * 3, Z.in_frames2, &P.frames2));
    MH_TRY(to_device(c, idx, idx ? n : 0, Z.in_idx, &P.idx));
    MH_TRY(to_device(c, mass, mass ? natoms : 0, Z.in_mass, &P.mass));
    P.stride1 = stride1;
    P.stride2 = stride2;
    P.F1 = F1;
    P.F2 = F2;
    P.natoms = natoms;
    P.n = (uint32_t)n;

    MH_HIP(hipMemsetAsync(flags, 0, 16, c->stream));
    hipLaunchKernelGGL(tb_centre_kernel<PackIn<Real>>, dim3((uint32_t)L.Ftot), dim3(256), 0, c->stream, P, centre, flags);
    if (!fit) hipLaunchKernelGGL(tb_origin_kernel<>, dim3(1), dim3(1), 0, c->stream, centre, F1, origin);
    // the weights' sum and the index check decide the status, read back before the products are enqueued
    MH_TRY(check_selection(c, flags, centre + 3, who, natoms));

    const size_t Fpad = ((size_t)L.T1p + (sym ? 0 : L.T2p)) * RM_TILE;
    const double *org = fit ? nullptr : origin;
    hipLaunchKernelGGL(rm_pack_kernel<Real>, dim3(L.nchunks, L.T1p), dim3(256), 0, c->stream, P, 0, L.T1p, L.Kpad, centre, org, packed1, gpart, Fpad,
                       (size_t)0);
    if (!sym)
        hipLaunchKernelGGL(rm_pack_kernel<Real>, dim3(L.nchunks, L.T2p), dim3(256), 0, c->stream, P, 1, L.T2p, L.Kpad, centre, org, packed2, gpart, Fpad,
                           (size_t)L.T1p * RM_TILE);
    hipLaunchKernelGGL(rm_g_kernel, dim3((uint32_t)((Fpad + 255) / 256)), dim3(256), 0, c->stream, gpart, L.nchunks, Fpad, G);

    const bool out_dev = is_device_ptr(out);
    FinishP<Real> Fp{};
    Fp.G1 = G;
    Fp.G2 = sym ? G : G + (size_t)L.T1p * RM_TILE;
    Fp.sumw = centre + 3;
    Fp.F1 = F1;
    Fp.F2 = cols;
    Fp.sym = sym ? 1 : 0;
    Fp.fit = fit ? 1 : 0;
    if (out_dev) {
        Fp.out = out;
        Fp.ld = ld;
    } else {
        // not out_buffer: reserve adds headroom and reports MOLAR_HIP_ERR_HIP, which callers of this entry may rely on
        MH_TRY(Z.out.reserve(F1 * cols * sizeof(Real)));
        Fp.out = Z.out.as<Real>();
        Fp.ld = cols;
    }
    GramP Q{};
    Q.A = packed1;
    Q.B = packed2;
    Q.T1 = L.T1;
    Q.T2 = L.T2;
    Q.T1p = L.T1p;
    Q.T2p = L.T2p;
    Q.Kpad = L.Kpad;
    Q.ksteps = L.ksteps;
    Q.kper = L.kper;
    Q.sym = sym ? 1 : 0;
    const dim3 grid(L.T2p / RM_COLS, (L.T1 + RM_ROWS - 1) / RM_ROWS, L.ksplits);
    if (L.ksplits == 1) {
        Q.part = nullptr;
        hipLaunchKernelGGL((rm_gram_kernel<Real, true>), grid, dim3(64 * RM_ROWS), 0, c->stream, Q, Fp);
    } else {
        Q.part = part;
        hipLaunchKernelGGL((rm_gram_kernel<Real, false>), grid, dim3(64 * RM_ROWS), 0, c->stream, Q, Fp);
        hipLaunchKernelGGL(rm_finish_kernel<Real>, dim3((uint32_t)((size_t)L.T1 * L.T2p)), dim3(256), 0, c->stream, part, L.ksplits, L.T1, L.T2p, Fp);
    }
    MH_HIP(hipGetLastError());
    if (!out_dev) {
        MH_HIP(hipMemcpy2DAsync(out, ld * sizeof(Real), Fp.out, cols * sizeof(Real), cols * sizeof(Real), F1, hipMemcpyDeviceToHost, c->stream));
        MH_HIP(hipStreamSynchronize(c->stream));
    }
    return MOLAR_HIP_OK;
}

}  // namespace

namespace mh {
void rmsd_matrix_release(molar_hip_ctx *c) {
    release_state(c->rmsdm);
}
}  // namespace mh

extern "C" {

int molar_hip_rmsd_matrix_plan(size_t nframes1, size_t nframes2, size_t n, size_t *workspace_bytes, uint32_t *ksplits) {
    const Layout L = make_layout(nframes1, nframes2, n);
    const bool none = nframes1 == 0 || n == 0;
    if (workspace_bytes) *workspace_bytes = none ? 0 : L.bytes;
    if (ksplits) *ksplits = none ? 1u : L.ksplits;
    return MOLAR_HIP_OK;
}

int molar_hip_rmsd_matrix(molar_hip_ctx *c, const float *frames1, size_t nframes1, size_t frame_stride1, const float *frames2, size_t nframes2,
                          size_t frame_stride2, size_t natoms, const uint64_t *idx, size_t n, const float *mass, int fit, float *out, size_t ld) {
    return rmsd_matrix_run<float>(c, "rmsd_matrix", frames1, nframes1, frame_stride1, frames2, nframes2, frame_stride2, natoms, idx, n, mass, fit, out, ld);
}

int molar_hip_rmsd_matrix_f64(molar_hip_ctx *c, const double *frames1, size_t nframes1, size_t frame_stride1, const double *frames2, size_t nframes2,
                              size_t frame_stride2, size_t natoms, const uint64_t *idx, size_t n, const double *mass, int fit, double *out,
                              size_t ld) {
    return rmsd_matrix_run<double>(c, "rmsd_matrix_f64", frames1, nframes1, frame_stride1, frames2, nframes2, frame_stride2, natoms, idx, n, mass, fit,
                                   out, ld);
}

}  // extern "C"
