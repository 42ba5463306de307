// sfactor.hip - static structure factors of a block of trajectory frames by the direct sum over the reciprocal lattice of each
// frame's own box: the collective density rho_g(m; f) = sum_j w_j exp(-2 pi i m.s_j(f)) per group of atoms, its mean, the
// partial products S_ab(m) and their spherical (circular) average over shells of |q|.  The definition is in molar_hip.h.
//
// On an integer lattice the exponential factorises, exp(-2 pi i m.s) = Ex^h Ey^k Ez^l, so the whole grid of a (frame, group)
// is one complex matrix product over the atoms, C[row][col] = sum_j A[j][row] B[j][col], on v_mfma_f64_16x16x4_f64:
//
//   layout 0 (L > 0, or K = L = 0):  rows enumerate (h, k), columns l:   A = Ex^h Ey^k,  B = w Ez^l
//   layout 1 (L = 0, K > 0):         rows enumerate k, columns h:        A = Ey^k,       B = w Ex^h
//
// The operands are never in memory.  Stages, all on the context's stream:
//
//   boxes (one thread per frame: the inverse in double)
//   ->  prep: the indices, the labels and the weights judged, the atoms of every group counted (integer atomics)
//   ->  64 bytes read back: the status
//   ->  partition: a stable radix sort of the selection by label (devsort.hip), every group a contiguous range of the sorted
//       selection padded to a multiple of 4 with entries of weight 0; a group's range is cut into items of atom_chunk atoms
//   ->  per block of frame_block frames:
//         gram (a workgroup takes a 128 x 64 block of the grid, one item and one frame; per 16 atoms it forms s, writes the
//         powers of the three base phasors its block needs to LDS, and its four waves form their operands from two LDS reads
//         and one complex product and issue the MFMAs; the block goes to the workspace)
//         ->  finish (one lane per (frame, group, m): the items of the group in order; rho in double, and rounded to Real)
//         ->  products (one lane per (pair, m) or (group, m): the frames of the block in order into the running sums)
//         ->  shells under per-frame boxes (|q| and the bin per (frame, m); one lane per (frame, pair, shell) walks m in order;
//             one lane per (pair, shell) then adds the frames in order)
//   ->  the means over the ok frames, the shells under one box from the sums of S_ab, everything rounded to Real.
//
// Only integer atomics: no result depends on the order in which workgroups arrive, the same call gives the same bits.
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "boxmath.hpp"
#include "common.hpp"
#include "stages.hpp"
#include "traj_block.hpp"

using namespace mh;

struct molar_hip_sfactor_state {
    DevBuf in_frames, in_idx, in_weight, in_labels, in_boxes;   // host inputs staged here
    DevBuf sort_tmp;                                            // scratch of the device sort
    DevBuf ws;                                                  // the workspace molar_hip_sfactor_plan reports
};

namespace {

typedef unsigned long long u64;

constexpr uint32_t SF_WG = 256;                // threads of every workgroup here
constexpr uint32_t SF_RB = 128, SF_CB = 64;    // rows and columns of the grid block of a workgroup of the gram kernel: 2 x 2 waves of 64 x 32
constexpr uint32_t SF_CH = 16;                 // atoms whose powers are in LDS at a time (four MFMA steps)
constexpr uint32_t SF_SEG = 8;                 // powers per recurrence: one sincospi, then at most SF_SEG - 1 complex products
constexpr uint32_t SF_EMAX = 196;              // powers per atom a block can need: 128 + 2 of its rows, 64 of its columns, rounded up
constexpr uint32_t SF_BLK = SF_RB * SF_CB * 2; // doubles of one block
constexpr uint32_t SF_ATOM_CHUNK = 2048;       // atoms of an item (a K split) unless MOLAR_HIP_SFACTOR_ATOM_CHUNK says otherwise
constexpr uint32_t SF_MAX_FRAMES = 256;        // frames per block at the most
constexpr size_t SF_FRAME_BYTES = (size_t)1 << 30;   // the per-frame regions of a block together, unless one frame's are larger
constexpr double SF_TWO_PI = 6.283185307179586476925286766559;

// flags[0]: an index not below natoms; [1]: a box matrix without an inverse; [3]: a box vector of zero length;
// [4]: a selected weight that is not finite; [5]: a label not below ngroups; [7]: a block that needs more powers than SF_EMAX
constexpr uint32_t SF_FLAG_WORDS = 16;

struct Cx {
    double re, im;
};

// The lattice and how it is laid over rows and columns.
struct Shape {
    uint32_t H, K, L, W;        // W = 2K + 1
    uint32_t layout, R, Cn;     // rows and columns of the product
    uint32_t nrb, ncb;          // blocks of SF_RB rows and SF_CB columns
    uint32_t Q;
};

int make_shape(const char *who, const molar_hip_sfactor_grid *grid, Shape *S) {
    if (!grid) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: the grid is null", who);
    if (grid->reserved != 0) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: grid reserved = %u is not 0", who, grid->reserved);
    for (int d = 0; d < 3; ++d)
        if (grid->hmax[d] >= 1024u) return fail(MOLAR_HIP_ERR_TOO_LARGE, "%s: hmax[%d] = %u is not below 2^10", who, d, grid->hmax[d]);
    if (grid->nshells > 0 && !(grid->dq > 0.0 && std::isfinite(grid->dq) && std::isfinite(grid->qmin)))
        return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: shells of width dq = %g from qmin = %g", who, grid->dq, grid->qmin);
    S->H = grid->hmax[0];
    S->K = grid->hmax[1];
    S->L = grid->hmax[2];
    S->W = 2u * S->K + 1u;
    S->layout = (S->L == 0u && S->K > 0u) ? 1u : 0u;
    S->R = S->layout ? S->W : (S->H + 1u) * S->W;
    S->Cn = S->layout ? S->H + 1u : 2u * S->L + 1u;
    S->nrb = (S->R + SF_RB - 1u) / SF_RB;
    S->ncb = (S->Cn + SF_CB - 1u) / SF_CB;
    const size_t Q = (size_t)(S->H + 1u) * S->W * (2u * S->L + 1u);
    if (Q >= 0x80000000ull) return fail(MOLAR_HIP_ERR_TOO_LARGE, "%s: 2^31 lattice points or more", who);
    S->Q = (uint32_t)Q;
    return 0;
}

uint32_t env_u32(const char *name) {
    const char *e = std::getenv(name);
    if (!e || !*e) return 0u;
    const long v = std::strtol(e, nullptr, 10);
    return v > 0 && v < 0x40000000l ? (uint32_t)v : 0u;
}

// Where everything lives in the workspace, from the sizes alone (the plan entry and the call share it).
struct Layout {
    size_t G, P, ns;
    uint32_t atom_chunk, ksplits, items_cap, frame_block, ntiles;
    size_t selcap;
    size_t off_flags, off_inv, off_bad, off_ok, off_fv, off_cnt, off_start, off_goff, off_gitem, off_items, off_nitems, off_atom, off_w, off_iota,
        off_keys, off_perm, off_acc_sab, off_acc_mean, off_out_sab, off_out_mean, off_acc_shell, off_acc_count, off_out_shell, off_bins0, off_frames;
    size_t sz_part, sz_rho, sz_stage, sz_bins, sz_spart, sz_cpart, per_frame;   // the per-frame regions, each a multiple of 256 bytes
    size_t bytes;
};

size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

Layout make_layout(size_t F, size_t n, size_t G, const Shape &S, size_t ns) {
    Layout Y{};
    Y.G = G;
    Y.P = G * (G + 1) / 2;
    Y.ns = ns;
    uint32_t ac = env_u32("MOLAR_HIP_SFACTOR_ATOM_CHUNK");
    if (ac == 0u) ac = SF_ATOM_CHUNK;
    Y.atom_chunk = (ac + SF_CH - 1u) / SF_CH * SF_CH;
    Y.ksplits = (uint32_t)std::max<size_t>(1, (n + Y.atom_chunk - 1) / Y.atom_chunk);
    Y.items_cap = (uint32_t)std::min<size_t>((size_t)Y.ksplits + G, 0xFFFFFFFFull);
    Y.ntiles = S.nrb * S.ncb;
    Y.selcap = n + 3 * G;
    const size_t Q = S.Q;
    Y.sz_part = up256((size_t)Y.items_cap * Y.ntiles * SF_BLK * 8);
    Y.sz_rho = up256(G * Q * 16);
    Y.sz_stage = up256(G * Q * 16);
    Y.sz_bins = up256(Q * 4);
    Y.sz_spart = up256(Y.P * ns * 8);
    Y.sz_cpart = up256(ns * 8);
    Y.per_frame = Y.sz_part + Y.sz_rho + Y.sz_stage + Y.sz_bins + Y.sz_spart + Y.sz_cpart;
    const uint32_t fb_env = env_u32("MOLAR_HIP_SFACTOR_FRAME_BLOCK");
    // min(F, frame_block) frames fit, and the region never shrinks when an argument grows (frame_block * per_frame alone would)
    size_t region = std::min(std::min<size_t>(F, SF_MAX_FRAMES) * Y.per_frame, std::max(SF_FRAME_BYTES, Y.per_frame));
    size_t fb = std::max<size_t>(1, std::min<size_t>(std::min<size_t>(F, SF_MAX_FRAMES), Y.per_frame ? region / Y.per_frame : 1));
    if (fb_env) {
        fb = std::max<size_t>(1, std::min<size_t>(fb_env, std::max<size_t>(F, 1)));
        region = fb * Y.per_frame;
    }
    Y.frame_block = (uint32_t)fb;
    Carve ws;
    ws.take(Y.off_flags, SF_FLAG_WORDS * 4);
    ws.take(Y.off_inv, F * 9 * 8);
    ws.take(Y.off_bad, F * 4);
    ws.take(Y.off_ok, F * 4);
    ws.take(Y.off_fv, 16);
    ws.take(Y.off_cnt, G * 4);
    ws.take(Y.off_start, G * 4);
    ws.take(Y.off_goff, G * 4);
    ws.take(Y.off_gitem, (G + 1) * 4);
    ws.take(Y.off_items, (size_t)Y.items_cap * 16);
    ws.take(Y.off_nitems, 16);
    ws.take(Y.off_atom, Y.selcap * 8);
    ws.take(Y.off_w, Y.selcap * 8);
    ws.take(Y.off_iota, n * 4);
    ws.take(Y.off_keys, n * 4);
    ws.take(Y.off_perm, n * 4);
    ws.take(Y.off_acc_sab, Y.P * Q * 8);
    ws.take(Y.off_acc_mean, G * Q * 16);
    ws.take(Y.off_out_sab, Y.P * Q * 8);
    ws.take(Y.off_out_mean, G * Q * 16);
    ws.take(Y.off_acc_shell, Y.P * ns * 8);
    ws.take(Y.off_acc_count, ns * 8);
    ws.take(Y.off_out_shell, Y.P * ns * 8);
    ws.take(Y.off_bins0, Q * 4);
    ws.take(Y.off_frames, region);
    Y.bytes = ws.bytes;
    return Y;
}

// the sizes alone: what both the plan and the call refuse
int check_sizes(const char *who, size_t G, const Shape &S) {
    if (G >= 0x80000000ull || G * (size_t)S.Q >= 0x80000000ull) return fail(MOLAR_HIP_ERR_TOO_LARGE, "%s: 2^31 entries (groups times lattice points) or more", who);
    if (G * (G + 1) / 2 * (size_t)S.Q >= ((size_t)1 << 40)) return fail(MOLAR_HIP_ERR_TOO_LARGE, "%s: 2^40 entries (pairs of groups times lattice points) or more", who);
    return 0;
}

// ---------------------------------------------------------------- small kernels

// One thread per frame: the inverse of the frame's box as PeriodicBox::from_matrix forms it (its two errors raise flags[3] and
// flags[1]), column-major.
template <class Real>
__global__ void __launch_bounds__(64) sf_box_kernel(const Real *__restrict__ boxes, size_t box_stride, size_t F, double *__restrict__ inv,
                                                    uint32_t *__restrict__ flags) {
    const size_t f = (size_t)blockIdx.x * 64u + threadIdx.x;
    if (f >= F) return;
    double m[9], v[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) m[q] = (double)boxes[f * box_stride + q];
    bool ok = true;
    for (int k = 0; k < 3; ++k)
        if (sqrt(norm2(D3{m[3 * k], m[3 * k + 1], m[3 * k + 2]})) == 0.0) ok = false;
#pragma unroll
    for (int q = 0; q < 9; ++q) v[q] = __builtin_nan("");
    if (!ok) flags[3] = 1u;
    else if (!inverse3(m, v)) flags[1] = 1u;
#pragma unroll
    for (int q = 0; q < 9; ++q) inv[f * 9 + q] = v[q];
}

template <class Real>
struct Sel {
    const uint64_t *idx;
    size_t n, natoms;
    const Real *weight;
    const uint32_t *labels;
    uint32_t ngroups;
};

// Grid-stride over the selection: the flags above and the atoms of every group.
template <class Real>
__global__ void __launch_bounds__(SF_WG) sf_prep_kernel(Sel<Real> P, uint32_t *__restrict__ cnt, uint32_t *__restrict__ iota, uint32_t *__restrict__ flags) {
    const size_t step = (size_t)gridDim.x * SF_WG, t0 = (size_t)blockIdx.x * SF_WG + threadIdx.x;
    for (size_t k = t0; k < P.n; k += step) {
        const uint64_t a = P.idx ? P.idx[k] : (uint64_t)k;
        if (a >= P.natoms) flags[0] = 1u;
        else if (P.weight && !isfinite((double)P.weight[a])) flags[4] = 1u;
        if (P.labels) {
            const uint32_t g = P.labels[k];
            if (g >= P.ngroups) flags[5] = 1u;
            else atomicAdd(&cnt[g], 1u);
            iota[k] = (uint32_t)k;
        } else if (k == 0) {
            cnt[0] = (uint32_t)P.n;
        }
    }
}

struct Groups {
    const uint32_t *cnt;
    uint32_t *start, *goff, *gitem, *items, *nitems;
    uint32_t G, atom_chunk, items_cap;
};

// One thread: where every group starts in the sorted selection (start) and in the padded one (goff), and the items - group,
// first and last padded position - in group order, a group's items in order of position; gitem[g] .. gitem[g + 1] are the
// items of group g.
__global__ void sf_groups_kernel(Groups Z) {
    uint32_t pos = 0, ni = 0, us = 0;
    for (uint32_t g = 0; g < Z.G; ++g) {
        const uint32_t c = Z.cnt[g], np = (c + 3u) & ~3u;
        Z.start[g] = us;
        Z.goff[g] = pos;
        Z.gitem[g] = ni;
        for (uint32_t k = 0; k < np && ni < Z.items_cap; k += Z.atom_chunk) {
            Z.items[4 * ni] = g;
            Z.items[4 * ni + 1] = pos + k;
            Z.items[4 * ni + 2] = pos + min(k + Z.atom_chunk, np);
            Z.items[4 * ni + 3] = 0u;
            ++ni;
        }
        pos += np;
        us += c;
    }
    Z.gitem[Z.G] = ni;
    Z.nitems[0] = ni;
    Z.nitems[1] = pos;
}

// The padded selection filled with entries of weight 0 (the first selected atom), then the sorted selection scattered into it.
template <class Real>
__global__ void __launch_bounds__(SF_WG) sf_fill_kernel(Sel<Real> P, size_t selcap, uint64_t *__restrict__ atom, double *__restrict__ w) {
    const size_t j = (size_t)blockIdx.x * SF_WG + threadIdx.x;
    if (j >= selcap) return;
    atom[j] = P.idx ? P.idx[0] : 0ull;
    w[j] = 0.0;
}
template <class Real>
__global__ void __launch_bounds__(SF_WG) sf_scatter_kernel(Sel<Real> P, const uint32_t *__restrict__ keys, const uint32_t *__restrict__ perm,
                                                           const uint32_t *__restrict__ start, const uint32_t *__restrict__ goff,
                                                           uint64_t *__restrict__ atom, double *__restrict__ w) {
    const size_t j = (size_t)blockIdx.x * SF_WG + threadIdx.x;
    if (j >= P.n) return;
    const uint32_t g = keys ? keys[j] : 0u;
    const size_t k = perm ? perm[j] : j;
    const uint64_t a = P.idx ? P.idx[k] : (uint64_t)k;
    const size_t dst = (size_t)goff[g] + (j - start[g]);
    atom[dst] = a;
    w[dst] = P.weight ? (double)P.weight[a] : 1.0;
}

// ---------------------------------------------------------------- the gram kernel

template <class Real>
struct Gram {
    const Real *frames;
    size_t stride, f0;
    const double *inv;            // [F][9]
    const uint64_t *atom;         // the padded sorted selection
    const double *w;
    const uint32_t *items;        // [items][4]
    const uint32_t *nitems;
    Shape S;
    double *part;                 // [frames of the block][items_cap][tiles][SF_RB][SF_CB][2]
    uint32_t items_cap;
    uint32_t *bad;                // [F]
    uint32_t *flags;
};

// row of the product -> the powers of Ex and Ey of A; column -> the power of Ez (layout 0) or Ex (layout 1) of B
__device__ __forceinline__ void row_powers(const Shape &S, uint32_t row, uint32_t &h, int &k) {
    if (S.layout) {
        h = 0u;
        k = (int)row - (int)S.K;
    } else {
        h = row / S.W;
        k = (int)(row - h * S.W) - (int)S.K;
    }
}
__device__ __forceinline__ int col_power(const Shape &S, uint32_t col) { return S.layout ? (int)col : (int)col - (int)S.L; }

__device__ __forceinline__ Cx cmul(Cx a, Cx b) { return Cx{a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }

// Workgroup (x, y, z): block x of the grid (row block x / ncb, column block x % ncb), item y, frame f0 + z.  Wave v takes rows
// 64 (v >> 1) .. + 64 and columns 32 (v & 1) .. + 32 of the block: four row tiles times two column tiles, a real and an
// imaginary accumulator each (16 accumulators, the registers of fluct's 64 x 64 real block).
// Per SF_CH atoms of the item:
//   1. threads 0 .. 15: atom j: s = inv p, s_d -= floor(s_d); a coordinate that is not finite raises bad[f]; an entry behind the
//      item's end has weight 0 and s = 0.
//   2. the powers the block needs, per atom three tables of non-negative powers p in [lo_d, hi_d] (d = x, y, z; what the rows
//      and columns of the block reach, negative powers are conjugates): a task takes one atom and SF_SEG consecutive powers of
//      one table; the first is E^p0 = (cos, -sin)(2 pi t), t = p0 s_d - floor(p0 s_d), by sincospi(2 t), every next one the
//      product of the one before with E^1 = (cos, -sin)(2 pi s_d), re = ar br - ai bi, im = ar bi + ai br.
//   3. four MFMA steps of four atoms: lane l forms A for row (l & 15) of each of its four row tiles and B for column (l & 15)
//      of its two column tiles, of atom 4 step + (l >> 4):  layout 0: A = X[h] * Y[|k|] (conjugated for k < 0),
//      B = w * Z[|l|] (conjugated for l < 0);  layout 1: A = Y[|k|] (conjugated), B = w * X[h];  then per tile pair
//      re += Ar Br, re += (-Ai) Bi, im += Ar Bi, im += Ai Br, in that order.
// Rows and columns of a block beyond the grid take the powers of the last row and column: their results are never read, and a
// tile pair without a row or a column of the grid issues no MFMA (a wave-uniform mask).
template <class Real>
__global__ void __launch_bounds__(SF_WG) __attribute__((amdgpu_waves_per_eu(2))) sf_gram_kernel(Gram<Real> P) {
    __shared__ Cx tab[SF_CH * SF_EMAX];
    __shared__ double sh_s[SF_CH][3];
    __shared__ double sh_w[SF_CH];
    __shared__ int sh_lo[3], sh_hi[3];
    const uint32_t item = blockIdx.y;
    if (item >= P.nitems[0]) return;
    const Shape S = P.S;
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const uint32_t rb = blockIdx.x / S.ncb, cb = blockIdx.x - rb * S.ncb;
    const uint32_t row0 = rb * SF_RB, col0 = cb * SF_CB;
    const size_t f = P.f0 + blockIdx.z;
    const uint32_t k0 = P.items[4 * item + 1], k1 = P.items[4 * item + 2];

    // the ranges of the three tables
    if (t < 3u) {
        sh_lo[t] = 0x7FFFFFFF;
        sh_hi[t] = -1;
    }
    __syncthreads();
    if (t < SF_RB) {
        uint32_t h;
        int k;
        row_powers(S, min(row0 + t, S.R - 1u), h, k);
        const int ak = k < 0 ? -k : k;
        if (!S.layout) {
            atomicMin(&sh_lo[0], (int)h);
            atomicMax(&sh_hi[0], (int)h);
        }
        atomicMin(&sh_lo[1], ak);
        atomicMax(&sh_hi[1], ak);
    } else if (t < SF_RB + SF_CB) {
        const int p = col_power(S, min(col0 + (t - SF_RB), S.Cn - 1u));
        const int ap = p < 0 ? -p : p;
        const int d = S.layout ? 0 : 2;
        atomicMin(&sh_lo[d], ap);
        atomicMax(&sh_hi[d], ap);
    }
    __syncthreads();
    int lo[3], cnt[3];
    uint32_t off[3], nseg[3];
    uint32_t E = 0, nsegs = 0;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        lo[d] = sh_lo[d];
        cnt[d] = sh_hi[d] >= sh_lo[d] ? sh_hi[d] - sh_lo[d] + 1 : 0;
        off[d] = E;
        E += (uint32_t)cnt[d];
        nseg[d] = ((uint32_t)cnt[d] + SF_SEG - 1u) / SF_SEG;
        nsegs += nseg[d];
    }
    if (E > SF_EMAX) {                 // cannot happen (see SF_EMAX); nothing is written out of bounds if it does
        if (t == 0u) P.flags[7] = 1u;
        return;
    }

    // where this lane's operands are in an atom's slab
    const uint32_t wr = wave >> 1, wc = wave & 1u;
    uint32_t aox[4], aoy[4], bo[2];
    bool asg[4], bsg[2];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        uint32_t h;
        int k;
        row_powers(S, min(row0 + wr * 64u + (uint32_t)i * 16u + (lane & 15u), S.R - 1u), h, k);
        asg[i] = k < 0;
        aox[i] = S.layout ? 0u : off[0] + (h - (uint32_t)lo[0]);
        aoy[i] = off[1] + (uint32_t)((k < 0 ? -k : k) - lo[1]);
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int p = col_power(S, min(col0 + wc * 32u + (uint32_t)j * 16u + (lane & 15u), S.Cn - 1u));
        const int d = S.layout ? 0 : 2;
        bsg[j] = p < 0;
        bo[j] = off[d] + (uint32_t)((p < 0 ? -p : p) - lo[d]);
    }

    // tile pairs of this wave that hold a row and a column of the grid (bit 2 i + j): the others are never read and take no MFMA
    uint32_t live = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
            if (row0 + wr * 64u + (uint32_t)i * 16u < S.R && col0 + wc * 32u + (uint32_t)j * 16u < S.Cn) live |= 1u << (2 * i + j);
    live = __builtin_amdgcn_readfirstlane(live);

    d4 re[4][2], im[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            re[i][j] = d4{0.0, 0.0, 0.0, 0.0};
            im[i][j] = d4{0.0, 0.0, 0.0, 0.0};
        }

    const Real *p = P.frames + f * P.stride;
    const double *inv = P.inv + f * 9;
    for (uint32_t kc = k0; kc < k1; kc += SF_CH) {
        __syncthreads();                                   // the MFMA steps of the chunk before have read the tables
        if (t < SF_CH) {
            const uint32_t j = kc + t;
            double s[3] = {0.0, 0.0, 0.0}, w = 0.0;
            if (j < k1) {
                const uint64_t a = P.atom[j];
                w = P.w[j];
                const D3 x{(double)p[3 * a], (double)p[3 * a + 1], (double)p[3 * a + 2]};
                if (!(isfinite(x.x) && isfinite(x.y) && isfinite(x.z))) atomicOr(&P.bad[f], 1u);
                const D3 v = mat_vec(inv, x);
                s[0] = v.x - floor(v.x);
                s[1] = v.y - floor(v.y);
                s[2] = v.z - floor(v.z);
            }
            sh_s[t][0] = s[0];
            sh_s[t][1] = s[1];
            sh_s[t][2] = s[2];
            sh_w[t] = w;
        }
        __syncthreads();
        for (uint32_t task = t; task < SF_CH * nsegs; task += SF_WG) {
            const uint32_t a = task / nsegs;
            uint32_t sg = task - a * nsegs;
            int d = 0;
            if (sg >= nseg[0]) {
                sg -= nseg[0];
                d = 1;
                if (sg >= nseg[1]) {
                    sg -= nseg[1];
                    d = 2;
                }
            }
            const double sd = sh_s[a][d];
            double sn, cs;
            sincospi(2.0 * sd, &sn, &cs);
            const Cx e1{cs, -sn};
            const uint32_t q0 = sg * SF_SEG, q1 = min(q0 + SF_SEG, (uint32_t)cnt[d]);
            double tt = (double)(lo[d] + (int)q0) * sd;
            tt -= floor(tt);
            sincospi(2.0 * tt, &sn, &cs);
            Cx cur{cs, -sn};
            Cx *dst = tab + a * SF_EMAX + off[d];
            dst[q0] = cur;
            for (uint32_t q = q0 + 1u; q < q1; ++q) {
                cur = cmul(cur, e1);
                dst[q] = cur;
            }
        }
        __syncthreads();
#pragma unroll
        for (uint32_t ks = 0; ks < SF_CH / 4u; ++ks) {
            const uint32_t a = ks * 4u + (lane >> 4);
            const Cx *slab = tab + a * SF_EMAX;
            const double w = sh_w[a];
            double ar[4], ai[4], nai[4], br[2], bi[2];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                Cx y = slab[aoy[i]];
                if (asg[i]) y.im = -y.im;
                if (S.layout) {
                    ar[i] = y.re;
                    ai[i] = y.im;
                } else {
                    const Cx v = cmul(slab[aox[i]], y);
                    ar[i] = v.re;
                    ai[i] = v.im;
                }
                nai[i] = -ai[i];
            }
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                Cx z = slab[bo[j]];
                if (bsg[j]) z.im = -z.im;
                br[j] = w * z.re;
                bi[j] = w * z.im;
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    if (live >> (2 * i + j) & 1u) re[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(ar[i], br[j], re[i][j], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    if (live >> (2 * i + j) & 1u) im[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(ar[i], bi[j], im[i][j], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    if (live >> (2 * i + j) & 1u) re[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(nai[i], bi[j], re[i][j], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    if (live >> (2 * i + j) & 1u) im[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(ai[i], br[j], im[i][j], 0, 0, 0);
        }
    }

    double *dst = P.part + (((size_t)blockIdx.z * P.items_cap + item) * (S.nrb * S.ncb) + blockIdx.x) * SF_BLK;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const size_t row = mfma_c_row(wr * 64u + (uint32_t)i * 16u, lane, (uint32_t)r), col = mfma_c_col(wc * 32u + (uint32_t)j * 16u, lane);
                double *o = dst + (row * SF_CB + col) * 2u;
                o[0] = re[i][j][r];
                o[1] = im[i][j][r];
            }
}

// Where rho goes for the caller: rows (f, g) of `stride` Reals from `base` (null: not asked for).
template <class Real>
struct RhoOut {
    Real *base;
    size_t stride;
};

// One lane per (frame z of the block, group, m): the blocks of the group's items added in item order; a frame that is not ok
// is NaN.  rho64[z][g][m] in double for the products, and rounded to Real for the caller.
template <class Real>
__global__ void __launch_bounds__(SF_WG) sf_finish_kernel(const double *__restrict__ part, uint32_t items_cap, const uint32_t *__restrict__ gitem, Shape S,
                                                          uint32_t G, size_t f0, const uint32_t *__restrict__ bad, Cx *__restrict__ rho64, RhoOut<Real> O) {
    const size_t gm = (size_t)blockIdx.x * SF_WG + threadIdx.x;
    if (gm >= (size_t)G * S.Q) return;
    const uint32_t g = (uint32_t)(gm / S.Q), m = (uint32_t)(gm - (size_t)g * S.Q);
    uint32_t row, col;
    if (S.layout) {
        col = m / S.W;
        row = m - col * S.W;
    } else {
        row = m / S.Cn;
        col = m - row * S.Cn;
    }
    const uint32_t rb = row / SF_RB, cb = col / SF_CB, ntiles = S.nrb * S.ncb;
    const size_t offs = ((size_t)(row - rb * SF_RB) * SF_CB + (col - cb * SF_CB)) * 2u;
    const uint32_t z = blockIdx.y;
    Cx sum{0.0, 0.0};
    for (uint32_t it = gitem[g]; it < gitem[g + 1]; ++it) {
        const double *src = part + (((size_t)z * items_cap + it) * ntiles + (rb * S.ncb + cb)) * SF_BLK + offs;
        sum.re += src[0];
        sum.im += src[1];
    }
    if (bad[f0 + z]) sum = Cx{__builtin_nan(""), __builtin_nan("")};
    rho64[((size_t)z * G + g) * S.Q + m] = sum;
    if (O.base) {
        Real *o = O.base + ((size_t)z * G + g) * O.stride + 2u * (size_t)m;
        o[0] = (Real)sum.re;
        o[1] = (Real)sum.im;
    }
}

// ---------------------------------------------------------------- products and shells

__device__ __forceinline__ void pair_of(uint32_t p, uint32_t G, uint32_t &a, uint32_t &b) {
    a = 0;
    while (p >= G - a) {
        p -= G - a;
        ++a;
    }
    b = a + p;
}
__device__ __forceinline__ double re_prod(Cx x, Cx y) { return x.re * y.re + x.im * y.im; }   // Re(x conj y)

// One lane per (pair, m): the ok frames of the block in order into acc_sab; then one lane per (group, m) into acc_mean.
__global__ void __launch_bounds__(SF_WG) sf_products_kernel(const Cx *__restrict__ rho64, uint32_t nf, size_t f0, const uint32_t *__restrict__ bad, uint32_t G,
                                                            uint32_t Q, size_t npq, double *__restrict__ acc_sab, Cx *__restrict__ acc_mean) {
    const size_t i = (size_t)blockIdx.x * SF_WG + threadIdx.x;
    if (i < npq) {
        if (!acc_sab) return;
        const uint32_t p = (uint32_t)(i / Q), m = (uint32_t)(i - (size_t)p * Q);
        uint32_t a, b;
        pair_of(p, G, a, b);
        double s = acc_sab[i];
        for (uint32_t z = 0; z < nf; ++z)
            if (!bad[f0 + z]) s += re_prod(rho64[((size_t)z * G + a) * Q + m], rho64[((size_t)z * G + b) * Q + m]);
        acc_sab[i] = s;
        return;
    }
    const size_t gm = i - npq;
    if (gm >= (size_t)G * Q || !acc_mean) return;
    Cx s = acc_mean[gm];
    for (uint32_t z = 0; z < nf; ++z)
        if (!bad[f0 + z]) {
            const Cx v = rho64[(size_t)z * G * Q + gm];
            s.re += v.re;
            s.im += v.im;
        }
    acc_mean[gm] = s;
}

struct ShellSpec {
    double qmin, dq;
    uint32_t ns;
};

// One lane per (m, frame z of the block): the shell of m under the frame's box, -1 where m is not of the canonical half-space
// (h > 0, or h = 0 and k > 0, or h = k = 0 and l > 0) or lies in no shell.  v_r = (inv[3r] h + inv[3r+1] k) + inv[3r+2] l,
// |q| = 2 pi sqrt((v0 v0 + v1 v1) + v2 v2), bin = floor((|q| - qmin) / dq).
__global__ void __launch_bounds__(SF_WG) sf_bins_kernel(const double *__restrict__ inv, size_t f0, Shape S, ShellSpec Z, int32_t *__restrict__ bins) {
    const uint32_t m = blockIdx.x * SF_WG + threadIdx.x;
    if (m >= S.Q) return;
    const uint32_t nl = 2u * S.L + 1u;
    const uint32_t hk = m / nl;
    const int l = (int)(m - hk * nl) - (int)S.L;
    const uint32_t h = hk / S.W;
    const int k = (int)(hk - h * S.W) - (int)S.K;
    int32_t b = -1;
    if (h > 0u || k > 0 || (k == 0 && l > 0)) {
        const double *v = inv + (f0 + blockIdx.y) * 9;
        const double dh = (double)h, dk = (double)k, dl = (double)l;
        const double v0 = (v[0] * dh + v[1] * dk) + v[2] * dl, v1 = (v[3] * dh + v[4] * dk) + v[5] * dl, v2 = (v[6] * dh + v[7] * dk) + v[8] * dl;
        const double q = SF_TWO_PI * sqrt((v0 * v0 + v1 * v1) + v2 * v2);
        const double x = floor((q - Z.qmin) / Z.dq);
        if (x >= 0.0 && x < (double)Z.ns) b = (int32_t)x;
    }
    bins[(size_t)blockIdx.y * S.Q + m] = b;
}

// Per-frame boxes.  One lane per (pair, shell) and frame z of the block: the members of the shell in index order.
__global__ void __launch_bounds__(SF_WG) sf_shell_frame_kernel(const Cx *__restrict__ rho64, const int32_t *__restrict__ bins, uint32_t G, uint32_t Q, uint32_t ns,
                                                               size_t nps, double *__restrict__ spart, u64 *__restrict__ cpart) {
    const size_t i = (size_t)blockIdx.x * SF_WG + threadIdx.x;
    if (i >= nps) return;
    const uint32_t p = (uint32_t)(i / ns), sb = (uint32_t)(i - (size_t)p * ns), z = blockIdx.y;
    uint32_t a, b;
    pair_of(p, G, a, b);
    const Cx *ra = rho64 + ((size_t)z * G + a) * Q, *rbp = rho64 + ((size_t)z * G + b) * Q;
    const int32_t *bz = bins + (size_t)z * Q;
    double s = 0.0;
    u64 c = 0;
    for (uint32_t m = 0; m < Q; ++m)
        if (bz[m] == (int32_t)sb) {
            s += re_prod(ra[m], rbp[m]);
            ++c;
        }
    spart[(size_t)z * nps + i] = s;
    if (p == 0u) cpart[(size_t)z * ns + sb] = c;
}
// ... and one lane per (pair, shell): the ok frames of the block in order.
__global__ void __launch_bounds__(SF_WG) sf_shell_fold_kernel(const double *__restrict__ spart, const u64 *__restrict__ cpart, uint32_t nf, size_t f0,
                                                              const uint32_t *__restrict__ bad, uint32_t ns, size_t nps, double *__restrict__ acc,
                                                              u64 *__restrict__ count) {
    const size_t i = (size_t)blockIdx.x * SF_WG + threadIdx.x;
    if (i >= nps) return;
    double s = acc[i];
    u64 c = i < ns ? count[i] : 0;
    for (uint32_t z = 0; z < nf; ++z)
        if (!bad[f0 + z]) {
            s += spart[(size_t)z * nps + i];
            if (i < ns) c += cpart[(size_t)z * ns + i];
        }
    acc[i] = s;
    if (i < ns) count[i] = c;
}
// One box for every frame: the membership is that of frame 0, and the sums over the frames of S_ab are binned once, the
// members in index order.
__global__ void __launch_bounds__(SF_WG) sf_shell_once_kernel(const double *__restrict__ acc_sab, const int32_t *__restrict__ bins, uint32_t Q, uint32_t ns,
                                                              size_t nps, const u64 *__restrict__ fv, double *__restrict__ acc, u64 *__restrict__ count) {
    const size_t i = (size_t)blockIdx.x * SF_WG + threadIdx.x;
    if (i >= nps) return;
    const uint32_t p = (uint32_t)(i / ns), sb = (uint32_t)(i - (size_t)p * ns);
    double s = 0.0;
    u64 c = 0;
    for (uint32_t m = 0; m < Q; ++m)
        if (bins[m] == (int32_t)sb) {
            s += acc_sab[(size_t)p * Q + m];
            ++c;
        }
    acc[i] = s;
    if (p == 0u) count[sb] = c * fv[0];
}

// The ok frames: ok[f] = 1 - bad[f], fv[0] = how many.
__global__ void __launch_bounds__(SF_WG) sf_ok_kernel(const uint32_t *__restrict__ bad, size_t F, uint32_t *__restrict__ ok, u64 *__restrict__ fv) {
    __shared__ u64 sh;
    if (threadIdx.x == 0u) sh = 0;
    __syncthreads();
    u64 c = 0;
    for (size_t f = threadIdx.x; f < F; f += SF_WG) {
        const uint32_t o = bad[f] ? 0u : 1u;
        ok[f] = o;
        c += o;
    }
    if (c) atomicAdd(&sh, c);
    __syncthreads();
    if (threadIdx.x == 0u) fv[0] = sh;
}

// The means: sums / Fv (NaN without an ok frame), and shell sums / counts (NaN for a count of 0), rounded to Real.
template <class Real>
__global__ void __launch_bounds__(SF_WG) sf_mean_kernel(const double *__restrict__ acc, size_t count, const u64 *__restrict__ fv, Real *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * SF_WG + threadIdx.x;
    if (i >= count) return;
    out[i] = fv[0] ? (Real)(acc[i] / (double)fv[0]) : (Real)__builtin_nan("");
}
template <class Real>
__global__ void __launch_bounds__(SF_WG) sf_shell_out_kernel(const double *__restrict__ acc, const u64 *__restrict__ count, uint32_t ns, size_t nps,
                                                             Real *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * SF_WG + threadIdx.x;
    if (i >= nps) return;
    const u64 c = count[i % ns];
    out[i] = c ? (Real)(acc[i] / (double)c) : (Real)__builtin_nan("");
}

int ceil_log2(size_t n) {
    int c = 0;
    while (c < 63 && ((size_t)1 << c) < n) ++c;
    return c;
}

template <class T>
int copy_any(molar_hip_ctx *c, T *dst, const T *dev, size_t count, bool &wait) {
    if (!dst) return 0;
    if (!is_device_ptr(dst)) wait = true;
    MH_HIP(hipMemcpyAsync(dst, dev, count * sizeof(T), hipMemcpyDefault, c->stream));
    return 0;
}

uint32_t blocks_of(size_t items) { return (uint32_t)((items + SF_WG - 1) / SF_WG); }

template <class Real>
int sfactor_run(molar_hip_ctx *c, const char *who, const Real *frames, size_t F, size_t stride, size_t natoms, const uint64_t *idx, size_t n,
                const Real *weight, const uint32_t *labels, size_t ngroups, const Real *boxes, size_t box_stride, const molar_hip_sfactor_grid *grid,
                Real *rho, size_t rho_stride, uint32_t *frame_ok, Real *rho_mean, Real *sab, Real *shell, uint64_t *shell_count) {
    // the arguments are judged before the context is used
    if (!c) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "null context");
    if (n == 0) return fail(MOLAR_HIP_ERR_SIZES, "%s: empty selection", who);
    const size_t G = labels ? ngroups : 1;
    if (G == 0) return fail(MOLAR_HIP_ERR_SIZES, "%s: labels and ngroups = 0", who);
    Shape S{};
    MH_TRY(make_shape(who, grid, &S));
    if (box_stride != 0 && box_stride != 9) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: box_stride = %zu is neither 0 nor 9", who, box_stride);
    if (natoms == 0) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: a selection of %zu atoms out of natoms = 0", who, n);
    MH_TRY(check_no_index(who, "n", idx, n, natoms));
    MH_TRY(check_stride(who, "the frame stride", F, stride, natoms));
    if (rho && rho_stride < 2 * (size_t)S.Q) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: rho_stride = %zu is below 2 Q = %zu", who, rho_stride, 2 * (size_t)S.Q);
    if (!boxes) return fail(MOLAR_HIP_ERR_NO_PBC, "%s: a reciprocal lattice without a box", who);
    if (n >= 0x7FFFFF00ull || F >= 0x7FFFFFF0ull) return fail(MOLAR_HIP_ERR_TOO_LARGE, "%s: more than 2^31 atoms or frames", who);
    MH_TRY(check_sizes(who, G, S));
    const size_t ns = grid->nshells;
    const Layout Y = make_layout(F, n, G, S, ns);
    if ((size_t)Y.ksplits + G > 65535u) return fail(MOLAR_HIP_ERR_TOO_LARGE, "%s: %u splits of the atoms and %zu groups are more than 65535 items", who, Y.ksplits, G);
    if ((size_t)Y.ntiles >= 0x7FFFFFFFull) return fail(MOLAR_HIP_ERR_TOO_LARGE, "%s: 2^31 blocks of the lattice", who);
    if (F == 0) return MOLAR_HIP_OK;
    if (!frames) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: the frames pointer is null", who);
    MH_TRY(check_index(who, "idx", idx, n, natoms));
    // labels in host memory are walked here; those in device memory are judged by the prep kernel before one is used as an address
    const bool labels_dev = is_device_ptr(labels);
    if (labels && !labels_dev)
        for (size_t k = 0; k < n; ++k)
            if (labels[k] >= G) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: labels[%zu] = %u is not below ngroups = %zu", who, k, labels[k], G);
    MH_HIP(hipSetDevice(c->device));

    molar_hip_sfactor_state &Z = state_of(c->sfactor);
    MH_TRY(grow_exact(Z.ws, Y.bytes, who, "the workspace"));
    char *W = Z.ws.as<char>();
    auto u32at = [&](size_t off) { return reinterpret_cast<uint32_t *>(W + off); };
    auto f64at = [&](size_t off) { return reinterpret_cast<double *>(W + off); };
    uint32_t *flags = u32at(Y.off_flags), *bad = u32at(Y.off_bad), *ok_d = u32at(Y.off_ok);
    u64 *fv = reinterpret_cast<u64 *>(W + Y.off_fv);
    double *inv = f64at(Y.off_inv);
    uint32_t *cnt = u32at(Y.off_cnt), *iota = u32at(Y.off_iota), *keys = u32at(Y.off_keys), *perm = u32at(Y.off_perm);
    uint64_t *atom_d = reinterpret_cast<uint64_t *>(W + Y.off_atom);
    double *w_d = f64at(Y.off_w);

    Sel<Real> P{};
    const Real *frames_d = nullptr, *boxes_d = nullptr;
    P.n = n;
    P.natoms = natoms;
    P.ngroups = (uint32_t)G;
    MH_TRY(to_device(c, frames, (F - 1) * stride + natoms * 3, Z.in_frames, &frames_d));
    MH_TRY(to_device(c, idx, idx ? n : 0, Z.in_idx, &P.idx));
    MH_TRY(to_device(c, weight, weight ? natoms : 0, Z.in_weight, &P.weight));
    MH_TRY(to_device(c, labels, labels ? n : 0, Z.in_labels, &P.labels));
    MH_TRY(to_device(c, boxes, box_stride ? F * 9 : 9, Z.in_boxes, &boxes_d));

    MH_HIP(hipMemsetAsync(flags, 0, SF_FLAG_WORDS * 4, c->stream));
    MH_HIP(hipMemsetAsync(cnt, 0, G * 4, c->stream));
    const uint32_t fblocks = (uint32_t)((F + 63) / 64);
    hipLaunchKernelGGL(sf_box_kernel<Real>, dim3(fblocks), dim3(64), 0, c->stream, boxes_d, box_stride, F, inv, flags);
    hipLaunchKernelGGL(sf_prep_kernel<Real>, dim3(std::min<uint32_t>(blocks_of(n), 1024u)), dim3(SF_WG), 0, c->stream, P, cnt, iota, flags);
    MH_HIP(hipGetLastError());
    // the one read-back: the status.  Nothing below runs, no label is used as an address and no output is touched after a bad argument.
    uint32_t hf[SF_FLAG_WORDS];
    MH_TRY(read_back(c, hf, flags, sizeof hf));
    if (hf[0]) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: a selection index is not below natoms = %zu", who, natoms);
    if (hf[5]) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: a label is not below ngroups = %zu", who, G);
    if (hf[4]) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: a selected weight is not finite", who);
    if (hf[3]) return fail(MOLAR_HIP_ERR_ZERO_LENGTH_VECTOR, "%s: zero length box vector", who);
    if (hf[1]) return fail(MOLAR_HIP_ERR_INVERSE_FAILED, "%s: box matrix inverse failed", who);

    // the partition
    if (P.labels) MH_TRY(device_sort_pairs_u32(c->stream, Z.sort_tmp, P.labels, keys, iota, perm, n, std::max(1, ceil_log2(G))));
    Groups Gr{};
    Gr.cnt = cnt;
    Gr.start = u32at(Y.off_start);
    Gr.goff = u32at(Y.off_goff);
    Gr.gitem = u32at(Y.off_gitem);
    Gr.items = u32at(Y.off_items);
    Gr.nitems = u32at(Y.off_nitems);
    Gr.G = (uint32_t)G;
    Gr.atom_chunk = Y.atom_chunk;
    Gr.items_cap = Y.items_cap;
    hipLaunchKernelGGL(sf_groups_kernel, dim3(1), dim3(1), 0, c->stream, Gr);
    hipLaunchKernelGGL(sf_fill_kernel<Real>, dim3(blocks_of(Y.selcap)), dim3(SF_WG), 0, c->stream, P, Y.selcap, atom_d, w_d);
    hipLaunchKernelGGL(sf_scatter_kernel<Real>, dim3(blocks_of(n)), dim3(SF_WG), 0, c->stream, P, P.labels ? keys : nullptr, P.labels ? perm : nullptr, Gr.start,
                       Gr.goff, atom_d, w_d);

    const size_t Q = S.Q, GQ = G * Q, PQ = Y.P * Q, nps = Y.P * ns;
    const bool want_shell = ns != 0 && (shell || shell_count);
    const bool shell_once = want_shell && box_stride == 0;
    const bool want_sab = sab != nullptr || shell_once;
    double *acc_sab = f64at(Y.off_acc_sab), *acc_shell = f64at(Y.off_acc_shell);
    Cx *acc_mean = reinterpret_cast<Cx *>(W + Y.off_acc_mean);
    u64 *acc_count = reinterpret_cast<u64 *>(W + Y.off_acc_count);
    int32_t *bins0 = reinterpret_cast<int32_t *>(W + Y.off_bins0);
    MH_HIP(hipMemsetAsync(bad, 0, F * 4, c->stream));
    if (want_sab) MH_HIP(hipMemsetAsync(acc_sab, 0, PQ * 8, c->stream));
    if (rho_mean) MH_HIP(hipMemsetAsync(acc_mean, 0, GQ * 16, c->stream));
    if (want_shell) {
        MH_HIP(hipMemsetAsync(acc_shell, 0, nps * 8, c->stream));
        MH_HIP(hipMemsetAsync(acc_count, 0, ns * 8, c->stream));
    }

    // the per-frame regions of a block
    const size_t fb = Y.frame_block;
    char *WF = W + Y.off_frames;
    double *part = reinterpret_cast<double *>(WF);
    Cx *rho64 = reinterpret_cast<Cx *>(WF + fb * Y.sz_part);
    Real *stage = reinterpret_cast<Real *>(WF + fb * (Y.sz_part + Y.sz_rho));
    int32_t *bins = reinterpret_cast<int32_t *>(WF + fb * (Y.sz_part + Y.sz_rho + Y.sz_stage));
    double *spart = reinterpret_cast<double *>(WF + fb * (Y.sz_part + Y.sz_rho + Y.sz_stage + Y.sz_bins));
    u64 *cpart = reinterpret_cast<u64 *>(WF + fb * (Y.sz_part + Y.sz_rho + Y.sz_stage + Y.sz_bins + Y.sz_spart));

    Gram<Real> A{};
    A.frames = frames_d;
    A.stride = stride;
    A.inv = inv;
    A.atom = atom_d;
    A.w = w_d;
    A.items = Gr.items;
    A.nitems = Gr.nitems;
    A.S = S;
    A.part = part;
    A.items_cap = Y.items_cap;
    A.bad = bad;
    A.flags = flags;
    const ShellSpec SS{grid->qmin, grid->dq, (uint32_t)ns};
    const bool rho_dev = rho && is_device_ptr(rho);
    bool wait = false;
    if (shell_once) hipLaunchKernelGGL(sf_bins_kernel, dim3(blocks_of(Q), 1), dim3(SF_WG), 0, c->stream, inv, (size_t)0, S, SS, bins0);
    for (size_t f0 = 0; f0 < F; f0 += fb) {
        const uint32_t nf = (uint32_t)std::min<size_t>(fb, F - f0);
        A.f0 = f0;
        hipLaunchKernelGGL(sf_gram_kernel<Real>, dim3(Y.ntiles, Y.items_cap, nf), dim3(SF_WG), 0, c->stream, A);
        RhoOut<Real> O{nullptr, 0};
        if (rho_dev) O = RhoOut<Real>{rho + f0 * G * rho_stride, rho_stride};
        else if (rho) O = RhoOut<Real>{stage, 2 * Q};
        hipLaunchKernelGGL(sf_finish_kernel<Real>, dim3(blocks_of(GQ), nf), dim3(SF_WG), 0, c->stream, part, Y.items_cap, Gr.gitem, S, (uint32_t)G, f0, bad, rho64, O);
        if (rho && !rho_dev) {
            MH_HIP(hipMemcpy2DAsync(rho + f0 * G * rho_stride, rho_stride * sizeof(Real), stage, 2 * Q * sizeof(Real), 2 * Q * sizeof(Real), (size_t)nf * G,
                                    hipMemcpyDeviceToHost, c->stream));
            wait = true;
        }
        if (want_sab || rho_mean)
            hipLaunchKernelGGL(sf_products_kernel, dim3(blocks_of(PQ + GQ)), dim3(SF_WG), 0, c->stream, rho64, nf, f0, bad, (uint32_t)G, (uint32_t)Q, PQ,
                               want_sab ? acc_sab : nullptr, rho_mean ? acc_mean : nullptr);
        if (want_shell && !shell_once) {
            hipLaunchKernelGGL(sf_bins_kernel, dim3(blocks_of(Q), nf), dim3(SF_WG), 0, c->stream, inv, f0, S, SS, bins);
            hipLaunchKernelGGL(sf_shell_frame_kernel, dim3(blocks_of(nps), nf), dim3(SF_WG), 0, c->stream, rho64, bins, (uint32_t)G, (uint32_t)Q, (uint32_t)ns, nps,
                               spart, cpart);
            hipLaunchKernelGGL(sf_shell_fold_kernel, dim3(blocks_of(nps)), dim3(SF_WG), 0, c->stream, spart, cpart, nf, f0, bad, (uint32_t)ns, nps, acc_shell,
                               acc_count);
        }
        MH_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(sf_ok_kernel, dim3(1), dim3(SF_WG), 0, c->stream, bad, F, ok_d, fv);
    Real *out_sab = reinterpret_cast<Real *>(W + Y.off_out_sab), *out_mean = reinterpret_cast<Real *>(W + Y.off_out_mean);
    Real *out_shell = reinterpret_cast<Real *>(W + Y.off_out_shell);
    if (shell_once)
        hipLaunchKernelGGL(sf_shell_once_kernel, dim3(blocks_of(nps)), dim3(SF_WG), 0, c->stream, acc_sab, bins0, (uint32_t)Q, (uint32_t)ns, nps, fv, acc_shell, acc_count);
    if (sab) hipLaunchKernelGGL(sf_mean_kernel<Real>, dim3(blocks_of(PQ)), dim3(SF_WG), 0, c->stream, acc_sab, PQ, fv, out_sab);
    if (rho_mean)
        hipLaunchKernelGGL(sf_mean_kernel<Real>, dim3(blocks_of(2 * GQ)), dim3(SF_WG), 0, c->stream, reinterpret_cast<const double *>(acc_mean), 2 * GQ, fv, out_mean);
    if (want_shell && shell) hipLaunchKernelGGL(sf_shell_out_kernel<Real>, dim3(blocks_of(nps)), dim3(SF_WG), 0, c->stream, acc_shell, acc_count, (uint32_t)ns, nps, out_shell);
    MH_HIP(hipGetLastError());
    MH_TRY(copy_any(c, frame_ok, ok_d, F, wait));
    MH_TRY(copy_any(c, rho_mean, out_mean, 2 * GQ, wait));
    MH_TRY(copy_any(c, sab, out_sab, PQ, wait));
    if (want_shell) {
        MH_TRY(copy_any(c, shell, out_shell, nps, wait));
        MH_TRY(copy_any(c, reinterpret_cast<u64 *>(shell_count), acc_count, ns, wait));
    }
    return finish_copies(c, wait);
}

}  // namespace

namespace mh {
void sfactor_release(molar_hip_ctx *c) {
    release_state(c->sfactor);
}
}  // namespace mh

extern "C" {

int molar_hip_sfactor_plan(size_t nframes, size_t n, size_t ngroups, const molar_hip_sfactor_grid *grid, size_t *workspace_bytes, uint32_t *layout,
                           uint32_t *row_block, uint32_t *col_block, uint32_t *atom_chunk, uint32_t *ksplits, uint32_t *frame_block) {
    Shape S{};
    MH_TRY(make_shape("sfactor_plan", grid, &S));
    const size_t G = ngroups ? ngroups : 1;
    MH_TRY(check_sizes("sfactor_plan", G, S));
    const Layout Y = make_layout(nframes, n, G, S, grid->nshells);
    if (workspace_bytes) *workspace_bytes = (nframes == 0 || n == 0) ? 0 : Y.bytes;
    if (layout) *layout = S.layout;
    if (row_block) *row_block = SF_RB;
    if (col_block) *col_block = SF_CB;
    if (atom_chunk) *atom_chunk = Y.atom_chunk;
    if (ksplits) *ksplits = Y.ksplits;
    if (frame_block) *frame_block = Y.frame_block;
    return MOLAR_HIP_OK;
}

int molar_hip_sfactor(molar_hip_ctx *c, const float *frames, size_t nframes, size_t frame_stride, size_t natoms, const uint64_t *idx, size_t n,
                      const float *weight, const uint32_t *labels, size_t ngroups, const float *boxes, size_t box_stride,
                      const molar_hip_sfactor_grid *grid, float *rho, size_t rho_stride, uint32_t *frame_ok, float *rho_mean, float *sab, float *shell,
                      uint64_t *shell_count) {
    return sfactor_run<float>(c, "sfactor", frames, nframes, frame_stride, natoms, idx, n, weight, labels, ngroups, boxes, box_stride, grid, rho, rho_stride,
                              frame_ok, rho_mean, sab, shell, shell_count);
}

int molar_hip_sfactor_f64(molar_hip_ctx *c, const double *frames, size_t nframes, size_t frame_stride, size_t natoms, const uint64_t *idx, size_t n,
                          const double *weight, const uint32_t *labels, size_t ngroups, const double *boxes, size_t box_stride,
                          const molar_hip_sfactor_grid *grid, double *rho, size_t rho_stride, uint32_t *frame_ok, double *rho_mean, double *sab,
                          double *shell, uint64_t *shell_count) {
    return sfactor_run<double>(c, "sfactor_f64", frames, nframes, frame_stride, natoms, idx, n, weight, labels, ngroups, boxes, box_stride, grid, rho,
                               rho_stride, frame_ok, rho_mean, sab, shell, shell_count);
}

}  // extern "C"
