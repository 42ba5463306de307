// mindist.hip - minimum distances between two selections (or inside one) over a block of trajectory frames: the smallest
// distance of every frame and the pair that has it, for every atom its distance to the other set and its nearest atom there,
// the smallest distance between every pair of groups per frame, and the mean, the minimum and the contact frequency of that
// matrix over the valid frames.  The definition is in molar_hip.h.
//
// Every reduction is a minimum under a total order - (d2, i, j) for a pair, the bits of d2 for a value (a non-negative double
// orders as its bits) - so no result depends on the order of evaluation; the only atomics are 64-bit integer minima.  The
// metric is shortest_vector of boxmath.hpp itself: the orthorhombic path is that function with the terms dropped that are
// products with the zeros of a diagonal box and its inverse (they add +-0 to a sum and change no bit of a norm), so the value
// of a pair is bit-equal to what intcoord.hip forms for it on every path and no winner is recomputed.  shortest_vector is odd
// up to which of two candidates of equal norm it keeps, so d2(-v) = d2(v) to the bit: the pass that sees the pairs from set 2
// and the two halves of a matrix inside one set give the same bits.
//
// Stages, all on the context's stream:
//
//   boxes (one thread per box: box_from_matrix in double; a refused box marks its frames)
//   ->  prep: indices and labels judged, the atoms of every group counted (integer atomics)
//   ->  64 bytes read back: the status
//   ->  with labels: one stable radix sort of a set by label (devsort.hip), every group a contiguous run of sorted positions
//   ->  per block of frame_block frames:
//         gather (both sets as f64 structure-of-arrays in sorted order; a coordinate that is not finite marks the frame)
//         rows pass (a lane owns MD_R atoms of the row set, the atoms of the column set arrive by wave-uniform loads; per
//           column split the smallest (d2, column) of every row)  ->  row fold (the splits in order; atom1 / near1 or atom2)
//           ->  frame fold (one workgroup per frame: the smallest (d2, i, j))
//         groups pass (the same loop over the runs of the column groups; at the end of a run the lanes of one row group
//           take their minimum across the wave and its first lane issues one 64-bit atomicMin on the cell)
//           ->  time fold (one lane per cell walks the block's frames in order: mat, and the running sum, minimum, count)
//   ->  the valid frames, the mean.
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "boxmath.hpp"
#include "common.hpp"
#include "stages.hpp"
#include "traj_block.hpp"

using namespace mh;

struct molar_hip_mindist_state {
    DevBuf in_frames, in_idx1, in_idx2, in_labels1, in_labels2, in_boxes;   // host inputs staged here
    DevBuf sort_tmp;                                                      // scratch of the device sort
    DevBuf ws;                                                            // the workspace molar_hip_mindist_plan reports
};

namespace {

typedef unsigned long long u64;

constexpr uint32_t MD_WG = 256;                   // threads of every workgroup here
constexpr uint32_t MD_R = 2;                      // rows a lane owns
constexpr uint32_t MD_ROWS_WAVE = 64 * MD_R;      // rows per wave
constexpr uint32_t MD_ROWS_WG = MD_WG * MD_R;     // rows per workgroup
constexpr uint32_t MD_CT = 64;                    // columns per tile: a column split is a whole number of tiles
constexpr uint32_t MD_MAX_SPLITS = 64;
constexpr uint32_t MD_TARGET_WGS = 1024;          // column splits are added until a launch has this many workgroups
constexpr uint32_t MD_MAX_FRAMES = 256;           // frames per block at the most
constexpr size_t MD_FRAME_BYTES = (size_t)1 << 30;   // the per-frame regions of a block together, unless one frame's are larger
constexpr u64 MD_INF_BITS = 0x7FF0000000000000ull;
constexpr uint32_t MD_NONE = 0xFFFFFFFFu;

// flags[0]: an index not below natoms; [5]: a label not below its ngroups; [8]: a box that needs the general path
constexpr uint32_t MD_FLAG_WORDS = 16;

enum : uint32_t { OUT_DIST = 1u, OUT_ATOM1 = 2u, OUT_ATOM2 = 4u, OUT_MAT = 8u };

uint32_t env_u32(const char *name) {
    const char *e = std::getenv(name);
    if (!e || !*e) return 0u;
    const long v = std::strtol(e, nullptr, 10);
    return v > 0 && v < 0x40000000l ? (uint32_t)v : 0u;
}

size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

// Column splits of a pass over `rows` x `cols` with `frames` frames per launch, and the columns of a split.
struct ColSplits {
    uint32_t cper, splits;
};
ColSplits col_splits(size_t rows, size_t cols, size_t frames) {
    const size_t tiles = std::max<size_t>(1, (cols + MD_CT - 1) / MD_CT);
    const size_t have = std::max<size_t>(1, (rows + MD_ROWS_WG - 1) / MD_ROWS_WG) * std::max<size_t>(1, frames);
    size_t cs = (MD_TARGET_WGS + have - 1) / have;
    const uint32_t e = env_u32("MOLAR_HIP_MINDIST_COL_SPLITS");
    if (e) cs = e;
    cs = std::max<size_t>(1, std::min<size_t>(std::min<size_t>(cs, MD_MAX_SPLITS), tiles));
    const size_t tper = (tiles + cs - 1) / cs;
    return ColSplits{(uint32_t)(tper * MD_CT), (uint32_t)((tiles + tper - 1) / tper)};
}

// Where everything lives in the workspace, from the sizes alone (the plan entry and the call share it).
struct Layout {
    size_t n1, n2, G1, G2, cells;
    bool same, fwd, swp, groups;       // the passes: rows of set 1, rows of set 2, the group matrix
    ColSplits cs_fwd, cs_swp, cs_grp;
    uint32_t frame_block;
    size_t off_flags, off_boxes, off_boxbad, off_bad, off_ok, off_nv, off_cnt1, off_cnt2, off_gs1, off_gs2, off_iota, off_key1, off_key2, off_perm1,
        off_perm2, off_dist, off_pair, off_acc_sum, off_acc_min, off_acc_freq, off_out_mean, off_out_min, off_frames;
    size_t sz_x1, sz_x2, sz_pd2, sz_pj, sz_rd2, sz_rj, sz_mat, sz_s_atom, sz_s_near, sz_s_mat, per_frame;   // per frame, multiples of 256 bytes
    size_t bytes;
};

Layout make_layout(size_t F, size_t n1, size_t n2, size_t G1, size_t G2, bool same, uint32_t outputs, uint32_t frame_block) {
    Layout Y{};
    Y.same = same;
    Y.n1 = n1;
    Y.n2 = same ? n1 : n2;
    Y.G1 = G1;
    Y.G2 = same ? G1 : G2;
    Y.cells = Y.G1 * Y.G2;
    Y.swp = (outputs & OUT_ATOM2) != 0;
    Y.fwd = (outputs & OUT_ATOM1) != 0 || ((outputs & OUT_DIST) != 0 && !Y.swp);
    Y.groups = (outputs & OUT_MAT) != 0;
    const size_t launch = std::min<size_t>(std::max<size_t>(F, 1), MD_MAX_FRAMES);
    Y.cs_fwd = col_splits(Y.n1, Y.n2, launch);
    Y.cs_swp = col_splits(Y.n2, Y.n1, launch);
    Y.cs_grp = Y.cs_fwd;
    const size_t nmax = std::max(Y.n1, Y.n2);
    const size_t part = std::max(Y.fwd ? (size_t)Y.cs_fwd.splits * Y.n1 : 0, Y.swp ? (size_t)Y.cs_swp.splits * Y.n2 : 0);
    Y.sz_x1 = up256(3 * Y.n1 * 8);
    Y.sz_x2 = same ? 0 : up256(3 * Y.n2 * 8);
    Y.sz_pd2 = up256(part * 8);
    Y.sz_pj = up256(part * 4);
    Y.sz_rd2 = (Y.fwd || Y.swp) ? up256(nmax * 8) : 0;
    Y.sz_rj = (Y.fwd || Y.swp) ? up256(nmax * 4) : 0;
    Y.sz_mat = Y.groups ? up256(Y.cells * 8) : 0;
    Y.sz_s_atom = (Y.fwd || Y.swp) ? up256(nmax * 8) : 0;
    Y.sz_s_near = Y.fwd ? up256(Y.n1 * 8) : 0;
    Y.sz_s_mat = Y.groups ? up256(Y.cells * 8) : 0;
    Y.per_frame = Y.sz_x1 + Y.sz_x2 + Y.sz_pd2 + Y.sz_pj + Y.sz_rd2 + Y.sz_rj + Y.sz_mat + Y.sz_s_atom + Y.sz_s_near + Y.sz_s_mat;
    // min(F, frame_block) frames fit, and the region never shrinks when an argument grows
    size_t region = std::min(launch * Y.per_frame, std::max(MD_FRAME_BYTES, Y.per_frame));
    size_t fb = std::max<size_t>(1, std::min<size_t>(launch, Y.per_frame ? region / Y.per_frame : 1));
    uint32_t fb_ask = frame_block ? frame_block : env_u32("MOLAR_HIP_MINDIST_FRAME_BLOCK");
    if (fb_ask) {
        fb = std::max<size_t>(1, std::min<size_t>(std::min<size_t>(fb_ask, MD_MAX_FRAMES), std::max<size_t>(F, 1)));
        region = fb * Y.per_frame;
    }
    Y.frame_block = (uint32_t)fb;
    Carve ws;
    ws.take(Y.off_flags, MD_FLAG_WORDS * 4);
    ws.take(Y.off_boxes, F * sizeof(BoxD));
    ws.take(Y.off_boxbad, F * 4);
    ws.take(Y.off_bad, F * 4);
    ws.take(Y.off_ok, F * 4);
    ws.take(Y.off_nv, 16);
    ws.take(Y.off_cnt1, Y.G1 * 4);
    ws.take(Y.off_cnt2, Y.G2 * 4);
    ws.take(Y.off_gs1, (Y.G1 + 1) * 4);
    ws.take(Y.off_gs2, (Y.G2 + 1) * 4);
    ws.take(Y.off_iota, nmax * 4);
    ws.take(Y.off_key1, Y.n1 * 4);
    ws.take(Y.off_key2, Y.n2 * 4);
    ws.take(Y.off_perm1, Y.n1 * 4);
    ws.take(Y.off_perm2, Y.n2 * 4);
    ws.take(Y.off_dist, F * 8);
    ws.take(Y.off_pair, F * 16);
    ws.take(Y.off_acc_sum, Y.groups ? Y.cells * 8 : 0);
    ws.take(Y.off_acc_min, Y.groups ? Y.cells * 8 : 0);
    ws.take(Y.off_acc_freq, Y.groups ? Y.cells * 4 : 0);
    ws.take(Y.off_out_mean, Y.groups ? Y.cells * 8 : 0);
    ws.take(Y.off_out_min, Y.groups ? Y.cells * 8 : 0);
    ws.take(Y.off_frames, region);
    Y.bytes = ws.bytes;
    return Y;
}

// the sizes alone: what both the plan and the call refuse
int check_sizes(const char *who, size_t F, size_t n1, size_t n2, size_t G1, size_t G2) {
    if (n1 >= 0x7FFFFF00ull || n2 >= 0x7FFFFF00ull || F >= 0x7FFFFFF0ull) return fail(MOLAR_HIP_ERR_TOO_LARGE, "%s: 2^31 atoms or frames or more", who);
    if (G1 >= 0x7FFFFFFFull || G2 >= 0x7FFFFFFFull || G1 * G2 >= 0x7FFFFFFFull) return fail(MOLAR_HIP_ERR_TOO_LARGE, "%s: 2^31 cells (pairs of groups) or more", who);
    return 0;
}

int check_spec(const char *who, const molar_hip_mindist_spec *spec) {
    if (!spec) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: the spec is null", who);
    if (spec->pbc > 7u) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: pbc = %u is not a PbcDims mask", who, spec->pbc);
    if (spec->same > 1u || spec->exclude_same_group > 1u)
        return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: same = %u, exclude_same_group = %u are not 0 or 1", who, spec->same, spec->exclude_same_group);
    if (spec->exclude_same_group && !spec->same) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: exclude_same_group without same", who);
    if (std::isnan(spec->cutoff)) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: the cutoff is NaN", who);
    return 0;
}

// ---------------------------------------------------------------- small kernels

// One thread per box: PeriodicBox::from_matrix in double.  A refused box raises boxbad; a box that is not diagonal, or whose
// inverse is not, raises flags[8]: the orthorhombic path would not be shortest_vector for it.
template <class Real>
__global__ void __launch_bounds__(64) md_box_kernel(const Real *__restrict__ boxes, size_t nbox, BoxD *__restrict__ out, uint32_t *__restrict__ boxbad,
                                                    uint32_t *__restrict__ flags) {
    const size_t f = (size_t)blockIdx.x * 64u + threadIdx.x;
    if (f >= nbox) return;
    double m9[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) m9[q] = (double)boxes[f * 9 + q];
    const int bad = box_from_matrix_device(m9, out + f);
    boxbad[f] = bad ? 1u : 0u;
    if (bad) return;
    const BoxD &b = out[f];
    bool diag = b.nshift == 0;
    for (int q = 0; q < 9; ++q)
        if (q != 0 && q != 4 && q != 8 && !(b.m[q] == 0.0 && b.inv[q] == 0.0)) diag = false;
    if (!diag) flags[8] = 1u;
}

struct Sel {
    const uint64_t *idx;
    size_t n, natoms;
    const uint32_t *labels;
    uint32_t ngroups;
};

// Grid-stride over a selection: indices and labels judged, the atoms of every group counted.
__global__ void __launch_bounds__(MD_WG) md_prep_kernel(Sel P, uint32_t *__restrict__ cnt, uint32_t *__restrict__ flags) {
    const size_t step = (size_t)gridDim.x * MD_WG, t0 = (size_t)blockIdx.x * MD_WG + threadIdx.x;
    for (size_t k = t0; k < P.n; k += step) {
        if (P.idx && P.idx[k] >= P.natoms) flags[0] = 1u;
        if (P.labels) {
            const uint32_t g = P.labels[k];
            if (g >= P.ngroups) flags[5] = 1u;
            else atomicAdd(&cnt[g], 1u);
        }
    }
}

__global__ void __launch_bounds__(MD_WG) md_iota_kernel(uint32_t *__restrict__ iota, size_t n) {
    const size_t k = (size_t)blockIdx.x * MD_WG + threadIdx.x;
    if (k < n) iota[k] = (uint32_t)k;
}

// One thread: where every group starts among the sorted positions; gstart[G] = n.
__global__ void md_groups_start_kernel(const uint32_t *__restrict__ cnt, uint32_t G, uint32_t n, bool labelled, uint32_t *__restrict__ gstart) {
    uint32_t pos = 0;
    for (uint32_t g = 0; g < G; ++g) {
        gstart[g] = pos;
        pos += labelled ? cnt[g] : n;
    }
    gstart[G] = pos;
}

// A set of a block of frames as f64 structure-of-arrays x[frame][3][n] in sorted order; a coordinate that is not finite, or a
// refused box, marks the frame.
template <class Real>
__global__ void __launch_bounds__(MD_WG) md_gather_kernel(const Real *__restrict__ frames, size_t stride, size_t f0, const uint64_t *__restrict__ idx,
                                                          const uint32_t *__restrict__ perm, uint32_t n, double *__restrict__ x,
                                                          const uint32_t *__restrict__ boxbad, uint32_t box_step, uint32_t *__restrict__ bad) {
    const uint32_t s = blockIdx.x * MD_WG + threadIdx.x, fl = blockIdx.y;
    if (s >= n) return;
    const size_t f = f0 + fl;
    if (s == 0u && boxbad && boxbad[f * box_step]) bad[f] = 1u;
    const size_t k = perm ? perm[s] : s;
    const uint64_t a = idx ? idx[k] : (uint64_t)k;
    const Real *p = frames + f * stride + 3 * a;
    const double px = (double)p[0], py = (double)p[1], pz = (double)p[2];
    double *o = x + (size_t)fl * 3 * n + s;
    o[0] = px;
    o[n] = py;
    o[2 * (size_t)n] = pz;
    if (!(isfinite(px) && isfinite(py) && isfinite(pz))) bad[f] = 1u;
}

// ---------------------------------------------------------------- the pair passes

// MODE 0: the plain difference.  MODE 1: shortest_vector under a diagonal box with a diagonal inverse and a full mask, the
// zero terms dropped; MODE 3: the same under any mask (a dimension that is not periodic keeps its fractional coordinate:
// the rounded part times 0).  MODE 2: shortest_vector.
// In MODE 1 and 3 the fractional coordinate is rounded to nearest EVEN (one instruction) where shortest_vector rounds half
// away from zero (six).  The two differ only where the fraction is exactly one half; there f - round(f) is -1/2 by the one
// and +1/2 or -1/2 by the other, both exact, and the component m (f - round(f)) enters the result only squared: d2 has the
// same bits.
constexpr uint32_t MD_CHUNK = 8;     // columns whose coordinates are loaded together

template <int MODE>
__device__ __forceinline__ double pair_d2(const BoxD *__restrict__ box, uint32_t pbc, double px, double py, double pz, D3 v) {
    if constexpr (MODE == 0) {
        return norm2(v);
    } else if constexpr (MODE == 1) {
        double fx = box->inv[0] * v.x, fy = box->inv[4] * v.y, fz = box->inv[8] * v.z;
        fx -= __builtin_rint(fx);
        fy -= __builtin_rint(fy);
        fz -= __builtin_rint(fz);
        return norm2(D3{box->m[0] * fx, box->m[4] * fy, box->m[8] * fz});
    } else if constexpr (MODE == 3) {
        double fx = box->inv[0] * v.x, fy = box->inv[4] * v.y, fz = box->inv[8] * v.z;
        fx -= __builtin_rint(fx) * px;
        fy -= __builtin_rint(fy) * py;
        fz -= __builtin_rint(fz) * pz;
        return norm2(D3{box->m[0] * fx, box->m[4] * fy, box->m[8] * fz});
    } else {
        return norm2(shortest_vector(*box, v, pbc));
    }
}

struct Rows {
    uint32_t i[MD_R];       // sorted position, clamped to the set
    bool live[MD_R];
    D3 x[MD_R];
};

__device__ __forceinline__ Rows load_rows(const double *__restrict__ xr, uint32_t nr) {
    Rows R;
#pragma unroll
    for (uint32_t r = 0; r < MD_R; ++r) {
        const uint32_t i = blockIdx.x * MD_ROWS_WG + r * MD_WG + threadIdx.x;
        R.live[r] = i < nr;
        R.i[r] = R.live[r] ? i : nr - 1u;
        R.x[r] = D3{xr[R.i[r]], xr[(size_t)nr + R.i[r]], xr[2 * (size_t)nr + R.i[r]]};
    }
    return R;
}

// Rows pass.  Workgroup (x, y, z): rows x MD_ROWS_WG .. of the row set, column split y, frame z of the block.  The columns
// arrive by loads at wave-uniform addresses, MD_CHUNK at a time: the column operand of every instruction is a scalar register.
// part_d2 / part_j [frame][split][row]: the smallest d2 of the row over the split and the column that has it - its position
// in the caller's set (origc; LAB = false: the sorted position is that) - the lowest position among equal d2.
// SKIP: with same the column that is the row itself is skipped, with skip_groups so is every column of the row's group.
template <int MODE, bool LAB, bool SKIP>
__global__ void __launch_bounds__(MD_WG) md_rows_kernel(const double *__restrict__ xr_all, const double *__restrict__ xc_all, uint32_t nr, uint32_t nc,
                                                        const uint32_t *__restrict__ keyr, const uint32_t *__restrict__ keyc,
                                                        const uint32_t *__restrict__ origc, const BoxD *__restrict__ boxes, uint32_t box_step, size_t f0,
                                                        uint32_t pbc, uint32_t same, uint32_t skip_groups, uint32_t cper, double *__restrict__ part_d2,
                                                        uint32_t *__restrict__ part_j) {
    const uint32_t fl = blockIdx.z, split = blockIdx.y;
    const uint32_t c0 = split * cper, c1 = min(c0 + cper, nc);
    const double *__restrict__ xr = xr_all + (size_t)fl * 3 * nr;
    const double *__restrict__ xc = xc_all + (size_t)fl * 3 * nc;
    const double *__restrict__ yc = xc + nc;
    const double *__restrict__ zc = yc + nc;
    const BoxD *__restrict__ box = MODE ? boxes + (f0 + fl) * box_step : nullptr;
    const double px = (pbc & 1u) ? 1.0 : 0.0, py = (pbc & 2u) ? 1.0 : 0.0, pz = (pbc & 4u) ? 1.0 : 0.0;
    const Rows R = load_rows(xr, nr);
    uint32_t skip_i[MD_R], skip_lab[MD_R], bj[MD_R];
    double best[MD_R];
#pragma unroll
    for (uint32_t r = 0; r < MD_R; ++r) {
        skip_i[r] = same ? R.i[r] : MD_NONE;
        skip_lab[r] = skip_groups ? ((LAB && keyr) ? keyr[R.i[r]] : 0u) : MD_NONE;
        best[r] = __builtin_inf();
        bj[r] = MD_NONE;
    }
    auto column = [&](uint32_t j, D3 xj, uint32_t labj, uint32_t oj) {
#pragma unroll
        for (uint32_t r = 0; r < MD_R; ++r) {
            double d2 = pair_d2<MODE>(box, pbc, px, py, pz, xj - R.x[r]);
            if (SKIP && (j == skip_i[r] || labj == skip_lab[r])) d2 = __builtin_inf();
            const bool better = LAB ? (d2 < best[r] || (d2 == best[r] && oj < bj[r])) : d2 < best[r];
            best[r] = better ? d2 : best[r];
            bj[r] = better ? oj : bj[r];
        }
    };
    uint32_t j = c0;
    for (; j + MD_CHUNK <= c1; j += MD_CHUNK) {
        double cx[MD_CHUNK], cy[MD_CHUNK], cz[MD_CHUNK];
        uint32_t cl[MD_CHUNK], co[MD_CHUNK];
#pragma unroll
        for (uint32_t u = 0; u < MD_CHUNK; ++u) {
            cx[u] = xc[j + u];
            cy[u] = yc[j + u];
            cz[u] = zc[j + u];
            cl[u] = LAB ? keyc[j + u] : 0u;
            co[u] = LAB ? origc[j + u] : j + u;
        }
#pragma unroll
        for (uint32_t u = 0; u < MD_CHUNK; ++u) column(j + u, D3{cx[u], cy[u], cz[u]}, cl[u], co[u]);
    }
    for (; j < c1; ++j) column(j, D3{xc[j], yc[j], zc[j]}, LAB ? keyc[j] : 0u, LAB ? origc[j] : j);
#pragma unroll
    for (uint32_t r = 0; r < MD_R; ++r)
        if (R.live[r]) {
            const size_t o = ((size_t)fl * gridDim.y + split) * nr + R.i[r];
            part_d2[o] = best[r];
            part_j[o] = best[r] < __builtin_inf() ? bj[r] : MD_NONE;
        }
}

// Groups pass.  The same workgroups over the same loop, cut at the ends of the runs of the column groups (gsc[g] ..
// gsc[g + 1] are the sorted positions of column group g).  At the end of a run a lane holds the minimum of each of its rows
// over the run; row r of lane l is sorted position base + r MD_WG + l, so the rows of one group are runs of consecutive lanes:
// a segmented minimum over the wave (six steps, the links between lanes made once) leaves a group's minimum in its first
// lane, which issues one atomicMin on the bits of d2 in cell (row group, column group) of the frame.
template <int MODE>
__global__ void __launch_bounds__(MD_WG) md_groups_kernel(const double *__restrict__ xr_all, const double *__restrict__ xc_all, uint32_t nr, uint32_t nc,
                                                          const uint32_t *__restrict__ keyr, const uint32_t *__restrict__ keyc,
                                                          const uint32_t *__restrict__ gsc, uint32_t Gr, uint32_t Gc, const BoxD *__restrict__ boxes,
                                                          uint32_t box_step, size_t f0, uint32_t pbc, uint32_t same, uint32_t skip_groups, uint32_t cper,
                                                          u64 *mat) {
    const uint32_t fl = blockIdx.z, split = blockIdx.y, lane = threadIdx.x & 63u;
    const uint32_t c0 = split * cper, c1 = min(c0 + cper, nc);
    const double *__restrict__ xr = xr_all + (size_t)fl * 3 * nr;
    const double *__restrict__ xc = xc_all + (size_t)fl * 3 * nc;
    const double *__restrict__ yc = xc + nc;
    const double *__restrict__ zc = yc + nc;
    const BoxD *__restrict__ box = MODE ? boxes + (f0 + fl) * box_step : nullptr;
    const double px = (pbc & 1u) ? 1.0 : 0.0, py = (pbc & 2u) ? 1.0 : 0.0, pz = (pbc & 4u) ? 1.0 : 0.0;
    const Rows R = load_rows(xr, nr);
    uint32_t skip_i[MD_R], lab[MD_R], link[MD_R];
    bool head[MD_R];
#pragma unroll
    for (uint32_t r = 0; r < MD_R; ++r) {
        skip_i[r] = same ? R.i[r] : MD_NONE;
        lab[r] = R.live[r] ? (keyr ? keyr[R.i[r]] : 0u) : MD_NONE;
        link[r] = 0u;
#pragma unroll
        for (uint32_t k = 0; k < 6u; ++k) {
            const uint32_t other = __shfl_down(lab[r], 1u << k, 64);
            if (lane + (1u << k) < 64u && other == lab[r]) link[r] |= 1u << k;
        }
        const uint32_t before = __shfl_up(lab[r], 1u, 64);
        head[r] = lane == 0u || before != lab[r];
    }
    u64 *cells = mat + (size_t)fl * Gr * Gc;
    for (uint32_t g = keyc ? keyc[c0] : 0u; g < Gc; ++g) {
        const uint32_t gs = gsc[g], ge = gsc[g + 1u];
        if (gs >= c1) break;
        const uint32_t s = max(gs, c0), e = min(ge, c1);
        double m[MD_R];
#pragma unroll
        for (uint32_t r = 0; r < MD_R; ++r) m[r] = __builtin_inf();
        auto column = [&](uint32_t j, D3 xj) {
#pragma unroll
            for (uint32_t r = 0; r < MD_R; ++r) {
                double d2 = pair_d2<MODE>(box, pbc, px, py, pz, xj - R.x[r]);
                if (j == skip_i[r]) d2 = __builtin_inf();
                m[r] = d2 < m[r] ? d2 : m[r];
            }
        };
        uint32_t j = s;
        for (; j + MD_CHUNK <= e; j += MD_CHUNK) {
            double cx[MD_CHUNK], cy[MD_CHUNK], cz[MD_CHUNK];
#pragma unroll
            for (uint32_t u = 0; u < MD_CHUNK; ++u) {
                cx[u] = xc[j + u];
                cy[u] = yc[j + u];
                cz[u] = zc[j + u];
            }
#pragma unroll
            for (uint32_t u = 0; u < MD_CHUNK; ++u) column(j + u, D3{cx[u], cy[u], cz[u]});
        }
        for (; j < e; ++j) column(j, D3{xc[j], yc[j], zc[j]});
        if (s >= e) continue;
#pragma unroll
        for (uint32_t r = 0; r < MD_R; ++r) {
            double v = (skip_groups && lab[r] == g) ? __builtin_inf() : m[r];
#pragma unroll
            for (uint32_t k = 0; k < 6u; ++k) {
                const double other = __shfl_down(v, 1u << k, 64);
                if ((link[r] >> k) & 1u) v = other < v ? other : v;
            }
            if (head[r] && lab[r] != MD_NONE && v < __builtin_inf()) atomicMin(&cells[(size_t)lab[r] * Gc + g], (u64)__double_as_longlong(v));
        }
    }
}

// ---------------------------------------------------------------- folds

template <class Real>
__device__ __forceinline__ Real real_nan() {
    return (Real)__builtin_nan("");
}

// One lane per (frame of the block, sorted row): the column splits in order under (d2, column); the row's result goes to its
// position in the caller's set (origr; null: the sorted position): rd2 / rj for the frame fold, and the distance and the
// nearest atom to the outputs (null: not asked for).
template <class Real>
__global__ void __launch_bounds__(MD_WG) md_rowfold_kernel(const double *__restrict__ part_d2, const uint32_t *__restrict__ part_j, uint32_t splits, uint32_t nr,
                                                           const uint32_t *__restrict__ origr, const uint32_t *__restrict__ bad, size_t f0,
                                                           double *__restrict__ rd2, uint32_t *__restrict__ rj, Real *__restrict__ atom, size_t ld,
                                                           uint64_t *__restrict__ near, size_t ldn) {
    const uint32_t i = blockIdx.x * MD_WG + threadIdx.x, fl = blockIdx.y;
    if (i >= nr) return;
    double best = __builtin_inf();
    uint32_t bj = MD_NONE;
    for (uint32_t s = 0; s < splits; ++s) {
        const size_t o = ((size_t)fl * splits + s) * nr + i;
        const double d = part_d2[o];
        const uint32_t c = part_j[o];
        if (d < best || (d == best && c < bj)) {
            best = d;
            bj = c;
        }
    }
    const uint32_t o = origr ? origr[i] : i;
    rd2[(size_t)fl * nr + o] = best;
    rj[(size_t)fl * nr + o] = bj;
    const bool isbad = bad[f0 + fl] != 0u;
    if (atom) atom[fl * ld + o] = isbad ? real_nan<Real>() : (Real)sqrt(best);
    if (near) near[fl * ldn + o] = (isbad || bj == MD_NONE) ? ~(uint64_t)0 : (uint64_t)bj;
}

// One workgroup per frame of the block: the smallest (d2, i, j) over the rows; swapped: the rows are set 2, so a row's position
// is j and its nearest atom is i.
template <class Real>
__global__ void __launch_bounds__(MD_WG) md_framefold_kernel(const double *__restrict__ rd2, const uint32_t *__restrict__ rj, uint32_t nr, bool swapped,
                                                             const uint32_t *__restrict__ bad, size_t f0, Real *__restrict__ dist, uint64_t *__restrict__ pair) {
    __shared__ double sd[MD_WG];
    __shared__ uint32_t sa[MD_WG], sb[MD_WG];
    const uint32_t fl = blockIdx.x, t = threadIdx.x;
    double best = __builtin_inf();
    uint32_t ba = MD_NONE, bb = MD_NONE;
    auto take = [&](double d, uint32_t a, uint32_t b) {
        if (d < best || (d == best && (a < ba || (a == ba && b < bb)))) {
            best = d;
            ba = a;
            bb = b;
        }
    };
    for (uint32_t o = t; o < nr; o += MD_WG) {
        const double d = rd2[(size_t)fl * nr + o];
        const uint32_t c = rj[(size_t)fl * nr + o];
        if (c != MD_NONE) take(d, swapped ? c : o, swapped ? o : c);
    }
    sd[t] = best;
    sa[t] = ba;
    sb[t] = bb;
    __syncthreads();
    for (uint32_t w = MD_WG / 2; w > 0u; w >>= 1) {
        if (t < w) {
            take(sd[t + w], sa[t + w], sb[t + w]);
            sd[t] = best;
            sa[t] = ba;
            sb[t] = bb;
        }
        __syncthreads();
    }
    if (t == 0u) {
        const size_t f = f0 + fl;
        const bool isbad = bad[f] != 0u;
        if (dist) dist[f] = isbad ? real_nan<Real>() : (Real)sqrt(best);
        if (pair) {
            pair[2 * f] = (isbad || ba == MD_NONE) ? ~(uint64_t)0 : (uint64_t)ba;
            pair[2 * f + 1] = (isbad || ba == MD_NONE) ? ~(uint64_t)0 : (uint64_t)bb;
        }
    }
}

__global__ void __launch_bounds__(MD_WG) md_fill_u64_kernel(u64 *__restrict__ p, size_t count, u64 v) {
    const size_t i = (size_t)blockIdx.x * MD_WG + threadIdx.x;
    if (i < count) p[i] = v;
}

// One lane per cell: the frames of the block in order.  mat (null: not asked for) gets the frame's distance, NaN for a frame
// that is not valid; such a frame enters none of the running sum, minimum and count below the cutoff.
template <class Real>
__global__ void __launch_bounds__(MD_WG) md_timefold_kernel(const u64 *__restrict__ cells_all, size_t cells, uint32_t nf, size_t f0,
                                                            const uint32_t *__restrict__ bad, double cutoff, Real *__restrict__ mat,
                                                            double *__restrict__ acc_sum, double *__restrict__ acc_min, uint32_t *__restrict__ acc_freq) {
    const size_t i = (size_t)blockIdx.x * MD_WG + threadIdx.x;
    if (i >= cells) return;
    double s = acc_sum[i], mn = acc_min[i];
    uint32_t c = acc_freq[i];
    for (uint32_t fl = 0; fl < nf; ++fl) {
        const bool isbad = bad[f0 + fl] != 0u;
        const double d = sqrt(__longlong_as_double((long long)cells_all[(size_t)fl * cells + i]));
        if (mat) mat[(size_t)fl * cells + i] = isbad ? real_nan<Real>() : (Real)d;
        if (isbad) continue;
        s += d;
        mn = d < mn ? d : mn;
        c += d < cutoff ? 1u : 0u;
    }
    acc_sum[i] = s;
    acc_min[i] = mn;
    acc_freq[i] = c;
}

// The valid frames: ok[f] = 1 - bad[f], nv[0] = how many.
__global__ void __launch_bounds__(MD_WG) md_ok_kernel(const uint32_t *__restrict__ bad, size_t F, uint32_t *__restrict__ ok, u64 *__restrict__ nv) {
    __shared__ u64 sh;
    if (threadIdx.x == 0u) sh = 0;
    __syncthreads();
    u64 c = 0;
    for (size_t f = threadIdx.x; f < F; f += MD_WG) {
        const uint32_t o = bad[f] ? 0u : 1u;
        ok[f] = o;
        c += o;
    }
    if (c) atomicAdd(&sh, c);
    __syncthreads();
    if (threadIdx.x == 0u) nv[0] = sh;
}

// mean = sum / valid frames (NaN without one), and the minimum rounded to Real.
template <class Real>
__global__ void __launch_bounds__(MD_WG) md_finish_kernel(const double *__restrict__ acc_sum, const double *__restrict__ acc_min, size_t cells,
                                                          const u64 *__restrict__ nv, double *__restrict__ mean, Real *__restrict__ mn) {
    const size_t i = (size_t)blockIdx.x * MD_WG + threadIdx.x;
    if (i >= cells) return;
    mean[i] = nv[0] ? acc_sum[i] / (double)nv[0] : __builtin_nan("");
    mn[i] = (Real)acc_min[i];
}

int ceil_log2(size_t n) {
    int c = 0;
    while (c < 63 && ((size_t)1 << c) < n) ++c;
    return c;
}

template <class T>
int copy_any(molar_hip_ctx *c, T *dst, const T *dev, size_t count, bool &wait) {
    if (!dst || dst == dev) return 0;
    if (!is_device_ptr(dst)) wait = true;
    MH_HIP(hipMemcpyAsync(dst, dev, count * sizeof(T), hipMemcpyDefault, c->stream));
    return 0;
}

uint32_t blocks_of(size_t items) { return (uint32_t)((items + MD_WG - 1) / MD_WG); }

// One set after the prep: sorted labels, the permutation and the starts of the groups.
struct SetDev {
    const uint64_t *idx;
    const uint32_t *labels;      // as passed (device)
    uint32_t *cnt, *gstart, *key, *perm;
    uint32_t n, G;
    const uint32_t *keys() const { return labels ? key : nullptr; }
    const uint32_t *perms() const { return labels ? perm : nullptr; }
};

template <int MODE, bool LAB, bool SKIP>
void launch_rows_as(hipStream_t st, dim3 grid, const double *xr, const double *xc, const SetDev &R, const SetDev &Cs, const BoxD *boxes, uint32_t box_step, size_t f0,
                    const molar_hip_mindist_spec &sp, uint32_t cper, double *pd2, uint32_t *pj) {
    hipLaunchKernelGGL((md_rows_kernel<MODE, LAB, SKIP>), grid, dim3(MD_WG), 0, st, xr, xc, R.n, Cs.n, R.keys(), Cs.keys(), Cs.perms(), boxes, box_step, f0, sp.pbc,
                       sp.same, sp.exclude_same_group, cper, pd2, pj);
}
template <int MODE>
void launch_rows(hipStream_t st, dim3 grid, bool lab, bool skip, const double *xr, const double *xc, const SetDev &R, const SetDev &Cs, const BoxD *boxes,
                 uint32_t box_step, size_t f0, const molar_hip_mindist_spec &sp, uint32_t cper, double *pd2, uint32_t *pj) {
    if (lab && skip) launch_rows_as<MODE, true, true>(st, grid, xr, xc, R, Cs, boxes, box_step, f0, sp, cper, pd2, pj);
    else if (lab) launch_rows_as<MODE, true, false>(st, grid, xr, xc, R, Cs, boxes, box_step, f0, sp, cper, pd2, pj);
    else if (skip) launch_rows_as<MODE, false, true>(st, grid, xr, xc, R, Cs, boxes, box_step, f0, sp, cper, pd2, pj);
    else launch_rows_as<MODE, false, false>(st, grid, xr, xc, R, Cs, boxes, box_step, f0, sp, cper, pd2, pj);
}

template <class Real>
int mindist_run(molar_hip_ctx *c, const char *who, const Real *frames, size_t F, size_t stride, size_t natoms, const uint64_t *idx1, size_t n1,
                const uint32_t *labels1, size_t ngroups1, const uint64_t *idx2, size_t n2, const uint32_t *labels2, size_t ngroups2, const Real *boxes,
                size_t box_stride, const molar_hip_mindist_spec *spec, Real *dist, uint64_t *pair, Real *atom1, uint64_t *near1, size_t ld1, Real *atom2,
                size_t ld2, Real *mat, double *mat_mean, Real *mat_min, uint32_t *mat_freq, uint32_t *frame_ok, uint64_t *nvalid) {
    // the arguments are judged before the context is used
    if (!c) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "null context");
    MH_TRY(check_spec(who, spec));
    const molar_hip_mindist_spec sp = *spec;
    const bool same = sp.same != 0;
    if (same && (idx2 || labels2)) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: same = 1 with a second index or second labels", who);
    if (same && atom2) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: same = 1 with atom2 (it would be atom1)", who);
    if (same) {
        n2 = n1;
        ngroups2 = ngroups1;
    }
    if (n1 == 0 || n2 == 0) return fail(MOLAR_HIP_ERR_SIZES, "%s: an empty selection", who);
    if ((labels1 && ngroups1 == 0) || (labels2 && ngroups2 == 0)) return fail(MOLAR_HIP_ERR_SIZES, "%s: labels and ngroups = 0", who);
    const size_t G1 = labels1 ? ngroups1 : 1, G2 = same ? G1 : (labels2 ? ngroups2 : 1);
    if (box_stride != 0 && box_stride != 9) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: box_stride = %zu is neither 0 nor 9", who, box_stride);
    if (natoms == 0) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: selections out of natoms = 0", who);
    MH_TRY(check_no_index(who, "n1", idx1, n1, natoms));
    if (!same) MH_TRY(check_no_index(who, "n2", idx2, n2, natoms));
    MH_TRY(check_stride(who, "the frame stride", F, stride, natoms));
    if ((atom1 || near1) && F > 1 && ld1 < n1) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: ld1 = %zu is below n1 = %zu", who, ld1, n1);
    if (atom2 && F > 1 && ld2 < n2) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: ld2 = %zu is below n2 = %zu", who, ld2, n2);
    MH_TRY(check_sizes(who, F, n1, n2, G1, G2));
    const bool want_mat = mat || mat_mean || mat_min || mat_freq;
    const uint32_t outputs = ((dist || pair) ? OUT_DIST : 0u) | ((atom1 || near1) ? OUT_ATOM1 : 0u) | (atom2 ? OUT_ATOM2 : 0u) | (want_mat ? OUT_MAT : 0u);
    const Layout Y = make_layout(F, n1, n2, G1, G2, same, outputs, sp.frame_block);
    if (F == 0) return MOLAR_HIP_OK;
    if (!frames) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: the frames pointer is null", who);
    MH_TRY(check_index(who, "idx1", idx1, n1, natoms));
    MH_TRY(check_index(who, "idx2", idx2, n2, natoms));
    // labels in host memory are walked here; those in device memory are judged by the prep kernel before one is used as an address
    if (labels1 && !is_device_ptr(labels1))
        for (size_t k = 0; k < n1; ++k)
            if (labels1[k] >= G1) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: labels1[%zu] = %u is not below ngroups1 = %zu", who, k, labels1[k], G1);
    if (labels2 && !is_device_ptr(labels2))
        for (size_t k = 0; k < n2; ++k)
            if (labels2[k] >= G2) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: labels2[%zu] = %u is not below ngroups2 = %zu", who, k, labels2[k], G2);
    MH_HIP(hipSetDevice(c->device));

    molar_hip_mindist_state &Z = state_of(c->mindist);
    MH_TRY(grow_exact(Z.ws, Y.bytes, who, "the workspace"));
    char *W = Z.ws.as<char>();
    auto u32at = [&](size_t off) { return reinterpret_cast<uint32_t *>(W + off); };
    auto f64at = [&](size_t off) { return reinterpret_cast<double *>(W + off); };
    uint32_t *flags = u32at(Y.off_flags), *bad = u32at(Y.off_bad), *ok_d = u32at(Y.off_ok), *boxbad = u32at(Y.off_boxbad);
    u64 *nv = reinterpret_cast<u64 *>(W + Y.off_nv);
    BoxD *boxes64 = reinterpret_cast<BoxD *>(W + Y.off_boxes);

    const bool use_box = boxes != nullptr && sp.pbc != 0u;
    const size_t nbox = box_stride ? F : 1;
    const Real *frames_d = nullptr, *boxes_d = nullptr;
    SetDev S1{}, S2{};
    MH_TRY(to_device(c, frames, (F - 1) * stride + natoms * 3, Z.in_frames, &frames_d));
    MH_TRY(to_device(c, idx1, idx1 ? n1 : 0, Z.in_idx1, &S1.idx));
    MH_TRY(to_device(c, labels1, labels1 ? n1 : 0, Z.in_labels1, &S1.labels));
    MH_TRY(to_device(c, idx2, idx2 ? n2 : 0, Z.in_idx2, &S2.idx));
    MH_TRY(to_device(c, labels2, labels2 ? n2 : 0, Z.in_labels2, &S2.labels));
    if (use_box) MH_TRY(to_device(c, boxes, nbox * 9, Z.in_boxes, &boxes_d));
    S1.cnt = u32at(Y.off_cnt1);
    S1.gstart = u32at(Y.off_gs1);
    S1.key = u32at(Y.off_key1);
    S1.perm = u32at(Y.off_perm1);
    S1.n = (uint32_t)n1;
    S1.G = (uint32_t)G1;
    S2.cnt = u32at(Y.off_cnt2);
    S2.gstart = u32at(Y.off_gs2);
    S2.key = u32at(Y.off_key2);
    S2.perm = u32at(Y.off_perm2);
    S2.n = (uint32_t)n2;
    S2.G = (uint32_t)G2;
    if (same) S2 = S1;

    MH_HIP(hipMemsetAsync(flags, 0, MD_FLAG_WORDS * 4, c->stream));
    MH_HIP(hipMemsetAsync(S1.cnt, 0, G1 * 4, c->stream));
    if (!same) MH_HIP(hipMemsetAsync(S2.cnt, 0, G2 * 4, c->stream));
    if (use_box)
        hipLaunchKernelGGL(md_box_kernel<Real>, dim3((uint32_t)((nbox + 63) / 64)), dim3(64), 0, c->stream, boxes_d, nbox, boxes64, boxbad, flags);
    hipLaunchKernelGGL(md_prep_kernel, dim3(std::min<uint32_t>(blocks_of(n1), 1024u)), dim3(MD_WG), 0, c->stream, Sel{S1.idx, n1, natoms, S1.labels, (uint32_t)G1},
                       S1.cnt, flags);
    if (!same)
        hipLaunchKernelGGL(md_prep_kernel, dim3(std::min<uint32_t>(blocks_of(n2), 1024u)), dim3(MD_WG), 0, c->stream,
                           Sel{S2.idx, n2, natoms, S2.labels, (uint32_t)G2}, S2.cnt, flags);
    MH_HIP(hipGetLastError());
    // the one read-back: the status.  Nothing below runs, no index or label is used as an address and no output is touched after a bad argument.
    uint32_t hf[MD_FLAG_WORDS];
    MH_TRY(read_back(c, hf, flags, sizeof hf));
    if (hf[0]) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: a selection index is not below natoms = %zu", who, natoms);
    if (hf[5]) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: a label is not below its ngroups", who);
    const int mode = !use_box ? 0 : (hf[8] ? 2 : (sp.pbc == MOLAR_HIP_PBC_FULL ? 1 : 3));

    // the partition
    uint32_t *iota = u32at(Y.off_iota);
    if (S1.labels || S2.labels) hipLaunchKernelGGL(md_iota_kernel, dim3(blocks_of(std::max(n1, n2))), dim3(MD_WG), 0, c->stream, iota, std::max(n1, n2));
    if (S1.labels) MH_TRY(device_sort_pairs_u32(c->stream, Z.sort_tmp, S1.labels, S1.key, iota, S1.perm, n1, std::max(1, ceil_log2(G1))));
    if (!same && S2.labels) MH_TRY(device_sort_pairs_u32(c->stream, Z.sort_tmp, S2.labels, S2.key, iota, S2.perm, n2, std::max(1, ceil_log2(G2))));
    hipLaunchKernelGGL(md_groups_start_kernel, dim3(1), dim3(1), 0, c->stream, S1.cnt, (uint32_t)G1, (uint32_t)n1, S1.labels != nullptr, S1.gstart);
    if (!same) hipLaunchKernelGGL(md_groups_start_kernel, dim3(1), dim3(1), 0, c->stream, S2.cnt, (uint32_t)G2, (uint32_t)n2, S2.labels != nullptr, S2.gstart);

    const size_t cells = Y.cells;
    double *acc_sum = f64at(Y.off_acc_sum), *acc_min = f64at(Y.off_acc_min);
    uint32_t *acc_freq = u32at(Y.off_acc_freq);
    MH_HIP(hipMemsetAsync(bad, 0, F * 4, c->stream));
    if (want_mat) {
        MH_HIP(hipMemsetAsync(acc_sum, 0, cells * 8, c->stream));
        MH_HIP(hipMemsetAsync(acc_freq, 0, cells * 4, c->stream));
        hipLaunchKernelGGL(md_fill_u64_kernel, dim3(blocks_of(cells)), dim3(MD_WG), 0, c->stream, reinterpret_cast<u64 *>(acc_min), cells, MD_INF_BITS);
    }

    // the per-frame regions of a block
    const size_t fb = Y.frame_block;
    char *q = W + Y.off_frames;
    auto region = [&](size_t per) {
        char *p = q;
        q += fb * per;
        return p;
    };
    double *x1 = reinterpret_cast<double *>(region(Y.sz_x1));
    double *x2 = same ? x1 : reinterpret_cast<double *>(region(Y.sz_x2));
    double *pd2 = reinterpret_cast<double *>(region(Y.sz_pd2));
    uint32_t *pj = reinterpret_cast<uint32_t *>(region(Y.sz_pj));
    double *rd2 = reinterpret_cast<double *>(region(Y.sz_rd2));
    uint32_t *rj = reinterpret_cast<uint32_t *>(region(Y.sz_rj));
    u64 *matblk = reinterpret_cast<u64 *>(region(Y.sz_mat));
    Real *s_atom = reinterpret_cast<Real *>(region(Y.sz_s_atom));
    uint64_t *s_near = reinterpret_cast<uint64_t *>(region(Y.sz_s_near));
    Real *s_mat = reinterpret_cast<Real *>(region(Y.sz_s_mat));

    // whole-block results: in place when the destination is device memory
    Real *dist_w = reinterpret_cast<Real *>(W + Y.off_dist);
    uint64_t *pair_w = reinterpret_cast<uint64_t *>(W + Y.off_pair);
    Real *dist_d = dist ? (is_device_ptr(dist) ? dist : dist_w) : nullptr;
    uint64_t *pair_d = pair ? (is_device_ptr(pair) ? pair : pair_w) : nullptr;
    const bool atom1_dev = atom1 && is_device_ptr(atom1), near1_dev = near1 && is_device_ptr(near1), atom2_dev = atom2 && is_device_ptr(atom2);
    const bool mat_dev = mat && is_device_ptr(mat);
    const BoxD *bx = use_box ? boxes64 : nullptr;
    const uint32_t box_step = box_stride ? 1u : 0u;
    const bool lab_fwd = S2.labels != nullptr, lab_swp = S1.labels != nullptr;
    bool wait = false;
    auto rows_pass = [&](dim3 grid, bool lab, const double *xr, const double *xc, const SetDev &R, const SetDev &Cs, size_t f0, uint32_t cper) {
        if (mode == 0) launch_rows<0>(c->stream, grid, lab, same, xr, xc, R, Cs, bx, box_step, f0, sp, cper, pd2, pj);
        else if (mode == 1) launch_rows<1>(c->stream, grid, lab, same, xr, xc, R, Cs, bx, box_step, f0, sp, cper, pd2, pj);
        else if (mode == 3) launch_rows<3>(c->stream, grid, lab, same, xr, xc, R, Cs, bx, box_step, f0, sp, cper, pd2, pj);
        else launch_rows<2>(c->stream, grid, lab, same, xr, xc, R, Cs, bx, box_step, f0, sp, cper, pd2, pj);
    };
    for (size_t f0 = 0; f0 < F; f0 += fb) {
        const uint32_t nf = (uint32_t)std::min<size_t>(fb, F - f0);
        hipLaunchKernelGGL(md_gather_kernel<Real>, dim3(blocks_of(n1), nf), dim3(MD_WG), 0, c->stream, frames_d, stride, f0, S1.idx, S1.perms(), (uint32_t)n1, x1,
                           use_box ? boxbad : nullptr, box_step, bad);
        if (!same)
            hipLaunchKernelGGL(md_gather_kernel<Real>, dim3(blocks_of(n2), nf), dim3(MD_WG), 0, c->stream, frames_d, stride, f0, S2.idx, S2.perms(), (uint32_t)n2,
                               x2, (const uint32_t *)nullptr, box_step, bad);
        if (Y.fwd) {
            const dim3 grid((uint32_t)((n1 + MD_ROWS_WG - 1) / MD_ROWS_WG), Y.cs_fwd.splits, nf);
            rows_pass(grid, lab_fwd, x1, x2, S1, S2, f0, Y.cs_fwd.cper);
            Real *a_out = atom1 ? (atom1_dev ? atom1 + f0 * ld1 : s_atom) : nullptr;
            uint64_t *n_out = near1 ? (near1_dev ? near1 + f0 * ld1 : s_near) : nullptr;
            hipLaunchKernelGGL(md_rowfold_kernel<Real>, dim3(blocks_of(n1), nf), dim3(MD_WG), 0, c->stream, pd2, pj, Y.cs_fwd.splits, (uint32_t)n1, S1.perms(), bad, f0,
                               rd2, rj, a_out, atom1_dev ? ld1 : n1, n_out, near1_dev ? ld1 : n1);
            if (dist_d || pair_d)
                hipLaunchKernelGGL(md_framefold_kernel<Real>, dim3(nf), dim3(MD_WG), 0, c->stream, rd2, rj, (uint32_t)n1, false, bad, f0, dist_d, pair_d);
            if (atom1 && !atom1_dev) {
                MH_HIP(hipMemcpy2DAsync(atom1 + f0 * ld1, ld1 * sizeof(Real), s_atom, n1 * sizeof(Real), n1 * sizeof(Real), nf, hipMemcpyDeviceToHost, c->stream));
                wait = true;
            }
            if (near1 && !near1_dev) {
                MH_HIP(hipMemcpy2DAsync(near1 + f0 * ld1, ld1 * 8, s_near, n1 * 8, n1 * 8, nf, hipMemcpyDeviceToHost, c->stream));
                wait = true;
            }
        }
        if (Y.swp) {
            const dim3 grid((uint32_t)((n2 + MD_ROWS_WG - 1) / MD_ROWS_WG), Y.cs_swp.splits, nf);
            rows_pass(grid, lab_swp, x2, x1, S2, S1, f0, Y.cs_swp.cper);
            Real *a_out = atom2_dev ? atom2 + f0 * ld2 : s_atom;
            hipLaunchKernelGGL(md_rowfold_kernel<Real>, dim3(blocks_of(n2), nf), dim3(MD_WG), 0, c->stream, pd2, pj, Y.cs_swp.splits, (uint32_t)n2, S2.perms(), bad, f0,
                               rd2, rj, a_out, atom2_dev ? ld2 : n2, (uint64_t *)nullptr, (size_t)0);
            if (!Y.fwd && (dist_d || pair_d))
                hipLaunchKernelGGL(md_framefold_kernel<Real>, dim3(nf), dim3(MD_WG), 0, c->stream, rd2, rj, (uint32_t)n2, true, bad, f0, dist_d, pair_d);
            if (!atom2_dev) {
                MH_HIP(hipMemcpy2DAsync(atom2 + f0 * ld2, ld2 * sizeof(Real), s_atom, n2 * sizeof(Real), n2 * sizeof(Real), nf, hipMemcpyDeviceToHost, c->stream));
                wait = true;
            }
        }
        if (want_mat) {
            hipLaunchKernelGGL(md_fill_u64_kernel, dim3(blocks_of((size_t)nf * cells)), dim3(MD_WG), 0, c->stream, matblk, (size_t)nf * cells, MD_INF_BITS);
            const dim3 grid((uint32_t)((n1 + MD_ROWS_WG - 1) / MD_ROWS_WG), Y.cs_grp.splits, nf);
#define MD_GROUPS(M)                                                                                                                                          \
    hipLaunchKernelGGL(md_groups_kernel<M>, grid, dim3(MD_WG), 0, c->stream, x1, x2, (uint32_t)n1, (uint32_t)n2, S1.keys(), S2.keys(), S2.gstart, (uint32_t)G1, \
                       (uint32_t)G2, bx, box_step, f0, sp.pbc, sp.same, sp.exclude_same_group, Y.cs_grp.cper, matblk)
            if (mode == 0) MD_GROUPS(0);
            else if (mode == 1) MD_GROUPS(1);
            else if (mode == 3) MD_GROUPS(3);
            else MD_GROUPS(2);
#undef MD_GROUPS
            Real *m_out = mat ? (mat_dev ? mat + f0 * cells : s_mat) : nullptr;
            hipLaunchKernelGGL(md_timefold_kernel<Real>, dim3(blocks_of(cells)), dim3(MD_WG), 0, c->stream, matblk, cells, nf, f0, bad, sp.cutoff, m_out, acc_sum, acc_min,
                               acc_freq);
            if (mat && !mat_dev) {
                MH_HIP(hipMemcpyAsync(mat + f0 * cells, s_mat, (size_t)nf * cells * sizeof(Real), hipMemcpyDeviceToHost, c->stream));
                wait = true;
            }
        }
        MH_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(md_ok_kernel, dim3(1), dim3(MD_WG), 0, c->stream, bad, F, ok_d, nv);
    double *out_mean = f64at(Y.off_out_mean);
    Real *out_min = reinterpret_cast<Real *>(W + Y.off_out_min);
    if (want_mat) hipLaunchKernelGGL(md_finish_kernel<Real>, dim3(blocks_of(cells)), dim3(MD_WG), 0, c->stream, acc_sum, acc_min, cells, nv, out_mean, out_min);
    MH_HIP(hipGetLastError());
    MH_TRY(copy_any(c, dist, dist_d, F, wait));
    MH_TRY(copy_any(c, pair, pair_d, 2 * F, wait));
    MH_TRY(copy_any(c, frame_ok, ok_d, F, wait));
    MH_TRY(copy_any(c, reinterpret_cast<u64 *>(nvalid), nv, 1, wait));
    if (want_mat) {
        MH_TRY(copy_any(c, mat_mean, out_mean, cells, wait));
        MH_TRY(copy_any(c, mat_min, out_min, cells, wait));
        MH_TRY(copy_any(c, mat_freq, acc_freq, cells, wait));
    }
    return finish_copies(c, wait);
}

}  // namespace

namespace mh {
void mindist_release(molar_hip_ctx *c) {
    release_state(c->mindist);
}
}  // namespace mh

extern "C" {

int molar_hip_mindist_plan(size_t nframes, size_t n1, size_t n2, size_t ngroups1, size_t ngroups2, const molar_hip_mindist_spec *spec, uint32_t outputs,
                           size_t *workspace_bytes, uint32_t *rows_per_wave, uint32_t *rows_per_block, uint32_t *cols_per_tile, uint32_t *col_splits,
                           uint32_t *frame_block) {
    MH_TRY(check_spec("mindist_plan", spec));
    if (outputs > 15u) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "mindist_plan: outputs = %u holds a bit that names no output", outputs);
    const bool same = spec->same != 0;
    const size_t G1 = ngroups1 ? ngroups1 : 1, G2 = same ? G1 : (ngroups2 ? ngroups2 : 1);
    if (same) n2 = n1;
    MH_TRY(check_sizes("mindist_plan", nframes, n1, n2, G1, G2));
    const Layout Y = make_layout(nframes, n1, n2, G1, G2, same, outputs, spec->frame_block);
    if (workspace_bytes) *workspace_bytes = (nframes == 0 || n1 == 0 || n2 == 0) ? 0 : Y.bytes;
    if (rows_per_wave) *rows_per_wave = MD_ROWS_WAVE;
    if (rows_per_block) *rows_per_block = MD_ROWS_WG;
    if (cols_per_tile) *cols_per_tile = MD_CT;
    if (col_splits) *col_splits = (Y.swp && !Y.fwd) ? Y.cs_swp.splits : Y.cs_fwd.splits;
    if (frame_block) *frame_block = Y.frame_block;
    return MOLAR_HIP_OK;
}

int molar_hip_mindist(molar_hip_ctx *c, const float *frames, size_t nframes, size_t frame_stride, size_t natoms, const uint64_t *idx1, size_t n1,
                      const uint32_t *labels1, size_t ngroups1, const uint64_t *idx2, size_t n2, const uint32_t *labels2, size_t ngroups2, const float *boxes,
                      size_t box_stride, const molar_hip_mindist_spec *spec, float *dist, uint64_t *pair, float *atom1, uint64_t *near1, size_t ld1, float *atom2,
                      size_t ld2, float *mat, double *mat_mean, float *mat_min, uint32_t *mat_freq, uint32_t *frame_ok, uint64_t *nvalid) {
    return mindist_run<float>(c, "mindist", frames, nframes, frame_stride, natoms, idx1, n1, labels1, ngroups1, idx2, n2, labels2, ngroups2, boxes, box_stride, spec,
                              dist, pair, atom1, near1, ld1, atom2, ld2, mat, mat_mean, mat_min, mat_freq, frame_ok, nvalid);
}

int molar_hip_mindist_f64(molar_hip_ctx *c, const double *frames, size_t nframes, size_t frame_stride, size_t natoms, const uint64_t *idx1, size_t n1,
                          const uint32_t *labels1, size_t ngroups1, const uint64_t *idx2, size_t n2, const uint32_t *labels2, size_t ngroups2,
                          const double *boxes, size_t box_stride, const molar_hip_mindist_spec *spec, double *dist, uint64_t *pair, double *atom1, uint64_t *near1,
                          size_t ld1, double *atom2, size_t ld2, double *mat, double *mat_mean, double *mat_min, uint32_t *mat_freq, uint32_t *frame_ok,
                          uint64_t *nvalid) {
    return mindist_run<double>(c, "mindist_f64", frames, nframes, frame_stride, natoms, idx1, n1, labels1, ngroups1, idx2, n2, labels2, ngroups2, boxes, box_stride,
                               spec, dist, pair, atom1, near1, ld1, atom2, ld2, mat, mat_mean, mat_min, mat_freq, frame_ok, nvalid);
}

}  // extern "C"
