// search_f64.hip - the eight distance_search drivers for MolAR built with its `f64` feature (Float = f64:
// molar/src/aliases.rs:10-13, molar/Cargo.toml:56-60), correct before fast.
//
// The f32 search (search.hip, pair_kernels.hpp) is the tuned product path; an f64 build of MolAR flips `Float` for the
// whole crate including distance_search, so results there are decided by f64 arithmetic: which cell an atom near a cell
// face lands in, which pairs at the cutoff are hits, and the distances themselves.  This file restates the drivers once
// more with every operation in double:
//   * inputs are used where they lie if they are device memory (staged otherwise); grid dims on the host from the box or
//     from a zero-seeded bounding box reduced on the device (distance_search.rs:103-110, 602-646);
//   * populate / populate_pbc (drop rule, wrap, later-dimension quirk, :120-210) per selected atom on the device; the
//     reference's push order - in-box atoms of a cell before its wrapped atoms, each in selection order - is a STABLE radix
//     sort (rocPRIM) by the key 2 * cell + wrapped; cell starts by binary search; the 14-mask plan, its scan and one record
//     per 64-row slot by small kernels (:217-269).  Three small read-backs (vdW radii maximum / bounding box, number of
//     slots, number of results);
//   * one 64-lane wave per slot evaluates the exact f64 predicate - plain |p2 - p1|^2 or PeriodicBox::distance_squared
//     (periodic_box.rs:286-318) for entries across the periodic boundary - with the second cell's atoms resident in
//     registers (up to 256 of them; larger cells chunk by chunk from memory) and the rows handed round with v_readlane:
//     first to count, then, behind an exclusive scan of the slot counts, to write (i, j, sqrt(d2)) at its place of the
//     reference's output order (plan order, then i-major / j-minor, :949-953);
//   * records are 24-byte positions + 8-byte ids; results are (usize, usize, f64) columns or usize ids (within).
//   * the fused histogram (molar_hip_search_histogram_f64) walks the same slots in one persistent kernel that bins every
//     hit's d2 in LDS instead of writing it (hist64_kernel).
//   * `within` as a set (molar_hip_within_count_f64 / _fill_f64) needs no slots: the plan is inverted into per-cell partner
//     lists and one wave per (first cell, 64-row block) walks them with a mask of the rows still looking; found rows set a flag,
//     the ascending flagged ids are the set (within64_flags_kernel, csr_kernels.hpp).  Not here: the kernel for small second
//     sets walked from the inner selection's side and the grid hold of the f32 form (within.hip) - tunings, f32 only.
//   * SearchConnectivity (molar_hip_search_connectivity_f64) and unwrap_connectivity (molar_hip_unwrap_connectivity_f64): the
//     single-selection search into the context's columns, the CSR by one stable sort as in f32 (filled by
//     molar_hip_search_connectivity_fill), the stack walk on the host by the template both precisions use (unwrap_walk.hpp).
// 1M atoms, rc 1.0 nm, 2.1e8 results, frame and result resident: see tools/bench_search_f64.py, profiles/r05_search_f64.jsonl.
// tests/test_gpu_search_f64.py compares all eight drivers bit for bit with the f64 build of the CPU checker.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "boxmath.hpp"
#include "common.hpp"
#include "csr_kernels.hpp"
#include "hoststream.hpp"
#include "search_core.hpp"
#include "stages.hpp"
#include "unwrap_walk.hpp"

using namespace mh;

struct molar_hip_search64_state {
    int kind = 0;
    uint64_t dims[3] = {1, 1, 1};
    uint64_t total = 0;
    uint32_t nslots = 0;
    bool have = false;
    bool use_box = false;
    uint8_t pbc = 0;
    double cutoff = 0.0;
    double prune_limit2 = 0.0; // (cutoff + margin)^2: rows of wrapped entries farther than this from the second cell's image box are skipped
    DevBuf aabbA, aabbB;       // per cell: lo[3], hi[3] of its items
    bool approx = false;       // wrapped entries classified by the distance to the adjacent image (count and fill alike)
    double band_lo = 1.0, band_hi = 1.0;
    DevBuf posA, idA, vdwA, posB, idB, vdwB, slots, slot_cnt, slot_base, box, out_i, out_j, out_d;
    // device pipeline of the grid and the plan
    DevBuf in_xyz[2], in_idx[2], in_vdw[2];      // staging of host inputs
    DevBuf key_in, key_out, val_in, val_out, pos3, startA, startB, task_ns, task_first, cub_tmp, partial, flags;
    // fused histogram (molar_hip_search_histogram_f64): bin edges of the last range, [bins of a host-bins call][pair count],
    // the slot counter of the persistent kernel
    DevBuf hedges, hsum, hnext;
    std::vector<double> h_edges;
    double edges_min = 0.0, edges_max = 0.0;
    size_t edges_n = 0;
    int occ_key = -1, occ_blocks = 0;    // workgroups per CU of the last (kernel, LDS size) launched
    // `within` as a set (molar_hip_within_count_f64 / _fill_f64): per first-set cell the second-set cells its plan entries
    // meet, one flag byte per id, the flags counted per tile of 2048 and the scan of those counts
    DevBuf w_part_cnt, w_part, w_flags, w_tile_cnt, w_tile_off, w_out;
    uint64_t w_nflags = 0, w_total = 0;
    bool have_within = false;
};

namespace {

// MASK of distance_search.rs:39-60
__constant__ uint8_t MASKS64[14][6] = {
    {0, 0, 0, 0, 0, 0},
    {0, 0, 0, 1, 0, 0}, {0, 0, 0, 0, 1, 0}, {0, 0, 0, 0, 0, 1},
    {0, 0, 0, 1, 1, 0}, {0, 0, 0, 1, 0, 1}, {0, 0, 0, 0, 1, 1},
    {0, 0, 0, 1, 1, 1},
    {1, 0, 0, 0, 1, 0}, {1, 0, 0, 0, 0, 1}, {0, 1, 0, 0, 0, 1},
    {1, 1, 0, 0, 0, 1}, {1, 0, 1, 0, 1, 0}, {0, 1, 1, 1, 0, 0},
};

// Rust `as usize` / `as isize` on f64: saturating, NaN -> 0
MH_HD uint64_t as_usize(double x) {
    if (!(x > 0.0)) return 0;
    if (x >= 18446744073709551615.0) return ~0ull;
    return (uint64_t)x;
}
MH_HD int64_t as_isize(double x) {
    if (x != x) return 0;
    if (x >= 9223372036854775807.0) return INT64_MAX;
    if (x <= -9223372036854775808.0) return INT64_MIN;
    return (int64_t)x;
}

struct Slot64 {                    // what a wave needs for one 64-row slot
    uint32_t a0, rows, i0, b0, n2, flags;     // flags: wrap | tri << 8
    uint32_t cb, pad1;                         // cb: the second cell (its bounding box prunes rows)
};

// one set of the search as the caller gave it (device addresses)
struct SetIn {
    const double *xyz;
    const unsigned long long *idx;     // NULL: all atoms
    const double *vdw;                 // per SELECTED atom, or NULL
    uint64_t natoms;
    uint32_t nsel;
    int ids_local;
};
struct GridP {
    BoxD box;
    int use_box;
    uint32_t pbc;
    uint32_t dims[3];
    uint32_t ncells;
    double lower[3], upper[3];
};

// Grid::populate (:120-142) / populate_pbc (:144-210) for one selected atom: its cell, whether it was wrapped (the reference
// pushes the atoms found inside the box first, the wrapped ones after them, :180, :203-209) and the position stored with it.
// Sort key = 2 * cell + wrapped; dropped atoms get the key 2 * ncells.
__global__ void __launch_bounds__(256) assign64_kernel(SetIn S, GridP G, uint32_t *__restrict__ key, uint32_t *__restrict__ val,
                                                       double *__restrict__ pos3, int *__restrict__ err) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= S.nsel) return;
    val[k] = k;
    const uint64_t a = S.idx ? S.idx[k] : (uint64_t)k;
    const uint32_t dropped = 2u * G.ncells;
    if (a >= S.natoms) {
        *err = 1;
        key[k] = dropped;
        return;
    }
    const double p[3] = {S.xyz[3 * a], S.xyz[3 * a + 1], S.xyz[3 * a + 2]};
    double q[3] = {p[0], p[1], p[2]};
    uint64_t loc[3] = {0, 0, 0};
    uint32_t phase = 0;
    if (!G.use_box) {
        bool ok = true;
        for (int d = 0; d < 3; ++d) {
            const double dim_sz = G.upper[d] - G.lower[d];
            const int64_t nn = as_isize(floor((double)G.dims[d] * (p[d] - G.lower[d]) / dim_sz));    // :131
            if (nn < 0 || nn >= (int64_t)G.dims[d]) { ok = false; break; }
            loc[d] = (uint64_t)nn;
        }
        if (!ok) {
            key[k] = dropped;
            return;
        }
    } else {
        const D3 rel = mat_vec(G.box.inv, D3{p[0], p[1], p[2]});                             // :156
        double r[3] = {rel.x, rel.y, rel.z};
        bool correct = true, drop = false;
        for (int d = 0; d < 3; ++d)                                                          // :161-171
            if (r[d] < 0.0 || r[d] >= 1.0) {
                if (!((G.pbc >> d) & 1u)) { drop = true; break; }
                correct = false;
                break;
            }
        if (drop) {
            key[k] = dropped;
            return;
        }
        if (!correct) {                                                                      // :181-199
            for (int d = 0; d < 3; ++d)
                if ((G.pbc >> d) & 1u) {
                    r[d] = r[d] - trunc(r[d]);                                               // fract()
                    if (r[d] < 0.0) r[d] = 1.0 + r[d];
                }
            const D3 w = mat_vec(G.box.m, D3{r[0], r[1], r[2]});                              // :196
            q[0] = w.x; q[1] = w.y; q[2] = w.z;
            phase = 1;
        }
        for (int d = 0; d < 3; ++d) {
            uint64_t l = as_usize(floor(r[d] * (double)G.dims[d]));                          // :175, :191
            if (l > G.dims[d] - 1u) l = G.dims[d] - 1u;
            loc[d] = l;
        }
    }
    const uint32_t cell = (uint32_t)(loc[0] + loc[1] * G.dims[0] + loc[2] * (uint64_t)G.dims[0] * G.dims[1]);
    key[k] = 2u * cell + phase;
    pos3[3 * (size_t)k] = q[0];
    pos3[3 * (size_t)k + 1] = q[1];
    pos3[3 * (size_t)k + 2] = q[2];
}

// the grid's items in the reference's push order (the radix sort is stable: equal keys keep the selection's order)
__global__ void __launch_bounds__(256) gather64_kernel(SetIn S, uint32_t n, uint32_t ncells, const uint32_t *__restrict__ key_sorted,
                                                       const uint32_t *__restrict__ val_sorted, const double *__restrict__ pos3,
                                                       double *__restrict__ pos, unsigned long long *__restrict__ id,
                                                       double *__restrict__ vdw) {
    const uint32_t s = blockIdx.x * 256u + threadIdx.x;
    if (s >= n || key_sorted[s] >= 2u * ncells) return;
    const uint32_t k = val_sorted[s];
    pos[3 * (size_t)s] = pos3[3 * (size_t)k];
    pos[3 * (size_t)s + 1] = pos3[3 * (size_t)k + 1];
    pos[3 * (size_t)s + 2] = pos3[3 * (size_t)k + 2];
    id[s] = S.ids_local ? (unsigned long long)k : (S.idx ? S.idx[k] : (unsigned long long)k);
    if (vdw) vdw[s] = S.vdw[k];
}

// start[c] = first sorted item with key >= 2 c, c = 0 .. ncells (start[ncells] = items kept)
__global__ void __launch_bounds__(256) cellstart64_kernel(const uint32_t *__restrict__ key_sorted, uint32_t n, uint32_t ncells,
                                                          uint32_t *__restrict__ start) {
    const uint32_t c = blockIdx.x * 256u + threadIdx.x;
    if (c > ncells) return;
    const uint32_t want = 2u * c;
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (key_sorted[mid] < want) lo = mid + 1;
        else hi = mid;
    }
    start[c] = lo;
}

// bounding box of every cell's items (row pruning of the pair kernels): one wave per cell
__global__ void __launch_bounds__(256) aabb64_kernel(const uint32_t *__restrict__ start, uint32_t ncells, const double *__restrict__ pos,
                                                     double *__restrict__ aabb) {
    const uint32_t c = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (c >= ncells) return;
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (uint32_t k = start[c] + lane; k < start[c + 1]; k += 64u)
        for (int d = 0; d < 3; ++d) {
            const double v = pos[3 * (size_t)k + d];
            lo[d] = fmin(lo[d], v);
            hi[d] = fmax(hi[d], v);
        }
    for (int d = 0; d < 3; ++d)
        for (int off = 32; off > 0; off >>= 1) {
            lo[d] = fmin(lo[d], __shfl_xor(lo[d], off, 64));
            hi[d] = fmax(hi[d], __shfl_xor(hi[d], off, 64));
        }
    if (lane == 0)
        for (int d = 0; d < 3; ++d) { aabb[6 * (size_t)c + d] = lo[d]; aabb[6 * (size_t)c + 3 + d] = hi[d]; }
}

// compute_min_max (:602-616, seeded with zeros) over the selected atoms: per-workgroup partials {lo[3], hi[3]}
__global__ void __launch_bounds__(256) minmax64_kernel(SetIn S, double *__restrict__ partial, int *__restrict__ err) {
    double lo[3] = {0.0, 0.0, 0.0}, hi[3] = {0.0, 0.0, 0.0};
    for (uint32_t k = blockIdx.x * 256u + threadIdx.x; k < S.nsel; k += gridDim.x * 256u) {
        const uint64_t a = S.idx ? S.idx[k] : (uint64_t)k;
        if (a >= S.natoms) { *err = 1; continue; }
        for (int d = 0; d < 3; ++d) {
            const double v = S.xyz[3 * a + d];
            if (v < lo[d]) lo[d] = v;
            if (v > hi[d]) hi[d] = v;
        }
    }
    __shared__ double sh[4][6];
    for (int d = 0; d < 3; ++d)
        for (int off = 32; off > 0; off >>= 1) {
            const double l2 = __shfl_xor(lo[d], off, 64), h2 = __shfl_xor(hi[d], off, 64);
            if (l2 < lo[d]) lo[d] = l2;
            if (h2 > hi[d]) hi[d] = h2;
        }
    if ((threadIdx.x & 63u) == 0u)
        for (int d = 0; d < 3; ++d) { sh[threadIdx.x >> 6][d] = lo[d]; sh[threadIdx.x >> 6][3 + d] = hi[d]; }
    __syncthreads();
    if (threadIdx.x < 6u) {
        double v = sh[0][threadIdx.x];
        for (int w = 1; w < 4; ++w) {
            const double o = sh[w][threadIdx.x];
            if (threadIdx.x < 3u ? o < v : o > v) v = o;
        }
        partial[6 * blockIdx.x + threadIdx.x] = v;
    }
}

// Iterator::reduce(Float::max) over the radii (:781-783): NaN-ignoring max; per-workgroup partials (NaN where a workgroup saw
// only NaNs or nothing)
__global__ void __launch_bounds__(256) fmax64_kernel(const double *__restrict__ v, uint32_t n, double *__restrict__ partial) {
    double m = __builtin_nan("");
    for (uint32_t k = blockIdx.x * 256u + threadIdx.x; k < n; k += gridDim.x * 256u) m = fmax(m, v[k]);
    for (int off = 32; off > 0; off >>= 1) m = fmax(m, __shfl_xor(m, off, 64));
    __shared__ double sh[4];
    if ((threadIdx.x & 63u) == 0u) sh[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = fmax(fmax(sh[0], sh[1]), fmax(sh[2], sh[3]));
}

// search_plan (:217-269): element t of the plan in the reference's loop order - x outer, z inner, the 14 masks, and for two
// sets (pair.0, pair.1) then (pair.1, pair.0) - as (first cell, second cell, wrap | tri << 8), or first == 0xFFFFFFFF
struct Entry64 {
    uint32_t ca, cb, flags;
};
__device__ __forceinline__ Entry64 plan_entry(const GridP &G, uint64_t t, uint32_t mult) {
    const uint32_t half = (uint32_t)(t % mult);
    const uint64_t tm = t / mult;
    const uint32_t m = (uint32_t)(tm % 14u);
    const uint64_t cs = tm / 14u;
    const uint32_t z = (uint32_t)(cs % G.dims[2]), y = (uint32_t)((cs / G.dims[2]) % G.dims[1]), x = (uint32_t)(cs / ((uint64_t)G.dims[2] * G.dims[1]));
    uint32_t cc[2][3] = {{x + MASKS64[m][0], y + MASKS64[m][1], z + MASKS64[m][2]}, {x + MASKS64[m][3], y + MASKS64[m][4], z + MASKS64[m][5]}};
    uint32_t wrap = 0, wrapped[2] = {0u, 0u};             // dims in which the first / the second listed cell went round
    for (int i = 0; i < 2; ++i)
        for (int d = 0; d < 3; ++d)
            if (cc[i][d] == G.dims[d]) {
                if ((G.pbc >> d) & 1u) { cc[i][d] = 0; wrap |= 1u << d; wrapped[i] |= 1u << d; }
                else return Entry64{0xFFFFFFFFu, 0u, 0u};                                    // :241-244
            }
    const uint32_t i1 = cc[0][0] + cc[0][1] * G.dims[0] + cc[0][2] * G.dims[0] * G.dims[1];
    const uint32_t i2 = cc[1][0] + cc[1][1] * G.dims[0] + cc[1][2] * G.dims[0] * G.dims[1];
    // bits 12-14: the dims in which the entry's SECOND (column) cell is the one that went round
    if (mult == 1u) return Entry64{i1, i2, wrap | (i1 == i2 ? 0x100u : 0u) | (wrapped[1] << 12)};   // :432-517
    // (pair.0, pair.1) then (pair.1, pair.0): rows are always atoms of the FIRST set (:686-693)
    return half ? Entry64{i2, i1, wrap | (wrapped[0] << 12)} : Entry64{i1, i2, wrap | (wrapped[1] << 12)};
}

__global__ void __launch_bounds__(256) plan64_kernel(GridP G, uint64_t ntasks, uint32_t mult, const uint32_t *__restrict__ startA,
                                                     const uint32_t *__restrict__ startB, uint32_t *__restrict__ task_ns) {
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (t > ntasks) return;
    uint32_t ns = 0;
    if (t < ntasks) {
        const Entry64 e = plan_entry(G, t, mult);
        if (e.ca != 0xFFFFFFFFu) {
            const uint32_t n1 = startA[e.ca + 1] - startA[e.ca], n2 = startB[e.cb + 1] - startB[e.cb];
            if (n1 && n2) ns = (n1 + 63u) / 64u;
        }
    }
    task_ns[t] = ns;                                   // task_ns[ntasks] = 0: its scan is the number of slots
}

__global__ void __launch_bounds__(256) slots64_kernel(GridP G, uint64_t ntasks, uint32_t mult, const uint32_t *__restrict__ startA,
                                                      const uint32_t *__restrict__ startB, const uint32_t *__restrict__ task_first,
                                                      Slot64 *__restrict__ slots) {
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (t >= ntasks) return;
    const uint32_t first = task_first[t], ns = task_first[t + 1] - first;
    if (!ns) return;
    const Entry64 e = plan_entry(G, t, mult);
    const uint32_t n1 = startA[e.ca + 1] - startA[e.ca], n2 = startB[e.cb + 1] - startB[e.cb];
    for (uint32_t q = 0; q < ns; ++q) {
        Slot64 s{};
        s.a0 = startA[e.ca];
        s.i0 = q * 64u;
        s.rows = n1 - s.i0 < 64u ? n1 - s.i0 : 64u;
        s.b0 = startB[e.cb];
        s.n2 = n2;
        s.flags = e.flags;
        s.cb = e.cb;
        slots[first + q] = s;
    }
}

struct Params64 {
    const double *posA, *posB, *vdwA, *vdwB;
    const unsigned long long *idA, *idB;
    const BoxD *box;
    const Slot64 *slots;
    uint32_t nslots;
    int kind;
    int use_box;
    double cutoff2;
    // entries across the periodic boundary: classify with the plain distance to the second cell's adjacent image and decide
    // with PeriodicBox::distance_squared only inside [band_lo, band_hi] * cutoff^2 (see molar_hip_search_count_f64)
    int approx_wrapped;
    double band_lo, band_hi;
    const double *aabbB;      // per cell of the second grid: lo[3], hi[3]
    double prune_limit2;
};

// squared distance of one candidate: plain (:488) or PeriodicBox::distance_squared for an entry that wrapped (:485-486)
__device__ __forceinline__ double pair_d2(const Params64 &P, uint32_t wrap, D3 a, D3 b) {
    const D3 v = b - a;                                                                      // p2 - p1
    if (P.use_box && wrap) return norm2(shortest_vector(*P.box, v, wrap));
    return norm2(v);
}

__device__ __forceinline__ double lane_bcast(double v, uint32_t r) {      // lane r's value in every lane (r uniform)
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), (int)r), hi = __builtin_amdgcn_readlane(__double2hiint(v), (int)r);
    return __hiloint2double(hi, lo);
}

// One 64-row slot whose second cell fits NCH chunks of 64 atoms: the second cell's atoms stay in registers (one per lane and
// chunk), the slot's rows are loaded once (one per lane) and handed round with v_readlane - no memory access in the row loop.
// Same predicate, same order of operations and of results as the generic loop below.
// Output queue of a wave in LDS (fill pass): hits are pushed in order as (i, j, d2) and written 64 at a time - one 512-byte
// block per column, naturally aligned after the slot's first flush (which only goes up to the next 64-entry boundary of the
// output) - with the square roots taken for 64 lanes at once.
struct Fifo64 {
    unsigned long long *fi, *fj;
    double *fd;
    uint32_t head, tail, quota;
};
constexpr uint32_t FIFO64_CAP = 128;

__device__ __forceinline__ void fifo64_flush(Fifo64 &F, uint32_t count, uint32_t lane, unsigned long long off,
                                             unsigned long long *__restrict__ out_i, unsigned long long *__restrict__ out_j,
                                             double *__restrict__ out_d) {
    if (lane < count) {
        const uint32_t sl = (F.head + lane) & (FIFO64_CAP - 1u);
        const unsigned long long at = off + F.head + lane;
        __builtin_nontemporal_store(F.fi[sl], &out_i[at]);
        __builtin_nontemporal_store(F.fj[sl], &out_j[at]);
        __builtin_nontemporal_store(sqrt(F.fd[sl]), &out_d[at]);                  // d2.sqrt() (:448)
    }
    F.head += count;
}

// The fused histogram (hist64_kernel): a hit's d2 goes into the workgroup's 32-bit LDS counters, at the largest b with edges[b]
// <= d2 (histogram_edges64: the formula's own table over d2), found from an f32 estimate corrected step by step against the edges.
struct Hist64 {
    uint32_t *hist;                  // the workgroup's counters (LDS)
    const double *edges;             // nbins + 1 edges: LDS copy or global memory
    unsigned long long *bins;
    uint32_t nbins;
    float hmin, scale, hn;           // the f32 estimate: (sqrt(d2) - hmin) * scale, clamped to [0, n]
};

__device__ __forceinline__ void hist64_add(const Hist64 &H, double d2) {
    float est = (__builtin_amdgcn_sqrtf((float)d2) - H.hmin) * H.scale;
    est = __builtin_fminf(__builtin_fmaxf(est, 0.0f), H.hn);                // also sends a NaN to 0
    int b = (int)est;
    while (b < (int)H.nbins && H.edges[b + 1] <= d2) ++b;
    while (b >= 0 && H.edges[b] > d2) --b;
    if ((uint32_t)b < H.nbins) __hip_atomic_fetch_add(H.hist + b, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// the workgroup's counters into the bins by one wave, beside the others still counting
__device__ __forceinline__ void hist64_flush(const Hist64 &H, uint32_t lane) {
    for (uint32_t b = lane; b < H.nbins; b += 64u) {
        const uint32_t v = __hip_atomic_exchange(H.hist + b, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (v) atomicAdd(H.bins + b, (unsigned long long)v);
    }
}

// What a slot's walk does with a hit: counts it, writes it - (i, j, sqrt(d2)), or the row's id for the within stream - or
// bins its d2.  Writing and binning need the hit's exact d2: they decide every band-classified candidate inside the band's
// upper edge by PeriodicBox::distance_squared, so a binned d2 is exactly the d2 whose square root the fill pass writes.
// The arguments a mode does not use (F and the output columns when binning, H otherwise) are dead after inlining.
enum { RUN_COUNT = 0, RUN_FILL = 1, RUN_HIST = 2 };

template <int MODE, int KIND, int NCH>
__device__ __forceinline__ uint32_t run64(const Params64 &P, const Slot64 &S, uint32_t lane, unsigned long long off,
                                          unsigned long long *__restrict__ out_i, unsigned long long *__restrict__ out_j,
                                          double *__restrict__ out_d, Fifo64 F, const Hist64 &H) {
    const uint32_t wrap = S.flags & 7u;
    const bool tri = (S.flags >> 8) & 1u;
    constexpr bool VDW = KIND == MOLAR_HIP_SEARCH_DOUBLE_VDW, WITHIN = KIND == MOLAR_HIP_SEARCH_WITHIN;
    constexpr bool FILL = MODE == RUN_FILL, HIST = MODE == RUN_HIST, EXACT = FILL || HIST;
    static_assert(!(HIST && WITHIN), "the histogram bins pairs; the within stream has none");
    double bx[NCH], by[NCH], bz[NCH], bv[NCH];
    unsigned long long bid[NCH];
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
        const uint32_t j = (uint32_t)k * 64u + lane;
        bx[k] = by[k] = bz[k] = bv[k] = 0.0;
        bid[k] = 0ull;
        if (j < S.n2) {
            const size_t rb = (size_t)S.b0 + j;
            bx[k] = P.posB[3 * rb]; by[k] = P.posB[3 * rb + 1]; bz[k] = P.posB[3 * rb + 2];
            if (VDW) bv[k] = P.vdwB[rb];
            if (FILL && !WITHIN) bid[k] = P.idB[rb];
        }
    }
    F.head = F.tail = 0u;
    F.quota = 64u - ((uint32_t)off & 63u);
    // b + S is the image of the second cell next to the first one (second cell went round: + box vector, first cell: -)
    const bool approx = P.approx_wrapped && P.use_box && wrap != 0u && !(P.box->nshift != 0 && wrap == MOLAR_HIP_PBC_FULL);
    double cx[NCH], cy[NCH], cz[NCH];
    double Sx = 0.0, Sy = 0.0, Sz = 0.0;
    if (approx) {
        for (int d = 0; d < 3; ++d) {
            if (!((wrap >> d) & 1u)) continue;
            const double sgn = ((S.flags >> (12 + d)) & 1u) ? 1.0 : -1.0;
            Sx += sgn * P.box->m[3 * d];
            Sy += sgn * P.box->m[3 * d + 1];
            Sz += sgn * P.box->m[3 * d + 2];
        }
#pragma unroll
        for (int k = 0; k < NCH; ++k) { cx[k] = bx[k] + Sx; cy[k] = by[k] + Sy; cz[k] = bz[k] + Sz; }
    }
    double ax = 0.0, ay = 0.0, az = 0.0, av = 0.0;
    unsigned long long aid = 0ull;
    if (lane < S.rows) {
        const size_t ra = (size_t)S.a0 + S.i0 + lane;
        ax = P.posA[3 * ra]; ay = P.posA[3 * ra + 1]; az = P.posA[3 * ra + 2];
        if (VDW) av = P.vdwA[ra];
        if (FILL) aid = P.idA[ra];
    }
    // Rows that cannot have a hit.  Every position of the second cell lies inside the cell's bounding box [lo, hi], and each
    // f64 operation of d2 = ((dx*dx)+(dy*dy))+(dz*dz) is monotone in |dx|, |dy|, |dz|: the same expression on the distances to
    // the box is a lower bound of every d2 of the row IN f64 ARITHMETIC (vdW: against the largest pair cutoff).  Entries
    // classified by the adjacent image: against the image box with the margin of the band; other wrapped entries: no pruning.
    unsigned long long live;
    {
        bool need = lane < S.rows;
        if (!tri && (wrap == 0u || !P.use_box || approx)) {
            const double *bb = P.aabbB + 6 * (size_t)S.cb;
            double px = ax, py = ay, pz = az, lim = P.cutoff2;
            if (approx) {
                px = ax - Sx;
                py = ay - Sy;
                pz = az - Sz;
                lim = P.prune_limit2;
            }
            const double ex = fmax(fmax(bb[0] - px, px - bb[3]), 0.0), ey = fmax(fmax(bb[1] - py, py - bb[4]), 0.0),
                         ez = fmax(fmax(bb[2] - pz, pz - bb[5]), 0.0);
            need = need && !((ex * ex + ey * ey) + ez * ez > lim);
        }
        live = __builtin_amdgcn_ballot_w64(need);
    }
    uint32_t acc = 0, total = 0;
    while (live) {
        const uint32_t r = (uint32_t)__builtin_ctzll(live);
        live &= live - 1ull;
        const D3 a = D3{lane_bcast(ax, r), lane_bcast(ay, r), lane_bcast(az, r)};
        const double vdw_a = VDW ? lane_bcast(av, r) : 0.0;
        const uint32_t i = S.i0 + r;
        unsigned long long idr = 0ull;
        if (FILL && !WITHIN)
            idr = ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(aid >> 32), (int)r) << 32) |
                  (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)aid, (int)r);
        bool any = false;
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
            if (tri && (uint32_t)k * 64u + 63u <= i) continue;                  // the whole chunk has j <= i (:443)
            const uint32_t j = (uint32_t)k * 64u + lane;
            bool hit = j < S.n2 && !(tri && j <= i);
            double cut2 = P.cutoff2;
            if (VDW) {
                const double cut = (vdw_a + bv[k]) + 2.220446049250313e-16;    // :392, :423
                cut2 = cut * cut;
            }
            double d2;
            if (approx) {
                const double ex = cx[k] - a.x, ey = cy[k] - a.y, ez = cz[k] - a.z;
                const double q2 = (ex * ex + ey * ey) + ez * ez;
                const bool sure = q2 < cut2 * P.band_lo, maybe = hit && q2 <= cut2 * P.band_hi;
                d2 = q2;
                // hits carry the reference's own distance; candidates inside the band are decided by it
                if (__builtin_amdgcn_ballot_w64(maybe && (EXACT || !sure))) {
                    if (maybe && (EXACT || !sure)) d2 = pair_d2(P, wrap, a, D3{bx[k], by[k], bz[k]});
                }
                hit = maybe && (sure || d2 <= cut2);
            } else {
                d2 = pair_d2(P, wrap, a, D3{bx[k], by[k], bz[k]});
                hit = hit && d2 <= cut2;
            }
            if (WITHIN) {
                any = any || hit;
            } else if (HIST) {
                const unsigned long long m = __builtin_amdgcn_ballot_w64(hit);
                if (!m) continue;
                total += (uint32_t)__popcll(m);
                if (hit) hist64_add(H, d2);
            } else if (!FILL) {
                acc += hit ? 1u : 0u;
            } else {
                const unsigned long long m = __builtin_amdgcn_ballot_w64(hit);
                if (!m) continue;
                if (hit) {
                    const uint32_t sl = (F.tail + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u))) & (FIFO64_CAP - 1u);
                    F.fi[sl] = idr;
                    F.fj[sl] = bid[k];
                    F.fd[sl] = d2;
                }
                F.tail += (uint32_t)__popcll(m);
                if (F.tail - F.head >= 64u) {
                    __builtin_amdgcn_wave_barrier();
                    do {
                        fifo64_flush(F, F.quota, lane, off, out_i, out_j, out_d);
                        F.quota = 64u;
                    } while (F.tail - F.head >= 64u);
                    __builtin_amdgcn_wave_barrier();
                }
            }
        }
        if (WITHIN && __builtin_amdgcn_ballot_w64(any)) {                       // the row's first hit only (:287-290)
            if (FILL && lane == 0) out_i[off] = P.idA[(size_t)S.a0 + S.i0 + r];
            off += 1;
            total += 1;
        }
    }
    if (MODE == RUN_COUNT && !WITHIN) {
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
        total = acc;
    }
    if (FILL && !WITHIN && F.tail != F.head) {
        __builtin_amdgcn_wave_barrier();
        fifo64_flush(F, F.tail - F.head, lane, off, out_i, out_j, out_d);
    }
    return total;
}

// second cells of more than 256 atoms: pair64_kernel's chunk loop with the hits binned (see there why it is a copy)
template <int KIND>
__device__ __forceinline__ unsigned long long hist64_chunks(const Params64 &P, const Slot64 &S, uint32_t lane, const Hist64 &H,
                                                            uint32_t &since_flush, uint32_t flush_at) {
    const uint32_t wrap = S.flags & 7u;
    const bool tri = (S.flags >> 8) & 1u;
    unsigned long long total = 0;
    for (uint32_t r = 0; r < S.rows; ++r) {
        const uint32_t ra = S.a0 + S.i0 + r;
        const D3 a = D3{P.posA[3 * ra], P.posA[3 * ra + 1], P.posA[3 * ra + 2]};
        const double vdw_a = (KIND == MOLAR_HIP_SEARCH_DOUBLE_VDW) ? P.vdwA[ra] : 0.0;
        for (uint32_t j0 = 0; j0 < S.n2; j0 += 64u) {
            const uint32_t j = j0 + lane;
            bool hit = false;
            double d2 = 0.0;
            if (j < S.n2 && !(tri && j <= S.i0 + r)) {            // same cell: j in i+1..n (:443)
                const uint32_t rb = S.b0 + j;
                d2 = pair_d2(P, wrap, a, D3{P.posB[3 * rb], P.posB[3 * rb + 1], P.posB[3 * rb + 2]});
                if (KIND == MOLAR_HIP_SEARCH_DOUBLE_VDW) {
                    const double cut = (vdw_a + P.vdwB[rb]) + 2.220446049250313e-16;        // :392, :423
                    hit = d2 <= cut * cut;
                } else {
                    hit = d2 <= P.cutoff2;
                }
            }
            const unsigned long long m = __builtin_amdgcn_ballot_w64(hit);
            if (!m) continue;
            const uint32_t cnt = (uint32_t)__popcll(m);
            total += cnt;
            if (hit) hist64_add(H, d2);
            since_flush += cnt;
            if (since_flush > flush_at) {
                hist64_flush(H, lane);
                since_flush = 0;
            }
        }
    }
    return total;
}

template <bool FILL, int KIND>
__global__ void __launch_bounds__(64) pair64_kernel(Params64 P, uint32_t *__restrict__ slot_cnt,
                                                    const unsigned long long *__restrict__ slot_base,
                                                    unsigned long long *__restrict__ out_i, unsigned long long *__restrict__ out_j,
                                                    double *__restrict__ out_d) {
    const uint32_t s = blockIdx.y * gridDim.x + blockIdx.x;
    if (s >= P.nslots) return;
    const Slot64 S = P.slots[s];
    const uint32_t lane = threadIdx.x;
    const uint32_t wrap = S.flags & 7u;
    const bool tri = (S.flags >> 8) & 1u;
    unsigned long long off = FILL ? slot_base[s] : 0ull;
    const uint32_t nch = (S.n2 + 63u) >> 6;
    constexpr int MODE = FILL ? RUN_FILL : RUN_COUNT;
    constexpr uint32_t QN = (FILL && KIND != MOLAR_HIP_SEARCH_WITHIN) ? FIFO64_CAP : 1u;
    __shared__ unsigned long long q_i[QN], q_j[QN];
    __shared__ double q_d[QN];
    if (nch <= 4u) {
        uint32_t t;
        const Hist64 H{};                              // binning only
        const Fifo64 F{q_i, q_j, q_d, 0u, 0u, 64u};
        switch (nch) {
            case 1: t = run64<MODE, KIND, 1>(P, S, lane, off, out_i, out_j, out_d, F, H); break;
            case 2: t = run64<MODE, KIND, 2>(P, S, lane, off, out_i, out_j, out_d, F, H); break;
            case 3: t = run64<MODE, KIND, 3>(P, S, lane, off, out_i, out_j, out_d, F, H); break;
            default: t = run64<MODE, KIND, 4>(P, S, lane, off, out_i, out_j, out_d, F, H); break;
        }
        if (!FILL && lane == 0) slot_cnt[s] = t;
        return;
    }
    // Second cells of more than 256 atoms: chunk by chunk from memory; rows are atoms of the first set's grid, columns of the
    // second set's (the same for SINGLE).  hist64_chunks is this loop with binning: as ONE function template the two reordered
    // every pair64_kernel's scalar prologue (7-16 instructions more, one 20 fewer), which wants a timing before it is adopted.
    const double *pa = P.posA, *pb = P.posB;
    const unsigned long long *ia = P.idA, *ib = P.idB;
    const double *va = P.vdwA, *vb = P.vdwB;
    uint32_t total = 0;
    for (uint32_t r = 0; r < S.rows; ++r) {
        const uint32_t ra = S.a0 + S.i0 + r;
        const D3 a = D3{pa[3 * ra], pa[3 * ra + 1], pa[3 * ra + 2]};
        const double vdw_a = (KIND == MOLAR_HIP_SEARCH_DOUBLE_VDW) ? va[ra] : 0.0;
        bool found = false;                                       // WITHIN: first hit of the row only (:287-290)
        for (uint32_t j0 = 0; j0 < S.n2 && !found; j0 += 64u) {
            const uint32_t j = j0 + lane;
            bool hit = false;
            double d2 = 0.0;
            if (j < S.n2 && !(tri && j <= S.i0 + r)) {            // same cell: j in i+1..n (:443)
                const uint32_t rb = S.b0 + j;
                d2 = pair_d2(P, wrap, a, D3{pb[3 * rb], pb[3 * rb + 1], pb[3 * rb + 2]});
                if (KIND == MOLAR_HIP_SEARCH_DOUBLE_VDW) {
                    const double cut = (vdw_a + vb[rb]) + 2.220446049250313e-16;        // :392, :423
                    hit = d2 <= cut * cut;
                } else {
                    hit = d2 <= P.cutoff2;
                }
            }
            const unsigned long long m = __builtin_amdgcn_ballot_w64(hit);
            if (!m) continue;
            if (KIND == MOLAR_HIP_SEARCH_WITHIN) {
                if (FILL && lane == 0) out_i[off] = ia[ra];
                off += 1;
                total += 1;
                found = true;
                continue;
            }
            const uint32_t cnt = (uint32_t)__popcll(m);
            if (FILL && hit) {
                const unsigned long long at = off + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                out_i[at] = ia[ra];
                out_j[at] = ib[S.b0 + j];
                out_d[at] = sqrt(d2);                             // d2.sqrt() (:448)
            }
            off += cnt;
            total += cnt;
        }
    }
    if (!FILL && lane == 0) slot_cnt[s] = total;
}

template <bool FILL>
void launch_pair64(int kind, dim3 grid, hipStream_t stream, const Params64 &P, uint32_t *slot_cnt, const unsigned long long *slot_base,
                   unsigned long long *out_i, unsigned long long *out_j, double *out_d) {
    switch (kind) {
        case MOLAR_HIP_SEARCH_SINGLE: hipLaunchKernelGGL((pair64_kernel<FILL, MOLAR_HIP_SEARCH_SINGLE>), grid, dim3(64), 0, stream, P, slot_cnt, slot_base, out_i, out_j, out_d); break;
        case MOLAR_HIP_SEARCH_DOUBLE: hipLaunchKernelGGL((pair64_kernel<FILL, MOLAR_HIP_SEARCH_DOUBLE>), grid, dim3(64), 0, stream, P, slot_cnt, slot_base, out_i, out_j, out_d); break;
        case MOLAR_HIP_SEARCH_WITHIN: hipLaunchKernelGGL((pair64_kernel<FILL, MOLAR_HIP_SEARCH_WITHIN>), grid, dim3(64), 0, stream, P, slot_cnt, slot_base, out_i, out_j, out_d); break;
        default: hipLaunchKernelGGL((pair64_kernel<FILL, MOLAR_HIP_SEARCH_DOUBLE_VDW>), grid, dim3(64), 0, stream, P, slot_cnt, slot_base, out_i, out_j, out_d); break;
    }
}

inline dim3 grid_of(uint32_t n) {
    const unsigned gx = n < (1u << 20) ? (n ? n : 1u) : (1u << 20);
    return dim3(gx, (n + gx - 1u) / gx);
}

// ---- the fused histogram in f64 (molar_hip_search_histogram_f64): search + Histogram1D::add_one (stats.rs:29-35) in ONE pass,
// no count pass, no offsets, no pair list.
//
// The slots are those of the count and fill passes, walked by the same run64 in its RUN_HIST mode: instead of being written,
// a hit's d2 is binned (Hist64, hist64_add).  Second cells above 256 atoms: hist64_chunks, pair64_kernel's loop with binning.
//
// The kernel is persistent: a one-wave workgroup per slot, as the count and fill passes run, would have to flush nbins
// counters per slot (5e4 slots a frame at 250k atoms).  Instead about (CUs x resident workgroups) workgroups of H64_WAVES
// waves each hold one histogram; their waves take slots from one global counter (one atomic per slot) until none is left,
// and the workgroup adds each non-zero counter to the caller's bins with one 64-bit atomic at the end.
//
// Counter overflow: a wave flushes the whole LDS histogram (exchange each counter with 0, add what it held to the bins) when
// the hits it has added since its last flush pass `flush_at` (checked after every slot, and after every chunk in the chunk
// loop).  Every counter then holds at most the sum over the waves of their hits since their own last flush, i.e. less than
// H64_WAVES * (flush_at + 16384) < 2^32 (at most 16384 hits between two checks: a 64-row slot of <= 256 columns).
constexpr int H64_WAVES = 8;
constexpr uint32_t H64_FLUSH_AT = 0xFFFFFFFFu / (uint32_t)H64_WAVES - 16384u;
constexpr size_t H64_EDGES_LDS = 40960;   // the edges join the counters in LDS while both fit in this (nbins <= 3412)

// EL: the edges are copied into LDS behind the counters (else read from global memory)
template <int KIND, bool EL>
__global__ void __launch_bounds__(64 * H64_WAVES) hist64_kernel(Params64 P, uint32_t *__restrict__ next_slot, const double *__restrict__ edges,
                                                                uint32_t nbins, float hmin, float scale, uint32_t flush_at,
                                                                unsigned long long *__restrict__ bins, unsigned long long *__restrict__ count) {
    extern __shared__ double h64_lds[];
    __shared__ unsigned long long wg_total;
    uint32_t *hist = reinterpret_cast<uint32_t *>(h64_lds);
    double *ledges = h64_lds + (nbins + 1u) / 2u;
    for (uint32_t b = threadIdx.x; b < nbins; b += blockDim.x) hist[b] = 0u;
    if (EL)
        for (uint32_t b = threadIdx.x; b <= nbins; b += blockDim.x) ledges[b] = edges[b];
    if (threadIdx.x == 0) wg_total = 0ull;
    __syncthreads();
    const Hist64 H{hist, EL ? ledges : edges, bins, nbins, hmin, scale, (float)nbins};
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t since_flush = 0;
    unsigned long long total = 0;
    for (;;) {
        uint32_t s = 0;
        if (lane == 0) s = atomicAdd(next_slot, 1u);
        s = (uint32_t)__builtin_amdgcn_readlane((int)s, 0);
        if (s >= P.nslots) break;
        const Slot64 S = P.slots[s];
        const uint32_t nch = (S.n2 + 63u) >> 6;
        if (nch > 4u) {
            total += hist64_chunks<KIND>(P, S, lane, H, since_flush, flush_at);
            continue;
        }
        uint32_t t;
        switch (nch) {
            case 1: t = run64<RUN_HIST, KIND, 1>(P, S, lane, 0ull, nullptr, nullptr, nullptr, Fifo64{}, H); break;
            case 2: t = run64<RUN_HIST, KIND, 2>(P, S, lane, 0ull, nullptr, nullptr, nullptr, Fifo64{}, H); break;
            case 3: t = run64<RUN_HIST, KIND, 3>(P, S, lane, 0ull, nullptr, nullptr, nullptr, Fifo64{}, H); break;
            default: t = run64<RUN_HIST, KIND, 4>(P, S, lane, 0ull, nullptr, nullptr, nullptr, Fifo64{}, H); break;
        }
        total += t;
        since_flush += t;
        if (since_flush > flush_at) {
            hist64_flush(H, lane);
            since_flush = 0;
        }
    }
    if (lane == 0 && total) atomicAdd(&wg_total, total);
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < nbins; b += blockDim.x) {
        const uint32_t v = hist[b];
        if (v) atomicAdd(bins + b, (unsigned long long)v);
    }
    if (threadIdx.x == 0 && wg_total) atomicAdd(count, wg_total);
}

template <int KIND, bool EL>
const void *hist64_fn() { return reinterpret_cast<const void *>(&hist64_kernel<KIND, EL>); }

// ================================================================= `within` as a set in f64 (selection/ast.rs:589-631)
//
// What a caller of distance_search_within(_pbc) keeps is SortedSet::from_unsorted(stream) (selection_expr.rs:112): the set of
// first-set atoms with a second-set atom in range.  The set needs no stream, no offsets and no second pass, and an atom that
// has been found needs no further candidate in ANY of its plan entries (within.hip has the f32 form of the same idea):
//  * within64_partners_kernel inverts the plan with plan_entry - the same wrap / drop rules, the same incomplete
//    neighbourhoods of sheared boxes, both halves of every two-set entry - into per-first-cell lists of (second cell, flags);
//  * within64_flags_kernel: one wave per (first-set cell, share of its 64-row blocks).  The wave loads its rows once (one per
//    lane, as run64 does), keeps a mask of the rows still looking and walks the cell's partners: rows pruned against the
//    partner's bounding box with run64's exact f64 lower bound, the partner's atoms 64 at a time in registers, the live rows
//    handed round with v_readlane; a row leaves the mask at its first hit, the wave leaves the list when the mask is empty.
//    Found rows set flags[id] (plain byte stores), id being what the stream would carry;
//  * ascending flagged ids ARE the sorted, de-duplicated set: csr_kernels.hpp's tile counts and compaction.
constexpr uint32_t W64_MAX_PART = 28;
// every (mask, half) pair of the plan has exactly one first cell per origin cell, and origin -> first cell is one to one:
// a cell is the first cell of at most 14 masks x 2 halves entries
static_assert(W64_MAX_PART == 2u * sizeof(MASKS64) / sizeof(MASKS64[0]), "partner lists are sized for the plan's stencil");

__global__ void __launch_bounds__(256) within64_partners_kernel(GridP G, uint64_t ntasks, const uint32_t *__restrict__ startA,
                                                                const uint32_t *__restrict__ startB, uint32_t *__restrict__ part_cnt,
                                                                uint2 *__restrict__ part) {
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (t >= ntasks) return;
    const Entry64 e = plan_entry(G, t, 2u);
    if (e.ca == 0xFFFFFFFFu) return;
    if (startA[e.ca + 1] == startA[e.ca] || startB[e.cb + 1] == startB[e.cb]) return;
    const uint32_t s = atomicAdd(&part_cnt[e.ca], 1u);
    if (s < W64_MAX_PART) part[(size_t)e.ca * W64_MAX_PART + s] = make_uint2(e.cb, e.flags);
}

// The hit decision of one candidate as run64's count pass (FILL = false) makes it: row atom a against column atom b (`cand`:
// the lane holds a column).  Entries classified by the adjacent image (`approx`; c = b + S): the plain distance to c decides
// outside [band_lo, band_hi] * cutoff^2, PeriodicBox::distance_squared inside the band; every other entry: pair_d2.
// (A copy, not a helper shared with run64: routing the two through one changed run64's ISA.  Tried twice; the second time, the
// image shift and the pruning bound as two __forceinline__ helpers, by 60-100 instructions per pair and histogram kernel.)
__device__ __forceinline__ bool within64_hit(const Params64 &P, uint32_t wrap, bool approx, bool cand, D3 a, D3 b, D3 c) {
    const double cut2 = P.cutoff2;
    if (approx) {
        const double ex = c.x - a.x, ey = c.y - a.y, ez = c.z - a.z;
        const double q2 = (ex * ex + ey * ey) + ez * ez;
        const bool sure = q2 < cut2 * P.band_lo, maybe = cand && q2 <= cut2 * P.band_hi;
        double d2 = q2;
        if (__builtin_amdgcn_ballot_w64(maybe && !sure)) {
            if (maybe && !sure) d2 = pair_d2(P, wrap, a, b);
        }
        return maybe && (sure || d2 <= cut2);
    }
    return cand && pair_d2(P, wrap, a, b) <= cut2;
}

__global__ void __launch_bounds__(64) within64_flags_kernel(Params64 P, const uint32_t *__restrict__ startA, const uint32_t *__restrict__ startB,
                                                            const uint32_t *__restrict__ part_cnt, const uint2 *__restrict__ part,
                                                            uint8_t *__restrict__ flags, uint32_t nsplit) {
    const uint32_t lane = threadIdx.x, ca = blockIdx.x;
    const uint32_t a0 = startA[ca], n1 = startA[ca + 1] - a0;
    uint32_t np = part_cnt[ca];
    if (n1 == 0u || np == 0u) return;
    if (np > W64_MAX_PART) np = W64_MAX_PART;
    for (uint32_t i0 = blockIdx.y * 64u; i0 < n1; i0 += nsplit * 64u) {
        const uint32_t rows = n1 - i0 < 64u ? n1 - i0 : 64u;
        double ax = 0.0, ay = 0.0, az = 0.0;
        uint32_t aid = 0u;
        if (lane < rows) {
            const size_t ra = (size_t)a0 + i0 + lane;
            ax = P.posA[3 * ra]; ay = P.posA[3 * ra + 1]; az = P.posA[3 * ra + 2];
            aid = (uint32_t)P.idA[ra];
        }
        const unsigned long long full = __builtin_amdgcn_ballot_w64(lane < rows);
        unsigned long long live = full;                      // rows still looking for a partner atom
        for (uint32_t pi = 0; pi < np && live; ++pi) {
            const uint2 e = part[(size_t)ca * W64_MAX_PART + pi];
            const uint32_t cb = (uint32_t)__builtin_amdgcn_readfirstlane((int)e.x), fl = (uint32_t)__builtin_amdgcn_readfirstlane((int)e.y);
            const uint32_t wrap = fl & 7u;
            const uint32_t b0 = startB[cb], n2 = startB[cb + 1] - b0;
            // b + S is the image of the second cell next to the first one (run64)
            const bool approx = P.approx_wrapped && P.use_box && wrap != 0u && !(P.box->nshift != 0 && wrap == MOLAR_HIP_PBC_FULL);
            double Sx = 0.0, Sy = 0.0, Sz = 0.0;
            if (approx)
                for (int d = 0; d < 3; ++d) {
                    if (!((wrap >> d) & 1u)) continue;
                    const double sgn = ((fl >> (12 + d)) & 1u) ? 1.0 : -1.0;
                    Sx += sgn * P.box->m[3 * d];
                    Sy += sgn * P.box->m[3 * d + 1];
                    Sz += sgn * P.box->m[3 * d + 2];
                }
            unsigned long long cand = live;
            if (wrap == 0u || !P.use_box || approx) {        // run64's row pruning: an f64 lower bound of every d2 of the row
                const double *bb = P.aabbB + 6 * (size_t)cb;
                double px = ax, py = ay, pz = az, lim = P.cutoff2;
                if (approx) {
                    px = ax - Sx;
                    py = ay - Sy;
                    pz = az - Sz;
                    lim = P.prune_limit2;
                }
                const double ex = fmax(fmax(bb[0] - px, px - bb[3]), 0.0), ey = fmax(fmax(bb[1] - py, py - bb[4]), 0.0),
                             ez = fmax(fmax(bb[2] - pz, pz - bb[5]), 0.0);
                cand &= __builtin_amdgcn_ballot_w64(!((ex * ex + ey * ey) + ez * ez > lim));
            }
            for (uint32_t j0 = 0; j0 < n2 && cand; j0 += 64u) {
                const bool inb = j0 + lane < n2;
                double bx = 0.0, by = 0.0, bz = 0.0;
                if (inb) {
                    const size_t rb = (size_t)b0 + j0 + lane;
                    bx = P.posB[3 * rb]; by = P.posB[3 * rb + 1]; bz = P.posB[3 * rb + 2];
                }
                const D3 b = D3{bx, by, bz}, cimg = D3{bx + Sx, by + Sy, bz + Sz};
                unsigned long long rm = cand;
                while (rm) {
                    const uint32_t r = (uint32_t)__builtin_ctzll(rm);
                    rm &= rm - 1ull;
                    const D3 a = D3{lane_bcast(ax, r), lane_bcast(ay, r), lane_bcast(az, r)};
                    if (__builtin_amdgcn_ballot_w64(within64_hit(P, wrap, approx, inb, a, b, cimg))) {   // the row's first hit (:287-290)
                        live &= ~(1ull << r);
                        cand &= ~(1ull << r);
                    }
                }
            }
        }
        if (((full & ~live) >> lane) & 1ull) flags[aid] = 1u;
    }
}

// SearchConnectivity::from_iter (connectivity.rs:19-35) over the f64 search's id columns: pair p pushes j onto i's list
// (entry 2p), then i onto j's (entry 2p + 1) - conn_entries_kernel of connectivity.hip for two uint64 columns
__global__ void __launch_bounds__(256) conn64_entries_kernel(const unsigned long long *__restrict__ pi, const unsigned long long *__restrict__ pj,
                                                             unsigned long long npairs, uint32_t *__restrict__ row, uint32_t *__restrict__ nb) {
    const unsigned long long p = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    if (p >= npairs) return;
    const uint32_t i = (uint32_t)pi[p], j = (uint32_t)pj[p];
    reinterpret_cast<uint2 *>(row)[p] = make_uint2(i, j);
    reinterpret_cast<uint2 *>(nb)[p] = make_uint2(j, i);
}

}  // namespace

namespace mh {
void search64_release(molar_hip_ctx *c) {
    release_state(c->s64);
}
}  // namespace mh

extern "C" {

// a small host-side input (a box, a corner) that may lie in device memory
static int host_copy(molar_hip_ctx *c, const double *src, size_t count, double *dst) {
    if (is_device_ptr(src)) MH_HIP(hipMemcpy(dst, src, count * 8, hipMemcpyDeviceToHost));
    else std::memcpy(dst, src, count * 8);
    return 0;
}

// grid of one set on the device: items in the reference's push order (pos / id / vdw), CSR starts per cell
static int build_grid64(molar_hip_ctx *c, molar_hip_search64_state &Z, const SetIn &S, const GridP &G, DevBuf &pos, DevBuf &id, DevBuf &vdw,
                        DevBuf &start, int *err_dev) {
    const uint32_t n = S.nsel;
    MH_TRY(start.reserve(((size_t)G.ncells + 1) * 4));
    MH_TRY(pos.reserve((size_t)(n ? n : 1) * 24));
    MH_TRY(id.reserve((size_t)(n ? n : 1) * 8));
    if (S.vdw) MH_TRY(vdw.reserve((size_t)(n ? n : 1) * 8));
    if (n == 0) {
        MH_HIP(hipMemsetAsync(start.p, 0, ((size_t)G.ncells + 1) * 4, c->stream));
        return 0;
    }
    MH_TRY(Z.key_in.reserve((size_t)n * 4));
    MH_TRY(Z.key_out.reserve((size_t)n * 4));
    MH_TRY(Z.val_in.reserve((size_t)n * 4));
    MH_TRY(Z.val_out.reserve((size_t)n * 4));
    MH_TRY(Z.pos3.reserve((size_t)n * 24));
    const unsigned nb = (n + 255u) / 256u;
    hipLaunchKernelGGL(assign64_kernel, dim3(nb), dim3(256), 0, c->stream, S, G, Z.key_in.as<uint32_t>(), Z.val_in.as<uint32_t>(),
                       Z.pos3.as<double>(), err_dev);
    int end_bit = 1;
    while (end_bit < 32 && (2ull * G.ncells) >> end_bit) ++end_bit;            // keys 0 .. 2 * ncells
    MH_TRY(device_sort_pairs_u32(c->stream, Z.cub_tmp, Z.key_in.as<uint32_t>(), Z.key_out.as<uint32_t>(), Z.val_in.as<uint32_t>(), Z.val_out.as<uint32_t>(),
                                 n, end_bit));
    hipLaunchKernelGGL(gather64_kernel, dim3(nb), dim3(256), 0, c->stream, S, n, G.ncells, Z.key_out.as<uint32_t>(), Z.val_out.as<uint32_t>(),
                       Z.pos3.as<double>(), pos.as<double>(), id.as<unsigned long long>(), S.vdw ? vdw.as<double>() : nullptr);
    hipLaunchKernelGGL(cellstart64_kernel, dim3((G.ncells + 1u + 255u) / 256u), dim3(256), 0, c->stream, Z.key_out.as<uint32_t>(), n, G.ncells,
                       start.as<uint32_t>());
    MH_HIP(hipGetLastError());
    return 0;
}

// What the first half of a search's prologue leaves for the second (prepare64) or for the partner lists of the set form
struct Prep64 {
    GridP G;
    BoxD box;
    double ext[3];
    uint64_t dims[3];
    double cutoff;
    uint32_t mult;
    bool two, vdw, use_box;
    int *err_dev;                          // raised by the grid build: a selection index out of range
    const uint32_t *startA, *startB;
};

// The parameter block of an evaluation from the cached state
static Params64 params64(const molar_hip_search64_state &Z) {
    const bool two = Z.kind != MOLAR_HIP_SEARCH_SINGLE;
    const DevBuf &pB = two ? Z.posB : Z.posA, &iB = two ? Z.idB : Z.idA, &vB = two ? Z.vdwB : Z.vdwA;
    return Params64{Z.posA.as<double>(), pB.as<double>(), Z.vdwA.as<double>(), vB.as<double>(),
                    Z.idA.as<unsigned long long>(), iB.as<unsigned long long>(), Z.box.as<BoxD>(), Z.slots.as<Slot64>(), Z.nslots,
                    Z.kind, Z.use_box ? 1 : 0, Z.cutoff * Z.cutoff, Z.approx ? 1 : 0, Z.band_lo, Z.band_hi, (two ? Z.aabbB : Z.aabbA).as<double>(), Z.prune_limit2};
}

// First half of the prologue, up to the point where the slot form and the set form part: the sets on the device, the box,
// the bounds, the grid dims, both grids and the cells' bounding boxes.  Enqueues only (but for the vdW radii maximum and the
// non-periodic bounding box, which the host needs for the grid).  *empty: a vdW search with an empty set.
static int prepare64_grids(molar_hip_ctx *c, const molar_hip_search_desc_f64 *q, Prep64 *R, bool *empty) {
    MH_HIP(hipSetDevice(c->device));
    if (!c->s64) c->s64 = new molar_hip_search64_state;
    molar_hip_search64_state &Z = *c->s64;
    Z.have = false;
    Z.have_within = false;
    const int kind = q->kind;
    if (kind < MOLAR_HIP_SEARCH_SINGLE || kind > MOLAR_HIP_SEARCH_DOUBLE_VDW)
        return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "search_count_f64: unknown kind %d", kind);
    const bool two = kind != MOLAR_HIP_SEARCH_SINGLE, vdw = kind == MOLAR_HIP_SEARCH_DOUBLE_VDW;
    if (vdw && (!q->vdw1 || !q->vdw2)) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "vdw search: radii pointer is null");
    if (!q->xyz1 || (two && !q->xyz2)) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "search_f64: xyz pointer is null");
    // ---- the two sets on the device (in place if they are device memory)
    SetIn S[2] = {};
    const double *hvdw[2] = {nullptr, nullptr};            // radii the host can read without a copy
    for (int w = 0; w < (two ? 2 : 1); ++w) {
        const double *xyz = w ? q->xyz2 : q->xyz1, *vd = vdw ? (w ? q->vdw2 : q->vdw1) : nullptr;
        const uint64_t *idx = w ? q->idx2 : q->idx1;
        const size_t natoms = w ? q->natoms2 : q->natoms1, nidx = w ? q->n2 : q->n1;
        const size_t nsel = idx ? nidx : natoms;
        if (nsel >= 0x7FFFFFFFull) return fail(MOLAR_HIP_ERR_TOO_LARGE, "search_f64: %zu atoms exceed the 2^31 limit", nsel);
        const double *dx, *dv;             // in place if they are device memory, staged otherwise
        const uint64_t *di;
        MH_TRY(to_device(c, xyz, natoms * 3, Z.in_xyz[w], &dx));
        MH_TRY(to_device(c, idx, idx ? nsel : 0, Z.in_idx[w], &di));
        MH_TRY(to_device(c, vd, vd ? nsel : 0, Z.in_vdw[w], &dv));
        S[w] = SetIn{dx, reinterpret_cast<const unsigned long long *>(di), dv, (uint64_t)natoms, (uint32_t)nsel, (q->ids_local || vdw) ? 1 : 0};
        if (vd && !is_device_ptr(vd)) hvdw[w] = vd;
    }
    BoxD box{};
    const bool use_box = q->box9 != nullptr;
    if (use_box) {
        double hb[9];
        MH_TRY(host_copy(c, q->box9, 9, hb));
        MH_TRY(box64_from_matrix(hb, &box));
    }
    Z.kind = kind;
    Z.use_box = use_box;
    Z.pbc = use_box ? q->pbc : 0;
    Z.total = 0;
    Z.nslots = 0;
    Z.dims[0] = Z.dims[1] = Z.dims[2] = 1;
    *empty = false;
    constexpr unsigned PARTS = 256;                        // workgroups of the reductions whose result the host needs
    MH_TRY(Z.partial.reserve((size_t)PARTS * 6 * 8 * 2));
    MH_TRY(Z.flags.reserve(64));
    MH_HIP(hipMemsetAsync(Z.flags.p, 0, 64, c->stream));
    int *err_dev = Z.flags.as<int>();
    std::vector<double> hpart((size_t)PARTS * 6 * 2);
    double cutoff = q->cutoff;
    if (vdw) {
        if (S[0].nsel == 0 || S[1].nsel == 0) {        // the reference unwrap()s an empty max: nothing to report here
            *empty = true;
            return MOLAR_HIP_OK;
        }
        double mx[2];
        for (int w = 0; w < 2; ++w) {                    // Iterator::reduce(Float::max): NaN-ignoring max (:781-783)
            if (hvdw[w]) {
                double m = hvdw[w][0];
                for (size_t k = 1; k < S[w].nsel; ++k) m = std::fmax(m, hvdw[w][k]);
                mx[w] = m;
                continue;
            }
            const unsigned nb = std::min<unsigned>(PARTS, (S[w].nsel + 255u) / 256u);
            hipLaunchKernelGGL(fmax64_kernel, dim3(nb), dim3(256), 0, c->stream, S[w].vdw, S[w].nsel, Z.partial.as<double>());
            MH_HIP(hipMemcpyAsync(hpart.data(), Z.partial.p, (size_t)nb * 8, hipMemcpyDeviceToHost, c->stream));
            MH_HIP(hipStreamSynchronize(c->stream));
            double m = hpart[0];
            for (unsigned b = 1; b < nb; ++b) m = std::fmax(m, hpart[b]);
            mx[w] = m;
        }
        cutoff = (mx[0] + mx[1]) + 2.220446049250313e-16;
    }
    if (!(cutoff > 0.0)) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "search_f64: cutoff must be positive (got %g)", cutoff);
    Z.cutoff = cutoff;
    double lower[3] = {0, 0, 0}, upper[3] = {0, 0, 0}, ext[3];
    if (use_box) {
        ext[0] = (box.m[0] + box.m[3]) + box.m[6];                                          // get_lab_extents (:369-375)
        ext[1] = (box.m[1] + box.m[4]) + box.m[7];
        ext[2] = (box.m[2] + box.m[5]) + box.m[8];
    } else {
        if (kind == MOLAR_HIP_SEARCH_WITHIN) {
            if (!q->lower3 || !q->upper3) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "non-periodic within search needs lower3/upper3");
            MH_TRY(host_copy(c, q->lower3, 3, lower));
            MH_TRY(host_copy(c, q->upper3, 3, upper));
        } else {
            // compute_min_max (:602-616, seeded with zeros) + compute_bounding_box_single / _double (:618-646)
            double lo[2][3] = {}, hi[2][3] = {};
            for (int w = 0; w < (two ? 2 : 1); ++w) {
                const unsigned nb = std::max(1u, std::min<unsigned>(PARTS, (S[w].nsel + 255u) / 256u));
                hipLaunchKernelGGL(minmax64_kernel, dim3(nb), dim3(256), 0, c->stream, S[w], Z.partial.as<double>(), err_dev);
                MH_HIP(hipMemcpyAsync(hpart.data(), Z.partial.p, (size_t)nb * 48, hipMemcpyDeviceToHost, c->stream));
                MH_HIP(hipStreamSynchronize(c->stream));
                for (unsigned b = 0; b < nb; ++b)
                    for (int d = 0; d < 3; ++d) {
                        if (hpart[6 * b + d] < lo[w][d]) lo[w][d] = hpart[6 * b + d];
                        if (hpart[6 * b + 3 + d] > hi[w][d]) hi[w][d] = hpart[6 * b + 3 + d];
                    }
            }
            for (int d = 0; d < 3; ++d) {
                lower[d] = lo[0][d];
                upper[d] = hi[0][d];
                if (two) {
                    lower[d] = lo[0][d] < lo[1][d] ? lo[0][d] : lo[1][d];
                    upper[d] = hi[0][d] > hi[1][d] ? hi[0][d] : hi[1][d];
                }
                lower[d] += (-cutoff - 2.220446049250313e-16);
                upper[d] += (cutoff + 2.220446049250313e-16);
            }
        }
        for (int d = 0; d < 3; ++d) ext[d] = upper[d] - lower[d];
    }
    uint64_t dims[3];
    double ncell_d = 1.0;
    for (int d = 0; d < 3; ++d) {                                                            // :103-110
        dims[d] = std::max<uint64_t>(as_usize(std::floor(ext[d] / cutoff)), 1);
        ncell_d *= (double)dims[d];
    }
    const uint32_t mult = two ? 2u : 1u;
    if (!(ncell_d * 14.0 * mult < 2.0e9))
        return fail(MOLAR_HIP_ERR_TOO_LARGE, "search_f64: grid of %.3g cells (the plan of this path holds one word per entry)", ncell_d);
    std::memcpy(Z.dims, dims, sizeof dims);
    GridP G{};
    G.box = box;
    G.use_box = use_box ? 1 : 0;
    G.pbc = Z.pbc;
    for (int d = 0; d < 3; ++d) { G.dims[d] = (uint32_t)dims[d]; G.lower[d] = lower[d]; G.upper[d] = upper[d]; }
    G.ncells = (uint32_t)(dims[0] * dims[1] * dims[2]);
    // ---- grids (populate / populate_pbc) and the plan, on the device
    MH_TRY(build_grid64(c, Z, S[0], G, Z.posA, Z.idA, Z.vdwA, Z.startA, err_dev));
    if (two) MH_TRY(build_grid64(c, Z, S[1], G, Z.posB, Z.idB, Z.vdwB, Z.startB, err_dev));
    const uint32_t *startA = Z.startA.as<uint32_t>(), *startB = two ? Z.startB.as<uint32_t>() : startA;
    {   // bounding boxes of the second grid's cells
        DevBuf &bb = two ? Z.aabbB : Z.aabbA;
        MH_TRY(bb.reserve((size_t)G.ncells * 48));
        hipLaunchKernelGGL(aabb64_kernel, dim3((G.ncells + 3u) / 4u), dim3(256), 0, c->stream, startB, G.ncells,
                           (two ? Z.posB : Z.posA).as<double>(), bb.as<double>());
    }
    R->G = G;
    R->box = box;
    std::memcpy(R->ext, ext, sizeof ext);
    std::memcpy(R->dims, dims, sizeof dims);
    R->cutoff = cutoff;
    R->mult = mult;
    R->two = two;
    R->vdw = vdw;
    R->use_box = use_box;
    R->err_dev = err_dev;
    R->startA = startA;
    R->startB = startB;
    return MOLAR_HIP_OK;
}

// Entries across the periodic boundary (search.hip, make_params, derives the same bound for f32): the reference evaluates
// v = p2 - p1, f = inv v, f -= round(f), s = M f; the kernels classify with (b + S) - a.  With u = 2^-53, L the largest
// |coordinate| the box allows and kappa = || |M| |M^-1| ||_inf the two difference vectors disagree by at most
// e = (4 kappa + 9) u L per component, d2 near cutoff^2 by 2 sqrt(3) e / rc relative to cutoff^2.  Outside a band of
// 1e-9 + four times that around cutoff^2 the plain distance to the adjacent image decides; inside it, and for every hit's
// distance, PeriodicBox::distance_squared itself.  Needs >= 4 cells along every periodic dimension (round(f_d) = +-1 for
// every pair of a wrapped entry that can be within the cutoff).  Host arithmetic only.
static void classify64(molar_hip_search64_state &Z, const Prep64 &R) {
    const BoxD &box = R.box;
    const double *ext = R.ext, cutoff = R.cutoff;
    const uint64_t *dims = R.dims;
    const bool use_box = R.use_box, vdw = R.vdw;
    Z.approx = false;
    Z.band_lo = Z.band_hi = 1.0;
    if (use_box) {
        bool ok = true;
        double lmax = 0.0, lsum = 0.0, kappa = 0.0;
        for (int d = 0; d < 3; ++d) {
            if (((Z.pbc >> d) & 1u) && dims[d] < 4u) ok = false;
            lmax = std::fmax(lmax, std::fabs(ext[d]));
            double row = 0.0;
            for (int k = 0; k < 3; ++k) {
                lmax = std::fmax(lmax, std::fabs(box.m[3 * k + d]));
                row += std::fabs(box.m[3 * k + d]);
            }
            lsum = std::fmax(lsum, row);
        }
        lmax = std::fmax(lmax, lsum);
        for (int i = 0; i < 3; ++i) {
            double row = 0.0;
            for (int j = 0; j < 3; ++j)
                for (int k = 0; k < 3; ++k) row += std::fabs(box.m[3 * k + i]) * std::fabs(box.inv[3 * j + k]);
            kappa = std::fmax(kappa, row);
        }
        const double e = (4.0 * kappa + 9.0) * 1.1102230246251565e-16 * lmax;
        const double rel = 1.0e-9 + 4.0 * 2.0 * 1.7320508075688772 * e / cutoff;
        if (ok && !vdw && std::isfinite(kappa) && rel < 1.0e-3) {        // (vdW: the cutoff differs from pair to pair - always exact)
            Z.approx = true;
            Z.band_lo = 1.0 - rel;
            Z.band_hi = 1.0 + rel;
            const double lim = cutoff + (1.0e-9 + 4.0 * 1.7320508075688772 * e);      // row pruning against the image box: the same margin
            Z.prune_limit2 = lim * lim;
        }
    }
}

// Everything of a search before its evaluation, shared by the count pass and the fused histogram: prepare64_grids, then the
// plan, its scan (read back: the number of slots), the slot records and the classification of wrapped entries.  *P is the
// parameter block of the evaluation; *empty: nothing to evaluate (no slot, or a vdW search with an empty set).
static int prepare64(molar_hip_ctx *c, const molar_hip_search_desc_f64 *q, Params64 *P, bool *empty) {
    Prep64 R;
    MH_TRY(prepare64_grids(c, q, &R, empty));
    if (*empty) return MOLAR_HIP_OK;
    molar_hip_search64_state &Z = *c->s64;
    const GridP &G = R.G;
    const BoxD &box = R.box;
    const uint32_t mult = R.mult;
    const uint32_t *startA = R.startA, *startB = R.startB;
    int *err_dev = R.err_dev;
    const uint64_t ntasks = (uint64_t)G.ncells * 14ull * mult;
    MH_TRY(Z.task_ns.reserve((ntasks + 1) * 4));
    MH_TRY(Z.task_first.reserve((ntasks + 1) * 4));
    hipLaunchKernelGGL(plan64_kernel, dim3((unsigned)((ntasks + 1 + 255) / 256)), dim3(256), 0, c->stream, G, ntasks, mult, startA, startB,
                       Z.task_ns.as<uint32_t>());
    MH_TRY(device_exclusive_sum_u32(c, Z.cub_tmp, Z.task_ns.as<uint32_t>(), Z.task_first.as<uint32_t>(), ntasks + 1));
    struct { uint32_t nslots; int err; } hs = {0, 0};
    MH_HIP(hipMemcpyAsync(&hs.nslots, Z.task_first.as<uint32_t>() + ntasks, 4, hipMemcpyDeviceToHost, c->stream));
    MH_HIP(hipMemcpyAsync(&hs.err, err_dev, 4, hipMemcpyDeviceToHost, c->stream));
    MH_HIP(hipStreamSynchronize(c->stream));
    if (hs.err) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "search_f64: selection index out of range");
    if (hs.nslots >= 0x7FFFFF00u) return fail(MOLAR_HIP_ERR_TOO_LARGE, "search_f64: plan too large");
    Z.nslots = hs.nslots;
    Z.total = 0;
    if (Z.nslots == 0) {
        *empty = true;
        return MOLAR_HIP_OK;
    }
    MH_TRY(Z.slots.reserve((size_t)Z.nslots * sizeof(Slot64)));
    hipLaunchKernelGGL(slots64_kernel, dim3((unsigned)((ntasks + 255) / 256)), dim3(256), 0, c->stream, G, ntasks, mult, startA, startB,
                       Z.task_first.as<uint32_t>(), Z.slots.as<Slot64>());
    MH_TRY(Z.box.reserve(sizeof box));
    MH_HIP(hipMemcpyAsync(Z.box.p, &box, sizeof box, hipMemcpyHostToDevice, c->stream));
    classify64(Z, R);
    *P = params64(Z);
    return MOLAR_HIP_OK;
}

int molar_hip_search_count_f64(molar_hip_ctx *c, const molar_hip_search_desc_f64 *q, uint64_t *out_count) {
    if (!c || !q) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "search_count_f64: null argument");
    Params64 P{};
    bool empty = false;
    MH_TRY(prepare64(c, q, &P, &empty));
    molar_hip_search64_state &Z = *c->s64;
    if (empty) {
        Z.have = true;
        if (out_count) *out_count = 0;
        return MOLAR_HIP_OK;
    }
    // ---- count, offsets
    MH_TRY(Z.slot_cnt.reserve(((size_t)Z.nslots + 1) * 4));
    MH_TRY(Z.slot_base.reserve(((size_t)Z.nslots + 1) * 8));
    MH_HIP(hipMemsetAsync(Z.slot_cnt.as<uint32_t>() + Z.nslots, 0, 4, c->stream));
    launch_pair64<false>(Z.kind, grid_of(Z.nslots), c->stream, P, Z.slot_cnt.as<uint32_t>(), nullptr, nullptr, nullptr, nullptr);
    MH_HIP(hipGetLastError());
    MH_TRY(device_exclusive_sum_u32_u64(c, Z.cub_tmp, Z.slot_cnt.as<uint32_t>(), Z.slot_base.as<unsigned long long>(), (size_t)Z.nslots + 1));
    unsigned long long run = 0;
    MH_HIP(hipMemcpyAsync(&run, Z.slot_base.as<unsigned long long>() + Z.nslots, 8, hipMemcpyDeviceToHost, c->stream));
    MH_HIP(hipStreamSynchronize(c->stream));
    Z.total = run;
    Z.have = true;
    if (out_count) *out_count = run;
    return MOLAR_HIP_OK;
}

static int fill64(molar_hip_ctx *c, uint64_t *oi, uint64_t *oj, double *od, bool within) {
    if (!c || !c->s64 || !c->s64->have) return fail(MOLAR_HIP_ERR_NO_SEARCH, "no cached f64 search: call molar_hip_search_count_f64 first");
    molar_hip_search64_state &Z = *c->s64;
    if ((Z.kind == MOLAR_HIP_SEARCH_WITHIN) != within)
        return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, within ? "fill_ids_f64 is for within searches" : "within search yields ids: use molar_hip_search_fill_ids_f64");
    if (Z.total == 0 || Z.nslots == 0) return MOLAR_HIP_OK;
    MH_HIP(hipSetDevice(c->device));
    const size_t n = (size_t)Z.total;
    auto dev = [&](void *user, DevBuf &own, size_t bytes, void **out) -> int {
        if (user && is_device_ptr(user)) { *out = user; return 0; }
        MH_TRY(own.reserve(bytes));
        *out = own.p;
        return 0;
    };
    void *di, *dj = nullptr, *dd = nullptr;
    MH_TRY(dev(oi, Z.out_i, n * 8, &di));
    if (!within) {
        MH_TRY(dev(oj, Z.out_j, n * 8, &dj));
        MH_TRY(dev(od, Z.out_d, n * 8, &dd));
    }
    const Params64 P = params64(Z);
    launch_pair64<true>(Z.kind, grid_of(Z.nslots), c->stream, P, nullptr, Z.slot_base.as<unsigned long long>(),
                        static_cast<unsigned long long *>(di), static_cast<unsigned long long *>(dj), static_cast<double *>(dd));
    MH_HIP(hipGetLastError());
    std::vector<RingJob> jobs;
    if (oi && di != oi) jobs.push_back(RingJob{di, n * 8, RING_COPY, oi, nullptr});
    if (oj && dj != oj) jobs.push_back(RingJob{dj, n * 8, RING_COPY, oj, nullptr});
    if (od && dd != od) jobs.push_back(RingJob{dd, n * 8, RING_COPY, od, nullptr});
    if (n * 8 * jobs.size() >= (24u << 20)) {
        MH_TRY(ring_to_host(c, jobs));              // large results: pinned ring + host threads (hoststream.hpp)
    } else {
        for (const RingJob &J : jobs) MH_HIP(hipMemcpyAsync(J.dst0, J.src, J.bytes, hipMemcpyDeviceToHost, c->stream));
    }
    MH_HIP(hipStreamSynchronize(c->stream));
    return MOLAR_HIP_OK;
}

int molar_hip_search_fill_f64(molar_hip_ctx *c, uint64_t *i, uint64_t *j, double *dist) { return fill64(c, i, j, dist, false); }

int molar_hip_search_fill_ids_f64(molar_hip_ctx *c, uint64_t *ids) { return fill64(c, ids, nullptr, nullptr, true); }

int molar_hip_search_grid_dims_f64(molar_hip_ctx *c, uint64_t dims[3]) {
    if (!c || !c->s64 || !c->s64->have || !dims) return fail(MOLAR_HIP_ERR_NO_SEARCH, "no cached f64 search");
    for (int d = 0; d < 3; ++d) dims[d] = c->s64->dims[d];
    return MOLAR_HIP_OK;
}

// The f64 twin of histogram_edges (search.hip): edges[b], b = 0..nbins, is the smallest non-negative double x whose bin
// floor(n * (sqrt(x) - min) / (max - min)) is >= b, found by bisection over the bit patterns of the non-negative doubles
// (ordered like the values) with the formula itself.  Each IEEE step of the formula is monotone, so the bin is a
// non-decreasing function of x, and "the largest b with edges[b] <= x" IS the formula.  False unless min < max and both
// and their difference are finite, and nbins > 0.
static bool histogram_edges64(double hmin, double hmax, size_t nbins, double *edges) {
    if (!(hmax > hmin) || !std::isfinite(hmin) || !std::isfinite(hmax) || !std::isfinite(hmax - hmin) || nbins == 0) return false;
    const double hn = (double)nbins, range = hmax - hmin;
    auto bin_of = [&](uint64_t bits) -> double {
        double x;
        std::memcpy(&x, &bits, 8);
        volatile double d = std::sqrt(x);
        volatile double t = d - hmin;
        volatile double u = hn * t;
        volatile double v = u / range;
        return std::floor(v);
    };
    for (size_t b = 0; b <= nbins; ++b) {
        uint64_t lo = 0u, hi = 0x7FF0000000000000ull;           // +0.0 .. +inf; bin_of(+inf) = +inf >= b
        if (bin_of(lo) >= (double)b) {
            hi = lo;
        } else {
            while (hi - lo > 1u) {                                // invariant: bin_of(lo) < b <= bin_of(hi)
                const uint64_t mid = lo + (hi - lo) / 2u;
                if (bin_of(mid) >= (double)b) hi = mid;
                else lo = mid;
            }
        }
        std::memcpy(&edges[b], &hi, 8);
    }
    return true;
}

int molar_hip_histogram_edges_f64(double hmin, double hmax, size_t nbins, double *edges) {
    if (!edges) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "histogram_edges_f64: null argument");
    if (!histogram_edges64(hmin, hmax, nbins, edges))
        return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "histogram_edges_f64: needs finite min < max and nbins > 0");
    return MOLAR_HIP_OK;
}

// argument checks of the fused f64 histogram; the edges of (hmin, hmax, nbins) on the device (computed when the range changes)
static int hist64_begin(molar_hip_ctx *c, const molar_hip_search_desc_f64 *q, double hmin, double hmax, size_t nbins, const void *bins) {
    if (!c || !q || !bins) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "search_histogram_f64: null argument");
    if (q->kind == MOLAR_HIP_SEARCH_WITHIN)
        return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "search_histogram_f64: a within search has no distances");
    if (q->kind < MOLAR_HIP_SEARCH_SINGLE || q->kind > MOLAR_HIP_SEARCH_DOUBLE_VDW)
        return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "search_histogram_f64: unknown kind %d", (int)q->kind);
    if (nbins == 0 || nbins > 8192) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "search_histogram_f64: nbins must be in 1..8192");
    MH_HIP(hipSetDevice(c->device));
    if (!c->s64) c->s64 = new molar_hip_search64_state;
    molar_hip_search64_state &Z = *c->s64;
    Z.have = false;                   // the histogram reuses the cached search's buffers: fill_f64 has nothing to fill after it
    if (Z.edges_n == nbins && Z.edges_min == hmin && Z.edges_max == hmax) return 0;
    Z.edges_n = 0;
    Z.h_edges.resize(nbins + 1);
    if (!histogram_edges64(hmin, hmax, nbins, Z.h_edges.data()))
        return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "search_histogram_f64: needs finite min < max");
    MH_TRY(Z.hedges.reserve((nbins + 1) * 8));
    MH_HIP(hipStreamSynchronize(c->stream));          // a kernel of an earlier call may still read the old table
    MH_HIP(hipMemcpyAsync(Z.hedges.p, Z.h_edges.data(), (nbins + 1) * 8, hipMemcpyHostToDevice, c->stream));
    MH_HIP(hipStreamSynchronize(c->stream));
    Z.edges_min = hmin;
    Z.edges_max = hmax;
    Z.edges_n = nbins;
    return 0;
}

// one frame: the search's prologue, then hist64_kernel adding into bins / count (device memory)
static int hist64_frame(molar_hip_ctx *c, const molar_hip_search_desc_f64 *q, size_t nbins, unsigned long long *bins,
                        unsigned long long *count) {
    Params64 P{};
    bool empty = false;
    MH_TRY(prepare64(c, q, &P, &empty));
    molar_hip_search64_state &Z = *c->s64;
    Z.have = false;
    if (empty) return 0;
    const bool el = (size_t)(nbins + 1) / 2 * 8 + (nbins + 1) * 8 <= H64_EDGES_LDS;
    const size_t lds = (size_t)(nbins + 1) / 2 * 8 + (el ? (nbins + 1) * 8 : 0);
    const void *fn = nullptr;
    switch (Z.kind) {
        case MOLAR_HIP_SEARCH_SINGLE: fn = el ? hist64_fn<MOLAR_HIP_SEARCH_SINGLE, true>() : hist64_fn<MOLAR_HIP_SEARCH_SINGLE, false>(); break;
        case MOLAR_HIP_SEARCH_DOUBLE: fn = el ? hist64_fn<MOLAR_HIP_SEARCH_DOUBLE, true>() : hist64_fn<MOLAR_HIP_SEARCH_DOUBLE, false>(); break;
        default: fn = el ? hist64_fn<MOLAR_HIP_SEARCH_DOUBLE_VDW, true>() : hist64_fn<MOLAR_HIP_SEARCH_DOUBLE_VDW, false>(); break;
    }
    // persistent grid: as many workgroups as are resident at once (occupancy of this kernel and LDS size, cached), no more
    // than the slots need
    const int key = (int)(Z.kind * 2 + (el ? 1 : 0)) | (int)(lds << 4);
    if (Z.occ_key != key) {
        int per_cu = 0;
        MH_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, 64 * H64_WAVES, lds));
        Z.occ_blocks = per_cu > 0 ? per_cu : 1;
        Z.occ_key = key;
    }
    const unsigned nwg = (unsigned)std::max<uint64_t>(1u, std::min<uint64_t>((uint64_t)Z.occ_blocks * c->num_cus,
                                                                             ((uint64_t)Z.nslots + H64_WAVES - 1) / H64_WAVES));
    MH_TRY(Z.hnext.reserve(4));
    MH_HIP(hipMemsetAsync(Z.hnext.p, 0, 4, c->stream));
    uint32_t flush_at = H64_FLUSH_AT;
    if (const char *e = std::getenv("MOLAR_HIP_HIST64_FLUSH")) {      // tests: flush the LDS counters after fewer hits
        const unsigned long v = std::strtoul(e, nullptr, 10);
        if (v > 0 && v < flush_at) flush_at = (uint32_t)v;
    }
    const double range = Z.edges_max - Z.edges_min;
    const float hmin = (float)Z.edges_min, scale = (float)((double)nbins / range);
    uint32_t nb32 = (uint32_t)nbins;
    void *args[] = {&P, &Z.hnext.p, &Z.hedges.p, &nb32, const_cast<float *>(&hmin), const_cast<float *>(&scale), &flush_at, &bins, &count};
    MH_HIP(hipLaunchKernel(fn, dim3(nwg), dim3(64 * H64_WAVES), args, lds, c->stream));
    return 0;
}

int molar_hip_search_histogram_f64(molar_hip_ctx *c, const molar_hip_search_desc_f64 *q, double hmin, double hmax, size_t nbins,
                                   uint64_t *bins, uint64_t *out_count) {
    MH_TRY(hist64_begin(c, q, hmin, hmax, nbins, bins));
    molar_hip_search64_state &Z = *c->s64;
    const bool dev = is_device_ptr(bins);
    // hsum: [bins of a call with host bins][the pair count]
    MH_TRY(Z.hsum.reserve((nbins + 1) * 8));
    unsigned long long *hsum = Z.hsum.as<unsigned long long>();
    MH_HIP(hipMemsetAsync(dev ? hsum + nbins : hsum, 0, dev ? 8 : (nbins + 1) * 8, c->stream));
    MH_TRY(hist64_frame(c, q, nbins, dev ? reinterpret_cast<unsigned long long *>(bins) : hsum, hsum + nbins));
    MH_HIP(hipGetLastError());
    if (dev && !out_count) return MOLAR_HIP_OK;      // the kernel may still run: molar_hip_synchronize before reading the bins
    if (dev) {
        unsigned long long tot = 0;
        MH_HIP(hipMemcpyAsync(&tot, hsum + nbins, 8, hipMemcpyDeviceToHost, c->stream));
        MH_HIP(hipStreamSynchronize(c->stream));
        *out_count = tot;
        return MOLAR_HIP_OK;
    }
    std::vector<unsigned long long> h(nbins + 1);
    MH_HIP(hipMemcpyAsync(h.data(), hsum, (nbins + 1) * 8, hipMemcpyDeviceToHost, c->stream));
    MH_HIP(hipStreamSynchronize(c->stream));
    for (size_t b = 0; b < nbins; ++b) bins[b] += h[b];
    if (out_count) *out_count = h[nbins];
    return MOLAR_HIP_OK;
}

int molar_hip_search_histogram_frames_f64(molar_hip_ctx *c, const molar_hip_search_desc_f64 *q, size_t nframes, size_t xyz1_stride,
                                          size_t xyz2_stride, const double *boxes9, double hmin, double hmax, size_t nbins,
                                          uint64_t *bins) {
    MH_TRY(hist64_begin(c, q, hmin, hmax, nbins, bins));
    molar_hip_search64_state &Z = *c->s64;
    const bool dev = is_device_ptr(bins);
    MH_TRY(Z.hsum.reserve((nbins + 1) * 8));
    unsigned long long *hsum = Z.hsum.as<unsigned long long>();
    MH_HIP(hipMemsetAsync(dev ? hsum + nbins : hsum, 0, dev ? 8 : (nbins + 1) * 8, c->stream));
    for (size_t k = 0; k < nframes; ++k) {       // frame by frame: one slot-count read-back each
        molar_hip_search_desc_f64 f = *q;
        f.xyz1 = q->xyz1 ? q->xyz1 + k * xyz1_stride : nullptr;
        f.xyz2 = q->xyz2 ? q->xyz2 + k * xyz2_stride : nullptr;
        if (boxes9) f.box9 = boxes9 + 9 * k;
        MH_TRY(hist64_frame(c, &f, nbins, dev ? reinterpret_cast<unsigned long long *>(bins) : hsum, hsum + nbins));
        MH_HIP(hipGetLastError());
    }
    if (dev) return MOLAR_HIP_OK;                // molar_hip_synchronize before reading the bins
    std::vector<unsigned long long> h(nbins);
    MH_HIP(hipMemcpyAsync(h.data(), hsum, nbins * 8, hipMemcpyDeviceToHost, c->stream));
    MH_HIP(hipStreamSynchronize(c->stream));
    for (size_t b = 0; b < nbins; ++b) bins[b] += h[b];
    return MOLAR_HIP_OK;
}

// `within` as a set (see within64_flags_kernel): the prologue up to the grids, the partner lists, the flag pass, the flags
// counted per tile and scanned - one read-back: the size of the set (with the grid build's error flag).
int molar_hip_within_count_f64(molar_hip_ctx *c, const molar_hip_search_desc_f64 *q, uint64_t *out_count) {
    if (!c || !q) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "within_count_f64: null argument");
    if (q->kind != MOLAR_HIP_SEARCH_WITHIN)
        return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "within_count_f64: the request must be of kind MOLAR_HIP_SEARCH_WITHIN");
    const size_t nsel1 = q->idx1 ? q->n1 : q->natoms1, nsel2 = q->idx2 ? q->n2 : q->natoms2;
    const uint64_t nflags = q->ids_local ? nsel1 : (q->idx1 ? q->natoms1 : nsel1);       // the id range: one flag per id
    if (nflags >= 0xFFFFFFF0ull) return fail(MOLAR_HIP_ERR_TOO_LARGE, "within_count_f64: ids of %llu atoms exceed 32 bits", (unsigned long long)nflags);
    Prep64 R;
    bool empty = false;
    MH_TRY(prepare64_grids(c, q, &R, &empty));      // (the cached f64 search is gone: its buffers hold this request's grids)
    molar_hip_search64_state &Z = *c->s64;
    Z.w_nflags = nflags;
    Z.w_total = 0;
    if (out_count) *out_count = 0;
    struct { unsigned long long total; int err; } hs = {0ull, 0};
    if (nsel1 == 0 || nsel2 == 0 || nflags == 0) {
        MH_HIP(hipMemcpyAsync(&hs.err, R.err_dev, 4, hipMemcpyDeviceToHost, c->stream));
        MH_HIP(hipStreamSynchronize(c->stream));
        if (hs.err) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "search_f64: selection index out of range");
        Z.have_within = true;
        return MOLAR_HIP_OK;
    }
    MH_TRY(Z.box.reserve(sizeof R.box));
    MH_HIP(hipMemcpyAsync(Z.box.p, &R.box, sizeof R.box, hipMemcpyHostToDevice, c->stream));
    classify64(Z, R);
    const Params64 P = params64(Z);
    const uint32_t ncells = R.G.ncells;
    const uint64_t ntasks = (uint64_t)ncells * 14ull * 2ull, ntiles = (nflags + 2047) / 2048;
    const size_t flag_bytes = (size_t)((nflags + 3) & ~(uint64_t)3);
    MH_TRY(Z.w_flags.reserve(flag_bytes));
    MH_TRY(Z.w_tile_cnt.reserve((ntiles + 1) * 4));
    MH_TRY(Z.w_tile_off.reserve((ntiles + 1) * 8));
    MH_TRY(Z.w_part_cnt.reserve((size_t)ncells * 4));
    MH_TRY(Z.w_part.reserve((size_t)ncells * W64_MAX_PART * sizeof(uint2)));
    MH_HIP(hipMemsetAsync(Z.w_flags.p, 0, flag_bytes, c->stream));
    MH_HIP(hipMemsetAsync(Z.w_part_cnt.p, 0, (size_t)ncells * 4, c->stream));
    MH_HIP(hipMemsetAsync(Z.w_tile_cnt.p, 0, (ntiles + 1) * 4, c->stream));
    hipLaunchKernelGGL(within64_partners_kernel, dim3((unsigned)((ntasks + 255) / 256)), dim3(256), 0, c->stream, R.G, ntasks, R.startA, R.startB,
                       Z.w_part_cnt.as<uint32_t>(), Z.w_part.as<uint2>());
    // cells of many 64-row blocks get several waves (a share of the blocks each)
    uint32_t nsplit = (uint32_t)(((uint64_t)nsel1 / 64u) / ncells) + 1u;
    if (nsplit > 64u) nsplit = 64u;
    hipLaunchKernelGGL(within64_flags_kernel, dim3(ncells, nsplit), dim3(64), 0, c->stream, P, R.startA, R.startB, Z.w_part_cnt.as<uint32_t>(),
                       Z.w_part.as<uint2>(), Z.w_flags.as<uint8_t>(), nsplit);
    hipLaunchKernelGGL(flag_tile_count_kernel, dim3((unsigned)ntiles), dim3(256), 0, c->stream, Z.w_flags.as<uint8_t>(), nflags,
                       Z.w_tile_cnt.as<uint32_t>());
    MH_HIP(hipGetLastError());
    MH_TRY(device_exclusive_sum_u32_u64(c, Z.cub_tmp, Z.w_tile_cnt.as<uint32_t>(), Z.w_tile_off.as<unsigned long long>(), (size_t)ntiles + 1));
    MH_HIP(hipMemcpyAsync(&hs.total, Z.w_tile_off.as<unsigned long long>() + ntiles, 8, hipMemcpyDeviceToHost, c->stream));
    MH_HIP(hipMemcpyAsync(&hs.err, R.err_dev, 4, hipMemcpyDeviceToHost, c->stream));
    MH_HIP(hipStreamSynchronize(c->stream));
    if (hs.err) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "search_f64: selection index out of range");
    Z.w_total = hs.total;
    Z.have_within = true;
    if (out_count) *out_count = hs.total;
    return MOLAR_HIP_OK;
}

int molar_hip_within_fill_f64(molar_hip_ctx *c, uint64_t *ids) {
    if (!c || !c->s64 || !c->s64->have_within)
        return fail(MOLAR_HIP_ERR_NO_SEARCH, "no cached f64 within set: call molar_hip_within_count_f64 first");
    molar_hip_search64_state &Z = *c->s64;
    if (Z.w_total == 0) return MOLAR_HIP_OK;
    if (!ids) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "within_fill_f64: null output");
    MH_HIP(hipSetDevice(c->device));
    return flags_to_ids(c, Z.w_flags.as<uint8_t>(), Z.w_nflags, Z.w_tile_off.as<unsigned long long>(), Z.w_total, Z.w_out, ids, is_device_ptr(ids));
}

// SearchConnectivity (connectivity.rs:8-60) of the f64 single-selection search: count, scan and fill into the context's own
// columns, then the CSR on the device by the one build both precisions share (connectivity.hip: connectivity_begin, the
// entries written here, connectivity_finish) - molar_hip_search_connectivity_fill copies it out.
int molar_hip_search_connectivity_f64(molar_hip_ctx *c, const molar_hip_search_desc_f64 *q, uint64_t *out_rows, uint64_t *out_entries) {
    if (!c || !q) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "search_connectivity_f64: null argument");
    if (q->kind != MOLAR_HIP_SEARCH_SINGLE)
        return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "search_connectivity_f64: ids of one selection index the lists - the request must be of kind MOLAR_HIP_SEARCH_SINGLE");
    connectivity_forget(c);
    uint64_t npairs = 0;
    MH_TRY(molar_hip_search_count_f64(c, q, &npairs));
    const size_t nsel = q->idx1 ? q->n1 : q->natoms1;
    const uint64_t nrows = q->ids_local ? nsel : (q->idx1 ? q->natoms1 : nsel);
    if (nrows >= 0xFFFFFFF0ull) return fail(MOLAR_HIP_ERR_TOO_LARGE, "search_connectivity_f64: too many rows");
    const uint64_t nent = 2ull * npairs;
    if (nent >= 0x7FFFFFFFull) return fail(MOLAR_HIP_ERR_TOO_LARGE, "search_connectivity_f64: %llu list entries", (unsigned long long)nent);
    MH_TRY(fill64(c, nullptr, nullptr, nullptr, false));          // (i, j, d) into the context's columns; nothing leaves the device
    molar_hip_search64_state &Z = *c->s64;
    uint32_t *row_in = nullptr, *nb_in = nullptr;
    MH_TRY(connectivity_begin(c, nrows, npairs, &row_in, &nb_in));
    const unsigned nbP = (unsigned)((npairs + 255) / 256);
    if (nbP)
        hipLaunchKernelGGL(conn64_entries_kernel, dim3(nbP), dim3(256), 0, c->stream, Z.out_i.as<unsigned long long>(),
                           Z.out_j.as<unsigned long long>(), (unsigned long long)npairs, row_in, nb_in);
    MH_TRY(connectivity_finish(c));
    if (out_rows) *out_rows = nrows;
    if (out_entries) *out_entries = nent;
    return MOLAR_HIP_OK;
}

// Modify::unwrap_connectivity_dim (molar/src/modify.rs:72-131) with Float = f64: the neighbour search over the selection with
// LOCAL ids under full PBC whatever `pbc_dims` (:77-78) and the CSR on the device (molar_hip_search_connectivity_f64), the
// stack walk on the host with boxmath.hpp's closest_image over pbc_dims (unwrap_walk.hpp: the same template as the f32 entry).
int molar_hip_unwrap_connectivity_f64(molar_hip_ctx *c, double *xyz, size_t natoms, const uint64_t *idx, size_t n, const double *box9,
                                      double cutoff, uint8_t pbc_dims, uint64_t *group_offsets, uint64_t *group_ids, size_t *ngroups) {
    if (!c || !xyz) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "unwrap_connectivity_f64: null argument");
    if (!box9) return fail(MOLAR_HIP_ERR_NO_PBC, "no periodic box");                               // require_box (:76)
    const size_t nsel = idx ? n : natoms;
    if (nsel == 0) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "unwrap_connectivity_f64 of an empty selection");
    if (nsel >= 0x7FFFFFFFull) return fail(MOLAR_HIP_ERR_TOO_LARGE, "unwrap_connectivity_f64: %zu atoms exceed the 32-bit local ids", nsel);
    MH_HIP(hipSetDevice(c->device));
    double hb[9];
    MH_TRY(host_copy(c, box9, 9, hb));
    BoxD b;
    MH_TRY(box64_from_matrix(hb, &b));
    molar_hip_search_desc_f64 q{};
    q.kind = MOLAR_HIP_SEARCH_SINGLE;
    q.cutoff = cutoff;
    q.xyz1 = xyz; q.natoms1 = natoms; q.idx1 = idx; q.n1 = n;
    q.ids_local = 1;
    q.box9 = box9;
    q.pbc = MOLAR_HIP_PBC_FULL;
    uint64_t nrows = 0, nent = 0;
    MH_TRY(molar_hip_search_connectivity_f64(c, &q, &nrows, &nent));
    std::vector<uint64_t> off(nsel + 1, 0), adj((size_t)(nent ? nent : 1));
    MH_TRY(molar_hip_search_connectivity_fill(c, off.data(), adj.data()));
    // ---- the coordinates of the frame and the selection on the host
    const bool dev = is_device_ptr(xyz);
    std::vector<double> hostcopy;
    double *h = xyz;
    if (dev) {
        hostcopy.resize(natoms * 3);
        MH_HIP(hipMemcpyAsync(hostcopy.data(), xyz, natoms * 24, hipMemcpyDeviceToHost, c->stream));
        MH_HIP(hipStreamSynchronize(c->stream));
        h = hostcopy.data();
    }
    std::vector<uint64_t> hidx;
    if (idx && is_device_ptr(idx)) {
        hidx.resize(n);
        MH_HIP(hipMemcpy(hidx.data(), idx, n * 8, hipMemcpyDeviceToHost));
    }
    const uint64_t *ix = hidx.empty() ? idx : hidx.data();
    unwrap_walk<double, D3>(h, ix, nsel, b, pbc_dims & 7u, off.data(), adj.data(), group_offsets, group_ids, ngroups);
    if (dev) {
        MH_HIP(hipMemcpyAsync(xyz, hostcopy.data(), natoms * 24, hipMemcpyHostToDevice, c->stream));
        MH_HIP(hipStreamSynchronize(c->stream));
    }
    return MOLAR_HIP_OK;
}

}  // extern "C"
