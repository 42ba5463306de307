// search_shape.hpp — what follows from the shape of a search alone (mh::SearchShape, common.hpp): grid dimensions, kernel
// family, slot bound, the policy for wrapped pairs; and when a request may reuse the held grid of the `within` requests before
// it (mh::HeldGrid).  Host only and pure: no context, no HIP call (tests/cpp/test_search_shape.cpp runs them without a device).
#pragma once

#include <algorithm>
#include <cmath>
#include <cstring>

#include "common.hpp"

namespace mh {

// the kinds whose cutoff the request states (SINGLE, DOUBLE): hit history, small- and large-cell kernels, fused histogram
inline bool fixed_cutoff_kind(int kind) { return kind == MOLAR_HIP_SEARCH_SINGLE || kind == MOLAR_HIP_SEARCH_DOUBLE; }

inline uint64_t grid_cells(const SearchShape &s) { return (uint64_t)s.dims[0] * s.dims[1] * s.dims[2]; }

// Grid::from_cutoff_and_extents (distance_search.rs:103-110): s.dims from s.cutoff and the extents
inline int dims_from_extents(SearchShape &s, const float ext[3]) {
    double cells = 1.0;
    for (int d = 0; d < 3; ++d) {
        const float q = std::floor(ext[d] / s.cutoff);
        uint64_t n = (q > 0.0f) ? (q >= 4.0e9f ? 4000000000ull : (uint64_t)q) : 0ull;   // `as usize` saturates
        if (n < 1) n = 1;
        s.dims[d] = (uint32_t)n;
        cells *= (double)n;
    }
    if (cells > 1.0e8)
        return fail(MOLAR_HIP_ERR_TOO_LARGE, "search grid %u x %u x %u has too many cells (cutoff %g)", s.dims[0],
                    s.dims[1], s.dims[2], (double)s.cutoff);
    return 0;
}

// The cells a set's mean population is judged by: the OCCUPIED cells where the last search of this shape has told
// (occ_use, latched by prepare_search - a slab or a solute in a mostly empty periodic box), all cells otherwise.
inline uint64_t judged_cells(const SearchShape &s, int set) {
    const uint64_t all = grid_cells(s);
    return s.occ_use[set] ? std::min<uint64_t>(s.occ_use[set], all) : all;
}

// Frames of small cells (contact / hydrogen-bond cutoffs) of the fixed-cutoff kinds go to pair_small.hip: 16 lanes per slot up to 13
// atoms per cell on average, 32 up to 19, 0 = the regular kernels (1M atoms: 0.30 / 0.35 / 0.40 / 0.45 / 0.50 nm take 1.30 / 1.00 /
// 0.89 / 1.01 / 0.99 ms per frame against 2.91 / 2.14 / 1.66 / 1.30 / 1.07; at 0.55 nm - 23 atoms per cell - the regular kernels win).
// Decided from the sets' sizes and the grid alone: the grid build (no spatial order for these) and both passes agree on it.
inline int small_cell_lanes(const SearchShape &s) {
#ifdef MH_NO_SMALL_CELLS
    return 0;           // (A/B builds: every frame through the regular kernels)
#endif
    if (!fixed_cutoff_kind(s.kind)) return 0;
    int lanes = 16;
    const int nsets = s.kind == MOLAR_HIP_SEARCH_SINGLE ? 1 : 2;
    for (int k = 0; k < nsets; ++k) {
        const uint64_t cells = judged_cells(s, k), n = s.set[k].n;
        const int l = n <= 13ull * cells ? 16 : (n <= 19ull * cells ? 32 : 0);
        lanes = (l == 0 || lanes == 0) ? 0 : std::max(lanes, l);
    }
    return lanes;
}

// The kernel family of the count and fill passes, as molar_hip_search_cell_kernels reports it: 16 / 32 = pair_small.hip with that
// many lanes per slot, 0 = the regular kernels, -1 = the wide instances (more than 448 atoms per judged cell of the second set on
// average, i.e. cells above 512 are common: 128 registers per lane, up to 16 chunks of the second cell resident), -2 = the huge
// ones (more than 1000: cells above 1024 atoms are the rule, 256 registers per lane, up to 2048 atoms resident - pair_k7.hip).
inline int pair_family(const SearchShape &s) {
    if (const int lanes = small_cell_lanes(s)) return lanes;
    if (!fixed_cutoff_kind(s.kind)) return 0;
    const int b = s.kind == MOLAR_HIP_SEARCH_SINGLE ? 0 : 1;
    const uint64_t cells = judged_cells(s, b), n = s.set[b].n;
    return n > 1000ull * cells ? -2 : (n > 448ull * cells ? -1 : 0);
}

// Does the count pass of this search record hit history for the fill pass to replay?  The fixed-cutoff kinds do - except on
// frames of small cells: pair_small.hip evaluates in both passes and never touches the buffer, so its plan accounts for none
// (a plan that did made the first resident frame of such a trajectory grow the buffer and run count and fill again for nothing).
inline bool records_hit_history(const SearchShape &s) { return fixed_cutoff_kind(s.kind) && small_cell_lanes(s) == 0; }

// Grids of large cells (more than 384 atoms per cell on average, i.e. cells of more than KREG * 64 atoms are the rule) order their
// atoms by a stable device sort instead of ranking every atom against its whole cell (build_grid); the fused histogram walks
// such cells in blocks, and its batched form leaves them to the frame-by-frame path.
inline bool sorted_by_device_sort(uint64_t n, uint64_t ncells) { return n > 384ull * ncells; }

// the shape a grid's occupancy is remembered for
inline unsigned long long occ_key_of(const SearchShape &s) {
    unsigned long long h = 1469598103934665603ull;
    auto mix = [&](unsigned long long v) { h = (h ^ v) * 1099511628211ull; };
    mix((unsigned long long)s.kind + 1u); mix(s.set[0].n); mix(s.kind == MOLAR_HIP_SEARCH_SINGLE ? 0u : s.set[1].n);
    mix(s.dims[0]); mix(s.dims[1]); mix(s.dims[2]); mix(s.use_box ? 1u : 2u);
    return h ? h : 1ull;
}

// plan entries: 14 half-shell masks per cell, both orders of the two grids
inline uint64_t plan_entries(const SearchShape &s) { return grid_cells(s) * 14ull * (s.kind != MOLAR_HIP_SEARCH_SINGLE ? 2ull : 1ull); }

// Host-side upper bound of the slot count.  Every set-1 cell is the first cell of at most 14 (two grids: 28) tasks, so
// sum_t ceil(n1(t)/64) <= mult*N1/64 + ntasks; entries wrapping in all three dims of a triclinic box use 2-row (<= 1024 rows)
// or 8-row slots: <= 28 tasks of <= 512 slots.  hist_plan: the one-kernel plan of the fused histogram cuts same-cell entries
// into 32-row slots, one such entry per cell.
inline uint64_t slots_bound(const SearchShape &s, bool hist_plan) {
    const uint64_t n0 = s.set[0].n;
    uint64_t bound = (s.kind != MOLAR_HIP_SEARCH_SINGLE ? 28ull : 14ull) * ((n0 + 63ull) / 64ull) + plan_entries(s) + 28ull * 512ull;
    if (hist_plan) bound += (n0 + 31ull) / 32ull + grid_cells(s);
    return bound;
}

// Plans of at most this many entries (+ terminator) go through plan_tiles_kernel / plan_slots_kernel on the main stream
constexpr uint64_t FPLAN_MAX_TASKS = 1ull << 22;

// Are the slots of this search cut from the LIVE rows of its plan entries (live_rows_kernel, search.hip)?  The regular family of
// the fixed-cutoff kinds only - the instances of pair_kernel compiled with the gather - and plans that take plan_tiles_kernel /
// plan_slots_kernel; everything else (small-, wide- and huge-cell families, vdW and `within`, the fused histogram's own plans, the
// contact kernels, the f64 search) walks consecutive slots.  And frames whose first cells hold 96 atoms on average over ALL cells
// of the grid: the liveness kernel costs one wave per plan entry, empty entries included, while slots are only saved where an
// entry has more than one (measured, profiles/live_rows_ab.txt sections 1, 4 and 7: 1M atoms at 1.2 / 1.0 nm - 261 / 108 atoms per cell - gain 4-6 %
// / hold; at 0.8 / 0.6 nm - 57 / 32 per cell, one slot per entry as a rule - the kernel's 1.9e5 / 4.4e5 waves beside the count
// pass cost 1.4 / 30 %, and a slab in a mostly empty box up to 2x).  Plans of at most 8192 entries - the liveness kernel is then
// at most one resident round of one-wave workgroups (256 CUs x 32 waves) - qualify whatever their density: frames without a box,
// whose grid is padded by a shell of empty cells, are such.  The masks (68 bytes per entry, at most 28 entries per cell) thus stay below
// 20 bytes per atom.
constexpr uint32_t LIVE_ROW_GROUPS = 8;        // 64-row groups per entry: first cells of up to 512 atoms (KREG chunks)
inline bool live_row_slots(const SearchShape &s) {
    return fixed_cutoff_kind(s.kind) && pair_family(s) == 0 && plan_entries(s) + 1 <= FPLAN_MAX_TASKS &&
           (plan_entries(s) <= 8192ull || (uint64_t)s.set[0].n >= 96ull * grid_cells(s));
}
// bytes of a generation's live-row buffer: the mask words of every entry, then the entries' live counts
inline size_t live_rows_mask_words(const SearchShape &s) { return (size_t)plan_entries(s) * LIVE_ROW_GROUPS; }
inline size_t live_rows_bytes(const SearchShape &s) { return live_rows_mask_words(s) * 8u + (size_t)plan_entries(s) * 4u; }

// ---- the held grid of `within` requests (mh::HeldGrid, common.hpp; molar_hip_within_hold)
// A first set in HOST memory is staged, so the hold would serve a copy: a fingerprint of the caller's array (its two ends and
// 512 atoms spread over it - not every atom: the caller's promise covers the rest) tells an array updated in place, or a new one
// that the allocator put at the old address, from the one that was staged.  Never 0, which stands for "device memory, read in place".
inline uint64_t held_fingerprint(const float *xyz, size_t natoms) {
    uint64_t fp = 0xcbf29ce484222325ull;
    auto mix = [&](size_t atom) {
        uint32_t w[3];
        std::memcpy(w, xyz + 3 * atom, 12);
        for (int k = 0; k < 3; ++k) fp = (fp ^ w[k]) * 0x100000001b3ull;
    };
    const size_t n = natoms, step = n > 512 ? n / 512 : 1;
    for (size_t a = 0; a < n && a < 64; ++a) mix(a);
    for (size_t a = 0; a < n; a += step) mix(a);
    for (size_t a = n > 64 ? n - 64 : 0; a < n; ++a) mix(a);
    return fp | 1ull;
}

// Does the request name the held first set?  Same grid generation, same pointers and sizes, same ids, same box and periodicity,
// the same fingerprint (`s`: kind-independent part of the request's shape - set, use_box, pbc, box - as prepare_search has it
// BEFORE staging: a request that passes keeps the staged coordinates).
inline bool held_names_request(const HeldGrid &h, const molar_hip_search_desc &q, const SearchShape &s, uint64_t fp) {
    return h.valid && h.fp == fp && h.set == s.set && h.xyz == q.xyz1 && h.natoms == q.natoms1 && h.idx == q.idx1 && h.n == q.n1 &&
           h.ids_local == q.ids_local && h.use_box == s.use_box && h.pbc == s.pbc &&
           (!s.use_box || std::memcmp(&h.box, &s.box, sizeof s.box) == 0);
}

// Does the search come to the same cells?  (The cutoff and, without a box, the caller's bounds decide the grid: asked once
// dims_from_extents has run.)
inline bool held_same_cells(const HeldGrid &h, const SearchShape &s) {
    bool same = h.dims[0] == s.dims[0] && h.dims[1] == s.dims[1] && h.dims[2] == s.dims[2];
    for (int d = 0; d < 3 && !s.use_box; ++d) same = same && h.lower[d] == s.lower[d] && h.upper[d] == s.upper[d];
    return same;
}

// the record of the grid this request builds for its first set
inline HeldGrid held_remember(const molar_hip_search_desc &q, const SearchShape &s, uint64_t fp) {
    HeldGrid h;
    h.valid = true;
    h.set = s.set;
    h.fp = fp;
    h.xyz = q.xyz1; h.idx = q.idx1; h.natoms = q.natoms1; h.n = q.n1;
    h.ids_local = q.ids_local;
    h.use_box = s.use_box; h.pbc = s.pbc; h.box = s.box;
    for (int d = 0; d < 3; ++d) { h.dims[d] = s.dims[d]; h.lower[d] = s.lower[d]; h.upper[d] = s.upper[d]; }
    return h;
}

// How the pair kernels treat entries that wrap around the box (SearchParams carries these six under the same names).
struct WrapPolicy {
    uint32_t wrap_kind;        // 1 diagonal, 2 upper triangular (GROMACS-style boxes), 3 general: which products a wrapped pair may skip
    uint32_t prune_wrapped;    // rows of wrapped entries are pruned against the image box
    uint32_t approx_wrapped;   // wrapped candidates are classified by the plain distance to the image cell outside [band_lo, band_hi]
    float band_lo, band_hi;
    float prune_limit2;        // (cutoff + pruning margin)^2
};

inline WrapPolicy wrapped_pair_policy(const SearchShape &s) {
    WrapPolicy W{};
    const float cutoff2 = s.cutoff * s.cutoff;
    // zero pattern shared by the matrix and its inverse -> which products a wrapped pair may skip
    W.wrap_kind = 3u;   // WK_GENERAL
    if (s.use_box) {
        const float *m = s.box.m, *iv = s.box.inv;
        auto z = [&](int k) { return m[k] == 0.0f && iv[k] == 0.0f; };
        const bool lower_zero = z(1) && z(2) && z(5);            // (1,0) (2,0) (2,1)
        const bool upper_zero = z(3) && z(6) && z(7);            // (0,1) (0,2) (1,2)
        if (lower_zero && upper_zero) W.wrap_kind = 1u;          // WK_DIAG
        else if (lower_zero) W.wrap_kind = 2u;                   // WK_UPPER (GROMACS-style boxes)
    }
    // image-box pruning of wrapped entries argues with n_d = round(f_d) in {-1,0,1}; keep the exhaustive
    // path on degenerate grids (a periodic dimension with fewer than 3 cells): they are tiny anyway
    W.prune_wrapped = 0u;
    if (s.use_box) {
        bool ok = true;
        for (int d = 0; d < 3; ++d)
            if (((s.pbc >> d) & 1u) && s.dims[d] < 3u) ok = false;
        W.prune_wrapped = ok ? 1u : 0u;
    }
    // Wrapped entries: classify with the plain distance to the image cell (b + S - a), decide exactly inside a band
    // around cutoff^2, and prune rows against the image box with a margin.  How far can the two evaluations of a
    // wrapped difference vector disagree?  u = 2^-24, L = largest |coordinate| the box allows (lab extents, box
    // vectors), kappa = || |M| |M^-1| ||_inf (1 for a rectangular box, grows with shear):
    //   reference (periodic_box.rs:291-297): v = p2 - p1 (error <= u L per component), f = inv v (3 products, 2 sums:
    //     <= 4u sum|inv||v| per component), s = M f (the error of f amplified by |M|: <= 4u kappa L, plus 4u L of
    //     its own roundings)                                            => <= (4 kappa + 5) u L per component
    //   approximate: S summed from box columns (<= 2u L), b + S (u L), - a (u L)   => <= 4u L per component
    // so a component of the difference vector differs by at most e = (4 kappa + 9) u L, a distance by sqrt(3) e, and
    // d2 near cutoff^2 by 2 sqrt(3) rc e, i.e. by 2 sqrt(3) (4 kappa + 9) u L/rc relative to cutoff^2.  The band is
    // 2e-4 plus FOUR times that; the pruning margin is 1e-3 nm plus four times sqrt(3) e.  Both therefore scale with
    // the box size AND its shear; boxes for which the band would exceed 5 % of cutoff^2 or the margin 5 % of the
    // cutoff take the exact path for every wrapped candidate.
    W.approx_wrapped = 0u;
    W.band_lo = W.band_hi = cutoff2;
    float margin = 1.0e-3f;
    if (s.use_box) {
        bool ok = (uint64_t)s.set[0].n + (uint64_t)s.set[1].n < (1ull << 26);   // (row<<26 | position) packing
        float ext[3], lmax = 0.f;
        molar_hip_box_lab_extents(&s.box, ext);
        for (int d = 0; d < 3; ++d) {
            if (((s.pbc >> d) & 1u) && s.dims[d] < 4u) ok = false;   // round(f_d) must be +-1 for wrapped pairs
            lmax = std::fmax(lmax, std::fabs(ext[d]));
            for (int k = 0; k < 3; ++k) lmax = std::fmax(lmax, std::fabs(s.box.m[3 * k + d]));
        }
        // atoms sit inside the cell along periodic dims, so a coordinate is bounded by the sum of the |box vectors|
        float lsum = 0.f;
        for (int d = 0; d < 3; ++d) {
            float row = 0.f;
            for (int k = 0; k < 3; ++k) row += std::fabs(s.box.m[3 * k + d]);
            lsum = std::fmax(lsum, row);
        }
        lmax = std::fmax(lmax, lsum);
        double kappa = 0.0;
        for (int i = 0; i < 3; ++i) {
            double row = 0.0;
            for (int j = 0; j < 3; ++j) {
                double e = 0.0;
                for (int k = 0; k < 3; ++k) e += std::fabs((double)s.box.m[3 * k + i]) * std::fabs((double)s.box.inv[3 * j + k]);
                row += e;
            }
            kappa = std::fmax(kappa, row);
        }
        const double u = 5.9604645e-8;
        const double e = (4.0 * kappa + 9.0) * u * (double)lmax;                   // per-component disagreement bound
        const double rel = 2.0e-4 + 4.0 * 2.0 * 1.7320508 * e / (double)s.cutoff;
        margin = (float)(1.0e-3 + 4.0 * 1.7320508 * e);
        if (!(margin < 0.05f * s.cutoff) || !std::isfinite(kappa)) {
            W.prune_wrapped = 0u;
            ok = false;
        }
        if (ok && rel < 0.05) {
            W.approx_wrapped = 1u;
            W.band_lo = cutoff2 * (float)(1.0 - rel);
            W.band_hi = cutoff2 * (float)(1.0 + rel);
        }
    }
    const float lim = s.cutoff + margin;
    W.prune_limit2 = lim * lim;
    return W;
}

}  // namespace mh
