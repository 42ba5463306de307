// within.hip - `within` as a set (molar_hip_within_count / _fill) and the switch of the held grid (molar_hip_within_hold): a
// consumer of the f32 search.  The request is prepared by the search (search_core.hpp: grids, no plan); the kernels here walk
// the cells themselves.  What the set keeps between count and fill is this unit's state, behind molar_hip_ctx::within.
#include <algorithm>
#include <vector>

#include "common.hpp"
#include "csr_kernels.hpp"
#include "pair_kernels.hpp"
#include "search_core.hpp"
#include "search_shape.hpp"

using namespace mh;
using namespace mh::pairk;

struct molar_hip_within_state {
    DevBuf w_list;             // small second sets: ids found, in the order they were found (within_small_kernel)
    bool w_small = false;      // the cached within set was made by the small path (the list holds it)
    uint64_t w_list_dirty = 0; // flags set through the list by the previous small-path call, to be cleared before the next
    bool w_flags_all_dirty = false;   // the previous call went through the partner lists: any flag may be set
    DevBuf w_flags, w_part_cnt, w_part, w_tile_cnt, w_tile_off;
    uint64_t within_nflags = 0, within_total = 0;
    bool have_within = false;
};

void mh::within_release(molar_hip_ctx *c) { release_state(c->within); }

namespace {

// ================================================================= `within` as a set (selection/ast.rs:589-631)
//
// What a caller of distance_search_within(_pbc) keeps is the SET of first-set atoms with a second-set atom in range: the
// raw stream (one id per plan entry in which the atom has a hit, :271-322,519-598) goes through SortedSet::from_unsorted
// (selection_expr.rs:112).  A set needs no stream, no offsets and no second pass - and an atom that has been found needs
// no further candidates, in ANY of its up to 28 plan entries:
//  * within_partners_kernel inverts the plan (same decode_task as every other kernel, so the same wrap / drop rules and
//    the same incomplete neighbourhoods of sheared boxes): per first-set cell the list of (second-set cell, wrap dims)
//    it meets, from both halves of every entry;
//  * within_flags_kernel: one wave per (first-set cell, share of its 64-row blocks) walks that list with a mask of the
//    rows still looking; per partner the rows that cannot reach its bounding box are left out (plain entries: the
//    exact f32 lower bound of run_fast), the partner's atoms are loaded 64 at a time, every remaining row is fetched
//    with one LDS broadcast and tested with the reference's arithmetic (PeriodicBox::distance_squared over the entry's
//    wrap dims for wrapped entries); a row leaves the mask at its first hit, the wave leaves the list when the mask is
//    empty; found rows set flags[id];
//  * ids are indices into a sorted selection (or 0..n), so the flagged positions in ascending order ARE the sorted,
//    de-duplicated result: a count per 2048-flag tile, a scan of the tile counts and one compaction pass.
constexpr uint32_t WITHIN_MAX_PART = 28;
// every (mask, half) pair of the plan has exactly one first-set cell as its origin: a cell is the first cell of at most
// 14 masks x 2 halves entries.  A plan with more masks or another stencil must grow the lists with it.
static_assert(WITHIN_MAX_PART == 2u * sizeof(pairk::MASKS) / sizeof(pairk::MASKS[0]), "partner lists are sized for the plan's stencil");

__global__ void __launch_bounds__(256) within_partners_kernel(const SearchParams *__restrict__ Pp, uint32_t *__restrict__ part_cnt,
                                                              uint32_t *__restrict__ part) {
    const SearchParams &P = *Pp;
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (t >= P.ntasks) return;
    const Task T = decode_task<MOLAR_HIP_SEARCH_WITHIN, false>(P, t);
    if (!T.valid) return;
    const uint32_t s = atomicAdd(&part_cnt[T.ca], 1u);
    if (s < WITHIN_MAX_PART) part[(size_t)T.ca * WITHIN_MAX_PART + s] = T.cb | (T.wrap << 28);
}

// `within` against a SMALL second set (a ligand, a few residues: selection/ast.rs:589-631 on the shapes of
// molar/benches/within_size_bench.rs): the plan is walked from the second set's side.  One wave per (second-set atom, one of
// the 28 (mask, half) combinations); the wave of the FIRST atom of each occupied second-set cell finds the one plan entry
// that has this cell as its second cell through that combination (decode_task on the candidate entry index: the
// reference's own wrap / drop rules decide, nothing is re-derived), and tests the rows of the entry's first cell, 64 at a
// time, lanes = rows, against the cell's few atoms with the reference's arithmetic (distance_squared over the entry's wrap
// dims for wrapped entries).  A row that finds a partner sets its flag byte with an atomic OR on the containing word; the
// lane that turned it on appends the id to a list - the result, unsorted, with its length in memory.  No partner lists over
// all cells, no pass over the whole plan, no flag scan: two launches and one read-back for `within 0.8 of <20 atoms>`.
__global__ void __launch_bounds__(64) within_small_kernel(const SearchParams *__restrict__ Pp, uint32_t n2, uint32_t ncells, uint32_t by_cell,
                                                          uint32_t *__restrict__ flags32, uint32_t *__restrict__ list,
                                                          uint32_t *__restrict__ list_n) {
    const SearchParams &P = *Pp;
    const uint32_t lane = threadIdx.x;
    const uint32_t j = blockIdx.x / 28u, combo = blockIdx.x % 28u;
    uint32_t cell;
    if (by_cell) {                  // fewer cells than second-set atoms (large cutoffs): one wave per (cell, combination)
        cell = j;
        if (cell >= ncells || P.csb[cell + 1] == P.csb[cell]) return;
    } else {
        if (j >= n2) return;
        // the cell of sorted second-set atom j: the last cell whose start is <= j (binary search over cell_start)
        uint32_t lo = 0u, hi = ncells;
        while (hi - lo > 1u) {
            const uint32_t mid = (lo + hi) >> 1;
            if (P.csb[mid] <= j) lo = mid;
            else hi = mid;
        }
        cell = lo;
        if (P.csb[cell] != j) return;                               // not the first atom of its cell
    }
    const uint32_t m = combo >> 1, half = combo & 1u;
    const uint32_t cz = cell / (P.dx * P.dy), cy = (cell / P.dx) % P.dy, cx = cell % P.dx;
    const uint32_t cc[3] = {cx, cy, cz}, dims[3] = {P.dx, P.dy, P.dz};
    uint32_t home[3];
    for (int d = 0; d < 3; ++d) {
        const uint32_t off = half ? MASKS[m][d] : MASKS[m][3 + d];   // offset of the entry's SECOND cell from its home cell
        if (cc[d] >= off) home[d] = cc[d] - off;
        else if ((P.pbc >> d) & 1u) home[d] = dims[d] - 1u;          // reached across the periodic boundary
        else return;
    }
    const uint64_t cidx = ((uint64_t)home[0] * P.dy + home[1]) * P.dz + home[2];          // x outer, z inner
    const uint64_t t = (cidx * 14ull + m) * 2ull + half;
    if (t >= P.ntasks) return;
    const Task T = decode_task<MOLAR_HIP_SEARCH_WITHIN, false>(P, t);
    if (!T.valid || T.cb != cell) return;
    const float cutoff2 = P.cutoff2;
    const bool wrapped = P.use_box && T.wrap != 0u;
    float4 lo4 = make_float4(0.f, 0.f, 0.f, 0.f), hi4 = lo4;
    if (!wrapped) {
        lo4 = gload4(P.aabb_b, 2 * T.cb);
        hi4 = gload4(P.aabb_b, 2 * T.cb + 1);
    }
    // (blockIdx.y: a share of the first cell's 64-row blocks - large cutoffs mean cells of thousands of atoms)
    for (uint32_t i0 = blockIdx.y * 64u; i0 < T.n1; i0 += gridDim.y * 64u) {
        const bool have = i0 + lane < T.n1;
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
        if (have) a = gload4(P.sa, T.a0 + i0 + lane);
        bool look = have;
        if (!wrapped) look = look && !(aabb_d2(a.x, a.y, a.z, lo4.x, lo4.y, lo4.z, hi4.x, hi4.y, hi4.z) > cutoff2);
        if (__builtin_amdgcn_ballot_w64(look) == 0ull) continue;
        bool found = false;
        for (uint32_t k0 = 0; k0 < T.n2; k0 += 64u) {
            // 64 partner atoms at a time into the lanes, handed round with v_readlane (one load per 64 partners, not one each)
            float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
            if (k0 + lane < T.n2) q = gload4(P.sb, T.b0 + k0 + lane);
            const uint32_t cnt = T.n2 - k0 < 64u ? T.n2 - k0 : 64u;
            for (uint32_t kk = 0; kk < cnt; ++kk) {
                const float bx = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(q.x), kk));
                const float by = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(q.y), kk));
                const float bz = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(q.z), kk));
                const float dx = bx - a.x, dy = by - a.y, dz = bz - a.z;                   // p2 - p1
                const float d2 = wrapped ? wrapped_d2_exact<true>(P, T.wrap, dx, dy, dz)    // :306-321
                                         : (dx * dx + dy * dy) + dz * dz;                  // :281-292
                found = found || (look && d2 <= cutoff2);
                if ((kk & 7u) == 7u && __builtin_amdgcn_ballot_w64(look && !found) == 0ull) break;      // every row has its partner (:289, :318)
            }
            if (__builtin_amdgcn_ballot_w64(look && !found) == 0ull) break;
        }
        if (found) {
            const uint32_t id = __float_as_uint(a.w);
            const uint32_t bit = 1u << (8u * (id & 3u));
            const uint32_t old = atomicOr(&flags32[id >> 2], bit);
            if (!(old & bit)) list[atomicAdd(list_n, 1u)] = id;
        }
    }
}

// clears the flags a small-path call set (through its list) instead of a memset over every flag
__global__ void __launch_bounds__(256) within_clear_kernel(const uint32_t *__restrict__ list, uint32_t n, uint8_t *__restrict__ flags) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) flags[list[i]] = 0u;
}

__global__ void __launch_bounds__(64) within_flags_kernel(const SearchParams *__restrict__ Pp, const uint32_t *__restrict__ part_cnt,
                                                          const uint32_t *__restrict__ part, uint8_t *__restrict__ flags,
                                                          uint32_t nsplit) {
    __shared__ float4 la[64];
    const SearchParams &P = *Pp;
    const uint32_t lane = threadIdx.x, ca = blockIdx.x, split = blockIdx.y;
    const uint32_t a0 = P.csa[ca], n1 = P.csa[ca + 1] - a0;
    uint32_t np = part_cnt[ca];
    if (n1 == 0u || np == 0u) return;
    if (np > WITHIN_MAX_PART) np = WITHIN_MAX_PART;
    const float cutoff2 = P.cutoff2;
    for (uint32_t i0 = split * 64u; i0 < n1; i0 += nsplit * 64u) {
        const uint32_t rows = n1 - i0 < 64u ? n1 - i0 : 64u;
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
        if (lane < rows) a = gload4(P.sa, a0 + i0 + lane);
        __builtin_amdgcn_wave_barrier();
        la[lane] = a;
        __builtin_amdgcn_wave_barrier();
        const unsigned long long full = rows == 64u ? ~0ull : ((1ull << rows) - 1ull);
        unsigned long long live = full;                      // rows still looking for a partner atom
        for (uint32_t pi = 0; pi < np && live; ++pi) {
            const uint32_t e = __builtin_amdgcn_readfirstlane(part[(size_t)ca * WITHIN_MAX_PART + pi]);
            const uint32_t cb = e & 0x0FFFFFFFu, wrap = e >> 28;
            const uint32_t b0 = P.csb[cb], n2 = P.csb[cb + 1] - b0;
            unsigned long long cand = live;
            if (!wrap) {       // rows that cannot reach the partner's box: the f32 lower bound of every d2 of the row (run_fast)
                const float4 lo = gload4(P.aabb_b, 2 * cb), hi = gload4(P.aabb_b, 2 * cb + 1);
                cand &= __builtin_amdgcn_ballot_w64(!(aabb_d2(a.x, a.y, a.z, lo.x, lo.y, lo.z, hi.x, hi.y, hi.z) > cutoff2));
            }
            for (uint32_t j0 = 0; j0 < n2 && cand; j0 += 64u) {
                const bool inb = j0 + lane < n2;
                float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
                if (inb) q = gload4(P.sb, b0 + j0 + lane);
                unsigned long long rm = cand;
                while (rm) {
                    const uint32_t r = (uint32_t)__builtin_ctzll(rm);
                    rm &= rm - 1ull;
                    const float4 p = lload4(la, r);                                  // one broadcast ds_read per row
                    const float dx = q.x - p.x, dy = q.y - p.y, dz = q.z - p.z;      // p2 - p1
                    const float d2 = wrap ? wrapped_d2_exact<true>(P, wrap, dx, dy, dz)    // :306-321 (distance_squared over the entry's dims)
                                          : (dx * dx + dy * dy) + dz * dz;          // :281-292
                    if (__builtin_amdgcn_ballot_w64(inb && d2 <= cutoff2)) {         // `break` at the first hit (:289, :318)
                        live &= ~(1ull << r);
                        cand &= ~(1ull << r);
                    }
                }
            }
        }
        const unsigned long long found = full & ~live;
        if ((found >> lane) & 1ull) flags[__float_as_uint(a.w)] = 1u;
    }
}

}  // namespace

extern "C" {

int molar_hip_within_count(molar_hip_ctx *c, const molar_hip_search_desc *q, uint64_t *out_count) {
    if (!c || !q) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "within: null argument");
    if (q->kind != MOLAR_HIP_SEARCH_WITHIN) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "within: the request must be of kind MOLAR_HIP_SEARCH_WITHIN");
    molar_hip_within_state &W = state_of(c->within);
    W.have_within = false;
    SearchCall call;
    call.plan = false;                            // no slots, no offsets: this path walks cells
    call.size_masks = false;
    call.within_set = true;
    bool degenerate;                              // (never: a WITHIN request is no vdW request)
    MH_TRY(prepare_search(c, q, call, &degenerate));
    c->have_search = false;                       // not a cached search for the fill calls of the stream form
    const SearchShape &cur = c->cur;
    const uint64_t nflags = q->ids_local ? cur.set[0].n : (q->idx1 ? q->natoms1 : cur.set[0].n);
    W.within_nflags = nflags;
    W.within_total = 0;
    if (out_count) *out_count = 0;
    if (cur.set[0].n == 0 || cur.set[1].n == 0 || nflags == 0) {
        W.have_within = true;
        return MOLAR_HIP_OK;
    }
    const uint32_t ncells = (uint32_t)grid_cells(cur);
    const uint64_t ntiles = (nflags + 2047) / 2048;
    const size_t flag_bytes = (nflags + 3) & ~(size_t)3;
    const bool fresh_flags = W.w_flags.cap < flag_bytes;
    MH_TRY(W.w_flags.reserve(flag_bytes));
    MH_TRY(W.w_tile_cnt.reserve((ntiles + 1) * 4));
    MH_TRY(W.w_tile_off.reserve((ntiles + 1) * 8));
    MH_TRY(upload_search_params(c, cur));
    // flags: all zero between calls.  A small-path call leaves only the flags of its list set: those are cleared through the list.
    if (fresh_flags || W.w_flags_all_dirty) MH_HIP(hipMemsetAsync(W.w_flags.p, 0, flag_bytes, c->stream));
    else if (W.w_list_dirty)
        hipLaunchKernelGGL(within_clear_kernel, dim3((unsigned)((W.w_list_dirty + 255) / 256)), dim3(256), 0, c->stream, W.w_list.as<uint32_t>() + 1,
                           (uint32_t)W.w_list_dirty, W.w_flags.as<uint8_t>());
    W.w_flags_all_dirty = false;
    W.w_list_dirty = 0;
    W.w_small = (uint64_t)cur.set[1].n * 28ull <= (1ull << 17);           // <= 4681 second-set atoms: one wave per (atom, combination)
    if (W.w_small) {
        MH_TRY(W.w_list.reserve((nflags + 1) * 4));
        MH_HIP(hipMemsetAsync(W.w_list.p, 0, 4, c->stream));               // word 0: the list's length, then the ids
        // cells of many 64-row blocks (large cutoffs) get several waves per (cell, combination)
        uint32_t wsplit = (uint32_t)(((uint64_t)cur.set[0].n / 64u) / ncells) + 1u;
        if (wsplit > 64u) wsplit = 64u;
        const uint32_t by_cell = ncells < cur.set[1].n ? 1u : 0u;
        hipLaunchKernelGGL(within_small_kernel, dim3((by_cell ? ncells : cur.set[1].n) * 28u, wsplit), dim3(64), 0, c->stream, c->params.as<SearchParams>(), cur.set[1].n, ncells, by_cell,
                           W.w_flags.as<uint32_t>(), W.w_list.as<uint32_t>() + 1, W.w_list.as<uint32_t>());
        MH_HIP(hipGetLastError());
        uint32_t tot = 0;
        MH_TRY(read_back(c, &tot, W.w_list.p, 4));
        W.within_total = tot;
        W.w_list_dirty = tot;
        W.have_within = true;
        if (out_count) *out_count = tot;
        return MOLAR_HIP_OK;
    }
    W.w_flags_all_dirty = true;
    MH_TRY(W.w_part_cnt.reserve((size_t)ncells * 4));
    MH_TRY(W.w_part.reserve((size_t)ncells * WITHIN_MAX_PART * 4));
    MH_HIP(hipMemsetAsync(W.w_part_cnt.p, 0, (size_t)ncells * 4, c->stream));
    MH_HIP(hipMemsetAsync(W.w_tile_cnt.p, 0, (ntiles + 1) * 4, c->stream));
    hipLaunchKernelGGL(within_partners_kernel, dim3((unsigned)((cur.ntasks + 255) / 256)), dim3(256), 0, c->stream, c->params.as<SearchParams>(),
                       W.w_part_cnt.as<uint32_t>(), W.w_part.as<uint32_t>());
    // big cells get several waves (a share of their 64-row blocks each)
    uint32_t nsplit = (uint32_t)(((uint64_t)cur.set[0].n / 64u) / ncells) + 1u;
    if (nsplit > 64u) nsplit = 64u;
    hipLaunchKernelGGL(within_flags_kernel, dim3(ncells, nsplit), dim3(64), 0, c->stream, c->params.as<SearchParams>(),
                       W.w_part_cnt.as<uint32_t>(), W.w_part.as<uint32_t>(), W.w_flags.as<uint8_t>(), nsplit);
    hipLaunchKernelGGL(flag_tile_count_kernel, dim3((unsigned)ntiles), dim3(256), 0, c->stream, W.w_flags.as<uint8_t>(), nflags,
                       W.w_tile_cnt.as<uint32_t>());
    MH_HIP(hipGetLastError());
    MH_TRY(scan_counts_u64(c, W.w_tile_cnt.as<uint32_t>(), W.w_tile_off.as<unsigned long long>(), ntiles + 1));
    unsigned long long tot = 0;
    MH_TRY(read_back(c, &tot, W.w_tile_off.as<unsigned long long>() + ntiles, 8));
    W.within_total = tot;
    W.have_within = true;
    if (out_count) *out_count = tot;
    return MOLAR_HIP_OK;
}

// The first set of consecutive `within` requests stays the same while a selection expression is evaluated against one frame
// (`within 0.3 of resid 1`, `within 0.8 of resid 1`, ...: within_size_bench.rs:13-47 asks 1600 times): with the hold on, a
// request that names the same first set (same pointers and sizes, same box and periodicity) and comes to the same grid
// reuses the staged coordinates and the grid of the one before.  The CALLER promises that the first set's coordinates do not
// change while the hold is on (in Rust: for as long as it holds the `&State`); any other search on the context ends the reuse.
int molar_hip_within_hold(molar_hip_ctx *c, int on) {
    if (!c) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "null context");
    c->within_hold = on != 0;
    if (!on) c->held.valid = false;
    return MOLAR_HIP_OK;
}

int molar_hip_within_fill(molar_hip_ctx *c, uint64_t *ids) {
    if (!c || !c->within || !c->within->have_within) return fail(MOLAR_HIP_ERR_NO_SEARCH, "no cached within set: call molar_hip_within_count first");
    molar_hip_within_state &W = *c->within;
    if (W.within_total == 0) return MOLAR_HIP_OK;
    if (!ids) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "within_fill: null output");
    MH_HIP(hipSetDevice(c->device));
    const bool dev = is_device_ptr(ids);
    // (the list of a small second set with a LARGE cutoff is long - 1.9e4 ids for `within 2.5 of 210 atoms` in a 100k-atom box: sorting it
    // on the host took 0.25 ms of a 0.68 ms call; from 4096 ids on, the flags are compacted on the device like the large path's)
    if (W.w_small && !dev && W.within_total <= 4096) {           // the list IS the set: bring it over, sort it (SortedSet::from_unsorted, selection_expr.rs:112), widen it
        std::vector<uint32_t> l((size_t)W.within_total);
        MH_TRY(read_back(c, l.data(), W.w_list.as<uint32_t>() + 1, l.size() * 4));
        std::sort(l.begin(), l.end());
        for (size_t k = 0; k < l.size(); ++k) ids[k] = l[k];
        return MOLAR_HIP_OK;
    }
    if (W.w_small) {                   // device output: compact the flags (they hold the same set)
        const uint64_t ntiles = (W.within_nflags + 2047) / 2048;
        MH_HIP(hipMemsetAsync(W.w_tile_cnt.p, 0, (ntiles + 1) * 4, c->stream));
        hipLaunchKernelGGL(flag_tile_count_kernel, dim3((unsigned)ntiles), dim3(256), 0, c->stream, W.w_flags.as<uint8_t>(), W.within_nflags,
                           W.w_tile_cnt.as<uint32_t>());
        MH_TRY(scan_counts_u64(c, W.w_tile_cnt.as<uint32_t>(), W.w_tile_off.as<unsigned long long>(), ntiles + 1));
    }
    return flags_to_ids(c, W.w_flags.as<uint8_t>(), W.within_nflags, W.w_tile_off.as<unsigned long long>(), W.within_total, c->wide_i, ids, dev);
}

}  // extern "C"
