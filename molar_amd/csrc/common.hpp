// common.hpp — context, device buffers and error plumbing of libmolar_hip.so.
// gfx950 only; host side is plain C++17 over the HIP runtime (no torch, no third-party libs).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../include/molar_hip.h"

namespace mh {

// ---------------------------------------------------------------- errors (tpr_last_error idiom, wrapper.cpp:32,156)

inline std::string &last_error() {
    static thread_local std::string e;
    return e;
}

inline int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    last_error() = buf;
    return code;
}

#define MH_HIP(expr)                                                                                   \
    do {                                                                                               \
        hipError_t _e = (expr);                                                                        \
        if (_e != hipSuccess)                                                                          \
            return ::mh::fail(MOLAR_HIP_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), \
                              __FILE__, __LINE__);                                                     \
    } while (0)

#define MH_TRY(expr)          \
    do {                      \
        int _rc = (expr);     \
        if (_rc) return _rc;  \
    } while (0)

// first statement of an entry that takes a context
#define MH_CTX(c)                                                                    \
    do {                                                                             \
        if (!(c)) return ::mh::fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "null context"); \
        MH_HIP(hipSetDevice((c)->device));                                           \
    } while (0)

// ---------------------------------------------------------------- grow-only device buffer
// Owns its memory: whatever holds a DevBuf frees it by going away, so nothing keeps a list of buffers to release.  Move-only.
// None lives at namespace scope or as a static: a destructor must not run after the HIP runtime has shut down.

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
    DevBuf &operator=(DevBuf &&o) noexcept {
        if (this != &o) {
            release();
            p = std::exchange(o.p, nullptr);
            cap = std::exchange(o.cap, 0);
        }
        return *this;
    }
    ~DevBuf() { release(); }
    int reserve(size_t bytes) {
        if (bytes <= cap) return 0;
        if (p) {
            MH_HIP(hipFree(p));
            p = nullptr;
            cap = 0;
        }
        size_t want = bytes + bytes / 8 + 256;   // headroom: frames of one trajectory vary a little
        MH_HIP(hipMalloc(&p, want));
        cap = want;
        return 0;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    template <class T>
    T *as() const { return reinterpret_cast<T *>(p); }
};

// true if `p` is device-accessible HIP memory (device or managed); false for ordinary host memory
inline bool is_device_ptr(const void *p) {
    if (!p) return false;
    hipPointerAttribute_t a;
    hipError_t e = hipPointerGetAttributes(&a, p);
    if (e != hipSuccess) {
        (void)hipGetLastError();   // unregistered host memory reports an error on some ROCm versions
        return false;
    }
    return a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged || a.type == hipMemoryTypeArray;
}

// ---------------------------------------------------------------- per-set grid state of the cached search

struct GridSet {
    uint32_t n = 0;            // selected atoms handed in
    DevBuf xyz_stage;          // host xyz staged here
    DevBuf idx_stage;          // host idx staged here (uint64)
    DevBuf vdw_stage;
    const float *d_xyz = nullptr;
    const uint64_t *d_idx = nullptr;
    const float *d_vdw = nullptr;
    DevBuf key;                // u32 per atom: cell<<1 | wrapped, 0xFFFFFFFF = dropped
    DevBuf cell_count;         // u32 [ncells+1] -> scanned in place into cell_start
    DevBuf cnt_pad;            // cell counters at one per 128-byte line while binning (crowded grids)
    DevBuf cursor;             // u32 per atom: arrival order inside its cell
    DevBuf tmp_key;            // u32 per kept atom (unsorted inside the cell)
    DevBuf sort_buf;           // grids of large cells: keys and atom numbers, unsorted and sorted (4 x u32 per atom; devsort.hip)
    DevBuf sorted;             // float4 {x,y,z,id-bits} in reference cell order
    DevBuf sorted_vdw;         // float per sorted atom (vdw searches)
    DevBuf aabb;               // float4 lo/hi per cell
    DevBuf perm;               // float4 per sorted atom: the cell in Morton order, {x,y,z,position} (count pass of the fast path)
    DevBuf chunk_aabb;         // float4 lo/hi per 64-atom Morton chunk, slot (cell_start >> 6) + cell + k
    DevBuf h16;                // 8 x f16 per sorted atom (the reference's cell order, like `sorted`): hi/lo split of the position relative to the
                               // cell's origin and of its squared norm - the B operand of the matrix-core count pass
    DevBuf cell_org;           // float4 per cell: origin (centre of the bounding box), .w = bound on |position - origin|
    DevBuf live;               // first set of a search with live-row slots (search_shape.hpp, live_row_slots): per plan entry LIVE_ROW_GROUPS
                               // 64-bit masks of the first cell's rows that can have a hit in the second cell, then a u32 live count per
                               // entry (live_rows_kernel, behind the grid build: the masks are of the generation like the grid itself)
};

// ---------------------------------------------------------------- the shape of one search
// What the host helpers of search.hip need to know about the search in hand; what follows from it alone (grid dimensions,
// kernel family, slot bound, the policy for wrapped pairs) is in search_shape.hpp.  The context keeps one, the cached search;
// a caller that describes frames which are not the cached search (hist_frames_group) builds its own and hands them down.
struct SearchShape {
    int kind = 0;
    bool use_box = false;
    uint8_t pbc = 0;
    float cutoff = 0.f;
    molar_hip_box box{};
    float lower[3]{}, upper[3]{};
    uint32_t dims[3]{1, 1, 1};
    uint64_t ntasks = 0;
    uint64_t nslots_bound = 0;   // host-side upper bound of the slot count (sizes the launches)
    GridSet *set = nullptr;      // set[0], set[1]: the grids of the first / second set
    uint32_t occ_use[2] = {0, 0};   // occupied cells of the two grids, latched per search from the context's hint
                                    // (0: not known for this search, the grid's cell count stands in)
};

// ---------------------------------------------------------------- the held grid of `within` requests
// molar_hip_within_hold: the first set of a `within` request as it was staged and binned, for later requests against the SAME
// first set to reuse.  What decides the reuse is in search_shape.hpp (held_names_request, held_same_cells, held_remember); a
// search that stages or bins the first set of that grid generation again ends it (valid = false).
struct HeldGrid {
    bool valid = false;
    const GridSet *set = nullptr;      // the grid generation the held grid lives in
    uint64_t fp = 0;                   // fingerprint of a host-memory first set as it was staged (0: device memory, read in place)
    const float *xyz = nullptr;        // the request's first set as the caller named it ...
    const uint64_t *idx = nullptr;
    size_t natoms = 0, n = 0;
    int ids_local = 0;
    bool use_box = false;              // ... and the frame it was binned in
    uint8_t pbc = 0;
    molar_hip_box box{};
    uint32_t dims[3]{0, 0, 0};
    float lower[3]{}, upper[3]{};      // (the caller's bounds: they decide the grid of a request without a box)
};

// ---------------------------------------------------------------- the sizes of one search
struct SearchSizes {            // written by the plan and offsets kernels into pinned host memory, read by the host after the stream
    unsigned long long total;       // results of the search                   (slot_offsets_kernel / scan_slot_counts)
    unsigned long long mask_units;  // hit-history units, 0 for kinds without  (slotmap_kernel / plan_slots_kernel)
    unsigned long long slots;       // slots the plan came to                  (the same two)
    unsigned long long occupied;    // occupied cells, set 1 << 32 | set 0; 0 = not reported
};
// the kernels' stores and the copy fallback of resident_enqueue (search.hip) address the fields at these offsets
static_assert(sizeof(SearchSizes) == 32 && offsetof(SearchSizes, total) == 0 && offsetof(SearchSizes, mask_units) == 8 &&
                  offsetof(SearchSizes, slots) == 16 && offsetof(SearchSizes, occupied) == 24,
              "SearchSizes: total, mask_units, slots, occupied, 64 bits each, in this order");

}  // namespace mh

struct molar_hip_search64_state;        // the cached f64 search (search_f64.hip)
struct molar_hip_sasa_state;            // point tables, grid and scratch of the surface-area calls (sasa.hip)
struct molar_hip_rmsd_matrix_state;     // packed operands, partial covariances and staging of the all-pairs RMSD (rmsd_matrix.hip)
struct molar_hip_fluct_state;           // fits, packed deviations, partial covariances and staging of the fluctuations (fluct.hip)
struct molar_hip_msd_state;             // boxes, unwrapped particle trajectories, partial lag sums and staging of the displacements (msd.hip)
struct molar_hip_density_state;         // boxes, centres, the frames' integer bins and the running sums of the density calls (density.hip)
struct molar_hip_intcoord_state;        // staged inputs, the boxes, staged results and the chunk partials of the internal-coordinate calls (intcoord.hip)
struct molar_hip_tcf_state;             // staged inputs, the f64 vector trajectories, chunk partials and staged results of the time correlation calls (tcf.hip)
struct molar_hip_sfactor_state;         // staged inputs, the partition by label, the blocks of the gram kernel, rho of a block of frames and the running sums of the structure factor calls (sfactor.hip)
struct molar_hip_mindist_state;         // staged inputs, the boxes, the partition by label, both sets of a block of frames in f64, row partials, the block's group matrix and the running reductions of the minimum-distance calls (mindist.hip)
struct molar_hip_vanhove_state;         // staged inputs, the partition by label, the particle-major f64 trajectories and staged counts of the van Hove calls (vanhove.hip)
struct molar_hip_hbonds_state;          // keys, the cached bonds of a frame or a block and the block's table (hbonds.hip)
struct molar_hip_lifetimes_state;       // the bit matrix, histograms and staging of the lifetime correlations (lifetimes.hip)
struct molar_hip_within_state;          // flags, lists and the cached `within` set (within.hip)
struct molar_hip_connectivity_state;    // the cached SearchConnectivity CSR of either precision (connectivity.hip)
struct molar_hip_contacts_state;        // the second context, labels, accumulators and forest of the contacts / clusters calls (contacts.hip)

// frames per launch of molar_hip_search_histogram_frames (search.hip, hist_frames_group)
#ifndef MH_HIST_BATCH
#define MH_HIST_BATCH 16
#endif

struct molar_hip_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    int num_cus = 256;

    // Pinned bounce buffer: read-backs (read_back below), staging of small tables, results a kernel or a bulk copy leaves for the
    // host to read after the stream.  Its contents mean nothing across any call that may use it, ensure_pinned may move it, nothing
    // may hold its address across a call - and no kernel of the search stores here: its sizes have their own home (h_sizes).
    void *h_pinned = nullptr;
    size_t h_pinned_cap = 0;
    molar_hip_search64_state *s64 = nullptr;      // created by the first molar_hip_search_count_f64
    molar_hip_sasa_state *sasa = nullptr;         // created by the first molar_hip_sasa*
    molar_hip_rmsd_matrix_state *rmsdm = nullptr; // created by the first molar_hip_rmsd_matrix*
    molar_hip_fluct_state *fluct = nullptr;       // created by the first molar_hip_fluct*
    molar_hip_msd_state *msd = nullptr;           // created by the first molar_hip_msd*
    molar_hip_density_state *density = nullptr;   // created by the first molar_hip_density*
    molar_hip_intcoord_state *intcoord = nullptr;   // created by the first molar_hip_intcoord*
    molar_hip_tcf_state *tcf = nullptr;           // created by the first molar_hip_tcf*
    molar_hip_sfactor_state *sfactor = nullptr;   // created by the first molar_hip_sfactor*
    molar_hip_mindist_state *mindist = nullptr;   // created by the first molar_hip_mindist*
    molar_hip_vanhove_state *vanhove = nullptr;   // created by the first molar_hip_vanhove*
    molar_hip_hbonds_state *hbonds = nullptr;     // created by the first molar_hip_hbonds*
    molar_hip_lifetimes_state *lifetimes = nullptr;   // created by the first molar_hip_lifetimes*
    molar_hip_within_state *within = nullptr;         // created by the first molar_hip_within_count
    molar_hip_connectivity_state *conn = nullptr;     // created by the first molar_hip_search_connectivity / _f64
    molar_hip_contacts_state *contacts = nullptr;     // created by the first molar_hip_search_contacts* / _clusters*
    // ring of pinned chunks for large results that go to pageable host memory (hoststream.hpp), allocated on first use
    void *ring[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    hipEvent_t ring_ev[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};

    // ---- cached search (count -> fill)
    // Four things describe a search, and only the first two are kept here:
    //  * its SHAPE - kind, box, cutoff, grid dimensions, plan and slot bounds, the grid generation it refers to - is `cur`, one
    //    value; the helpers of search.hip are functions of a shape, so frames that are not the cached search are described by
    //    shapes of the caller's own and leave `cur` alone;
    //  * what OUTLASTS a request: have_search / total / mask_units, the buffers, the hints (occ_key, occ_cells, occ_valid), the
    //    tickets, the record of a held `within` grid (`held`);
    //  * what ONE request asks of the shared helpers (plan or not, side stream, output capacity ...) travels down the call
    //    chain as a SearchCall argument (search_core.hpp);
    //  * WHERE a grid is built - the stream, that stream's scan and sort scratch, the launch shape that goes with it - is a
    //    GridLane argument (search.hip: main_lane, side_lane).  `stream` is assigned when the context is created or handed a
    //    stream and never swapped for the length of a call: whatever reads it gets the main stream.
    // What a CONSUMER of the search keeps across its own calls - the `within` set, the connectivity CSR, the contacts and
    // clusters calls' second context and work areas - is not here: each has a state of its own behind one pointer above
    // (within.hip, connectivity.hip, contacts.hip; they reach the search through search_core.hpp).
    // have_search says that a count has finished and the fill calls may run - nothing else: a request that came to nothing
    // (empty vdW input) is reported by prepare_search through its `degenerate` argument.
    bool have_search = false;
    mh::SearchShape cur;                 // the cached search; cur.set = the grid generation it refers to
    uint64_t total = 0;
    // Two generations of the grids: the pipelined resident search (molar_hip_search_resident_begin) builds the grid of
    // the next frame on `side_stream` while the pair kernels of the frame before it still read theirs.
    mh::GridSet set_store[2][2];
    molar_hip_ctx() { cur.set = set_store[0]; }
    hipStream_t side_stream = nullptr;   // grid build of a pipelined search (created on first use, highest priority)
    hipEvent_t grid_done = nullptr;
    bool env_no_side = false;            // MOLAR_HIP_NO_SIDE_STREAM, read once in molar_hip_create
    bool env_no_mfma = false;            // MOLAR_HIP_NO_MFMA_COUNT: count pass of plain entries on the vector ALUs (A/B runs)
    bool env_no_mfma_wrapped = false;    // MOLAR_HIP_NO_MFMA_WRAPPED: count pass of wrapped entries on the vector ALUs (A/B runs)
    bool env_host_grid_wait = false;     // MOLAR_HIP_HOST_GRID_WAIT: the host, not the main stream, waits for the side stream's grid
    bool env_no_tile_sum = false;        // MOLAR_HIP_NO_TILE_SUM: slot offsets by the general three-kernel scan (A/B runs)
    uint32_t env_debug_skip = 0;         // MOLAR_HIP_DEBUG_SKIP (builds with -DMOLAR_HIP_DEBUG_KNOBS only), read once
    uint32_t env_debug_launch = 0, dbg_launches = 0;   // MOLAR_HIP_DEBUG_LAUNCH (same builds): which histogram launch records its wave times
    hipEvent_t gen_free[2] = {nullptr, nullptr};   // recorded on the main stream behind the last asynchronous reader of
                                                   // a grid generation (histogram calls that do not wait): what the side
                                                   // stream waits for before it rebuilds the generation
    bool env_no_bin_tile = false;        // MOLAR_HIP_NO_BIN_TILE: the grid's binning with one global atomic per atom (A/B runs)
    int hist_gen = 0;                    // generation of the last asynchronous histogram call
    mh::DevBuf scan_tmp_side;            // block sums of the scans on the side stream (the two streams may scan at the same time)
    mh::DevBuf params;         // SearchParams block read by the pair kernels
    mh::DevBuf task_desc;      // TaskDesc per task (plan entry)
    mh::DevBuf task_nb;        // u32 per task (+1): 64-row blocks of the task, scanned in place -> first slot
    mh::DevBuf slot_desc;      // SlotDesc per slot (+1): what a wave of the pair kernels needs to start
    mh::DevBuf slot_cnt;       // u32 per slot (+1): results of the slot
    mh::DevBuf slot_base;      // u64 per slot (+1): output offset (last = grand total)
    mh::DevBuf tile_sum;       // u64 per tile of 256 slots: results of the tile (tile_sums_kernel -> slot_offsets_kernel)
    bool params_fresh = false;                 // the plan kernel of this search left a parameter block the count pass can use as it is
    unsigned long long params_fresh_cap = 0;   // ... written with this output capacity
    mh::DevBuf scan_tmp;       // block sums for the scans
    mh::DevBuf sort_tmp, sort_tmp_side;   // scratch of the device sort (devsort.hip), per stream
    mh::DevBuf scan_state;     // ticket + tile descriptors of the single-pass scans (zeroed by the plan kernel)
    mh::DevBuf fplan_tiles;    // plan_tiles_kernel -> plan_slots_kernel: slot / hit-history totals per tile of 256 plan entries
    mh::DevBuf slot_stat;      // u64[2] left by plan_slots_kernel: slots of the last plan, slots consecutive rows would have given
    bool slot_stat_valid = false;          // ... the last search was planned that way (molar_hip_search_slot_counts)
    bool plan_live = false;                // the slot records of the cached search are cut from live rows: launch_pairs takes the
                                           // pair_kernel<.., LIVE = true> instances
    mh::DevBuf out_pairs_set[2];   // ctx-owned result buffers (device-resident results / host staging); the second
    mh::DevBuf out_dist_set[2];    // set exists for the pipelined begin/end searches only
    mh::DevBuf &out_pairs = out_pairs_set[0];
    mh::DevBuf &out_dist = out_dist_set[0];
    // pipelined resident searches (molar_hip_search_resident_begin/_end): two result sets, two tickets
    struct Ticket {
        bool pending = false, degenerate = false;
        unsigned long long cap0 = 0, maskcap0 = 0, serial = 0, launched = 0, ntasks = 0;
        int kind = -1;
        unsigned long long occ_key = 0;
        hipEvent_t done = nullptr;
        molar_hip_search_desc desc{};
    } tickets[2];
    int next_ticket = 0;
    bool resident_no_dist = false;          // molar_hip_search_resident_planes: the resident calls of the C ABI fill the (i, j) plane only
                                            // (a setting of the caller's: internal users that want the plane alone say so by argument)
    unsigned long long search_serial = 0;   // counts resident searches enqueued on this context
    // Resident searches launch their count and fill passes over the slots the plan of the SEARCH BEFORE came to (+ 3 % + 512)
    // instead of the host's bound (14 N / 64 + entries: 13 % above the real count on the headline frame - 3.7e4 workgroups per
    // pass that only find out they have nothing to do); the plan writes its real slot count beside the other sizes, and a
    // search that needed more slots than were launched is repeated with the bound where its sizes are read.
    unsigned long long trim_real = 0, trim_ntasks = 0;   // slots of the last resident search whose sizes were read, and its plan
    int trim_kind = -1;
    // The one home of the searches' SearchSizes records: a pinned array allocated with the context, one entry per ticket and one
    // for the calls that wait for their search themselves.  d_sizes is the array's device-side address, resolved once (null: the
    // device cannot store there and the sizes are copied behind the passes, resident_enqueue).
    static constexpr int SIZES_SYNC = 2, SIZES_ENTRIES = 3;
    mh::SearchSizes *h_sizes = nullptr, *d_sizes = nullptr;
    // Occupied cells of the two sets' grids as the last finished search of this shape found them (the grid build counts them, the
    // offsets kernel hands them to the host with the sizes): small_cell_lanes() judges a frame by its atoms per OCCUPIED cell when it
    // knows - a slab or a solute in a mostly empty periodic box has a small mean and crowded cells.  Latched per search into cur.occ_use.
    unsigned long long occ_key = 0;
    uint32_t occ_cells[2] = {0, 0};
    bool occ_valid = false;
    mh::DevBuf out_ids;
    mh::DevBuf wide_i, wide_j; // usize widening
    mh::DevBuf hist;           // u64 bins
    mh::DevBuf dbg;            // builds with -DMOLAR_HIP_DEBUG_KNOBS: per-wave time accounting of hist_kernel
    mh::DevBuf hist_queue;     // slot queues and list counters of the fused histogram (hist_kernels.hpp)
    mh::DevBuf slot_desc_rest; // fused histogram: records of the slots the generic kernel takes (hist_plan_kernel)
    unsigned long long hist_frames = 0;   // fused-histogram launches of this context (mod 4: which pair of list counters a launch uses)
    // molar_hip_search_histogram_frames: groups of frames through one set of launches (search.hip, hist_frames_group)
    mh::GridSet hb_sets[2][MH_HIST_BATCH][2];           // grids of a group's frames (first / second set), two generations
    bool hb_zeroed[2][MH_HIST_BATCH][2] = {};           // a set's padded cell counters are zero (the frames' unpad kernel leaves them so)
    uint32_t hb_zeroed_cells[2][MH_HIST_BATCH][2] = {}; // ... for a grid of this many cells
    mh::DevBuf hb_lean[2], hb_rest[2];    // the group's two slot lists
    mh::DevBuf hb_blocks[2];              // [parameter blocks | grid records] of the group
    void *hb_pin = nullptr;               // pinned staging of those records: four slots
    hipEvent_t hb_pin_ev[4] = {nullptr, nullptr, nullptr, nullptr};
    bool hb_pin_used[4] = {false, false, false, false};
    unsigned hb_pin_next = 0;
    mh::DevBuf hist_edges;     // f32[nbins + 1]: smallest d2 that reaches each bin (hist_kernel), for the cached (min, max, nbins)
    float edges_min = 0.f, edges_max = 0.f;
    size_t edges_nbins = 0;    // 0: no table cached
    // molar_hip_within_hold: reuse of the first set's staged coordinates and grid across `within` requests (prepare_search reads
    // and ends it: it belongs to the search, not to within.hip's state)
    bool within_hold = false;          // the caller's switch
    mh::HeldGrid held;
    mh::DevBuf task_mu;        // u32 per task (+1): 64-word hit-history units of the task's slots
    mh::DevBuf task_moff;      // u64 per task (+1): exclusive scan of task_mu
    mh::DevBuf maskbuf;        // hit bits recorded by the count pass, replayed by the fill pass
    uint64_t mask_units = 0;

    // molar_hip_xtc_histogram: a second context for the decoder thread (its own stream and pinned staging), two windows of frames, bins + index
    molar_hip_ctx *aux = nullptr;
    mh::DevBuf xh_win[2], xh_bins;

    // ---- profiling (HIP events on `stream`)
    bool profiling = false;
    bool profile_frames = false;   // molar_hip_profile_enable(ctx, 2): ONE span (class 5) around count + offsets + fill of a resident search, none inside
    struct Span { int cls; hipEvent_t a, b; };
    std::vector<Span> spans;
    std::vector<hipEvent_t> event_pool;

    mh::DevBuf fit_redo;       // membrane fit: lipids k_membrane_fit_lanes hands to the one-lane kernel
    // ---- measure scratch
    mh::DevBuf m_xyz1, m_xyz2, m_idx1, m_idx2, m_mass1, m_mass2, m_partials, m_results, m_out;
};

namespace mh {

// the units that own a state of the context free it (molar_hip_destroy, api.hip)
void search64_release(molar_hip_ctx *c);
void sasa_release(molar_hip_ctx *c);
void rmsd_matrix_release(molar_hip_ctx *c);
void fluct_release(molar_hip_ctx *c);
void msd_release(molar_hip_ctx *c);
void density_release(molar_hip_ctx *c);
void intcoord_release(molar_hip_ctx *c);
void tcf_release(molar_hip_ctx *c);
void sfactor_release(molar_hip_ctx *c);
void mindist_release(molar_hip_ctx *c);
void vanhove_release(molar_hip_ctx *c);
void hbonds_release(molar_hip_ctx *c);
void lifetimes_release(molar_hip_ctx *c);
void within_release(molar_hip_ctx *c);
void connectivity_release(molar_hip_ctx *c);
void contacts_release(molar_hip_ctx *c);

// ---------------------------------------------------------------- the per-context state of a unit

// created by the first call that gets this far
template <class State>
State &state_of(State *&slot) {
    if (!slot) slot = new State;
    return *slot;
}

// the end of a *_release: the state (its DevBuf members free themselves) and the context's pointer
template <class State>
void release_state(State *&slot) {
    delete slot;
    slot = nullptr;
}

// The block result the context keeps after molar_hip_hbonds_frames, for the units that consume it in place (lifetimes.hip):
// the frames' offsets (HOST memory, nframes + 1), the table row of every entry (DEVICE memory), the rows of the table.
struct HbondsBlockView {
    const uint64_t *frame_offsets;
    size_t nframes;
    const uint32_t *bond_of_entry;
    size_t rows, entries;
    uint64_t serial;              // counts the blocks of this context: a caller's record of a block is stale when it differs
};
// false: the context holds no block result
bool hbonds_block_view(const molar_hip_ctx *c, HbondsBlockView *out);

// RAII span: records an event pair around a group of launches when profiling is on
struct Prof {
    molar_hip_ctx *c;
    int cls;
    hipStream_t stream;
    hipEvent_t a = nullptr, b = nullptr;
    static hipEvent_t get(molar_hip_ctx *c) {
        if (!c->event_pool.empty()) {
            hipEvent_t e = c->event_pool.back();
            c->event_pool.pop_back();
            return e;
        }
        hipEvent_t e = nullptr;
        (void)hipEventCreate(&e);
        return e;
    }
    // (on the context's stream unless the launches of the span go to another one: a grid build on the side stream)
    Prof(molar_hip_ctx *ctx, int k) : Prof(ctx, k, ctx->stream) {}
    Prof(molar_hip_ctx *ctx, int k, hipStream_t on) : c(ctx), cls(k), stream(on) {
        if (!c->profiling) return;
        if (c->profile_frames ? (k >= 1 && k <= 3) : k == 5) return;      // frame mode: the three passes share the frame's span
        a = get(c);
        b = get(c);
        (void)hipEventRecord(a, stream);
    }
    ~Prof() {
        if (!c->profiling || !a) return;
        (void)hipEventRecord(b, stream);
        c->spans.push_back({cls, a, b});
    }
};

inline int ensure_pinned(molar_hip_ctx *c, size_t bytes) {
    if (bytes <= c->h_pinned_cap) return 0;
    if (c->h_pinned) (void)hipHostFree(c->h_pinned);
    c->h_pinned = nullptr;
    c->h_pinned_cap = 0;
    MH_HIP(hipHostMalloc(&c->h_pinned, bytes + 4096, hipHostMallocDefault));
    c->h_pinned_cap = bytes + 4096;
    return 0;
}

// The one read-back: `bytes` of device memory into `dst_host` through the bounce buffer, complete when the call returns.
inline int read_back(molar_hip_ctx *c, void *dst_host, const void *src_dev, size_t bytes) {
    MH_TRY(ensure_pinned(c, bytes));
    MH_HIP(hipMemcpyAsync(c->h_pinned, src_dev, bytes, hipMemcpyDeviceToHost, c->stream));
    MH_HIP(hipStreamSynchronize(c->stream));
    std::memcpy(dst_host, c->h_pinned, bytes);
    return 0;
}

// device-side address of a pinned SearchSizes record or array (null: the device cannot store there)
inline SearchSizes *sizes_device_address(SearchSizes *pinned) {
    void *d = nullptr;
    if (hipHostGetDevicePointer(&d, pinned, 0) == hipSuccess) return static_cast<SearchSizes *>(d);
    (void)hipGetLastError();
    return nullptr;
}

// the context's SearchSizes array (molar_hip_ctx::h_sizes), once per context
inline int alloc_search_sizes(molar_hip_ctx *c) {
    MH_HIP(hipHostMalloc(reinterpret_cast<void **>(&c->h_sizes), molar_hip_ctx::SIZES_ENTRIES * sizeof(SearchSizes), hipHostMallocDefault));
    for (int i = 0; i < molar_hip_ctx::SIZES_ENTRIES; ++i) c->h_sizes[i] = SearchSizes{};
    c->d_sizes = sizes_device_address(c->h_sizes);
    return 0;
}

// Make `src` (host or device, `bytes` long) readable by kernels: device pointers are used in
// place, host buffers are copied into `stage` on the context's stream.
template <class T>
inline int to_device(molar_hip_ctx *c, const T *src, size_t count, DevBuf &stage, const T **out) {
    if (!src || count == 0) {
        *out = nullptr;
        return 0;
    }
    if (is_device_ptr(src)) {
        *out = src;
        return 0;
    }
    MH_TRY(stage.reserve(count * sizeof(T)));
    MH_HIP(hipMemcpyAsync(stage.p, src, count * sizeof(T), hipMemcpyHostToDevice, c->stream));
    *out = stage.as<T>();
    return 0;
}

// CSR selections: offsets[nsel] = number of index entries; offsets may live on either side
inline int csr_total(const uint64_t *offsets, size_t nsel, uint64_t *last) {
    if (is_device_ptr(offsets)) MH_HIP(hipMemcpy(last, offsets + nsel, 8, hipMemcpyDeviceToHost));
    else *last = offsets[nsel];
    return 0;
}

}  // namespace mh
