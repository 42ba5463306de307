// search_core.hpp - what a CONSUMER of the f32 search calls: a unit that is itself a search request and then does something of
// its own with the grid, the plan or the pair list (within.hip, connectivity.hip, contacts.hip).  Declarations only; the
// functions are search.hip's.  (stages.hpp is the other door: the resident search without its wait, for units that chain device
// work behind it.)  The parameter block's layout, the plan, GridLane and launch_pairs stay inside search.hip.
#pragma once

#include "common.hpp"

namespace mh {

// What ONE request asks of the helpers below (prepare_search, build_grid, the plan, launch_pairs), beyond its descriptor.  It
// lives on the caller's stack and goes down the call chain by reference; the context holds only what outlasts a request.
// `side` is a wish: prepare_search decides (takes_side_lane) and hands the grid build the lane it chose (GridLane, search.hip) - the
// stream is an argument of the helpers that launch a grid, not a field they find swapped.
struct SearchCall {
    bool plan = true;              // prepare_search enqueues the plan (false: the caller walks cells, or plans inside launch_pairs)
    bool within_set = false;       // the request is molar_hip_within_count's: its first set's grid may be held (molar_hip_within_hold)
    bool hist_plan = false;        // fused histogram of the fixed-cutoff kinds: grid and slot bound for hist_plan_kernel
    bool size_masks = true;        // count -> fill pair: read the plan's sizes back and size the hit-history buffer exactly
    bool side = false;             // the grid may be built on the side stream (pipelined searches, asynchronous histograms) ...
    hipEvent_t side_wait = nullptr;            // ... which first waits for this (the last reader of the grid generation)
    unsigned long long out_cap = ~0ull;        // resident searches: the output capacity in the parameter block (plan kernel, pair passes)
    SearchSizes *sizes_dev = nullptr;          // resident searches: device-side address of the pinned record the kernels write
    bool drop_nonfinite = false;   // the grid leaves atoms with a non-finite coordinate out (stages.hpp, search_resident_enqueue)
    uint32_t slot_launch = 0;      // resident searches: slots the count and fill passes launch (0: the bound; common.hpp, trim_real)
    bool live_rows = true;         // the slots go to the count / fill passes, which walk live-ranked slots where live_row_slots() says so
                                   // (false: another kernel reads the records - the contact kernels - and wants consecutive rows)
};

// Everything of a search up to its pair passes: the request described in c->cur, the grids built, the plan enqueued.
// *degenerate: the request came to nothing (empty vdW input) - nothing was enqueued, c->cur says one cell and no plan entries,
// c->total is 0; what that means for the context's cached search is the caller's to say.
int prepare_search(molar_hip_ctx *c, const molar_hip_search_desc *q, const SearchCall &call, bool *degenerate);

// the SearchParams block of `shape` into c->params, on the main stream (a request prepared without a plan has none yet)
int upload_search_params(molar_hip_ctx *c, const SearchShape &shape);

// exclusive scan of n u32 counts into u64 offsets on the main stream, with the main lane's scratch
int scan_counts_u64(molar_hip_ctx *c, const uint32_t *counts, unsigned long long *offsets, uint64_t n);

// One whole resident search into the context's result buffers, the (i, j) plane only, complete when the call returns:
// c->total pairs in c->out_pairs.
int resident_pairs(molar_hip_ctx *c, const molar_hip_search_desc *q);

// connectivity.hip: the CSR of SearchConnectivity from 2 * npairs (row, neighbour) entries, for both precisions.  _begin ends
// the cached CSR, reserves and hands out the two entry arrays (2 * npairs u32 each) for the caller's kernel to fill on the main
// stream; _finish sorts them by row (stable), widens the neighbours, bisects the offsets and caches the result for
// molar_hip_search_connectivity_fill.  _forget only ends the cached CSR: the f64 entry says so before its count, which may fail
// before the number of pairs is known.
void connectivity_forget(molar_hip_ctx *c);
int connectivity_begin(molar_hip_ctx *c, uint64_t nrows, uint64_t npairs, uint32_t **row_in, uint32_t **nb_in);
int connectivity_finish(molar_hip_ctx *c);

}  // namespace mh
