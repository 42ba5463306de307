/*
 * molar_hip.h — C ABI of libmolar_hip.so, the MI355X (gfx950) engine for MolAR's per-frame
 * hot path: distance_search, PeriodicBox, Measure (COM/COG/gyration/inertia/rmsd/fit) and
 * Modify (apply_transform/unwrap_simple).
 *
 * This is the drop-in boundary.  It follows the reference's own runtime-plugin
 * convention (molar_gromacs/gromacs/wrapper.hpp:34-81): opaque handle + open/close,
 * thread-local last_error string, caller-owned output buffers filled after a count call,
 * plain C types only.  Each entry point names the reference interface it replaces
 * (paths relative to /root/reference/).
 *
 * Data layout handed over by MolAR (providers.rs:96-136, state.rs:22-28, atom_storage.rs:272):
 *   xyz   : whole frame, AoS float[3*natoms] (Vec<Pos>, Pos = Point3<f32>)
 *   idx   : sorted selection index slice (usize -> uint64_t), NULL = identity 0..natoms
 *   mass  : full-length column float[natoms], gathered through idx
 *   box9  : column-major float[9], COLUMNS are the box vectors a,b,c (periodic_box.rs:7-13)
 *   pbc   : PbcDims bit mask, bit d <=> dimension d (periodic_box.rs:81-114)
 *
 * Every pointer argument may be a HOST pointer or a DEVICE (HIP) pointer; the library detects
 * which (hipPointerGetAttributes) and stages host buffers through its own device buffers.
 * Device-resident inputs/outputs are used in place: no copy, kernels read/write them directly.
 *
 * Threading: a context is owned by one thread at a time (MolAR calls the search from one
 * thread, distance_search.rs:949); use one context per thread / per GPU.
 */
#ifndef MOLAR_HIP_H
#define MOLAR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* status codes: MeasureError (molar/src/measure.rs:732-762), PeriodicBoxError
 * (periodic_box.rs:131-144), LipidOrderError (measure.rs:718-729) */
enum {
    MOLAR_HIP_OK = 0,
    MOLAR_HIP_ERR_SIZES = 1,
    MOLAR_HIP_ERR_ZERO_MASS = 2,
    MOLAR_HIP_ERR_SVD = 3,           /* the rotation is found by Horn's quaternion method, which cannot fail to converge like an
                                      * SVD; this code is returned when the covariance is not finite (NaN / inf coordinates) */
    MOLAR_HIP_ERR_NO_PBC = 4,
    MOLAR_HIP_ERR_ZERO_LENGTH_VECTOR = 5,
    MOLAR_HIP_ERR_INVERSE_FAILED = 6,
    MOLAR_HIP_ERR_LIPID_TAIL_TOO_SHORT = 7,
    MOLAR_HIP_ERR_LIPID_NORMALS_COUNT = 8,
    MOLAR_HIP_ERR_LIPID_BOND_ORDER_COUNT = 9,
    MOLAR_HIP_ERR_ANGLE_TOO_SMALL = 10,
    MOLAR_HIP_ERR_INVALID_ARGUMENT = 50,
    MOLAR_HIP_ERR_TOO_LARGE = 51,
    MOLAR_HIP_ERR_NO_SEARCH = 52,
    MOLAR_HIP_ERR_IO = 53,        /* trajectory file: open/seek failure, truncated or corrupt frame */
    MOLAR_HIP_ERR_HIP = 100       /* HIP runtime failure, text in molar_hip_last_error() */
};

#define MOLAR_HIP_PBC_FULL 7u     /* periodic_box.rs:126 */
#define MOLAR_HIP_PBC_NONE 0u     /* periodic_box.rs:128 */

/* ------------------------------------------------------------------ lifecycle */

typedef struct molar_hip_ctx molar_hip_ctx;   /* opaque, like TprHandle (wrapper.hpp:34-36) */

/* Create an engine bound to HIP device `device`.  NULL on error (no GPU, bad ordinal);
 * message via molar_hip_last_error().  Mirrors tpr_open/tpr_close (wrapper.hpp:42-44). */
molar_hip_ctx *molar_hip_create(int device);
void molar_hip_destroy(molar_hip_ctx *ctx);
/* Thread-local text of the last failure on this thread; mirrors tpr_last_error (wrapper.hpp:46). */
const char *molar_hip_last_error(void);
const char *molar_hip_version(void);
/* Number of visible HIP devices, 0 if none / no driver (never fails). */
int molar_hip_device_count(void);
/* Run this context's kernels on an existing hipStream_t (e.g. torch's current stream). */
int molar_hip_set_stream(molar_hip_ctx *ctx, void *hip_stream);
int molar_hip_synchronize(molar_hip_ctx *ctx);

/* Per-kernel-class timing with HIP events recorded on the context's stream (what bench.py's
 * roofline line is computed from).  Classes: 0 grid build (bin/scan/scatter/place), 1 pair count
 * kernel, 2 offset scan, 3 pair fill kernel, 4 measure/fit kernels.  read() synchronises the
 * stream, returns the accumulated milliseconds and launch counts since the last read, and resets.
 * enable(ctx, 2): the resident searches record ONE span per search instead - class 5: count pass +
 * offset scan + fill pass between a single pair of events (an event record is a barrier packet of
 * 5-10 us on the stream, so the three bracketed passes of mode 1 read longer than they run). */
#define MOLAR_HIP_PROFILE_CLASSES 8
int molar_hip_profile_enable(molar_hip_ctx *ctx, int on);
int molar_hip_profile_read(molar_hip_ctx *ctx, float ms[MOLAR_HIP_PROFILE_CLASSES],
                           uint64_t launches[MOLAR_HIP_PROFILE_CLASSES]);

/* Device-memory ceilings of this GPU, measured in the caller's process (SURVEY.md §8d "measured device-copy ceiling
 * from a trivial float4 copy kernel in the same run").  copy: `bytes` device-to-device `reps` times, best of three
 * float4 kernels (grid-stride; four loads in flight per thread; the same non-temporal), (read + written bytes) / time.
 * write: a write-only float4 stream of `bytes` (the pair list is write traffic), bytes / time.  GB/s.
 * Diagnostics, not part of the reference. */
int molar_hip_copy_bandwidth(molar_hip_ctx *ctx, size_t bytes, int reps, float *gb_per_s);
int molar_hip_write_bandwidth(molar_hip_ctx *ctx, size_t bytes, int reps, float *gb_per_s);

/* ------------------------------------------------------------------ PeriodicBox (periodic_box.rs:15-23) */

typedef struct {
    float m[9];          /* column-major, columns a,b,c */
    float inv[9];        /* nalgebra try_inverse */
    int32_t nshift;      /* tric_corrections.len(), 0 for orthogonal boxes */
    float shifts[26 * 3];
} molar_hip_box;

/* PeriodicBox::from_matrix (periodic_box.rs:156-176): ERR_ZERO_LENGTH_VECTOR / ERR_INVERSE_FAILED. */
int molar_hip_box_from_matrix(const float m9[9], molar_hip_box *out);
/* PeriodicBox::from_vectors_angles (periodic_box.rs:188-235), angles in degrees. */
int molar_hip_box_from_vectors_angles(float a, float b, float c, float alpha, float beta, float gamma,
                                      molar_hip_box *out);
/* shortest_vector_dims (periodic_box.rs:286-318), host arithmetic identical to the device code. */
void molar_hip_box_shortest_vector(const molar_hip_box *box, const float v[3], uint8_t pbc, float out[3]);
/* get_lab_extents (periodic_box.rs:369-375): row sums, what sizes the search grid. */
void molar_hip_box_lab_extents(const molar_hip_box *box, float out[3]);
/* get_box_extents (:364-366): lengths of the box vectors. */
void molar_hip_box_extents(const molar_hip_box *box, float out[3]);
/* to_box_coords (:340-344) = inv*v, to_lab_coords (:356-360) = M*v. */
void molar_hip_box_to_box_coords(const molar_hip_box *box, const float v[3], float out[3]);
void molar_hip_box_to_lab_coords(const molar_hip_box *box, const float v[3], float out[3]);
/* is_inside (:348-352): all fractional coordinates in [0,1). */
int molar_hip_box_is_inside(const molar_hip_box *box, const float p[3]);
/* wrap_point / wrap_vec (:409-434), including the reference's `1.0 - bv` for negative fractions. */
void molar_hip_box_wrap_point(const molar_hip_box *box, const float p[3], float out[3]);

/* ------------------------------------------------------------------ distance search (distance_search.rs) */

enum {
    MOLAR_HIP_SEARCH_SINGLE = 0,      /* distance_search_single(_pbc)      :892-954 */
    MOLAR_HIP_SEARCH_DOUBLE = 1,      /* distance_search_double(_pbc)      :659-754 */
    MOLAR_HIP_SEARCH_WITHIN = 2,      /* distance_search_within(_pbc)      :519-598 */
    MOLAR_HIP_SEARCH_DOUBLE_VDW = 3   /* distance_search_double_vdw(_pbc)  :767-879 */
};

/* One search request.  Set 1 = (xyz1, natoms1, idx1, n1); set 2 likewise (unused for SINGLE).
 * The reference takes iterators of &Pos and of ids; here positions are gathered through idx
 * and the emitted ids are idx values (ids_local=0: iter_index(), molar_python/src/lib.rs:296-302)
 * or 0..n-1 (ids_local=1: modify.rs:78, all vdw drivers :791-792).
 * box9 == NULL selects the non-periodic driver, otherwise the *_pbc driver with `pbc`.
 * WITHIN without a box needs lower/upper (selection/ast.rs:597-612 computes them from min_max). */
typedef struct {
    int32_t kind;
    float cutoff;              /* ignored for DOUBLE_VDW (derived from the radii, :781-783) */
    const float *xyz1;
    size_t natoms1;
    const uint64_t *idx1;
    size_t n1;
    const float *xyz2;
    size_t natoms2;
    const uint64_t *idx2;
    size_t n2;
    const float *vdw1;         /* DOUBLE_VDW: radii per SELECTED atom, length n1 / n2 */
    const float *vdw2;
    int32_t ids_local;
    const float *box9;
    uint8_t pbc;
    const float *lower3;       /* WITHIN non-periodic only */
    const float *upper3;
} molar_hip_search_desc;

/* Phase 1 (count): builds the cell grid on the GPU, evaluates every cell pair of the
 * reference's search plan, returns the number of results in reference order.  The request
 * stays cached in ctx for the fill calls (tpr_n* then tpr_fill_*, wrapper.hpp:48-61). */
int molar_hip_search_count(molar_hip_ctx *ctx, const molar_hip_search_desc *desc, uint64_t *out_count);
/* Phase 2 (fill), results in exactly the reference's order (plan order, then i-major, j-minor;
 * distance_search.rs:949-953).  pairs: uint32 [count][2] (i,j); dist: float[count] = sqrt(d2)
 * (DistanceSearchOutput for (usize,usize,Float), :22-26).  Either may be NULL to skip it.
 * Outputs in DEVICE memory should be aligned to 16 bytes (pairs) and 8 bytes (dist) - the fill pass
 * writes two results per lane and store instruction (hipMalloc and framework allocators give 256
 * bytes).  An offset view that is not aligned like that is filled through the context's own buffers
 * and copied device to device: the same result, one more pass over it. */
int molar_hip_search_fill(molar_hip_ctx *ctx, uint32_t *pairs, float *dist);
/* Same, widened to MolAR's usize: separate i[], j[] arrays of uint64. */
int molar_hip_search_fill_usize(molar_hip_ctx *ctx, uint64_t *i, uint64_t *j, float *dist);
/* WITHIN results (DistanceSearchOutput for usize, :10-14): ids of set-1 atoms, duplicates kept
 * exactly as the reference emits them (callers sort+dedup, selection_expr.rs:112). */
int molar_hip_search_fill_ids(molar_hip_ctx *ctx, uint64_t *ids);
/* `within <cutoff> [pbc] of <inner>` as the SET its callers keep (LogicalNode::Within, selection/ast.rs:589-631): the raw
 * stream of distance_search_within(_pbc) (distance_search.rs:519-598, one id per plan entry in which the atom has a hit)
 * goes through SortedSet::from_unsorted (selection_expr.rs:112), so what reaches the user is the sorted, de-duplicated
 * ids of the first-set atoms with a second-set atom within the cutoff.  This pair computes exactly that set without
 * the stream: same grid, same plan entries (wrap / drop rules, wrapped entries through PeriodicBox::distance_squared
 * over the entry's dims), but an atom stops looking at its first hit in ANY entry, and the set comes out of a flag
 * array in ascending order.  `desc` must be of kind MOLAR_HIP_SEARCH_WITHIN (non-periodic: lower3 / upper3 as for the
 * stream form); ids are what the stream would carry (idx1 values, or 0..n1 with ids_local).  The `self` keyword
 * (:627-629) is the caller's union with the inner selection.  ids: uint64[count], host or device. */
int molar_hip_within_count(molar_hip_ctx *ctx, const molar_hip_search_desc *desc, uint64_t *out_count);
int molar_hip_within_fill(molar_hip_ctx *ctx, uint64_t *ids);
/* Consecutive `within` requests against one frame (selection/ast.rs:589-631 evaluated for several inner selections or cutoffs;
 * within_size_bench.rs:13-47) name the same first set: with the hold on, a molar_hip_within_count whose request has the same
 * first-set pointers and sizes, the same box and periodicity and comes to the same grid reuses the staged coordinates and the
 * grid of the request before it.  The caller promises that those coordinates do not change while the hold is on (for a Rust
 * caller: while it holds the `&State`); any other search on the context, or on = 0, ends the reuse.  A first set in host
 * memory is additionally checked by a fingerprint of the array (both ends and 512 atoms spread over it), so a frame updated
 * in place - or a new array at the old address - is staged again; a set in device memory is read in place, and there the
 * promise is all there is: toggle the hold per frame. */
int molar_hip_within_hold(molar_hip_ctx *ctx, int on);
/* SearchConnectivity (molar/src/connectivity.rs:8-60: `for (i, j) in pairs { conn[i].push(j); conn[j].push(i) }`) of a
 * single-selection search, built on the device from the resident pair list.  CSR over the request's id range - local ids
 * (desc->ids_local): the selection's length; global ids: natoms - with every list in the reference's push order; an atom
 * without a pair has an empty list (the reference's map has no key for it).  Count-then-fill like the searches: the first
 * call runs the search (the request must be of kind MOLAR_HIP_SEARCH_SINGLE), builds the CSR in context-owned device memory
 * and returns rows and entries (= 2 x pairs, < 2^31: MOLAR_HIP_ERR_TOO_LARGE beyond); the second copies offsets[rows + 1] and
 * neigh[entries] to host or device memory.  The CSR is uint64 in both precisions: molar_hip_search_connectivity_fill is also
 * the fill call of molar_hip_search_connectivity_f64. */
int molar_hip_search_connectivity(molar_hip_ctx *ctx, const molar_hip_search_desc *desc, uint64_t *out_rows, uint64_t *out_entries);
int molar_hip_search_connectivity_fill(molar_hip_ctx *ctx, uint64_t *offsets, uint64_t *neigh);
/* Modify::unwrap_connectivity_dim (molar/src/modify.rs:72-131): neighbour search of the selection with local ids under
 * full PBC on the GPU, SearchConnectivity's adjacency in pair order (connectivity.rs:19-35) and the reference's stack
 * walk on the host - every atom is moved to the closest image (over `pbc_dims`) of the atom it was reached from.  xyz:
 * float[natoms][3], host or device, modified in place.  Returns the selections of the reference's result as a CSR of
 * LOCAL indices, each sorted (select(&sel_vec)); as there, the atom a connected component starts from is not a member
 * of its group and one-atom components give no group.  group_offsets: capacity n + 1 (or natoms + 1 with idx == NULL),
 * group_ids: capacity n; either may be NULL (the coordinates are unwrapped all the same, *ngroups is still counted).
 * Errors: MOLAR_HIP_ERR_NO_PBC without a box. */
int molar_hip_unwrap_connectivity(molar_hip_ctx *ctx, float *xyz, size_t natoms, const uint64_t *idx, size_t n,
                                  const float *box9, float cutoff, uint8_t pbc_dims, uint64_t *group_offsets,
                                  uint64_t *group_ids, size_t *ngroups);
/* Grid dims of the cached search (Grid::get_dims, :212-214). */
int molar_hip_search_grid_dims(molar_hip_ctx *ctx, uint64_t dims[3]);
/* Which pair kernels the context's last search of a fixed-cutoff kind ran: *lanes = 16 or 32 for the small-cell kernels (frames of
 * a few atoms per cell: contact / hydrogen-bond cutoffs), 0 for the regular ones, -1 / -2 for the instances that keep second cells
 * of up to 1024 / 2048 atoms in registers (frames of more than 448 / 1000 atoms per cell).  The choice follows the atoms per OCCUPIED cell
 * once a search of the same shape (kind, set sizes, grid dims) has finished on this context - every grid build counts its occupied
 * cells and the host learns the count with the result sizes - and the atoms per cell until then: a slab or a solute in a mostly
 * empty periodic box has few atoms per cell on average and many per occupied cell, and moves to the regular kernels from its
 * second or third frame on.  occupied_cells (may be NULL): the counts that search went by, 0 = not known then.  Diagnostic; the
 * results do not depend on the choice. */
int molar_hip_search_cell_kernels(molar_hip_ctx *ctx, int32_t *lanes, uint64_t occupied_cells[2]);
/* How the plan of the search this context prepared LAST was cut into slots (one wave of the count and fill passes each): the number
 * of slots it produced and the number that slots of 64 CONSECUTIVE rows per plan entry would have given.  Where the regular kernels
 * of the fixed-cutoff kinds cut slots from the rows of an entry that can have a hit at all (dense frames)
 * the first number is the smaller one; every other search that keeps the record - vdW and stream-form `within` searches included -
 * reports two equal numbers.  The numbers sit in device memory and are read when asked for: the call waits for the context's
 * stream, and with pipelined searches (molar_hip_search_resident_begin / _end) it answers for the search begun last, not for the
 * one ended last.  MOLAR_HIP_ERR_NO_SEARCH when the search prepared last kept no such record: plans of more than 2^22 entries, the
 * fused histograms of the fixed-cutoff kinds, `within` sets, contact counts.  Diagnostic; results do not depend on it. */
int molar_hip_search_slot_counts(molar_hip_ctx *ctx, uint64_t *slots, uint64_t *consecutive_slots);
/* Device-resident result of the cached search: fills ctx-owned buffers (reused across frames)
 * and returns their device addresses; valid until the next search on this ctx. */
int molar_hip_search_fill_device(molar_hip_ctx *ctx, const uint32_t **d_pairs, const float **d_dist);
/* The resident path in one call and ONE host round trip: count, offset scan and fill are enqueued back to back
 * into ctx-owned buffers sized by earlier frames of the trajectory; if a buffer turns out too small (first
 * frame) it grows and the affected pass repeats.  Same result, order and validity rules as
 * molar_hip_search_count + molar_hip_search_fill_device; the cached search stays available to the other fill
 * variants.  The result is complete in device memory when the call returns.  Not for WITHIN (ids, not pairs). */
int molar_hip_search_resident(molar_hip_ctx *ctx, const molar_hip_search_desc *desc, uint64_t *out_count,
                              const uint32_t **d_pairs, const float **d_dist);
/* Which planes the resident searches (molar_hip_search_resident, _begin / _end) fill: want_dist = 0 selects the
 * DistanceSearchOutput of (usize, usize) (distance_search.rs:14-20) - (i, j) only, 8 bytes per result, no square roots - for
 * consumers that never read the distances (SearchConnectivity, patches); the d_dist pointers then come back NULL.  Not while
 * pipelined searches are in flight.  Default: both planes. */
int molar_hip_search_resident_planes(molar_hip_ctx *ctx, int want_dist);
/* The same search split in two so that a per-frame loop never leaves the GPU idle: _begin enqueues everything for
 * one frame and returns at once with a ticket (0 or 1); _end waits for that frame only and returns its result.
 * Two searches may be in flight, each with its own result set, so the loop is
 *     begin(frame k+1); end(frame k); consume k; ...
 * and the host work of frame k+1 (and the result round trip of frame k) hides behind the kernels of frame k.
 * The kernels still run in order on the context's one stream.  A frame that outgrows a buffer is repeated inside
 * _end (after the younger search has drained), so `desc` and everything it points to must stay valid until _end.
 * A result set is valid until the second _begin after the one that produced it (ticket 0's set is also the one
 * molar_hip_search_resident and molar_hip_search_fill_device write: end the tickets before mixing those in).
 * On a context that owns its stream, with inputs already in device memory, the grid of the new frame is built on an
 * internal side stream while the kernels of the frame in flight run; the inputs must therefore be complete in
 * memory when _begin is called (a context created on a caller's stream keeps everything on that stream).  Errors: both sets in flight
 * (_begin), unknown or already finished ticket (_end). */
int molar_hip_search_resident_begin(molar_hip_ctx *ctx, const molar_hip_search_desc *desc, int32_t *ticket);
int molar_hip_search_resident_end(molar_hip_ctx *ctx, int32_t ticket, uint64_t *out_count, const uint32_t **d_pairs,
                                  const float **d_dist);
/* Consumer-fused variant: never materialises pairs; every emitted distance d goes through
 * Histogram1D::add_one (molar_membrane/src/stats.rs:29-35): b=floor(n*(d-min)/(max-min)),
 * counted in integers (bins: uint64[nbins], accumulated INTO, so frames can be summed).  With `bins` in device
 * memory the sum stays on the GPU, and with out_count == NULL the call returns without waiting for the kernels
 * (frames of a trajectory queue up back to back; molar_hip_synchronize before reading the bins).  Calls of that
 * asynchronous form on a context that owns its stream build their grid on the internal side stream under the
 * histogram kernel of the frame before: as for _begin, the inputs must be complete in memory at the call. */
int molar_hip_search_histogram(molar_hip_ctx *ctx, const molar_hip_search_desc *desc, float hmin,
                               float hmax, size_t nbins, uint64_t *bins, uint64_t *out_count);
/* The same for a block of a trajectory: `nframes` frames of the request's first set, frame k at desc->xyz1 + k * xyz1_stride
 * floats (second set: xyz2 + k * xyz2_stride), box of frame k at boxes9 + 9 k (NULL: desc->box9 for every frame) - the state
 * iterator of analysis_task.rs:245-252 / io.rs:198-271 handed over a window at a time.  The sums in `bins` are those of
 * nframes calls of molar_hip_search_histogram (integer bins do not care how their pairs are grouped).  Periodic requests of
 * kind SINGLE or DOUBLE whose coordinates, indices and bins are all in device memory, on a context that owns its stream, run in
 * groups of up to sixteen frames that share their launches - the grids of a group are built together on the side stream while the group before
 * is still in its histogram kernel, one plan launch and one persistent kernel walk the slots of all of them - and the call
 * does not wait (molar_hip_synchronize before reading the bins; the frames must be complete in memory at the call).  Anything
 * else is walked frame by frame through molar_hip_search_histogram. */
int molar_hip_search_histogram_frames(molar_hip_ctx *ctx, const molar_hip_search_desc *desc, size_t nframes, size_t xyz1_stride,
                                      size_t xyz2_stride, const float *boxes9, float hmin, float hmax, size_t nbins,
                                      uint64_t *bins);
/* Host arithmetic, no GPU: the table the fused histogram bins with.  Histogram1D::add_one's bin (stats.rs:29-35) is a
 * non-decreasing function of the squared distance; edges[b], b = 0..nbins (nbins + 1 floats), is the smallest
 * non-negative float d2 whose bin floor(n*(sqrt(d2)-min)/(max-min)) is >= b, found by bisection with the formula
 * itself, so "largest b with edges[b] <= d2" IS the formula.  INVALID_ARGUMENT unless min < max, both finite. */
int molar_hip_histogram_edges(float hmin, float hmax, size_t nbins, float *edges);

/* The second fused consumer: contact counts.  Never materialises pairs.  Let L be the list the search described by `desc`
 * emits, ids taken as POSITIONS IN THE SELECTION (desc->ids_local has no effect here).  L includes the reference's
 * duplicates - the same-cell cross pairs of the two-set search, and repeated cell pairs when a periodic dimension has two
 * cells or fewer - and the counts inherit them (the occupancy of the frames form is immune: it records "non-zero").
 *   *out_count = |L|.
 *   SINGLE: deg1[p] += entries with p as first OR second member (the length of SearchConnectivity's list of p); deg2 must be
 *           NULL; map is ngroups1 x ngroups1, row-major, and an entry (a, b) adds 1 at [min(g1[a], g1[b])][max(..)]: only the
 *           upper triangle with the diagonal is used (which member of a single-set entry comes first follows the plan).
 *   DOUBLE: deg1[p] += entries with first member p, deg2[p] += entries with second member p; map is ngroups1 x ngroups2 and
 *           [g1[a]][g2[b]] += 1.
 * Every output is uint64, accumulated INTO, host or device memory, and may be NULL (all NULL: the call only counts).
 * Atoms the reference drops (outside a non-periodic dimension of the grid) get 0.  With every requested output in device
 * memory and out_count == NULL the call returns without waiting (molar_hip_synchronize before reading) - except that labels
 * in DEVICE memory are checked on the device first, one 4-byte read-back per call; labels in host memory are checked on the
 * host.  INVALID_ARGUMENT: kinds WITHIN and DOUBLE_VDW, deg2 with SINGLE, a map without labels, a label >= ngroups (nothing
 * at all is added to any output then).  TOO_LARGE: ngroups1 * ngroups2 > 2^24 (the map is dense).  f32 only.  The call
 * works on a search state of its own: a cached search of the context (count -> fill, a held `within` grid) stays valid. */
typedef struct {
    const uint32_t *group1;   /* label per SELECTED atom of set 1, length n1 (host or device) */
    size_t ngroups1;
    const uint32_t *group2;   /* DOUBLE: labels of set 2, length n2; SINGLE: ignored */
    size_t ngroups2;
} molar_hip_contact_groups;

int molar_hip_search_contacts(molar_hip_ctx *ctx, const molar_hip_search_desc *desc, const molar_hip_contact_groups *groups /* may be NULL */,
                              uint64_t *deg1, uint64_t *deg2, uint64_t *map, uint64_t *out_count);
/* The same for a block of a trajectory (frames laid out as for molar_hip_search_histogram_frames): the sums are those of
 * nframes single calls, and occupancy[r][c] (uint32, the map's shape, accumulated INTO, host or device, may be asked for
 * without `map`) += 1 for every frame whose own contribution to map[r][c] is non-zero (a frame's own map is kept in 32 bits:
 * one frame may add fewer than 2^32 entries to one group pair).  Labels are checked once for the block.  The frames are walked one after the other; with every requested output in device memory the call does not wait. */
int molar_hip_search_contacts_frames(molar_hip_ctx *ctx, const molar_hip_search_desc *desc, const molar_hip_contact_groups *groups,
                                     size_t nframes, size_t xyz1_stride, size_t xyz2_stride, const float *boxes9,
                                     uint64_t *deg1, uint64_t *deg2, uint64_t *map, uint32_t *occupancy);

/* The third fused consumer: connected components of the contact graph (clusters, aggregates, leaflets, the pieces of a
 * selection).  Never materialises pairs.  The PARTICLES are the selected atoms of set 1 (ids = positions in the selection), or,
 * with labels groups->group1 / ngroups1 (one label per selected atom; group2 / ngroups2 are ignored), the groups: P = n1 or
 * ngroups1.  Two particles are joined when some entry (i, j) of the list L the search described by `desc` emits has its ends in
 * them (L's own f32 predicate, L taken as a set); the components are those of that graph over all P particles.  A label no atom
 * carries, and an atom the reference drops (outside a non-periodic dimension of the grid), is a component of its own.
 * Components are numbered 0 .. C-1 IN THE ORDER OF THEIR SMALLEST PARTICLE, so every output is unique: the same call gives the
 * same bits.  Outputs, each optional (NULL), host or device memory, sized by the caller from P alone, OVERWRITTEN:
 *   comp_of[P]     uint32: the component of each particle;
 *   sizes[P]       uint32: particles per component, entries C .. P-1 are 0;
 *   offsets[P + 1] uint64, members[P] uint32: the particles of component k are members[offsets[k] .. offsets[k + 1]), ascending;
 *                  entries C+1 .. P of offsets are P;
 *   *out_ncomponents = C (host memory).
 * The call is host-synchronous: everything is complete when it returns.  INVALID_ARGUMENT: any kind but
 * MOLAR_HIP_SEARCH_SINGLE, a label >= ngroups1 (labels are checked as for molar_hip_search_contacts; nothing is written then).
 * TOO_LARGE: P >= 2^31 - 2.  f32 only.  A component that is connected to its own periodic image is not told apart from any
 * other.  Like the contacts calls it works on a search state of its own: a cached search of the context stays valid. */
int molar_hip_search_clusters(molar_hip_ctx *ctx, const molar_hip_search_desc *desc, const molar_hip_contact_groups *groups /* may be NULL */,
                              uint32_t *comp_of, uint32_t *sizes, uint64_t *offsets, uint32_t *members, uint32_t *out_ncomponents);
/* The same for a block of a trajectory (frames laid out as for molar_hip_search_contacts_frames; set 1 only), each output
 * optional, host or device: ncomponents[f] and largest[f] (uint32, per frame: C and the size of the largest component,
 * overwritten), size_hist[P + 1] (uint64, ADDED INTO: size_hist[s] += the components of s particles, summed over the frames) and
 * comp_of_frames[nframes * P] (each frame's comp_of, overwritten).  Labels are checked once for the block.  The frames are
 * walked one after the other on one stream; the call is host-synchronous. */
int molar_hip_search_clusters_frames(molar_hip_ctx *ctx, const molar_hip_search_desc *desc, const molar_hip_contact_groups *groups,
                                     size_t nframes, size_t xyz1_stride, const float *boxes9, uint32_t *ncomponents, uint32_t *largest,
                                     uint64_t *size_hist, uint32_t *comp_of_frames);
/* Counters of the union-find, for measurements: out4 (may be NULL) receives what the clusters calls of this context added up
 * since the counters were switched on - [hits of the pair loop, hits that reached the forest (the ends are different particles
 * whose members cached in the wave differ), compare-and-swaps issued, path-shortening atomic minima issued] - then enable != 0
 * zeroes them and switches them on (the calls take an instrumented instance of the kernel), 0 switches them off.  Diagnostic;
 * results do not depend on it. */
int molar_hip_search_clusters_counters(molar_hip_ctx *ctx, int32_t enable, uint64_t *out4);

/* ------------------------------------------------------------------ hydrogen bonds
 * The third consumer of the two-set search, with the geometric definition GROMACS (gmx hbond), MDAnalysis
 * (HydrogenBondAnalysis) and VMD (hbonds) share; the reference has no such routine.  One frame and three selections: the
 * donors are set 1 of a request of kind MOLAR_HIP_SEARCH_DOUBLE, the acceptors its set 2 - of the SAME frame array (xyz2 == xyz1,
 * natoms2 == natoms1) - and the donors' hydrogens a CSR over the donors: the hydrogens of the donor at position p of set 1 are
 * the atoms h_idx[h_offsets[p] .. h_offsets[p + 1]) of the frame (none, one or several; nh = h_offsets[n1] entries in all).
 * (D, H, A) is a hydrogen bond when
 *   1. (D, A) is in the list L the search described by `desc` emits (its f32 predicate d2 <= cutoff^2, its grid, plan and wrap
 *      rules; L taken as a SET: its duplicates do not count twice),
 *   2. D and A are not the same atom of the frame,
 *   3. in f64 from the f32 coordinates, with minimum-image vectors over desc->pbc when there is a box (boxmath.hpp in double):
 *      MOLAR_HIP_HBOND_DHA_MIN: angle(D-H-A) >= angle_deg (MDAnalysis / VMD, usually 150);
 *      MOLAR_HIP_HBOND_HDA_MAX: angle(H-D-A) <= angle_deg (GROMACS, usually 30);
 *      a triple with a zero-length arm (H on D, or H on A) is never a bond,
 *   4. with max_ha > 0: |H -> A| <= max_ha.
 * The result is the sorted set of triples, ordered by (position of D in set 1, position of H in the CSR, position of A in set 2),
 * as frame atom indices uint32 [count][3], with the optional f64 columns dist_da = |D -> A|, dist_ha = |H -> A| and the angle of the
 * chosen kind in degrees (atan2(|u x v|, u . v)).  Integer atomics only and a sort: the same call gives the same bits.
 *
 * molar_hip_hbonds_count runs the search and the stages and keeps the result in the context; molar_hip_hbonds_fill copies it out
 * (each destination host or device memory, or NULL).  molar_hip_hbonds_counts does the same and adds, for every bond, 1 to
 * don_count[position of D] (length n1), acc_count[position of A] (length n2) and map[group1[D's position]][group2[A's position]]
 * (ngroups1 x ngroups2, row-major) - uint64, accumulated INTO, host or device memory, any of them NULL; label rules and the 2^24
 * cap of the map as for molar_hip_search_contacts.  Its result can be filled as well.
 *
 * molar_hip_hbonds_frames walks a block of frames one after the other (layout of molar_hip_search_histogram_frames: frame k at
 * desc->xyz1 + k * xyz_stride floats, box of frame k at boxes9 + 9 k, NULL: desc->box9 for every frame).  per_frame[k] is set to
 * the bonds of frame k (uint64, host or device); the counts accumulate over the frames; *out_total is the number of entries and
 * *out_unique the number of rows of the bond table.  Kept on the device for molar_hip_hbonds_frames_fill: the frames' lists one
 * after the other (frame_offsets[nframes + 1], uint64) with their columns, the TABLE of the block - the sorted distinct triples,
 * in the order above - with occupancy[row] = the number of frames the bond is present in (uint32), and bond_of_entry[entry] =
 * the table row of every entry (uint32): the sparse presence matrix frames x bonds.
 *
 * The calls replace the context's cached search like any other search (they run the resident two-set search for the (i, j) plane
 * and leave the setting of molar_hip_search_resident_planes as it was), and each form replaces the hydrogen-bond result of the
 * other.  Every call waits for its result.  f32 only.
 *   INVALID_ARGUMENT  a kind other than DOUBLE; xyz2 != xyz1 or natoms2 != natoms1; an h_idx entry >= natoms; h_offsets that do not
 *                     start at 0, decrease, or do not end at nh; angle_deg outside [0, 180]; max_ha < 0; an unknown angle kind; a
 *                     map without labels, a label >= ngroups; pipelined searches in flight (molar_hip_search_resident_begin)
 *   TOO_LARGE         nh or the acceptors >= 2^32; 2^31 - 1 entries or more in a frame or a block; ngroups1 * ngroups2 > 2^24
 *   NO_SEARCH         a fill without the count of its form
 * A request that is refused adds nothing to any output. */
enum {
    MOLAR_HIP_HBOND_DHA_MIN = 0,
    MOLAR_HIP_HBOND_HDA_MAX = 1
};
int molar_hip_hbonds_count(molar_hip_ctx *ctx, const molar_hip_search_desc *desc, const uint64_t *h_offsets, const uint64_t *h_idx,
                           size_t nh, int32_t angle_kind, double angle_deg, double max_ha, uint64_t *out_count);
int molar_hip_hbonds_fill(molar_hip_ctx *ctx, uint32_t *triples, double *dist_da, double *dist_ha, double *angle_deg);
int molar_hip_hbonds_counts(molar_hip_ctx *ctx, const molar_hip_search_desc *desc, const uint64_t *h_offsets, const uint64_t *h_idx,
                            size_t nh, int32_t angle_kind, double angle_deg, double max_ha, const molar_hip_contact_groups *groups,
                            uint64_t *don_count, uint64_t *acc_count, uint64_t *map, uint64_t *out_count);
int molar_hip_hbonds_frames(molar_hip_ctx *ctx, const molar_hip_search_desc *desc, const uint64_t *h_offsets, const uint64_t *h_idx,
                            size_t nh, int32_t angle_kind, double angle_deg, double max_ha, size_t nframes, size_t xyz_stride,
                            const float *boxes9, const molar_hip_contact_groups *groups, uint64_t *per_frame, uint64_t *don_count,
                            uint64_t *acc_count, uint64_t *map, uint64_t *out_total, uint64_t *out_unique);
int molar_hip_hbonds_frames_fill(molar_hip_ctx *ctx, uint64_t *frame_offsets, uint32_t *triples, double *dist_da, double *dist_ha,
                                 double *angle_deg, uint32_t *bond_of_entry, uint32_t *table, uint32_t *occupancy);

/* ---- Lifetime correlations of presence data: the intermittent (Luzar-Chandler) and the continuous (survival) correlation
 * numerators, the distribution of run lengths and per-row statistics of a sparse presence matrix frames x rows (gmx hbond
 * -ac / -life, MDAnalysis HydrogenBondAnalysis.lifetime and SurvivalProbability).  Hydrogen bonds are one case (the rows of the
 * bond table of molar_hip_hbonds_frames); contacts and the members of a shell (`within` sets per frame) are others.
 *   input: F = nframes, R = nrows; frame_offsets[F + 1] (uint64) and row_of_entry[E] (uint32), E = frame_offsets[F]: the
 *     entries of frame t are row_of_entry[frame_offsets[t] .. frame_offsets[t + 1]).  h_r(t) = 1 iff row r occurs among the
 *     entries of frame t (a row named twice in one frame counts once).  group_of_row[R] (uint32 labels below ngroups) puts
 *     every row into a group; NULL: one group (ngroups is not read).
 *   gap filling: gap = g >= 0 (MDAnalysis' intermittency) comes first: h'_r(u) = 1 iff h_r(u) = 1, or there are p < u < q with
 *     h_r(p) = h_r(q) = 1 and q - p - 1 <= g.  Everything below is defined on h'.
 *   curves per group G, uint64, for tau = 0 .. max_lag; the origins are t = 0, s, 2 s, ... (s = origin_stride >= 1) with
 *     t + tau <= F - 1, and count[tau] = (F - 1 - tau) / s + 1 is their number, a function of F, s and tau alone:
 *       inter[G][tau] = sum_{r in G} sum_t h'_r(t) h'_r(t + tau)                  (intermittent correlation, numerator)
 *       cont[G][tau]  = sum_{r in G} sum_t prod_{u = t .. t + tau} h'_r(u)        (continuous correlation / survival, numerator)
 *     laid out [ngroups][max_lag + 1].  C(tau) = (x[tau] / count[tau]) / (x[0] / count[0]) is the usual normalisation.
 *     MDAnalysis' other normalisation, the mean over the origins of per-origin ratios, is NOT computed.
 *   run_hist[G][l], l = 0 .. F, uint64, laid out [ngroups][F + 1]: the number of maximal runs of exactly l consecutive present
 *     frames in the rows of G (the lifetime distribution); entry 0 is always 0.
 *   per row, uint32 [R]: events[r] the number of runs, longest[r] the longest run, present[r] the number of present frames
 *     (after gap filling).
 * Every output may be NULL and is then not computed; each is host or device memory and is written, not accumulated into.
 * frame_offsets, row_of_entry and group_of_row may each be host or device memory (offsets in device memory are copied to the
 * host first: they are judged there).  Rows and labels in device memory are judged on the device before a kernel uses one as
 * an address.  Integer atomics only: the same call gives the same bits.  The call waits for its result.
 * molar_hip_hbonds_frames_lifetimes does the same on the block result the context keeps after molar_hip_hbonds_frames: the rows
 * are the rows of the bond table, and nothing is copied out and back (bond_of_entry is read where it lies; the nframes + 1
 * offsets, which the context keeps in host memory, are sent to the device).  Its outputs are sized by THAT block: R rows and F frames as
 * molar_hip_hbonds_frames_shape reports them (each pointer may be NULL), with *serial the number of blocks the context has
 * finished - a caller that kept the serial of the block it sized its outputs for knows from a different one that another block
 * has taken its place.
 *   ERR_SIZES         nrows == 0 or nframes == 0 (a block without a bond)
 *   INVALID_ARGUMENT  max_lag >= nframes; origin_stride == 0; offsets that do not start at 0, decrease, or end at E > 0 with
 *                     row_of_entry == NULL; a row >= nrows; a label >= ngroups
 *   TOO_LARGE         the bit matrix cannot be allocated; 2^32 entries or more; 2^31 frames or more; more than 2^32 rows
 *   NO_SEARCH         the chained call, or molar_hip_hbonds_frames_shape, without a block result
 * A call that is refused writes nothing.  One GPU; cross-correlations between rows are out of scope.
 * molar_hip_lifetimes_plan is a pure host function: the bytes of device workspace such a call allocates (kept by the context,
 * grows only: the bit matrix of nrows x (ceil(nframes / 64) + 1) 64-bit words, the origin masks and, with want_cont, one
 * histogram of ngroups x (nframes + 1) words; staging of host-memory arguments not included) and words_per_row =
 * ceil(nframes / 64).  ngroups == 0 stands for one group. */
int molar_hip_lifetimes_plan(size_t nframes, size_t nrows, size_t ngroups, int want_cont, size_t *workspace_bytes,
                             uint32_t *words_per_row);
int molar_hip_lifetimes(molar_hip_ctx *ctx, const uint64_t *frame_offsets, const uint32_t *row_of_entry, size_t nframes,
                        size_t nrows, const uint32_t *group_of_row, size_t ngroups, size_t max_lag, size_t origin_stride,
                        size_t gap, uint64_t *inter, uint64_t *cont, uint64_t *run_hist, uint32_t *events, uint32_t *longest,
                        uint32_t *present);
int molar_hip_hbonds_frames_shape(molar_hip_ctx *ctx, size_t *nframes, size_t *nrows, size_t *nentries, uint64_t *serial);
int molar_hip_hbonds_frames_lifetimes(molar_hip_ctx *ctx, const uint32_t *group_of_row, size_t ngroups, size_t max_lag,
                                      size_t origin_stride, size_t gap, uint64_t *inter, uint64_t *cont, uint64_t *run_hist,
                                      uint32_t *events, uint32_t *longest, uint32_t *present);

/* ---- the drivers for MolAR built with its `f64` feature (Float = f64, aliases.rs:10-13): every operation in double -
 * cell assignment, the predicate d2 <= cutoff^2 and the distances - results as (usize, usize, f64) columns or usize ids.
 * Same request / count-then-fill convention as above.  Coordinates, index lists, radii and the result columns may be host or
 * device memory (device memory is used in place); grid and plan are built on the device.  In f64 there are the eight drivers,
 * the fused histogram, `within` as a set, SearchConnectivity and unwrap_connectivity (below).  Still f32 only: the matrix-core
 * count, the resident and pipelined resident forms, the small-second-set `within` kernel and the grid hold
 * (molar_hip_within_hold), the fused contact counts (molar_hip_search_contacts), and the chained membrane frame. */
typedef struct {
    int32_t kind;
    double cutoff;
    const double *xyz1;
    size_t natoms1;
    const uint64_t *idx1;
    size_t n1;
    const double *xyz2;
    size_t natoms2;
    const uint64_t *idx2;
    size_t n2;
    const double *vdw1;
    const double *vdw2;
    int32_t ids_local;
    const double *box9;
    uint8_t pbc;
    const double *lower3;
    const double *upper3;
} molar_hip_search_desc_f64;
int molar_hip_search_count_f64(molar_hip_ctx *ctx, const molar_hip_search_desc_f64 *desc, uint64_t *out_count);
int molar_hip_search_fill_f64(molar_hip_ctx *ctx, uint64_t *i, uint64_t *j, double *dist);
int molar_hip_search_fill_ids_f64(molar_hip_ctx *ctx, uint64_t *ids);
int molar_hip_search_grid_dims_f64(molar_hip_ctx *ctx, uint64_t dims[3]);
/* The consumer-fused histogram in f64 (molar_hip_search_histogram with every operation in double): the pairs and distances
 * molar_hip_search_count_f64 + _fill_f64 report for the same request (kinds SINGLE, DOUBLE, DOUBLE_VDW; WITHIN is
 * INVALID_ARGUMENT), each distance through the f64 Histogram1D::add_one (stats.rs:29-35): b = floor(n*(d-min)/(max-min)),
 * kept if 0 <= b < n.  One pass, no pair list.  bins: uint64[nbins] in host or device memory, accumulated INTO; nbins in
 * 1..8192 and finite min < max, else INVALID_ARGUMENT.  out_count (may be NULL): pairs within the cutoff, binned or not
 * (= search_count_f64's count).  With device bins and out_count == NULL the call may return before the kernel ends
 * (molar_hip_synchronize before reading the bins); otherwise it waits.  A histogram call invalidates the cached f64
 * search: fill_f64 / fill_ids_f64 / grid_dims_f64 then return NO_SEARCH until the next search_count_f64. */
int molar_hip_search_histogram_f64(molar_hip_ctx *ctx, const molar_hip_search_desc_f64 *desc, double hmin, double hmax,
                                   size_t nbins, uint64_t *bins, uint64_t *out_count);
/* The same for a block of frames: frame k at desc->xyz1 + k * xyz1_stride doubles (second set: xyz2 + k * xyz2_stride), its
 * box at boxes9 + 9 k (NULL: desc->box9 for every frame).  The sums equal those of nframes calls of
 * molar_hip_search_histogram_f64; the frames are walked one after the other.  With device bins the call may return before
 * the last kernel ends. */
int molar_hip_search_histogram_frames_f64(molar_hip_ctx *ctx, const molar_hip_search_desc_f64 *desc, size_t nframes,
                                          size_t xyz1_stride, size_t xyz2_stride, const double *boxes9,
                                          double hmin, double hmax, size_t nbins, uint64_t *bins);
/* Host arithmetic, no GPU: the f64 twin of molar_hip_histogram_edges.  edges[b], b = 0..nbins (nbins + 1 doubles), is the
 * smallest non-negative double d2 whose bin floor(n*(sqrt(d2)-min)/(max-min)) is >= b, found by bisection over the ordered
 * bit patterns of the non-negative doubles with the formula itself, so "largest b with edges[b] <= d2" IS the formula.
 * INVALID_ARGUMENT unless min < max, both finite (and max - min finite), and nbins > 0. */
int molar_hip_histogram_edges_f64(double hmin, double hmax, size_t nbins, double *edges);
/* `within` as the SET its callers keep, in f64: molar_hip_within_count / _fill with every operation in double.  The result is
 * exactly sort + dedup of what molar_hip_search_count_f64 + _fill_ids_f64 return for the same request - same grid, same plan
 * entries, same predicate per candidate (wrapped entries classified by the adjacent image and decided by
 * PeriodicBox::distance_squared inside the band around the cutoff, as the stream's count pass does) - without the stream:
 * one pass in which an atom stops looking at its first hit in ANY entry, the set out of a flag array in ascending order, one
 * read-back (the count).  `desc` must be of kind MOLAR_HIP_SEARCH_WITHIN, else INVALID_ARGUMENT (non-periodic: lower3 /
 * upper3 as for the stream form); ids are what the stream would carry (idx1 values, or 0..n1 with ids_local), 32-bit on the
 * device (TOO_LARGE beyond).  ids: uint64[count], host or device, ascending, unique; with count == 0 the fill call has nothing
 * to write and returns OK.  The count call invalidates the cached f64 search (fill_f64 / fill_ids_f64 / grid_dims_f64 return
 * NO_SEARCH until the next search_count_f64); _fill_f64 without a count before it returns NO_SEARCH.  Not in f64: the kernel
 * for small second sets walked from the inner selection's side and the grid hold (molar_hip_within_hold) - f32-only tunings;
 * this form is correct for an inner selection of any size and walks every first-set cell for it. */
int molar_hip_within_count_f64(molar_hip_ctx *ctx, const molar_hip_search_desc_f64 *desc, uint64_t *out_count);
int molar_hip_within_fill_f64(molar_hip_ctx *ctx, uint64_t *ids);
/* SearchConnectivity of the f64 single-selection search (molar_hip_search_connectivity with every operation of the search in
 * double): runs the f64 search into context-owned device columns and builds the CSR on the device - entry 2p = (row i,
 * neighbour j), entry 2p + 1 = (row j, neighbour i), one stable sort by row - in the reference's push order.  Kind SINGLE
 * only (INVALID_ARGUMENT otherwise); rows = the selection's length for local ids, natoms for global ones; TOO_LARGE at
 * >= 2^31 entries.  There is no _fill_f64: the CSR is uint64 in both precisions and lives in the same context fields, so the
 * fill call is molar_hip_search_connectivity_fill. */
int molar_hip_search_connectivity_f64(molar_hip_ctx *ctx, const molar_hip_search_desc_f64 *desc, uint64_t *out_rows,
                                      uint64_t *out_entries);
/* Modify::unwrap_connectivity_dim with Float = f64: the contract of molar_hip_unwrap_connectivity - search over the selection
 * with local ids under FULL periodicity whatever pbc_dims, the reference's stack walk on the host (closest image over
 * pbc_dims, in double), the same quirks (start atom not a member of its group, one-atom components give no group, members
 * sorted), NO_PBC without a box.  xyz: double[natoms][3], host or device, modified in place. */
int molar_hip_unwrap_connectivity_f64(molar_hip_ctx *ctx, double *xyz, size_t natoms, const uint64_t *idx, size_t n,
                                      const double *box9, double cutoff, uint8_t pbc_dims, uint64_t *group_offsets,
                                      uint64_t *group_ids, size_t *ngroups);

/* ------------------------------------------------------------------ Measure (measure.rs) */

/* min_max :22-36 */
int molar_hip_min_max(molar_hip_ctx *ctx, const float *xyz, size_t natoms, const uint64_t *idx, size_t n,
                      float lower[3], float upper[3]);
/* center_of_geometry :39-47 */
int molar_hip_center_of_geometry(molar_hip_ctx *ctx, const float *xyz, size_t natoms, const uint64_t *idx,
                                 size_t n, float out[3]);
/* center_of_mass :60-75 (ERR_ZERO_MASS) */
int molar_hip_center_of_mass(molar_hip_ctx *ctx, const float *xyz, size_t natoms, const uint64_t *idx, size_t n,
                             const float *mass, float out[3]);
/* center_of_geometry_pbc_dims :156-168 / center_of_mass_pbc_dims :197-220 (ERR_NO_PBC if box9==NULL) */
int molar_hip_center_of_geometry_pbc(molar_hip_ctx *ctx, const float *xyz, size_t natoms, const uint64_t *idx,
                                     size_t n, const float *box9, uint8_t pbc, float out[3]);
int molar_hip_center_of_mass_pbc(molar_hip_ctx *ctx, const float *xyz, size_t natoms, const uint64_t *idx,
                                 size_t n, const float *mass, const float *box9, uint8_t pbc, float out[3]);
/* gyration :78-87, gyration_pbc :222-232 (box9 != NULL) */
int molar_hip_gyration(molar_hip_ctx *ctx, const float *xyz, size_t natoms, const uint64_t *idx, size_t n,
                       const float *mass, const float *box9, float *out);
/* inertia :90-99 / inertia_pbc :234-244: moments ascending, axes column-major (cols = axes);
 * tensor9 (optional) receives the raw tensor (column-major). */
int molar_hip_inertia(molar_hip_ctx *ctx, const float *xyz, size_t natoms, const uint64_t *idx, size_t n,
                      const float *mass, const float *box9, float moments[3], float axes9[9], float tensor9[9]);
/* rmsd :485-504 (ERR_SIZES), rmsd_mw :538-558 (masses of selection 1) */
int molar_hip_rmsd(molar_hip_ctx *ctx, const float *xyz1, size_t natoms1, const uint64_t *idx1, size_t n1,
                   const float *xyz2, size_t natoms2, const uint64_t *idx2, size_t n2, float *out);
int molar_hip_rmsd_mw(molar_hip_ctx *ctx, const float *xyz1, size_t natoms1, const uint64_t *idx1, size_t n1,
                      const float *mass1, const float *xyz2, size_t natoms2, const uint64_t *idx2, size_t n2,
                      float *out);
/* fit_transform :507-522 / fit_transform_at_origin :525-535 (at_origin != 0):
 * IsometryMatrix3 as R (column-major) and t, p -> R p + t. */
int molar_hip_fit_transform(molar_hip_ctx *ctx, const float *xyz1, size_t natoms1, const uint64_t *idx1,
                            size_t n1, const float *mass1, const float *xyz2, size_t natoms2,
                            const uint64_t *idx2, size_t n2, const float *mass2, int at_origin, float R9[9],
                            float t3[3]);

/* ---- MolAR built with its `f64` feature (Float = f64: molar/src/aliases.rs:10-13, molar/Cargo.toml:56-60).
 * The Measure / Modify methods (centres, gyration, rmsd, fit, inertia, min_max, apply, translate, periodic centres and unwrap) on double-precision coordinates and masses, same argument meaning and
 * error codes as the f32 entries above; every per-atom term is formed and accumulated in f64 (two passes where the
 * reference has two: centre, then centred terms).  The f64 search entries are listed with the search above. */
/* center_of_geometry :39-47, center_of_mass :60-75 (ERR_ZERO_MASS) */
int molar_hip_center_of_geometry_f64(molar_hip_ctx *ctx, const double *xyz, size_t natoms, const uint64_t *idx,
                                     size_t n, double out[3]);
int molar_hip_center_of_mass_f64(molar_hip_ctx *ctx, const double *xyz, size_t natoms, const uint64_t *idx, size_t n,
                                 const double *mass, double out[3]);
/* gyration :78-87 */
int molar_hip_gyration_f64(molar_hip_ctx *ctx, const double *xyz, size_t natoms, const uint64_t *idx, size_t n,
                           const double *mass, double *out);
/* rmsd :485-504 (ERR_SIZES), rmsd_mw :538-558 */
int molar_hip_rmsd_f64(molar_hip_ctx *ctx, const double *xyz1, size_t natoms1, const uint64_t *idx1, size_t n1,
                       const double *xyz2, size_t natoms2, const uint64_t *idx2, size_t n2, double *out);
int molar_hip_rmsd_mw_f64(molar_hip_ctx *ctx, const double *xyz1, size_t natoms1, const uint64_t *idx1, size_t n1,
                          const double *mass1, const double *xyz2, size_t natoms2, const uint64_t *idx2, size_t n2,
                          double *out);
/* fit_transform :507-522 / fit_transform_at_origin :525-535: R column-major, p -> R p + t */
int molar_hip_fit_transform_f64(molar_hip_ctx *ctx, const double *xyz1, size_t natoms1, const uint64_t *idx1,
                                size_t n1, const double *mass1, const double *xyz2, size_t natoms2,
                                const uint64_t *idx2, size_t n2, const double *mass2, int at_origin, double R9[9],
                                double t3[3]);
/* min_max :22-36; inertia :90-99 (moments ascending, axes column-major, optional raw tensor); translate modify.rs:16-23 */
int molar_hip_min_max_f64(molar_hip_ctx *ctx, const double *xyz, size_t natoms, const uint64_t *idx, size_t n,
                          double lower[3], double upper[3]);
int molar_hip_inertia_f64(molar_hip_ctx *ctx, const double *xyz, size_t natoms, const uint64_t *idx, size_t n,
                          const double *mass, double moments[3], double axes9[9], double tensor9[9]);
int molar_hip_translate_f64(molar_hip_ctx *ctx, double *xyz, size_t natoms, const uint64_t *idx, size_t n,
                            const double shift3[3]);

/* ---- Solvent-accessible surface area per atom (Measure::sasa, measure.rs:427; pymolar sel.sasa().areas / .total_area).
 * The reference delegates to an analytic power-diagram crate; this library computes the same quantity by Shrake-Rupley,
 * defined operation by operation so that the exposed-point counts are exact integers (Real = float, or double for _f64):
 *   R_i = vdw_i + probe.  Points u_k, k < npoints: z = 1 - (2k+1)/npoints, r = sqrt(1 - z z), phi = k (pi (3 - sqrt 5)),
 *   u_k = (r cos phi, r sin phi, z), computed on the host in double, then rounded to Real (molar_hip_sasa_points).
 *   j != i is a neighbour of i iff (dx dx + dy dy) + dz dz < (R_i + R_j)(R_i + R_j), d = c_j - c_i (strict compare).
 *   Point k of i is buried iff a neighbour j has (tx tx + ty ty) + tz tz < R_j R_j, t = R_i u_k - d.  No contraction.
 *   exposed_i = points not buried; area_i = ((4 pi R_i^2) exposed_i) / npoints in double, rounded to Real;
 *   total = sum of the areas in double (fixed order).
 * An atom with a non-finite coordinate or radius or with R_i <= 0 gets exposed = 0, area = 0 and buries nothing.  No periodic
 * box (the reference's sasa() takes none).  npoints in 1..4096, probe finite and >= 0, else ERR_INVALID_ARGUMENT.
 * idx == NULL: atoms 0 .. n-1, all atoms when n is 0 (n > natoms: ERR_INVALID_ARGUMENT); an empty selection (idx != NULL,
 * n == 0) is no error, its total is 0.  vdw: one radius per SELECTED atom, selection order.  Every pointer may be host
 * or device memory; areas, exposed and total are optional (NULL). */
int molar_hip_sasa_points(uint32_t npoints, float *out_xyz);
int molar_hip_sasa_points_f64(uint32_t npoints, double *out_xyz);
int molar_hip_sasa(molar_hip_ctx *ctx, const float *xyz, size_t natoms, const uint64_t *idx, size_t n, const float *vdw,
                   float probe, uint32_t npoints, float *areas, uint32_t *exposed, double *total);
int molar_hip_sasa_f64(molar_hip_ctx *ctx, const double *xyz, size_t natoms, const uint64_t *idx, size_t n,
                       const double *vdw, double probe, uint32_t npoints, double *areas, uint32_t *exposed, double *total);
/* the same over nframes frames, frame f at frames + f * frame_stride (floats, >= 3 natoms): every frame is enqueued behind the
 * one before it and the call waits once; areas[nframes][n] (optional), totals[nframes]; frame by frame the results are
 * those of molar_hip_sasa bit for bit */
int molar_hip_sasa_frames(molar_hip_ctx *ctx, const float *frames, size_t nframes, size_t frame_stride, size_t natoms,
                          const uint64_t *idx, size_t n, const float *vdw, float probe, uint32_t npoints, float *areas,
                          double *totals);

/* ---- Per-atom volumes with the areas (Measure::sasa_vol, measure.rs:435; Sasa::volumes / total_volume, sasa.rs:92,97;
 * pymolar sel.sasa_vol().volumes / .total_volume).  volume_i is the volume of atom i's ball inside its power cell (the
 * points whose power distance |x - c_i|^2 - R_i^2 is smallest for i); the volumes add up to the volume of the union of the
 * balls.  Evaluated on the point table of the areas: along u_k from c_i the ray stays inside the ball and the power cell on
 * an interval [lo_k, hi_k], and the cone around u_k contributes (hi_k^3 - lo_k^3) / 3 times 4 pi / npoints.  Operation by
 * operation (Real = float, or double for _f64; no contraction; R_i, u_k, the neighbour filter with
 * dd = (dx dx + dy dy) + dz dz, d = c_j - c_i, and the atoms that take no part exactly as for molar_hip_sasa):
 *   lo_k = 0, hi_k = R_i for every k.  Per neighbour j, in any order (only min and max are taken):
 *     c = ((dd + R_i R_i) - R_j R_j) * 0.5;  a = (u_kx dx + u_ky dy) + u_kz dz;  t = c / a (IEEE division);
 *     a > 0 and t < hi_k: hi_k = t;   a < 0 and t > lo_k: lo_k = t;   a == 0 and c < 0: hi_k = 0;
 *     anything else (NaN, an infinite t that fails its compare) changes nothing.
 *   hi_k = max(hi_k, lo_k): an empty interval contributes 0.
 *   s_i = sum over k of (double)hi_k^3 - (double)lo_k^3, cubes and sum in double;
 *   volume_i = ((4 pi / 3) s_i) / npoints in double, rounded to Real;  total_volume = sum of the volumes in double, in the
 *   fixed order of the areas' total.
 * A non-neighbour's radical plane never enters ball i, so the filter changes nothing but the work.  An atom that takes no
 * part gets volume 0 and cuts nobody.  Coincident atoms of equal radius (a == 0 and c == 0 for every k)
 * each keep their full ball: there the volumes add up to more than the union.  exposed, areas and total are those of
 * molar_hip_sasa on the same input bit for bit.  Arguments, checks and errors as for the three calls above; every output
 * pointer is optional. */
int molar_hip_sasa_vol(molar_hip_ctx *ctx, const float *xyz, size_t natoms, const uint64_t *idx, size_t n, const float *vdw,
                       float probe, uint32_t npoints, float *areas, uint32_t *exposed, double *total, float *volumes,
                       double *total_volume);
int molar_hip_sasa_vol_f64(molar_hip_ctx *ctx, const double *xyz, size_t natoms, const uint64_t *idx, size_t n,
                           const double *vdw, double probe, uint32_t npoints, double *areas, uint32_t *exposed, double *total,
                           double *volumes, double *total_volume);
/* frames as in molar_hip_sasa_frames: areas[nframes][n], totals[nframes], volumes[nframes][n], total_volumes[nframes]; frame
 * by frame the results are those of molar_hip_sasa_vol bit for bit */
int molar_hip_sasa_vol_frames(molar_hip_ctx *ctx, const float *frames, size_t nframes, size_t frame_stride, size_t natoms,
                              const uint64_t *idx, size_t n, const float *vdw, float probe, uint32_t npoints, float *areas,
                              double *totals, float *volumes, double *total_volumes);

/* ---- All-pairs minimum RMSD over the frames of a block, or of one block against another: out[a][b] is the rmsd_mw of frame
 * a after the mass-weighted fit_transform onto frame b (measure.rs:507-522 with :538-558; with unit masses the fit followed by
 * rmsd, :485-504), for every pair at once from one Gram product on the f64 matrix cores instead of one fit_rmsd_batch call per
 * reference frame.  Frame f of a block is at frames + f * frame_stride (elements, >= 3 natoms, as for molar_hip_sasa_frames).
 * Operation by operation (Real = float, or double for _f64; everything below is formed and accumulated in double from the
 * exact inputs, only the result is rounded to Real):
 *   selection idx[0..n), shared by all frames; idx == NULL: atoms 0 .. n-1.  w_k = mass[idx[k]] (mass: one per ATOM, >= 0);
 *   mass == NULL: w_k = 1.  W = sum_k w_k.
 *   fit != 0:  c_f = sum_k w_k p_f,k / W,  x_f,k = p_f,k - c_f,  q_f,k = sqrt(w_k) x_f,k,  G_f = sum_k |q_f,k|^2,
 *     C_ab = sum_k q_a,k q_b,k^T (3x3),  lambda = largest eigenvalue of Horn's 4x4 matrix of C_ab (the maximum of
 *     sum_k w_k (R x_a,k) . x_b,k over PROPER rotations R: a mirror image does not give 0),
 *     out[a][b] = sqrt(max(0, (G_a + G_b) - 2 lambda) / W).
 *   fit == 0:  no superposition, out[a][b] = sqrt(sum_k w_k |p_a,k - p_b,k|^2 / W), by the same route with trace(C_ab) in
 *     place of lambda and ONE origin in place of the centres: c_0 of the first block (if that frame holds a non-finite
 *     coordinate, the first finite centre of the first block).
 *   All sums have a fixed order that depends on the sizes alone (no floating-point atomics): the same call gives the same bits.
 *   The products of the Gram matrix are the matrix cores' (v_mfma_f64_16x16x4_f64), so results are bounded, not fixed
 *   bit for bit:  |out^2 - exact^2| <= (3 n + 16) 2^-53 (G_a + G_b) / W + 4 eps exact^2, eps = 2^-24 (2^-53 for _f64).
 * frames2 == NULL (symmetric form): out is [nframes1][ld] over the pairs of block 1; only pairs with b >= a are computed and
 *   each is stored twice, so out[a][b] == out[b][a] bit for bit, and out[a][a] is exactly 0.  nframes2 / frame_stride2 are
 *   not read.
 * frames2 != NULL (rectangular form): block 1 against block 2, out is [nframes1][ld] with nframes2 columns used (the rest of a
 *   row is not touched); both blocks share natoms, idx and mass.  frames2 == frames1 is still the rectangular form.
 * frames, idx, mass and out may each be host or device memory.  A device `out` is written on the context's stream and not
 * waited for (the call itself waits once, early, for the 16 bytes that decide its status).
 * Errors: n == 0 or ld below the column count: ERR_SIZES; W == 0: ERR_ZERO_MASS; an index not below natoms, n > natoms without
 * an index, a stride below 3 natoms: ERR_INVALID_ARGUMENT; a workspace that cannot be allocated: ERR_TOO_LARGE with the byte
 * count in molar_hip_last_error().  nframes1 == 0 (or nframes2 == 0 in the rectangular form) is a successful no-op.  A frame
 * with a non-finite selected coordinate gives NaN in its row and column (its diagonal entry included) and leaves every other
 * entry as it would be without that frame; the status stays MOLAR_HIP_OK.
 * molar_hip_rmsd_matrix_plan is a pure host function: the bytes of device workspace such a call allocates (kept by the
 * context and reused; staging of host-memory arguments not included; never smaller for a larger argument) and the number of
 * workgroups the atom dimension is split over (1: the finish is fused into the Gram kernel).  nframes2 == 0: symmetric. */
int molar_hip_rmsd_matrix_plan(size_t nframes1, size_t nframes2, size_t n, size_t *workspace_bytes, uint32_t *ksplits);
int molar_hip_rmsd_matrix(molar_hip_ctx *ctx, const float *frames1, size_t nframes1, size_t frame_stride1,
                          const float *frames2, size_t nframes2, size_t frame_stride2, size_t natoms, const uint64_t *idx,
                          size_t n, const float *mass, int fit, float *out, size_t ld);
int molar_hip_rmsd_matrix_f64(molar_hip_ctx *ctx, const double *frames1, size_t nframes1, size_t frame_stride1,
                              const double *frames2, size_t nframes2, size_t frame_stride2, size_t natoms,
                              const uint64_t *idx, size_t n, const double *mass, int fit, double *out, size_t ld);

/* ---- Fluctuations of a block of trajectory frames about their mean structure: the mean, the per-atom RMSF and the 3n x 3n
 * positional covariance (the input of a principal-component analysis), after an optional mass-weighted fit of every frame
 * onto a reference, in one call instead of fit_rmsd_batch(apply) on a copy of the block followed by reductions.  Frame f is
 * at frames + f * frame_stride (elements, >= 3 natoms), as for molar_hip_rmsd_matrix.  Operation by operation (Real = float,
 * or double for _f64; everything below is formed and accumulated in double from the exact inputs, only the results are
 * rounded to Real; F = nframes):
 *   selection idx[0..n), shared by all frames; idx == NULL: atoms 0 .. n-1.  w_k = mass[idx[k]] (mass: one per ATOM, >= 0);
 *   mass == NULL: w_k = 1.  W = sum_k w_k.  c_f = sum_k w_k x_f,k / W.
 *   reference r_k: ref[k] (the selected atoms packed, [n][3]); ref == NULL: x_0,k.  c_ref = sum_k w_k r_k / W, y_k = r_k - c_ref.
 *   fit != 0:  R_f = the proper rotation that minimises sum_k w_k |R (x_f,k - c_f) - y_k|^2: the dominant eigenvector of
 *     Horn's 4x4 matrix of S_f = sum_k w_k (x_f,k - c_f) y_k^T by Jacobi sweeps at f64 working precision, as a rotation
 *     matrix, followed by one Newton step R <- R + R (I - R^T R) / 2 (R^T R = I to a few 2^-53).  z_f,k = R_f (x_f,k - c_f) + c_ref;  t_f = c_ref - R_f c_f, so that p' = R p + t is fit_rmsd_batch's convention.
 *     Where the optimal rotation is not unique (n < 3, collinear selections) any optimal proper rotation is a correct answer.
 *   fit == 0:  z_f,k = x_f,k.  Internally every frame is taken about ONE origin, c_0 (if frame 0 holds a non-finite coordinate,
 *     the first finite c_f), so that the cancellation below happens at the scale of the structure.
 *   mean_k = (1/F) sum_f z_f,k;  rmsf_k = sqrt((1/F) sum_f |z_f,k - mean_k|^2);
 *   cov[3k+d][3l+e] = (1/F) sum_f (z_f,k,d - mean_k,d) (z_f,l,e - mean_l,e):  two passes - the mean is finished first and
 *     the deviations are taken about it, never E[z z] - m m.  Unweighted, in nm and nm^2 (the mass-weighted covariance is a
 *     row and column scaling).  Atoms of zero weight still get their mean, rmsf and covariance.
 *   iterations = I > 0 (fit != 0 only; ignored otherwise): after a pass its mean, kept in f64 on the device, becomes the
 *     reference and the frames are fitted again: 1 + I passes, the outputs are those of the last one.
 *   fit_out[f] = {R_f (9, column-major), t_f (3), sqrt(sum_k w_k |z_f,k - r_k|^2 / W)} against the reference of the last
 *     pass, the distance by the Gram route (sum w |x - c_f|^2 + sum w |y|^2 - 2 sum w (R x) . y).  fit == 0: R = I, t = 0 and
 *     the distance of the frame as it stands.
 *   cov is computed on the f64 matrix cores (v_mfma_f64_16x16x4_f64, K = frames) for the tiles on and above the diagonal and
 *     every entry is stored twice: cov[i][j] == cov[j][i] bit for bit.  cov is [3n][ld], ld >= 3n; the rest of a row is not
 *     touched.
 *   All sums have a fixed order that depends on the sizes alone (no floating-point atomics): the same call gives the same bits.
 * Every output (mean [n][3], rmsf [n], cov, fit_out [nframes][13]) may be NULL and is then not computed; frames, idx, mass,
 * ref and every output may each be host or device memory.  Device outputs are written on the context's stream and not waited
 * for (the call itself waits once, early, for the 16 bytes that decide its status).
 * Errors: n == 0, or cov != NULL with ld below 3n: ERR_SIZES; W == 0: ERR_ZERO_MASS; an index not below natoms, n > natoms
 * without an index, a stride below 3 natoms (with more than one frame: the stride of a single frame is not read, as for
 * molar_hip_rmsd_matrix), iterations < 0: ERR_INVALID_ARGUMENT; a workspace or a covariance that cannot be allocated, more
 * than 65535 * 4096 selected atoms, a covariance of more than 65532 * 16 coordinates: ERR_TOO_LARGE with the byte count in molar_hip_last_error().  nframes == 0 is a successful no-op.  A frame with a
 * non-finite selected coordinate gives NaN in its own fit_out row and in every entry of mean, rmsf and cov that it enters
 * (with a fit: all of them); the status stays MOLAR_HIP_OK and nothing is read back for it.
 * molar_hip_fluct_plan is a pure host function: the bytes of device workspace such a call allocates (kept by the context,
 * grows only; staging of host-memory arguments not included; never smaller for a larger argument, and never larger without
 * the covariance than with it) and the number of workgroups the frames of the covariance are split over (1: the scaling and
 * the mirrored store are fused into the covariance kernel; always 1 with want_cov == 0). */
int molar_hip_fluct_plan(size_t nframes, size_t n, int want_cov, size_t *workspace_bytes, uint32_t *ksplits);
int molar_hip_fluct(molar_hip_ctx *ctx, const float *frames, size_t nframes, size_t frame_stride, size_t natoms,
                    const uint64_t *idx, size_t n, const float *mass, const float *ref, int fit, int iterations, float *mean,
                    float *rmsf, float *cov, size_t ld, float *fit_out);
int molar_hip_fluct_f64(molar_hip_ctx *ctx, const double *frames, size_t nframes, size_t frame_stride, size_t natoms,
                        const uint64_t *idx, size_t n, const double *mass, const double *ref, int fit, int iterations,
                        double *mean, double *rmsf, double *cov, size_t ld, double *fit_out);

/* ---- Mean-squared displacement of a block of trajectory frames: the no-jump unwrap of every selected atom along time, the
 * displacement of each particle (an atom, or the centre of mass of a group of atoms), the optional removal of the drift of a
 * reference set, and MSD(tau), its fourth moment and the per-particle curves over all time origins, in one call (gmx msd,
 * MDAnalysis EinsteinMSD).  Frame f is at frames + f * frame_stride (elements, >= 3 natoms), as for molar_hip_rmsd_matrix.
 * Operation by operation (Real = float, or double for _f64; everything below is formed and accumulated in double from the
 * exact inputs, only the outputs are rounded to Real; F = nframes):
 *   selection idx[0..n), shared by all frames; idx == NULL: atoms 0 .. n-1.  w_k = mass[idx[k]] (mass: one per ATOM, >= 0);
 *   mass == NULL: w_k = 1.
 *   boxes: one column-major box9 for all frames (box_stride == 0) or [F][9] (box_stride == 9), made a PeriodicBox in double
 *     (from_matrix: inverse and triclinic corrections); boxes == NULL or pbc == 0: the trajectory is taken as already
 *     unwrapped and no image is removed.  pbc is the PbcDims byte.
 *   no-jump displacement, per selected atom k:  u_k(0) = 0;  for f >= 1  s = x_k(f) - x_k(f-1) (exact in double for float
 *     inputs),  d = shortest_vector_dims(box_f, s, pbc) (periodic_box.rs:286-318: fractional rounding half away from zero on
 *     the periodic dimensions, the triclinic image search for the full mask only),  u_k(f) = u_k(f-1) + d, added in frame
 *     order.  The box of the LATER frame is used: the displacement ("toroidal-view") scheme, valid under a fluctuating box.
 *   particles: group_offsets[nparticles + 1] is a CSR over the selection order, atoms [off[g], off[g+1]) of the selection
 *     form particle g; group_offsets == NULL: every selected atom is a particle, P = n (nparticles is not read).
 *     U_g(f) = sum_k w_k u_k(f) / W_g over the atoms of g in index order (a group of more than 256 atoms: in pieces of 256,
 *     each by a fixed tree, the pieces in order), W_g = sum_k w_k: the displacement of the group's centre of mass, correct
 *     even when the molecule is split across the box in frame 0, because only displacements enter.
 *   drift removal: ref_idx[0..nref) is a second selection (ref_idx == NULL: atoms 0 .. nref-1), weighted with mass;
 *     D(f) = its weighted mean no-jump displacement, U_g(f) -= D(f).  nref == 0: none.
 *   lags: msd_dims (bits x, y, z; 1 .. 7) picks the components of r^2 = sum_d Delta_d^2, Delta = U_g(t+tau) - U_g(t); the
 *     origins are t = 0, origin_stride, 2 origin_stride, ... while t + tau <= F - 1, count[tau] their number.  For
 *     tau = 0 .. max_lag:  msd[tau] = sum_g sum_t r^2 / (P count[tau]);  m4[tau] the same with r^4 (the non-Gaussian
 *     parameter is ndims / (ndims + 2) * m4 / msd^2 - 1);  msd_particle[g][tau] = sum_t r^2 / count[tau], laid out [P][ld],
 *     ld >= max_lag + 1, the rest of a row is not touched.  msd[0] is exactly 0.  r^2 and the sum of r^4 are formed with
 *     fused multiply-adds.
 *   disp [F][P][3]: the U_g(f) themselves, the unwrapped particle trajectory relative to frame 0.
 *   All sums have a fixed order that depends on the sizes alone (no floating-point atomics): the same call gives the same bits.
 * Every output (msd [max_lag+1], m4 [max_lag+1], msd_particle, disp) may be NULL and is then not computed; with only disp
 * asked for the lag kernel does not run.  frames, idx, mass, boxes, group_offsets, ref_idx and every output may each be host
 * or device memory (group_offsets in device memory are copied to the host first: they decide the launch geometry).  Device
 * outputs are written on the context's stream and not waited for (the call itself waits once, after the unwrap, for the 16
 * bytes that decide its status).
 * Errors: n == 0, msd_particle != NULL with ld below max_lag + 1, offsets that do not start at 0, are not increasing (an empty
 * group) or do not end at n: ERR_SIZES; W_g == 0 for a particle or for the reference set: ERR_ZERO_MASS; max_lag >= nframes
 * (with nframes >= 1), origin_stride == 0, msd_dims == 0 or > 7, pbc > 7, a box_stride other than 0 and 9, an index not below
 * natoms, natoms == 0, n (or nref) > natoms without an index, a stride below 3 natoms (with more than one frame):
 * ERR_INVALID_ARGUMENT; pbc != 0 with boxes == NULL: ERR_NO_PBC; a box with a vector of zero length:
 * ERR_ZERO_LENGTH_VECTOR, one without an inverse: ERR_INVERSE_FAILED (as PeriodicBox::from_matrix); a workspace or a result that cannot be allocated: ERR_TOO_LARGE with the byte count in
 * molar_hip_last_error().  The errors of the arguments alone are reported before the context is used.  nframes == 0 is a
 * successful no-op.  A non-finite selected coordinate gives NaN in its
 * particle's disp from that frame on, in that particle's row of msd_particle and in every msd / m4 entry the particle
 * enters; rows of other particles are as without it; with drift removal and the atom in the reference set everything is
 * NaN; the status stays MOLAR_HIP_OK and nothing is read back for it.
 * molar_hip_msd_plan is a pure host function: the bytes of device workspace such a call allocates (kept by the context,
 * grows only; staging of host-memory arguments not included; never smaller for a larger argument; per_frame_boxes: the
 * call has box_stride == 9 and pbc != 0; want_lags == 0: only disp is asked for, and nothing is reserved for the lag
 * stage) and the two launch-shape sizes of the lag kernel: particle_chunk, the particles a workgroup adds in order, and
 * lag_block, the lags of a workgroup (one lane each). */
int molar_hip_msd_plan(size_t nframes, size_t n, size_t nparticles, size_t nref, size_t max_lag, int per_frame_boxes,
                       int want_lags, size_t *workspace_bytes, uint32_t *particle_chunk, uint32_t *lag_block);
int molar_hip_msd(molar_hip_ctx *ctx, const float *frames, size_t nframes, size_t frame_stride, size_t natoms,
                  const uint64_t *idx, size_t n, const float *mass, const float *boxes, size_t box_stride, uint8_t pbc,
                  const uint64_t *group_offsets, size_t nparticles, const uint64_t *ref_idx, size_t nref, size_t max_lag,
                  size_t origin_stride, uint32_t msd_dims, float *msd, float *m4, float *msd_particle, size_t ld,
                  float *disp);
int molar_hip_msd_f64(molar_hip_ctx *ctx, const double *frames, size_t nframes, size_t frame_stride, size_t natoms,
                      const uint64_t *idx, size_t n, const double *mass, const double *boxes, size_t box_stride,
                      uint8_t pbc, const uint64_t *group_offsets, size_t nparticles, const uint64_t *ref_idx, size_t nref,
                      size_t max_lag, size_t origin_stride, uint32_t msd_dims, double *msd, double *m4,
                      double *msd_particle, size_t ld, double *disp);

/* ---- Density profiles and density maps of a block of trajectory frames: every selected atom of every frame is put into a
 * bin of a regular grid by its position, and the bins' sums of weights per unit volume are averaged over the frames (gmx
 * density with -center / -relative, gmx densmap, VMD volmap / gmx spatial on fitted frames).  The frame block, idx, boxes,
 * box_stride and pbc are those of molar_hip_msd.  Operation by operation (Real = float, or double for _f64; positions,
 * centres and bin coordinates are formed in double from the exact inputs; F = nframes):
 *   selection idx[0..n), idx == NULL: atoms 0 .. n-1.  w_k = weight[idx[k]] (one per ATOM, any sign: masses, charges,
 *     electron counts); weight == NULL: number density, w_k = 1.  labels[n] (one per SELECTED atom) below ngroups gives the
 *     group g of an atom; labels == NULL: one group, G = 1 (ngroups is not read).
 *   grid: nbins[d] bins along dimension d (1 integrates over it: (1,1,nz) is a profile along z, (nx,ny,1) a lateral map,
 *     (nx,ny,nz) a volume map), bin index (bx ny + by) nz + bz, nb = nx ny nz < 2^31, G nb < 2^31.
 *     mode BOX (fractional coordinates, right under a fluctuating box):  s = inv(box_f) p (the inverse of from_matrix,
 *       M v as ((M_r0 v0) + M_r1 v1) + M_r2 v2);  u_d = s_d;  on a periodic dimension of pbc  u_d -= floor(u_d);  on the
 *       others an atom with u_d outside [0, 1) is dropped.  binvol_f = |det box_f| / nb.  lo and hi are not read.
 *     mode LAB (frames the caller has fitted):  u_d = ((p_d - c_d) - lo_d) * (1 / (hi_d - lo_d)), c = 0 without centring;
 *       atoms with u_d outside [0, 1) are dropped: intervals are half-open, an atom on an interior edge belongs to the
 *       upper bin, one on hi is outside.  binvol = ((w_x / nx) (w_y / ny)) (w_z / nz), w_d = hi_d - lo_d.  Boxes are not read.
 *     b_d = min(floor(u_d nbins[d]), nbins[d] - 1) (the min only guards a product that rounds up to nbins[d]).
 *   centring: centre_idx[0..ncentre) (NULL: atoms 0 .. ncentre-1), centre_weight (one per ATOM, >= 0, NULL: 1) and the mask
 *     grid.centre_dims (bits x, y, z); ncentre == 0 or a mask of 0: none.  Per frame, thread t of 256 adds atoms t, t + 256,
 *     ... in that order and a fixed tree adds the threads (as the centres of molar_hip_rmsd_matrix).  On a masked dimension
 *     that is periodic in BOX mode the centre is the circular mean of the fractional coordinate, theta = 2 pi s,
 *     c = atan2(-sum w sin theta, -sum w cos theta) / (2 pi) + 1/2: right for a slab split across the cell boundary.  On a
 *     masked non-periodic dimension in BOX mode c = sum w s / sum w, and in both  u_d = (s_d - c_d) + 1/2  before wrapping.
 *     In LAB mode c = sum w p / sum w on the masked dimensions and lo, hi are relative to it.
 *   accumulation, in integers alone:  q_k = llrint(w_k 2^S) (round to nearest even),  S = 62 - ceil(log2 n) - e  clamped
 *     to at most 52, e the smallest integer with max |w_k| < 2^e over the selection (all weights zero: S = 52;
 *     weight == NULL: S = 0, q = 1), so that n |q| < 2^62 and no sum can overflow whatever the bins; S is returned through
 *     weight_scale_log2 (host memory, may be NULL).  I_f[g][b] = sum of q_k over the atoms of group g in bin b of frame f.
 *   outputs:  density[G][nb] = (sum over f in frame order of (double)I_f[g][b] * (2^-S / binvol_f)) / F, rounded to Real: the
 *     mean over the frames of sum w per unit volume;  count[G][nb] (uint64): atoms over the whole block;  outside[F]
 *     (uint64): selected atoms of frame f that were dropped, outside the range or with a coordinate that is not finite (a
 *     centre that is not finite drops every atom of its frame; the status stays MOLAR_HIP_OK);  centre[F][3]: the centre
 *     used, fractional in BOX mode, 0 on the dimensions not masked;  binvol[F].
 *   Only integer atomics are used and every floating-point sum has a fixed order: the same call gives the same bits.
 * frames, idx, weight, labels, boxes, centre_idx, centre_weight and every output may each be host or device memory, and
 * every output may be NULL.  Device outputs are written on the context's stream and not waited for (the call itself waits
 * once, for the 64 bytes that decide its status and carry the largest |weight|).
 * Errors: n == 0, labels with ngroups == 0: ERR_SIZES; a stride below 3 natoms (with more than one frame), an index not
 * below natoms, n (or ncentre) > natoms without an index, natoms == 0, a box_stride other than 0 and 9, pbc > 7, a mode
 * other than the two, nbins[d] == 0, hi <= lo (or a range that is not finite) in LAB mode, centre_dims > 7, a selected
 * weight that is not finite, weights so large that raw S < 0, a label not below ngroups, a centre weight that is negative or
 * not finite: ERR_INVALID_ARGUMENT; BOX mode with boxes == NULL: ERR_NO_PBC; a box with a vector of zero length:
 * ERR_ZERO_LENGTH_VECTOR, one without an inverse: ERR_INVERSE_FAILED; centre weights that add up to zero: ERR_ZERO_MASS;
 * 2^31 bins, cells, atoms or frames, or a workspace that cannot be allocated: ERR_TOO_LARGE (the byte count in
 * molar_hip_last_error()).  The errors of the arguments alone are reported before the context is used; weights, labels and
 * indices in device memory are judged on the device before any kernel uses one, and no output is touched after an error.
 * nframes == 0 is a successful no-op.
 * molar_hip_density_plan is a pure host function: the bytes of device workspace such a call allocates (kept by the context,
 * grows only; staging of host-memory arguments not included; never smaller for a larger argument), frame_chunk, the frames
 * whose integer bins are held at once and folded in order, atom_chunk, the selected atoms of one frame a workgroup of the
 * binning kernels takes, and lds_cells, the largest G nb the on-chip binning kernel takes (above it: integer atomics
 * straight into memory; both give the same integers). */
enum { MOLAR_HIP_DENSITY_BOX = 0, MOLAR_HIP_DENSITY_LAB = 1 };
typedef struct {
    uint32_t mode;
    uint32_t nbins[3];
    double lo[3], hi[3];
    uint32_t centre_dims;
} molar_hip_density_grid;
int molar_hip_density_plan(size_t nframes, size_t n, size_t ngroups, const molar_hip_density_grid *grid,
                           size_t *workspace_bytes, uint32_t *frame_chunk, uint32_t *atom_chunk, uint32_t *lds_cells);
int molar_hip_density(molar_hip_ctx *ctx, const float *frames, size_t nframes, size_t frame_stride, size_t natoms,
                      const uint64_t *idx, size_t n, const float *weight, const uint32_t *labels, size_t ngroups,
                      const float *boxes, size_t box_stride, uint8_t pbc, const molar_hip_density_grid *grid,
                      const uint64_t *centre_idx, size_t ncentre, const float *centre_weight, float *density,
                      uint64_t *count, uint64_t *outside, float *centre, float *binvol, int32_t *weight_scale_log2);
int molar_hip_density_f64(molar_hip_ctx *ctx, const double *frames, size_t nframes, size_t frame_stride, size_t natoms,
                          const uint64_t *idx, size_t n, const double *weight, const uint32_t *labels, size_t ngroups,
                          const double *boxes, size_t box_stride, uint8_t pbc, const molar_hip_density_grid *grid,
                          const uint64_t *centre_idx, size_t ncentre, const double *centre_weight, double *density,
                          uint64_t *count, uint64_t *outside, double *centre, double *binvol,
                          int32_t *weight_scale_log2);

/* ---- Internal coordinates of a block of trajectory frames: the distance, the angle or the dihedral of every tuple of
 * atoms in every frame (gmx distance, gmx angle, gmx angle -type dihedral / gmx chi / gmx rama), as a series, as histograms
 * per group of tuples, as joint histograms of pairs of tuples (the Ramachandran / Janin map) and as a mean and a spread per
 * tuple.  The frame block, boxes, box_stride and pbc are those of molar_hip_msd.  Operation by operation (Real = float, or
 * double for _f64; everything is formed in double from the exact inputs and rounded to Real at the end; F = nframes,
 * T = ntuples, one kind per call, spec.kind = atoms per tuple):
 *   tuples[T][kind]: atom indices into a frame.  Every bond vector B - A is formed on its own and, when pbc != 0, reduced
 *     with shortest_vector (the f64 PeriodicBox of that frame's box, the masked dimensions): a molecule split across the
 *     cell boundary needs no unwrap.  dot(a, b) = ((ax bx) + ay by) + az bz, the cross product without fused operations.
 *   DISTANCE (A,B):      |B - A|.
 *   ANGLE (A,B,C):       u = A - B, v = C - B;  theta = atan2(|u x v|, u . v) in [0, pi].
 *   DIHEDRAL (A,B,C,D):  b1 = B - A, b2 = C - B, b3 = D - C, n1 = b1 x b2, n2 = b2 x b3;
 *                        phi = atan2(|b2| (b1 . n2), n1 . n2) in (-pi, pi], radians: IUPAC, cis = 0, trans = pi, the sign of
 *                        (b1 x b2) . b3.
 *   invalid values: a coordinate of the tuple that is not finite, |u|^2 = 0 or |v|^2 = 0 (ANGLE), n1 = 0 or n2 = 0 in every
 *     component (DIHEDRAL), or a value that is not finite (a box that is not).  An invalid value is NaN in `values` and
 *     enters nothing else; the status stays MOLAR_HIP_OK.  (A DISTANCE of 0 is valid.)
 *   values[F][T], row stride ld >= T: the series.
 *   hist[G][nbins] (uint64): counts over all frames per group labels[t] < ngroups; labels == NULL: one group, G = 1
 *     (ngroups is not read).  The bin of a value v:
 *       DISTANCE  floor((v - lo) / (hi - lo) * nbins) for lo <= v < hi only (others are not counted),
 *       ANGLE     floor(v / pi * nbins), v = pi in the last bin,
 *       DIHEDRAL  floor((v + pi) / (2 pi) * nbins) mod nbins,
 *     each capped at nbins - 1 (the cap only guards a product that rounds up to nbins).
 *   map[G2][map_bins][map_bins] (uint64): the joint histogram of (value of tuple pairs[p][0], value of tuple pairs[p][1])
 *     within a frame by the same rule with map_bins bins, the first value the slower index; a frame is counted only when
 *     both values are valid (and, for DISTANCE, in range); per group pair_labels[p] < npair_groups (NULL: one group).  The
 *     two values are recomputed: the map does not need the series.
 *   mean[T], spread[T] over the n valid frames of a tuple, added in frame order within chunks of frame_chunk frames and
 *     the chunks added in chunk order:  DISTANCE, ANGLE: S1 = sum v, S2 = sum v v, mean = S1 / n,
 *     spread = sqrt(max(0, S2 / n - mean mean));  DIHEDRAL: C = sum cos phi, S = sum sin phi, mean = atan2(S, C),
 *     spread = 1 - hypot(C, S) / n, the circular variance.  n = 0: both NaN.  valid[T] (uint64) = n.
 *   Only integer atomics are used and every floating-point sum has a fixed order: the same call gives the same bits.
 * frames, tuples, labels, boxes, pairs, pair_labels and every output may each be host or device memory, and every output
 * may be NULL (pairs and pair_labels are read only for a map).  Device outputs are written on the context's stream and not
 * waited for (the call waits once, for the 64 bytes of its status, when a box or an index in device memory is to be judged).
 * Errors: labels with ngroups == 0, pair_labels with npair_groups == 0: ERR_SIZES; a spec that is NULL, a kind other than
 * the three, reserved != 0, for DISTANCE a range that is not finite or lo >= hi, G nbins >= 2^31, G2 map_bins^2 >= 2^31,
 * hist with nbins == 0, map with map_bins == 0 or without pairs, ld < T, tuples == NULL, natoms == 0, a stride below
 * 3 natoms (with more than one frame), a box_stride other than 0 and 9, pbc > 7, a tuple index not below natoms, a label not
 * below its number of groups, a pair entry not below T: ERR_INVALID_ARGUMENT; pbc != 0 with boxes == NULL: ERR_NO_PBC; a
 * box with a vector of zero length: ERR_ZERO_LENGTH_VECTOR, one without an inverse: ERR_INVERSE_FAILED; 2^31 tuples, pairs,
 * frames or workgroups, or memory that cannot be allocated: ERR_TOO_LARGE.  The errors of the arguments alone are reported
 * before the context is used; tuples, pairs and labels in device memory are judged on the device before any kernel uses
 * one as an address, and no output is touched after an error.  nframes == 0 or ntuples == 0 is a successful no-op.
 * molar_hip_intcoord_plan is a pure host function: the bytes of device workspace such a call allocates (the chunk partials
 * [frame chunks][T] when want_stats, i.e. when mean, spread or valid is asked for; kept by the context, grows only; staging
 * of host-memory arguments and results and the per-frame box records not included; never smaller for a larger argument),
 * frame_chunk and tuple_chunk, the frames and the tuples (or pairs) a workgroup takes, and lds_cells, the largest G nbins
 * (G2 map_bins^2) the on-chip histogram takes (above it: integer atomics straight into memory; both give the same
 * integers; the environment variable MOLAR_HIP_INTCOORD_GLOBAL forces the latter). */
enum { MOLAR_HIP_IC_DISTANCE = 2, MOLAR_HIP_IC_ANGLE = 3, MOLAR_HIP_IC_DIHEDRAL = 4 };
typedef struct {
    uint32_t kind;
    uint32_t nbins;
    uint32_t map_bins;
    uint32_t reserved;
    double lo, hi;
} molar_hip_intcoord_spec;
int molar_hip_intcoord_plan(size_t nframes, size_t ntuples, size_t ngroups, size_t npairs, size_t npair_groups,
                            const molar_hip_intcoord_spec *spec, int want_stats, size_t *workspace_bytes,
                            uint32_t *frame_chunk, uint32_t *tuple_chunk, uint32_t *lds_cells);
int molar_hip_intcoord(molar_hip_ctx *ctx, const float *frames, size_t nframes, size_t frame_stride, size_t natoms,
                       const uint64_t *tuples, size_t ntuples, const uint32_t *labels, size_t ngroups,
                       const float *boxes, size_t box_stride, uint8_t pbc, const molar_hip_intcoord_spec *spec,
                       const uint64_t *pairs, size_t npairs, const uint32_t *pair_labels, size_t npair_groups,
                       float *values, size_t ld, uint64_t *hist, uint64_t *map, float *mean, float *spread,
                       uint64_t *valid);
int molar_hip_intcoord_f64(molar_hip_ctx *ctx, const double *frames, size_t nframes, size_t frame_stride, size_t natoms,
                           const uint64_t *tuples, size_t ntuples, const uint32_t *labels, size_t ngroups,
                           const double *boxes, size_t box_stride, uint8_t pbc, const molar_hip_intcoord_spec *spec,
                           const uint64_t *pairs, size_t npairs, const uint32_t *pair_labels, size_t npair_groups,
                           double *values, size_t ld, uint64_t *hist, uint64_t *map, double *mean, double *spread,
                           uint64_t *valid);

/* ---- Time correlation functions of vectors over a block of trajectory frames: the reorientation of bond vectors, dipoles
 * and plane normals (gmx rotacf -P 1 / -P 2), N-H order parameters, the velocity autocorrelation (gmx velacc), the
 * autocorrelation of a dihedral as the vector (cos phi, sin phi, 0) - over all time origins, per vector and per group of
 * vectors.  The frame block, boxes, box_stride and pbc are those of molar_hip_msd; max_lag and origin_stride work as there.
 * Operation by operation (Real = float, or double for _f64; everything is formed in double from the exact inputs and
 * rounded to Real at the end; F = nframes, V = nvectors, L = max_lag, os = origin_stride, one kind per call):
 *   tuples[V][kind]: atom indices into a frame.  The vector w of tuple v in frame f:
 *     kind 1 (A):      w = p[A]: the block holds any per-atom 3-vectors (velocities, dipoles, (cos phi, sin phi, 0));
 *                      boxes and pbc are not read.
 *     kind 2 (A,B):    w = sv(p[B] - p[A]), sv = shortest_vector of that frame's f64 PeriodicBox on the dimensions of pbc
 *                      when pbc != 0 (else the difference as it is): a molecule cut by the cell boundary needs no unwrap.
 *     kind 3 (A,B,C):  w = sv(p[B] - p[A]) x sv(p[C] - p[A]), the plane normal; the cross product without fused operations.
 *     The components outside spec.dims (bits x, y, z) are then set to 0.
 *     mode UNIT: u = w / sqrt((wx wx + wy wy) + wz wz), every component divided;  mode RAW: u = w.
 *   bad frames: a frame is bad for v when a component of w (after the mask) is not finite, or, in UNIT mode, when
 *     (wx wx + wy wy) + wz wz is exactly 0.  A vector with at least one bad frame is left out of every sum: its rows of
 *     c1_vec and c2_vec, its mean and its s2 are NaN; bad_frames[v] (uint32) = its bad frames; the status stays
 *     MOLAR_HIP_OK.  So the number of terms of a lag is n(tau) = (F - 1 - tau) / os + 1 (integer division) for every valid
 *     vector, and the results of the other vectors are bit for bit what they would be without it.
 *   per pair of frames d = fma(uz(t), uz(t + tau), fma(uy(t), uy(t + tau), ux(t) ux(t + tau)));
 *     S1_v[tau] = sum_t d,  S2_v[tau] = sum_t fma(d, d, .),  t = 0, os, 2 os, ... while t + tau <= F - 1, in that order.
 *   c1_vec[V][ld], c2_vec[V][ld], ld >= L + 1 (the rest of a row is not touched):
 *     c1_vec = S1_v / n(tau),  c2_vec = 1.5 (S2_v / n(tau)) - 0.5.
 *   c1[G][L + 1], c2[G][L + 1]: per group labels[v] < ngroups (labels == NULL: one group, G = 1, ngroups is not read) the
 *     S_v of the group's valid vectors added in index order within chunks of vec_chunk vectors (a run of one label within
 *     a chunk is added up first), the chunks in chunk order;  c1 = S1 / (N_g n(tau)),  c2 = 1.5 (S2 / (N_g n(tau))) - 0.5;
 *     N_g = nvalid[g] (uint64), the valid vectors of the group; N_g = 0: a NaN row.
 *   c2 is the Legendre polynomial P2 of the cosine between u(t) and u(t + tau) WHATEVER dims is: with a mask the masked
 *     (projected) vector is normalised and P2(x) = (3 x^2 - 1) / 2 is applied to its cosine, not a two-dimensional analogue.
 *   mean[V][3] = sum_f u(f) / F;  s2[V] = 1.5 q - 0.5,  q = ((xx^2 + yy^2) + zz^2) + 2 ((xy^2 + xz^2) + yz^2) of the second
 *     moments ab = sum_f u_a(f) u_b(f) / F: the long-time limit of c2, the generalised order parameter S^2 of Lipari and
 *     Szabo.  The sums run in frame order within chunks of frame_chunk frames, the chunks in chunk order.
 *   c2, c2_vec and s2 are defined in UNIT mode only.
 *   No floating-point atomics are used and every sum has an order fixed by the sizes alone: the same call gives the same
 *   bits.
 * frames, tuples, labels, boxes and every output may each be host or device memory, and every output may be NULL; the lag
 * stage does not run when none of c1, c2, c1_vec, c2_vec is asked for, and d^2 is not formed when neither c2 nor c2_vec is.
 * Device outputs are written on the context's stream and not waited for; the call waits once, for the 64 bytes of its
 * status (and once more for results that go to host memory).
 * Errors: nvectors == 0, labels with ngroups == 0, ld < max_lag + 1 with c1_vec or c2_vec: ERR_SIZES; a spec that is NULL, a
 * kind other than 1, 2, 3, a mode other than the two, dims == 0 or > 7, reserved != 0, pbc > 7, a box_stride other than 0
 * and 9, max_lag >= nframes (with nframes >= 1), origin_stride == 0, c2, c2_vec or s2 in RAW mode, tuples == NULL,
 * natoms == 0, a stride below 3 natoms (with more than one frame), a tuple index not below natoms, a label not below
 * ngroups: ERR_INVALID_ARGUMENT; pbc != 0 with boxes == NULL for kinds 2 and 3: ERR_NO_PBC; a box with a vector of zero
 * length: ERR_ZERO_LENGTH_VECTOR, one without an inverse: ERR_INVERSE_FAILED; 2^31 vectors, groups, frames or workgroups, or
 * a workspace that cannot be allocated (its bytes are in molar_hip_last_error()): ERR_TOO_LARGE.  The errors of the
 * arguments alone are reported before the context is used; tuples and labels in device memory are judged on the device
 * before any kernel uses one as an address (the vector stage reads atom 0 for a bad index and writes the workspace only),
 * and no output is touched after an error.  nframes == 0 is a successful no-op.
 * molar_hip_tcf_plan is a pure host function: the bytes of device workspace such a call allocates (the status, the boxes,
 * 76 bytes per vector and chunk of frame_chunk frames; with want_lags - any of c1, c2, c1_vec, c2_vec - the f64 vectors
 * U[V][F][3]; with want_groups - c1 or c2 - 16 bytes per chunk of vectors, group and lag; kept by the context, grows only;
 * staging of host-memory arguments and results not included; never smaller for a larger argument), and the launch shape:
 * frame_chunk, the frames a lane of the vector stage walks; vec_chunk, the vectors a workgroup of the lag stage adds up;
 * lag_block = 64 lags_per_lane, the lags of a workgroup; lags_per_lane (R: a lane owns R consecutive lags and takes R
 * origins at a time when origin_stride == 1; the lags behind the last whole block go to one block of the narrowest lane
 * of 1, 2 or 4 lags that holds them; the environment variable MOLAR_HIP_TCF_R = 1, 2 or 4 overrides R for A/B runs);
 * segment, the origins staged at a time, and window = segment + lag_block, the frames they reach. */
enum { MOLAR_HIP_TCF_UNIT = 0, MOLAR_HIP_TCF_RAW = 1 };
typedef struct {
    uint32_t kind;
    uint32_t mode;
    uint32_t dims;
    uint32_t reserved;
} molar_hip_tcf_spec;
int molar_hip_tcf_plan(size_t nframes, size_t nvectors, size_t ngroups, size_t max_lag, int per_frame_boxes, int want_lags,
                       int want_groups, size_t *workspace_bytes, uint32_t *frame_chunk, uint32_t *vec_chunk,
                       uint32_t *lag_block, uint32_t *lags_per_lane, uint32_t *segment, uint32_t *window);
int molar_hip_tcf(molar_hip_ctx *ctx, const float *frames, size_t nframes, size_t frame_stride, size_t natoms,
                  const uint64_t *tuples, size_t nvectors, const uint32_t *labels, size_t ngroups, const float *boxes,
                  size_t box_stride, uint8_t pbc, const molar_hip_tcf_spec *spec, size_t max_lag, size_t origin_stride,
                  float *c1, float *c2, float *c1_vec, float *c2_vec, size_t ld, uint64_t *nvalid, float *mean, float *s2,
                  uint32_t *bad_frames);
int molar_hip_tcf_f64(molar_hip_ctx *ctx, const double *frames, size_t nframes, size_t frame_stride, size_t natoms,
                      const uint64_t *tuples, size_t nvectors, const uint32_t *labels, size_t ngroups, const double *boxes,
                      size_t box_stride, uint8_t pbc, const molar_hip_tcf_spec *spec, size_t max_lag, size_t origin_stride,
                      double *c1, double *c2, double *c1_vec, double *c2_vec, size_t ld, uint64_t *nvalid, double *mean,
                      double *s2, uint32_t *bad_frames);

/* ---- Static structure factors over a block of trajectory frames, by the direct sum over the reciprocal lattice of each
 * frame's own box: the structure factor of a liquid (gmx saxs, gmx scattering), the partial structure factors S_ab(q) that
 * X-ray and neutron intensities are assembled from, the lateral S(q_xy) of the head groups of a bilayer, and the per-frame
 * collective density rho(q, t) an intermediate scattering function starts from.  The frame block, idx, boxes and
 * box_stride (0: one box, 9: one per frame) are those of molar_hip_density; there is no pbc argument: the lattice is
 * whatever 3 x 3 matrix the caller passes - normally the frame's box, or a fixed "virtual" box for a fixed q grid under
 * NPT or for a system that is not periodic.  Operation by operation (Real = float, or double for _f64; everything is
 * formed in double from the exact inputs and rounded to Real at the end; F = nframes, G = the groups, P = G (G + 1) / 2):
 *   selection, weights, groups: as in molar_hip_density.  idx[0 .. n), or atoms 0 .. n-1; weight: one per ATOM, of any sign
 *     (scattering lengths of hydrogen are negative), NULL: 1; labels[n]: one per SELECTED atom, below ngroups, the species,
 *     NULL: one group (ngroups is not read); groups may be empty.
 *   fractional coordinate: s = inv(box_f) p with the inverse and the association of the density call's BOX mode,
 *     s_d = ((inv_d0 x) + inv_d1 y) + inv_d2 z; then s_d -= floor(s_d), which is exact and only keeps the phase small:
 *     periodicity of the system is not assumed.
 *   lattice: Miller indices m = (h, k, l), h in [0, H], k in [-K, K], l in [-L, L], (H, K, L) = grid.hmax;
 *     Q = (H + 1)(2K + 1)(2L + 1); the index of m is (h (2K + 1) + (k + K)) (2L + 1) + (l + L).  Only h >= 0 is stored: real
 *     weights give rho(-m) = conj rho(m); the plane h = 0 holds both halves.  q_f(m) = 2 pi inv(box_f)^T m.  A lateral
 *     analysis is L = 0, the Fourier series of a profile K = L = 0.
 *   collective density: rho_g(m; f) = sum over the atoms j of group g of w_j exp(-2 pi i m.s_j(f)), formed as
 *     sum_j (Ex_j^h Ey_j^k) (w_j Ez_j^l), E_d = (cos, -sin)(2 pi s_d), on the f64 matrix cores.  A power E^p, p >= 0: the
 *     powers a block of the lattice needs are taken in runs of 8 consecutive p; the first of a run is
 *     (cos, -sin)(2 pi t), t = p s_d - floor(p s_d), by sincospi(2 t), every next one the product of the one before with
 *     E^1 (re = ar br - ai bi, im = ar bi + ai br): at most 7 products behind a sincospi.  A negative power is the conjugate.
 *     Ex^h Ey^k is one such complex product, w Ez^l two real ones.  The sum over the atoms: the atoms of a group in the order
 *     of the selection, padded to a multiple of 4 with terms of weight 0, in K splits of atom_chunk atoms; within a split the
 *     MFMA chain (four atoms per step; per step re += Ar Br, re += (-Ai) Bi, im += Ar Bi, im += Ai Br), then the splits in
 *     order.
 *   rho[F][G][Q][2]: the series (re, im); row (f, g) starts at (f G + g) rho_stride, rho_stride >= 2 Q (the rest of a row is
 *     not touched).
 *   frame_ok[F] (uint32): 0 where a selected coordinate of the frame is not finite.  Such a frame's rows of rho are NaN
 *     and it enters no average; the status stays MOLAR_HIP_OK.  Fv = the ok frames; Fv = 0: every average is NaN.
 *   rho_mean[G][Q][2] = sum_f rho / Fv over the ok frames in frame order: the coherent part, so that the caller can form
 *     <|rho|^2> - |<rho>|^2.
 *   sab[P][Q] = sum_f Re(rho_a conj rho_b) / Fv, Re(x conj y) = xr yr + xi yi of the double rho, the ok frames in frame
 *     order; the pairs a <= b are ordered a-major.  It is not normalised: divide by N or by sum w^2 (sfactor_normalize in
 *     the Python package).
 *   shell[P][nshells], shell_count[nshells] (uint64): the spherical (for L = 0 circular) average.  For every ok frame,
 *     every m of the canonical half-space - h > 0, or h = 0 and k > 0, or h = k = 0 and l > 0, never m = 0 - with
 *     v_r = (inv_0r h + inv_1r k) + inv_2r l (column r of that frame's inverse), |q| = 2 pi sqrt((v0 v0 + v1 v1) + v2 v2)
 *     and bin = floor((|q| - qmin) / dq), kept when in [0, nshells): |q| comes from that frame's box, so a box that
 *     fluctuates is handled.  shell[p][b] = (the sum of Re(rho_a conj rho_b) over the members) / shell_count[b], NaN where
 *     the count is 0; shell_count: the members over the whole block.  box_stride == 9: the members of a frame are added
 *     in index order, then the frames in order.  box_stride == 0: the membership is the same in every frame, and the sums
 *     over the frames of S_ab are binned once, the members in index order.  nshells == 0: no shells.
 *   No floating-point atomics are used and every sum has an order fixed by the sizes and the plan: the same call gives the
 *   same bits.  The bits may depend on atom_chunk (where a K split ends) and on box_stride (the two orders of the shells),
 *   on nothing else of the plan: not on frame_block, not on the device's occupancy.
 * frames, idx, weight, labels, boxes and every output may each be host or device memory, and every output may be NULL.
 * Device outputs are written on the context's stream and not waited for; the call waits once, for the 64 bytes of its
 * status (and once more for results that go to host memory).
 * Errors: n == 0, labels with ngroups == 0: ERR_SIZES; a grid that is NULL, reserved != 0, dq <= 0 or dq or qmin not finite
 * with nshells > 0, a box_stride other than 0 and 9, natoms == 0, n > natoms without an index, a stride below 3 natoms
 * (with more than one frame), rho_stride < 2 Q with rho, an index not below natoms, a selected weight that is not finite, a
 * label not below ngroups: ERR_INVALID_ARGUMENT; boxes == NULL: ERR_NO_PBC; a box with a vector of zero length:
 * ERR_ZERO_LENGTH_VECTOR, one without an inverse: ERR_INVERSE_FAILED; hmax[d] >= 2^10, G Q >= 2^31, P Q >= 2^40, 2^31 atoms or
 * frames, more than 65535 K splits and groups together, or a workspace that cannot be allocated (its bytes are in
 * molar_hip_last_error()): ERR_TOO_LARGE.  The errors of the arguments alone are reported before the context is used;
 * indices, labels and weights in device memory are judged on the device before one is used as an address, and no output is
 * touched after an error.  nframes == 0 is a successful no-op.
 * molar_hip_sfactor_plan is a pure host function: the bytes of device workspace such a call allocates (the boxes, the
 * partition, the running sums and staged results, and per frame of a block the blocks of the K splits, rho in double and
 * its staging, the bins and the shells' partial sums; kept by the context, grows only; staging of host-memory inputs and
 * the scratch of the sort not included; never smaller for a larger argument), and the launch shape: layout (0: rows
 * enumerate (h, k) and columns l; 1, taken for L = 0 with K > 0: rows enumerate k and columns h; with K = L = 0 layout 0
 * has one live column in its column tile - a limit), row_block x col_block: the block of rows and columns of a workgroup
 * (2 x 2 waves of 64 x 32), atom_chunk: the atoms of a K split (a multiple of 16), ksplits = ceil(n / atom_chunk),
 * frame_block: the frames whose rho is held at once.  The environment variables MOLAR_HIP_SFACTOR_ATOM_CHUNK and
 * MOLAR_HIP_SFACTOR_FRAME_BLOCK override the two, for the plan and the call alike (A/B runs and tests). */
typedef struct {
    uint32_t hmax[3];
    double qmin, dq;
    uint32_t nshells;
    uint32_t reserved;
} molar_hip_sfactor_grid;
int molar_hip_sfactor_plan(size_t nframes, size_t n, size_t ngroups, const molar_hip_sfactor_grid *grid,
                           size_t *workspace_bytes, uint32_t *layout, uint32_t *row_block, uint32_t *col_block,
                           uint32_t *atom_chunk, uint32_t *ksplits, uint32_t *frame_block);
int molar_hip_sfactor(molar_hip_ctx *ctx, const float *frames, size_t nframes, size_t frame_stride, size_t natoms,
                      const uint64_t *idx, size_t n, const float *weight, const uint32_t *labels, size_t ngroups,
                      const float *boxes, size_t box_stride, const molar_hip_sfactor_grid *grid, float *rho,
                      size_t rho_stride, uint32_t *frame_ok, float *rho_mean, float *sab, float *shell,
                      uint64_t *shell_count);
int molar_hip_sfactor_f64(molar_hip_ctx *ctx, const double *frames, size_t nframes, size_t frame_stride, size_t natoms,
                          const uint64_t *idx, size_t n, const double *weight, const uint32_t *labels, size_t ngroups,
                          const double *boxes, size_t box_stride, const molar_hip_sfactor_grid *grid, double *rho,
                          size_t rho_stride, uint32_t *frame_ok, double *rho_mean, double *sab, double *shell,
                          uint64_t *shell_count);

/* ---- Minimum distances between two selections (or inside one) over a block of trajectory frames: how close two
 * selections come in every frame and which pair it is (gmx mindist, gmx pairdist), how far every atom is from the other
 * selection (every water from the protein, every lipid from a peptide), and the matrix of smallest distances between
 * groups - residues, lipids, molecules - with its mean, minimum and contact frequency over the frames (gmx mdmat).  There
 * is no cutoff in the search: every pair is evaluated, O(n1 n2) per frame.  The frame block, the boxes and box_stride (0:
 * one box, 9: one per frame) are those of molar_hip_intcoord.  Operation by operation (Real = float, or double for _f64;
 * everything is formed in double from the exact inputs and rounded to Real at the end; F = nframes):
 *   sets: set 1 is idx1[0 .. n1), or atoms 0 .. n1-1; set 2 is idx2[0 .. n2), or atoms 0 .. n2-1.  i and j below are POSITIONS
 *     within the sets.  labels1[n1] below ngroups1 and labels2[n2] below ngroups2 make the groups G1 and G2; NULL: one
 *     group (the ngroups is not read).  Groups may be empty and labels need not be sorted.
 *   spec.same = 1: set 2 is set 1 (idx2, labels2 must be NULL; n2, ngroups2 are not read; atom2 must be NULL, it would be
 *     atom1).  The pair i = j is skipped, and with spec.exclude_same_group = 1 so is every pair inside one group (without
 *     labels that is every pair).
 *   distance of a pair: d2 = norm2(shortest_vector(box_f, x_j - x_i, spec.pbc)) with shortest_vector and box_from_matrix
 *     of PeriodicBox in double - any PbcDims mask, triclinic cells, the correction shifts for a full mask - the metric of
 *     molar_hip_intcoord and molar_hip_msd; boxes == NULL or spec.pbc == 0: the plain difference (the boxes are not read).
 *     The distance is sqrt(d2).  Every minimum is taken over d2; equal d2 give the lowest i, then the lowest j.
 *   dist[F], pair[F][2] (uint64): the smallest distance of the frame and the pair (i, j) that has it - the smallest under
 *     the order (d2, i, j).  No pair at all (one atom with same, everything excluded): +inf and UINT64_MAX.  dist[f] is
 *     bit-equal to what molar_hip_intcoord returns for the distance of that pair.
 *   atom1[F][n1], near1[F][n1] (uint64): for every atom of set 1 its distance to set 2 and the position j of its nearest atom
 *     there (the lowest j among equal distances; +inf and UINT64_MAX without a partner).  Row f of both starts at f ld1,
 *     ld1 >= n1 (the rest of a row is not touched).
 *   atom2[F][n2]: the same seen from set 2; row f starts at f ld2, ld2 >= n2.
 *   mat[F][G1][G2]: the smallest distance between group a of set 1 and group b of set 2 in every frame; +inf for an empty
 *     group, a group of one atom against itself, or an excluded diagonal.  With same the matrix is exactly symmetric.
 *   frame_ok[F] (uint32): 0 where a selected coordinate of either set is not finite, or (with boxes and spec.pbc != 0)
 *     box_from_matrix refuses the frame's box (a vector of zero length, no inverse).  Every per-frame output of such a
 *     frame is NaN (pair, near1: UINT64_MAX), it enters none of the three reductions below, and the status stays
 *     MOLAR_HIP_OK.  nvalid[1] (uint64): the valid frames.
 *   mat_mean[G1][G2] (double in both entries) = the sum over the valid frames, in frame order, of the double distances,
 *     divided by nvalid: +inf where any valid frame gave +inf, NaN without a valid frame.
 *   mat_min[G1][G2]: the minimum over the valid frames (+inf without one).
 *   mat_freq[G1][G2] (uint32): the valid frames whose double distance is below spec.cutoff: the contact frequency map.
 *   spec.frame_block: the frames walked at once (0: chosen from the plan; 256 at the most).  The frames of a block are
 *     folded in frame order, so no result depends on it, and mat of the whole block is never held: the reductions do not
 *     need the mat output.
 *   Every reduction is a minimum under a total order, or a sum in frame order; the only atomics are 64-bit integer minima on
 *   the bits of d2.  The same call gives the same bits, whatever the plan.
 * frames, idx1, idx2, labels1, labels2, boxes and every output may each be host or device memory, and every output may be
 * NULL.  Device outputs are written on the context's stream and not waited for; the call waits once, for the 64 bytes of its
 * status (and once more for results that go to host memory).
 * Errors: n1 == 0 or n2 == 0, labels with ngroups == 0: ERR_SIZES; a spec that is NULL, pbc > 7, same or exclude_same_group
 * other than 0 and 1, exclude_same_group without same, a cutoff that is NaN, same with idx2, labels2 or atom2, a box_stride
 * other than 0 and 9, natoms == 0, n1 or n2 > natoms without an index, a stride below 3 natoms, ld1 < n1 or ld2 < n2 (each
 * with more than one frame), an index not below natoms, a label not below its ngroups: ERR_INVALID_ARGUMENT; 2^31 atoms,
 * frames or cells G1 G2, or a workspace that cannot be allocated: ERR_TOO_LARGE.  The errors of the arguments alone are
 * reported before the context is used; indices and labels in device memory are judged on the device before one is used as an
 * address, and no output is touched after an error.  nframes == 0 is a successful no-op.
 * molar_hip_mindist_plan is a pure host function.  outputs: which results the call would be asked for, the sum of
 * MOLAR_HIP_MINDIST_DIST (dist, pair), _ATOM1 (atom1, near1), _ATOM2 and _MAT (any of the four matrices).  It gives the bytes of
 * device workspace (the boxes, the partition, the running reductions, and per frame of a block both sets in double, the row
 * partials of every column split, the group matrix and staged results; kept by the context, grows only; staging of
 * host-memory inputs and the scratch of the sort not included) and the launch shape: rows_per_wave (a lane owns two atoms of
 * the row set), rows_per_block (four waves), cols_per_tile (a column split is a whole number of tiles), col_splits (the
 * splits of the column set of the first pass, more when rows and frames alone do not fill the device), frame_block.  The
 * passes: rows of set 1 against columns of set 2 for atom1 / near1 (and dist / pair); rows of set 2 for atom2 (dist / pair
 * come from it when atom1 / near1 are not asked for); the group pass for the matrices.  The environment variables
 * MOLAR_HIP_MINDIST_COL_SPLITS and MOLAR_HIP_MINDIST_FRAME_BLOCK override the two, for the plan and the call alike (A/B runs
 * and tests); spec.frame_block goes before the variable. */
#define MOLAR_HIP_MINDIST_DIST 1u
#define MOLAR_HIP_MINDIST_ATOM1 2u
#define MOLAR_HIP_MINDIST_ATOM2 4u
#define MOLAR_HIP_MINDIST_MAT 8u
typedef struct {
    uint32_t pbc;
    uint32_t same;
    uint32_t exclude_same_group;
    uint32_t frame_block;
    double cutoff;
} molar_hip_mindist_spec;
int molar_hip_mindist_plan(size_t nframes, size_t n1, size_t n2, size_t ngroups1, size_t ngroups2,
                           const molar_hip_mindist_spec *spec, uint32_t outputs, size_t *workspace_bytes,
                           uint32_t *rows_per_wave, uint32_t *rows_per_block, uint32_t *cols_per_tile, uint32_t *col_splits,
                           uint32_t *frame_block);
int molar_hip_mindist(molar_hip_ctx *ctx, const float *frames, size_t nframes, size_t frame_stride, size_t natoms,
                      const uint64_t *idx1, size_t n1, const uint32_t *labels1, size_t ngroups1, const uint64_t *idx2,
                      size_t n2, const uint32_t *labels2, size_t ngroups2, const float *boxes, size_t box_stride,
                      const molar_hip_mindist_spec *spec, float *dist, uint64_t *pair, float *atom1, uint64_t *near1,
                      size_t ld1, float *atom2, size_t ld2, float *mat, double *mat_mean, float *mat_min,
                      uint32_t *mat_freq, uint32_t *frame_ok, uint64_t *nvalid);
int molar_hip_mindist_f64(molar_hip_ctx *ctx, const double *frames, size_t nframes, size_t frame_stride, size_t natoms,
                          const uint64_t *idx1, size_t n1, const uint32_t *labels1, size_t ngroups1,
                          const uint64_t *idx2, size_t n2, const uint32_t *labels2, size_t ngroups2, const double *boxes,
                          size_t box_stride, const molar_hip_mindist_spec *spec, double *dist, uint64_t *pair,
                          double *atom1, uint64_t *near1, size_t ld1, double *atom2, size_t ld2, double *mat,
                          double *mat_mean, double *mat_min, uint32_t *mat_freq, uint32_t *frame_ok, uint64_t *nvalid);

/* ---- The self part of the van Hove function G_s(r, tau) over a block of trajectory frames: the distribution of the
 * displacements of every particle over a list of lags and all time origins, per group of particles (gmx vanhove) - what
 * MSD(tau) and its fourth moment (molar_hip_msd) summarise in two numbers: hopping, cage escape, exponential tails.  traj is an
 * ALREADY UNWRAPPED particle trajectory: frame f is at traj + f * frame_stride (elements, >= 3 natoms), particle a at 3 a of
 * its frame - the disp [F][P][3] of molar_hip_msd (natoms = P), which does the no-jump unwrap, the centres of mass and the
 * drift removal, or the raw coordinates of a system that is not periodic.  The call takes no box and removes no image.
 * Operation by operation (Real = float, or double for _f64; everything is formed in double from the exact inputs; F = nframes):
 *   selection idx[0..n), shared by all frames; idx == NULL: particles 0 .. n-1.  k below is a POSITION within the selection.
 *   lags[0..L) (uint64): strictly increasing, each below F; lag 0 is allowed.  A list, not a range.
 *   origins: t = 0, origin_stride, 2 origin_stride, ... while t + tau <= F - 1;
 *     norigins[l] = (F - 1 - lags[l]) / origin_stride + 1.
 *   dims: the bits x, y, z (1 .. 7) of the components that enter, nd of them.
 *   labels[0..n) (uint32), each below ngroups = G; NULL: one group (ngroups is not read).  Groups may be empty and labels need
 *     not be sorted.
 *   per particle k, lag l and origin t:  Delta_d = x_k,d(t + tau_l) - x_k,d(t) in double for the components of dims;
 *     v = sqrt(r2), r2 = 0, then r2 = fma(Delta_d, Delta_d, r2) for d = x, y, z in that order (as molar_hip_msd forms r^2),
 *     sqrt correctly rounded;  flags & MOLAR_HIP_VANHOVE_SIGNED (one component only): v = Delta_d.
 *     lo <= v < hi: the pair enters bin floor((v - lo) / (hi - lo) * nbins) of hist[g][l], a bin above nbins - 1 (a product
 *     that rounds up) taken as nbins - 1 - the DISTANCE formula of molar_hip_intcoord; otherwise it is counted in
 *     outside[g][l].
 *   a particle with a coordinate of dims that is not finite in any frame of the block is left out of every count: bad[k] is
 *     the number of such frames of particle k, nvalid[g] the particles of group g with bad[k] == 0.  The counts of the other
 *     particles are as without it.
 *   For every (g, l):  sum_b hist[g][l][b] + outside[g][l] = nvalid[g] * norigins[l].
 * Outputs (each may be NULL, host or device memory): hist [G][L][nbins], outside [G][L], norigins [L], nvalid [G] (uint64),
 * bad [n] (uint32).  Only integer atomics: the same call gives the same bits.  traj, idx, labels and lags may each be host or
 * device memory.  Device outputs are written on the context's stream and not waited for; the call waits once, for the 64
 * bytes of its status (and once more for results that go to host memory).
 * Errors: n == 0, nlags == 0, labels with ngroups == 0: ERR_SIZES; a lag not below F, lags that are not
 * strictly increasing, origin_stride == 0, dims == 0 or > 7, an unknown bit of flags, SIGNED with more than one bit of dims,
 * lo >= hi, a lo or hi that is not finite, nbins == 0, a label not below G, an index not below natoms, natoms == 0,
 * n > natoms without an index, a stride below 3 natoms (with more than one frame), a null lags or (with frames) traj:
 * ERR_INVALID_ARGUMENT; 2^31 particles, frames or cells G L nbins, or a workspace that cannot be allocated: ERR_TOO_LARGE.  The
 * errors of the arguments alone are reported before the context is used; labels, lags and indices in device memory are judged on the device
 * before one is used as an address, and no output is touched after an error.  nframes == 0 is a successful no-op.
 * molar_hip_vanhove_plan is a pure host function (ndims = 1, 2 or 3: the bits set in dims).  It gives the bytes of device
 * workspace (the partition by label, bad, nvalid and the particle-major f64 trajectories [n][ndims][F]; kept by the context,
 * grows only; staging of host-memory arguments and the scratch of the sort not included; never smaller for a larger argument)
 * and every launch-shape size the kernels branch on: particles_per_wg, the sorted particles a workgroup walks;
 * origins_per_pass, the frames of origins a workgroup holds in registers at a time; lag_tile, the lags of one workgroup;
 * on_chip, whether the counts go to an on-chip histogram (nbins <= lds_cells; lag_tile * nbins <= lds_cells then) or straight
 * to memory; lds_cells, that limit; pass_splits, the workgroups that share the passes of one (particle chunk, lag tile);
 * pairs_per_flush, the largest number of pairs one 32-bit on-chip cell can receive between two flushes - particles_per_wg
 * times the origins a workgroup walks, below 2^32 for every call the entry accepts.  The environment variable
 * MOLAR_HIP_VANHOVE_ONCHIP = 0 sends the counts to memory whatever nbins is, for the plan and the call alike, and
 * MOLAR_HIP_VANHOVE_COMBINE = 1 switches on the combining of equal cells of a wave (A/B runs and tests; no count changes). */
#define MOLAR_HIP_VANHOVE_SIGNED 1u
int molar_hip_vanhove_plan(size_t nframes, size_t n, size_t ngroups, size_t nlags, size_t nbins, uint32_t ndims,
                           size_t *workspace_bytes, uint32_t *particles_per_wg, uint32_t *origins_per_pass,
                           uint32_t *lag_tile, uint32_t *on_chip, uint32_t *lds_cells, uint32_t *pass_splits,
                           uint64_t *pairs_per_flush);
int molar_hip_vanhove(molar_hip_ctx *ctx, const float *traj, size_t nframes, size_t frame_stride, size_t natoms,
                      const uint64_t *idx, size_t n, const uint32_t *labels, size_t ngroups, const uint64_t *lags,
                      size_t nlags, size_t origin_stride, uint32_t dims, uint32_t flags, double lo, double hi,
                      size_t nbins, uint64_t *hist, uint64_t *outside, uint64_t *norigins, uint64_t *nvalid,
                      uint32_t *bad);
int molar_hip_vanhove_f64(molar_hip_ctx *ctx, const double *traj, size_t nframes, size_t frame_stride, size_t natoms,
                          const uint64_t *idx, size_t n, const uint32_t *labels, size_t ngroups, const uint64_t *lags,
                          size_t nlags, size_t origin_stride, uint32_t dims, uint32_t flags, double lo, double hi,
                          size_t nbins, uint64_t *hist, uint64_t *outside, uint64_t *norigins, uint64_t *nvalid,
                          uint32_t *bad);

/* the per-frame loop of benches/comparison_small.rs:14-25 in f64, same argument meaning as molar_hip_fit_rmsd_batch:
 * every frame's selection fitted onto the reference selection (masses of the frame's atoms; the reference centre with
 * the same column through ref_idx), RMSD / centre of mass / gyration of the FITTED selection, frames moved if apply.
 * Outputs (each optional): rmsd[F], R[F][9] column-major, t[F][3], com[F][3], gyr[F]. */
int molar_hip_fit_rmsd_batch_f64(molar_hip_ctx *ctx, double *frames, size_t nframes, size_t natoms,
                                 const uint64_t *idx, size_t n, const double *mass, const double *ref_xyz,
                                 size_t ref_natoms, const uint64_t *ref_idx, int apply, double *rmsd_out,
                                 double *R_out, double *t_out, double *com_out, double *gyr_out);
/* the periodic centres (:156-168, :197-220), gyration_pbc (:222-232) and unwrap_simple_dim (modify.rs:40-54) with an f64
 * PeriodicBox built from box9 (column-major, columns a,b,c) exactly as PeriodicBox::from_matrix does: ERR_NO_PBC if
 * box9 == NULL, ERR_ZERO_LENGTH_VECTOR / ERR_INVERSE_FAILED from the construction. */
int molar_hip_center_of_geometry_pbc_f64(molar_hip_ctx *ctx, const double *xyz, size_t natoms, const uint64_t *idx,
                                         size_t n, const double *box9, uint8_t pbc, double out[3]);
int molar_hip_center_of_mass_pbc_f64(molar_hip_ctx *ctx, const double *xyz, size_t natoms, const uint64_t *idx,
                                     size_t n, const double *mass, const double *box9, uint8_t pbc, double out[3]);
int molar_hip_gyration_pbc_f64(molar_hip_ctx *ctx, const double *xyz, size_t natoms, const uint64_t *idx, size_t n,
                               const double *mass, const double *box9, double *out);
int molar_hip_unwrap_simple_f64(molar_hip_ctx *ctx, double *xyz, size_t natoms, const uint64_t *idx, size_t n,
                                const double *box9, uint8_t pbc);
/* rotate (modify.rs:25-30) about the origin, in place; principal_transform :102-109 / _pbc :246-257 (box9 != NULL) */
int molar_hip_rotate_f64(molar_hip_ctx *ctx, double *xyz, size_t natoms, const uint64_t *idx, size_t n,
                         const double unit_axis3[3], double angle);
int molar_hip_principal_transform_f64(molar_hip_ctx *ctx, const double *xyz, size_t natoms, const uint64_t *idx,
                                      size_t n, const double *mass, const double *box9, double R9[9], double t3[3]);
/* Measure::lipid_tail_order (measure.rs:270-422) in f64, CSR layout and error codes of molar_hip_lipid_tail_order */
int molar_hip_lipid_tail_order_f64(molar_hip_ctx *ctx, const double *xyz, size_t natoms, const uint64_t *idx,
                                   const uint64_t *tail_offsets, size_t ntails, int order_type, const double *normals,
                                   const uint64_t *normal_offsets, const uint8_t *bond_orders, double *out);
/* inertia_pbc :234-244 */
int molar_hip_inertia_pbc_f64(molar_hip_ctx *ctx, const double *xyz, size_t natoms, const uint64_t *idx, size_t n,
                              const double *mass, const double *box9, double moments[3], double axes9[9],
                              double tensor9[9]);
/* apply_transform (modify.rs:32-36), in place */
int molar_hip_apply_transform_f64(molar_hip_ctx *ctx, double *xyz, size_t natoms, const uint64_t *idx, size_t n,
                                  const double R9[9], const double t3[3]);

/* Batched selections (CSR): selection k = idx[offsets[k] .. offsets[k+1]).  Replaces the rayon loops over
 * ParSplit sub-selections / per-lipid selections (selection/system.rs:193-213, molar_membrane/src/lib.rs:
 * 135-137, lipid_molecule.rs:65-99) where one GPU launch per ~100-atom selection would be slower than the
 * serial loop.  out: float[K][3].  mass == NULL => center_of_geometry, else center_of_mass (ERR_ZERO_MASS if
 * any selection has zero total mass). */
int molar_hip_center_batch(molar_hip_ctx *ctx, const float *xyz, size_t natoms, const uint64_t *idx,
                           const uint64_t *offsets, size_t nsel, const float *mass, float *out);
/* Modify::unwrap_simple_dim (modify.rs:40-54) applied to every selection of the CSR list, in place. */
int molar_hip_unwrap_simple_batch(molar_hip_ctx *ctx, float *xyz, size_t natoms, const uint64_t *idx,
                                  const uint64_t *offsets, size_t nsel, const float *box9, uint8_t pbc);
/* The two batch entries above in f64 (MolAR's `f64` feature), same arguments with double: centres in the reference's serial
 * order of additions (COM with masses, COG without), and unwrap_simple_dim per selection in place (ERR_NO_PBC if box9 ==
 * NULL).  Pointers may be host or device memory, as for the other _f64 entries. */
int molar_hip_center_batch_f64(molar_hip_ctx *ctx, const double *xyz, size_t natoms, const uint64_t *idx,
                               const uint64_t *offsets, size_t nsel, const double *mass, double *out);
int molar_hip_unwrap_simple_batch_f64(molar_hip_ctx *ctx, double *xyz, size_t natoms, const uint64_t *idx,
                                      const uint64_t *offsets, size_t nsel, const double *box9, uint8_t pbc);
/* Membrane::compute_initial_normals (molar_membrane/src/lib.rs:456-505), host arithmetic: tail->head unit
 * vectors, then two neighbour-averaging passes over the patches (CSR patch_offsets/patch_ids; the second
 * pass updates normals in place, in lipid order, exactly like the reference loop).  valid may be NULL. */
int molar_hip_membrane_initial_normals(size_t nlipids, const float *head_markers, const float *tail_markers,
                                       const uint64_t *patch_offsets, const uint64_t *patch_ids,
                                       const uint8_t *valid, float *normals_out);

/* Membrane::compute_patches' list building (molar_membrane/src/lib.rs:548-557) from the (i, j) pairs of the
 * marker search, in pair order: patch_ids[i].push(j); patch_ids[j].push(i).  Host arrays; patch_offsets[K+1],
 * patch_ids[2*npairs]. */
int molar_hip_membrane_patches_from_pairs(const uint32_t *pairs, size_t npairs, size_t nlipids,
                                          uint64_t *patch_offsets, uint64_t *patch_ids);
/* One iteration of Membrane::smooth (molar_membrane/src/lib.rs:661-812) for all lipids on the GPU: local
 * frame from the lipid's normal (lipid_molecule.rs:190-196), patch markers into that frame through
 * PeriodicBox::shortest_vector, quadric fit (get_quad_coefs :844-863), Voronoi cell of the marker among its patch
 * (molar/src/voronoi_cell.rs:62-211), curvatures + fitted normal (lipid_molecule.rs:102-188), cell area, fitted
 * patch points, then the scatter-average of the markers (:781-809).  Replaces the rayon par_iter over lipids.
 * Host pointers.  Patches are CSR over lipid ids (compute_patches :539-558).  The state arrays are IN/OUT exactly
 * like the fields of LipidMolecule: a lipid that is (or becomes) invalid keeps its previous values; optional
 * outputs may be NULL.  Lipid i owns slots [patch_offsets[i] + 4*i, patch_offsets[i+1] + 4*(i+1)) of neib_ids
 * and voro_vertexes and fills the first nvert[i] of them (a cell has at most patch_len + 4 vertices).
 * Eigenpairs: nalgebra's symmetric_eigen leaves order and sign open; here princ_curvs are descending and each
 * direction has a positive first non-zero local component. */
typedef struct {
    size_t nlipids;
    const uint64_t *patch_offsets;   /* [nlipids+1] */
    const uint64_t *patch_ids;       /* [patch_offsets[nlipids]] */
} molar_hip_membrane_patches;
typedef struct {
    float *head_markers;             /* [K][3]  required */
    float *normals;                  /* [K][3]  required: in = normal defining the local frame, out = fitted normal */
    uint8_t *valid;                  /* [K]     required */
    float *quad_coefs;               /* [K][6]  a,b,c,d,e,f of z = a x^2 + b y^2 + c xy + d x + e y + f */
    float *mean_curv, *gauss_curv;   /* [K] */
    float *princ_curvs;              /* [K][2] */
    float *princ_dirs;               /* [K][2][3] */
    float *area;                     /* [K] */
    uint32_t *nvert;                 /* [K] */
    uint64_t *neib_ids;              /* [E + 4K] slotted, see above */
    float *voro_vertexes;            /* [E + 4K][3] slotted */
    float *fitted_patch_points;      /* [E][3] aligned with patch_ids */
} molar_hip_membrane_state;
int molar_hip_membrane_smooth(molar_hip_ctx *ctx, const molar_hip_membrane_patches *patches, const float *box9,
                              molar_hip_membrane_state *state);

/* patches_from_nth_shell (molar_membrane/src/lib.rs:562-583), host arithmetic: from the Voronoi neighbours a smoothing
 * pass left (nvert / neib_ids of molar_hip_membrane_state, slotted by patch_offsets), the patch of every valid lipid
 * becomes its n-th neighbour shell - the direct neighbours widened (n_shells - 2) times by the neighbours of every
 * member, the lipid itself included from n_shells = 3 on as in the reference; lipids that are not valid keep the patch
 * they have.  The reference collects a HashSet (order unspecified); here ids ascend.  Count-then-fill: with out_ids ==
 * NULL (or too small a capacity) only out_offsets[nlipids + 1] and *needed are written.  nvert[i] of a VALID lipid above
 * its slots (patch length + 4) is an error; a lipid that is not valid may still be walked as a member of a shell (it
 * keeps the neighbours an earlier pass left, as in the reference) and its count is clamped to its slots. */
int molar_hip_membrane_nth_shell_patches(size_t nlipids, const uint8_t *valid, const uint64_t *patch_offsets,
                                         const uint64_t *patch_ids, const uint32_t *nvert, const uint64_t *neib_ids,
                                         size_t n_shells, uint64_t *out_offsets, uint64_t *out_ids, size_t capacity,
                                         size_t *needed);
/* smooth_curvature (lib.rs:584-621), host arithmetic, in place: mean and Gaussian curvature of every valid lipid
 * averaged with those of the valid members of its n-th neighbour shell (sums in ascending id, f32, from the values
 * before the call); n_shells == 0 leaves everything as it is. */
int molar_hip_membrane_smooth_curvature(size_t nlipids, const uint8_t *valid, const uint64_t *patch_offsets,
                                        const uint32_t *nvert, const uint64_t *neib_ids, size_t n_shells,
                                        float *mean_curv, float *gauss_curv);

/* The staged Membrane::compute in f64 (MolAR's `f64` feature, molar_membrane's `f64 = ["molar/f64"]`).  The state is
 * molar_hip_membrane_state with double in place of float; the integer parts of the chain (search_count_f64 / _fill_f64,
 * membrane_patches_from_pairs, membrane_nth_shell_patches) and lipid_tail_order_f64 are shared with the other entries. */
typedef struct {
    double *head_markers;            /* [K][3]  required */
    double *normals;                 /* [K][3]  required: in = normal defining the local frame, out = fitted normal */
    uint8_t *valid;                  /* [K]     required */
    double *quad_coefs;              /* [K][6]  a,b,c,d,e,f of z = a x^2 + b y^2 + c xy + d x + e y + f */
    double *mean_curv, *gauss_curv;  /* [K] */
    double *princ_curvs;             /* [K][2] */
    double *princ_dirs;              /* [K][2][3] */
    double *area;                    /* [K] */
    uint32_t *nvert;                 /* [K] */
    uint64_t *neib_ids;              /* [E + 4K] slotted like molar_hip_membrane_state */
    double *voro_vertexes;           /* [E + 4K][3] slotted */
    double *fitted_patch_points;     /* [E][3] aligned with patch_ids */
} molar_hip_membrane_state_f64;
/* One iteration of Membrane::smooth (lib.rs:661-812) in f64: the contract of molar_hip_membrane_smooth (host pointers,
 * IN/OUT state, invalid lipids keep their values, slot layout, princ_curvs descending with the same sign convention on
 * princ_dirs, error codes), every operation in double in the reference's order. */
int molar_hip_membrane_smooth_f64(molar_hip_ctx *ctx, const molar_hip_membrane_patches *patches, const double *box9,
                                  molar_hip_membrane_state_f64 *state);
/* compute_initial_normals (lib.rs:456-505) and smooth_curvature (:584-621) in f64: host arithmetic, the arguments of
 * molar_hip_membrane_initial_normals / _smooth_curvature with double. */
int molar_hip_membrane_initial_normals_f64(size_t nlipids, const double *head_markers, const double *tail_markers,
                                           const uint64_t *patch_offsets, const uint64_t *patch_ids,
                                           const uint8_t *valid, double *normals_out);
int molar_hip_membrane_smooth_curvature_f64(size_t nlipids, const uint8_t *valid, const uint64_t *patch_offsets,
                                            const uint32_t *nvert, const uint64_t *neib_ids, size_t n_shells,
                                            double *mean_curv, double *gauss_curv);

/* One whole frame of Membrane::compute (molar_membrane/src/lib.rs:410-454) as a chain of kernels with no host round
 * trip inside: unwrap of every lipid (lipid_molecule.rs:75-76) -> head / mid / tail-end markers (:65-99) -> PBC search
 * among the valid lipids' head markers and the patch lists in push order (compute_patches, lib.rs:539-558) ->
 * compute_initial_normals (:456-505, including the second pass that updates normals in place in lipid order) ->
 * max_smooth_iter iterations of smooth (:661-812) -> lipid_tail_order of every tail with its lipid's normal (:435-443).
 * With the neighbour-shell options (molar_hip_membrane_plan_set_shells, lib.rs:562-621) the chain also covers
 * patches_from_nth_shell - a first smoothing pass on the search patches, the patches rebuilt as the n-th Voronoi shell on
 * the device, then max_smooth_iter passes on them - and smooth_curvature after the passes.
 * The stages are the ones behind molar_hip_unwrap_simple_batch, _center_batch, _search_*, _membrane_patches_from_pairs,
 * _membrane_initial_normals, _membrane_smooth and _lipid_tail_order, and give the same bits; what differs is that the
 * pair list, the patches and every per-lipid array stay in device memory between them.
 *
 * A plan holds what is constant over a trajectory (the index lists, masses, options) and the per-lipid `valid` flags,
 * which the reference carries from frame to frame (LipidMolecule::valid: a lipid dropped by smooth stays out of the
 * patches of later frames until reset_valid_lipids, lib.rs:269-273).  Two frames may be in flight:
 *     begin(frame k+1); end(frame k); fetch / use the device view of k; ...
 * so the host work of a frame hides behind the kernels of the one before it.  Frames are chained on the context's
 * stream in begin order, `valid` included.  The result of a frame stays readable until the second _begin after its own.
 * Sizes that vary with the frame (pairs, patch entries, shell-patch entries) are provisioned from earlier frames; a
 * frame that outgrows them is repeated inside _end, transparently.  All pointers of the description are host memory and
 * are copied at creation. */
typedef struct molar_hip_membrane_plan molar_hip_membrane_plan;
typedef struct {
    size_t natoms, nlipids;
    const uint64_t *lipid_idx;        /* CSR of whole lipids: lipid k = lipid_idx[lipid_offsets[k] .. lipid_offsets[k+1]) */
    const uint64_t *lipid_offsets;    /* [nlipids + 1] */
    const uint64_t *marker_idx;       /* CSR of 3 * nlipids selections: head, mid, tail-end of lipid 0, head of lipid 1, ... */
    const uint64_t *marker_offsets;   /* [3 * nlipids + 1] */
    const float *masses;              /* [natoms] */
    size_t ntails;
    const uint64_t *tail_idx;         /* CSR of the tails' carbons in chain order, layout of molar_hip_lipid_tail_order */
    const uint64_t *tail_offsets;     /* [ntails + 1] */
    const uint32_t *tail_lipid;       /* [ntails] the lipid whose normal a tail is measured against */
    const uint8_t *tail_bonds;        /* bond orders, layout of molar_hip_lipid_tail_order */
    float cutoff;                     /* patch search radius (MembraneOptions::cutoff) */
    int32_t order_type;               /* 0 Sz, 1 Scd, 2 ScdCorr */
    int32_t max_smooth_iter;          /* >= 1 */
    int32_t unwrap;                   /* make every lipid whole before the markers are taken */
    int32_t use_global_normal;        /* order against global_normal instead of the lipid's normal */
    float global_normal[3];
} molar_hip_membrane_desc;
/* Device addresses of one frame's results (valid as described above); E = patch entries of the frame. */
typedef struct {
    size_t nlipids, patch_entries, npairs;
    const float *head, *mid, *tail;             /* [K][3] markers before smoothing */
    const uint64_t *patch_offsets, *patch_ids;  /* [K+1], [E] */
    const float *initial_normals;               /* [K][3] */
    const uint8_t *valid;                       /* [K] after the frame */
    const float *smoothed_head, *normals;       /* [K][3] */
    const float *quad_coefs, *mean_curv, *gauss_curv, *princ_curvs, *princ_dirs, *area;
    const uint32_t *nvert;
    const uint64_t *neib_ids;                   /* [E + 4K] slotted like molar_hip_membrane_state */
    const float *voro_vertexes;                 /* [E + 4K][3] */
    const float *fitted_patch_points;           /* [E][3] */
    const float *order;                         /* concatenated per tail, layout of molar_hip_lipid_tail_order */
    size_t norder;
} molar_hip_membrane_view;
/* Host destinations for molar_hip_membrane_frame_fetch: any pointer may be NULL (skipped); the E-sized arrays are
 * written up to the frame's patch_entries (see the view). */
typedef struct {
    float *head, *mid, *tail;
    uint64_t *patch_offsets, *patch_ids;
    float *initial_normals;
    uint8_t *valid;
    float *smoothed_head, *normals;
    float *quad_coefs, *mean_curv, *gauss_curv, *princ_curvs, *princ_dirs, *area;
    uint32_t *nvert;
    uint64_t *neib_ids;
    float *voro_vertexes;
    float *fitted_patch_points;
    float *order;
} molar_hip_membrane_out;
int molar_hip_membrane_plan_create(molar_hip_ctx *ctx, const molar_hip_membrane_desc *desc, molar_hip_membrane_plan **out);
void molar_hip_membrane_plan_destroy(molar_hip_membrane_plan *plan);
/* valid[nlipids] from host memory (NULL: all valid = reset_valid_lipids, lib.rs:269-273).  No frame may be in flight: with
 * a ticket pending the call changes nothing and returns MOLAR_HIP_ERR_INVALID_ARGUMENT - end the frames first (the flags
 * feed the kernels of a frame from its first launch on). */
int molar_hip_membrane_plan_set_valid(molar_hip_membrane_plan *plan, const uint8_t *valid);
/* n_shells_patch / n_shells_smoothing of MembraneOptions (molar_membrane/src/lib.rs:53-85); 0 / 0 (the default) = the chain
 * as before.  With n_shells_patch > 0 a frame smooths once on the search patches, rebuilds every valid lipid's patch as its
 * n-th neighbour shell (the definition of molar_hip_membrane_nth_shell_patches, ids ascending; invalid lipids keep their
 * patch), re-slots the state from zero and smooths max_smooth_iter more times; with n_shells_smoothing > 0 the curvatures are
 * averaged over the n-th shell of the final patches (molar_hip_membrane_smooth_curvature).  Same bits as those staged calls.
 * The view and the fetch then report the FINAL patch lists (patch_entries = entries of the shell patches).  No frame may be in
 * flight (as for _plan_set_valid): with a ticket pending the call changes nothing and returns ERR_INVALID_ARGUMENT. */
int molar_hip_membrane_plan_set_shells(molar_hip_membrane_plan *plan, size_t n_shells_patch, size_t n_shells_smoothing);
/* xyz: float[natoms][3], device memory (unwrapped in place, and read until the frame ends) or host memory (uploaded;
 * the unwrapped frame is written back before _begin returns).  box9: column-major box matrix.  Returns with a ticket
 * (0 or 1) without waiting for the frame. */
int molar_hip_membrane_frame_begin(molar_hip_membrane_plan *plan, float *xyz, const float *box9, int32_t *ticket);
/* Waits for that frame; `view` may be NULL.  Errors of the frame's stages surface here (ERR_ZERO_MASS,
 * ERR_LIPID_TAIL_TOO_SHORT, ...). */
int molar_hip_membrane_frame_end(molar_hip_membrane_plan *plan, int32_t ticket, molar_hip_membrane_view *view);
/* Copies the chosen arrays of an ended frame to host memory. */
int molar_hip_membrane_frame_fetch(molar_hip_membrane_plan *plan, int32_t ticket, const molar_hip_membrane_out *out);
/* _frame_end and the fetch of per-lipid results in one wait: the chosen arrays leave on the frame's stream right behind its last
 * kernel (what LipidGroup::frame_update reads every frame, molar_membrane/src/lipid_group.rs: flags, normals, curvatures, areas,
 * vertex counts, order).  The arrays sized by the frame's patch entries (patch_ids, neib_ids, voro_vertexes,
 * fitted_patch_points) must be NULL here - their length is only known from the view; _frame_fetch brings them afterwards. */
int molar_hip_membrane_frame_end_fetch(molar_hip_membrane_plan *plan, int32_t ticket, molar_hip_membrane_view *view,
                                       const molar_hip_membrane_out *out);

/* Measure::lipid_tail_order (measure.rs:270-422), batched over `ntails` tails given as CSR:
 * tail t holds the carbons idx[tail_offsets[t] .. tail_offsets[t+1]) (n_t atoms), its normals are
 * normals[3*normal_offsets[t] .. 3*normal_offsets[t+1]) (1 or n_t-2 vectors), its n_t-1 bond orders
 * start at bond_orders[tail_offsets[t]-t], its n_t-2 results go to out[tail_offsets[t]-2t ..).
 * order_type: 0 Sz, 1 Scd, 2 ScdCorr (measure.rs:708-716).  Size violations of any tail return
 * ERR_LIPID_TAIL_TOO_SHORT / _NORMALS_COUNT / _BOND_ORDER_COUNT (measure.rs:281-291); bond order
 * counts are implied by the layout, so the third can only come from a NULL bond_orders.
 * Replaces the per-lipid rayon loop of molar_membrane (lib.rs:435-443, lipid_molecule.rs:48-59). */
int molar_hip_lipid_tail_order(molar_hip_ctx *ctx, const float *xyz, size_t natoms, const uint64_t *idx,
                               const uint64_t *tail_offsets, size_t ntails, int order_type, const float *normals,
                               const uint64_t *normal_offsets, const uint8_t *bond_orders, float *out);

/* ------------------------------------------------------------------ XTC frames (molar/src/io/xtc_handler.rs)
 *
 * Feeds the path with trajectory frames: MolAR's XtcFileHandler over the un-vendored `molly` crate
 * (read_state :64-112 -> State{coords, time, pbox}; seek_frame :200-218; seek_time :220-229 = first frame with
 * time >= t, :282-297).  GROMACS XTC, magic 1995 and 2023.  The file is indexed once at open (headers only);
 * molar_hip_xtc_read decodes `count` consecutive frames on `nthreads` host threads (0 = all cores; a frame's bit
 * stream is serial, frames are independent) into xyz[count][natoms][3] (nm), which may be host memory or device
 * memory (then through pinned staging and async copies on the context's stream; ctx may be NULL for host output).
 * box9 of a frame is column-major with columns a,b,c (Matrix3f::from_iterator(boxvec), :100).  A truncated last
 * frame ends the index (the reference reports Eof there, :325-332).  Returns ERR_IO / ERR_SIZES (frames of
 * different atom counts in one read). */
typedef struct molar_hip_xtc molar_hip_xtc;
molar_hip_xtc *molar_hip_xtc_open(const char *path);
molar_hip_xtc *molar_hip_xtc_open_memory(const void *data, size_t bytes);   /* borrowed, must outlive the handle */
void molar_hip_xtc_close(molar_hip_xtc *x);
size_t molar_hip_xtc_nframes(const molar_hip_xtc *x);
size_t molar_hip_xtc_natoms(const molar_hip_xtc *x);
int molar_hip_xtc_frame_info(const molar_hip_xtc *x, size_t frame, int32_t *natoms, int32_t *step, float *time,
                             float box9[9], float *precision);
int molar_hip_xtc_seek_time(const molar_hip_xtc *x, float t, size_t *frame);
int molar_hip_xtc_read(molar_hip_ctx *ctx, const molar_hip_xtc *x, size_t first, size_t count, float *xyz,
                       int nthreads);
/* The same window decoded ON THE DEVICE, one lane per frame (64 frames per wave): the window's compressed bytes go over the
 * link (about a third of the decoded size), `xyz_dev` (device memory, float[count][natoms][3]) is written by the kernel.
 * Bit-identical to molar_hip_xtc_read (one decoder, compiled for both sides).  A lane is far slower than a host core, so
 * this pays for windows of hundreds to thousands of frames - when the consumers of a multi-GPU node outrun the host's
 * decoder threads.  Frames whose packed triples exceed 64 bits fall back to the host decoder inside the call. */
int molar_hip_xtc_read_device(molar_hip_ctx *ctx, const molar_hip_xtc *x, size_t first, size_t count, float *xyz_dev);
/* A radial distance histogram over a block of the trajectory in one call (BASELINE config 4 for a caller without device memory
 * of its own - the process_frame loop of an RDF task, analysis_task.rs:245-252, with Histogram1D::add_one over every distance of
 * distance_search_single_pbc, molar_membrane/src/stats.rs:29-35): frames [first, first + count) are decoded on `decode_threads`
 * host threads (0 = all) into windows of 16 frames in HBM while the window before is in the fused histogram
 * (molar_hip_search_histogram_frames: selection idx - NULL = all atoms - of every frame against itself, cutoff, the frame's own
 * box from its header, periodic dimensions `pbc`); integer bins, ADDED into bins[nbins] (host) at the end.  The same sums as
 * molar_hip_xtc_read + molar_hip_search_histogram frame by frame. */
int molar_hip_xtc_histogram(molar_hip_ctx *ctx, const molar_hip_xtc *x, size_t first, size_t count, const uint64_t *idx, size_t n,
                            float cutoff, uint8_t pbc, float hmin, float hmax, size_t nbins, uint64_t *bins, int decode_threads);
/* The same between TWO selections of every frame (distance_search_double_pbc: the radial distribution of one species around
 * another); idx1 / idx2 NULL = all atoms.  Selections may overlap (an atom against itself counts at distance 0, as in the
 * reference). */
int molar_hip_xtc_histogram_double(molar_hip_ctx *ctx, const molar_hip_xtc *x, size_t first, size_t count, const uint64_t *idx1,
                                   size_t n1, const uint64_t *idx2, size_t n2, float cutoff, uint8_t pbc, float hmin, float hmax,
                                   size_t nbins, uint64_t *bins, int decode_threads);
/* Writer (xtc_handler.rs:117-168, write_state through molly::XTCWriter): ONE frame in GROMACS' compressed coordinate format
 * (magic 1995; xdrfile's algorithm: integer grid at `precision`, mixed-radix triples, runs of small deltas with an adaptive
 * delta size) into out[cap]; *out_len = bytes written, frames are simply concatenated in a file.  96 + 16 * natoms bytes
 * always suffice.  box9 as in the header (9 floats, the order the file stores).  Host memory only. */
int molar_hip_xtc_encode_frame(const float *xyz, size_t natoms, const float *box9, int32_t step, float time, float precision,
                               uint8_t *out, size_t cap, size_t *out_len);

/* ------------------------------------------------------------------ Modify (modify.rs) */

/* apply_transform :32-36 — in place on xyz (host buffers are copied back). */
int molar_hip_apply_transform(molar_hip_ctx *ctx, float *xyz, size_t natoms, const uint64_t *idx, size_t n,
                              const float R9[9], const float t3[3]);
/* unwrap_simple_dim :40-54 */
int molar_hip_unwrap_simple(molar_hip_ctx *ctx, float *xyz, size_t natoms, const uint64_t *idx, size_t n,
                            const float *box9, uint8_t pbc);

/* ------------------------------------------------------------------ batched per-frame analysis */

/* The per-frame align+RMSD loop of the reference's benchmark (benches/comparison_small.rs:14-25,
 * SURVEY.md §3.4) for `nframes` frames resident in one buffer frames[nframes][natoms][3]:
 *   tr = fit_transform(cur, ref); apply_transform(cur, tr); rmsd(cur, ref);
 *   center_of_mass(cur); gyration(cur)
 * Selection idx/mass are shared by all frames (topology-side arrays).  `frames` is modified in
 * place when apply != 0.  Outputs are per frame; any of them may be NULL.
 * Replaces the serial frame loop of AnalysisTask::run (analysis_task.rs:202-252) for this task. */
int molar_hip_fit_rmsd_batch(molar_hip_ctx *ctx, float *frames, size_t nframes, size_t natoms,
                             const uint64_t *idx, size_t n, const float *mass, const float *ref_xyz,
                             size_t ref_natoms, const uint64_t *ref_idx, int apply, float *rmsd_out,
                             float *R_out /*[nframes][9]*/, float *t_out /*[nframes][3]*/,
                             float *com_out /*[nframes][3]*/, float *gyr_out /*[nframes]*/);

/* The same loop for a trajectory whose frames live in HOST memory, at the rate the SELECTION crosses the link (a Rust
 * AnalysisTask hands its State's coords over frame by frame, analysis_task.rs:245-252; molar_hip_fit_rmsd_batch on a host frame
 * stages all natoms x 12 bytes from pageable memory per call).  _create packs the frame-invariant columns once (reference
 * selection, the masses of the selected atoms; all topology-side arrays in host memory) and starts `host_threads` threads
 * (0: min(8, cores / 2)) that take the selected atoms out of a frame into pinned staging.  _begin(frame) gathers, sends the packed
 * selection behind the frame before it, enqueues the batch entry's kernels on it and returns a ticket (0..2; up to three frames
 * in flight: `begin(k + 1); end(k)`); _end(ticket) waits for that frame and returns what the batch entry returns per frame
 * (each output optional) - bit-identical to it: same terms, same order.  apply != 0: the fitted selection is written into the
 * frame handed to _begin (which must stay valid, and untouched, until _end) - apply_transform (modify.rs:32-36).  Errors as for
 * the batch entry (ERR_SIZES, ERR_ZERO_MASS, ERR_SVD_FAILED from _end). */
typedef struct molar_hip_fit_stream molar_hip_fit_stream;
int molar_hip_fit_stream_create(molar_hip_ctx *ctx, size_t natoms, const uint64_t *idx, size_t n, const float *mass,
                                const float *ref_xyz, size_t ref_natoms, const uint64_t *ref_idx, int host_threads,
                                molar_hip_fit_stream **out);
int molar_hip_fit_stream_begin(molar_hip_fit_stream *stream, float *xyz, int apply, int32_t *ticket);
int molar_hip_fit_stream_end(molar_hip_fit_stream *stream, int32_t ticket, float *rmsd, float R9[9], float t3[3], float com3[3],
                             float *gyration);
void molar_hip_fit_stream_destroy(molar_hip_fit_stream *stream);

/* ------------------------------------------------------------------ batched over K selections (CSR)
 * What MolAR runs from rayon over a ParSplit (selection/system.rs:193-213, README.md:656-691): the same Measure method
 * on thousands of small sub-selections (residues, lipids, molecules).  Selection k is idx[offsets[k] .. offsets[k+1]);
 * one 64-lane wave works on each.  Outputs are per selection, caller-allocated (host or device). */

/* gyration (measure.rs:78-87); with box9 != NULL gyration_pbc (:222-232).  out[nsel]. */
int molar_hip_gyration_batch(molar_hip_ctx *ctx, const float *xyz, size_t natoms, const uint64_t *idx,
                             const uint64_t *offsets, size_t nsel, const float *mass, const float *box9, float *out);

/* rmsd (measure.rs:485-504) of selection k of frame 1 against selection k of frame 2 (idx2 NULL: same atoms); with
 * mass1 != NULL rmsd_mw (:538-558).  out[nsel]. */
int molar_hip_rmsd_batch(molar_hip_ctx *ctx, const float *xyz1, size_t natoms1, const uint64_t *idx1, const float *xyz2,
                         size_t natoms2, const uint64_t *idx2, const uint64_t *offsets, size_t nsel, const float *mass1,
                         float *out);

/* fit_transform (measure.rs:507-522) of every selection of frame 1 onto its counterpart in frame 2 (idx2 NULL: same
 * atoms; mass2 NULL or mass1: the column mass1 read through idx2, selection 2's own masses - INVALID_ARGUMENT if idx2
 * differs from idx1 and frame 2 has more atoms than that column); apply != 0 moves the selections of xyz1 in place
 * (modify.rs:32-36).  Any output may be NULL: R_out[nsel][9] column-major, t_out[nsel][3], and of the FITTED selection
 * rmsd_out[nsel] (unweighted, :485-504), com_out[nsel][3], gyr_out[nsel]. */
int molar_hip_fit_batch(molar_hip_ctx *ctx, float *xyz1, size_t natoms1, const uint64_t *idx1, const float *mass1,
                        const float *xyz2, size_t natoms2, const uint64_t *idx2, const float *mass2,
                        const uint64_t *offsets, size_t nsel, int apply, float *R_out, float *t_out, float *rmsd_out,
                        float *com_out, float *gyr_out);

/* ------------------------------------------------------------------ Modify::translate / rotate, principal axes */

/* translate (modify.rs:16-23): p += shift for every selected atom, in place. */
int molar_hip_translate(molar_hip_ctx *ctx, float *xyz, size_t natoms, const uint64_t *idx, size_t n, const float shift3[3]);

/* rotate (modify.rs:25-30): p <- Rotation3::from_axis_angle(unit_axis, angle) * p about the origin, in place. */
int molar_hip_rotate(molar_hip_ctx *ctx, float *xyz, size_t natoms, const uint64_t *idx, size_t n,
                     const float unit_axis3[3], float angle);

/* principal_transform (measure.rs:102-109) / principal_transform_pbc (:246-257, box9 != NULL): the isometry
 * Translation(cm) * Rotation(axes^-1) * Translation(-cm) (:646-649) as R9 (column-major) and t3, p -> R p + t. */
int molar_hip_principal_transform(molar_hip_ctx *ctx, const float *xyz, size_t natoms, const uint64_t *idx, size_t n,
                                  const float *mass, const float *box9, float R9[9], float t3[3]);


#ifdef __cplusplus
}
#endif
#endif /* MOLAR_HIP_H */
