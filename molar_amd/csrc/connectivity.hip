// connectivity.hip - SearchConnectivity on the device (molar_hip_search_connectivity / _fill) and unwrap_connectivity: a consumer
// of the f32 search (search_core.hpp: the resident pair list), and the one home of the CSR build for both precisions
// (search_f64.hip writes its entries between connectivity_begin and connectivity_finish).  The cached CSR is this unit's state,
// behind molar_hip_ctx::conn.
#include <vector>

#include "boxmath.hpp"
#include "common.hpp"
#include "csr_kernels.hpp"
#include "hoststream.hpp"
#include "search_core.hpp"
#include "stages.hpp"
#include "unwrap_walk.hpp"

using namespace mh;

struct molar_hip_connectivity_state {
    DevBuf conn_deg;           // scratch of the sort
    DevBuf conn_off;           // u64 per row (+1): offsets
    DevBuf conn_ent;           // four u32 arrays of conn_entries each: rows and neighbours, unsorted and sorted
    DevBuf conn_neigh;         // u64 per entry: the lists
    uint64_t conn_rows = 0, conn_entries = 0;
    bool have_conn = false;
};

void mh::connectivity_release(molar_hip_ctx *c) { release_state(c->conn); }

void mh::connectivity_forget(molar_hip_ctx *c) {
    if (c->conn) c->conn->have_conn = false;
}

int mh::connectivity_begin(molar_hip_ctx *c, uint64_t nrows, uint64_t npairs, uint32_t **row_in, uint32_t **nb_in) {
    molar_hip_connectivity_state &N = state_of(c->conn);
    N.have_conn = false;
    const uint64_t nent = 2ull * npairs;
    MH_TRY(N.conn_off.reserve((nrows + 1) * 8));
    MH_TRY(N.conn_ent.reserve((nent ? nent : 1) * 16));
    MH_TRY(N.conn_neigh.reserve((nent ? nent : 1) * 8));
    N.conn_rows = nrows;
    N.conn_entries = nent;
    *row_in = N.conn_ent.as<uint32_t>();
    *nb_in = *row_in + nent;
    return 0;
}

int mh::connectivity_finish(molar_hip_ctx *c) {
    molar_hip_connectivity_state &N = *c->conn;
    const uint64_t nrows = N.conn_rows, nent = N.conn_entries;
    uint32_t *row_in = N.conn_ent.as<uint32_t>(), *nb_in = row_in + nent, *row_out = nb_in + nent, *nb_out = row_out + nent;
    if (nent) {
        int end_bit = 1;
        while (end_bit < 32 && (nrows >> end_bit)) ++end_bit;
        MH_TRY(device_sort_pairs_u32(c->stream, N.conn_deg, row_in, row_out, nb_in, nb_out, (size_t)nent, end_bit));
        hipLaunchKernelGGL(conn_widen_kernel, dim3((unsigned)((nent + 255) / 256)), dim3(256), 0, c->stream, nb_out, (unsigned long long)nent,
                           N.conn_neigh.as<unsigned long long>());
    }
    hipLaunchKernelGGL(conn_offsets_kernel, dim3((unsigned)((nrows + 1 + 255) / 256)), dim3(256), 0, c->stream, row_out, (unsigned long long)nent,
                       (uint32_t)nrows, N.conn_off.as<unsigned long long>());
    MH_HIP(hipGetLastError());
    N.have_conn = true;
    return 0;
}

namespace {

// ================================================================= SearchConnectivity on the device (connectivity.rs:19-35)
// `for (i, j) in pairs { conn[i].push(j); conn[j].push(i) }` as CSR: degrees by atomics, an exclusive scan, every entry
// dropped into its list in arrival order, then moved to its place - the number of entries of the same list that come from
// earlier pairs (a pair feeds a list at most once per side; the entry of its i side precedes that of its j side when i == j
// never happens: the single searches emit i != j).  Lists are a handful of bonded neighbours long, so the ranking reads its
// own list; the result is the reference's push order exactly.
// SearchConnectivity::from_iter (connectivity.rs:19-35): pair p pushes j onto i's list (entry 2p), then i onto j's (entry 2p + 1).
// A list in push order is the entries of its row in entry order: a STABLE sort of the entries by row (devsort.hip).  (Until the end
// of round 5: atomics into buckets, then every entry ranked against its whole list - quadratic in the list length, 10 ms of an
// 11 ms call for 25k atoms at rc 1.0 nm, 420 entries per list.)
__global__ void __launch_bounds__(256) conn_entries_kernel(const uint2 *__restrict__ pairs, unsigned long long npairs, uint32_t *__restrict__ row,
                                                           uint32_t *__restrict__ nb) {
    const unsigned long long p = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    if (p >= npairs) return;
    const uint2 ij = pairs[p];
    reinterpret_cast<uint2 *>(row)[p] = make_uint2(ij.x, ij.y);
    reinterpret_cast<uint2 *>(nb)[p] = make_uint2(ij.y, ij.x);
}

}  // namespace

extern "C" {

// SearchConnectivity (connectivity.rs:8-60) of a single-selection search, built on the device from the resident pair list:
// CSR over the id range of the request (local ids: the selection's length; global ids: natoms), lists in the reference's push
// order.  Count-then-fill: the first call runs the search and builds the CSR in context-owned device memory and returns the
// number of entries (2 x pairs); the second copies offsets (rows + 1) and neighbours to host or device memory.
int molar_hip_search_connectivity(molar_hip_ctx *c, const molar_hip_search_desc *q, uint64_t *out_rows, uint64_t *out_entries) {
    if (!c || !q) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "search_connectivity: null argument");
    if (q->kind != MOLAR_HIP_SEARCH_SINGLE)
        return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "search_connectivity: ids of one selection index the lists - the request must be of kind MOLAR_HIP_SEARCH_SINGLE");
    connectivity_forget(c);
    // the lists hold ids only: the (i, j) plane alone (DistanceSearchOutput of (usize, usize), distance_search.rs:14-20)
    MH_TRY(resident_pairs(c, q));
    const uint64_t npairs = c->total;
    const uint32_t *d_pairs = c->out_pairs.as<uint32_t>();
    const size_t nsel = q->idx1 ? q->n1 : q->natoms1;
    const uint64_t nrows = q->ids_local ? nsel : (q->idx1 ? q->natoms1 : nsel);
    if (nrows >= 0xFFFFFFF0ull) return fail(MOLAR_HIP_ERR_TOO_LARGE, "search_connectivity: too many rows");
    const uint64_t nent = 2ull * npairs;
    if (nent >= 0x7FFFFFFFull) return fail(MOLAR_HIP_ERR_TOO_LARGE, "search_connectivity: %llu list entries", (unsigned long long)nent);
    uint32_t *row_in = nullptr, *nb_in = nullptr;
    MH_TRY(connectivity_begin(c, nrows, npairs, &row_in, &nb_in));
    const unsigned nbP = (unsigned)((npairs + 255) / 256);
    if (nbP)
        hipLaunchKernelGGL(conn_entries_kernel, dim3(nbP), dim3(256), 0, c->stream, reinterpret_cast<const uint2 *>(d_pairs), (unsigned long long)npairs,
                           row_in, nb_in);
    MH_TRY(connectivity_finish(c));
    if (out_rows) *out_rows = nrows;
    if (out_entries) *out_entries = nent;
    return MOLAR_HIP_OK;
}

int molar_hip_search_connectivity_fill(molar_hip_ctx *c, uint64_t *offsets, uint64_t *neigh) {
    if (!c || !c->conn || !c->conn->have_conn) return fail(MOLAR_HIP_ERR_NO_SEARCH, "no cached connectivity: call molar_hip_search_connectivity first");
    molar_hip_connectivity_state &N = *c->conn;
    MH_HIP(hipSetDevice(c->device));
    if (offsets) MH_HIP(hipMemcpyAsync(offsets, N.conn_off.p, (N.conn_rows + 1) * 8, hipMemcpyDefault, c->stream));
    if (neigh && N.conn_entries) {
        // large lists into ordinary host memory: the pinned ring and its host threads (hoststream.hpp), as the pair lists travel
        // (25k atoms at rc 1.0 nm: 83 MB of neighbours, 11 ms through the runtime's pageable copy)
        if (!is_device_ptr(neigh) && ring_pays(N.conn_entries * 8, neigh)) {
            MH_HIP(hipStreamSynchronize(c->stream));
            std::vector<RingJob> jobs;
            jobs.push_back(RingJob{N.conn_neigh.p, (size_t)N.conn_entries * 8, RING_COPY, neigh, nullptr});
            return ring_to_host(c, jobs);
        }
        MH_HIP(hipMemcpyAsync(neigh, N.conn_neigh.p, N.conn_entries * 8, hipMemcpyDefault, c->stream));
    }
    MH_HIP(hipStreamSynchronize(c->stream));
    return MOLAR_HIP_OK;
}

// Modify::unwrap_connectivity_dim (molar/src/modify.rs:72-131).  The neighbour search - the heavy part - runs on the GPU
// (distance_search_single_pbc over the selection with LOCAL ids under full PBC, :77-78); the adjacency lists in push
// order (SearchConnectivity::from_iter, connectivity.rs:19-35: for (i, j) in pair order conn[i].push(j), conn[j].push(i))
// are built on the device from the resident pair list (molar_hip_search_connectivity), and the reference's stack walk (:84-128) - serial by nature: every
// atom is pulled to the closest image of the atom it was REACHED FROM, whose position the walk may just have changed -
// runs on the host over that CSR with the same f32 arithmetic (boxmath.hpp's closest_image, the one the kernels use).
// Quirks kept: the atom a component starts from (0, then the lowest unused index) is not a member of the selection
// the component returns (:97-98,111-113); a component of one atom returns no selection; members are emitted as the
// reference's `select(&sel_vec)` makes them, sorted.
int molar_hip_unwrap_connectivity(molar_hip_ctx *c, float *xyz, size_t natoms, const uint64_t *idx, size_t n, const float *box9,
                                  float cutoff, uint8_t pbc_dims, uint64_t *group_offsets, uint64_t *group_ids, size_t *ngroups) {
    if (!c || !xyz) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "unwrap_connectivity: null argument");
    if (!box9) return fail(MOLAR_HIP_ERR_NO_PBC, "no periodic box");                               // require_box (:76)
    const size_t nsel = idx ? n : natoms;
    if (nsel == 0) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "unwrap_connectivity of an empty selection");
    if (nsel >= 0x7FFFFFFFull) return fail(MOLAR_HIP_ERR_TOO_LARGE, "unwrap_connectivity: %zu atoms exceed the 32-bit local ids", nsel);
    MH_HIP(hipSetDevice(c->device));
    molar_hip_box b;
    MH_TRY(molar_hip_box_from_matrix(box9, &b));
    // ---- the search, local ids (0..len), full PBC whatever `dims` (:77-78)
    molar_hip_search_desc q{};
    q.kind = MOLAR_HIP_SEARCH_SINGLE;
    q.cutoff = cutoff;
    q.xyz1 = xyz; q.natoms1 = natoms; q.idx1 = idx; q.n1 = n;
    q.ids_local = 1;
    q.box9 = box9;
    q.pbc = MOLAR_HIP_PBC_FULL;
    // ---- adjacency in push order: SearchConnectivity on the device, only the CSR comes to the host
    uint64_t nrows = 0, nent = 0;
    MH_TRY(molar_hip_search_connectivity(c, &q, &nrows, &nent));
    std::vector<uint64_t> off(nsel + 1, 0), adj((size_t)(nent ? nent : 1));
    MH_TRY(molar_hip_search_connectivity_fill(c, off.data(), adj.data()));
    // ---- the coordinates of the frame on the host
    const bool dev = is_device_ptr(xyz);
    std::vector<float> hostcopy;
    float *h = xyz;
    if (dev) {
        hostcopy.resize(natoms * 3);
        MH_HIP(hipMemcpyAsync(hostcopy.data(), xyz, natoms * 12, hipMemcpyDeviceToHost, c->stream));
        MH_HIP(hipStreamSynchronize(c->stream));
        h = hostcopy.data();
    }
    std::vector<uint64_t> hidx;
    if (idx && is_device_ptr(idx)) {      // the walk reads the selection on the host
        hidx.resize(n);
        MH_HIP(hipMemcpy(hidx.data(), idx, n * 8, hipMemcpyDeviceToHost));
    }
    const uint64_t *ix = hidx.empty() ? idx : hidx.data();
    // ---- the walk (:80-128), one template with the f64 entry (unwrap_walk.hpp)
    unwrap_walk<float, V3>(h, ix, nsel, b, pbc_dims & 7u, off.data(), adj.data(), group_offsets, group_ids, ngroups);
    if (dev) {
        MH_HIP(hipMemcpyAsync(xyz, hostcopy.data(), natoms * 12, hipMemcpyHostToDevice, c->stream));
        MH_HIP(hipStreamSynchronize(c->stream));
    }
    return MOLAR_HIP_OK;
}

}  // extern "C"
