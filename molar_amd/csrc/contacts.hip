// contacts.hip - the fused contact counts (molar_hip_search_contacts / _frames) and the connected components of the contact
// graph (molar_hip_search_clusters / _frames / _counters): consumers of the f32 search that read the slot records of its regular
// plan with kernels of their own (contact_kernels.hpp, cluster_kernels.hpp).  They share a second context, the label check and
// the per-frame search; all they keep is this unit's state, behind molar_hip_ctx::contacts of the CALLER's context.
#include <algorithm>
#include <vector>

#include "common.hpp"
#include "cluster_kernels.hpp"
#include "contact_kernels.hpp"
#include "search_core.hpp"
#include "stages.hpp"

using namespace mh;
using namespace mh::pairk;

struct molar_hip_contacts_state {
    // A second context on the caller's stream holds the grid, plan and slot records of these calls, so the cached search of the
    // caller's (count -> fill, a held `within` grid, the histogram's grid generations) is not disturbed.  It is nothing but a
    // holder of a cached search: the buffers of the calls themselves are here.
    molar_hip_ctx *search = nullptr;
    // contacts: staged labels, 64-bit accumulators of outputs that go to host memory [count | deg1 | deg2 | map], the per-frame
    // 32-bit map of the frames form and the occupancy of a host caller
    DevBuf g1, g2, acc, frame, occ;
    // clusters (labels staged in g1): the forest and what is derived from it [parent | root | flag | rank | comp | sizes | iota |
    // sorted keys | members | offsets], the scratch of its scans and sort, the per-frame results of the frames form
    // [size_hist | ncomponents | largest]
    DevBuf cl_work, cl_tmp, cl_acc;
    // molar_hip_search_clusters_counters: the four words and the switch
    DevBuf cl_stats;
    bool cl_counting = false;
};

// the second context goes first, with the stream it borrowed handed back: the caller's stream is still alive here
void mh::contacts_release(molar_hip_ctx *c) {
    if (!c->contacts) return;
    if (molar_hip_ctx *s = c->contacts->search) {
        s->stream = c->stream;
        molar_hip_destroy(s);
    }
    release_state(c->contacts);
}

// ================================================================= fused contact counts (contact_kernels.hpp, pair_k9.hip)
//
// molar_hip_search_contacts / _frames.  The grid, the REGULAR plan and its slot records are those of the count pass
// (prepare_search with ids_local forced on, so the id an atom carries is its position in the selection); contact_kernel walks
// the slot list once and adds degrees, map and |L| on chip-summed portions.  All of it runs on a second context that shares
// the caller's stream (molar_hip_contacts_state::search): nothing the caller has cached in its own context - a counted search
// waiting for its fill, a held `within` grid, the histogram's grid generations - is touched.
// Outputs in device memory are added into directly; outputs in host memory go through zeroed 64-bit accumulators that are
// read back and added on the host at the end of the call (of the block, in the frames form).
// Occupancy (frames form): the kernel adds the frame's map into ONE 32-bit scratch matrix of ngroups1 * ngroups2 words; behind
// the frame's kernel contact_fold_kernel adds it into the map, counts its non-zero entries into the occupancy and clears it.
// The frames are walked one after the other on one stream, so the fold of frame k is ordered in front of the kernel of
// frame k + 1 and one scratch (4 bytes per map entry, 64 MiB at the 2^24 cap) serves the whole block.
namespace {

__global__ void __launch_bounds__(256) contact_check_labels_kernel(const uint32_t *__restrict__ g, size_t n, uint32_t ngroups, uint32_t *__restrict__ flag) {
    for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (size_t)gridDim.x * 256u)
        if (g[i] >= ngroups) *flag = 1u;
}

__global__ void __launch_bounds__(256) contact_fold_kernel(uint32_t *__restrict__ frame, size_t n, unsigned long long *__restrict__ map,
                                                           uint32_t *__restrict__ occ) {
    for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (size_t)gridDim.x * 256u) {
        const uint32_t v = frame[i];
        if (v) {
            if (map) map[i] += v;
            if (occ) occ[i] += 1u;
            frame[i] = 0u;
        }
    }
}

struct ContactCall {
    molar_hip_contacts_state *z = nullptr;
    molar_hip_ctx *s = nullptr;        // the second context (z->search)
    bool two = false;
    size_t n1 = 0, n2 = 0, nmap = 0;
    const uint32_t *g1 = nullptr, *g2 = nullptr;                 // device labels (NULL: no map, no occupancy)
    size_t ng2 = 0;
    uint64_t *h_deg1 = nullptr, *h_deg2 = nullptr, *h_map = nullptr;   // caller's HOST outputs (added at the end)
    uint32_t *h_occ = nullptr;
    unsigned long long *t_count = nullptr, *t_deg1 = nullptr, *t_deg2 = nullptr, *t_map = nullptr;   // what the kernels add into
    uint32_t *t_frame = nullptr, *t_occ = nullptr;
};

constexpr size_t CONTACT_MAP_MAX = (size_t)1 << 24;

// labels of one set: checked (on the host when they are host memory, else by a kernel and a 4-byte read-back), then device-readable
int contact_labels(molar_hip_ctx *s, const uint32_t *g, size_t n, size_t ngroups, DevBuf &stage, const uint32_t **out, const char *who) {
    const uint32_t ng = (uint32_t)ngroups;
    if (!is_device_ptr(g)) {
        for (size_t i = 0; i < n; ++i)
            if (g[i] >= ng)
                return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: label %u of atom %zu is not below ngroups = %zu", who, g[i], i, ngroups);
        return to_device(s, g, n, stage, out);
    }
    *out = g;
    if (n == 0) return 0;
    MH_TRY(s->hist.reserve(64));
    uint32_t *flag = s->hist.as<uint32_t>();
    MH_HIP(hipMemsetAsync(flag, 0, 4, s->stream));
    const unsigned nb = (unsigned)std::min<size_t>((n + 255) / 256, 1024);
    hipLaunchKernelGGL(contact_check_labels_kernel, dim3(nb), dim3(256), 0, s->stream, g, n, ng, flag);
    MH_HIP(hipGetLastError());
    uint32_t bad = 0;
    MH_TRY(read_back(s, &bad, flag, 4));
    if (bad) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: a label is not below ngroups = %zu", who, ngroups);
    return 0;
}

// the state of the contacts and clusters calls and its second context, made on first use, on the caller's stream
int contacts_context(molar_hip_ctx *c, molar_hip_contacts_state **state, molar_hip_ctx **out) {
    MH_HIP(hipSetDevice(c->device));
    molar_hip_contacts_state &Z = state_of(c->contacts);
    if (!Z.search) {
        molar_hip_ctx *s = molar_hip_create(c->device);
        if (!s) return MOLAR_HIP_ERR_HIP;
        (void)hipStreamDestroy(s->stream);
        s->own_stream = false;
        Z.search = s;
    }
    Z.search->stream = c->stream;
    *state = &Z;
    *out = Z.search;
    return 0;
}

// The search of one frame as the contact and the cluster kernels want it, in the second context: ids are positions in the
// selection whatever the caller's list would carry, the regular plan over consecutive rows, no hit history.  *nslots: the
// slots to launch over (0: nothing to do); the plan kernel leaves the parameter block in s->params.
int frame_search(molar_hip_ctx *s, const molar_hip_search_desc *q, uint32_t *nslots) {
    *nslots = 0;
    molar_hip_search_desc qq = *q;
    qq.ids_local = 1;
    SearchCall call;
    call.size_masks = false;
    call.live_rows = false;
    bool degenerate;
    MH_TRY(prepare_search(s, &qq, call, &degenerate));
    s->params_fresh = false;
    if (degenerate) return 0;               // (never: empty sets have returned before they get here)
    *nslots = (uint32_t)s->cur.nslots_bound;
    return 0;
}

// frame f of a block: the request with its coordinates and box moved on
molar_hip_search_desc frame_desc(const molar_hip_search_desc *q, size_t f, size_t xyz1_stride, size_t xyz2_stride, const float *boxes9) {
    molar_hip_search_desc qf = *q;
    qf.xyz1 = q->xyz1 + f * xyz1_stride;
    if (q->xyz2) qf.xyz2 = q->xyz2 + f * xyz2_stride;
    if (boxes9) qf.box9 = boxes9 + 9 * f;
    return qf;
}

int contacts_begin(molar_hip_ctx *c, const molar_hip_search_desc *q, const molar_hip_contact_groups *groups, uint64_t *deg1, uint64_t *deg2,
                   uint64_t *map, uint32_t *occ, ContactCall &K, const char *who) {
    if (!c || !q) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: null argument", who);
    if (q->kind != MOLAR_HIP_SEARCH_SINGLE && q->kind != MOLAR_HIP_SEARCH_DOUBLE)
        return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: only the SINGLE and DOUBLE kinds have contact counts (got kind %d)", who, q->kind);
    K.two = q->kind == MOLAR_HIP_SEARCH_DOUBLE;
    if (!K.two && deg2) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: deg2 must be NULL for a single-set search (deg1 counts both members)", who);
    if (!q->xyz1 || (K.two && !q->xyz2)) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "search: xyz pointer is null");
    K.n1 = q->idx1 ? q->n1 : q->natoms1;
    K.n2 = K.two ? (q->idx2 ? q->n2 : q->natoms2) : 0;
    const bool want_map = map != nullptr || occ != nullptr;
    size_t G1 = 0, G2 = 0;
    if (want_map) {
        if (!groups || !groups->group1 || (K.two && !groups->group2))
            return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: a map or an occupancy needs group labels", who);
        G1 = groups->ngroups1;
        G2 = K.two ? groups->ngroups2 : G1;
        if (G1 > CONTACT_MAP_MAX || G2 > CONTACT_MAP_MAX || G1 * G2 > CONTACT_MAP_MAX)
            return fail(MOLAR_HIP_ERR_TOO_LARGE, "%s: the map is dense, ngroups1 * ngroups2 may be 2^24 at most (got %zu x %zu)", who, G1, G2);
        if ((G1 == 0 && K.n1 != 0) || (G2 == 0 && (K.two ? K.n2 : K.n1) != 0))
            return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: a label is not below ngroups = 0", who);
    }
    K.nmap = G1 * G2;
    K.ng2 = G2;
    MH_TRY(contacts_context(c, &K.z, &K.s));
    molar_hip_ctx *s = K.s;
    molar_hip_contacts_state &Z = *K.z;
    if (want_map && K.nmap) {
        MH_TRY(contact_labels(s, groups->group1, K.n1, G1, Z.g1, &K.g1, who));
        if (K.two) MH_TRY(contact_labels(s, groups->group2, K.n2, G2, Z.g2, &K.g2, who));
        else K.g2 = K.g1;
    }
    // ---- where the sums go
    const bool d1 = deg1 && !is_device_ptr(deg1), d2 = deg2 && !is_device_ptr(deg2), dm = map && !is_device_ptr(map);
    const size_t words = 1 + (d1 ? K.n1 : 0) + (d2 ? K.n2 : 0) + (dm ? K.nmap : 0);
    MH_TRY(Z.acc.reserve(words * 8));
    MH_HIP(hipMemsetAsync(Z.acc.p, 0, words * 8, s->stream));
    unsigned long long *w = Z.acc.as<unsigned long long>();
    K.t_count = w;
    w += 1;
    K.t_deg1 = reinterpret_cast<unsigned long long *>(deg1);
    K.t_deg2 = reinterpret_cast<unsigned long long *>(deg2);
    K.t_map = reinterpret_cast<unsigned long long *>(map);
    if (d1) { K.h_deg1 = deg1; K.t_deg1 = w; w += K.n1; }
    if (d2) { K.h_deg2 = deg2; K.t_deg2 = w; w += K.n2; }
    if (dm) { K.h_map = map; K.t_map = w; w += K.nmap; }
    if (occ && K.nmap) {
        MH_TRY(Z.frame.reserve(K.nmap * 4));
        MH_HIP(hipMemsetAsync(Z.frame.p, 0, K.nmap * 4, s->stream));
        K.t_frame = Z.frame.as<uint32_t>();
        K.t_occ = occ;
        if (!is_device_ptr(occ)) {
            MH_TRY(Z.occ.reserve(K.nmap * 4));
            MH_HIP(hipMemsetAsync(Z.occ.p, 0, K.nmap * 4, s->stream));
            K.h_occ = occ;
            K.t_occ = Z.occ.as<uint32_t>();
        }
    }
    return 0;
}

// one frame: grid, plan, the contact kernel and (frames form with occupancy) the fold - enqueued, nothing waited for beyond what
// prepare_search itself needs (the bounding box of a non-periodic request is read back)
int contacts_frame(ContactCall &K, const molar_hip_search_desc *q) {
    if (K.n1 == 0 || (K.two && K.n2 == 0)) return 0;
    molar_hip_ctx *s = K.s;
    uint32_t nslots;
    MH_TRY(frame_search(s, q, &nslots));
    if (nslots == 0) return 0;
    ContactArgs A{};
    A.g1 = K.g1;
    A.g2 = K.g2;
    A.ng2 = (uint32_t)K.ng2;
    A.deg1 = K.t_deg1;
    A.deg2 = K.two ? K.t_deg2 : K.t_deg1;
    A.map = K.t_frame ? nullptr : K.t_map;
    A.map32 = K.t_frame;
    if (!A.map && !A.map32) A.g1 = A.g2 = nullptr;
    A.count = K.t_count;
    {
        Prof prof(s, 3);
        launch_contacts(s->cur.kind, (unsigned)s->num_cus, s->stream, s->params.as<SearchParams>(), s->slot_desc.as<SlotDesc>(), nslots, A);
        MH_HIP(hipGetLastError());
    }
    if (K.t_frame) {
        const unsigned nb = (unsigned)std::min<size_t>((K.nmap + 255) / 256, (size_t)s->num_cus * 16);
        hipLaunchKernelGGL(contact_fold_kernel, dim3(nb), dim3(256), 0, s->stream, K.t_frame, K.nmap, K.t_map, K.t_occ);
        MH_HIP(hipGetLastError());
    }
    return 0;
}

int contacts_end(ContactCall &K, uint64_t *out_count) {
    molar_hip_ctx *s = K.s;
    auto add_back = [&](uint64_t *dst, const unsigned long long *src, size_t n) -> int {
        if (!dst || n == 0) return 0;
        std::vector<unsigned long long> h(n);
        MH_TRY(read_back(s, h.data(), src, n * 8));
        for (size_t i = 0; i < n; ++i) dst[i] += h[i];
        return 0;
    };
    MH_TRY(add_back(K.h_deg1, K.t_deg1, K.n1));
    MH_TRY(add_back(K.h_deg2, K.t_deg2, K.n2));
    MH_TRY(add_back(K.h_map, K.t_map, K.nmap));
    if (K.h_occ && K.nmap) {
        std::vector<uint32_t> h(K.nmap);
        MH_TRY(read_back(s, h.data(), K.t_occ, K.nmap * 4));
        for (size_t i = 0; i < K.nmap; ++i) K.h_occ[i] += h[i];
    }
    if (out_count) {
        unsigned long long tot = 0;
        MH_TRY(read_back(s, &tot, K.t_count, 8));
        *out_count = tot;
    }
    return 0;
}

// ================================================================= connected components (cluster_kernels.hpp, pair_k12.hip)
//
// molar_hip_search_clusters / _frames.  Grid, plan and slot records as for the contacts calls, in the same second context and
// under the same settings (frame_search: ids are positions in the selection, consecutive rows, no hit history), so nothing the caller has
// cached is touched.  Per frame, all on one stream: parent = identity; cluster_kernel unites the ends of every hit; then
// flatten -> scan of the root flags (ranks) -> labels and sizes -> (members wanted) scan of the sizes and one stable sort of
// (component, particle).  Everything is computed in this context's work area and copied to the caller's arrays, host or device.
struct ClusterCall {
    molar_hip_contacts_state *z = nullptr;
    molar_hip_ctx *s = nullptr;        // the second context (z->search)
    size_t n = 0, np = 0;              // selected atoms, particles
    const uint32_t *g = nullptr;       // device labels (NULL: every atom is a particle)
    bool members = false;              // offsets / members are wanted
    unsigned long long *stats = nullptr;
    uint32_t *parent = nullptr, *root = nullptr, *flag = nullptr, *rank = nullptr, *comp = nullptr, *sizes = nullptr, *iota = nullptr,
             *keys = nullptr, *memb = nullptr;
    unsigned long long *offsets = nullptr;
};

int clusters_begin(molar_hip_ctx *c, const molar_hip_search_desc *q, const molar_hip_contact_groups *groups, bool want_members, ClusterCall &K,
                   const char *who) {
    if (!c || !q) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: null argument", who);
    if (q->kind != MOLAR_HIP_SEARCH_SINGLE)
        return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: only the SINGLE kind has connected components (got kind %d)", who, q->kind);
    if (!q->xyz1) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "search: xyz pointer is null");
    K.n = q->idx1 ? q->n1 : q->natoms1;
    const bool grouped = groups && groups->group1;
    K.np = grouped ? groups->ngroups1 : K.n;
    if (grouped && K.np == 0 && K.n != 0) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: a label is not below ngroups = 0", who);
    if (K.np + 1 >= 0x7FFFFFFFull) return fail(MOLAR_HIP_ERR_TOO_LARGE, "%s: %zu particles", who, K.np);
    K.members = want_members;
    MH_TRY(contacts_context(c, &K.z, &K.s));
    molar_hip_ctx *s = K.s;
    molar_hip_contacts_state &Z = *K.z;
    if (grouped && K.n) MH_TRY(contact_labels(s, groups->group1, K.n, K.np, Z.g1, &K.g, who));
    if (Z.cl_counting) K.stats = Z.cl_stats.as<unsigned long long>();
    const size_t np = K.np, words = (9 * np + 3 + 1) & ~(size_t)1;
    MH_TRY(Z.cl_work.reserve(words * 4 + (np + 1) * 8));
    uint32_t *w = Z.cl_work.as<uint32_t>();
    K.parent = w; w += np;
    K.root = w; w += np;
    K.flag = w; w += np + 1;
    K.rank = w; w += np + 1;
    K.comp = w; w += np;
    K.sizes = w; w += np + 1;
    K.iota = w; w += np;
    K.keys = w; w += np;
    K.memb = w;
    K.offsets = reinterpret_cast<unsigned long long *>(Z.cl_work.as<uint32_t>() + words);
    return 0;
}

// one frame, enqueued: the forest, its union over the frame's hits, and what is derived from it
int clusters_frame(ClusterCall &K, const molar_hip_search_desc *q) {
    if (K.np == 0) return 0;
    molar_hip_ctx *s = K.s;
    molar_hip_contacts_state &Z = *K.z;
    const unsigned cus = (unsigned)s->num_cus;
    const uint32_t np = (uint32_t)K.np;
    launch_cluster_init(cus, s->stream, K.parent, np);
    MH_HIP(hipGetLastError());
    if (K.n != 0) {
        uint32_t nslots;
        MH_TRY(frame_search(s, q, &nslots));
        if (nslots != 0) {
            ClusterArgs A{};
            A.g = K.g;
            A.parent = K.parent;
            A.stats = K.stats;
            Prof prof(s, 3);
            launch_clusters(cus, s->stream, s->params.as<SearchParams>(), s->slot_desc.as<SlotDesc>(), nslots, A);
            MH_HIP(hipGetLastError());
        }
    }
    launch_cluster_flatten(cus, s->stream, K.parent, np, K.root, K.flag);
    MH_HIP(hipGetLastError());
    MH_TRY(device_exclusive_sum_u32(s, Z.cl_tmp, K.flag, K.rank, (size_t)np + 1));      // rank[np] = number of components
    MH_HIP(hipMemsetAsync(K.sizes, 0, ((size_t)np + 1) * 4, s->stream));
    launch_cluster_label(cus, s->stream, K.root, K.rank, np, K.comp, K.sizes, K.iota);
    MH_HIP(hipGetLastError());
    if (K.members) {
        MH_TRY(device_exclusive_sum_u32_u64(s, Z.cl_tmp, K.sizes, K.offsets, (size_t)np + 1));
        int end_bit = 1;
        while (end_bit < 32 && ((uint64_t)1 << end_bit) < (uint64_t)np) ++end_bit;
        MH_TRY(device_sort_pairs_u32(s->stream, Z.cl_tmp, K.comp, K.keys, K.iota, K.memb, np, end_bit));
    }
    return 0;
}

// a result of this context's work area to the caller's array, host or device
int cluster_out(molar_hip_ctx *s, void *dst, const void *src, size_t bytes) {
    if (!dst || bytes == 0) return 0;
    if (is_device_ptr(dst)) {
        MH_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s->stream));
        return 0;
    }
    return read_back(s, dst, src, bytes);
}

}  // namespace

extern "C" {

int molar_hip_search_clusters(molar_hip_ctx *c, const molar_hip_search_desc *q, const molar_hip_contact_groups *groups, uint32_t *comp_of,
                              uint32_t *sizes, uint64_t *offsets, uint32_t *members, uint32_t *out_ncomponents) {
    ClusterCall K;
    MH_TRY(clusters_begin(c, q, groups, offsets != nullptr || members != nullptr, K, "search_clusters"));
    molar_hip_ctx *s = K.s;
    if (out_ncomponents) *out_ncomponents = 0;
    if (K.np == 0) {
        if (offsets && is_device_ptr(offsets)) MH_HIP(hipMemsetAsync(offsets, 0, 8, s->stream));
        else if (offsets) offsets[0] = 0;
        MH_HIP(hipStreamSynchronize(s->stream));
        return MOLAR_HIP_OK;
    }
    MH_TRY(clusters_frame(K, q));
    MH_TRY(cluster_out(s, comp_of, K.comp, K.np * 4));
    MH_TRY(cluster_out(s, sizes, K.sizes, K.np * 4));
    MH_TRY(cluster_out(s, offsets, K.offsets, (K.np + 1) * 8));
    MH_TRY(cluster_out(s, members, K.memb, K.np * 4));
    if (out_ncomponents) MH_TRY(read_back(s, out_ncomponents, K.rank + K.np, 4));
    MH_HIP(hipStreamSynchronize(s->stream));
    return MOLAR_HIP_OK;
}

int molar_hip_search_clusters_frames(molar_hip_ctx *c, const molar_hip_search_desc *q, const molar_hip_contact_groups *groups, size_t nframes,
                                     size_t xyz1_stride, const float *boxes9, uint32_t *ncomponents, uint32_t *largest, uint64_t *size_hist,
                                     uint32_t *comp_of_frames) {
    ClusterCall K;
    MH_TRY(clusters_begin(c, q, groups, false, K, "search_clusters_frames"));
    molar_hip_ctx *s = K.s;
    molar_hip_contacts_state &Z = *K.z;
    if (nframes == 0) return MOLAR_HIP_OK;
    // [size_hist of a host caller | ncomponents | largest], zeroed
    const size_t nh = K.np + 1, acc_bytes = nh * 8 + nframes * 8;
    MH_TRY(Z.cl_acc.reserve(acc_bytes));
    MH_HIP(hipMemsetAsync(Z.cl_acc.p, 0, acc_bytes, s->stream));
    unsigned long long *t_hist = Z.cl_acc.as<unsigned long long>();
    uint32_t *t_ncomp = reinterpret_cast<uint32_t *>(t_hist + nh), *t_largest = t_ncomp + nframes;
    const bool host_hist = size_hist && !is_device_ptr(size_hist);
    unsigned long long *hist = host_hist ? t_hist : reinterpret_cast<unsigned long long *>(size_hist);
    for (size_t f = 0; f < nframes; ++f) {
        const molar_hip_search_desc qf = frame_desc(q, f, xyz1_stride, 0, boxes9);
        MH_TRY(clusters_frame(K, &qf));
        if (K.np == 0) continue;
        launch_cluster_frame((unsigned)s->num_cus, s->stream, K.flag, K.rank, K.sizes, (uint32_t)K.np, t_ncomp + f, t_largest + f, hist);
        MH_HIP(hipGetLastError());
        if (comp_of_frames) MH_TRY(cluster_out(s, comp_of_frames + f * K.np, K.comp, K.np * 4));
    }
    MH_TRY(cluster_out(s, ncomponents, t_ncomp, nframes * 4));
    MH_TRY(cluster_out(s, largest, t_largest, nframes * 4));
    if (host_hist) {
        std::vector<unsigned long long> h(nh);
        MH_TRY(read_back(s, h.data(), t_hist, nh * 8));
        for (size_t i = 0; i < nh; ++i) size_hist[i] += h[i];
    }
    MH_HIP(hipStreamSynchronize(s->stream));
    return MOLAR_HIP_OK;
}

int molar_hip_search_clusters_counters(molar_hip_ctx *c, int32_t enable, uint64_t *out4) {
    MH_CTX(c);
    if (out4) {
        for (int k = 0; k < 4; ++k) out4[k] = 0;
        if (c->contacts && c->contacts->cl_stats.p) MH_TRY(read_back(c, out4, c->contacts->cl_stats.p, 32));
    }
    if (!enable && !c->contacts) return MOLAR_HIP_OK;       // never switched on, nothing to switch off
    molar_hip_contacts_state &Z = state_of(c->contacts);
    Z.cl_counting = enable != 0;
    if (Z.cl_counting) {
        MH_TRY(Z.cl_stats.reserve(32));
        MH_HIP(hipMemsetAsync(Z.cl_stats.p, 0, 32, c->stream));
    }
    return MOLAR_HIP_OK;
}

int molar_hip_search_contacts(molar_hip_ctx *c, const molar_hip_search_desc *q, const molar_hip_contact_groups *groups, uint64_t *deg1, uint64_t *deg2,
                              uint64_t *map, uint64_t *out_count) {
    ContactCall K;
    MH_TRY(contacts_begin(c, q, groups, deg1, deg2, map, nullptr, K, "search_contacts"));
    MH_TRY(contacts_frame(K, q));
    return contacts_end(K, out_count);
}

int molar_hip_search_contacts_frames(molar_hip_ctx *c, const molar_hip_search_desc *q, const molar_hip_contact_groups *groups, size_t nframes,
                                     size_t xyz1_stride, size_t xyz2_stride, const float *boxes9, uint64_t *deg1, uint64_t *deg2, uint64_t *map,
                                     uint32_t *occupancy) {
    ContactCall K;
    MH_TRY(contacts_begin(c, q, groups, deg1, deg2, map, occupancy, K, "search_contacts_frames"));
    for (size_t f = 0; f < nframes; ++f) {
        const molar_hip_search_desc qf = frame_desc(q, f, xyz1_stride, xyz2_stride, boxes9);
        MH_TRY(contacts_frame(K, &qf));
    }
    return contacts_end(K, nullptr);
}

}  // extern "C"
