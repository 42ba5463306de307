// hbonds.hip - hydrogen bonds of one frame or of a block of frames: the consumer of the two-set pair list at contact cutoffs.
// The definition is in molar_hip.h.  The pair list of a 0.35 nm donor-acceptor search is small (about five acceptors per donor),
// so it stays in HBM and the resident two-set search produces it unchanged; what is new comes behind it on the context's stream:
//
//   filter   one lane per list entry (p, q): the donor's hydrogens in turn, minimum-image vectors and the criteria in f64; a hit
//            is the key (position of H in the CSR) << 32 | q.  Keys are appended by ballot and mbcnt, one integer atomic per wave
//            and round of hydrogens, into a buffer sized by earlier frames: the counter keeps counting past the end, and a
//            frame that did not fit is filtered again into a grown buffer.  The order of the keys means nothing:
//   sort     radix sort of the keys (the CSR is donor-major, so key order IS (donor, hydrogen, acceptor) order) and the first
//            of every run of equal neighbours: the list's duplicates are gone;
//   measure  one lane per bond: the geometry once more, the triple and the three f64 columns, and the counts - donors by one
//            integer atomic per run of equal donors in the wave (the keys are donor-major), acceptors and group pairs one each;
//   table    (frames form) one sort of the block's keys carrying the entry number, the first of every run: the rows.  A run's
//            length is the occupancy (a frame's list is a set), and its members go through the permutation to bond_of_entry.
//
// Three 8-byte read-backs per frame: the pair count (inside the search), the keys, the bonds.
#include <algorithm>
#include <cmath>
#include <utility>
#include <vector>

#include "boxmath.hpp"
#include "common.hpp"
#include "stages.hpp"
#include "traj_block.hpp"

using namespace mh;

struct molar_hip_hbonds_state {
    DevBuf in_off, in_hidx, in_g1, in_g2;              // host inputs staged here
    DevBuf ctr;                                        // u64[4]: keys the filter found, bonds, table rows, a check's flag
    DevBuf keys, sorted;                               // one frame's keys as found and in order
    DevBuf ukeys, triples, dda, dha, ang;              // the result: bonds of the frame, or of the block's frames one after the other
    DevBuf acc;                                        // sums of a call whose count outputs are host memory [don | acc | map]
    DevBuf ent, bsorted, perm, tkeys, occ, boe, table;   // the block's table
    std::vector<uint64_t> frame_off;                   // the block's frames in the result
    uint64_t count = 0, unique = 0;
    uint64_t serial = 0;                               // blocks this context has finished (hbonds_block_view)
    int have = 0;                                      // 0: nothing, 1: a frame (molar_hip_hbonds_fill), 2: a block (_frames_fill)
};

namespace {

constexpr uint32_t HB_WG = 256;                        // lanes per workgroup of every kernel here
constexpr size_t HB_MIN_KEYS = 1024;                   // the key buffer of a fresh context
constexpr size_t HB_MAP_MAX = (size_t)1 << 24;
constexpr double HB_DEG = 57.29577951308232;           // 180 / pi

// what the filter and the measure kernels know about the frame and the criteria
struct HbFrame {
    const float *xyz;
    const uint64_t *idx1, *idx2;       // null: 0 .. n-1
    const uint64_t *hoff, *hidx;
    uint32_t n1;
    uint32_t use_box, pbc;
    int32_t kind;
    double angle_deg, max_ha;
    BoxD box;
};

struct HbCounts {
    unsigned long long *don, *acc, *map;
    const uint32_t *g1, *g2;
    uint32_t ng2;
};

struct HbGeo {
    double dda, dha, ang;
    bool bond;
};

__device__ __forceinline__ D3 hb_pos(const float *__restrict__ xyz, uint64_t a) {
    return D3{(double)xyz[3 * a], (double)xyz[3 * a + 1], (double)xyz[3 * a + 2]};
}

__device__ __forceinline__ D3 hb_vec(const HbFrame &F, D3 from, D3 to) {
    const D3 v = to - from;
    return F.use_box ? shortest_vector(F.box, v, F.pbc) : v;
}

// criteria 3 and 4 of the definition, and the columns
__device__ __forceinline__ HbGeo hb_geometry(const HbFrame &F, D3 d, D3 h, D3 a) {
    const D3 da = hb_vec(F, d, a), dh = hb_vec(F, d, h), ha = hb_vec(F, h, a);
    const bool dha = F.kind == MOLAR_HIP_HBOND_DHA_MIN;
    const D3 u = dha ? D3{-dh.x, -dh.y, -dh.z} : dh, v = dha ? ha : da;
    const D3 cr = D3{u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x};
    const double dot = (u.x * v.x + u.y * v.y) + u.z * v.z;
    HbGeo G;
    G.ang = atan2(sqrt(norm2(cr)), dot) * HB_DEG;
    G.dda = sqrt(norm2(da));
    G.dha = sqrt(norm2(ha));
    const bool arms = norm2(dh) > 0.0 && norm2(ha) > 0.0;
    const bool angle = dha ? G.ang >= F.angle_deg : G.ang <= F.angle_deg;
    G.bond = arms && angle && (!(F.max_ha > 0.0) || G.dha <= F.max_ha);
    return G;
}

__device__ __forceinline__ uint32_t hb_lane_rank(unsigned long long mask) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// One lane per entry of the pair list.  No lane leaves before the loop ends: the ballots are taken with the whole wave present.
__global__ void __launch_bounds__(HB_WG) hb_filter_kernel(HbFrame F, const uint2 *__restrict__ pairs, unsigned long long npairs,
                                                          unsigned long long *__restrict__ keys, unsigned long long cap,
                                                          unsigned long long *__restrict__ counter) {
    const unsigned long long e = (unsigned long long)blockIdx.x * HB_WG + threadIdx.x;
    bool live = e < npairs;
    uint32_t q = 0;
    unsigned long long h = 0, hend = 0;
    D3 d{0.0, 0.0, 0.0}, a{0.0, 0.0, 0.0};
    if (live) {
        const uint2 pr = pairs[e];
        q = pr.y;
        const uint64_t D = F.idx1 ? F.idx1[pr.x] : (uint64_t)pr.x, A = F.idx2 ? F.idx2[q] : (uint64_t)q;
        if (D == A) {
            live = false;
        } else {
            h = F.hoff[pr.x];
            hend = F.hoff[pr.x + 1];
            d = hb_pos(F.xyz, D);
            a = hb_pos(F.xyz, A);
        }
    }
    for (;;) {
        const bool more = live && h < hend;
        if (__builtin_amdgcn_ballot_w64(more) == 0ull) break;
        bool hit = false;
        if (more) hit = hb_geometry(F, d, hb_pos(F.xyz, F.hidx[h]), a).bond;
        const unsigned long long mask = __builtin_amdgcn_ballot_w64(hit);
        if (mask != 0ull) {
            const uint32_t rank = hb_lane_rank(mask);
            const int leader = __builtin_ctzll(mask);
            unsigned long long base = 0ull;
            if ((int)(threadIdx.x & 63u) == leader) base = atomicAdd(counter, (unsigned long long)__builtin_popcountll(mask));
            base = __shfl(base, leader);
            if (hit && base + rank < cap) keys[base + rank] = (h << 32) | q;
        }
        ++h;
    }
}

// the donor whose hydrogens include position h of the CSR: the last p with hoff[p] <= h (donors without hydrogens are passed over)
__device__ __forceinline__ uint32_t hb_donor_of(const uint64_t *__restrict__ hoff, uint32_t n1, uint64_t h) {
    uint32_t lo = 0, hi = n1;          // hoff[lo] <= h < hoff[hi]
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (hoff[mid] <= h) lo = mid;
        else hi = mid;
    }
    return lo;
}

// One lane per bond, keys in order.  triples / the columns / the counts: each written when asked for; with the columns null no
// coordinate is read (the rows of the block's table).
__global__ void __launch_bounds__(HB_WG) hb_measure_kernel(HbFrame F, const unsigned long long *__restrict__ ukeys, unsigned long long n,
                                                           uint32_t *__restrict__ triples, double *__restrict__ dda,
                                                           double *__restrict__ dha, double *__restrict__ ang, HbCounts K) {
    const unsigned long long e = (unsigned long long)blockIdx.x * HB_WG + threadIdx.x;
    const bool live = e < n;
    uint32_t p = 0, q = 0;
    if (live) {
        const unsigned long long key = ukeys[e];
        const uint64_t h = key >> 32;
        q = (uint32_t)key;
        p = hb_donor_of(F.hoff, F.n1, h);
        const uint64_t D = F.idx1 ? F.idx1[p] : (uint64_t)p, A = F.idx2 ? F.idx2[q] : (uint64_t)q, H = F.hidx[h];
        if (triples) {
            triples[3 * e] = (uint32_t)D;
            triples[3 * e + 1] = (uint32_t)H;
            triples[3 * e + 2] = (uint32_t)A;
        }
        if (dda) {
            const HbGeo G = hb_geometry(F, hb_pos(F.xyz, D), hb_pos(F.xyz, H), hb_pos(F.xyz, A));
            dda[e] = G.dda;
            dha[e] = G.dha;
            ang[e] = G.ang;
        }
    }
    if (K.don) {
        // the live lanes of a wave are its first ones and their donors do not decrease: a run of equal donors adds once
        const uint32_t lane = threadIdx.x & 63u;
        const uint32_t before = __shfl_up(p, 1);
        const bool head = live && (lane == 0u || before != p);
        const unsigned long long heads = __builtin_amdgcn_ballot_w64(head), lives = __builtin_amdgcn_ballot_w64(live);
        if (head) {
            const unsigned long long later = lane == 63u ? 0ull : heads >> (lane + 1u);
            const uint32_t next = later ? lane + 1u + (uint32_t)__builtin_ctzll(later) : (uint32_t)__builtin_popcountll(lives);
            atomicAdd(&K.don[p], (unsigned long long)(next - lane));
        }
    }
    if (live && K.acc) atomicAdd(&K.acc[q], 1ull);
    if (live && K.map) atomicAdd(&K.map[(size_t)K.g1[p] * K.ng2 + K.g2[q]], 1ull);
}

// flag = 1 when a value is not below the limit (h_idx against natoms, labels against ngroups: inputs in device memory)
template <class T>
__global__ void __launch_bounds__(HB_WG) hb_check_below_kernel(const T *__restrict__ v, size_t n, T limit, unsigned long long *__restrict__ flag) {
    for (size_t i = (size_t)blockIdx.x * HB_WG + threadIdx.x; i < n; i += (size_t)gridDim.x * HB_WG)
        if (v[i] >= limit) *flag = 1ull;
}

__global__ void __launch_bounds__(HB_WG) hb_add_kernel(unsigned long long *__restrict__ dst, const unsigned long long *__restrict__ src, size_t n) {
    for (size_t i = (size_t)blockIdx.x * HB_WG + threadIdx.x; i < n; i += (size_t)gridDim.x * HB_WG) dst[i] += src[i];
}

__global__ void __launch_bounds__(HB_WG) hb_iota_kernel(uint32_t *__restrict__ v, uint32_t n) {
    const uint32_t i = blockIdx.x * HB_WG + threadIdx.x;
    if (i < n) v[i] = i;
}

// One lane per row of the table: the row's run in the sorted keys of the block is found by bisection; its length is the
// occupancy, and its members, through the permutation of the sort, learn their row.
__global__ void __launch_bounds__(HB_WG) hb_rows_kernel(const unsigned long long *__restrict__ tkeys, uint32_t rows,
                                                        const unsigned long long *__restrict__ sorted, const uint32_t *__restrict__ perm,
                                                        uint32_t entries, uint32_t *__restrict__ occ, uint32_t *__restrict__ boe) {
    const uint32_t r = blockIdx.x * HB_WG + threadIdx.x;
    if (r >= rows) return;
    const unsigned long long key = tkeys[r];
    uint32_t lo = 0, hi = entries;          // the first entry that is not below the key
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (sorted[mid] < key) lo = mid + 1u;
        else hi = mid;
    }
    uint32_t m = 0;
    for (uint32_t k = lo; k < entries && sorted[k] == key; ++k, ++m) boe[perm[k]] = r;
    occ[r] = m;
}

inline unsigned blocks_of(size_t n) { return (unsigned)((n + HB_WG - 1) / HB_WG); }

// room for `need` bytes with the first `used` bytes kept
int grow_keep(molar_hip_ctx *c, DevBuf &b, size_t used, size_t need) {
    if (need <= b.cap) return 0;
    DevBuf g;
    MH_TRY(g.reserve(std::max(need, 2 * b.cap)));
    if (used) {
        MH_HIP(hipMemcpyAsync(g.p, b.p, used, hipMemcpyDeviceToDevice, c->stream));
        MH_HIP(hipStreamSynchronize(c->stream));
    }
    b = std::move(g);
    return 0;
}

// values of host or device memory below a limit: walked here, or by a kernel and one read-back; then readable by kernels
template <class T>
int checked_to_device(molar_hip_ctx *c, molar_hip_hbonds_state &Z, const T *v, size_t n, T limit, DevBuf &stage, const T **out, const char *who,
                      const char *what) {
    *out = nullptr;
    if (n == 0) return 0;
    if (!v) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: %s: null pointer", who, what);
    if (!is_device_ptr(v)) {
        for (size_t i = 0; i < n; ++i)
            if (v[i] >= limit)
                return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: %s[%zu] = %llu is not below %llu", who, what, i, (unsigned long long)v[i], (unsigned long long)limit);
        return to_device(c, v, n, stage, out);
    }
    unsigned long long *flag = Z.ctr.as<unsigned long long>() + 3;
    MH_HIP(hipMemsetAsync(flag, 0, 8, c->stream));
    hipLaunchKernelGGL(hb_check_below_kernel<T>, dim3(std::min(blocks_of(n), 1024u)), dim3(HB_WG), 0, c->stream, v, n, limit, flag);
    MH_HIP(hipGetLastError());
    unsigned long long bad = 0;
    MH_TRY(read_back(c, &bad, flag, 8));
    if (bad) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: an entry of %s is not below %llu", who, what, (unsigned long long)limit);
    *out = v;
    return 0;
}

// A request once it has been judged: sizes, the criteria, inputs readable by kernels, where the counts go.
struct HbCall {
    molar_hip_ctx *c = nullptr;
    molar_hip_hbonds_state *Z = nullptr;
    const char *who = "";
    size_t natoms = 0, n1 = 0, n2 = 0, nh = 0, nmap = 0;
    HbFrame F{};
    HbCounts K{};
    uint64_t *h_don = nullptr, *h_acc = nullptr, *h_map = nullptr;      // the caller's HOST count outputs (added at the end)
    uint64_t *d_don = nullptr, *d_acc = nullptr, *d_map = nullptr;      // a block's DEVICE count outputs (added at the end as well)
    bool want_cols = true;
};

int hb_begin(HbCall &X, molar_hip_ctx *c, const char *who, const molar_hip_search_desc *q, const uint64_t *h_offsets, const uint64_t *h_idx, size_t nh,
             int32_t angle_kind, double angle_deg, double max_ha, const molar_hip_contact_groups *groups, uint64_t *don, uint64_t *acc,
             uint64_t *map, bool block = false) {
    if (!c || !q) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: null argument", who);
    if (q->kind != MOLAR_HIP_SEARCH_DOUBLE)
        return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: donors and acceptors are the two sets of a DOUBLE search (got kind %d)", who, q->kind);
    if (!q->xyz1) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: xyz pointer is null", who);
    if (q->xyz2 != q->xyz1 || q->natoms2 != q->natoms1)
        return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: donors, hydrogens and acceptors are atoms of one frame array (xyz2 == xyz1, natoms2 == natoms1)", who);
    if (angle_kind != MOLAR_HIP_HBOND_DHA_MIN && angle_kind != MOLAR_HIP_HBOND_HDA_MAX)
        return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: angle kind %d is neither DHA_MIN nor HDA_MAX", who, angle_kind);
    if (!(angle_deg >= 0.0 && angle_deg <= 180.0)) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: angle_deg = %g is outside [0, 180]", who, angle_deg);
    if (!(max_ha >= 0.0)) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: max_ha = %g is negative", who, max_ha);
    X.c = c;
    X.who = who;
    X.natoms = q->natoms1;
    X.n1 = q->idx1 ? q->n1 : q->natoms1;
    X.n2 = q->idx2 ? q->n2 : q->natoms2;
    X.nh = nh;
    if (nh >= 0xFFFFFFFFull || X.n2 >= 0xFFFFFFFFull || X.n1 >= 0xFFFFFFFFull || X.natoms >= 0xFFFFFFFFull)
        return fail(MOLAR_HIP_ERR_TOO_LARGE, "%s: 2^32 hydrogen entries or atoms of a selection, or more", who);
    if (!h_offsets) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: h_offsets is null", who);
    MH_HIP(hipSetDevice(c->device));
    // the offsets are judged here
    std::vector<uint64_t> off_host;
    const uint64_t *off = h_offsets;
    if (is_device_ptr(h_offsets)) {
        off_host.resize(X.n1 + 1);
        MH_HIP(hipMemcpy(off_host.data(), h_offsets, (X.n1 + 1) * 8, hipMemcpyDeviceToHost));
        off = off_host.data();
    }
    if (off[0] != 0 || off[X.n1] != nh)
        return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: h_offsets run from %llu to %llu, not from 0 to nh = %zu", who, (unsigned long long)off[0], (unsigned long long)off[X.n1], nh);
    for (size_t p = 0; p < X.n1; ++p)
        if (off[p + 1] < off[p]) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: h_offsets decrease at donor %zu", who, p);
    size_t G1 = 0, G2 = 0;
    if (map) {
        if (!groups || !groups->group1 || !groups->group2) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: a map needs group labels", who);
        G1 = groups->ngroups1;
        G2 = groups->ngroups2;
        if (G1 > HB_MAP_MAX || G2 > HB_MAP_MAX || G1 * G2 > HB_MAP_MAX)
            return fail(MOLAR_HIP_ERR_TOO_LARGE, "%s: the map is dense, ngroups1 * ngroups2 may be 2^24 at most (got %zu x %zu)", who, G1, G2);
        if ((G1 == 0 && X.n1 != 0) || (G2 == 0 && X.n2 != 0)) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: a label is not below ngroups = 0", who);
    }
    X.nmap = G1 * G2;
    // (the same text as molar_hip_search_resident_planes: nothing of the context may be in flight while its setting is borrowed)
    if (c->tickets[0].pending || c->tickets[1].pending) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: pipelined searches are in flight", who);
    molar_hip_hbonds_state &Z = state_of(c->hbonds);
    X.Z = &Z;
    Z.have = 0;
    MH_TRY(Z.ctr.reserve(32));
    MH_TRY(checked_to_device<uint64_t>(c, Z, h_idx, nh, (uint64_t)X.natoms, Z.in_hidx, &X.F.hidx, who, "h_idx"));
    if (map && X.nmap) {
        MH_TRY(checked_to_device<uint32_t>(c, Z, groups->group1, X.n1, (uint32_t)G1, Z.in_g1, &X.K.g1, who, "group1"));
        MH_TRY(checked_to_device<uint32_t>(c, Z, groups->group2, X.n2, (uint32_t)G2, Z.in_g2, &X.K.g2, who, "group2"));
        X.K.ng2 = (uint32_t)G2;
    }
    MH_TRY(to_device(c, h_offsets, X.n1 + 1, Z.in_off, &X.F.hoff));
    X.F.n1 = (uint32_t)X.n1;
    X.F.kind = angle_kind;
    X.F.angle_deg = angle_deg;
    X.F.max_ha = max_ha;
    // ---- where the counts go: host outputs through zeroed sums that are added at the end.  Device outputs of one frame as they
    // are (nothing is refused behind its measure kernel); those of a BLOCK through the sums as well, because a later frame may
    // still be refused (too many entries, no memory) and a refused request adds nothing
    const bool sd = don && (block || !is_device_ptr(don)), sa = acc && (block || !is_device_ptr(acc)),
               sm = map && X.nmap && (block || !is_device_ptr(map));
    const bool hd = sd && !is_device_ptr(don), ha = sa && !is_device_ptr(acc), hm = sm && !is_device_ptr(map);
    const size_t words = (sd ? X.n1 : 0) + (sa ? X.n2 : 0) + (sm ? X.nmap : 0);
    X.K.don = reinterpret_cast<unsigned long long *>(don);
    X.K.acc = reinterpret_cast<unsigned long long *>(acc);
    X.K.map = X.nmap ? reinterpret_cast<unsigned long long *>(map) : nullptr;
    if (words) {
        MH_TRY(Z.acc.reserve(words * 8));
        MH_HIP(hipMemsetAsync(Z.acc.p, 0, words * 8, c->stream));
        unsigned long long *w = Z.acc.as<unsigned long long>();
        if (sd) { (hd ? X.h_don : X.d_don) = don; X.K.don = w; w += X.n1; }
        if (sa) { (ha ? X.h_acc : X.d_acc) = acc; X.K.acc = w; w += X.n2; }
        if (sm) { (hm ? X.h_map : X.d_map) = map; X.K.map = w; w += X.nmap; }
    }
    return 0;
}

// One frame: the search, then filter, sort and measure.  The frame's bonds go behind the first `base` entries of the result.
int hb_frame(HbCall &X, const molar_hip_search_desc *q, uint64_t base, uint64_t *nbonds) {
    molar_hip_ctx *c = X.c;
    molar_hip_hbonds_state &Z = *X.Z;
    *nbonds = 0;
    if (X.n1 == 0 || X.n2 == 0 || X.nh == 0) {
        c->have_search = false;
        return 0;
    }
    molar_hip_search_desc qq = *q;
    qq.ids_local = 1;                        // ids are positions in the selections
    HbFrame &F = X.F;
    F.use_box = (q->box9 != nullptr && (q->pbc & 7u) != 0u) ? 1u : 0u;
    F.pbc = q->pbc & 7u;
    if (F.use_box) {
        double m9[9];
        for (int k = 0; k < 9; ++k) m9[k] = (double)q->box9[k];
        MH_TRY(box64_from_matrix(m9, &F.box));
    }
    // the (i, j) plane alone, and the caller's setting back in place whatever the search says
    const bool planes = c->resident_no_dist;
    c->resident_no_dist = true;
    uint64_t npairs = 0;
    const uint32_t *pairs = nullptr;
    const int rc = molar_hip_search_resident(c, &qq, &npairs, &pairs, nullptr);
    c->resident_no_dist = planes;
    MH_TRY(rc);
    // (taken behind EVERY search, a frame without a pair included: the table's rows are decoded through them after the last frame)
    F.xyz = c->cur.set[0].d_xyz;
    F.idx1 = c->cur.set[0].d_idx;
    F.idx2 = c->cur.set[1].d_idx;
    if (npairs == 0) return 0;
    if (npairs >= ((unsigned long long)0x7FFFFFFF) * HB_WG) return fail(MOLAR_HIP_ERR_TOO_LARGE, "%s: %llu list entries", X.who, (unsigned long long)npairs);

    unsigned long long *ctr = Z.ctr.as<unsigned long long>();
    if (Z.keys.cap < HB_MIN_KEYS * 8) MH_TRY(Z.keys.reserve(HB_MIN_KEYS * 8));
    unsigned long long nkeys = 0;
    for (int pass = 0; pass < 2; ++pass) {
        const unsigned long long cap = Z.keys.cap / 8;
        MH_HIP(hipMemsetAsync(ctr, 0, 16, c->stream));
        hipLaunchKernelGGL(hb_filter_kernel, dim3(blocks_of(npairs)), dim3(HB_WG), 0, c->stream, F, reinterpret_cast<const uint2 *>(pairs),
                           (unsigned long long)npairs, Z.keys.as<unsigned long long>(), cap, ctr);
        MH_HIP(hipGetLastError());
        MH_TRY(read_back(c, &nkeys, ctr, 8));
        if (nkeys <= cap) break;
        MH_TRY(Z.keys.reserve((size_t)nkeys * 8));         // too small (a first frame): once more, into room for all of them
    }
    if (nkeys == 0) return 0;
    if (base + nkeys >= 0x7FFFFFFFull) return fail(MOLAR_HIP_ERR_TOO_LARGE, "%s: 2^31 - 1 entries or more", X.who);
    MH_TRY(Z.sorted.reserve((size_t)nkeys * 8));
    int end_bit = 33;
    while (end_bit < 64 && (X.nh - 1) >> (end_bit - 32)) ++end_bit;
    MH_TRY(device_sort_keys_u64(c->stream, c->sort_tmp, Z.keys.as<uint64_t>(), Z.sorted.as<uint64_t>(), (size_t)nkeys, end_bit));
    MH_TRY(grow_keep(c, Z.ukeys, (size_t)base * 8, (size_t)(base + nkeys) * 8));
    MH_TRY(device_unique_u64(c->stream, c->sort_tmp, Z.sorted.as<uint64_t>(), Z.ukeys.as<uint64_t>() + base, ctr + 1, (size_t)nkeys));
    unsigned long long nu = 0;
    MH_TRY(read_back(c, &nu, ctr + 1, 8));
    const size_t tot = (size_t)(base + nu);
    MH_TRY(grow_keep(c, Z.triples, (size_t)base * 12, tot * 12));
    if (X.want_cols) {
        MH_TRY(grow_keep(c, Z.dda, (size_t)base * 8, tot * 8));
        MH_TRY(grow_keep(c, Z.dha, (size_t)base * 8, tot * 8));
        MH_TRY(grow_keep(c, Z.ang, (size_t)base * 8, tot * 8));
    }
    hipLaunchKernelGGL(hb_measure_kernel, dim3(blocks_of(nu)), dim3(HB_WG), 0, c->stream, F, Z.ukeys.as<unsigned long long>() + base, nu,
                       Z.triples.as<uint32_t>() + 3 * base, X.want_cols ? Z.dda.as<double>() + base : nullptr,
                       X.want_cols ? Z.dha.as<double>() + base : nullptr, X.want_cols ? Z.ang.as<double>() + base : nullptr, X.K);
    MH_HIP(hipGetLastError());
    *nbonds = nu;
    return 0;
}

// the sums added to the outputs they stand for; the stream has nothing left to do when this returns
int hb_end(HbCall &X) {
    molar_hip_ctx *c = X.c;
    auto add_device = [&](uint64_t *dst, const unsigned long long *src, size_t n) -> int {
        if (!dst || n == 0) return 0;
        hipLaunchKernelGGL(hb_add_kernel, dim3(std::min(blocks_of(n), 2048u)), dim3(HB_WG), 0, c->stream, reinterpret_cast<unsigned long long *>(dst), src, n);
        MH_HIP(hipGetLastError());
        return 0;
    };
    MH_TRY(add_device(X.d_don, X.K.don, X.n1));
    MH_TRY(add_device(X.d_acc, X.K.acc, X.n2));
    MH_TRY(add_device(X.d_map, X.K.map, X.nmap));
    auto add_back = [&](uint64_t *dst, const unsigned long long *src, size_t n) -> int {
        if (!dst || n == 0) return 0;
        std::vector<unsigned long long> h(n);
        MH_TRY(read_back(c, h.data(), src, n * 8));
        for (size_t i = 0; i < n; ++i) dst[i] += h[i];
        return 0;
    };
    MH_TRY(add_back(X.h_don, X.K.don, X.n1));
    MH_TRY(add_back(X.h_acc, X.K.acc, X.n2));
    MH_TRY(add_back(X.h_map, X.K.map, X.nmap));
    MH_HIP(hipStreamSynchronize(c->stream));
    return 0;
}

// `bytes` of the result to host or device memory (null: nothing)
int hb_put(molar_hip_ctx *c, void *dst, const void *src, size_t bytes) {
    if (!dst || bytes == 0) return 0;
    MH_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDefault, c->stream));
    return 0;
}

// The table of a block of `E` entries: rows, occupancy, the row of every entry.
int hb_table(HbCall &X, uint64_t E, uint64_t *rows) {
    molar_hip_ctx *c = X.c;
    molar_hip_hbonds_state &Z = *X.Z;
    *rows = 0;
    if (E == 0) return 0;
    unsigned long long *ctr = Z.ctr.as<unsigned long long>();
    MH_TRY(Z.ent.reserve(E * 4));
    MH_TRY(Z.perm.reserve(E * 4));
    MH_TRY(Z.bsorted.reserve(E * 8));
    MH_TRY(Z.tkeys.reserve(E * 8));
    MH_TRY(Z.occ.reserve(E * 4));
    MH_TRY(Z.boe.reserve(E * 4));
    hipLaunchKernelGGL(hb_iota_kernel, dim3(blocks_of(E)), dim3(HB_WG), 0, c->stream, Z.ent.as<uint32_t>(), (uint32_t)E);
    MH_HIP(hipGetLastError());
    int end_bit = 33;
    while (end_bit < 64 && (X.nh - 1) >> (end_bit - 32)) ++end_bit;
    MH_TRY(device_sort_pairs_u64_u32(c->stream, c->sort_tmp, Z.ukeys.as<uint64_t>(), Z.bsorted.as<uint64_t>(), Z.ent.as<uint32_t>(),
                                     Z.perm.as<uint32_t>(), (size_t)E, end_bit));
    MH_TRY(device_unique_u64(c->stream, c->sort_tmp, Z.bsorted.as<uint64_t>(), Z.tkeys.as<uint64_t>(), ctr + 2, (size_t)E));
    unsigned long long R = 0;
    MH_TRY(read_back(c, &R, ctr + 2, 8));
    hipLaunchKernelGGL(hb_rows_kernel, dim3(blocks_of(R)), dim3(HB_WG), 0, c->stream, Z.tkeys.as<unsigned long long>(), (uint32_t)R,
                       Z.bsorted.as<unsigned long long>(), Z.perm.as<uint32_t>(), (uint32_t)E, Z.occ.as<uint32_t>(), Z.boe.as<uint32_t>());
    MH_HIP(hipGetLastError());
    MH_TRY(Z.table.reserve((size_t)R * 12));
    hipLaunchKernelGGL(hb_measure_kernel, dim3(blocks_of(R)), dim3(HB_WG), 0, c->stream, X.F, Z.tkeys.as<unsigned long long>(), R,
                       Z.table.as<uint32_t>(), (double *)nullptr, (double *)nullptr, (double *)nullptr, HbCounts{});
    MH_HIP(hipGetLastError());
    *rows = R;
    return 0;
}

}  // namespace

namespace mh {
void hbonds_release(molar_hip_ctx *c) {
    release_state(c->hbonds);
}

bool hbonds_block_view(const molar_hip_ctx *c, HbondsBlockView *out) {
    if (!c->hbonds || c->hbonds->have != 2) return false;
    const molar_hip_hbonds_state &Z = *c->hbonds;
    *out = HbondsBlockView{Z.frame_off.data(), Z.frame_off.size() - 1, Z.boe.as<uint32_t>(), (size_t)Z.unique, (size_t)Z.count, Z.serial};
    return true;
}
}  // namespace mh

extern "C" {

int molar_hip_hbonds_counts(molar_hip_ctx *c, const molar_hip_search_desc *q, const uint64_t *h_offsets, const uint64_t *h_idx, size_t nh,
                            int32_t angle_kind, double angle_deg, double max_ha, const molar_hip_contact_groups *groups, uint64_t *don_count,
                            uint64_t *acc_count, uint64_t *map, uint64_t *out_count) {
    HbCall X;
    MH_TRY(hb_begin(X, c, "hbonds", q, h_offsets, h_idx, nh, angle_kind, angle_deg, max_ha, groups, don_count, acc_count, map));
    uint64_t n = 0;
    MH_TRY(hb_frame(X, q, 0, &n));
    MH_TRY(hb_end(X));
    X.Z->count = n;
    X.Z->have = 1;
    if (out_count) *out_count = n;
    return MOLAR_HIP_OK;
}

int molar_hip_hbonds_count(molar_hip_ctx *c, const molar_hip_search_desc *q, const uint64_t *h_offsets, const uint64_t *h_idx, size_t nh,
                           int32_t angle_kind, double angle_deg, double max_ha, uint64_t *out_count) {
    return molar_hip_hbonds_counts(c, q, h_offsets, h_idx, nh, angle_kind, angle_deg, max_ha, nullptr, nullptr, nullptr, nullptr, out_count);
}

int molar_hip_hbonds_fill(molar_hip_ctx *c, uint32_t *triples, double *dist_da, double *dist_ha, double *angle_deg) {
    MH_CTX(c);
    if (!c->hbonds || c->hbonds->have != 1) return fail(MOLAR_HIP_ERR_NO_SEARCH, "hbonds_fill: no hydrogen bonds of a frame are cached (count first)");
    const molar_hip_hbonds_state &Z = *c->hbonds;
    const size_t n = (size_t)Z.count;
    MH_TRY(hb_put(c, triples, Z.triples.p, n * 12));
    MH_TRY(hb_put(c, dist_da, Z.dda.p, n * 8));
    MH_TRY(hb_put(c, dist_ha, Z.dha.p, n * 8));
    MH_TRY(hb_put(c, angle_deg, Z.ang.p, n * 8));
    MH_HIP(hipStreamSynchronize(c->stream));
    return MOLAR_HIP_OK;
}

int molar_hip_hbonds_frames(molar_hip_ctx *c, const molar_hip_search_desc *q, const uint64_t *h_offsets, const uint64_t *h_idx, size_t nh,
                            int32_t angle_kind, double angle_deg, double max_ha, size_t nframes, size_t xyz_stride, const float *boxes9,
                            const molar_hip_contact_groups *groups, uint64_t *per_frame, uint64_t *don_count, uint64_t *acc_count, uint64_t *map,
                            uint64_t *out_total, uint64_t *out_unique) {
    HbCall X;
    MH_TRY(hb_begin(X, c, "hbonds_frames", q, h_offsets, h_idx, nh, angle_kind, angle_deg, max_ha, groups, don_count, acc_count, map, /*block=*/true));
    MH_TRY(check_stride("hbonds_frames", "the frame stride", nframes, xyz_stride, q->natoms1));
    molar_hip_hbonds_state &Z = *X.Z;
    Z.frame_off.assign(nframes + 1, 0);
    std::vector<uint64_t> per(nframes, 0);
    for (size_t f = 0; f < nframes; ++f) {
        molar_hip_search_desc qf = *q;
        qf.xyz1 = qf.xyz2 = q->xyz1 + f * xyz_stride;
        if (boxes9) qf.box9 = boxes9 + 9 * f;
        MH_TRY(hb_frame(X, &qf, Z.frame_off[f], &per[f]));
        Z.frame_off[f + 1] = Z.frame_off[f] + per[f];
    }
    const uint64_t E = Z.frame_off[nframes];
    uint64_t rows = 0;
    MH_TRY(hb_table(X, E, &rows));
    MH_TRY(hb_end(X));
    MH_TRY(hb_put(c, per_frame, per.data(), nframes * 8));
    MH_HIP(hipStreamSynchronize(c->stream));
    Z.count = E;
    Z.unique = rows;
    Z.have = 2;
    ++Z.serial;
    if (out_total) *out_total = E;
    if (out_unique) *out_unique = rows;
    return MOLAR_HIP_OK;
}

int molar_hip_hbonds_frames_fill(molar_hip_ctx *c, uint64_t *frame_offsets, uint32_t *triples, double *dist_da, double *dist_ha, double *angle_deg,
                                 uint32_t *bond_of_entry, uint32_t *table, uint32_t *occupancy) {
    MH_CTX(c);
    if (!c->hbonds || c->hbonds->have != 2)
        return fail(MOLAR_HIP_ERR_NO_SEARCH, "hbonds_frames_fill: no hydrogen bonds of a block are cached (molar_hip_hbonds_frames first)");
    const molar_hip_hbonds_state &Z = *c->hbonds;
    const size_t n = (size_t)Z.count, rows = (size_t)Z.unique;
    MH_TRY(hb_put(c, frame_offsets, Z.frame_off.data(), Z.frame_off.size() * 8));
    MH_TRY(hb_put(c, triples, Z.triples.p, n * 12));
    MH_TRY(hb_put(c, dist_da, Z.dda.p, n * 8));
    MH_TRY(hb_put(c, dist_ha, Z.dha.p, n * 8));
    MH_TRY(hb_put(c, angle_deg, Z.ang.p, n * 8));
    MH_TRY(hb_put(c, bond_of_entry, Z.boe.p, n * 4));
    MH_TRY(hb_put(c, table, Z.table.p, rows * 12));
    MH_TRY(hb_put(c, occupancy, Z.occ.p, rows * 4));
    MH_HIP(hipStreamSynchronize(c->stream));
    return MOLAR_HIP_OK;
}

}  // extern "C"
