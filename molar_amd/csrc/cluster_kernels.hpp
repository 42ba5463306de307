// cluster_kernels.hpp - connected components of the contact graph (molar_hip_search_clusters): the third consumer of the slot
// records of the REGULAR plan, beside the count / fill passes and contact_kernel.  No pair is written: where the contact kernel
// adds one per hit, cluster_kernel unites the two ends of the hit in a lock-free union-find over the PARTICLES (the atoms of
// the selection, or their groups).  Included by contacts.hip (ClusterArgs, the launchers' declarations) and by pair_k12.hip, which
// instantiates the kernels.
//
// The forest.  parent[P], one word per particle, identity at the start (cluster_init_kernel).
//   Invariant: parent[x] <= x, and a word only ever falls.  So every path x, parent[x], parent[parent[x]] ... strictly falls and
//   ends at a root (parent[r] == r), the root of a finished component is its SMALLEST particle, and whatever value was once read
//   on the path above x stays a member of x's component for good.
//   find(x)      follows parent to a root; a walk of two or more steps shortens x's path with atomicMin(&parent[x], root).
//   unite(u, v)  finds both roots; equal: done.  Else the larger root is hooked under the smaller one by
//                atomicCAS(&parent[hi], hi, lo).  A lost race (hi is no root any more) returns hi's new parent, which is < hi:
//                the loop goes on from (that value, lo).  max(u, v) strictly falls from one round to the next, so every loop
//                ends on its own: no lock, no wait for another wave.
// Visibility.  Every access to parent inside cluster_kernel is an agent-scope atomic on the vector path: relaxed atomic loads
//   (global_load sc1: never served by this CU's L1), CAS and atomicMin (performed at the memory side, one order per word for
//   all eight XCDs).  What decides a union is the CAS alone: it succeeds only while parent[hi] == hi really holds.  A load that
//   returns an older value of a word is harmless - an older value is a LARGER member of the same component (see the invariant),
//   so the walk takes more steps, or the CAS fails and hands back the current value; it never joins what does not belong
//   together and never skips a union that is needed (two particles are skipped only when two walks met in one word).  The
//   kernels behind it (flatten, ranks, labels, sizes) are separate launches on the same stream and read parent with plain loads.
// What stays in the wave.  A hit between atoms of one particle is dropped.  Lane r keeps the smallest member seen so far of
//   row r's component, every lane the same for its own atom across the rows of a chunk; a hit whose two cached members are
//   equal issues nothing.  In a dense frame (one giant component) almost every hit ends at that comparison.
// Numbering.  Components are numbered in the order of their smallest particle: the rank of a root among the roots
//   (cluster_flatten_kernel, an exclusive scan of the root flags, cluster_label_kernel).  Sizes are integer atomic adds, the
//   members come from one stable sort of (component, particle): the same call gives the same bits whatever order the unions
//   happened in.
#pragma once

#include "contact_kernels.hpp"

namespace mh {
namespace pairk {

struct ClusterArgs {
    const uint32_t *g;               // label by selection position (NULL: every atom is a particle)
    uint32_t *parent;                // [P]
    unsigned long long *stats;       // instrumented instance: [hits, hits that reach the forest, CAS, atomicMin] added into
};

__device__ __forceinline__ uint32_t cluster_load(uint32_t *parent, uint32_t x) {
    return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <bool STATS>
__device__ __forceinline__ uint32_t cluster_find(uint32_t *parent, uint32_t x, uint32_t &nmin) {
    uint32_t r = x, steps = 0u;
    for (;;) {
        const uint32_t p = cluster_load(parent, r);
        if (p == r) break;
        r = p;                       // p < r: the walk falls
        ++steps;
    }
    if (steps >= 2u) {
        __hip_atomic_fetch_min(parent + x, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (STATS) ++nmin;
    }
    return r;
}

// unites the components of u and v; returns a member of the united component that was its root when the call saw it
template <bool STATS>
__device__ __forceinline__ uint32_t cluster_unite(uint32_t *parent, uint32_t u, uint32_t v, uint32_t &ncas, uint32_t &nmin) {
    for (;;) {
        u = cluster_find<STATS>(parent, u, nmin);
        v = cluster_find<STATS>(parent, v, nmin);
        if (u == v) return u;
        const uint32_t hi = u > v ? u : v, lo = u > v ? v : u;
        uint32_t seen = hi;
        __hip_atomic_compare_exchange_strong(parent + hi, &seen, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (STATS) ++ncas;
        if (seen == hi) return lo;
        u = seen;                    // hi was hooked by someone else meanwhile: seen < hi
        v = lo;
    }
}

__device__ __forceinline__ uint32_t cluster_wave_min(uint32_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)v, off, 64);
        v = o < v ? o : v;
    }
    return v;
}

__device__ __forceinline__ unsigned long long cluster_wave_sum(uint32_t v) {
    unsigned long long s = v;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    return s;
}

constexpr int CLUSTER_WAVES = CONTACT_WAVES;      // waves per workgroup; every wave walks its own slots

// the row loop of contact_kernel<SINGLE> (slot decode and hit decision are its own: contact_slot, contact_hit)
template <bool STATS>
__global__ void __launch_bounds__(64 * CLUSTER_WAVES) cluster_kernel(const SearchParams *__restrict__ Pp, const SlotDesc *__restrict__ slot_desc,
                                                                     const uint32_t nslots, const ClusterArgs A) {
    const SearchParams &P = *Pp;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t w0 = blockIdx.x * CLUSTER_WAVES + wave, stride = gridDim.x * CLUSTER_WAVES;
    const bool grouped = A.g != nullptr;
    uint32_t nhit = 0u, nreach = 0u, ncas = 0u, nmin = 0u;

    for (uint32_t w = w0; w < nslots; w += stride) {
        const uint32_t slot = nslots - 1u - w;          // the heavy wrapped entries at the far edge of the plan start first
        ContactSlot S;
        if (!contact_slot(P, slot_desc, slot, S)) continue;
        const uint32_t i0 = S.i0, rows = S.rows, n2 = S.n2;
        const bool tri = S.tri;

        float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
        if (lane < rows) a = gload4(P.sa, S.a0 + i0 + lane);
        uint32_t pa = __float_as_uint(a.w);                       // lane r: the particle of row r ...
        if (grouped && lane < rows) pa = gload_u32(A.g, pa);
        uint32_t rroot = pa;                                      // ... and the smallest member of its component seen so far
        if (lane < rows) rroot = cluster_load(A.parent, pa);

        const uint32_t nchunks = (n2 + 63u) >> 6;
        for (uint32_t c = 0; c < nchunks; ++c) {
            if (tri && c * 64u + 63u <= i0) continue;             // same cell, j in i+1..n: the whole chunk has j <= i
            const uint32_t jj = c * 64u + lane;
            const bool valid = jj < n2;
            float4 b = make_float4(3.0e38f, 3.0e38f, 3.0e38f, 0.f);
            if (valid) b = gload4(P.sb, S.b0 + jj);
            const float sbx = b.x + S.Sx, sby = b.y + S.Sy, sbz = b.z + S.Sz;          // the image (approx entries; S == 0 otherwise)
            uint32_t pb = __float_as_uint(b.w);                   // the particle of the lane's atom
            if (grouped && valid) pb = gload_u32(A.g, pb);
            uint32_t croot = pb;                                  // the smallest member of its component seen so far
            if (valid) croot = cluster_load(A.parent, pb);
            for (uint32_t r = 0; r < rows; ++r) {
                const float px = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(a.x), r));
                const float py = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(a.y), r));
                const float pz = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(a.z), r));
                const bool hit = contact_hit(P, S, valid, b, sbx, sby, sbz, px, py, pz, jj, r);
                const uint32_t pr = (uint32_t)__builtin_amdgcn_readlane((int)pa, r);
                const uint32_t rr = (uint32_t)__builtin_amdgcn_readlane((int)rroot, r);
                const bool reach = hit && pb != pr && croot != rr;
                if (STATS) {
                    nhit += hit ? 1u : 0u;
                    nreach += reach ? 1u : 0u;
                }
                if (__builtin_amdgcn_ballot_w64(reach) == 0ull) continue;
                uint32_t m = 0xFFFFFFFFu;
                if (reach) {
                    m = cluster_unite<STATS>(A.parent, croot, rr, ncas, nmin);
                    croot = m;
                }
                m = cluster_wave_min(m);                          // every lane that united is in row r's component now
                if (lane == r) rroot = m;
            }
        }
    }
    if (STATS) {
        const unsigned long long h = cluster_wave_sum(nhit), q = cluster_wave_sum(nreach), s = cluster_wave_sum(ncas), t = cluster_wave_sum(nmin);
        if (lane == 0u) {
            atomicAdd(&A.stats[0], h);
            atomicAdd(&A.stats[1], q);
            atomicAdd(&A.stats[2], s);
            atomicAdd(&A.stats[3], t);
        }
    }
}

}  // namespace pairk

// defined in pair_k12.hip: the union kernel's launcher, and the small kernels around it, one launch per step
void launch_clusters(unsigned num_cus, hipStream_t stream, const pairk::SearchParams *dP, const pairk::SlotDesc *slot_desc, uint32_t nslots,
                     const pairk::ClusterArgs &A);
void launch_cluster_init(unsigned num_cus, hipStream_t stream, uint32_t *parent, uint32_t np);
void launch_cluster_flatten(unsigned num_cus, hipStream_t stream, const uint32_t *parent, uint32_t np, uint32_t *root, uint32_t *flag);
void launch_cluster_label(unsigned num_cus, hipStream_t stream, const uint32_t *root, const uint32_t *rank, uint32_t np, uint32_t *comp,
                          uint32_t *sizes, uint32_t *iota);
void launch_cluster_frame(unsigned num_cus, hipStream_t stream, const uint32_t *flag, const uint32_t *rank, const uint32_t *sizes, uint32_t np,
                          uint32_t *ncomp, uint32_t *largest, unsigned long long *hist);

}  // namespace mh
