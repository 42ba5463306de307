// contact_kernels.hpp - the fused contact consumer of the distance search (molar_hip_search_contacts): per-atom contact
// counts and a group x group contact matrix straight from the pair loop, no pair written to memory.
// Included by contacts.hip (ContactArgs, the launcher's declaration) and by pair_k9.hip, which instantiates the kernels; and by
// cluster_kernels.hpp, whose kernel walks the same records with the same slot decode and hit decision (contact_slot, contact_hit).
//
// One kernel walks the slot records of the REGULAR plan (plan_kernel / slotmap_kernel: the list the count pass walks), every
// class of entry through one row loop:
//   * rows of the first cell are scalar (v_readlane of the 64 rows a wave loaded one per lane), the second cell is taken in
//     64-atom chunks, one atom per lane; hit masks come from ballot;
//   * plain and same-cell (j > i) entries use |p2 - p1|^2 in the list's operation order.  Wrapped entries are decided the way
//     the list decides them (run_fast): where the box allows the band classification (SearchParams::approx_wrapped) the plain
//     distance to the image cell b + S decides outside the band around cutoff^2 and PeriodicBox::distance_squared inside it;
//     a cell against its own image, the triclinic corner entries and boxes without the classification evaluate
//     PeriodicBox::distance_squared for every candidate (f32::round, general matrix form, the lattice-shift candidates where
//     all three dimensions wrap);
//   * second cells of any size are streamed chunk by chunk (no register-resident instance per size).
// Sums that share a destination are formed on chip before they leave the wave:
//   * a row's degree is a scalar popcount sum kept in lane `row`; a column's degree is a per-lane counter per chunk.  Both
//     leave the wave once per slot / per chunk of the slot: one 64-bit add per atom, to the atoms' selection positions;
//   * the map: a lane counts the hits of its own atom against the current RUN of rows of one group (rows of a cell are in
//     input order, so the row's group changes rarely).  When the row's group changes, or the chunk ends, lanes whose atoms
//     carry the same label and sit next to each other (a segmented scan over the chunk's label runs) are summed and the last
//     lane of each run adds one word.  Labels without locality (random) degrade to one add per lane and run - slow, correct.
#pragma once

#include "pair_kernels.hpp"

namespace mh {
namespace pairk {

struct ContactArgs {
    const uint32_t *g1;              // labels by selection position of set 1 (NULL: no map)
    const uint32_t *g2;              // ... of set 2 (SINGLE: == g1)
    uint32_t ng2;                    // row length of the map (SINGLE: ngroups1)
    unsigned long long *deg1;        // NULL: not wanted
    unsigned long long *deg2;        // SINGLE: == deg1 (second members count into the same array)
    unsigned long long *map;         // 64-bit map, or NULL
    uint32_t *map32;                 // per-frame 32-bit map (frames form with occupancy), or NULL; at most one of the two
    unsigned long long *count;       // |L|
};

// PeriodicBox::distance_squared (periodic_box.rs:286-318, 379-381) for one candidate, general matrix form, v = p2 - p1
__device__ __forceinline__ float contact_wrapped_d2(const SearchParams &P, uint32_t wrap, float vx, float vy, float vz) {
    const float *I = P.box.inv, *M = P.box.m;
    float fx = (I[0] * vx + I[3] * vy) + I[6] * vz;
    float fy = (I[1] * vx + I[4] * vy) + I[7] * vz;
    float fz = (I[2] * vx + I[5] * vy) + I[8] * vz;
    if (wrap & 1u) fx -= __builtin_roundf(fx);
    if (wrap & 2u) fy -= __builtin_roundf(fy);
    if (wrap & 4u) fz -= __builtin_roundf(fz);
    const float sx = (M[0] * fx + M[3] * fy) + M[6] * fz;
    const float sy = (M[1] * fx + M[4] * fy) + M[7] * fz;
    const float sz = (M[2] * fx + M[5] * fy) + M[8] * fz;
    float best2 = (sx * sx + sy * sy) + sz * sz;
    if (P.box.nshift != 0 && wrap == MOLAR_HIP_PBC_FULL) {   // triclinic candidates (:304-317)
        for (int k = 0; k < P.box.nshift; ++k) {
            const float cx = sx + P.box.shifts[3 * k], cy = sy + P.box.shifts[3 * k + 1], cz = sz + P.box.shifts[3 * k + 2];
            const float n2 = (cx * cx + cy * cy) + cz * cz;
            best2 = n2 < best2 ? n2 : best2;
        }
    }
    return best2;
}

// What a wave needs of one slot record of the regular plan (prepare_search with live_rows = false): the header's fields and the
// class of the entry.  Shared by the consumers that walk these records without writing a pair (contact_kernel here,
// cluster_kernel of cluster_kernels.hpp), so that every class of entry is decided by the same code in all of them.
struct ContactSlot {
    uint32_t a0, n1, b0, n2;         // first atoms and sizes of the two cells in the sorted arrays
    uint32_t i0, rows;               // first row of the slot in the first cell, rows of the slot (<= 64)
    uint32_t wrap;                   // dimensions the entry wraps in
    bool tri;                        // same cell: j > i only
    bool wrapped;                    // the entry crosses a periodic boundary
    bool approx;                     // ... and is band-classified (as run_fast): S moves the second cell next to the first one
    float Sx, Sy, Sz;
    float band_lo, band_hi, cutoff2;
};

// decodes slot record `slot`; false: the record is past the last slot or has no rows
__device__ __forceinline__ bool contact_slot(const SearchParams &P, const SlotDesc *__restrict__ slot_desc, uint32_t slot, ContactSlot &S) {
    const uint4 lo = reinterpret_cast<const uint4 *>(slot_desc + slot)[0];
    const uint4 hi = reinterpret_cast<const uint4 *>(slot_desc + slot)[1];
    const uint32_t fl = __builtin_amdgcn_readfirstlane(hi.y);
    if (!(fl & 0x200u)) return false;                   // past the last slot
    S.a0 = __builtin_amdgcn_readfirstlane(lo.x);
    S.n1 = __builtin_amdgcn_readfirstlane(lo.y);
    S.b0 = __builtin_amdgcn_readfirstlane(lo.z);
    S.n2 = __builtin_amdgcn_readfirstlane(lo.w);
    S.i0 = __builtin_amdgcn_readfirstlane(hi.z);
    const uint32_t rps = fl >> 16;
    S.wrap = fl & 7u;
    S.tri = (fl & 0x100u) != 0u;
    S.wrapped = P.use_box && S.wrap != 0u;
    if (S.i0 >= S.n1) return false;
    // band classification of a wrapped entry (as run_fast): b + S is the image of the second cell next to the first one
    S.approx = S.wrapped && !S.tri && P.approx_wrapped != 0u && !(P.box.nshift != 0 && S.wrap == MOLAR_HIP_PBC_FULL);
    S.Sx = S.Sy = S.Sz = 0.f;
    if (S.approx) {
        const uint32_t wrap_b = (fl >> 12) & 7u;
        for (int d = 0; d < 3; ++d) {
            if (!((S.wrap >> d) & 1u)) continue;
            const float sgn = ((wrap_b >> d) & 1u) ? 1.0f : -1.0f;   // second cell wrapped: +col, first cell: -col
            S.Sx += sgn * P.box.m[3 * d];
            S.Sy += sgn * P.box.m[3 * d + 1];
            S.Sz += sgn * P.box.m[3 * d + 2];
        }
    }
    S.band_lo = P.band_lo;
    S.band_hi = P.band_hi;
    S.cutoff2 = P.cutoff2;
    S.rows = S.n1 - S.i0 < rps ? S.n1 - S.i0 : rps;      // <= 64
    return true;
}

// Is the lane's atom b (position jj of the second cell, `valid`: there is one; sb = b + S) within the cutoff of row r of the slot,
// whose position is p?  The list's own decision; every lane of the wave calls it (the band's exact evaluation is entered on a ballot).
__device__ __forceinline__ bool contact_hit(const SearchParams &P, const ContactSlot &S, bool valid, const float4 &b, float sbx, float sby, float sbz,
                                            float px, float py, float pz, uint32_t jj, uint32_t r) {
    const float dx = b.x - px, dy = b.y - py, dz = b.z - pz;            // p2 - p1
    bool hit;
    if (S.approx) {
        const float ax = sbx - px, ay = sby - py, az = sbz - pz;
        const float d2a = (ax * ax + ay * ay) + az * az;
        const bool sure = d2a < S.band_lo, maybe = d2a <= S.band_hi;
        hit = sure;
        if (__builtin_amdgcn_ballot_w64(valid && maybe && !sure))
            hit = sure || (maybe && contact_wrapped_d2(P, S.wrap, dx, dy, dz) <= S.cutoff2);
    } else if (S.wrapped) {
        hit = contact_wrapped_d2(P, S.wrap, dx, dy, dz) <= S.cutoff2;
    } else {
        hit = (dx * dx + dy * dy) + dz * dz <= S.cutoff2;                  // (:446, :460, :488)
    }
    hit = hit && valid;
    if (S.tri) hit = hit && jj > S.i0 + r;
    return hit;
}

constexpr int CONTACT_WAVES = 4;      // waves per workgroup; every wave walks its own slots

template <int KIND>
__global__ void __launch_bounds__(64 * CONTACT_WAVES) contact_kernel(const SearchParams *__restrict__ Pp, const SlotDesc *__restrict__ slot_desc,
                                                                     const uint32_t nslots, const ContactArgs A) {
    constexpr bool SINGLE = KIND == MOLAR_HIP_SEARCH_SINGLE;
    const SearchParams &P = *Pp;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t w0 = blockIdx.x * CONTACT_WAVES + wave, stride = gridDim.x * CONTACT_WAVES;
    const bool has_map = A.g1 != nullptr;
    unsigned long long wave_total = 0;

    for (uint32_t w = w0; w < nslots; w += stride) {
        const uint32_t slot = nslots - 1u - w;          // the heavy wrapped entries at the far edge of the plan start first
        ContactSlot S;
        if (!contact_slot(P, slot_desc, slot, S)) continue;
        const uint32_t a0 = S.a0, b0 = S.b0, n2 = S.n2, i0 = S.i0, rows = S.rows;
        const bool tri = S.tri;

        float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
        if (lane < rows) a = gload4(P.sa, a0 + i0 + lane);
        const uint32_t ida = __float_as_uint(a.w);
        uint32_t ga = 0u;
        if (has_map && lane < rows) ga = gload_u32(A.g1, ida);
        uint32_t rowdeg = 0u;                                     // lane r: hits of row r in this slot

        const uint32_t nchunks = (n2 + 63u) >> 6;
        for (uint32_t c = 0; c < nchunks; ++c) {
            if (tri && c * 64u + 63u <= i0) continue;             // same cell, j in i+1..n (:443): the whole chunk has j <= i
            const uint32_t jj = c * 64u + lane;
            const bool valid = jj < n2;
            float4 b = make_float4(3.0e38f, 3.0e38f, 3.0e38f, 0.f);
            if (valid) b = gload4(P.sb, b0 + jj);
            const uint32_t idb = __float_as_uint(b.w);
            const float sbx = b.x + S.Sx, sby = b.y + S.Sy, sbz = b.z + S.Sz;          // the image (approx entries; S == 0 otherwise)
            // the chunk's label runs: lanes next to each other with the same label form a segment
            uint32_t gb = 0xFFFFFFFFu, seg = lane;
            bool tail = true, all_heads = true;
            if (has_map) {
                if (valid) gb = gload_u32(A.g2, idb);
                const uint32_t gprev = (uint32_t)__shfl_up((int)gb, 1, 64);
                const unsigned long long heads = __builtin_amdgcn_ballot_w64(lane == 0u || gprev != gb);
                seg = (uint32_t)__popcll(heads & (~0ull >> (63u - lane)));
                tail = lane == 63u || ((heads >> (lane + 1u)) & 1ull) != 0ull;
                all_heads = heads == ~0ull;
            }
            uint32_t colcnt = 0u, mcnt = 0u;
            uint32_t run = (uint32_t)__builtin_amdgcn_readfirstlane((int)ga);       // group of the current run of rows
            // one add per (run of rows of one group) x (run of lanes of one label)
            auto flush = [&](uint32_t grow) {
                if (__builtin_amdgcn_ballot_w64(mcnt != 0u) == 0ull) return;
                uint32_t s = mcnt;
                if (!all_heads) {
#pragma unroll
                    for (int off = 1; off < 64; off <<= 1) {
                        const uint32_t v = (uint32_t)__shfl_up((int)s, off, 64);
                        const uint32_t sg = (uint32_t)__shfl_up((int)seg, off, 64);
                        if (lane >= (uint32_t)off && sg == seg) s += v;
                    }
                }
                if (tail && s != 0u) {
                    uint32_t r = grow, q = gb;
                    if (SINGLE && q < r) { r = gb; q = grow; }     // upper triangle: [min][max]
                    const size_t at = (size_t)r * A.ng2 + q;
                    if (A.map32) atomicAdd(&A.map32[at], s);
                    else atomicAdd(&A.map[at], (unsigned long long)s);
                }
                mcnt = 0u;
            };
            for (uint32_t r = 0; r < rows; ++r) {
                const float px = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(a.x), r));
                const float py = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(a.y), r));
                const float pz = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(a.z), r));
                if (has_map) {
                    const uint32_t gr = (uint32_t)__builtin_amdgcn_readlane((int)ga, r);
                    if (gr != run) {
                        flush(run);
                        run = gr;
                    }
                }
                const bool hit = contact_hit(P, S, valid, b, sbx, sby, sbz, px, py, pz, jj, r);
                const unsigned long long mask = __builtin_amdgcn_ballot_w64(hit);
                const uint32_t cnt = (uint32_t)__popcll(mask);
                if (lane == r) rowdeg += cnt;
                wave_total += cnt;
                if (hit) {
                    colcnt += 1u;
                    mcnt += 1u;
                }
            }
            if (has_map) flush(run);
            if (A.deg2 && colcnt != 0u) atomicAdd(&A.deg2[idb], (unsigned long long)colcnt);
        }
        if (A.deg1 && rowdeg != 0u) atomicAdd(&A.deg1[ida], (unsigned long long)rowdeg);
    }
    if (lane == 0u && wave_total && A.count) atomicAdd(A.count, wave_total);
}

template <int KIND>
inline void launch_contact_kernel(unsigned num_cus, hipStream_t stream, const SearchParams *dP, const SlotDesc *slot_desc, uint32_t nslots,
                                  const ContactArgs &A) {
    unsigned nblk = (nslots + (unsigned)CONTACT_WAVES - 1u) / (unsigned)CONTACT_WAVES;
    const unsigned cap = num_cus * 8u;
    if (nblk > cap) nblk = cap;
    if (nblk == 0u) return;
    hipLaunchKernelGGL((contact_kernel<KIND>), dim3(nblk), dim3(64 * CONTACT_WAVES), 0, stream, dP, slot_desc, nslots, A);
}

}  // namespace pairk

// defined in pair_k9.hip.  kind: MOLAR_HIP_SEARCH_SINGLE or _DOUBLE
void launch_contacts(int kind, unsigned num_cus, hipStream_t stream, const pairk::SearchParams *dP, const pairk::SlotDesc *slot_desc,
                     uint32_t nslots, const pairk::ContactArgs &A);

}  // namespace mh
