// unwrap_walk.hpp - the stack walk of Modify::unwrap_connectivity_dim (molar/src/modify.rs:80-128) on the host, ONE
// template over the real type: molar_hip_unwrap_connectivity (connectivity.hip: float, molar_hip_box, V3) and
// molar_hip_unwrap_connectivity_f64 (search_f64.hip: double, BoxD, D3; boxmath.hpp) both run it over the CSR that
// SearchConnectivity built on the device.  Serial by nature: every atom is pulled to the closest image of the atom it was
// REACHED FROM, whose position the walk may just have changed.  closest_image is the one of the box type's header, with
// the reference's operation order in the real type.
// Quirks kept: the atom a component starts from (0, then the lowest unused index) is not a member of the selection the
// component returns (:97-98, 111-113); a component of one atom returns no selection; members are emitted as the
// reference's `select(&sel_vec)` makes them, sorted.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

namespace mh {

// h: the frame's coordinates on the host (modified in place); ix: the selection (NULL: atoms 0 .. nsel); off / adj: the
// CSR over local ids in push order; group_offsets (nsel + 1) / group_ids (nsel) may be NULL.
template <class Real, class Vec, class Box>
void unwrap_walk(Real *h, const uint64_t *ix, size_t nsel, const Box &b, uint32_t dims, const uint64_t *off, const uint64_t *adj,
                 uint64_t *group_offsets, uint64_t *group_ids, size_t *ngroups) {
    auto pos = [&](size_t k) -> Real * { return h + 3 * (ix ? ix[k] : (uint64_t)k); };
    std::vector<uint8_t> used(nsel, 0);
    std::vector<uint32_t> todo, sel_vec;
    todo.reserve(1024);
    size_t ng = 0, nids = 0, first_unused = 0;
    if (group_offsets) group_offsets[0] = 0;
    auto emit = [&]() {
        if (sel_vec.empty()) return;
        std::sort(sel_vec.begin(), sel_vec.end());
        if (group_ids) for (uint32_t v : sel_vec) group_ids[nids++] = v;
        else nids += sel_vec.size();
        ++ng;
        if (group_offsets) group_offsets[ng] = nids;
        sel_vec.clear();
    };
    todo.push_back(0);
    used[0] = 1;
    for (;;) {
        while (!todo.empty()) {
            const uint32_t cc = todo.back();
            todo.pop_back();
            const Real *pc = pos(cc);
            const Vec p0{pc[0], pc[1], pc[2]};
            for (uint64_t e = off[cc]; e < off[cc + 1]; ++e) {
                const uint32_t ind = (uint32_t)adj[e];
                if (used[ind]) continue;
                Real *pp = pos(ind);
                const Vec r = closest_image(b, Vec{pp[0], pp[1], pp[2]}, p0, dims);
                pp[0] = r.x; pp[1] = r.y; pp[2] = r.z;
                todo.push_back(ind);
                used[ind] = 1;
                sel_vec.push_back(ind);
            }
        }
        while (first_unused < nsel && used[first_unused]) ++first_unused;       // used.iter().find_position(false)
        if (first_unused == nsel) {
            emit();
            break;
        }
        todo.push_back((uint32_t)first_unused);
        used[first_unused] = 1;
        emit();
    }
    if (ngroups) *ngroups = ng;
}

}  // namespace mh
