// ContactMap (include/molar_hip.hpp -> molar_hip_search_contacts_frames) against the folds of the oracle's pair lists that the
// Python driver (tests/test_cpp_contacts.py) computes and hands over in a file: one single-selection frame through add_frame,
// and one two-selection trajectory block through add_trajectory_double_pbc.  Integers, compared for equality.
//
// File (little endian): u64 natoms, nframes, n1, n2, G1, G2; f32 cutoff, box9[9] (column-major); f32 frames[nframes][natoms][3];
// u64 idx1[n1], idx2[n2]; u32 l1[n1], l2[n2]; single frame 0 of idx1: u64 deg[n1], map[G1 * G1]; block: u64 deg1[n1], deg2[n2],
// map[G1 * G2]; u32 occ[G1 * G2].
#include <cstdio>
#include <vector>

#include "molar_hip.hpp"

using namespace molar;

static int failures = 0;
#define EXPECT(cond)                                                         \
    do {                                                                     \
        if (!(cond)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

template <class T>
static std::vector<T> take(std::FILE *f, size_t n) {
    std::vector<T> v(n);
    if (n && std::fread(v.data(), sizeof(T), n, f) != n) { std::printf("FAIL short read\n"); ++failures; }
    return v;
}

int main(int argc, char **argv) {
    if (argc < 2) { std::printf("usage: test_contacts_gpu <case file>\n"); return 2; }
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::printf("cannot open %s\n", argv[1]); return 2; }
    const auto head = take<uint64_t>(f, 6);
    const size_t natoms = head[0], nframes = head[1], n1 = head[2], n2 = head[3], G1 = head[4], G2 = head[5];
    const auto fl = take<float>(f, 10);
    const float cutoff = fl[0];
    const auto frames = take<float>(f, nframes * natoms * 3);
    const auto idx1 = take<uint64_t>(f, n1), idx2 = take<uint64_t>(f, n2);
    const auto l1 = take<uint32_t>(f, n1), l2 = take<uint32_t>(f, n2);
    const auto s_deg = take<uint64_t>(f, n1), s_map = take<uint64_t>(f, G1 * G1);
    const auto d_deg1 = take<uint64_t>(f, n1), d_deg2 = take<uint64_t>(f, n2), d_map = take<uint64_t>(f, G1 * G2);
    const auto d_occ = take<uint32_t>(f, G1 * G2);
    std::fclose(f);
    if (failures) return 1;

    Matrix3f m;
    for (int k = 0; k < 9; ++k) m.m[k] = fl[1 + k];
    const PeriodicBox box = PeriodicBox::from_matrix(m);
    Engine &eng = Engine::global();

    // ---- one single-selection frame
    Topology top;
    State st;
    top.masses.assign(natoms, 1.0f);
    for (size_t a = 0; a < natoms; ++a) st.coords.push_back(Pos{frames[3 * a], frames[3 * a + 1], frames[3 * a + 2]});
    st.pbox = box;
    System sys(top, st);
    SelBound sel(sys, idx1);
    ContactMap single(l1, G1);
    single.add_frame(cutoff, sel, nullptr, &box, PBC_FULL);
    EXPECT(single.frames == 1 && single.deg2.empty());
    EXPECT(single.deg1 == s_deg);
    EXPECT(single.map == s_map);
    uint64_t total = 0, nz = 0;
    for (uint64_t v : s_map) { total += v; nz += v ? 1 : 0; }
    EXPECT(total > 0 && single.entries() == total);
    uint64_t onz = 0;
    bool occ_ok = true;
    for (size_t k = 0; k < single.occupancy.size(); ++k) {
        onz += single.occupancy[k];
        occ_ok = occ_ok && single.occupancy[k] == (s_map[k] ? 1u : 0u);
    }
    EXPECT(occ_ok && onz == nz);
    single.add_frame(cutoff, sel, nullptr, &box, PBC_FULL);          // the same frame again: everything doubles
    bool twice = single.frames == 2;
    for (size_t k = 0; k < s_map.size(); ++k) twice = twice && single.map[k] == 2 * s_map[k] && single.occupancy[k] == (s_map[k] ? 2u : 0u);
    for (size_t k = 0; k < n1; ++k) twice = twice && single.deg1[k] == 2 * s_deg[k];
    EXPECT(twice);

    // ---- a two-selection trajectory block, one box for all frames
    ContactMap block(l1, G1, l2, G2);
    std::vector<float> boxes;
    for (size_t k = 0; k < nframes; ++k) boxes.insert(boxes.end(), fl.begin() + 1, fl.begin() + 10);
    block.add_trajectory_double_pbc(eng, frames.data(), nframes, natoms, boxes.data(), cutoff, idx1, idx2, PBC_FULL);
    EXPECT(block.frames == nframes);
    EXPECT(block.deg1 == d_deg1);
    EXPECT(block.deg2 == d_deg2);
    EXPECT(block.map == d_map);
    EXPECT(block.occupancy == d_occ);
    ContactMap sum(l1, G1, l2, G2);
    sum.add_trajectory_double_pbc(eng, frames.data(), 1, natoms, boxes.data(), cutoff, idx1, idx2, PBC_FULL);
    ContactMap rest(l1, G1, l2, G2);
    rest.add_trajectory_double_pbc(eng, frames.data() + natoms * 3, nframes - 1, natoms, boxes.data() + 9, cutoff, idx1, idx2, PBC_FULL);
    sum.merge(rest);
    EXPECT(sum.map == d_map && sum.occupancy == d_occ && sum.deg1 == d_deg1 && sum.deg2 == d_deg2 && sum.frames == nframes);

    // ---- a label out of range is refused
    std::vector<uint32_t> bad = l1;
    bad[0] = (uint32_t)G1;
    ContactMap refused(bad, G1);
    bool threw = false;
    try { refused.add_frame(cutoff, sel, nullptr, &box, PBC_FULL); } catch (const MolarError &) { threw = true; }
    EXPECT(threw);

    if (failures) return 1;
    std::printf("all contacts host-mirror tests passed\n");
    return 0;
}
