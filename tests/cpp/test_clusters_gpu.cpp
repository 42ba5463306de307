// molar::clusters / clusters_frames (include/molar_hip.hpp -> molar_hip_search_clusters / _frames) on one small frame whose
// partition is known by construction (tests/clusters_ref.py, blob_frame: 8 blobs, two pairs of them bridged, one pair across a
// face of the box), handed over in a file by the Python driver (tests/test_cpp_clusters.py).  Integers, compared for equality.
//
// File (little endian): u64 natoms, ncomponents; f32 cutoff, box9[9] (column-major); f32 xyz[natoms][3]; u32 comp_of[natoms];
// u32 labels[natoms] (the blob of every atom), u64 ngroups, gcomponents; u32 gcomp_of[ngroups].
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
    if (argc < 2) { std::printf("usage: test_clusters_gpu <case file>\n"); return 2; }
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::printf("cannot open %s\n", argv[1]); return 2; }
    const auto head = take<uint64_t>(f, 2);
    const size_t natoms = head[0], ncomp = head[1];
    const auto fl = take<float>(f, 10);
    const float cutoff = fl[0];
    const auto xyz = take<float>(f, natoms * 3);
    const auto comp_of = take<uint32_t>(f, natoms);
    const auto labels = take<uint32_t>(f, natoms);
    const auto ghead = take<uint64_t>(f, 2);
    const size_t ngroups = ghead[0], gcomp = ghead[1];
    const auto gcomp_of = take<uint32_t>(f, ngroups);
    std::fclose(f);
    if (failures) return 1;

    Matrix3f m;
    for (int k = 0; k < 9; ++k) m.m[k] = fl[1 + k];
    const PeriodicBox box = PeriodicBox::from_matrix(m);
    Engine &eng = Engine::global();
    Topology top;
    State st;
    top.masses.assign(natoms, 1.0f);
    for (size_t a = 0; a < natoms; ++a) st.coords.push_back(Pos{xyz[3 * a], xyz[3 * a + 1], xyz[3 * a + 2]});
    st.pbox = box;
    System sys(top, st);
    std::vector<usize> all(natoms);
    for (size_t a = 0; a < natoms; ++a) all[a] = a;
    SelBound sel(sys, all);

    // ---- atoms as particles
    const Clusters c = clusters(cutoff, sel, &box, PBC_FULL);
    EXPECT(c.ncomponents == ncomp && ncomp > 1);
    EXPECT(c.comp_of == comp_of);
    EXPECT(c.sizes.size() == ncomp && c.offsets.size() == ncomp + 1 && c.members.size() == natoms);
    std::vector<uint32_t> sizes(ncomp, 0);
    for (uint32_t k : comp_of) sizes[k] += 1;
    EXPECT(c.sizes == sizes);
    const auto parts = c.split();
    bool parts_ok = parts.size() == ncomp;
    for (size_t k = 0; parts_ok && k < ncomp; ++k) {
        parts_ok = parts[k].size() == sizes[k] && c.offsets[k + 1] - c.offsets[k] == sizes[k];
        for (size_t t = 0; parts_ok && t < parts[k].size(); ++t)
            parts_ok = comp_of[parts[k][t]] == k && (t == 0 || parts[k][t - 1] < parts[k][t]);
        parts_ok = parts_ok && (k == 0 || parts[k - 1][0] < parts[k][0]);          // numbered by the smallest member
    }
    EXPECT(parts_ok);

    // ---- the blobs as particles
    const Clusters g = clusters(cutoff, sel, &box, PBC_FULL, labels, ngroups);
    EXPECT(g.ncomponents == gcomp && g.comp_of == gcomp_of);

    // ---- the frames form: the same frame twice, on top of a histogram that is not zero
    std::vector<float> two(xyz);
    two.insert(two.end(), xyz.begin(), xyz.end());
    std::vector<float> boxes(fl.begin() + 1, fl.begin() + 10);
    boxes.insert(boxes.end(), fl.begin() + 1, fl.begin() + 10);
    ClusterSizes cs;
    cs.size_hist.assign(natoms + 1, 3);
    clusters_frames(eng, two.data(), 2, natoms, boxes.data(), cutoff, {}, PBC_FULL, cs);
    uint32_t largest = 0;
    std::vector<uint64_t> hist(natoms + 1, 3);
    for (uint32_t s : sizes) { hist[s] += 2; largest = s > largest ? s : largest; }
    EXPECT(cs.ncomponents == std::vector<uint32_t>(2, (uint32_t)ncomp));
    EXPECT(cs.largest == std::vector<uint32_t>(2, largest));
    EXPECT(cs.size_hist == hist);

    // ---- a label out of range is refused
    std::vector<uint32_t> bad = labels;
    bad[0] = (uint32_t)ngroups;
    bool threw = false;
    try { clusters(cutoff, sel, &box, PBC_FULL, bad, ngroups); } catch (const MolarError &) { threw = true; }
    EXPECT(threw);

    if (failures) return 1;
    std::printf("all clusters host-mirror tests passed\n");
    return 0;
}
