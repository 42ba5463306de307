// molar::min_distances of the C++ host mirror (include/molar_hip.hpp) on one small case whose input and expected numbers the
// Python side writes (tests/test_cpp_mindist.py: the longdouble reference of tests/mindist_ref.py with its bounds): two labelled
// selections under a sheared triclinic box.  The pairs, the nearest atoms, the contact counts, the ok frames and the positions of
// inf for equality, the distances within their bounds, the bits of the C call the wrapper forwards to, the f64 wrapper on the
// same numbers, and the wrapper's own argument check.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "molar_hip.hpp"

using namespace molar;

static int failures = 0;
#define EXPECT(cond)                                                         \
    do {                                                                     \
        if (!(cond)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

static std::vector<double> read_doubles(std::FILE *f, size_t count) {
    std::vector<double> v(count);
    for (double &x : v)
        if (std::fscanf(f, "%lf", &x) != 1) { std::printf("FAIL: the case file is short\n"); std::exit(1); }
    return v;
}

// the number of entries beyond their bound; an inf is expected exactly where the reference has one
template <class T>
static size_t beyond(const std::vector<T> &got, const std::vector<double> &want, const std::vector<double> &tol) {
    size_t bad = got.size() != want.size();
    for (size_t i = 0; i < want.size() && i < got.size(); ++i) {
        if (std::isinf(want[i])) bad += !((double)got[i] == want[i]);
        else bad += !(std::fabs((double)got[i] - want[i]) <= tol[i]);
    }
    return bad;
}
template <class T>
static size_t differ(const std::vector<T> &got, const std::vector<double> &want) {
    size_t bad = got.size() != want.size();
    for (size_t i = 0; i < want.size() && i < got.size(); ++i) bad += got[i] != (T)want[i];
    return bad;
}

struct Expected {
    std::vector<double> want, tol32, tol64;
};
static Expected read_expected(std::FILE *f, size_t count) {
    Expected e;
    e.want = read_doubles(f, count);
    e.tol32 = read_doubles(f, count);
    e.tol64 = read_doubles(f, count);
    return e;
}

int main(int argc, char **argv) {
    if (argc < 2) { std::printf("usage: test_mindist_gpu CASE_FILE\n"); return 2; }
    std::FILE *f = std::fopen(argv[1], "r");
    if (!f) { std::printf("cannot open %s\n", argv[1]); return 2; }
    size_t F, natoms, n1, n2, G1, G2;
    double cutoff;
    if (std::fscanf(f, "%zu %zu %zu %zu %zu %zu %lf", &F, &natoms, &n1, &n2, &G1, &G2, &cutoff) != 7) return 2;
    const std::vector<double> idx1_d = read_doubles(f, n1), idx2_d = read_doubles(f, n2), lab1_d = read_doubles(f, n1), lab2_d = read_doubles(f, n2);
    const std::vector<double> box_d = read_doubles(f, 9), xyz = read_doubles(f, F * natoms * 3);
    const std::vector<double> pair = read_doubles(f, 2 * F), near1 = read_doubles(f, F * n1), freq = read_doubles(f, G1 * G2), ok = read_doubles(f, F);
    const Expected dist = read_expected(f, F), atom1 = read_expected(f, F * n1), atom2 = read_expected(f, F * n2), mat = read_expected(f, F * G1 * G2),
                   mean = read_expected(f, G1 * G2), mn = read_expected(f, G1 * G2);
    std::fclose(f);

    std::vector<usize> idx1, idx2;
    std::vector<uint32_t> lab1, lab2;
    for (double v : idx1_d) idx1.push_back((usize)v);
    for (double v : idx2_d) idx2.push_back((usize)v);
    for (double v : lab1_d) lab1.push_back((uint32_t)v);
    for (double v : lab2_d) lab2.push_back((uint32_t)v);
    std::vector<float> x32(xyz.size());
    for (size_t i = 0; i < xyz.size(); ++i) x32[i] = (float)xyz[i];
    float box[9];
    for (int q = 0; q < 9; ++q) box[q] = (float)box_d[q];

    Engine &eng = Engine::global();
    MinDistanceOptions opt;
    opt.cutoff = cutoff;
    opt.ngroups1 = G1;
    opt.ngroups2 = G2;
    opt.want_atom1 = opt.want_atom2 = opt.want_mat = opt.want_mat_stats = true;
    const MinDistances got = min_distances(eng, x32.data(), F, natoms, box, opt, idx1, idx2, lab1, lab2);
    EXPECT(got.nframes == F && got.n1 == n1 && got.n2 == n2 && got.ngroups1 == G1 && got.ngroups2 == G2 && got.nvalid == F);
    EXPECT(differ(got.frame_ok, ok) == 0 && differ(got.pair, pair) == 0 && differ(got.near1, near1) == 0 && differ(got.mat_freq, freq) == 0);
    EXPECT(beyond(got.dist, dist.want, dist.tol32) == 0);
    EXPECT(beyond(got.atom1, atom1.want, atom1.tol32) == 0);
    EXPECT(beyond(got.atom2, atom2.want, atom2.tol32) == 0);
    EXPECT(beyond(got.mat, mat.want, mat.tol32) == 0);
    EXPECT(beyond(got.mat_mean, mean.want, mean.tol64) == 0);             // double in both entries
    EXPECT(beyond(got.mat_min, mn.want, mn.tol32) == 0);

    // the C call the wrapper forwards to: the same bits
    {
        molar_hip_mindist_spec spec{};
        spec.pbc = MOLAR_HIP_PBC_FULL;
        spec.cutoff = cutoff;
        std::vector<float> d(F, -1.0f), a1(F * n1, -1.0f);
        std::vector<uint64_t> p(2 * F, 7), nr(F * n1, 7);
        std::vector<uint32_t> fq(G1 * G2, 7);
        uint64_t nv = 0;
        EXPECT(molar_hip_mindist(eng.ctx(), x32.data(), F, natoms * 3, natoms, idx1.data(), n1, lab1.data(), G1, idx2.data(), n2, lab2.data(), G2, box, 0, &spec,
                                 d.data(), p.data(), a1.data(), nr.data(), n1, nullptr, 0, nullptr, nullptr, nullptr, fq.data(), nullptr, &nv) == 0);
        EXPECT(nv == F && p == got.pair && nr == got.near1 && fq == got.mat_freq);
        EXPECT(std::memcmp(d.data(), got.dist.data(), d.size() * sizeof(float)) == 0 && std::memcmp(a1.data(), got.atom1.data(), a1.size() * sizeof(float)) == 0);
    }

    // the distances alone: nothing else is made
    {
        const MinDistances r = min_distances(eng, x32.data(), F, natoms, box, MinDistanceOptions(), idx1, idx2);
        EXPECT(r.atom1.empty() && r.near1.empty() && r.atom2.empty() && r.mat.empty() && r.mat_mean.empty() && r.dist.size() == F && r.pair.size() == 2 * F);
        EXPECT(std::memcmp(r.dist.data(), got.dist.data(), F * sizeof(float)) == 0 && r.pair == got.pair);
    }

    // the f64 wrapper on the same numbers
    {
        std::vector<double> x64(xyz.size()), b64(9);
        for (size_t i = 0; i < xyz.size(); ++i) x64[i] = (double)x32[i];
        for (int k = 0; k < 9; ++k) b64[k] = (double)box[k];
        const MinDistancesOf<double> e = min_distances_f64(eng, x64.data(), F, natoms, b64.data(), opt, idx1, idx2, lab1, lab2);
        EXPECT(differ(e.frame_ok, ok) == 0 && differ(e.pair, pair) == 0 && differ(e.near1, near1) == 0 && differ(e.mat_freq, freq) == 0);
        EXPECT(beyond(e.dist, dist.want, dist.tol64) == 0 && beyond(e.atom1, atom1.want, atom1.tol64) == 0 && beyond(e.atom2, atom2.want, atom2.tol64) == 0 &&
               beyond(e.mat, mat.want, mat.tol64) == 0 && beyond(e.mat_mean, mean.want, mean.tol64) == 0 && beyond(e.mat_min, mn.want, mn.tol64) == 0);
    }

    bool threw = false;
    try { lab1.pop_back(); min_distances(eng, x32.data(), F, natoms, box, opt, idx1, idx2, lab1, lab2); } catch (const MolarError &) { threw = true; }
    EXPECT(threw);
    threw = false;
    try { lab1.push_back((uint32_t)G1); min_distances(eng, x32.data(), F, natoms, box, opt, idx1, idx2, lab1, lab2); } catch (const MolarError &e) {
        threw = e.code == MOLAR_HIP_ERR_INVALID_ARGUMENT;                                  // a label not below ngroups1
    }
    EXPECT(threw);

    std::printf("minimum distances: %zu frames, %zu x %zu atoms in %zu x %zu groups\n", F, n1, n2, G1, G2);
    if (failures) { std::printf("%d failure(s)\n", failures); return 1; }
    std::printf("all minimum-distance host-mirror tests passed\n");
    return 0;
}
