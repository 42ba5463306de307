// molar::vector_correlations of the C++ host mirror (include/molar_hip.hpp) on one small case whose input and expected numbers
// the Python side writes (tests/test_cpp_tcf.py: the longdouble reference of tests/tcf_ref.py with its bounds): bond vectors in
// an orthorhombic box, three groups.  The valid vectors and the bad frames for equality, every curve, mean and order parameter
// within its bound, the bits of the C call the wrapper forwards to, the f64 wrapper on the same numbers, and the wrapper's own
// argument check.
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

// the number of entries beyond their bound
template <class T>
static size_t beyond(const std::vector<T> &got, const std::vector<double> &want, const std::vector<double> &tol) {
    size_t bad = got.size() != want.size();
    for (size_t i = 0; i < want.size() && i < got.size(); ++i) bad += !(std::fabs((double)got[i] - want[i]) <= tol[i]);
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
    if (argc < 2) { std::printf("usage: test_tcf_gpu CASE_FILE\n"); return 2; }
    std::FILE *f = std::fopen(argv[1], "r");
    if (!f) { std::printf("cannot open %s\n", argv[1]); return 2; }
    size_t F, natoms, V, G, L;
    if (std::fscanf(f, "%zu %zu %zu %zu %zu", &F, &natoms, &V, &G, &L) != 5) return 2;
    const std::vector<double> tup_d = read_doubles(f, V * 2), lab_d = read_doubles(f, V), box_d = read_doubles(f, 9), xyz = read_doubles(f, F * natoms * 3);
    const std::vector<double> nvalid = read_doubles(f, G), bad = read_doubles(f, V);
    const Expected c1 = read_expected(f, G * (L + 1)), c2 = read_expected(f, G * (L + 1)), c1v = read_expected(f, V * (L + 1)), c2v = read_expected(f, V * (L + 1));
    const Expected mean = read_expected(f, V * 3), s2 = read_expected(f, V);
    std::fclose(f);

    std::vector<usize> tuples;
    std::vector<uint32_t> labels;
    for (double v : tup_d) tuples.push_back((usize)v);
    for (double v : lab_d) labels.push_back((uint32_t)v);
    std::vector<float> x32(xyz.size());
    for (size_t i = 0; i < xyz.size(); ++i) x32[i] = (float)xyz[i];
    float box[9];
    for (int q = 0; q < 9; ++q) box[q] = (float)box_d[q];

    Engine &eng = Engine::global();
    VectorCorrelationsOptions opt;
    opt.max_lag = L;
    opt.ngroups = G;
    opt.want_per_vector = true;
    const VectorCorrelations got = vector_correlations(eng, x32.data(), F, natoms, tuples, 2, box, opt, labels);
    EXPECT(got.nframes == F && got.nvectors == V && got.ngroups == G && got.nlags == L + 1);
    EXPECT(differ(got.nvalid, nvalid) == 0);
    EXPECT(differ(got.bad_frames, bad) == 0);
    EXPECT(beyond(got.c1, c1.want, c1.tol32) == 0);
    EXPECT(beyond(got.c2, c2.want, c2.tol32) == 0);
    EXPECT(beyond(got.c1_vec, c1v.want, c1v.tol32) == 0);
    EXPECT(beyond(got.c2_vec, c2v.want, c2v.tol32) == 0);
    EXPECT(beyond(got.mean, mean.want, mean.tol32) == 0);
    EXPECT(beyond(got.s2, s2.want, s2.tol32) == 0);

    // the C call the wrapper forwards to: the same bits
    {
        molar_hip_tcf_spec spec{};
        spec.kind = 2;
        spec.mode = MOLAR_HIP_TCF_UNIT;
        spec.dims = 7;
        std::vector<float> a(G * (L + 1), -1.0f), b(G * (L + 1), -1.0f), m(V * 3, -1.0f), s(V, -1.0f);
        std::vector<uint64_t> n(G, 7);
        std::vector<uint32_t> bf(V, 7);
        EXPECT(molar_hip_tcf(eng.ctx(), x32.data(), F, natoms * 3, natoms, tuples.data(), V, labels.data(), G, box, 0, MOLAR_HIP_PBC_FULL, &spec, L, 1, a.data(),
                             b.data(), nullptr, nullptr, 0, n.data(), m.data(), s.data(), bf.data()) == 0);
        EXPECT(n == got.nvalid && bf == got.bad_frames);
        EXPECT(std::memcmp(a.data(), got.c1.data(), a.size() * sizeof(float)) == 0 && std::memcmp(b.data(), got.c2.data(), b.size() * sizeof(float)) == 0 &&
               std::memcmp(m.data(), got.mean.data(), m.size() * sizeof(float)) == 0 && std::memcmp(s.data(), got.s2.data(), s.size() * sizeof(float)) == 0);
    }

    // the group curves alone, in RAW mode: no P2, nothing else is made
    {
        VectorCorrelationsOptions only = opt;
        only.mode = MOLAR_HIP_TCF_RAW;
        only.want_per_vector = false;
        only.want_stats = false;
        const VectorCorrelations r = vector_correlations(eng, x32.data(), F, natoms, tuples, 2, box, only, labels);
        EXPECT(r.c1.size() == G * (L + 1) && r.c2.empty() && r.c1_vec.empty() && r.mean.empty() && r.s2.empty() && r.bad_frames.empty() && r.nvalid == got.nvalid);
    }

    // the f64 wrapper on the same numbers
    {
        std::vector<double> x64(xyz.size()), b64(9);
        for (size_t i = 0; i < xyz.size(); ++i) x64[i] = (double)x32[i];
        for (int k = 0; k < 9; ++k) b64[k] = (double)box[k];
        const VectorCorrelationsOf<double> e = vector_correlations_f64(eng, x64.data(), F, natoms, tuples, 2, b64.data(), opt, labels);
        EXPECT(differ(e.nvalid, nvalid) == 0 && differ(e.bad_frames, bad) == 0);
        EXPECT(beyond(e.c1, c1.want, c1.tol64) == 0 && beyond(e.c2, c2.want, c2.tol64) == 0 && beyond(e.c1_vec, c1v.want, c1v.tol64) == 0 &&
               beyond(e.c2_vec, c2v.want, c2v.tol64) == 0 && beyond(e.mean, mean.want, mean.tol64) == 0 && beyond(e.s2, s2.want, s2.tol64) == 0);
    }

    bool threw = false;
    try { tuples.pop_back(); vector_correlations(eng, x32.data(), F, natoms, tuples, 2, box, opt); } catch (const MolarError &) { threw = true; }
    EXPECT(threw);
    threw = false;
    try { tuples.push_back((usize)natoms); vector_correlations(eng, x32.data(), F, natoms, tuples, 2, box, opt); } catch (const MolarError &e) {
        threw = e.code == MOLAR_HIP_ERR_INVALID_ARGUMENT;                                  // an index not below natoms
    }
    EXPECT(threw);

    std::printf("vector correlations: %zu frames, %zu vectors in %zu groups, %zu lags\n", F, V, G, L + 1);
    if (failures) { std::printf("%d failure(s)\n", failures); return 1; }
    std::printf("all vector-correlation host-mirror tests passed\n");
    return 0;
}
