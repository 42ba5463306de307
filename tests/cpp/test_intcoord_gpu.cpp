// molar::internal_coords of the C++ host mirror (include/molar_hip.hpp) on one small case whose input and expected numbers
// the Python side writes (tests/test_cpp_intcoord.py: the longdouble reference of tests/intcoord_ref.py with its bounds):
// dihedrals of a chain in an orthorhombic box, three groups, a map of neighbouring tuples.  The histogram, the map and the
// valid frames for equality, every value, mean and spread within its bound, the bits of the C call the wrapper forwards to,
// the f64 wrapper on the same numbers, and the wrapper's own argument check.
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
static size_t differ(const std::vector<uint64_t> &got, const std::vector<double> &want) {
    size_t bad = got.size() != want.size();
    for (size_t i = 0; i < want.size() && i < got.size(); ++i) bad += got[i] != (uint64_t)want[i];
    return bad;
}

int main(int argc, char **argv) {
    if (argc < 2) { std::printf("usage: test_intcoord_gpu CASE_FILE\n"); return 2; }
    std::FILE *f = std::fopen(argv[1], "r");
    if (!f) { std::printf("cannot open %s\n", argv[1]); return 2; }
    size_t F, natoms, T, G, nbins, P, mb;
    if (std::fscanf(f, "%zu %zu %zu %zu %zu %zu %zu", &F, &natoms, &T, &G, &nbins, &P, &mb) != 7) return 2;
    const std::vector<double> tup_d = read_doubles(f, T * 4), lab_d = read_doubles(f, T), pair_d = read_doubles(f, P * 2), box_d = read_doubles(f, 9);
    const std::vector<double> xyz = read_doubles(f, F * natoms * 3), hist = read_doubles(f, G * nbins), map = read_doubles(f, mb * mb), valid = read_doubles(f, T);
    const std::vector<double> val = read_doubles(f, F * T), vtol32 = read_doubles(f, F * T), vtol64 = read_doubles(f, F * T);
    const std::vector<double> mean = read_doubles(f, T), mtol32 = read_doubles(f, T), mtol64 = read_doubles(f, T);
    const std::vector<double> spread = read_doubles(f, T), stol32 = read_doubles(f, T), stol64 = read_doubles(f, T);
    std::fclose(f);

    std::vector<usize> tuples, pairs;
    std::vector<uint32_t> labels;
    for (double v : tup_d) tuples.push_back((usize)v);
    for (double v : pair_d) pairs.push_back((usize)v);
    for (double v : lab_d) labels.push_back((uint32_t)v);
    std::vector<float> x32(xyz.size());
    for (size_t i = 0; i < xyz.size(); ++i) x32[i] = (float)xyz[i];
    float box[9];
    for (int q = 0; q < 9; ++q) box[q] = (float)box_d[q];

    Engine &eng = Engine::global();
    InternalCoordsOptions opt;
    opt.nbins = (uint32_t)nbins;
    opt.map_bins = (uint32_t)mb;
    opt.ngroups = G;
    const InternalCoords got = internal_coords(eng, x32.data(), F, natoms, tuples, MOLAR_HIP_IC_DIHEDRAL, box, opt, labels, pairs);
    EXPECT(got.nframes == F && got.ntuples == T && got.ngroups == G && got.npair_groups == 1);
    EXPECT(differ(got.hist, hist) == 0);
    EXPECT(differ(got.map, map) == 0);
    EXPECT(differ(got.valid, valid) == 0);
    EXPECT(beyond(got.values, val, vtol32) == 0);
    EXPECT(beyond(got.mean, mean, mtol32) == 0);
    EXPECT(beyond(got.spread, spread, stol32) == 0);

    // the C call the wrapper forwards to: the same bits
    {
        molar_hip_intcoord_spec spec{};
        spec.kind = MOLAR_HIP_IC_DIHEDRAL;
        spec.nbins = (uint32_t)nbins;
        spec.map_bins = (uint32_t)mb;
        std::vector<float> v(F * T, -1.0f), m(T, -1.0f), s(T, -1.0f);
        std::vector<uint64_t> h(G * nbins, 7), mp(mb * mb, 7), n(T, 7);
        EXPECT(molar_hip_intcoord(eng.ctx(), x32.data(), F, natoms * 3, natoms, tuples.data(), T, labels.data(), G, box, 0, MOLAR_HIP_PBC_FULL, &spec,
                                  pairs.data(), P, nullptr, 1, v.data(), T, h.data(), mp.data(), m.data(), s.data(), n.data()) == 0);
        EXPECT(h == got.hist && mp == got.map && n == got.valid);
        EXPECT(std::memcmp(v.data(), got.values.data(), v.size() * sizeof(float)) == 0 && std::memcmp(m.data(), got.mean.data(), m.size() * sizeof(float)) == 0 &&
               std::memcmp(s.data(), got.spread.data(), s.size() * sizeof(float)) == 0);
    }

    // the histogram alone: nothing else is made
    {
        InternalCoordsOptions only = opt;
        only.want_values = false;
        only.want_stats = false;
        only.map_bins = 0;
        const InternalCoords h = internal_coords(eng, x32.data(), F, natoms, tuples, MOLAR_HIP_IC_DIHEDRAL, box, only, labels);
        EXPECT(h.hist == got.hist && h.values.empty() && h.map.empty() && h.mean.empty() && h.valid.empty());
    }

    // the f64 wrapper on the same numbers
    {
        std::vector<double> x64(xyz.size()), b64(9);
        for (size_t i = 0; i < xyz.size(); ++i) x64[i] = (double)x32[i];
        for (int k = 0; k < 9; ++k) b64[k] = (double)box[k];
        const InternalCoordsOf<double> e = internal_coords_f64(eng, x64.data(), F, natoms, tuples, MOLAR_HIP_IC_DIHEDRAL, b64.data(), opt, labels, pairs);
        EXPECT(differ(e.hist, hist) == 0 && differ(e.map, map) == 0 && differ(e.valid, valid) == 0);
        EXPECT(beyond(e.values, val, vtol64) == 0 && beyond(e.mean, mean, mtol64) == 0 && beyond(e.spread, spread, stol64) == 0);
    }

    bool threw = false;
    try { tuples.pop_back(); internal_coords(eng, x32.data(), F, natoms, tuples, MOLAR_HIP_IC_DIHEDRAL, box, opt); } catch (const MolarError &) { threw = true; }
    EXPECT(threw);
    threw = false;
    try { tuples.push_back((usize)natoms); internal_coords(eng, x32.data(), F, natoms, tuples, MOLAR_HIP_IC_DIHEDRAL, box, opt); } catch (const MolarError &e) {
        threw = e.code == MOLAR_HIP_ERR_INVALID_ARGUMENT;                                  // an index not below natoms
    }
    EXPECT(threw);

    std::printf("internal coordinates: %zu frames, %zu dihedrals in %zu groups, %zu pairs\n", F, T, G, P);
    if (failures) { std::printf("%d failure(s)\n", failures); return 1; }
    std::printf("all internal-coordinate host-mirror tests passed\n");
    return 0;
}
