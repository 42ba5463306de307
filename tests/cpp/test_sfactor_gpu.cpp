// molar::structure_factor of the C++ host mirror (include/molar_hip.hpp) on one small case whose input and expected numbers
// the Python side writes (tests/test_cpp_sfactor.py: the longdouble reference of tests/sfactor_ref.py with its bounds): two
// species with weights of both signs in a triclinic box, a selection, shells.  The ok frames and the shell counts for equality,
// rho, its mean, S_ab and the shells within their bounds (NaN where the reference is NaN), the bits of the C call the wrapper
// forwards to, the f64 wrapper on the same numbers, and the wrapper's own argument check.
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

// the number of entries beyond their bound; a NaN is expected exactly where the reference has one
template <class T>
static size_t beyond(const std::vector<T> &got, const std::vector<double> &want, const std::vector<double> &tol) {
    size_t bad = got.size() != want.size();
    for (size_t i = 0; i < want.size() && i < got.size(); ++i) {
        if (std::isnan(want[i])) bad += !std::isnan((double)got[i]);
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
    if (argc < 2) { std::printf("usage: test_sfactor_gpu CASE_FILE\n"); return 2; }
    std::FILE *f = std::fopen(argv[1], "r");
    if (!f) { std::printf("cannot open %s\n", argv[1]); return 2; }
    size_t F, natoms, n, G, H, K, L, ns;
    double qmin, dq;
    if (std::fscanf(f, "%zu %zu %zu %zu %zu %zu %zu %zu %lf %lf", &F, &natoms, &n, &G, &H, &K, &L, &ns, &qmin, &dq) != 10) return 2;
    const size_t Q = (H + 1) * (2 * K + 1) * (2 * L + 1), P = G * (G + 1) / 2;
    const std::vector<double> idx_d = read_doubles(f, n), lab_d = read_doubles(f, n), w_d = read_doubles(f, natoms), box_d = read_doubles(f, 9);
    const std::vector<double> xyz = read_doubles(f, F * natoms * 3), ok = read_doubles(f, F), count = read_doubles(f, ns);
    const Expected rho = read_expected(f, F * G * Q * 2), mean = read_expected(f, G * Q * 2), sab = read_expected(f, P * Q), shell = read_expected(f, P * ns);
    std::fclose(f);

    std::vector<usize> idx;
    std::vector<uint32_t> labels;
    for (double v : idx_d) idx.push_back((usize)v);
    for (double v : lab_d) labels.push_back((uint32_t)v);
    std::vector<float> x32(xyz.size()), w32(natoms);
    for (size_t i = 0; i < xyz.size(); ++i) x32[i] = (float)xyz[i];
    for (size_t i = 0; i < natoms; ++i) w32[i] = (float)w_d[i];
    float box[9];
    for (int q = 0; q < 9; ++q) box[q] = (float)box_d[q];

    Engine &eng = Engine::global();
    StructureFactorOptions opt;
    opt.hmax[0] = (uint32_t)H;
    opt.hmax[1] = (uint32_t)K;
    opt.hmax[2] = (uint32_t)L;
    opt.qmin = qmin;
    opt.dq = dq;
    opt.nshells = (uint32_t)ns;
    opt.ngroups = G;
    opt.want_rho = true;
    opt.want_mean = true;
    const StructureFactor got = structure_factor(eng, x32.data(), F, natoms, box, opt, idx, w32, labels);
    EXPECT(got.nframes == F && got.ngroups == G && got.npairs == P && got.nq == Q && got.nshells == ns);
    EXPECT(differ(got.frame_ok, ok) == 0);
    EXPECT(differ(got.shell_count, count) == 0);
    EXPECT(beyond(got.rho, rho.want, rho.tol32) == 0);
    EXPECT(beyond(got.rho_mean, mean.want, mean.tol32) == 0);
    EXPECT(beyond(got.sab, sab.want, sab.tol32) == 0);
    EXPECT(beyond(got.shell, shell.want, shell.tol32) == 0);

    // the C call the wrapper forwards to: the same bits
    {
        molar_hip_sfactor_grid grid{};
        grid.hmax[0] = (uint32_t)H;
        grid.hmax[1] = (uint32_t)K;
        grid.hmax[2] = (uint32_t)L;
        grid.qmin = qmin;
        grid.dq = dq;
        grid.nshells = (uint32_t)ns;
        std::vector<float> s(P * Q, -1.0f), sh(P * ns, -1.0f);
        std::vector<uint64_t> c(ns, 7);
        std::vector<uint32_t> fo(F, 7);
        EXPECT(molar_hip_sfactor(eng.ctx(), x32.data(), F, natoms * 3, natoms, idx.data(), n, w32.data(), labels.data(), G, box, 0, &grid, nullptr, 0, fo.data(),
                                 nullptr, s.data(), sh.data(), c.data()) == 0);
        EXPECT(c == got.shell_count && fo == got.frame_ok);
        EXPECT(std::memcmp(s.data(), got.sab.data(), s.size() * sizeof(float)) == 0 && std::memcmp(sh.data(), got.shell.data(), sh.size() * sizeof(float)) == 0);
    }

    // S_ab alone, without shells: nothing else is made
    {
        StructureFactorOptions only = opt;
        only.want_rho = false;
        only.want_mean = false;
        only.nshells = 0;
        const StructureFactor r = structure_factor(eng, x32.data(), F, natoms, box, only, idx, w32, labels);
        EXPECT(r.rho.empty() && r.rho_mean.empty() && r.shell.empty() && r.shell_count.empty() && r.sab.size() == P * Q);
        EXPECT(std::memcmp(r.sab.data(), got.sab.data(), r.sab.size() * sizeof(float)) == 0);
    }

    // the f64 wrapper on the same numbers
    {
        std::vector<double> x64(xyz.size()), w64(natoms), b64(9);
        for (size_t i = 0; i < xyz.size(); ++i) x64[i] = (double)x32[i];
        for (size_t i = 0; i < natoms; ++i) w64[i] = (double)w32[i];
        for (int k = 0; k < 9; ++k) b64[k] = (double)box[k];
        const StructureFactorOf<double> e = structure_factor_f64(eng, x64.data(), F, natoms, b64.data(), opt, idx, w64, labels);
        EXPECT(differ(e.frame_ok, ok) == 0 && differ(e.shell_count, count) == 0);
        EXPECT(beyond(e.rho, rho.want, rho.tol64) == 0 && beyond(e.rho_mean, mean.want, mean.tol64) == 0 && beyond(e.sab, sab.want, sab.tol64) == 0 &&
               beyond(e.shell, shell.want, shell.tol64) == 0);
    }

    bool threw = false;
    try { labels.pop_back(); structure_factor(eng, x32.data(), F, natoms, box, opt, idx, w32, labels); } catch (const MolarError &) { threw = true; }
    EXPECT(threw);
    threw = false;
    try { labels.push_back((uint32_t)G); structure_factor(eng, x32.data(), F, natoms, box, opt, idx, w32, labels); } catch (const MolarError &e) {
        threw = e.code == MOLAR_HIP_ERR_INVALID_ARGUMENT;                                  // a label not below ngroups
    }
    EXPECT(threw);

    std::printf("structure factor: %zu frames, %zu atoms in %zu groups, %zu lattice points, %zu shells\n", F, n, G, Q, ns);
    if (failures) { std::printf("%d failure(s)\n", failures); return 1; }
    std::printf("all structure-factor host-mirror tests passed\n");
    return 0;
}
