// molar::fluctuations of the C++ host mirror (include/molar_hip.hpp) on one small case whose input and expected numbers the
// Python side writes (tests/test_cpp_fluct.py: the numpy reference of tests/fluct_ref.py with its bounds): every entry of the
// mean, the RMSF, the covariance and the per-frame RMSD within its bound, the covariance exactly symmetric, and the bits of
// the C call the wrapper forwards to.  The f64 wrapper on the same numbers, and the wrapper's own argument checks.
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
static size_t beyond(const std::vector<T> &got, const std::vector<double> &want, const std::vector<double> &tol, bool squared = false) {
    size_t bad = 0;
    for (size_t i = 0; i < want.size(); ++i) {
        const double g = squared ? (double)got[i] * (double)got[i] : (double)got[i], w = squared ? want[i] * want[i] : want[i];
        bad += !(std::fabs(g - w) <= tol[i]);
    }
    return bad;
}

int main(int argc, char **argv) {
    if (argc < 2) { std::printf("usage: test_fluct_gpu CASE_FILE\n"); return 2; }
    std::FILE *f = std::fopen(argv[1], "r");
    if (!f) { std::printf("cannot open %s\n", argv[1]); return 2; }
    size_t F, natoms, n;
    int iterations;
    if (std::fscanf(f, "%zu %zu %zu %d", &F, &natoms, &n, &iterations) != 4) return 2;
    const std::vector<double> idx_d = read_doubles(f, n), mass_d = read_doubles(f, natoms), xyz = read_doubles(f, F * natoms * 3);
    const size_t M = 3 * n;
    const std::vector<double> mean_w = read_doubles(f, M), mean_t = read_doubles(f, M), rmsf_w = read_doubles(f, n), rmsf2_t = read_doubles(f, n);
    const std::vector<double> cov_w = read_doubles(f, M * M), cov_t = read_doubles(f, M * M), rmsd_w = read_doubles(f, F), rmsd2_t = read_doubles(f, F);
    // the same bounds with eps_out of the f64 entry
    const std::vector<double> mean_t64 = read_doubles(f, M), rmsf2_t64 = read_doubles(f, n), cov_t64 = read_doubles(f, M * M), rmsd2_t64 = read_doubles(f, F);
    std::fclose(f);

    Topology top;
    State st;
    for (size_t i = 0; i < natoms; ++i) {
        st.coords.push_back(Pos{(float)xyz[3 * i], (float)xyz[3 * i + 1], (float)xyz[3 * i + 2]});
        top.masses.push_back((float)mass_d[i]);
    }
    System sys(top, st);
    std::vector<usize> index;
    for (double v : idx_d) index.push_back((usize)v);
    SelBound sel(sys, index);
    std::vector<Pos> frames;
    for (size_t i = 0; i < F * natoms; ++i) frames.push_back(Pos{(float)xyz[3 * i], (float)xyz[3 * i + 1], (float)xyz[3 * i + 2]});

    const Fluctuations got = fluctuations(sel, frames, nullptr, true, iterations, true, true);
    EXPECT(got.mean.size() == M && got.rmsf.size() == n && got.cov.size() == M * M && got.fit.size() == 13 * F);
    EXPECT(beyond(got.mean, mean_w, mean_t) == 0);
    EXPECT(beyond(got.rmsf, rmsf_w, rmsf2_t, true) == 0);
    EXPECT(beyond(got.cov, cov_w, cov_t) == 0);
    std::vector<float> rmsd(F);
    for (size_t a = 0; a < F; ++a) rmsd[a] = got.fit[13 * a + 12];
    EXPECT(beyond(rmsd, rmsd_w, rmsd2_t, true) == 0);
    size_t asym = 0;
    for (size_t i = 0; i < M; ++i)
        for (size_t j = 0; j < M; ++j) asym += std::memcmp(&got.cov[i * M + j], &got.cov[j * M + i], sizeof(float)) != 0;
    EXPECT(asym == 0);

    // the C call the wrapper forwards to: the same bits
    std::vector<float> mean(M, -1.0f), rmsf(n, -1.0f), cov(M * M, -1.0f), fit(13 * F, -1.0f);
    EXPECT(molar_hip_fluct(sel.ctx(), &frames[0].x, F, natoms * 3, natoms, index.data(), n, top.masses.data(), nullptr, 1, iterations, mean.data(),
                           rmsf.data(), cov.data(), M, fit.data()) == 0);
    EXPECT(std::memcmp(mean.data(), got.mean.data(), M * sizeof(float)) == 0 && std::memcmp(rmsf.data(), got.rmsf.data(), n * sizeof(float)) == 0);
    EXPECT(std::memcmp(cov.data(), got.cov.data(), M * M * sizeof(float)) == 0 && std::memcmp(fit.data(), got.fit.data(), 13 * F * sizeof(float)) == 0);

    // only what is asked for comes back; the reference given as frame 0's selection changes no bit
    std::vector<Pos> ref0;
    for (usize a : index) ref0.push_back(frames[a]);
    const Fluctuations lean = fluctuations(sel, frames, &ref0, true, iterations);
    EXPECT(lean.cov.empty() && lean.fit.empty());
    EXPECT(std::memcmp(lean.mean.data(), got.mean.data(), M * sizeof(float)) == 0 && std::memcmp(lean.rmsf.data(), got.rmsf.data(), n * sizeof(float)) == 0);

    // the f64 wrapper on the same numbers
    {
        std::vector<double> m64(natoms);
        for (size_t i = 0; i < natoms; ++i) m64[i] = (double)top.masses[i];
        std::vector<double> x64(xyz.size());
        for (size_t i = 0; i < xyz.size(); ++i) x64[i] = (double)(float)xyz[i];
        const FluctuationsOf<double> d = fluctuations_f64(Engine::global(), x64.data(), F, natoms, index, m64.data(), nullptr, true, iterations, true, true);
        EXPECT(beyond(d.mean, mean_w, mean_t64) == 0);
        EXPECT(beyond(d.rmsf, rmsf_w, rmsf2_t64, true) == 0);
        EXPECT(beyond(d.cov, cov_w, cov_t64) == 0);
        std::vector<double> r64(F);
        for (size_t a = 0; a < F; ++a) r64[a] = d.fit[13 * a + 12];
        EXPECT(beyond(r64, rmsd_w, rmsd2_t64, true) == 0);
    }

    bool threw = false;
    try { frames.pop_back(); fluctuations(sel, frames); } catch (const MolarError &) { threw = true; }
    EXPECT(threw);
    threw = false;
    try { frames.push_back(Pos{0.0f, 0.0f, 0.0f}); ref0.pop_back(); fluctuations(sel, frames, &ref0); } catch (const MolarError &) { threw = true; }
    EXPECT(threw);

    std::printf("fluctuations: %zu frames, %zu of %zu atoms, %d iterations\n", F, n, natoms, iterations);
    if (failures) { std::printf("%d failure(s)\n", failures); return 1; }
    std::printf("all fluctuations host-mirror tests passed\n");
    return 0;
}
