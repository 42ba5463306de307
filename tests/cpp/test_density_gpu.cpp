// molar::density of the C++ host mirror (include/molar_hip.hpp) on one small case whose input and expected numbers the Python
// side writes (tests/test_cpp_density.py: the numpy reference of tests/density_ref.py with its bounds): a mass density profile
// along z of three groups over a selection with gaps, in an orthorhombic box.  The counts, the dropped atoms and the weights'
// scale for equality, every density entry within its bound, the bits of the C call the wrapper forwards to, the f64 wrapper on
// the same numbers, and the wrapper's own argument check.
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
    if (argc < 2) { std::printf("usage: test_density_gpu CASE_FILE\n"); return 2; }
    std::FILE *f = std::fopen(argv[1], "r");
    if (!f) { std::printf("cannot open %s\n", argv[1]); return 2; }
    size_t F, natoms, n, nz, G;
    int S;
    if (std::fscanf(f, "%zu %zu %zu %zu %zu %d", &F, &natoms, &n, &nz, &G, &S) != 6) return 2;
    const std::vector<double> idx_d = read_doubles(f, n), lab_d = read_doubles(f, n), mass_d = read_doubles(f, natoms), box_d = read_doubles(f, 9);
    const std::vector<double> xyz = read_doubles(f, F * natoms * 3), count = read_doubles(f, G * nz), outside = read_doubles(f, F);
    const std::vector<double> dens = read_doubles(f, G * nz), tol32 = read_doubles(f, G * nz), tol64 = read_doubles(f, G * nz);
    std::fclose(f);

    Topology top;
    State st;
    for (size_t i = 0; i < natoms; ++i) {
        st.coords.push_back(Pos{(float)xyz[3 * i], (float)xyz[3 * i + 1], (float)xyz[3 * i + 2]});
        top.masses.push_back((float)mass_d[i]);
    }
    System sys(top, st);
    std::vector<usize> index;
    std::vector<uint32_t> labels;
    for (double v : idx_d) index.push_back((usize)v);
    for (double v : lab_d) labels.push_back((uint32_t)v);
    SelBound sel(sys, index);
    std::vector<Pos> frames;
    for (size_t i = 0; i < F * natoms; ++i) frames.push_back(Pos{(float)xyz[3 * i], (float)xyz[3 * i + 1], (float)xyz[3 * i + 2]});
    float box[9];
    for (int q = 0; q < 9; ++q) box[q] = (float)box_d[q];

    const molar_hip_density_grid grid = profile_grid(2, (uint32_t)nz);
    EXPECT(grid.mode == MOLAR_HIP_DENSITY_BOX && grid.nbins[0] == 1 && grid.nbins[2] == nz && grid.centre_dims == 0);
    DensityOptions opt;
    opt.mass_weighted = true;
    opt.ngroups = G;
    const Density got = density(sel, frames, grid, box, opt, labels);
    EXPECT(got.ngroups == G && got.nbins == nz && got.weight_scale_log2 == S);
    EXPECT(differ(got.count, count) == 0);
    EXPECT(differ(got.outside, outside) == 0);
    EXPECT(beyond(got.density, dens, tol32) == 0);
    for (size_t fr = 0; fr < F; ++fr) EXPECT(got.centre[3 * fr + 2] == 0.0f && std::fabs(got.binvol[fr] - 3.0 * 3.5 * 4.0 / (double)nz) <= 1e-6);

    // the C call the wrapper forwards to: the same bits
    std::vector<float> d(G * nz, -1.0f), cen(F * 3, -1.0f), bv(F, -1.0f);
    std::vector<uint64_t> cnt(G * nz, 7), outs(F, 7);
    int32_t s2 = -1;
    EXPECT(molar_hip_density(sel.ctx(), &frames[0].x, F, natoms * 3, natoms, index.data(), n, top.masses.data(), labels.data(), G, box, 0, MOLAR_HIP_PBC_FULL,
                             &grid, nullptr, 0, nullptr, d.data(), cnt.data(), outs.data(), cen.data(), bv.data(), &s2) == 0);
    EXPECT(s2 == S && cnt == got.count && outs == got.outside);
    EXPECT(std::memcmp(d.data(), got.density.data(), d.size() * sizeof(float)) == 0 && std::memcmp(bv.data(), got.binvol.data(), bv.size() * sizeof(float)) == 0);

    // centred on the selection itself: the centre comes back, and nothing is outside in a periodic cell
    const Density centred = density(sel, frames, profile_grid(2, (uint32_t)nz, true), box, opt, labels, index);
    uint64_t total = 0;
    for (uint64_t v : centred.count) total += v;
    EXPECT(total == F * n && centred.centre[2] >= 0.0f && centred.centre[2] <= 1.0f && centred.centre[0] == 0.0f);

    // the f64 wrapper on the same numbers
    {
        std::vector<double> m64(natoms), x64(xyz.size()), b64(9);
        for (size_t i = 0; i < natoms; ++i) m64[i] = (double)top.masses[i];
        for (size_t i = 0; i < xyz.size(); ++i) x64[i] = (double)(float)xyz[i];
        for (int k = 0; k < 9; ++k) b64[k] = (double)box[k];
        const DensityOf<double> e = density_f64(Engine::global(), x64.data(), F, natoms, index, grid, m64.data(), b64.data(), opt, labels);
        EXPECT(e.weight_scale_log2 == S && differ(e.count, count) == 0 && differ(e.outside, outside) == 0);
        EXPECT(beyond(e.density, dens, tol64) == 0);
    }

    bool threw = false;
    try { frames.pop_back(); density(sel, frames, grid, box, opt, labels); } catch (const MolarError &) { threw = true; }
    EXPECT(threw);
    threw = false;
    try { frames.push_back(Pos{0.0f, 0.0f, 0.0f}); density(sel, frames, grid, nullptr, opt, labels); } catch (const MolarError &) { threw = true; }      // BOX mode without boxes
    EXPECT(threw);

    std::printf("density: %zu frames, %zu groups of %zu selected atoms, %zu bins\n", F, G, n, nz);
    if (failures) { std::printf("%d failure(s)\n", failures); return 1; }
    std::printf("all density host-mirror tests passed\n");
    return 0;
}
