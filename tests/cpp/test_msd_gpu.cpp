// molar::msd of the C++ host mirror (include/molar_hip.hpp) on one small case whose input and expected numbers the Python
// side writes (tests/test_cpp_msd.py: the numpy reference of tests/msd_ref.py with its bounds): a wrapped walk in an
// orthorhombic box, groups of unequal sizes over a selection, a drift reference set, lateral components, every second origin.
// Every entry of msd, m4, the per-particle curves and the displacements within its bound, the bits of the C call the wrapper
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

// the number of entries beyond their bound
template <class T>
static size_t beyond(const std::vector<T> &got, const std::vector<double> &want, const std::vector<double> &tol) {
    size_t bad = got.size() != want.size();
    for (size_t i = 0; i < want.size() && i < got.size(); ++i) bad += !(std::fabs((double)got[i] - want[i]) <= tol[i]);
    return bad;
}

struct Expected {
    std::vector<double> msd, msd_t, m4, m4_t, par, par_t, disp, disp_t;
};

static Expected read_expected(std::FILE *f, size_t F, size_t P, size_t L) {
    Expected e;
    e.msd = read_doubles(f, L + 1);
    e.msd_t = read_doubles(f, L + 1);
    e.m4 = read_doubles(f, L + 1);
    e.m4_t = read_doubles(f, L + 1);
    e.par = read_doubles(f, P * (L + 1));
    e.par_t = read_doubles(f, P * (L + 1));
    e.disp = read_doubles(f, F * P * 3);
    e.disp_t = read_doubles(f, F * P * 3);
    return e;
}

int main(int argc, char **argv) {
    if (argc < 2) { std::printf("usage: test_msd_gpu CASE_FILE\n"); return 2; }
    std::FILE *f = std::fopen(argv[1], "r");
    if (!f) { std::printf("cannot open %s\n", argv[1]); return 2; }
    size_t F, natoms, n, P, nref, L, stride;
    unsigned dims;
    if (std::fscanf(f, "%zu %zu %zu %zu %zu %zu %zu %u", &F, &natoms, &n, &P, &nref, &L, &stride, &dims) != 8) return 2;
    const std::vector<double> idx_d = read_doubles(f, n), off_d = read_doubles(f, P + 1), ref_d = read_doubles(f, nref), mass_d = read_doubles(f, natoms);
    const std::vector<double> box_d = read_doubles(f, 9), xyz = read_doubles(f, F * natoms * 3);
    const Expected e32 = read_expected(f, F, P, L), e64 = read_expected(f, F, P, L);
    std::fclose(f);

    Topology top;
    State st;
    for (size_t i = 0; i < natoms; ++i) {
        st.coords.push_back(Pos{(float)xyz[3 * i], (float)xyz[3 * i + 1], (float)xyz[3 * i + 2]});
        top.masses.push_back((float)mass_d[i]);
    }
    System sys(top, st);
    std::vector<usize> index, offsets, refset;
    for (double v : idx_d) index.push_back((usize)v);
    for (double v : off_d) offsets.push_back((usize)v);
    for (double v : ref_d) refset.push_back((usize)v);
    SelBound sel(sys, index);
    std::vector<Pos> frames;
    for (size_t i = 0; i < F * natoms; ++i) frames.push_back(Pos{(float)xyz[3 * i], (float)xyz[3 * i + 1], (float)xyz[3 * i + 2]});
    float box[9];
    for (int q = 0; q < 9; ++q) box[q] = (float)box_d[q];

    MsdOptions opt;
    opt.max_lag = L;
    opt.origin_stride = stride;
    opt.dims = dims;
    opt.want_particle = true;
    opt.want_disp = true;
    const Msd got = msd(sel, frames, box, opt, offsets, refset);
    EXPECT(got.nparticles == P && got.max_lag == L);
    EXPECT(beyond(got.msd, e32.msd, e32.msd_t) == 0);
    EXPECT(beyond(got.m4, e32.m4, e32.m4_t) == 0);
    EXPECT(beyond(got.msd_particle, e32.par, e32.par_t) == 0);
    EXPECT(beyond(got.disp, e32.disp, e32.disp_t) == 0);
    EXPECT(got.msd[0] == 0.0f);

    // the C call the wrapper forwards to: the same bits
    std::vector<float> m(L + 1, -1.0f), q(L + 1, -1.0f), par(P * (L + 1), -1.0f), disp(F * P * 3, -1.0f);
    EXPECT(molar_hip_msd(sel.ctx(), &frames[0].x, F, natoms * 3, natoms, index.data(), n, top.masses.data(), box, 0, MOLAR_HIP_PBC_FULL, offsets.data(), P,
                         refset.data(), nref, L, stride, dims, m.data(), q.data(), par.data(), L + 1, disp.data()) == 0);
    EXPECT(std::memcmp(m.data(), got.msd.data(), m.size() * sizeof(float)) == 0 && std::memcmp(q.data(), got.m4.data(), q.size() * sizeof(float)) == 0);
    EXPECT(std::memcmp(par.data(), got.msd_particle.data(), par.size() * sizeof(float)) == 0);
    EXPECT(std::memcmp(disp.data(), got.disp.data(), disp.size() * sizeof(float)) == 0);

    // only what is asked for comes back
    MsdOptions lean_opt = opt;
    lean_opt.want_particle = lean_opt.want_disp = false;
    const Msd lean = msd(sel, frames, box, lean_opt, offsets, refset);
    EXPECT(lean.msd_particle.empty() && lean.disp.empty());
    EXPECT(std::memcmp(lean.msd.data(), got.msd.data(), m.size() * sizeof(float)) == 0);

    // the f64 wrapper on the same numbers
    {
        std::vector<double> m64(natoms), x64(xyz.size()), b64(9);
        for (size_t i = 0; i < natoms; ++i) m64[i] = (double)top.masses[i];
        for (size_t i = 0; i < xyz.size(); ++i) x64[i] = (double)(float)xyz[i];
        for (int k = 0; k < 9; ++k) b64[k] = (double)box[k];
        const MsdOf<double> d = msd_f64(Engine::global(), x64.data(), F, natoms, index, m64.data(), b64.data(), opt, offsets, refset);
        EXPECT(beyond(d.msd, e64.msd, e64.msd_t) == 0);
        EXPECT(beyond(d.m4, e64.m4, e64.m4_t) == 0);
        EXPECT(beyond(d.msd_particle, e64.par, e64.par_t) == 0);
        EXPECT(beyond(d.disp, e64.disp, e64.disp_t) == 0);
    }

    bool threw = false;
    try { frames.pop_back(); msd(sel, frames, box, opt, offsets, refset); } catch (const MolarError &) { threw = true; }
    EXPECT(threw);
    threw = false;
    try { frames.push_back(Pos{0.0f, 0.0f, 0.0f}); opt.max_lag = F; msd(sel, frames, box, opt, offsets, refset); } catch (const MolarError &) { threw = true; }
    EXPECT(threw);

    std::printf("msd: %zu frames, %zu particles of %zu selected atoms, %zu lags\n", F, P, n, L + 1);
    if (failures) { std::printf("%d failure(s)\n", failures); return 1; }
    std::printf("all msd host-mirror tests passed\n");
    return 0;
}
