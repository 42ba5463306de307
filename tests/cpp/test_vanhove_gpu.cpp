// molar::van_hove of the C++ host mirror (include/molar_hip.hpp) on one small shape against counts computed here, with the
// arithmetic of the definition in molar_hip.h (the differences in double, r2 by std::fma in the order x, y, z, std::sqrt, the
// DISTANCE bin formula): an index, two groups with unsorted labels, a particle with a NaN, an origin stride; then the signed
// mode, the f64 wrapper on the same numbers, the bits of the C call the wrapper forwards to, and the wrapper's own argument check.
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

struct Counts {
    std::vector<uint64_t> hist, outside, norigins, nvalid;
    std::vector<uint32_t> bad;
};

static Counts expected(const std::vector<float> &x, size_t F, size_t natoms, const std::vector<usize> &index, const std::vector<uint32_t> &labels, size_t G,
                       const std::vector<uint64_t> &lags, const VanHoveOptions &opt) {
    const size_t n = index.size(), L = lags.size();
    Counts c;
    c.hist.assign(G * L * opt.nbins, 0);
    c.outside.assign(G * L, 0);
    c.norigins.assign(L, 0);
    c.nvalid.assign(G, 0);
    c.bad.assign(n, 0);
    for (size_t l = 0; l < L; ++l) c.norigins[l] = (F - 1 - lags[l]) / opt.origin_stride + 1;
    for (size_t k = 0; k < n; ++k) {
        const size_t a = index[k], g = labels[k];
        for (size_t f = 0; f < F; ++f) {
            bool fin = true;
            for (int d = 0; d < 3; ++d)
                if ((opt.dims >> d & 1u) && !std::isfinite(x[(f * natoms + a) * 3 + d])) fin = false;
            c.bad[k] += !fin;
        }
        if (c.bad[k]) continue;
        ++c.nvalid[g];
        for (size_t l = 0; l < L; ++l)
            for (size_t t = 0; t + lags[l] <= F - 1; t += opt.origin_stride) {
                double r2 = 0.0, v = 0.0;
                for (int d = 0; d < 3; ++d)
                    if (opt.dims >> d & 1u) {
                        const double e = (double)x[((t + lags[l]) * natoms + a) * 3 + d] - (double)x[(t * natoms + a) * 3 + d];
                        r2 = std::fma(e, e, r2);
                        v = e;
                    }
                if (!opt.is_signed) v = std::sqrt(r2);
                if (v >= opt.lo && v < opt.hi) {
                    const double fb = std::floor((v - opt.lo) / (opt.hi - opt.lo) * (double)opt.nbins);
                    size_t bin = fb > 0.0 ? (size_t)fb : 0;
                    if (bin > opt.nbins - 1) bin = opt.nbins - 1;
                    ++c.hist[(g * L + l) * opt.nbins + bin];
                } else {
                    ++c.outside[g * L + l];
                }
            }
    }
    return c;
}

static bool same(const VanHove &got, const Counts &want) {
    return got.hist == want.hist && got.outside == want.outside && got.norigins == want.norigins && got.nvalid == want.nvalid && got.bad == want.bad;
}

int main() {
    const size_t F = 40, natoms = 11, G = 2;
    std::vector<float> x(F * natoms * 3);
    uint32_t s = 12345u;
    auto rnd = [&]() { s = s * 1664525u + 1013904223u; return (double)(s >> 8) / 16777216.0 - 0.5; };
    std::vector<double> pos(natoms * 3);
    for (double &p : pos) p = 3.0 * rnd();
    for (size_t f = 0; f < F; ++f)
        for (size_t i = 0; i < natoms * 3; ++i) {
            if (f) pos[i] += 0.3 * rnd();
            x[f * natoms * 3 + i] = (float)pos[i];
        }
    x[(7 * natoms + 4) * 3 + 1] = std::nanf("");                              // particle 4, frame 7
    const std::vector<usize> index = {10, 0, 4, 3, 8, 2, 9, 6, 5};
    const std::vector<uint32_t> labels = {1, 0, 1, 1, 0, 0, 1, 0, 1};
    const std::vector<uint64_t> lags = {0, 1, 7, 39};

    Engine &eng = Engine::global();
    VanHoveOptions opt;
    opt.lo = 0.05;
    opt.hi = 1.1;
    opt.nbins = 8;
    opt.origin_stride = 3;
    opt.ngroups = G;
    const VanHove got = van_hove(eng, x.data(), F, natoms, lags, opt, index, labels);
    const Counts want = expected(x, F, natoms, index, labels, G, lags, opt);
    EXPECT(got.ngroups == G && got.nlags == lags.size() && got.nbins == 8 && got.edges.size() == 9 && got.edges[0] == 0.05 && got.edges[8] == 1.1);
    EXPECT(same(got, want));
    EXPECT(want.bad[2] == 1 && want.nvalid[0] == 4 && want.nvalid[1] == 4);
    uint64_t inside = 0, out = 0;
    for (uint64_t v : want.hist) inside += v;
    for (uint64_t v : want.outside) out += v;
    EXPECT(inside > 0 && out > 0);
    for (size_t g = 0; g < G; ++g)
        for (size_t l = 0; l < lags.size(); ++l) {
            uint64_t sum = got.outside[g * lags.size() + l];
            for (size_t b = 0; b < 8; ++b) sum += got.hist[(g * lags.size() + l) * 8 + b];
            EXPECT(sum == got.nvalid[g] * got.norigins[l]);
        }

    // the C call the wrapper forwards to: the same counts
    {
        std::vector<uint64_t> h(got.hist.size(), 7), o(got.outside.size(), 7);
        EXPECT(molar_hip_vanhove(eng.ctx(), x.data(), F, natoms * 3, natoms, index.data(), index.size(), labels.data(), G, lags.data(), lags.size(), 3, 7, 0, 0.05, 1.1,
                                 8, h.data(), o.data(), nullptr, nullptr, nullptr) == 0);
        EXPECT(h == got.hist && o == got.outside);
    }

    // signed, one component, one group, every particle
    {
        VanHoveOptions so;
        so.lo = -0.73;
        so.hi = 0.91;
        so.nbins = 7;
        so.dims = 4;
        so.is_signed = true;
        std::vector<usize> all(natoms);
        for (size_t i = 0; i < natoms; ++i) all[i] = i;
        const VanHove r = van_hove(eng, x.data(), F, natoms, lags, so);
        EXPECT(same(r, expected(x, F, natoms, all, std::vector<uint32_t>(natoms, 0), 1, lags, so)));
        EXPECT(r.bad[4] == 0);                                               // the NaN is in y, which dims leaves out
    }

    // the f64 wrapper on the same numbers
    {
        std::vector<double> x64(x.begin(), x.end());
        EXPECT(same(van_hove_f64(eng, x64.data(), F, natoms, lags, opt, index, labels), want));
    }

    bool threw = false;
    try { std::vector<uint32_t> l2(labels.begin(), labels.end() - 1); van_hove(eng, x.data(), F, natoms, lags, opt, index, l2); } catch (const MolarError &) { threw = true; }
    EXPECT(threw);
    threw = false;
    try { van_hove(eng, x.data(), F, natoms, {0, 40}, opt, index, labels); } catch (const MolarError &e) { threw = e.code == MOLAR_HIP_ERR_INVALID_ARGUMENT; }
    EXPECT(threw);

    if (failures) { std::printf("%d failure(s)\n", failures); return 1; }
    std::printf("all van Hove host-mirror tests passed\n");
    return 0;
}
