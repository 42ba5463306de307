// SelBound::sasa (include/molar_hip.hpp -> molar_hip_sasa) against a brute-force restatement of the definition in
// include/molar_hip.h, in float with the same operation order: the areas must agree to 1e-6 relative, the total with the
// double sum of the areas to 1e-12.  A topology without radii must be refused.
#include <cmath>
#include <cstdio>
#include <vector>

#include "molar_hip.hpp"

using namespace molar;

static int failures = 0;
#define EXPECT(cond)                                                         \
    do {                                                                     \
        if (!(cond)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

int main() {
    const size_t natoms = 600;
    const uint32_t npoints = 96;
    const float probe = 0.14f;
    uint32_t seed = 4242u;
    auto rnd = [&]() { seed = seed * 1664525u + 1013904223u; return ((seed >> 8) & 0xFFFF) / 65536.0f; };
    const float radii[5] = {0.12f, 0.152f, 0.155f, 0.17f, 0.18f};
    Topology top;
    State st;
    for (size_t i = 0; i < natoms; ++i) {
        st.coords.push_back(Pos{1.8f * rnd(), 1.8f * rnd(), 1.8f * rnd()});       // about 100 atoms / nm^3
        top.masses.push_back(12.0f);
        top.vdw.push_back(radii[(seed >> 20) % 5]);
    }
    System sys(top, st);
    std::vector<usize> index;
    for (size_t i = 0; i < natoms; ++i)
        if (i % 5 != 2) index.push_back(i);
    SelBound sel(sys, index);
    const Sasa got = sel.sasa(probe, npoints);
    EXPECT(got.areas.size() == index.size());

    std::vector<float> u(3 * npoints);
    EXPECT(molar_hip_sasa_points(npoints, u.data()) == 0);
    const size_t n = index.size();
    std::vector<float> R(n);
    for (size_t k = 0; k < n; ++k) R[k] = top.vdw[index[k]] + probe;
    double sum = 0.0;
    size_t partial = 0, worse = 0;
    for (size_t i = 0; i < n; ++i) {
        const Pos ci = st.coords[index[i]];
        std::vector<char> buried(npoints, 0);
        for (size_t j = 0; j < n; ++j) {
            if (j == i) continue;
            const Pos cj = st.coords[index[j]];
            const float dx = cj.x - ci.x, dy = cj.y - ci.y, dz = cj.z - ci.z;
            const float d2 = (dx * dx + dy * dy) + dz * dz, lim = R[i] + R[j];
            if (!(d2 < lim * lim)) continue;
            const float Rj2 = R[j] * R[j];
            for (uint32_t k = 0; k < npoints; ++k) {
                const float tx = R[i] * u[3 * k] - dx, ty = R[i] * u[3 * k + 1] - dy, tz = R[i] * u[3 * k + 2] - dz;
                if ((tx * tx + ty * ty) + tz * tz < Rj2) buried[k] = 1;
            }
        }
        uint32_t ex = 0;
        for (uint32_t k = 0; k < npoints; ++k) ex += buried[k] ? 0u : 1u;
        const double Rd = (double)R[i];
        const float want = (float)((((4.0 * 3.14159265358979323846) * (Rd * Rd)) * (double)ex) / (double)npoints);
        if (ex > 0 && ex < npoints) ++partial;
        if (std::fabs((double)got.areas[i] - (double)want) > 1e-6 * std::fabs((double)want)) ++worse;
        sum += (double)got.areas[i];
    }
    EXPECT(worse == 0);
    EXPECT(partial > 20);
    EXPECT(std::fabs(got.total_area - sum) <= 1e-12 * std::fabs(sum));
    std::printf("SelBound::sasa: %zu atoms, %zu partly exposed, total %.6f nm^2\n", n, partial, got.total_area);

    Topology bare;
    bare.masses = top.masses;
    System sys2(bare, st);
    bool threw = false;
    try { SelBound::all(sys2).sasa(); } catch (const MolarError &) { threw = true; }
    EXPECT(threw);

    if (failures) { std::printf("%d failure(s)\n", failures); return 1; }
    std::printf("all sasa host-mirror tests passed\n");
    return 0;
}
