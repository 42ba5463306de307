// SelBound::sasa_vol (include/molar_hip.hpp -> molar_hip_sasa_vol) against a brute-force restatement of the definition in
// include/molar_hip.h, in float with the same operations: the areas must equal those of SelBound::sasa bit for bit, the
// volumes agree to 1e-6 relative (+ 1e-12 of the ball), the total with the double sum of the volumes to 1e-12.  A topology
// without radii must be refused.
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
    uint32_t seed = 777u;
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
    const Sasa got = sel.sasa_vol(probe, npoints);
    const Sasa area = sel.sasa(probe, npoints);
    const size_t n = index.size();
    EXPECT(got.areas.size() == n && got.volumes.size() == n && area.volumes.empty());
    EXPECT(got.areas == area.areas && got.total_area == area.total_area);

    std::vector<float> u(3 * npoints);
    EXPECT(molar_hip_sasa_points(npoints, u.data()) == 0);
    std::vector<float> R(n);
    for (size_t k = 0; k < n; ++k) R[k] = top.vdw[index[k]] + probe;
    double sum = 0.0;
    size_t hidden = 0, cut = 0, worse = 0;
    std::vector<float> lo(npoints), hi(npoints);
    for (size_t i = 0; i < n; ++i) {
        const Pos ci = st.coords[index[i]];
        for (uint32_t k = 0; k < npoints; ++k) { lo[k] = 0.0f; hi[k] = R[i]; }
        for (size_t j = 0; j < n; ++j) {
            if (j == i) continue;
            const Pos cj = st.coords[index[j]];
            const float dx = cj.x - ci.x, dy = cj.y - ci.y, dz = cj.z - ci.z;
            const float dd = (dx * dx + dy * dy) + dz * dz, lim = R[i] + R[j];
            if (!(dd < lim * lim)) continue;
            const float c = ((dd + R[i] * R[i]) - R[j] * R[j]) * 0.5f;
            for (uint32_t k = 0; k < npoints; ++k) {
                const float a = (u[3 * k] * dx + u[3 * k + 1] * dy) + u[3 * k + 2] * dz;
                const float t = c / a;
                if (a > 0.0f) {
                    if (t < hi[k]) hi[k] = t;
                } else if (a < 0.0f) {
                    if (t > lo[k]) lo[k] = t;
                } else if (a == 0.0f && c < 0.0f) {
                    hi[k] = 0.0f;
                }
            }
        }
        double s = 0.0;
        for (uint32_t k = 0; k < npoints; ++k) {
            const double h = (double)(hi[k] < lo[k] ? lo[k] : hi[k]), l = (double)lo[k];
            s += (h * h) * h - (l * l) * l;
        }
        const float want = (float)((((4.0 * 3.14159265358979323846) / 3.0) * s) / (double)npoints);
        const double Rd = (double)R[i], ball = ((4.0 * 3.14159265358979323846) / 3.0) * Rd * Rd * Rd;
        if (want == 0.0f) ++hidden;
        if (want > 0.0f && (double)want < 0.9 * ball) ++cut;
        if (!(std::fabs((double)got.volumes[i] - (double)want) <= 1e-6 * (double)want + 1e-12 * ball)) ++worse;
        sum += (double)got.volumes[i];
    }
    EXPECT(worse == 0);
    EXPECT(cut > 100);
    EXPECT(std::fabs(got.total_volume - sum) <= 1e-12 * std::fabs(sum));
    std::printf("SelBound::sasa_vol: %zu atoms, %zu cut, %zu hidden, total %.6f nm^3\n", n, cut, hidden, got.total_volume);

    Topology bare;
    bare.masses = top.masses;
    System sys2(bare, st);
    bool threw = false;
    try { SelBound::all(sys2).sasa_vol(); } catch (const MolarError &) { threw = true; }
    EXPECT(threw);

    if (failures) { std::printf("%d failure(s)\n", failures); return 1; }
    std::printf("all sasa_vol host-mirror tests passed\n");
    return 0;
}
