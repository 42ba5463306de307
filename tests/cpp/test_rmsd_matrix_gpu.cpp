// molar::rmsd_matrix of the C++ host mirror (include/molar_hip.hpp) against the C call it forwards to: the same bits on one
// symmetric and one rectangular case, mass-weighted over a selection with gaps; the symmetric matrix is exactly symmetric with
// a zero diagonal, and a rigid copy of a frame comes out as (nearly) zero.
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

int main() {
    const size_t natoms = 300, F1 = 21, F2 = 9;
    uint32_t seed = 4242u;
    auto rnd = [&]() { seed = seed * 1664525u + 1013904223u; return ((seed >> 8) & 0xFFFF) / 65536.0f; };
    Topology top;
    State st;
    for (size_t i = 0; i < natoms; ++i) {
        st.coords.push_back(Pos{2.0f * rnd(), 2.0f * rnd(), 2.0f * rnd()});
        top.masses.push_back(1.0f + 15.0f * rnd());
    }
    System sys(top, st);
    std::vector<usize> index;
    for (size_t i = 0; i < natoms; ++i)
        if (i % 7 != 3) index.push_back(i);
    SelBound sel(sys, index);
    std::vector<Pos> frames1, frames2;
    for (size_t f = 0; f < F1; ++f)
        for (size_t i = 0; i < natoms; ++i) frames1.push_back(Pos{st.coords[i].x + 0.3f * rnd(), st.coords[i].y + 0.3f * rnd(), st.coords[i].z + 0.3f * rnd()});
    // frame 1 of the first block: frame 0 turned by 90 degrees about z and shifted
    for (size_t i = 0; i < natoms; ++i) frames1[natoms + i] = Pos{-frames1[i].y + 5.0f, frames1[i].x - 2.0f, frames1[i].z + 1.0f};
    for (size_t f = 0; f < F2; ++f)
        for (size_t i = 0; i < natoms; ++i) frames2.push_back(Pos{st.coords[i].x + 0.5f * rnd(), st.coords[i].y + 0.5f * rnd(), st.coords[i].z + 0.5f * rnd()});

    const std::vector<Float> symm = rmsd_matrix(sel, frames1);
    EXPECT(symm.size() == F1 * F1);
    std::vector<float> want(F1 * F1, -1.0f);
    EXPECT(molar_hip_rmsd_matrix(sel.ctx(), &frames1[0].x, F1, natoms * 3, nullptr, 0, 0, natoms, index.data(), index.size(), top.masses.data(), 1,
                                 want.data(), F1) == 0);
    EXPECT(std::memcmp(symm.data(), want.data(), want.size() * sizeof(float)) == 0);
    size_t asym = 0, diag = 0, small = 0;
    for (size_t a = 0; a < F1; ++a) {
        diag += symm[a * F1 + a] != 0.0f;
        for (size_t b = 0; b < F1; ++b) {
            asym += std::memcmp(&symm[a * F1 + b], &symm[b * F1 + a], sizeof(float)) != 0;
            small += a != b && !(symm[a * F1 + b] > 0.05f);
        }
    }
    EXPECT(asym == 0 && diag == 0);
    EXPECT(small == 2);                            // only the rigid copy and its mirror entry
    EXPECT(symm[1] < 1e-5f);                       // the float rounding of the rotated copy, nothing more

    const std::vector<Float> rect = rmsd_matrix(sel, frames1, &frames2, true, false);
    EXPECT(rect.size() == F1 * F2);
    std::vector<float> wide(F1 * (F2 + 3), -1.0f);
    EXPECT(molar_hip_rmsd_matrix(sel.ctx(), &frames1[0].x, F1, natoms * 3, &frames2[0].x, F2, natoms * 3, natoms, index.data(), index.size(), nullptr, 1,
                                 wide.data(), F2 + 3) == 0);
    size_t differ = 0, touched = 0;
    for (size_t a = 0; a < F1; ++a) {
        differ += std::memcmp(&rect[a * F2], &wide[a * (F2 + 3)], F2 * sizeof(float)) != 0;
        for (size_t b = F2; b < F2 + 3; ++b) touched += wide[a * (F2 + 3) + b] != -1.0f;
    }
    EXPECT(differ == 0 && touched == 0);
    std::printf("rmsd_matrix: %zu x %zu symmetric, %zu x %zu rectangular, rigid copy %.3g nm\n", F1, F1, F1, F2, (double)symm[1]);

    // the f64 wrapper: an empty index is the identity selection, and the bits are the C call's
    {
        std::vector<double> d1(frames1.size() * 3);
        for (size_t i = 0; i < frames1.size(); ++i) { d1[3 * i] = frames1[i].x; d1[3 * i + 1] = frames1[i].y; d1[3 * i + 2] = frames1[i].z; }
        const std::vector<double> all = rmsd_matrix_f64(Engine::global(), d1.data(), F1, nullptr, 0, natoms, {}, nullptr);
        std::vector<double> want64(F1 * F1, -1.0);
        EXPECT(molar_hip_rmsd_matrix_f64(Engine::global().ctx(), d1.data(), F1, natoms * 3, nullptr, 0, 0, natoms, nullptr, natoms, nullptr, 1,
                                         want64.data(), F1) == 0);
        EXPECT(all.size() == F1 * F1 && std::memcmp(all.data(), want64.data(), want64.size() * sizeof(double)) == 0);
        EXPECT(all[1] < 1e-5 && all[2] > 0.05);
    }

    bool threw = false;
    try { frames2.pop_back(); rmsd_matrix(sel, frames1, &frames2); } catch (const MolarError &) { threw = true; }
    EXPECT(threw);

    if (failures) { std::printf("%d failure(s)\n", failures); return 1; }
    std::printf("all rmsd_matrix host-mirror tests passed\n");
    return 0;
}
