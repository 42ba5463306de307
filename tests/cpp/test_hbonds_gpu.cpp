// molar::hbonds and molar::hbonds_frames of the C++ host mirror (include/molar_hip.hpp) on one box of rigid waters, every atom
// wrapped into an orthorhombic cell on its own.  What to expect is computed here by the definition of molar_hip.h in plain C++:
// all donor-acceptor pairs by the minimum image in double, every hydrogen of the donor, angle(D-H-A) >= 150 degrees by atan2.
// The case is checked to be a test first: no pair within 1e-5 nm of the cutoff, no angle within 1e-6 degrees of the threshold.
#include <array>
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

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static double uniform() {                       // xorshift64*, in [0, 1)
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return (double)((rng_state * 0x2545F4914F6CDD1Dull) >> 11) / 9007199254740992.0;
}

struct V { double x, y, z; };
static V sub(V a, V b) { return V{a.x - b.x, a.y - b.y, a.z - b.z}; }
static double dot(V a, V b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
static V cross(V a, V b) { return V{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
static V image(V v, double L) { return V{v.x - L * std::round(v.x / L), v.y - L * std::round(v.y / L), v.z - L * std::round(v.z / L)}; }

struct Expected {
    std::vector<std::array<uint32_t, 3>> triples;
    std::vector<double> angle, dist_da, dist_ha;
    std::vector<uint64_t> don, acc;
    bool is_a_test = true;
};

static Expected expect(const std::vector<Pos> &xyz, size_t nw, double L, double cutoff, double min_angle) {
    Expected e;
    e.don.assign(nw, 0);
    e.acc.assign(nw, 0);
    auto at = [&](size_t a) { return V{(double)xyz[a].x, (double)xyz[a].y, (double)xyz[a].z}; };
    const double deg = 180.0 / std::acos(-1.0);
    for (size_t p = 0; p < nw; ++p)
        for (size_t hk = 1; hk <= 2; ++hk)
            for (size_t q = 0; q < nw; ++q) {
                if (p == q) continue;
                const V d = at(3 * p), h = at(3 * p + hk), a = at(3 * q);
                const V da = image(sub(a, d), L), hd = image(sub(d, h), L), ha = image(sub(a, h), L);
                const double r = std::sqrt(dot(da, da));
                if (std::fabs(r - cutoff) < 1e-5) e.is_a_test = false;
                if (r > cutoff) continue;
                const V c = cross(hd, ha);
                const double ang = std::atan2(std::sqrt(dot(c, c)), dot(hd, ha)) * deg;
                if (std::fabs(ang - min_angle) < 1e-6) e.is_a_test = false;
                if (ang < min_angle) continue;
                e.triples.push_back({(uint32_t)(3 * p), (uint32_t)(3 * p + hk), (uint32_t)(3 * q)});
                e.angle.push_back(ang);
                e.dist_da.push_back(r);
                e.dist_ha.push_back(std::sqrt(dot(ha, ha)));
                ++e.don[p];
                ++e.acc[q];
            }
    return e;
}

static bool close_all(const std::vector<double> &got, const std::vector<double> &want, double tol) {
    if (got.size() != want.size()) return false;
    for (size_t i = 0; i < want.size(); ++i)
        if (!(std::fabs(got[i] - want[i]) <= tol)) return false;
    return true;
}

int main() {
    const size_t m = 7, nw = m * m * m;                 // 343 waters on a jittered lattice at water density
    const double L = (double)(float)(0.31 * m), cutoff = 0.35, half = 104.5 / 2.0 * std::acos(-1.0) / 180.0;      // (the cell is f32)
    std::vector<Pos> xyz(3 * nw);
    for (size_t w = 0; w < nw; ++w) {
        const V o{((double)(w / (m * m)) + 0.5 + 0.5 * (uniform() - 0.5)) * 0.31, ((double)(w / m % m) + 0.5 + 0.5 * (uniform() - 0.5)) * 0.31,
                  ((double)(w % m) + 0.5 + 0.5 * (uniform() - 0.5)) * 0.31};
        // an orthonormal pair (u, v) from two random directions
        V u{uniform() - 0.5, uniform() - 0.5, uniform() - 0.5}, t{uniform() - 0.5, uniform() - 0.5, uniform() - 0.5};
        const double un = std::sqrt(dot(u, u));
        u = V{u.x / un, u.y / un, u.z / un};
        V v = cross(u, t);
        const double vn = std::sqrt(dot(v, v));
        v = V{v.x / vn, v.y / vn, v.z / vn};
        const V site[3] = {o, V{o.x + 0.1 * (std::cos(half) * u.x + std::sin(half) * v.x), o.y + 0.1 * (std::cos(half) * u.y + std::sin(half) * v.y),
                                o.z + 0.1 * (std::cos(half) * u.z + std::sin(half) * v.z)},
                           V{o.x + 0.1 * (std::cos(half) * u.x - std::sin(half) * v.x), o.y + 0.1 * (std::cos(half) * u.y - std::sin(half) * v.y),
                             o.z + 0.1 * (std::cos(half) * u.z - std::sin(half) * v.z)}};
        for (int k = 0; k < 3; ++k) {               // every atom wrapped on its own
            auto wrap = [&](double c) { return (float)(c - L * std::floor(c / L)); };
            xyz[3 * w + k] = Pos{wrap(site[k].x), wrap(site[k].y), wrap(site[k].z)};
        }
    }
    const Expected e = expect(xyz, nw, L, cutoff, 150.0);
    EXPECT(e.is_a_test);
    EXPECT(e.triples.size() > 20);

    Topology top;
    top.masses.assign(3 * nw, 1.0f);
    State st;
    st.coords = xyz;
    Matrix3f bm{};
    bm.m = {(float)L, 0, 0, 0, (float)L, 0, 0, 0, (float)L};
    st.pbox = PeriodicBox::from_matrix(bm);
    System sys(top, st);
    Engine eng(0);
    std::vector<usize> ox(nw), hoff(nw + 1), hidx(2 * nw);
    for (size_t w = 0; w < nw; ++w) {
        ox[w] = 3 * w;
        hoff[w] = 2 * w;
        hidx[2 * w] = 3 * w + 1;
        hidx[2 * w + 1] = 3 * w + 2;
    }
    hoff[nw] = 2 * nw;
    SelBound donors(sys, ox, eng), acceptors(sys, ox, eng);

    const HBonds r = hbonds(donors, acceptors, hoff, hidx);
    EXPECT(r.triples == e.triples);
    EXPECT(r.don_count == e.don);
    EXPECT(r.acc_count == e.acc);
    EXPECT(close_all(r.angle, e.angle, 1e-9));
    EXPECT(close_all(r.dist_da, e.dist_da, 1e-12));
    EXPECT(close_all(r.dist_ha, e.dist_ha, 1e-12));

    // the GROMACS criterion holds for every bond of a rigid water found at DHA 150 and O-O 0.35: H-D-A below 30 degrees
    HBondOptions g;
    g.angle_kind = MOLAR_HIP_HBOND_HDA_MAX;
    g.angle_deg = 30.0;
    g.want_columns = false;
    const HBonds rg = hbonds(donors, acceptors, hoff, hidx, g);
    EXPECT(rg.dist_da.empty() && rg.triples.size() >= r.triples.size());
    size_t found = 0;
    for (const auto &t : r.triples) found += std::find(rg.triples.begin(), rg.triples.end(), t) != rg.triples.end();
    EXPECT(found == r.triples.size());

    // three frames: the frame, the frame again, and a frame without a bond (the cell and the coordinates four times as large)
    std::vector<Pos> frames;
    std::vector<Float> boxes;
    for (int f = 0; f < 3; ++f) {
        const float s = f == 2 ? 4.0f : 1.0f;
        for (const Pos &p : xyz) frames.push_back(Pos{p.x * s, p.y * s, p.z * s});
        for (int k = 0; k < 9; ++k) boxes.push_back(bm.m[k] * s);
    }
    // (a wrapped water scaled by 4 is torn apart: its hydrogens are 0.4 nm or a cell away, and no oxygens are within 0.35 nm)
    const HBonds b = hbonds_frames(donors, acceptors, frames, hoff, hidx, boxes.data());
    const uint64_t n = e.triples.size();
    EXPECT(b.per_frame == (std::vector<uint64_t>{n, n, 0}));
    EXPECT(b.frame_offsets == (std::vector<uint64_t>{0, n, 2 * n, 2 * n}));
    EXPECT(b.table == e.triples);
    EXPECT(b.occupancy == std::vector<uint32_t>(n, 2u));
    bool rows_ok = b.bond_of_entry.size() == 2 * n && b.triples.size() == 2 * n;
    for (size_t k = 0; rows_ok && k < 2 * n; ++k) rows_ok = b.bond_of_entry[k] == k % n && b.triples[k] == e.triples[k % n];
    EXPECT(rows_ok);
    for (size_t w = 0; w < nw; ++w) EXPECT(b.don_count[w] == 2 * e.don[w]);

    // the wrapper's own checks
    bool threw = false;
    try {
        hbonds(donors, acceptors, std::vector<usize>(nw, 0), hidx);
    } catch (const MolarError &) {
        threw = true;
    }
    EXPECT(threw);

    if (failures == 0) std::printf("all hbonds host-mirror tests passed (%zu bonds)\n", e.triples.size());
    return failures ? 1 : 0;
}
