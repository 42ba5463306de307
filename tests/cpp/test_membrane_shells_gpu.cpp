// MembraneFrames::set_shells (include/molar_hip.hpp -> molar_hip_membrane_plan_set_shells) over three frames against the
// stage-by-stage C calls it replaces: a smoothing pass, molar_hip_membrane_nth_shell_patches, the state re-slotted from zero,
// max_smooth_iter passes on the shell patches, the tail order, molar_hip_membrane_smooth_curvature.  Bit for bit.
#include <algorithm>
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

template <class T>
static bool same(const std::vector<T> &a, const std::vector<T> &b, size_t n) {
    return a.size() >= n && b.size() >= n && std::memcmp(a.data(), b.data(), n * sizeof(T)) == 0;
}

static void shells_tests(size_t n_patch, size_t n_smooth, int iters) {
    Engine &eng = Engine::global();
    // 2 x (12 x 12) lipids of 8 beads on a jittered lattice, heads out, tails towards the mid-plane
    const int side = 12, per = 8, K = 2 * side * side;
    const float L = side * 0.8f, Lz = 9.0f;
    const size_t natoms = (size_t)K * per;
    std::vector<float> xyz0(natoms * 3);
    uint32_t seed = 777u;
    auto rnd = [&]() { seed = seed * 1664525u + 1013904223u; return ((seed >> 8) & 0xFFFF) / 65536.0f - 0.5f; };
    for (int k = 0; k < K; ++k) {
        const int leaf = k / (side * side), a = k % (side * side);
        const float sgn = leaf == 0 ? 1.0f : -1.0f;
        const float cx = (a % side + 0.5f + 0.3f * rnd()) * 0.8f, cy = (a / side + 0.5f + 0.3f * rnd()) * 0.8f;
        for (int b = 0; b < per; ++b) {
            float *p = &xyz0[3 * ((size_t)k * per + b)];
            p[0] = cx + 0.05f * rnd(); p[1] = cy + 0.05f * rnd();
            p[2] = Lz / 2 + sgn * (2.0f - 0.25f * b) + 0.03f * rnd();
            for (int d = 0; d < 2; ++d) p[d] = p[d] - L * std::floor(p[d] / L);
        }
    }
    const float box9[9] = {L, 0, 0, 0, L, 0, 0, 0, Lz};
    std::vector<uint64_t> lipid_idx(natoms), lipid_off(K + 1), marker_idx, marker_off{0}, tail_idx, tail_off{0};
    std::vector<uint32_t> tail_lipid;
    std::vector<float> masses(natoms);
    for (size_t i = 0; i < natoms; ++i) { lipid_idx[i] = i; masses[i] = 12.0f + (i % 3); }
    for (int k = 0; k <= K; ++k) lipid_off[k] = (uint64_t)k * per;
    for (int k = 0; k < K; ++k) {
        const uint64_t f = (uint64_t)k * per;
        for (uint64_t b : {0, 1}) marker_idx.push_back(f + b);
        marker_off.push_back(marker_idx.size());
        for (uint64_t b : {2, 3}) marker_idx.push_back(f + b);
        marker_off.push_back(marker_idx.size());
        for (uint64_t b : {6, 7}) marker_idx.push_back(f + b);
        marker_off.push_back(marker_idx.size());
        for (uint64_t b = 2; b < 8; ++b) tail_idx.push_back(f + b);
        tail_off.push_back(tail_idx.size());
        tail_lipid.push_back((uint32_t)k);
    }
    std::vector<uint8_t> bonds(tail_idx.size() - K, 1);
    molar_hip_membrane_desc D{};
    D.natoms = natoms; D.nlipids = K;
    D.lipid_idx = lipid_idx.data(); D.lipid_offsets = lipid_off.data(); D.marker_idx = marker_idx.data(); D.marker_offsets = marker_off.data();
    D.masses = masses.data(); D.ntails = K; D.tail_idx = tail_idx.data(); D.tail_offsets = tail_off.data(); D.tail_lipid = tail_lipid.data();
    D.tail_bonds = bonds.data(); D.cutoff = 1.6f; D.order_type = 2; D.max_smooth_iter = iters; D.unwrap = 1;
    MembraneFrames mem(eng, D);
    mem.set_shells(n_patch, n_smooth);
    const PeriodicBox pbox = PeriodicBox::from_matrix(Matrix3f{{box9[0], box9[1], box9[2], box9[3], box9[4], box9[5], box9[6], box9[7], box9[8]}});
    std::vector<uint8_t> valid(K, 1);
    const size_t norder = tail_idx.size() - 2 * K;
    std::vector<uint64_t> noff(K + 1);
    for (int k = 0; k <= K; ++k) noff[k] = k;
    for (int frame = 0; frame < 3; ++frame) {
        std::vector<float> a(xyz0), b(xyz0);
        for (size_t i = 0; i < a.size(); ++i) { const float j = 0.02f * rnd(); a[i] += j; b[i] += j; }
        // ---- chained
        (void)mem.push(a.data(), pbox);
        std::vector<float> sh(K * 3), nrm(K * 3), coefs(K * 6), mean(K), gauss(K), pc(K * 2), pd(K * 6), area(K), order(norder);
        std::vector<uint64_t> poff(K + 1);
        std::vector<uint8_t> vout(K);
        std::vector<uint32_t> nvert(K);
        molar_hip_membrane_out O{};
        O.smoothed_head = sh.data(); O.normals = nrm.data(); O.quad_coefs = coefs.data(); O.mean_curv = mean.data(); O.gauss_curv = gauss.data();
        O.princ_curvs = pc.data(); O.princ_dirs = pd.data(); O.area = area.data(); O.order = order.data(); O.patch_offsets = poff.data();
        O.valid = vout.data(); O.nvert = nvert.data();
        auto v = mem.finish(O);
        EXPECT(v.has_value() && v->nlipids == (size_t)K);
        const size_t E = v->patch_entries, slots = E + 4 * (size_t)K;
        std::vector<float> fitted(E * 3), voro(slots * 3);
        std::vector<uint64_t> pids(E), neib(slots);
        molar_hip_membrane_out Oe{};
        Oe.fitted_patch_points = fitted.data(); Oe.voro_vertexes = voro.data(); Oe.patch_ids = pids.data(); Oe.neib_ids = neib.data();
        mem.fetch(Oe);
        // ---- stage by stage
        check(molar_hip_unwrap_simple_batch(eng.ctx(), b.data(), natoms, lipid_idx.data(), lipid_off.data(), K, box9, 7));
        EXPECT(std::memcmp(a.data(), b.data(), a.size() * 4) == 0);
        std::vector<float> mk(K * 9);
        check(molar_hip_center_batch(eng.ctx(), b.data(), natoms, marker_idx.data(), marker_off.data(), 3 * K, masses.data(), mk.data()));
        std::vector<float> h2(K * 3), t2(K * 3);
        for (int k = 0; k < K; ++k)
            for (int d = 0; d < 3; ++d) { h2[3 * k + d] = mk[9 * k + d]; t2[3 * k + d] = mk[9 * k + 6 + d]; }
        std::vector<uint64_t> vidx;
        for (int k = 0; k < K; ++k) if (valid[k]) vidx.push_back(k);
        molar_hip_search_desc q{};
        q.kind = MOLAR_HIP_SEARCH_SINGLE; q.cutoff = D.cutoff; q.xyz1 = h2.data(); q.natoms1 = K; q.idx1 = vidx.data(); q.n1 = vidx.size();
        q.ids_local = 0; q.box9 = box9; q.pbc = 7;
        uint64_t np = 0;
        check(molar_hip_search_count(eng.ctx(), &q, &np));
        std::vector<uint32_t> pairs(2 * np + 2);
        check(molar_hip_search_fill(eng.ctx(), pairs.data(), nullptr));
        EXPECT(np == v->npairs);
        std::vector<uint64_t> poff2(K + 1), pids2(2 * np + 1);
        check(molar_hip_membrane_patches_from_pairs(pairs.data(), np, K, poff2.data(), pids2.data()));
        std::vector<float> n02(K * 3, 0.f);
        check(molar_hip_membrane_initial_normals(K, h2.data(), t2.data(), poff2.data(), pids2.data(), valid.data(), n02.data()));
        // the state of new_membrane_state (lib.rs:152-177), every field carried from call to call
        std::vector<float> sh2(h2), nrm2(n02), coefs2(K * 6, 0.f), mean2(K, -100.f), gauss2(K, -100.f), pc2(K * 2, 0.f), pd2(K * 6, 0.f),
            area2(K, 0.f);
        std::vector<uint32_t> nvert2(K, 0);
        size_t E2 = 2 * np;
        std::vector<uint64_t> neib2(E2 + 4 * K, 0);
        std::vector<float> voro2((E2 + 4 * K) * 3, 0.f), fitted2(std::max<size_t>(E2, 1) * 3, 0.f);
        auto smooth = [&]() {
            molar_hip_membrane_patches PP{(size_t)K, poff2.data(), pids2.data()};
            molar_hip_membrane_state S{};
            S.head_markers = sh2.data(); S.normals = nrm2.data(); S.valid = valid.data(); S.quad_coefs = coefs2.data(); S.mean_curv = mean2.data();
            S.gauss_curv = gauss2.data(); S.princ_curvs = pc2.data(); S.princ_dirs = pd2.data(); S.area = area2.data(); S.nvert = nvert2.data();
            S.neib_ids = neib2.data(); S.voro_vertexes = voro2.data(); S.fitted_patch_points = fitted2.data();
            check(molar_hip_membrane_smooth(eng.ctx(), &PP, box9, &S));
        };
        if (n_patch) {
            smooth();
            std::vector<uint64_t> so(K + 1);
            size_t need = 0;
            check(molar_hip_membrane_nth_shell_patches(K, valid.data(), poff2.data(), pids2.data(), nvert2.data(), neib2.data(), n_patch, so.data(),
                                                       nullptr, 0, &need));
            std::vector<uint64_t> si(std::max<size_t>(need, 1));
            check(molar_hip_membrane_nth_shell_patches(K, valid.data(), poff2.data(), pids2.data(), nvert2.data(), neib2.data(), n_patch, so.data(),
                                                       si.data(), need, &need));
            EXPECT(need != E2);
            poff2 = so; pids2 = si; E2 = need;
            neib2.assign(E2 + 4 * K, 0); voro2.assign((E2 + 4 * K) * 3, 0.f); fitted2.assign(std::max<size_t>(E2, 1) * 3, 0.f);
            std::fill(nvert2.begin(), nvert2.end(), 0u);
        }
        for (int it = 0; it < iters; ++it) smooth();
        std::vector<float> order2(norder);
        check(molar_hip_lipid_tail_order(eng.ctx(), b.data(), natoms, tail_idx.data(), tail_off.data(), K, 2, nrm2.data(), noff.data(), bonds.data(),
                                         order2.data()));
        check(molar_hip_membrane_smooth_curvature(K, valid.data(), poff2.data(), nvert2.data(), neib2.data(), n_smooth, mean2.data(), gauss2.data()));
        EXPECT(E == E2 && poff2 == poff && same(pids2, pids, E));
        EXPECT(std::memcmp(valid.data(), vout.data(), K) == 0);
        EXPECT(same(sh2, sh, K * 3) && same(nrm2, nrm, K * 3) && same(coefs2, coefs, K * 6));
        EXPECT(same(mean2, mean, K) && same(gauss2, gauss, K) && same(pc2, pc, K * 2) && same(pd2, pd, K * 6) && same(area2, area, K));
        EXPECT(nvert2 == nvert && same(neib2, neib, slots) && same(voro2, voro, slots * 3) && same(fitted2, fitted, E * 3));
        EXPECT(same(order2, order, norder));
        size_t nvalid = 0;
        for (auto f : valid) nvalid += f;
        if (frame == 0) EXPECT(nvalid > (size_t)K / 4);
    }
}

int main() {
    try {
        shells_tests(3, 2, 1);
        shells_tests(4, 0, 2);
        shells_tests(0, 3, 1);
    } catch (const std::exception &e) {
        std::printf("exception: %s\n", e.what());
        return 2;
    }
    if (failures) { std::printf("%d failure(s)\n", failures); return 1; }
    std::printf("all membrane shell tests passed\n");
    return 0;
}
