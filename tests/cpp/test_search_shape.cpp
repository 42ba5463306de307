// The functions of a search's shape (molar_amd/csrc/search_shape.hpp) on the host: grid dimensions, the policy for wrapped
// pairs, the kernel family, the slot bound, the occupancy key, the held grid of `within` requests.  No device is needed: boxes come from the library's
// molar_hip_box_from_matrix, everything else is arithmetic.
//
// A wrong band or margin would change no search result - only which path wrapped pairs take - so the oracle suites cannot see
// it.  The expected values below are therefore literals, RECORDED FROM COMMIT 687ec6e (the last one in which this arithmetic
// sat inside make_params / small_cell_lanes / molar_hip_search_cell_kernels and read the context's fields): a throwaway
// program included that commit's search.hip, filled a default-constructed context with each row's inputs and printed
// dims_from_extents, make_params, small_cell_lanes and molar_hip_search_cell_kernels (host code only, -ffp-contract=off,
// floats with %.9g).  Floats are compared bit for bit with the float nearest the printed value.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../molar_amd/csrc/search_shape.hpp"

using namespace mh;

static int failures = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);        \
            ++failures;                                                          \
        }                                                                        \
    } while (0)

static bool same_bits(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }

// ---- dims_from_extents, wrapped_pair_policy, small_cell_lanes: inputs and the values 687ec6e computed for them
struct PolicyCase {
    const char *name;
    float box9[9];        // column-major
    bool use_box;         // false: the same extents as lower = 0, upper = lab extents
    unsigned pbc;
    float cutoff;
    int kind;
    unsigned n0, n1;
    int rc;               // of dims_from_extents
    unsigned dims[3];
    unsigned wrap_kind, prune, approx;
    float band_lo, band_hi, prune_limit2;
    int lanes;
};
static const unsigned P26 = 1u << 26;
static const PolicyCase POLICY[] = {
    // the three boxes of the issue: rectangular, two GROMACS-style triclinic ones (the first with 3 cells along z: no band)
    {"ortho", {4, 0, 0, 0, 5, 0, 0, 0, 6}, true, 7, 0.8f, 0, 4096, 0, 0, {5, 6, 7}, 1, 1, 1, 0.639820516f, 0.640179574f, 0.641652644f, 0},
    {"tric_a", {4, 0, 0, 0, 4, 0, 2, 2, 2.8284271f}, true, 7, 0.8f, 0, 4096, 0, 0, {7, 7, 3}, 2, 1, 0, 0.640000045f, 0.640000045f, 0.641675115f, 0},
    {"tric_b", {4, 0, 0, 1.5f, 5, 0, -1, 2, 6}, true, 7, 0.8f, 0, 4096, 0, 0, {5, 8, 7}, 2, 1, 1, 0.639790952f, 0.640209138f, 0.641682267f, 32},
    // no box: general wrap kind, nothing pruned, no band, the bare margin
    {"nobox", {4, 0, 0, 0, 5, 0, 0, 0, 6}, false, 7, 0.8f, 0, 4096, 0, 0, {5, 6, 7}, 3, 0, 0, 0.640000045f, 0.640000045f, 0.641601026f, 0},
    // a periodic dimension with 2 cells: pruning off; the same box periodic in x and y only: pruning (and the band) stay
    {"two_cells_z", {4, 0, 0, 0, 5, 0, 0, 0, 1.7f}, true, 7, 0.8f, 0, 4096, 0, 0, {5, 6, 2}, 1, 0, 0, 0.640000045f, 0.640000045f, 0.641644061f, 0},
    {"two_cells_z_pbc_xy", {4, 0, 0, 0, 5, 0, 0, 0, 1.7f}, true, 3, 0.8f, 0, 4096, 0, 0, {5, 6, 2}, 1, 1, 1, 0.639829099f, 0.640170991f, 0.641644061f, 0},
    // 3 cells along a periodic dimension: pruned, but no band (round(f_d) must be +-1)
    {"three_cells_x", {2.5f, 0, 0, 0, 5, 0, 0, 0, 6}, true, 7, 0.8f, 0, 4096, 0, 0, {3, 6, 7}, 1, 1, 0, 0.640000045f, 0.640000045f, 0.641652644f, 0},
    // (row << 26 | position) packing: 2^26 - 1 atoms in the two sets keep the band, 2^26 lose it
    {"pack_fits", {4, 0, 0, 0, 5, 0, 0, 0, 6}, true, 7, 0.8f, 1, P26 - 1u - 4096u, 4096, 0, {5, 6, 7}, 1, 1, 1, 0.639820516f, 0.640179574f, 0.641652644f, 0},
    {"pack_full", {4, 0, 0, 0, 5, 0, 0, 0, 6}, true, 7, 0.8f, 1, P26 - 4096u, 4096, 0, {5, 6, 7}, 1, 1, 0, 0.640000045f, 0.640000045f, 0.641652644f, 0},
    // a box so large against the cutoff that the margin passes 5 % of it: pruning and band off (the grid itself is refused)
    {"huge_box", {4000, 0, 0, 0, 4000, 0, 0, 0, 4000}, true, 7, 0.3f, 0, 4096, 0, MOLAR_HIP_ERR_TOO_LARGE, {13333, 13333, 13333}, 1, 0, 0, 0.0900000036f, 0.0900000036f, 0.103989214f, 16},
    // a matrix that is not triangular: general wrap kind
    {"general", {4, 0.5f, 0, 0, 5, 0, 0, 0, 6}, true, 7, 0.8f, 0, 4096, 0, 0, {5, 6, 7}, 3, 1, 1, 0.639816582f, 0.640183508f, 0.641656578f, 0},
    // the policy does not depend on the kind; small_cell_lanes does
    {"double_small", {4, 0, 0, 1.5f, 5, 0, -1, 2, 6}, true, 7, 0.8f, 1, 3000, 5000, 0, {5, 8, 7}, 2, 1, 1, 0.639790952f, 0.640209138f, 0.641682267f, 32},
    {"within", {4, 0, 0, 1.5f, 5, 0, -1, 2, 6}, true, 7, 0.8f, 2, 3000, 300, 0, {5, 8, 7}, 2, 1, 1, 0.639790952f, 0.640209138f, 0.641682267f, 0},
};

static void test_policy() {
    for (const PolicyCase &k : POLICY) {
        GridSet sets[2];
        SearchShape s;
        s.set = sets;
        molar_hip_box b{};
        CHECK(molar_hip_box_from_matrix(k.box9, &b) == 0);
        float ext[3];
        molar_hip_box_lab_extents(&b, ext);
        s.kind = k.kind;
        s.use_box = k.use_box;
        s.pbc = (uint8_t)k.pbc;
        s.cutoff = k.cutoff;
        if (k.use_box) s.box = b;
        else for (int d = 0; d < 3; ++d) { s.lower[d] = 0.f; s.upper[d] = ext[d]; }
        sets[0].n = k.n0;
        sets[1].n = k.n1;
        const int rc = dims_from_extents(s, ext);
        const WrapPolicy w = wrapped_pair_policy(s);
        const int lanes = small_cell_lanes(s);
        const bool ok = rc == k.rc && s.dims[0] == k.dims[0] && s.dims[1] == k.dims[1] && s.dims[2] == k.dims[2] && w.wrap_kind == k.wrap_kind &&
                        w.prune_wrapped == k.prune && w.approx_wrapped == k.approx && same_bits(w.band_lo, k.band_lo) && same_bits(w.band_hi, k.band_hi) &&
                        same_bits(w.prune_limit2, k.prune_limit2) && lanes == k.lanes;
        if (!ok) {
            std::printf("FAILED %s: rc %d dims %u %u %u wrap_kind %u prune %u approx %u band_lo %.9g band_hi %.9g prune_limit2 %.9g lanes %d\n", k.name, rc, s.dims[0],
                        s.dims[1], s.dims[2], w.wrap_kind, w.prune_wrapped, w.approx_wrapped, w.band_lo, w.band_hi, w.prune_limit2, lanes);
            ++failures;
        }
        if (!k.use_box) {     // no band: both ends are cutoff^2; the margin is the bare 1e-3 nm
            const float lim = k.cutoff + 1.0e-3f;
            CHECK(same_bits(w.band_lo, k.cutoff * k.cutoff) && same_bits(w.band_hi, k.cutoff * k.cutoff) && same_bits(w.prune_limit2, lim * lim));
        }
    }
}

// ---- small_cell_lanes and pair_family on a grid of 1000 cells: {kind, n0, n1, occ_use[0], occ_use[1]} -> what 687ec6e's
// small_cell_lanes and molar_hip_search_cell_kernels answered
struct FamilyCase { int kind; unsigned n0, n1, occ0, occ1; int lanes, family; };
static const FamilyCase FAMILY[] = {
    {0, 13000, 0, 0, 0, 16, 16},         // up to 13 atoms per cell: 16 lanes
    {0, 13001, 0, 0, 0, 32, 32},
    {0, 19000, 0, 0, 0, 32, 32},         // up to 19: 32 lanes
    {0, 19001, 0, 0, 0, 0, 0},
    {1, 13000, 13001, 0, 0, 32, 32},     // DOUBLE: the wider of the two sets ...
    {1, 13001, 13000, 0, 0, 32, 32},
    {1, 19001, 100, 0, 0, 0, 0},         // ... and 0 wins
    {1, 100, 19001, 0, 0, 0, 0},
    {2, 100, 100, 0, 0, 0, 0},           // WITHIN, VDW: the regular kernels
    {3, 100, 100, 0, 0, 0, 0},
    {0, 1300, 0, 100, 0, 16, 16},        // 100 occupied cells replace the 1000
    {0, 1301, 0, 100, 0, 32, 32},
    {0, 1901, 0, 100, 0, 0, 0},
    {0, 13000, 0, 5000, 0, 16, 16},      // (never more than the grid has)
    {0, 448000, 0, 0, 0, 0, 0},          // more than 448 per cell: wide; more than 1000: huge
    {0, 448001, 0, 0, 0, 0, -1},
    {0, 1000000, 0, 0, 0, 0, -1},
    {0, 1000001, 0, 0, 0, 0, -2},
    {1, 1000001, 448000, 0, 0, 0, 0},    // DOUBLE judges set 1
    {1, 100, 448001, 0, 0, 0, -1},
    {1, 100, 1000001, 0, 0, 0, -2},
    {0, 44801, 0, 100, 0, 0, -1},        // per occupied cell here too
    {1, 100, 100001, 0, 100, 0, -2},
    {1, 100001, 100, 100, 0, 0, 0},
    {2, 1000001, 1000001, 0, 0, 0, 0},
};

static void test_family() {
    GridSet sets[2];
    SearchShape s;
    s.set = sets;
    s.dims[0] = s.dims[1] = s.dims[2] = 10;
    for (const FamilyCase &f : FAMILY) {
        s.kind = f.kind;
        sets[0].n = f.n0;
        sets[1].n = f.n1;
        s.occ_use[0] = f.occ0;
        s.occ_use[1] = f.occ1;
        const int lanes = small_cell_lanes(s), family = pair_family(s);
        if (lanes != f.lanes || family != f.family) {
            std::printf("FAILED {%d, %u, %u, %u, %u}: lanes %d family %d\n", f.kind, f.n0, f.n1, f.occ0, f.occ1, lanes, family);
            ++failures;
        }
        CHECK(records_hit_history(s) == ((f.kind == 0 || f.kind == 1) && f.lanes == 0));
    }
}

// ---- plan_entries / slots_bound against the formula: 14 (two grids: 28) tasks per first-set cell, one slot per 64 rows and
// task, 28 corner entries of up to 512 slots; the fused histogram's plan adds one 32-row entry per cell
static void test_slots_bound() {
    GridSet sets[2];
    SearchShape s;
    s.set = sets;
    s.dims[0] = 5; s.dims[1] = 8; s.dims[2] = 7;
    const uint64_t ncells = 5 * 8 * 7;
    for (int kind = 0; kind < 2; ++kind)
        for (unsigned n0 : {0u, 1u, 63u, 64u, 65u, 4097u, 1000003u}) {
            s.kind = kind;
            sets[0].n = n0;
            sets[1].n = 77;               // (the second set's size is not part of the bound)
            const uint64_t mult = kind ? 2 : 1, ntasks = 14 * ncells * mult;
            const uint64_t plain = 14 * mult * (((uint64_t)n0 + 63) / 64) + ntasks + 28 * 512;
            CHECK(plan_entries(s) == ntasks);
            CHECK(slots_bound(s, false) == plain);
            CHECK(slots_bound(s, true) == plain + ((uint64_t)n0 + 31) / 32 + ncells);
        }
    CHECK(grid_cells(s) == ncells);
    CHECK(!sorted_by_device_sort(384 * ncells, ncells) && sorted_by_device_sort(384 * ncells + 1, ncells));
}

// ---- occ_key_of: non-zero; kind, set sizes (n1: DOUBLE only), every grid dimension and use_box are part of it
static void test_occ_key() {
    GridSet sets[2];
    SearchShape s;
    s.set = sets;
    s.kind = MOLAR_HIP_SEARCH_DOUBLE;
    s.use_box = true;
    s.dims[0] = 5; s.dims[1] = 8; s.dims[2] = 7;
    sets[0].n = 3000;
    sets[1].n = 5000;
    const unsigned long long key = occ_key_of(s);
    CHECK(key != 0);
    CHECK(key == 11973103181852634726ull);              // 687ec6e, the "double_small" row above
    auto differs = [&](auto change) {
        GridSet t[2];
        t[0].n = sets[0].n;
        t[1].n = sets[1].n;
        SearchShape v = s;
        v.set = t;
        change(v, t);
        return occ_key_of(v) != key && occ_key_of(v) != 0;
    };
    CHECK(differs([](SearchShape &v, GridSet *) { v.kind = MOLAR_HIP_SEARCH_WITHIN; }));
    CHECK(differs([](SearchShape &, GridSet *t) { t[0].n += 1; }));
    CHECK(differs([](SearchShape &, GridSet *t) { t[1].n += 1; }));
    CHECK(differs([](SearchShape &v, GridSet *) { v.dims[0] += 1; }));
    CHECK(differs([](SearchShape &v, GridSet *) { v.dims[1] += 1; }));
    CHECK(differs([](SearchShape &v, GridSet *) { v.dims[2] += 1; }));
    CHECK(differs([](SearchShape &v, GridSet *) { v.use_box = false; }));
    CHECK(!differs([](SearchShape &v, GridSet *) { v.cutoff = 0.5f; v.pbc = 3; v.occ_use[0] = 9; }));     // not part of the key
    s.kind = MOLAR_HIP_SEARCH_SINGLE;
    const unsigned long long single = occ_key_of(s);
    sets[1].n += 1;
    CHECK(single != 0 && single != key && occ_key_of(s) == single);        // SINGLE: the second set is not looked at
}

// ---- the held grid of `within` requests: the fingerprint of a host array, and what ends the reuse
// Coordinates by a fixed integer recurrence (exact in f32: 24 bits times a power of two).
static std::vector<float> recurrence(size_t natoms, uint32_t seed) {
    std::vector<float> v(3 * natoms);
    uint32_t x = seed;
    for (float &f : v) {
        x = x * 1664525u + 1013904223u;
        f = (float)(x >> 8) * (8.0f / 16777216.0f);
    }
    return v;
}

// The expected values are RECORDED FROM COMMIT f7b1d91, the last one in which the fingerprint was an inline lambda of
// prepare_search: a throwaway program held that block verbatim (around a struct with xyz1 and natoms1) and printed it for
// these three arrays.  A record of a running hold never outlives the process, so the value itself is free to change - pinning it
// is what makes this a regression test of the move.
static void test_held_fingerprint() {
    struct { size_t natoms; uint64_t want; size_t middle; } cases[] = {
        {10, 0x2738aa20d12dd355ull, 5}, {600, 0xfd7799a0bb088febull, 300}, {5000, 0xf8cfb23434bec7c3ull, 9 * 200}};   // middle = step * k
    for (size_t k = 0; k < 3; ++k) {
        const size_t n = cases[k].natoms;
        std::vector<float> v = recurrence(n, 12345u + (uint32_t)k);
        const uint64_t fp = held_fingerprint(v.data(), n);
        CHECK(fp == cases[k].want);
        CHECK(fp & 1ull);
        auto changed = [&](size_t atom) {
            std::vector<float> w = v;
            w[3 * atom + 1] += 0.25f;
            return held_fingerprint(w.data(), n) != fp;
        };
        CHECK(changed(0));
        CHECK(changed(n - 1));
        CHECK(changed(cases[k].middle));
        // what the fingerprint is: the two ends and every (n / 512)th atom - atom 1801 of 5000 is none of them
        if (n == 5000) CHECK(!changed(9 * 200 + 1));
    }
}

static void test_held_conditions() {
    GridSet gen_a[2], gen_b[2];
    const std::vector<float> xyz = recurrence(600, 7u);
    const uint64_t ids[4] = {1, 2, 3, 5};
    const float box9[9] = {4, 0, 0, 0, 5, 0, 0, 0, 6};
    for (const bool use_box : {true, false}) {
        SearchShape s;
        s.set = gen_a;
        s.kind = MOLAR_HIP_SEARCH_WITHIN;
        s.use_box = use_box;
        s.pbc = use_box ? 7 : 0;
        if (use_box) CHECK(molar_hip_box_from_matrix(box9, &s.box) == 0);
        s.dims[0] = 5; s.dims[1] = 6; s.dims[2] = 7;
        for (int d = 0; d < 3; ++d) { s.lower[d] = -1.f - (float)d; s.upper[d] = 4.f + (float)d; }
        molar_hip_search_desc q{};
        q.kind = MOLAR_HIP_SEARCH_WITHIN;
        q.xyz1 = xyz.data();
        q.natoms1 = 600;
        q.idx1 = ids;
        q.n1 = 4;
        q.ids_local = 0;
        const uint64_t fp = held_fingerprint(q.xyz1, q.natoms1);
        const HeldGrid h = held_remember(q, s, fp);
        // the unchanged request is accepted; nothing is, against a record that is not valid
        CHECK(h.valid && held_names_request(h, q, s, fp) && held_same_cells(h, s));
        CHECK(!held_names_request(HeldGrid{}, q, s, fp));
        HeldGrid ended = h;
        ended.valid = false;
        CHECK(!held_names_request(ended, q, s, fp));
        // one thing at a time: the request
        auto other_request = [&](auto change) {
            molar_hip_search_desc r = q;
            SearchShape v = s;
            uint64_t f = fp;
            change(r, v, f);
            return !held_names_request(h, r, v, f);
        };
        CHECK(other_request([&](molar_hip_search_desc &r, SearchShape &, uint64_t &) { r.xyz1 = xyz.data() + 3; }));
        CHECK(other_request([&](molar_hip_search_desc &r, SearchShape &, uint64_t &) { r.natoms1 = 599; }));
        CHECK(other_request([&](molar_hip_search_desc &r, SearchShape &, uint64_t &) { r.idx1 = ids + 1; }));
        CHECK(other_request([&](molar_hip_search_desc &r, SearchShape &, uint64_t &) { r.idx1 = nullptr; }));
        CHECK(other_request([&](molar_hip_search_desc &r, SearchShape &, uint64_t &) { r.n1 = 3; }));
        CHECK(other_request([&](molar_hip_search_desc &r, SearchShape &, uint64_t &) { r.ids_local = 1; }));
        CHECK(other_request([&](molar_hip_search_desc &, SearchShape &v, uint64_t &) { v.use_box = !v.use_box; }));
        CHECK(other_request([&](molar_hip_search_desc &, SearchShape &v, uint64_t &) { v.pbc ^= 2; }));
        CHECK(other_request([&](molar_hip_search_desc &, SearchShape &, uint64_t &f) { f ^= 2ull; }));
        CHECK(other_request([&](molar_hip_search_desc &, SearchShape &, uint64_t &f) { f = 0; }));          // the same address, now device memory
        CHECK(other_request([&](molar_hip_search_desc &, SearchShape &v, uint64_t &) { v.set = gen_b; }));  // the other grid generation
        // one entry of the box matrix: part of the request with a box, not looked at without one
        const bool box_matters = other_request([&](molar_hip_search_desc &, SearchShape &v, uint64_t &) { v.box.m[4] += 0.5f; });
        CHECK(box_matters == use_box);
        // the cutoff and the second set are not part of it
        CHECK(!other_request([&](molar_hip_search_desc &r, SearchShape &v, uint64_t &) { r.cutoff = 0.7f; v.cutoff = 0.7f; r.xyz2 = xyz.data(); r.natoms2 = 9; }));
        // one thing at a time: the grid
        auto other_cells = [&](auto change) {
            SearchShape v = s;
            change(v);
            return !held_same_cells(h, v);
        };
        for (int d = 0; d < 3; ++d) CHECK(other_cells([&](SearchShape &v) { v.dims[d] += 1; }));
        // the caller's bounds decide the grid of a request without a box; with a box they are ignored
        for (int d = 0; d < 3; ++d) {
            CHECK(other_cells([&](SearchShape &v) { v.lower[d] -= 0.5f; }) == !use_box);
            CHECK(other_cells([&](SearchShape &v) { v.upper[d] += 0.5f; }) == !use_box);
        }
    }
}

int main() {
    test_policy();
    test_family();
    test_slots_bound();
    test_occ_key();
    test_held_fingerprint();
    test_held_conditions();
    if (failures) {
        std::printf("%d search-shape checks failed\n", failures);
        return 1;
    }
    std::printf("all search-shape tests passed\n");
    return 0;
}
