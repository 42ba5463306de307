// The host helpers of molar_amd/csrc/traj_block.hpp that need no device: Carve and even_splits against the text the three
// units (rmsd_matrix.hip, fluct.hip, msd.hip) each had of their own before the header, restated here, and the checks of a
// selection against the codes and the message texts of those units, byte for byte.  A wrong split or offset changes what the
// plan entries report (tests/test_traj_plans_cpu.py has their numbers); this one says which helper did it.
#include <cstdio>
#include <cstring>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../molar_amd/csrc/traj_block.hpp"

using namespace mh;

static int failures = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);        \
            ++failures;                                                          \
        }                                                                        \
    } while (0)

static void test_carve() {
    const size_t regions[] = {0, 1, 16, 255, 256, 257, 511, 512, 4 * 8, 3 * 17 * 8, (size_t)1 << 33, ((size_t)1 << 33) + 1, 0, 7};
    // the lambda of the three make_layouts
    size_t bytes = 0;
    auto take = [&](size_t &off, size_t b) {
        off = bytes;
        bytes += (b + 255) & ~(size_t)255;
    };
    Carve ws;
    CHECK(ws.bytes == 0);
    for (size_t r : regions) {
        size_t want = ~(size_t)0, got = ~(size_t)0;
        take(want, r);
        ws.take(got, r);
        CHECK(got == want && ws.bytes == bytes);
        CHECK(got % 256 == 0 && ws.bytes - got >= r && ws.bytes - got < r + 256);
    }
}

static void test_even_splits() {
    for (uint32_t ksteps = 0; ksteps <= 700; ++ksteps)
        for (size_t ks0 = 0; ks0 <= 300; ++ks0) {
            // the tail of the two K-split computations as it stood in fluct.hip
            size_t ks = ks0;
            if (ks < 2) ks = 1;
            uint32_t kper = (uint32_t)((ksteps + ks - 1) / ks);
            if (kper == 0) kper = 1;
            const uint32_t ksplits = ksteps ? (ksteps + kper - 1) / kper : 1;
            const Splits s = even_splits(ksteps, ks0);
            CHECK(s.kper == kper && s.ksplits == ksplits);
            // no empty split, none beyond what was asked for, every step in one
            CHECK(s.ksplits >= 1 && s.ksplits <= ks && (size_t)s.kper * s.ksplits >= ksteps);
            if (ksteps) CHECK((size_t)s.kper * (s.ksplits - 1) < ksteps);
        }
    const Splits big = even_splits(0x1FFFFFFCu, 256);      // the largest selection rmsd_matrix takes: no overflow in 32 bits
    CHECK(big.kper == 0x1FFFFFFCu / 256 + 1 && big.ksplits == 256);
}

static bool failed_with(int rc, int code, const char *text) {
    if (rc == code && last_error() == text) return true;
    std::printf("  got %d \"%s\"\n", rc, last_error().c_str());
    return false;
}

static void test_checks() {
    const int INV = MOLAR_HIP_ERR_INVALID_ARGUMENT;
    const uint64_t idx[4] = {0, 9, 10, 3};
    last_error() = "untouched";
    // no index: the count is bounded by natoms; with an index it is not
    CHECK(check_no_index("fluct", "n", nullptr, 10, 10) == 0);
    CHECK(check_no_index("fluct", "n", idx, 11, 10) == 0);
    CHECK(check_no_index("msd", "nref", nullptr, 0, 0) == 0);
    CHECK(last_error() == "untouched");
    CHECK(failed_with(check_no_index("rmsd_matrix", "n", nullptr, 11, 10), INV, "rmsd_matrix: n = 11 exceeds natoms = 10 and there is no index"));
    CHECK(failed_with(check_no_index("msd_f64", "nref", nullptr, 7, 5), INV, "msd_f64: nref = 7 exceeds natoms = 5 and there is no index"));
    // the stride counts from the second frame on
    CHECK(check_stride("fluct", "the frame stride", 0, 0, 10) == 0);
    CHECK(check_stride("fluct", "the frame stride", 1, 0, 10) == 0);
    CHECK(check_stride("fluct", "the frame stride", 2, 30, 10) == 0);
    CHECK(failed_with(check_stride("fluct", "the frame stride", 2, 29, 10), INV, "fluct: the frame stride is below 3 * natoms = 30"));
    CHECK(failed_with(check_stride("rmsd_matrix_f64", "a frame stride", 3, 0, 4), INV, "rmsd_matrix_f64: a frame stride is below 3 * natoms = 12"));
    // the walk of an index in host memory: the first entry that is not below natoms
    CHECK(check_index("msd", "idx", nullptr, 4, 1) == 0);
    CHECK(check_index("msd", "idx", idx, 4, 11) == 0);
    CHECK(check_index("msd", "idx", idx, 2, 10) == 0);
    CHECK(check_index("msd", "idx", idx, 0, 0) == 0);
    CHECK(failed_with(check_index("msd", "idx", idx, 4, 10), INV, "msd: idx[2] = 10 is not below natoms = 10"));
    CHECK(failed_with(check_index("msd", "ref_idx", idx, 4, 9), INV, "msd: ref_idx[1] = 9 is not below natoms = 9"));
    std::vector<uint64_t> big(100000);
    for (size_t k = 0; k < big.size(); ++k) big[k] = k;
    CHECK(check_index("fluct", "idx", big.data(), big.size(), big.size()) == 0);
    CHECK(failed_with(check_index("fluct", "idx", big.data(), big.size(), big.size() - 1), INV, "fluct: idx[99999] = 99999 is not below natoms = 99999"));
}

// a DevBuf owns its memory: it cannot be copied, and a move leaves the source empty
static_assert(!std::is_copy_constructible<DevBuf>::value && !std::is_copy_assignable<DevBuf>::value, "a DevBuf is never copied");
static_assert(std::is_nothrow_move_constructible<DevBuf>::value, "a DevBuf moves without throwing");

// moves of buffers that hold nothing (no device call is made): source and target stay {nullptr, 0}
static void test_devbuf_move() {
    DevBuf a;
    DevBuf b(std::move(a));
    CHECK(a.p == nullptr && a.cap == 0 && b.p == nullptr && b.cap == 0);
    DevBuf c;
    c = std::move(b);
    CHECK(b.p == nullptr && b.cap == 0 && c.p == nullptr && c.cap == 0);
}

// "create on first use" and "delete (the buffers free themselves), null" with buffers that hold nothing (no device call is made)
struct State {
    DevBuf a, b;
    int tag = 7;
};

static void test_state() {
    State *slot = nullptr;
    State &s = state_of(slot);
    CHECK(slot == &s && s.tag == 7);
    s.tag = 8;
    CHECK(&state_of(slot) == &s && slot->tag == 8);
    release_state(slot);
    CHECK(slot == nullptr);
}

int main() {
    test_carve();
    test_even_splits();
    test_checks();
    test_state();
    test_devbuf_move();
    if (failures) {
        std::printf("%d traj-block checks FAILED\n", failures);
        return 1;
    }
    std::printf("all traj-block tests passed\n");
    return 0;
}
