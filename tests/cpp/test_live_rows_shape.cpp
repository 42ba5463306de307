// live_row_slots() and the size of a generation's live-row buffer (molar_amd/csrc/search_shape.hpp) on the host.  Which searches
// cut their slots from live rows changes no result - the oracle suites cannot see a rule that quietly says "never" or sizes the
// masks short - so the rule's cases and the buffer arithmetic are pinned here: expected values are worked out from the rule's
// text (regular family, fixed-cutoff kinds, plans of at most 2^22 entries; 96 atoms of the first set per cell of the grid on
// average, or a plan of at most 8192 entries; 8 mask words of 8 bytes and one 4-byte count per entry), not from what the code returns.
#include <cstdio>

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

static SearchShape shape(GridSet *sets, int kind, unsigned dx, unsigned dy, unsigned dz, unsigned n0, unsigned n1) {
    SearchShape s;
    s.kind = kind;
    s.dims[0] = dx; s.dims[1] = dy; s.dims[2] = dz;
    sets[0].n = n0;
    sets[1].n = n1;
    s.set = sets;
    return s;
}

int main() {
    GridSet sets[2];
    // the headline frame: 1M atoms, 16 x 16 x 15 cells of ~261 atoms
    SearchShape s = shape(sets, MOLAR_HIP_SEARCH_SINGLE, 16, 16, 15, 1000000, 0);
    CHECK(pair_family(s) == 0 && live_row_slots(s));
    CHECK(plan_entries(s) == 53760ull);
    CHECK(live_rows_mask_words(s) == 430080ull);                 // 53760 entries x 8 groups
    CHECK(live_rows_bytes(s) == 430080ull * 8ull + 53760ull * 4ull);
    // two grids: twice the entries
    s = shape(sets, MOLAR_HIP_SEARCH_DOUBLE, 4, 4, 4, 10000, 10000);
    CHECK(live_row_slots(s) && plan_entries(s) == 1792ull && live_rows_bytes(s) == 1792ull * 68ull);
    // the other kinds and the other kernel families keep consecutive slots
    s = shape(sets, MOLAR_HIP_SEARCH_DOUBLE_VDW, 4, 4, 4, 10000, 10000);
    CHECK(!live_row_slots(s));
    s = shape(sets, MOLAR_HIP_SEARCH_WITHIN, 4, 4, 4, 10000, 10000);
    CHECK(!live_row_slots(s));
    s = shape(sets, MOLAR_HIP_SEARCH_SINGLE, 10, 10, 10, 12000, 0);            // 12 atoms per cell: small-cell kernels
    CHECK(pair_family(s) == 16 && !live_row_slots(s));
    s = shape(sets, MOLAR_HIP_SEARCH_SINGLE, 4, 4, 4, 64 * 500, 0);            // 500 atoms per cell: wide instances
    CHECK(pair_family(s) == -1 && !live_row_slots(s));
    s = shape(sets, MOLAR_HIP_SEARCH_SINGLE, 4, 4, 4, 64 * 1100, 0);           // 1100: huge instances
    CHECK(pair_family(s) == -2 && !live_row_slots(s));
    // a slab in a mostly empty box: small cells by the mean, regular kernels once the occupied cells are known - and still
    // consecutive slots, since the liveness kernel's cost goes with ALL cells (13104 entries for 9720 atoms)
    s = shape(sets, MOLAR_HIP_SEARCH_SINGLE, 6, 6, 26, 9720, 0);
    CHECK(pair_family(s) != 0 && !live_row_slots(s));
    s.occ_use[0] = 144;
    CHECK(pair_family(s) == 0 && !live_row_slots(s));
    // the density rule: 1M atoms at 1.0 nm (21^3 cells, 108 per cell) yes, at 0.8 nm (26^3 cells, 57 per cell) no
    s = shape(sets, MOLAR_HIP_SEARCH_SINGLE, 21, 21, 21, 1000000, 0);
    CHECK(pair_family(s) == 0 && live_row_slots(s));
    s = shape(sets, MOLAR_HIP_SEARCH_SINGLE, 26, 26, 26, 1000000, 0);
    CHECK(pair_family(s) == 0 && !live_row_slots(s));
    // exactly 96 per cell qualifies, one atom fewer does not (1000 cells: 14000 entries, above the small-plan exemption)
    s = shape(sets, MOLAR_HIP_SEARCH_SINGLE, 10, 10, 10, 96 * 1000, 0);
    CHECK(live_row_slots(s));
    sets[0].n = 96 * 1000 - 1;
    CHECK(!live_row_slots(s));
    // it is the FIRST set's density that counts
    s = shape(sets, MOLAR_HIP_SEARCH_DOUBLE, 10, 10, 10, 40 * 1000, 300 * 1000);
    CHECK(pair_family(s) == 0 && plan_entries(s) == 28000ull && !live_row_slots(s));
    // small plans qualify whatever their density: 12 cells = 168 entries with 300 atoms; 585 cells = 8190 entries, 586 = 8204
    s = shape(sets, MOLAR_HIP_SEARCH_SINGLE, 3, 2, 2, 300, 0);
    CHECK(pair_family(s) == 0 && live_row_slots(s));
    s = shape(sets, MOLAR_HIP_SEARCH_SINGLE, 585, 1, 1, 585 * 30, 0);
    CHECK(pair_family(s) == 0 && live_row_slots(s));
    s = shape(sets, MOLAR_HIP_SEARCH_SINGLE, 586, 1, 1, 586 * 30, 0);
    CHECK(pair_family(s) == 0 && !live_row_slots(s));
    // plans beyond plan_tiles_kernel's reach never do
    s = shape(sets, MOLAR_HIP_SEARCH_SINGLE, 100, 100, 30, 100u * 300000u, 0);
    CHECK(plan_entries(s) + 1 > FPLAN_MAX_TASKS && pair_family(s) == 0 && !live_row_slots(s));
    if (failures) {
        std::printf("%d live-row shape checks FAILED\n", failures);
        return 1;
    }
    std::printf("all live-row shape tests passed\n");
    return 0;
}
