// The record of a search's result sizes (mh::SearchSizes, molar_amd/csrc/common.hpp) on the host.  The plan and offsets kernels
// store its fields into pinned memory, the copy fallback of resident_enqueue (search.hip) copies into them: both rely on four
// 64-bit words at offsets 0, 8, 16, 24.  What the header asserts at compile time is checked here at run time, against raw
// words, so that a reordered or retyped field fails loudly.  No device is needed.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <type_traits>

#include "../../molar_amd/csrc/common.hpp"

using mh::SearchSizes;

static int failures = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);        \
            ++failures;                                                          \
        }                                                                        \
    } while (0)

int main() {
    CHECK(sizeof(SearchSizes) == 32);
    CHECK(alignof(SearchSizes) == 8);
    CHECK(std::is_trivially_copyable<SearchSizes>::value && std::is_standard_layout<SearchSizes>::value);

    // the words as the kernels of the commit before the record wrote them: [0] total, [1] hit-history units, [2] slots,
    // [3] occupied cells of set 1 << 32 | of set 0
    const unsigned long long words[4] = {0x1111222233334444ull, 0x5555666677778888ull, 0x99990000aaaabbbbull, (7ull << 32) | 5ull};
    SearchSizes s;
    std::memcpy(&s, words, sizeof s);
    CHECK(s.total == words[0]);
    CHECK(s.mask_units == words[1]);
    CHECK(s.slots == words[2]);
    CHECK(s.occupied == words[3]);
    CHECK((uint32_t)s.occupied == 5u && (uint32_t)(s.occupied >> 32) == 7u);

    // and the other way: fields written by name land in those words
    s = SearchSizes{};
    s.total = 1;
    s.mask_units = 2;
    s.slots = 3;
    s.occupied = 4;
    unsigned long long back[4];
    std::memcpy(back, &s, sizeof back);
    CHECK(back[0] == 1 && back[1] == 2 && back[2] == 3 && back[3] == 4);

    // a cleared record is all zero bytes (occupied == 0: not reported)
    s = SearchSizes{};
    const unsigned char zero[32] = {};
    CHECK(std::memcmp(&s, zero, 32) == 0);

    // the fallback's fill: the slot count is a u32 in device memory, copied as four bytes into the low half of a cleared `slots`
    const uint32_t nslots = 0xfedcba98u;
    const unsigned long long total = 123456789012345ull, units = 4321ull;
    std::memcpy(&s.total, &total, 8);
    std::memcpy(&s.mask_units, &units, 8);
    std::memcpy(&s.slots, &nslots, 4);
    CHECK(s.total == total && s.mask_units == units && s.slots == 0xfedcba98ull && s.occupied == 0);
    CHECK((const char *)&s.total - (const char *)&s == 0 && (const char *)&s.mask_units - (const char *)&s == 8 &&
          (const char *)&s.slots - (const char *)&s == 16 && (const char *)&s.occupied - (const char *)&s == 24);

    if (failures) {
        std::printf("%d search-sizes checks FAILED\n", failures);
        return 1;
    }
    std::printf("all search-sizes tests passed\n");
    return 0;
}
