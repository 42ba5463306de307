// molar::lifetimes of the C++ host mirror (include/molar_hip.hpp) on one small presence matrix: 70 rows over 150 frames from a
// seeded on/off chain, with an empty row, a full row, a run across a word boundary, rows named twice in a frame and a frame
// without entries.  What to expect is computed here by the definition of molar_hip.h in plain C++ loops; every comparison is
// equality of integers.
#include <algorithm>
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

struct Expected {
    std::vector<uint64_t> inter, cont, hist, count;
    std::vector<uint32_t> events, longest, present;
};

static Expected expect(const std::vector<std::vector<int>> &h, const std::vector<uint32_t> &group, size_t G, size_t L, size_t s, size_t gap) {
    const size_t R = h.size(), F = h[0].size();
    std::vector<std::vector<int>> hp = h;
    for (size_t r = 0; r < R; ++r)
        for (size_t p = 0; p < F; ++p)
            for (size_t q = p + 2; q < F && q - p - 1 <= gap; ++q)
                if (h[r][p] && h[r][q])
                    for (size_t u = p + 1; u < q; ++u) hp[r][u] = 1;
    Expected e;
    e.inter.assign(G * (L + 1), 0);
    e.cont.assign(G * (L + 1), 0);
    e.hist.assign(G * (F + 1), 0);
    e.events.assign(R, 0);
    e.longest.assign(R, 0);
    e.present.assign(R, 0);
    for (size_t tau = 0; tau <= L; ++tau) e.count.push_back((F - 1 - tau) / s + 1);
    for (size_t r = 0; r < R; ++r) {
        const size_t g = group.empty() ? 0 : group[r];
        for (size_t tau = 0; tau <= L; ++tau)
            for (size_t t = 0; t + tau <= F - 1; t += s) {
                e.inter[g * (L + 1) + tau] += hp[r][t] * hp[r][t + tau];
                int all = 1;
                for (size_t u = t; u <= t + tau; ++u) all *= hp[r][u];
                e.cont[g * (L + 1) + tau] += all;
            }
        uint32_t run = 0;
        for (size_t u = 0; u <= F; ++u) {
            if (u < F && hp[r][u]) {
                ++run;
                ++e.present[r];
            } else if (run) {
                ++e.hist[g * (F + 1) + run];
                ++e.events[r];
                e.longest[r] = std::max(e.longest[r], run);
                run = 0;
            }
        }
    }
    return e;
}

static bool same(const Lifetimes &got, const Expected &e) {
    return got.inter == e.inter && got.cont == e.cont && got.run_hist == e.hist && got.count == e.count && got.events == e.events &&
           got.longest == e.longest && got.present == e.present;
}

int main() {
    const size_t R = 70, F = 150;
    std::vector<std::vector<int>> h(R, std::vector<int>(F, 0));
    for (size_t r = 0; r < R; ++r) {
        bool on = uniform() < 0.4;
        for (size_t t = 0; t < F; ++t) {
            h[r][t] = on;
            on = on ? uniform() >= 0.25 : uniform() < 0.15;
        }
    }
    for (size_t t = 0; t < F; ++t) {
        h[0][t] = 0;                                   // an empty row
        h[1][t] = 1;                                   // a full row
        h[2][t] = t >= 60 && t < 70;                   // a run across a word boundary
        h[3][t] = t == 63 || t == 65 || t == 128;      // a gap of one frame across a word boundary
    }
    for (size_t r = 0; r < R; ++r) h[r][77] = 0;       // a frame without entries
    std::vector<uint64_t> off{0};
    std::vector<uint32_t> rows, group(R);
    for (size_t t = 0; t < F; ++t) {
        for (size_t k = 0; k < R; ++k) {
            const size_t r = (k * 37 + t) % R;         // the rows of a frame in an order of its own
            if (h[r][t]) rows.push_back((uint32_t)r);
        }
        if (t % 5 == 0 && off.back() < rows.size()) rows.push_back(rows.back());      // a row named twice
        off.push_back(rows.size());
    }
    for (size_t r = 0; r < R; ++r) group[r] = (uint32_t)(r % 3 == 2 ? 3 : r % 3);      // group 2 of 4 stays empty

    Engine eng(0);
    const Lifetimes a = lifetimes(eng, off, rows, R);
    EXPECT(a.max_lag == F - 1 && a.ngroups == 1);
    EXPECT(same(a, expect(h, {}, 1, F - 1, 1, 0)));
    EXPECT(a.present[1] == F - 1 && a.longest[2] == 10 && a.events[0] == 0);

    LifetimeOptions opt;
    opt.max_lag = 129;
    opt.origin_stride = 7;
    opt.gap = 1;
    opt.ngroups = 4;
    const Lifetimes b = lifetimes(eng, off, rows, R, group, opt);
    EXPECT(same(b, expect(h, group, 4, 129, 7, 1)));
    EXPECT(b.present[3] == 4);                         // frame 64 was filled

    // the call's own errors, and the chained call without a block
    bool threw = false;
    try {
        opt.max_lag = F;
        lifetimes(eng, off, rows, R, group, opt);
    } catch (const MolarError &) {
        threw = true;
    }
    EXPECT(threw);
    threw = false;
    try {
        hbonds_frames_lifetimes(eng, HBonds());
    } catch (const MolarError &) {
        threw = true;
    }
    EXPECT(threw);

    if (failures == 0) std::printf("all lifetimes host-mirror tests passed (%zu entries)\n", rows.size());
    return failures ? 1 : 0;
}
