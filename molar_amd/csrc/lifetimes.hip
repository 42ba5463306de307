// lifetimes.hip - lifetime correlations of a sparse presence matrix frames x rows (the bond table of a block of hydrogen bonds,
// contacts, the members of a shell): the intermittent and the continuous correlation numerators, the run-length distribution
// and per-row statistics.  The definition is in molar_hip.h.  Presence is one bit, a lag is a shift, a product is an AND, a sum
// is a popcount; every result is an integer.
//
//   bits[R][W + 1], W = ceil(F / 64) 64-bit words per row and one word of zeros behind them; bits at or above F stay 0, which
//   alone enforces t + tau <= F - 1.
//
// Stages, all on the context's stream:
//
//   pack     one lane per entry: its frame by bisection of the offsets (inside the bracket the workgroup's first and last entry
//            give), its bit by one vector integer atomic OR.  A row that is not below R raises a flag and touches nothing; labels
//            in device memory are judged by a kernel of their own.
//   ->  16 bytes read back: the status.  Nothing below runs, and no output is touched, after a bad row or label.
//   gap      (g > 0) one lane per row walks its set bits in order and fills the zero runs of at most g frames between two of them,
//            in place, across word boundaries.
//   masks    one lane per word: the origins t = 0, s, 2 s, ... below F.
//   inter    the hot path: a wave owns a chunk of rows and LT_NQ lag words q, one lane per sub-word shift sh: tau = 64 q + sh.
//            b[w], b[w + q] and b[w + q + 1] are the same for the whole wave (scalar loads: LT_STEP words of origins per wait,
//            then the words behind them at the wave's lags per wait); a word pair costs a lane a shift each way, two ORs, two ANDs, two
//            popcounts and an add, and the shifts of a word serve two pairs.  Words without a present origin are skipped on a
//            uniform branch.  The sums stay in registers over the words and over the rows while the group does not change; then
//            one 64-bit integer atomic per lane and lag word.
//   runs     one lane per row walks its runs: events, longest, present, one count per run into the run-length histogram and,
//            for an origin stride above 1, one per present origin into the histogram of the frames that remain of its run; the
//            short runs of the first groups meet in LDS and leave with one atomic per bin and workgroup.
//   cont     one lane per (group, tau): cont[tau] = sum_l hist[l] max(0, l - tau) for stride 1; the origins whose run goes on for
//            tau frames or more otherwise.
//
// Integer atomics only: the same call gives the same bits.
#include <algorithm>
#include <vector>

#include "common.hpp"
#include "traj_block.hpp"

using namespace mh;

struct molar_hip_lifetimes_state {
    DevBuf in_off, in_rows, in_grp;                                      // host inputs staged here
    DevBuf ws;                                                           // the workspace molar_hip_lifetimes_plan reports
    DevBuf out_inter, out_cont, out_hist, out_ev, out_long, out_pres;    // results of a call whose destinations are host memory
};

namespace {

typedef unsigned long long u64;

constexpr uint32_t LT_WG = 256;              // lanes per workgroup of the per-entry, per-row and per-lag kernels
constexpr size_t LT_TARGET_WAVES = 32768;    // waves the intermittent kernel aims for
constexpr uint32_t LT_MAX_CHUNK = 1024;      // rows per wave at the most
constexpr uint32_t LT_STEP = 4;              // words of origins per step of the intermittent kernel's unrolled loop
constexpr uint32_t LT_NQ = 4;                // lag words (64 lags each) per wave of the intermittent kernel

// Where everything lives in the workspace, from the sizes alone (the plan entry and the call share it).
struct Layout {
    size_t W, Wp;                 // words per row, and with the word of zeros behind them
    size_t off_flags, off_bits, off_masks, off_hist, bytes;
};

Layout make_layout(size_t F, size_t R, size_t G, bool want_cont) {
    Layout Y{};
    Y.W = (F + 63) / 64;
    Y.Wp = Y.W + 1;
    Carve ws;
    ws.take(Y.off_flags, 16);
    ws.take(Y.off_bits, R * Y.Wp * 8);
    ws.take(Y.off_masks, Y.W * 8);
    ws.take(Y.off_hist, want_cont ? G * (F + 1) * 8 : 0);
    Y.bytes = ws.bytes;
    return Y;
}

inline unsigned blocks_of(size_t n) { return (unsigned)((n + LT_WG - 1) / LT_WG); }

// the frame of entry e, given off[lo] <= e < off[hi]: the last frame whose offset is not above e (frames without entries are
// passed over)
__device__ __forceinline__ uint32_t lt_frame_of(const u64 *__restrict__ off, u64 e, uint32_t lo, uint32_t hi) {
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (off[mid] <= e) lo = mid;
        else hi = mid;
    }
    return lo;
}

// One lane per entry.  flags[0]: a row that is not below R (nothing is written for it).
__global__ void __launch_bounds__(LT_WG) lt_pack_kernel(const u64 *__restrict__ off, const uint32_t *__restrict__ row_of_entry, u64 E, uint32_t F,
                                                        u64 R, size_t Wp, u64 *__restrict__ bits, uint32_t *__restrict__ flags) {
    // the frames of the workgroup's first and last entry, found by one lane each, bracket those of all the others
    __shared__ uint32_t sh_frame[2];
    const u64 e0 = (u64)blockIdx.x * LT_WG, e1 = E - e0 > LT_WG ? e0 + LT_WG - 1u : E - 1u, e = e0 + threadIdx.x;
    if (threadIdx.x == 0u) sh_frame[0] = lt_frame_of(off, e0, 0u, F);
    if (threadIdx.x == 64u) sh_frame[1] = lt_frame_of(off, e1, 0u, F);
    __syncthreads();
    if (e >= E) return;
    const u64 r = row_of_entry[e];
    if (r >= R) {
        flags[0] = 1u;
        return;
    }
    const uint32_t t = lt_frame_of(off, e, sh_frame[0], sh_frame[1] + 1u);
    atomicOr(&bits[r * Wp + (t >> 6)], 1ull << (t & 63u));
}

// flags[1]: a label that is not below the number of groups
__global__ void __launch_bounds__(LT_WG) lt_labels_kernel(const uint32_t *__restrict__ grp, size_t R, u64 G, uint32_t *__restrict__ flags) {
    for (size_t i = (size_t)blockIdx.x * LT_WG + threadIdx.x; i < R; i += (size_t)gridDim.x * LT_WG)
        if (grp[i] >= G) flags[1] = 1u;
}

// bits [lo, hi) of a row set, hi > lo
__device__ __forceinline__ void lt_fill(u64 *__restrict__ b, u64 lo, u64 hi) {
    const u64 w0 = lo >> 6, w1 = (hi - 1) >> 6;
    for (u64 w = w0; w <= w1; ++w) {
        u64 m = ~0ull;
        if (w == w0) m &= ~0ull << (lo & 63u);
        if (w == w1) m &= ~0ull >> (63u - ((hi - 1) & 63u));
        b[w] |= m;
    }
}

// One lane per row: the closing by g along the frame axis, in place.  The set bits go by in order; a fill only sets bits below
// the one in hand, so the word in the register stays the original one.
__global__ void __launch_bounds__(LT_WG) lt_gap_kernel(u64 *__restrict__ bits, size_t R, size_t W, size_t Wp, u64 g) {
    const size_t r = (size_t)blockIdx.x * LT_WG + threadIdx.x;
    if (r >= R) return;
    u64 *b = bits + r * Wp;
    bool any = false;
    u64 last = 0;
    for (size_t w = 0; w < W; ++w) {
        u64 x = b[w];
        while (x) {
            const u64 p = (u64)w * 64u + (u64)__builtin_ctzll(x);
            x &= x - 1;
            if (any && p - last > 1 && p - last - 1 <= g) lt_fill(b, last + 1, p);
            any = true;
            last = p;
        }
    }
}

// One lane per word: the origins below F.
__global__ void __launch_bounds__(LT_WG) lt_masks_kernel(u64 *__restrict__ masks, size_t W, u64 F, u64 s) {
    const size_t w = (size_t)blockIdx.x * LT_WG + threadIdx.x;
    if (w >= W) return;
    const u64 t0 = (u64)w * 64u;
    u64 m = 0;
    for (u64 t = (t0 + s - 1) / s * s; t < t0 + 64u && t < F; t += s) m |= 1ull << (t - t0);
    masks[w] = m;
}

// cnt + the present origins of the word `a` (masked) whose bit sh frames on, in the words (lo, hi) that follow, is set as well
__device__ __forceinline__ uint32_t lt_pair(u64 a, u64 lo, u64 hi, uint32_t sh, uint32_t cnt) {
    const u64 x = ((lo >> sh) | ((hi << 1) << (63u - sh))) & a;
    // v_bcnt_u32_b32 adds its count to an operand: written out, because the compiler forms two counts from zero and a v_add3
    uint32_t half, both;
    asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(half) : "v"((uint32_t)x), "v"(cnt));
    asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(both) : "v"((uint32_t)(x >> 32)), "v"(half));
    return both;
}

// The intermittent numerator.  Workgroup = one wave = (LT_NQ lag words q0 .. q0 + LT_NQ - 1, chunk of rows), blockIdx.x =
// (q0 / LT_NQ) * nchunks + chunk, so that the short lags - the long sums - start first; lane sh holds the lags tau = 64 (q0 + j) + sh,
// one count each.  Bit i of the row shifted by tau, word w, is bit 64 (w + q) + sh + i of the row: (b[w + q] >> sh) |
// (b[w + q + 1] << (64 - sh)), the second term in two steps because a shift by 64 is none.  The words of a row are the same for
// the whole wave (scalar loads); LT_STEP words of origins with their masks are waited for and decide the skip, then the
// LT_STEP + LT_NQ words that follow them at the wave's lags (the compiler keeps their loads behind the skip branch: a second
// wait); together they serve LT_STEP x LT_NQ word pairs.
__global__ void __launch_bounds__(64) lt_inter_kernel(const u64 *__restrict__ bits, const u64 *__restrict__ masks, const uint32_t *__restrict__ grp,
                                                      u64 *__restrict__ inter, uint32_t R, uint32_t W, uint32_t Wp, uint32_t chunk,
                                                      uint32_t nchunks, u64 L) {
    const uint32_t qb = blockIdx.x / nchunks, ch = blockIdx.x - qb * nchunks, q0 = qb * LT_NQ;
    const uint32_t sh = threadIdx.x;
    const uint32_t r0 = ch * chunk, r1 = R - r0 < chunk ? R : r0 + chunk;
    // words w with w + q <= W - 1 for the last lag word of the wave (all LT_NQ go together there) ...
    const uint32_t nw_all = q0 + LT_NQ - 1u < W ? W - (q0 + LT_NQ - 1u) : 0u;
    uint32_t cur = grp ? grp[r0] : 0u;
    u64 acc[LT_NQ];
#pragma unroll
    for (uint32_t j = 0; j < LT_NQ; ++j) acc[j] = 0;
    auto flush = [&](uint32_t g) {
#pragma unroll
        for (uint32_t j = 0; j < LT_NQ; ++j) {
            const u64 tau = (u64)(q0 + j) * 64u + sh;
            if (tau <= L && acc[j]) atomicAdd(&inter[(size_t)g * (L + 1) + tau], acc[j]);
            acc[j] = 0;
        }
    };
    for (uint32_t r = r0; r < r1; ++r) {
        const uint32_t g = grp ? grp[r] : 0u;
        if (g != cur) {
            flush(cur);
            cur = g;
        }
        const u64 *__restrict__ b = bits + (size_t)r * Wp;
        uint32_t cnt[LT_NQ];                         // (a row's count stays below F < 2^31)
#pragma unroll
        for (uint32_t j = 0; j < LT_NQ; ++j) cnt[j] = 0;
        uint32_t w = 0;
        for (; w + LT_STEP <= nw_all; w += LT_STEP) {
            u64 a[LT_STEP], c[LT_STEP + LT_NQ], any = 0;
#pragma unroll
            for (uint32_t k = 0; k < LT_STEP; ++k) a[k] = b[w + k] & masks[w + k];
#pragma unroll
            for (uint32_t k = 0; k < LT_STEP + LT_NQ; ++k) c[k] = b[w + q0 + k];
#pragma unroll
            for (uint32_t k = 0; k < LT_STEP; ++k) any |= a[k];
            if (any == 0ull) continue;
#pragma unroll
            for (uint32_t j = 0; j < LT_NQ; ++j)
#pragma unroll
                for (uint32_t k = 0; k < LT_STEP; ++k) cnt[j] = lt_pair(a[k], c[k + j], c[k + j + 1], sh, cnt[j]);
        }
        // ... and the words that are left, lag word by lag word: w + q <= W - 1
#pragma unroll
        for (uint32_t j = 0; j < LT_NQ; ++j) {
            const uint32_t q = q0 + j, nw = q < W ? W - q : 0u;
            for (uint32_t v = w; v < nw; ++v) {
                const u64 a = b[v] & masks[v];
                if (a == 0ull) continue;
                cnt[j] = lt_pair(a, b[v + q], b[v + q + 1], sh, cnt[j]);
            }
        }
#pragma unroll
        for (uint32_t j = 0; j < LT_NQ; ++j) acc[j] += cnt[j];
    }
    flush(cur);
}

struct LtRuns {
    const u64 *bits;
    const uint32_t *grp;
    size_t R, W, Wp;
    u64 F, s;
    u64 *hist;                    // [G][F + 1] runs by length, or null
    u64 *rem;                     // [G][F + 1] present origins by the frames that remain of their run, or null
    uint32_t *events, *longest, *present;
    uint32_t *flags;              // flags[2]: the longest run of all rows
    uint32_t nshort;              // bins below this are counted in LDS first (LT_SHORT, or 0 when 32 bits may not hold a workgroup's count)
};

constexpr uint32_t LT_SHORT = 256;           // run lengths (and remainders) below this and ...
constexpr uint32_t LT_FEW = 8;               // ... groups below this are counted in LDS first: short runs of few groups are the many

// one more in bin k of the histogram h of group g: in the workgroup's LDS copy when it has the bin
__device__ __forceinline__ void lt_count(u64 *__restrict__ h, uint32_t *sh, size_t g, u64 k, u64 F, uint32_t nshort) {
    if (g < LT_FEW && k < nshort) atomicAdd(&sh[g * LT_SHORT + k], 1u);
    else atomicAdd(&h[g * (F + 1) + k], 1ull);
}

// the run [e - len, e) of a row of group g ends
__device__ __forceinline__ void lt_close(const LtRuns &P, uint32_t *sh_hist, uint32_t *sh_rem, size_t g, u64 e, u64 len, uint32_t &events,
                                         uint32_t &longest) {
    ++events;
    if (len > longest) longest = (uint32_t)len;
    if (P.hist) lt_count(P.hist, sh_hist, g, len, P.F, P.nshort);
    if (P.rem) {
        const u64 a = e - len;
        for (u64 t = (a + P.s - 1) / P.s * P.s; t < e; t += P.s) lt_count(P.rem, sh_rem, g, e - 1 - t, P.F, P.nshort);
    }
}

// One lane per row: its runs in order, with the length of an open run carried across the words.  The counts of a workgroup meet
// in LDS (32-bit bins: a row adds fewer than F to one, and the host hands in nshort = 0 unless LT_WG rows of F fit) and go out with
// one atomic per bin that is not zero.
__global__ void __launch_bounds__(LT_WG) lt_runs_kernel(LtRuns P) {
    __shared__ uint32_t sh_hist[LT_FEW * LT_SHORT], sh_rem[LT_FEW * LT_SHORT];
    for (uint32_t i = threadIdx.x; i < LT_FEW * LT_SHORT; i += LT_WG) {
        sh_hist[i] = 0u;
        sh_rem[i] = 0u;
    }
    __syncthreads();
    const size_t r = (size_t)blockIdx.x * LT_WG + threadIdx.x;
    if (r < P.R) {
        const u64 *__restrict__ b = P.bits + r * P.Wp;
        const size_t g = P.grp ? P.grp[r] : 0u;
        uint32_t events = 0, longest = 0, present = 0;
        u64 run = 0;
        for (size_t w = 0; w < P.W; ++w) {
            const u64 x = b[w];
            present += (uint32_t)__builtin_popcountll(x);
            if (x == ~0ull) {
                run += 64u;
                continue;
            }
            uint32_t pos = 0;
            while (pos < 64u) {
                const u64 y = x >> pos;                  // bit 0: frame 64 w + pos; zeros come in from above
                if (y & 1ull) {
                    const uint32_t n = (uint32_t)__builtin_ctzll(~y);        // y is not all ones: x is not, or pos > 0
                    run += n;
                    pos += n;
                    if (pos < 64u) {
                        lt_close(P, sh_hist, sh_rem, g, (u64)w * 64u + pos, run, events, longest);
                        run = 0;
                    }
                } else {
                    if (run) {                           // (only at pos == 0: the run of the word before ends here)
                        lt_close(P, sh_hist, sh_rem, g, (u64)w * 64u + pos, run, events, longest);
                        run = 0;
                    }
                    pos += y ? (uint32_t)__builtin_ctzll(y) : 64u - pos;
                }
            }
        }
        if (run) lt_close(P, sh_hist, sh_rem, g, (u64)P.W * 64u, run, events, longest);      // (F is a multiple of 64 then: bits at or above F are 0)
        if (P.events) P.events[r] = events;
        if (P.longest) P.longest[r] = longest;
        if (P.present) P.present[r] = present;
        if (longest) atomicMax(&P.flags[2], longest);
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < LT_FEW * LT_SHORT; i += LT_WG) {
        const size_t at = (size_t)(i / LT_SHORT) * (P.F + 1) + i % LT_SHORT;
        if (sh_hist[i]) atomicAdd(&P.hist[at], (u64)sh_hist[i]);
        if (sh_rem[i]) atomicAdd(&P.rem[at], (u64)sh_rem[i]);
    }
}

// The continuous numerator, one lane per (group, tau), blockIdx.x = group * nblk + block of lags.  STRIDE1: from the runs by
// length, a run of l frames holds l - tau origins whose run goes on for tau frames more; otherwise from the present origins by
// the frames that remain of their run.
template <bool STRIDE1>
__global__ void __launch_bounds__(LT_WG) lt_cont_kernel(const u64 *__restrict__ h, const uint32_t *__restrict__ flags, u64 F, u64 L, uint32_t nblk,
                                                        u64 *__restrict__ cont) {
    const size_t g = blockIdx.x / nblk;
    const u64 tau = (u64)(blockIdx.x - g * nblk) * LT_WG + threadIdx.x;
    if (tau > L) return;
    const u64 *__restrict__ row = h + g * (F + 1);
    const u64 top = flags[2];                        // the longest run of all rows
    u64 sum = 0;
    if (STRIDE1) {
        for (u64 l = tau + 1; l <= top; ++l) sum += row[l] * (l - tau);
    } else {
        for (u64 k = tau; k < top; ++k) sum += row[k];
    }
    cont[g * (L + 1) + tau] = sum;
}

// What a call needs once its arguments have been judged: offsets in host memory (judged there) and, when the caller's are in
// device memory, those as well; rows in host or device memory.
struct LtCall {
    const char *who;
    const uint64_t *off_host, *off_dev;
    const uint32_t *rows;
    size_t F, R, E;
};

int lt_run(molar_hip_ctx *c, const LtCall &X, const uint32_t *group_of_row, size_t ngroups, size_t max_lag, size_t origin_stride, size_t gap,
           uint64_t *inter, uint64_t *cont, uint64_t *run_hist, uint32_t *events, uint32_t *longest, uint32_t *present) {
    const char *who = X.who;
    const size_t F = X.F, R = X.R, E = X.E, L = max_lag, G = group_of_row ? ngroups : 1;
    if (L >= F) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: max_lag = %zu is not below nframes = %zu", who, L, F);
    if (origin_stride == 0) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: origin_stride is zero", who);
    if (X.off_host[0] != 0) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: frame_offsets start at %llu, not at 0", who, (unsigned long long)X.off_host[0]);
    for (size_t t = 0; t < F; ++t)
        if (X.off_host[t + 1] < X.off_host[t]) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: frame_offsets decrease at frame %zu", who, t);
    if (X.off_host[F] != E) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: frame_offsets end at %llu, not at the %zu entries", who, (unsigned long long)X.off_host[F], E);
    if (E && !X.rows) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: %zu entries and row_of_entry is null", who, E);
    if (E >= 0x100000000ull) return fail(MOLAR_HIP_ERR_TOO_LARGE, "%s: 2^32 entries or more", who);
    if (F >= 0x7FFFFFF0ull) return fail(MOLAR_HIP_ERR_TOO_LARGE, "%s: 2^31 frames or more", who);
    if (R > 0x100000000ull) return fail(MOLAR_HIP_ERR_TOO_LARGE, "%s: more than 2^32 rows", who);
    if (group_of_row && G == 0) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: a label is not below ngroups = 0", who);
    // rows and labels in host memory are walked here; those in device memory are judged by the kernels (flags, below)
    const bool rows_dev = is_device_ptr(X.rows), grp_dev = is_device_ptr(group_of_row);
    if (!rows_dev)
        for (size_t e = 0; e < E; ++e)
            if (X.rows[e] >= R) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: row_of_entry[%zu] = %u is not below nrows = %zu", who, e, X.rows[e], R);
    if (group_of_row && !grp_dev)
        for (size_t r = 0; r < R; ++r)
            if (group_of_row[r] >= G) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: group_of_row[%zu] = %u is not below ngroups = %zu", who, r, group_of_row[r], G);
    const bool want_runs = cont || run_hist || events || longest || present;
    const bool stride1 = origin_stride == 1 || F == 1;
    const Layout Y = make_layout(F, R, G, cont != nullptr);
    const size_t nq = (L / 64 + LT_NQ) / LT_NQ;           // waves along the lags: LT_NQ lag words each
    const size_t chunk = std::max<size_t>(1, std::min<size_t>(LT_MAX_CHUNK, R * nq / LT_TARGET_WAVES));
    const size_t nchunks = (R + chunk - 1) / chunk, nblk = (L + LT_WG) / LT_WG;
    if (R >= 0xFFFFFF00ull || Y.W >= 0x7FFFFFFFull || nq * nchunks >= 0x7FFFFFFFull || G * nblk >= 0x7FFFFFFFull)
        return fail(MOLAR_HIP_ERR_TOO_LARGE, "%s: %zu rows, %zu groups and %zu lags are more than a launch takes", who, R, G, L + 1);

    molar_hip_lifetimes_state &Z = state_of(c->lifetimes);
    MH_TRY(grow_exact(Z.ws, Y.bytes, who, "the workspace"));
    char *Wk = Z.ws.as<char>();
    uint32_t *flags = reinterpret_cast<uint32_t *>(Wk + Y.off_flags);
    u64 *bits = reinterpret_cast<u64 *>(Wk + Y.off_bits), *masks = reinterpret_cast<u64 *>(Wk + Y.off_masks);
    u64 *tmp = reinterpret_cast<u64 *>(Wk + Y.off_hist);
    const uint64_t *off_dev = X.off_dev;
    const uint32_t *rows_d = nullptr, *grp_d = nullptr;
    if (!off_dev) MH_TRY(to_device(c, X.off_host, F + 1, Z.in_off, &off_dev));
    MH_TRY(to_device(c, X.rows, E, Z.in_rows, &rows_d));
    MH_TRY(to_device(c, group_of_row, group_of_row ? R : 0, Z.in_grp, &grp_d));
    u64 *inter_d, *cont_d, *hist_d;
    uint32_t *ev_d, *long_d, *pres_d;
    MH_TRY(out_buffer(reinterpret_cast<u64 *>(inter), G * (L + 1), Z.out_inter, who, &inter_d));
    MH_TRY(out_buffer(reinterpret_cast<u64 *>(cont), G * (L + 1), Z.out_cont, who, &cont_d));
    MH_TRY(out_buffer(reinterpret_cast<u64 *>(run_hist), G * (F + 1), Z.out_hist, who, &hist_d));
    MH_TRY(out_buffer(events, R, Z.out_ev, who, &ev_d));
    MH_TRY(out_buffer(longest, R, Z.out_long, who, &long_d));
    MH_TRY(out_buffer(present, R, Z.out_pres, who, &pres_d));

    MH_HIP(hipMemsetAsync(flags, 0, 16, c->stream));
    MH_HIP(hipMemsetAsync(bits, 0, R * Y.Wp * 8, c->stream));
    if (E)
        hipLaunchKernelGGL(lt_pack_kernel, dim3(blocks_of(E)), dim3(LT_WG), 0, c->stream, reinterpret_cast<const u64 *>(off_dev), rows_d, (u64)E,
                           (uint32_t)F, (u64)R, Y.Wp, bits, flags);
    if (grp_dev) hipLaunchKernelGGL(lt_labels_kernel, dim3(std::min(blocks_of(R), 1024u)), dim3(LT_WG), 0, c->stream, grp_d, R, (u64)G, flags);
    MH_HIP(hipGetLastError());
    // the rows and the labels decide the status: 16 bytes read back before a kernel uses a label as an address or an output is touched
    uint32_t hf[4];
    MH_TRY(read_back(c, hf, flags, sizeof hf));
    if (hf[0]) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: an entry of row_of_entry is not below nrows = %zu", who, R);
    if (hf[1]) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: an entry of group_of_row is not below ngroups = %zu", who, G);

    if (gap > 0 && F > 2) hipLaunchKernelGGL(lt_gap_kernel, dim3(blocks_of(R)), dim3(LT_WG), 0, c->stream, bits, R, Y.W, Y.Wp, (u64)gap);
    if (inter_d) {
        hipLaunchKernelGGL(lt_masks_kernel, dim3(blocks_of(Y.W)), dim3(LT_WG), 0, c->stream, masks, Y.W, (u64)F, (u64)std::min(origin_stride, F));
        MH_HIP(hipMemsetAsync(inter_d, 0, G * (L + 1) * 8, c->stream));
        hipLaunchKernelGGL(lt_inter_kernel, dim3((uint32_t)(nq * nchunks)), dim3(64), 0, c->stream, bits, masks, grp_d, inter_d, (uint32_t)R,
                           (uint32_t)Y.W, (uint32_t)Y.Wp, (uint32_t)chunk, (uint32_t)nchunks, (u64)L);
    }
    if (want_runs) {
        // the runs by length go to the caller's histogram when there is one, else (stride 1, where the continuous numerator is made
        // of them) to the workspace's; the present origins by what remains of their run (other strides) to the workspace's
        LtRuns P{};
        P.bits = bits;
        P.grp = grp_d;
        P.R = R;
        P.W = Y.W;
        P.Wp = Y.Wp;
        P.F = F;
        P.s = std::min(origin_stride, F);            // beyond F - 1 there is the origin 0 alone either way
        P.hist = hist_d ? hist_d : (cont_d && stride1 ? tmp : nullptr);
        P.rem = cont_d && !stride1 ? tmp : nullptr;
        P.events = ev_d;
        P.longest = long_d;
        P.present = pres_d;
        P.flags = flags;
        P.nshort = F < ((size_t)1 << 24) ? LT_SHORT : 0u;
        if (hist_d) MH_HIP(hipMemsetAsync(hist_d, 0, G * (F + 1) * 8, c->stream));
        if (cont_d && (P.rem || !hist_d)) MH_HIP(hipMemsetAsync(tmp, 0, G * (F + 1) * 8, c->stream));
        hipLaunchKernelGGL(lt_runs_kernel, dim3(blocks_of(R)), dim3(LT_WG), 0, c->stream, P);
        if (cont_d) {
            if (stride1) hipLaunchKernelGGL(lt_cont_kernel<true>, dim3((uint32_t)(G * nblk)), dim3(LT_WG), 0, c->stream, P.hist, flags, (u64)F, (u64)L, (uint32_t)nblk, cont_d);
            else hipLaunchKernelGGL(lt_cont_kernel<false>, dim3((uint32_t)(G * nblk)), dim3(LT_WG), 0, c->stream, P.rem, flags, (u64)F, (u64)L, (uint32_t)nblk, cont_d);
        }
    }
    MH_HIP(hipGetLastError());
    bool wait = true;                                // device destinations are waited for as well: the call returns a result
    MH_TRY(copy_out(c, reinterpret_cast<u64 *>(inter), inter_d, G * (L + 1), wait));
    MH_TRY(copy_out(c, reinterpret_cast<u64 *>(cont), cont_d, G * (L + 1), wait));
    MH_TRY(copy_out(c, reinterpret_cast<u64 *>(run_hist), hist_d, G * (F + 1), wait));
    MH_TRY(copy_out(c, events, ev_d, R, wait));
    MH_TRY(copy_out(c, longest, long_d, R, wait));
    MH_TRY(copy_out(c, present, pres_d, R, wait));
    return finish_copies(c, wait);
}

}  // namespace

namespace mh {
void lifetimes_release(molar_hip_ctx *c) {
    release_state(c->lifetimes);
}
}  // namespace mh

extern "C" {

int molar_hip_lifetimes_plan(size_t nframes, size_t nrows, size_t ngroups, int want_cont, size_t *workspace_bytes, uint32_t *words_per_row) {
    const Layout Y = make_layout(nframes, nrows, ngroups ? ngroups : 1, want_cont != 0);
    const bool none = nframes == 0 || nrows == 0;
    if (workspace_bytes) *workspace_bytes = none ? 0 : Y.bytes;
    if (words_per_row) *words_per_row = (uint32_t)Y.W;
    return MOLAR_HIP_OK;
}

int molar_hip_lifetimes(molar_hip_ctx *c, const uint64_t *frame_offsets, const uint32_t *row_of_entry, size_t nframes, size_t nrows,
                        const uint32_t *group_of_row, size_t ngroups, size_t max_lag, size_t origin_stride, size_t gap, uint64_t *inter,
                        uint64_t *cont, uint64_t *run_hist, uint32_t *events, uint32_t *longest, uint32_t *present) {
    MH_CTX(c);
    if (nrows == 0 || nframes == 0) return fail(MOLAR_HIP_ERR_SIZES, "lifetimes: %zu rows and %zu frames", nrows, nframes);
    if (!frame_offsets) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "lifetimes: frame_offsets is null");
    if (nframes >= 0x7FFFFFF0ull) return fail(MOLAR_HIP_ERR_TOO_LARGE, "lifetimes: 2^31 frames or more");
    // the offsets are judged on the host
    std::vector<uint64_t> off_host;
    LtCall X{"lifetimes", frame_offsets, nullptr, row_of_entry, nframes, nrows, 0};
    if (is_device_ptr(frame_offsets)) {
        off_host.resize(nframes + 1);
        MH_HIP(hipMemcpy(off_host.data(), frame_offsets, (nframes + 1) * 8, hipMemcpyDeviceToHost));
        X.off_host = off_host.data();
        X.off_dev = frame_offsets;
    }
    X.E = (size_t)X.off_host[nframes];
    return lt_run(c, X, group_of_row, ngroups, max_lag, origin_stride, gap, inter, cont, run_hist, events, longest, present);
}

int molar_hip_hbonds_frames_shape(molar_hip_ctx *c, size_t *nframes, size_t *nrows, size_t *nentries, uint64_t *serial) {
    MH_CTX(c);
    HbondsBlockView B;
    if (!hbonds_block_view(c, &B))
        return fail(MOLAR_HIP_ERR_NO_SEARCH, "hbonds_frames_shape: no hydrogen bonds of a block are cached (molar_hip_hbonds_frames first)");
    if (nframes) *nframes = B.nframes;
    if (nrows) *nrows = B.rows;
    if (nentries) *nentries = B.entries;
    if (serial) *serial = B.serial;
    return MOLAR_HIP_OK;
}

int molar_hip_hbonds_frames_lifetimes(molar_hip_ctx *c, const uint32_t *group_of_row, size_t ngroups, size_t max_lag, size_t origin_stride,
                                      size_t gap, uint64_t *inter, uint64_t *cont, uint64_t *run_hist, uint32_t *events, uint32_t *longest,
                                      uint32_t *present) {
    MH_CTX(c);
    HbondsBlockView B;
    if (!hbonds_block_view(c, &B))
        return fail(MOLAR_HIP_ERR_NO_SEARCH, "hbonds_frames_lifetimes: no hydrogen bonds of a block are cached (molar_hip_hbonds_frames first)");
    if (B.rows == 0 || B.nframes == 0) return fail(MOLAR_HIP_ERR_SIZES, "hbonds_frames_lifetimes: %zu rows and %zu frames", B.rows, B.nframes);
    const LtCall X{"hbonds_frames_lifetimes", B.frame_offsets, nullptr, B.bond_of_entry, B.nframes, B.rows, B.entries};
    return lt_run(c, X, group_of_row, ngroups, max_lag, origin_stride, gap, inter, cont, run_hist, events, longest, present);
}

}  // extern "C"
