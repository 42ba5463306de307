// vanhove.hip - the self part of the van Hove function over a block of trajectory frames: for every particle of an unwrapped
// trajectory, every lag of a list and every time origin the displacement |x(t + tau) - x(t)| (or one signed component),
// counted into a histogram per group of particles and lag (gmx vanhove).  The definition is in molar_hip.h.
//
//   Delta_d = x_k,d(t + tau_l) - x_k,d(t)          (double, the components of dims)
//   v       = sqrt(fma(Dz, Dz, fma(Dy, Dy, Dx Dx)))  |  Delta_d (SIGNED)
//   lo <= v < hi: hist[g][l][floor((v - lo) / (hi - lo) * nbins)] += 1, else outside[g][l] += 1
//
// Stages, all on the context's stream:
//
//   check (indices, labels and lags in device memory judged)  ->  64 bytes read back: the status
//   ->  with labels: one stable radix sort of the particles by label (devsort.hip): a group is a run of sorted positions
//   ->  gather: tiles of VH_TP particles by VH_TF frames through LDS into U [n][nd][F] (f64, particle-major, the components
//       of dims only), the non-finite values of every particle counted (one integer atomic per wave that found one)
//   ->  fold: nvalid per group (one integer atomic per run of a group inside a wave), norigins per lag
//   ->  pairs: a workgroup owns VH_PW sorted positions, one tile of lags and every nsplit-th pass of VH_PASS frames; a lane
//       owns VH_R frames of the pass as origins, holds them in registers and walks the lags of the tile: U(t) and
//       U(t + tau) are consecutive doubles across a wave.  Counts go to LDS by 32-bit integer atomics (one lag tile times
//       all bins, plus one cell per lag for `outside`), flushed with one 64-bit integer atomic per non-zero cell whenever
//       the label of the walked position changes and at the end; with more bins than VH_LDS_CELLS the atomics go to memory.
//
// Only integer atomics: the same call gives the same bits.
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "common.hpp"
#include "stages.hpp"
#include "traj_block.hpp"

using namespace mh;

struct molar_hip_vanhove_state {
    DevBuf in_traj, in_idx, in_labels, in_lags;               // host inputs staged here
    DevBuf sort_tmp;                                          // scratch of the device sort
    DevBuf ws;                                                // the workspace molar_hip_vanhove_plan reports
    DevBuf out_hist, out_outside, out_norigins;               // results on their way to host memory
};

namespace {

typedef unsigned long long u64;

constexpr uint32_t VH_WG = 256;             // lanes of a workgroup of the pair kernel
constexpr uint32_t VH_R = 4;                // origins a lane holds in registers
constexpr uint32_t VH_PASS = VH_WG * VH_R;  // frames of one pass
constexpr uint32_t VH_PW = 8;               // sorted positions a workgroup walks
constexpr uint32_t VH_MAX_TILE = 32;        // lags of one tile at the most
constexpr uint32_t VH_LDS_CELLS = 8192;     // lag tile times nbins the on-chip histogram holds: 4 bytes per cell, 32 KiB
constexpr size_t VH_TARGET_WGS = 2048;      // workgroups the pair kernel aims for when particles and tiles alone are few
constexpr uint32_t VH_TP = 32, VH_TF = 64;  // particles and frames of a tile of the gather
constexpr uint32_t VH_FLAG_WORDS = 16;      // [0]: an index not below natoms; [1]: a label not below ngroups; [2]: a lag not below F; [3]: lags not increasing
constexpr uint32_t VH_NONE = 0xFFFFFFFFu;   // a lane without a pair

// Equal cells of a wave combined ahead of the atomic: measured 7 % SLOWER on every shape of tools/bench_vanhove.py and no faster
// with lag 0 alone, where every pair of a wave meets one cell, so it is off; MOLAR_HIP_VANHOVE_COMBINE = 1
// switches it on for A/B runs.
bool combine_equal() {
    const char *e = std::getenv("MOLAR_HIP_VANHOVE_COMBINE");
    return e && e[0] == '1' && e[1] == 0;
}

// the on-chip histogram may be refused, so that both routes can be run on one input (MOLAR_HIP_VANHOVE_ONCHIP = 0; the plan
// entry and the call alike)
bool on_chip_allowed() {
    const char *e = std::getenv("MOLAR_HIP_VANHOVE_ONCHIP");
    return !(e && e[0] == '0' && e[1] == 0);
}

// Everything the kernels branch on and where everything lives in the workspace, from the sizes alone (the plan entry and the
// call share it).
struct Layout {
    uint32_t pw, lag_tile, ntiles, on_chip, nsplit;
    size_t nchunks, npasses;
    u64 pairs_per_flush;
    size_t off_flags, off_iota, off_key, off_perm, off_bad, off_nvalid, off_traj, bytes;
    bool too_large;
};

// The pairs one on-chip cell can receive between two flushes: every pair of the positions and origins a workgroup walks.
constexpr u64 flush_bound(u64 pw, u64 origins) { return pw * origins; }
static_assert(flush_bound(VH_PW, (u64)1 << 28) < ((u64)1 << 32), "VH_PW positions of 2^28 frames stay below 2^32 pairs");

Layout make_layout(size_t F, size_t n, size_t G, size_t L, size_t nbins, uint32_t nd) {
    Layout Y{};
    // VH_PW positions, fewer when their origins could reach 2^32 pairs in one cell
    Y.pw = (uint32_t)std::max<u64>(1, std::min<u64>(VH_PW, F ? 0xFFFFFFFFull / F : VH_PW));
    Y.on_chip = nbins <= VH_LDS_CELLS && on_chip_allowed() ? 1u : 0u;
    Y.lag_tile = Y.on_chip ? (uint32_t)std::min<size_t>(VH_MAX_TILE, std::max<size_t>(1, VH_LDS_CELLS / std::max<size_t>(nbins, 1))) : VH_MAX_TILE;
    Y.ntiles = (uint32_t)std::min<size_t>((L + Y.lag_tile - 1) / Y.lag_tile, 0xFFFFFFFFull);
    Y.nchunks = (n + Y.pw - 1) / Y.pw;
    Y.npasses = (F + VH_PASS - 1) / VH_PASS;
    const size_t wgs = std::max<size_t>(1, Y.nchunks * std::max<uint32_t>(Y.ntiles, 1));
    Y.nsplit = (uint32_t)std::max<size_t>(1, std::min<size_t>(Y.npasses, VH_TARGET_WGS / wgs));
    const size_t passes_per_wg = (Y.npasses + Y.nsplit - 1) / Y.nsplit;
    Y.pairs_per_flush = flush_bound(Y.pw, std::min<u64>(F, (u64)passes_per_wg * VH_PASS));
    const unsigned __int128 traj = (unsigned __int128)n * nd * F * 8;
    Y.too_large = traj >= ((unsigned __int128)1 << 62);
    Carve ws;
    ws.take(Y.off_flags, VH_FLAG_WORDS * 4);
    ws.take(Y.off_iota, n * 4);
    ws.take(Y.off_key, n * 4);
    ws.take(Y.off_perm, n * 4);
    ws.take(Y.off_bad, n * 4);
    ws.take(Y.off_nvalid, G * 8);
    ws.take(Y.off_traj, Y.too_large ? 0 : (size_t)traj);
    Y.bytes = ws.bytes;
    return Y;
}

// Grid-stride over the selection and the lags: whatever is in device memory is judged before it is used as an address.
__global__ void __launch_bounds__(256) vh_check_kernel(const uint64_t *__restrict__ idx, const uint32_t *__restrict__ labels, size_t n, size_t natoms, size_t G,
                                                       const uint64_t *__restrict__ lags, size_t L, size_t F, uint32_t *__restrict__ flags) {
    const size_t step = (size_t)gridDim.x * 256u;
    for (size_t k = (size_t)blockIdx.x * 256u + threadIdx.x; k < n; k += step) {
        if (idx && idx[k] >= natoms) flags[0] = 1u;
        if (labels && labels[k] >= G) flags[1] = 1u;
    }
    for (size_t l = (size_t)blockIdx.x * 256u + threadIdx.x; l < L; l += step) {
        if (lags[l] >= F) flags[2] = 1u;
        if (l > 0 && lags[l] <= lags[l - 1]) flags[3] = 1u;
    }
}

__global__ void __launch_bounds__(256) vh_iota_kernel(uint32_t *__restrict__ iota, size_t n) {
    const size_t k = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (k < n) iota[k] = (uint32_t)k;
}

template <class Real>
struct GatherP {
    const Real *traj;
    size_t stride, F, n;
    const uint64_t *idx;          // judged already
    const uint32_t *perm;         // sorted position -> position in the selection; null: the identity
    uint32_t dims, nd, pblocks;   // blockIdx.x = frame block * pblocks + particle block
    double *U;                    // [n][nd][F]
    uint32_t *bad;                // [n] in selection order, zeroed
};

// A tile of VH_TP sorted positions by VH_TF frames.  In: a lane owns a position and walks 8 frames; out: a wave owns a position
// and its 64 lanes the frames, so that U is written in whole lines.  A value that is not finite is counted for its particle.
template <class Real>
__global__ void __launch_bounds__(256) vh_gather_kernel(GatherP<Real> P) {
    __shared__ double tile[3][VH_TP][VH_TF + 1];
    const uint32_t fb = blockIdx.x / P.pblocks, pb = blockIdx.x - fb * P.pblocks;
    const size_t p0 = (size_t)pb * VH_TP, f0 = (size_t)fb * VH_TF;
    {
        const uint32_t pi = threadIdx.x & (VH_TP - 1u);
        const size_t pos = p0 + pi;
        if (pos < P.n) {
            const size_t k = P.perm ? P.perm[pos] : pos;
            const uint64_t a = P.idx ? P.idx[k] : (uint64_t)k;
            for (uint32_t fi = threadIdx.x / VH_TP; fi < VH_TF && f0 + fi < P.F; fi += 256u / VH_TP) {
                const Real *src = P.traj + (f0 + fi) * P.stride + 3 * a;
                uint32_t di = 0;
#pragma unroll
                for (uint32_t d = 0; d < 3; ++d)
                    if (P.dims >> d & 1u) tile[di++][pi][fi] = (double)src[d];
            }
        }
    }
    __syncthreads();
    const uint32_t fi = threadIdx.x & 63u;
    const size_t f = f0 + fi;
    const bool in = f < P.F;
    for (uint32_t pj = threadIdx.x >> 6; pj < VH_TP; pj += 4u) {
        const size_t pos = p0 + pj;
        if (pos >= P.n) break;                                  // the same for the whole wave
        bool notfinite = false;
        if (in)
            for (uint32_t di = 0; di < P.nd; ++di) {
                const double v = tile[di][pj][fi];
                P.U[(pos * P.nd + di) * P.F + f] = v;
                notfinite = notfinite || !isfinite(v);
            }
        const uint32_t cnt = (uint32_t)__popcll(__ballot(notfinite));
        if (cnt && fi == 0u) atomicAdd(&P.bad[P.perm ? P.perm[pos] : pos], cnt);
    }
}

// One thread per sorted position and per lag: the particles that enter, per group, and the origins of every lag.  The positions
// of a group are a run, so the valid lanes of every run inside a wave are counted from two ballots and the run's first lane adds
// them with ONE integer atomic (a hundred thousand particles of two species would otherwise meet at two addresses).
__global__ void __launch_bounds__(256) vh_fold_kernel(const uint32_t *__restrict__ bad, const uint32_t *__restrict__ key, const uint32_t *__restrict__ perm, size_t n,
                                                      u64 *__restrict__ nvalid, const uint64_t *__restrict__ lags, size_t L, size_t F, size_t os,
                                                      uint64_t *__restrict__ norigins) {
    const size_t pos = (size_t)blockIdx.x * 256u + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    const bool in = pos < n;
    const uint32_t g = !in ? VH_NONE : key ? key[pos] : 0u;              // the lanes behind the last position: a run of their own
    const bool valid = in && bad[perm ? perm[pos] : pos] == 0u;
    const uint32_t before = (uint32_t)__shfl_up((int)g, 1);
    const bool head = lane == 0u || g != before;
    const u64 heads = __ballot(head), valids = __ballot(valid);
    if (head && in) {
        const u64 above = lane == 63u ? 0ull : (heads >> (lane + 1u)) << (lane + 1u);
        const uint32_t end = above ? (uint32_t)__builtin_ctzll(above) : 64u;
        const u64 run = (end == 64u ? ~0ull : (1ull << end) - 1ull) & ~((1ull << lane) - 1ull);
        const uint32_t cnt = (uint32_t)__popcll(valids & run);
        if (cnt) atomicAdd(&nvalid[g], (u64)cnt);
    }
    if (norigins && pos < L) norigins[pos] = (F - 1 - lags[pos]) / os + 1;
}

struct PairQ {
    const double *U;              // [n][nd][F]
    const uint32_t *key;          // [n] the label of a sorted position; null: one group
    const uint32_t *perm;         // null: the identity
    const uint32_t *bad;          // [n] in selection order
    const uint64_t *lags;         // [L], judged
    uint32_t n, F, L, os, nbins, pw, lag_tile, ntiles, nsplit, npasses;
    double lo, hi;
    u64 *hist;                    // [G][L][nbins], zeroed; null: not wanted
    u64 *outside;                 // [G][L], zeroed; null: not wanted
};

// The DISTANCE formula of molar_hip_intcoord (ic_bin of intcoord.hip); nbins: outside.
__device__ __forceinline__ uint32_t vh_bin(double v, double lo, double hi, uint32_t nbins) {
    if (!(v >= lo && v < hi)) return nbins;
    const double fb = floor((v - lo) / (hi - lo) * (double)nbins);
    uint32_t bin = fb > 0.0 ? (uint32_t)fb : 0u;
    if (bin > nbins - 1u) bin = nbins - 1u;
    return bin;
}

// blockIdx.x = (chunk of positions * ntiles + lag tile) * nsplit + pass split.  Every loop below is uniform over the
// workgroup; a lane without a pair carries VH_NONE.  LDS: cell = lag of the tile * nbins + bin, `outside` of lag ll at
// VH_LDS_CELLS + ll.  COMBINE (off unless asked for, see combine_equal): when every pair of a wave falls into one cell - lag 0,
// short lags, a coarse grid - the leading lane adds their number; this changes no count.
template <int ND, bool SIGNED, bool LDS, bool COMBINE>
__global__ void __launch_bounds__(VH_WG) vh_pair_kernel(PairQ Q) {
    __shared__ uint32_t sh[LDS ? VH_LDS_CELLS + VH_MAX_TILE : 1];
    __shared__ uint32_t sh_lag[VH_MAX_TILE];
    const uint32_t tid = threadIdx.x;
    uint32_t b = blockIdx.x;
    const uint32_t split = b % Q.nsplit;
    b /= Q.nsplit;
    const uint32_t tile = b % Q.ntiles, chunk = b / Q.ntiles;
    const uint32_t l0 = tile * Q.lag_tile, nl = Q.L - l0 < Q.lag_tile ? Q.L - l0 : Q.lag_tile;
    const uint32_t cells = nl * Q.nbins;                         // LDS: at the most VH_LDS_CELLS by the plan
    if (tid < nl) sh_lag[tid] = (uint32_t)Q.lags[l0 + tid];
    if (LDS) {
        for (uint32_t i = tid; i < cells; i += VH_WG) sh[i] = 0u;
        if (tid < nl) sh[VH_LDS_CELLS + tid] = 0u;
    }
    __syncthreads();
    const uint32_t p0 = chunk * Q.pw, p1 = p0 + Q.pw < Q.n ? p0 + Q.pw : Q.n;
    uint32_t cur = Q.key ? Q.key[p0] : 0u;
    auto flush = [&](uint32_t g) {
        if (!LDS) return;
        __syncthreads();
        const size_t base = (size_t)g * Q.L + l0;
        for (uint32_t i = tid; i < cells; i += VH_WG) {
            const uint32_t cnt = sh[i];
            if (cnt) {
                if (Q.hist) atomicAdd(&Q.hist[base * Q.nbins + i], (u64)cnt);
                sh[i] = 0u;
            }
        }
        if (tid < nl) {
            const uint32_t cnt = sh[VH_LDS_CELLS + tid];
            if (cnt) {
                if (Q.outside) atomicAdd(&Q.outside[base + tid], (u64)cnt);
                sh[VH_LDS_CELLS + tid] = 0u;
            }
        }
        __syncthreads();
    };
    const uint32_t last = Q.F - 1u;
    for (uint32_t pos = p0; pos < p1; ++pos) {
        const uint32_t label = Q.key ? Q.key[pos] : 0u;
        if (label != cur) {
            flush(cur);
            cur = label;
        }
        if (Q.bad[Q.perm ? Q.perm[pos] : pos] != 0u) continue;
        const double *__restrict__ U = Q.U + (size_t)pos * ND * Q.F;
        const size_t gbase = (size_t)cur * Q.L + l0;
        for (uint32_t pass = split; pass < Q.npasses; pass += Q.nsplit) {
            const uint32_t t0 = pass * VH_PASS, tend = Q.F - t0 < VH_PASS ? Q.F : t0 + VH_PASS;
            if ((t0 + Q.os - 1u) / Q.os * (u64)Q.os >= tend) continue;             // a pass without an origin
            if (t0 + sh_lag[0] > last) break;                                      // no origin of this or a later pass reaches the shortest lag
            double o[VH_R][ND];
            bool ok[VH_R];
#pragma unroll
            for (uint32_t j = 0; j < VH_R; ++j) {
                const uint32_t t = t0 + j * VH_WG + tid;
                ok[j] = t < Q.F && t % Q.os == 0u;
#pragma unroll
                for (int d = 0; d < ND; ++d) o[j][d] = ok[j] ? U[(size_t)d * Q.F + t] : 0.0;
            }
            for (uint32_t ll = 0; ll < nl; ++ll) {
                const uint32_t tau = sh_lag[ll];
                if (t0 + tau > last) break;                                        // the lags increase
#pragma unroll
                for (uint32_t j = 0; j < VH_R; ++j) {
                    const uint32_t t = t0 + j * VH_WG + tid;
                    uint32_t bin = VH_NONE;
                    if (ok[j] && t + tau <= last) {
                        double v;
                        if (SIGNED) {
                            v = U[t + tau] - o[j][0];
                        } else {
                            double r2 = 0.0;
#pragma unroll
                            for (int d = 0; d < ND; ++d) {
                                const double e = U[(size_t)d * Q.F + t + tau] - o[j][d];
                                r2 = fma(e, e, r2);
                            }
                            v = sqrt(r2);
                        }
                        bin = vh_bin(v, Q.lo, Q.hi, Q.nbins);
                    }
                    if (LDS) {
                        const uint32_t cell = bin == VH_NONE ? VH_NONE : bin == Q.nbins ? VH_LDS_CELLS + ll : ll * Q.nbins + bin;
                        if (COMBINE) {
                            const u64 act = __ballot(cell != VH_NONE);
                            if (act) {
                                const uint32_t lead = (uint32_t)__builtin_ctzll(act);
                                const uint32_t first = (uint32_t)__builtin_amdgcn_readlane((int)cell, (int)lead);
                                if (__ballot(cell == first) == act) {
                                    if ((tid & 63u) == lead) atomicAdd(&sh[first], (uint32_t)__popcll(act));
                                } else if (cell != VH_NONE) {
                                    atomicAdd(&sh[cell], 1u);
                                }
                            }
                        } else if (cell != VH_NONE) {
                            atomicAdd(&sh[cell], 1u);
                        }
                    } else if (bin != VH_NONE) {
                        if (bin == Q.nbins) {
                            if (Q.outside) atomicAdd(&Q.outside[gbase + ll], (u64)1);
                        } else if (Q.hist) {
                            atomicAdd(&Q.hist[(gbase + ll) * Q.nbins + bin], (u64)1);
                        }
                    }
                }
            }
        }
    }
    flush(cur);
}

template <int ND, bool SIGNED>
void launch_pairs_nd(hipStream_t st, const PairQ &Q, uint32_t grid, bool lds, bool combine) {
    const dim3 g(grid), wg(VH_WG);
    if (!lds) hipLaunchKernelGGL((vh_pair_kernel<ND, SIGNED, false, false>), g, wg, 0, st, Q);
    else if (combine) hipLaunchKernelGGL((vh_pair_kernel<ND, SIGNED, true, true>), g, wg, 0, st, Q);
    else hipLaunchKernelGGL((vh_pair_kernel<ND, SIGNED, true, false>), g, wg, 0, st, Q);
}
void launch_pairs(hipStream_t st, const PairQ &Q, uint32_t grid, uint32_t nd, bool is_signed, bool lds, bool combine) {
    if (is_signed) launch_pairs_nd<1, true>(st, Q, grid, lds, combine);
    else if (nd == 1) launch_pairs_nd<1, false>(st, Q, grid, lds, combine);
    else if (nd == 2) launch_pairs_nd<2, false>(st, Q, grid, lds, combine);
    else launch_pairs_nd<3, false>(st, Q, grid, lds, combine);
}

int ceil_log2(size_t n) {
    int c = 0;
    while (c < 63 && ((size_t)1 << c) < n) ++c;
    return c;
}

uint32_t popcount3(uint32_t dims) { return (dims & 1u) + (dims >> 1 & 1u) + (dims >> 2 & 1u); }

// Deliver `count` values of the workspace to a destination on either side.
template <class T>
int deliver(molar_hip_ctx *c, T *dst, const T *src_dev, size_t count, bool &wait) {
    if (!dst) return 0;
    const bool dev = is_device_ptr(dst);
    MH_HIP(hipMemcpyAsync(dst, src_dev, count * sizeof(T), dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c->stream));
    if (!dev) wait = true;
    return 0;
}

template <class Real>
int vanhove_run(molar_hip_ctx *c, const char *who, const Real *traj, size_t F, size_t stride, size_t natoms, const uint64_t *idx, size_t n,
                const uint32_t *labels, size_t ngroups, const uint64_t *lags, size_t L, size_t origin_stride, uint32_t dims, uint32_t flags_arg, double lo,
                double hi, size_t nbins, uint64_t *hist, uint64_t *outside, uint64_t *norigins, uint64_t *nvalid, uint32_t *bad) {
    // the arguments are judged before the context is used
    if (!c) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "null context");
    const size_t G = labels ? ngroups : 1;
    if (n == 0) return fail(MOLAR_HIP_ERR_SIZES, "%s: no particles", who);
    if (L == 0) return fail(MOLAR_HIP_ERR_SIZES, "%s: no lags", who);
    if (G == 0) return fail(MOLAR_HIP_ERR_SIZES, "%s: labels and ngroups = 0", who);
    if (origin_stride == 0) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: origin_stride is zero", who);
    if (dims == 0 || dims > 7) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: dims = %u is not one of 1 .. 7", who, dims);
    if (flags_arg & ~(uint32_t)MOLAR_HIP_VANHOVE_SIGNED) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: flags = %u holds an unknown bit", who, flags_arg);
    const bool is_signed = (flags_arg & MOLAR_HIP_VANHOVE_SIGNED) != 0;
    const uint32_t nd = popcount3(dims);
    if (is_signed && nd != 1) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: SIGNED with dims = %u, which is more than one component", who, dims);
    if (!std::isfinite(lo) || !std::isfinite(hi)) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: the range is not finite", who);
    if (!(lo < hi)) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: lo = %g is not below hi = %g", who, lo, hi);
    if (nbins == 0) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: nbins = 0", who);
    if (G >= 0x80000000ull || L >= 0x80000000ull || nbins >= 0x80000000ull || (unsigned __int128)G * L * nbins >= 0x80000000ull)
        return fail(MOLAR_HIP_ERR_TOO_LARGE, "%s: 2^31 histogram cells (groups times lags times nbins) or more", who);
    if (!lags) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: the lags pointer is null", who);
    if (natoms == 0) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: %zu particles out of natoms = 0", who, n);
    MH_TRY(check_no_index(who, "n", idx, n, natoms));
    MH_TRY(check_stride(who, "the frame stride", F, stride, natoms));
    if (n >= 0x7FFFFF00ull || F >= 0x7FFFFF00ull) return fail(MOLAR_HIP_ERR_TOO_LARGE, "%s: 2^31 particles or frames", who);
    if (F == 0) return MOLAR_HIP_OK;
    if (!traj) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: the trajectory pointer is null", who);
    // what is in host memory is walked here; what is in device memory is judged by the check kernel before one is used as an address
    MH_TRY(check_index(who, "idx", idx, n, natoms));
    if (labels && !is_device_ptr(labels))
        for (size_t k = 0; k < n; ++k)
            if (labels[k] >= G) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: labels[%zu] = %u is not below ngroups = %zu", who, k, labels[k], G);
    if (!is_device_ptr(lags))
        for (size_t l = 0; l < L; ++l) {
            if (lags[l] >= F) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: lags[%zu] = %llu is not below nframes = %zu", who, l, (u64)lags[l], F);
            if (l > 0 && lags[l] <= lags[l - 1]) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: lags[%zu] = %llu does not exceed lags[%zu]", who, l, (u64)lags[l], l - 1);
        }
    const Layout Y = make_layout(F, n, G, L, nbins, nd);
    if (Y.too_large) return fail(MOLAR_HIP_ERR_TOO_LARGE, "%s: the particle trajectories exceed 2^62 bytes", who);
    if (Y.pairs_per_flush >= ((u64)1 << 32)) return fail(MOLAR_HIP_ERR_TOO_LARGE, "%s: %llu pairs between two flushes", who, Y.pairs_per_flush);
    const size_t pblocks = (n + VH_TP - 1) / VH_TP, fblocks = (F + VH_TF - 1) / VH_TF;
    const size_t pair_grid = Y.nchunks * Y.ntiles * Y.nsplit;
    if (pblocks * fblocks >= 0x7FFFFFFFull || pair_grid >= 0x7FFFFFFFull) return fail(MOLAR_HIP_ERR_TOO_LARGE, "%s: more than 2^31 workgroups", who);
    MH_HIP(hipSetDevice(c->device));

    molar_hip_vanhove_state &Z = state_of(c->vanhove);
    MH_TRY(grow_exact(Z.ws, Y.bytes, who, "the workspace"));
    char *W = Z.ws.as<char>();
    uint32_t *flags = reinterpret_cast<uint32_t *>(W + Y.off_flags), *iota = reinterpret_cast<uint32_t *>(W + Y.off_iota);
    uint32_t *key = reinterpret_cast<uint32_t *>(W + Y.off_key), *perm = reinterpret_cast<uint32_t *>(W + Y.off_perm);
    uint32_t *bad_d = reinterpret_cast<uint32_t *>(W + Y.off_bad);
    u64 *nvalid_d = reinterpret_cast<u64 *>(W + Y.off_nvalid);
    double *U = reinterpret_cast<double *>(W + Y.off_traj);

    const size_t cells = G * L * nbins;
    uint64_t *hist_d, *outside_d, *norigins_d;
    MH_TRY(out_buffer(hist, cells, Z.out_hist, who, &hist_d));
    MH_TRY(out_buffer(outside, G * L, Z.out_outside, who, &outside_d));
    MH_TRY(out_buffer(norigins, L, Z.out_norigins, who, &norigins_d));

    const Real *traj_dev = nullptr;
    const uint64_t *idx_dev = nullptr, *lags_dev = nullptr;
    const uint32_t *labels_dev = nullptr;
    MH_TRY(to_device(c, traj, (F - 1) * stride + natoms * 3, Z.in_traj, &traj_dev));
    MH_TRY(to_device(c, idx, idx ? n : 0, Z.in_idx, &idx_dev));
    MH_TRY(to_device(c, labels, labels ? n : 0, Z.in_labels, &labels_dev));
    MH_TRY(to_device(c, lags, L, Z.in_lags, &lags_dev));

    MH_HIP(hipMemsetAsync(flags, 0, VH_FLAG_WORDS * 4, c->stream));
    const size_t most = std::max(n, L);
    hipLaunchKernelGGL(vh_check_kernel, dim3((uint32_t)std::min<size_t>((most + 255) / 256, 1024)), dim3(256), 0, c->stream, idx_dev, labels_dev, n, natoms, G, lags_dev,
                       L, F, flags);
    MH_HIP(hipGetLastError());
    // the one read-back: the status.  Nothing below runs, no label, lag or index is used as an address and no output is touched
    // after a bad argument.
    uint32_t hf[VH_FLAG_WORDS];
    MH_TRY(read_back(c, hf, flags, sizeof hf));
    if (hf[0]) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: an index is not below natoms = %zu", who, natoms);
    if (hf[1]) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: a label is not below ngroups = %zu", who, G);
    if (hf[2]) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: a lag is not below nframes = %zu", who, F);
    if (hf[3]) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: the lags are not strictly increasing", who);

    MH_HIP(hipMemsetAsync(bad_d, 0, n * 4, c->stream));
    MH_HIP(hipMemsetAsync(nvalid_d, 0, G * 8, c->stream));
    if (labels_dev) {
        hipLaunchKernelGGL(vh_iota_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, c->stream, iota, n);
        MH_TRY(device_sort_pairs_u32(c->stream, Z.sort_tmp, labels_dev, key, iota, perm, n, std::max(1, ceil_log2(G))));
    }
    GatherP<Real> P{};
    P.traj = traj_dev;
    P.stride = stride;
    P.F = F;
    P.n = n;
    P.idx = idx_dev;
    P.perm = labels_dev ? perm : nullptr;
    P.dims = dims;
    P.nd = nd;
    P.pblocks = (uint32_t)pblocks;
    P.U = U;
    P.bad = bad_d;
    hipLaunchKernelGGL(vh_gather_kernel<Real>, dim3((uint32_t)(pblocks * fblocks)), dim3(256), 0, c->stream, P);
    const size_t os = std::min(origin_stride, F);               // beyond F - 1 there is the origin 0 alone either way
    hipLaunchKernelGGL(vh_fold_kernel, dim3((uint32_t)((most + 255) / 256)), dim3(256), 0, c->stream, bad_d, labels_dev ? key : nullptr, P.perm, n, nvalid_d, lags_dev, L, F,
                       os, norigins_d);
    if (hist_d || outside_d) {
        if (hist_d) MH_HIP(hipMemsetAsync(hist_d, 0, cells * 8, c->stream));
        if (outside_d) MH_HIP(hipMemsetAsync(outside_d, 0, G * L * 8, c->stream));
        PairQ Q{};
        Q.U = U;
        Q.key = labels_dev ? key : nullptr;
        Q.perm = P.perm;
        Q.bad = bad_d;
        Q.lags = lags_dev;
        Q.n = (uint32_t)n;
        Q.F = (uint32_t)F;
        Q.L = (uint32_t)L;
        Q.os = (uint32_t)os;
        Q.nbins = (uint32_t)nbins;
        Q.pw = Y.pw;
        Q.lag_tile = Y.lag_tile;
        Q.ntiles = Y.ntiles;
        Q.nsplit = Y.nsplit;
        Q.npasses = (uint32_t)Y.npasses;
        Q.lo = lo;
        Q.hi = hi;
        Q.hist = reinterpret_cast<u64 *>(hist_d);
        Q.outside = reinterpret_cast<u64 *>(outside_d);
        launch_pairs(c->stream, Q, (uint32_t)pair_grid, nd, is_signed, Y.on_chip != 0, combine_equal());
    }
    MH_HIP(hipGetLastError());
    bool wait = false;
    MH_TRY(copy_out(c, hist, hist_d, cells, wait));
    MH_TRY(copy_out(c, outside, outside_d, G * L, wait));
    MH_TRY(copy_out(c, norigins, norigins_d, L, wait));
    MH_TRY(deliver(c, nvalid, reinterpret_cast<const uint64_t *>(nvalid_d), G, wait));
    MH_TRY(deliver(c, bad, (const uint32_t *)bad_d, n, wait));
    return finish_copies(c, wait);
}

}  // namespace

namespace mh {
void vanhove_release(molar_hip_ctx *c) {
    release_state(c->vanhove);
}
}  // namespace mh

extern "C" {

int molar_hip_vanhove_plan(size_t nframes, size_t n, size_t ngroups, size_t nlags, size_t nbins, uint32_t ndims, size_t *workspace_bytes,
                           uint32_t *particles_per_wg, uint32_t *origins_per_pass, uint32_t *lag_tile, uint32_t *on_chip, uint32_t *lds_cells,
                           uint32_t *pass_splits, uint64_t *pairs_per_flush) {
    if (ndims < 1 || ndims > 3) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "vanhove_plan: ndims = %u is not 1, 2 or 3", ndims);
    if (nframes >= 0x7FFFFF00ull || n >= 0x7FFFFF00ull) return fail(MOLAR_HIP_ERR_TOO_LARGE, "vanhove_plan: 2^31 particles or frames");
    const Layout Y = make_layout(nframes, n, ngroups ? ngroups : 1, nlags, nbins, ndims);
    if (Y.too_large) return fail(MOLAR_HIP_ERR_TOO_LARGE, "vanhove_plan: the particle trajectories exceed 2^62 bytes");
    const bool none = nframes == 0 || n == 0;
    if (workspace_bytes) *workspace_bytes = none ? 0 : Y.bytes;
    if (particles_per_wg) *particles_per_wg = Y.pw;
    if (origins_per_pass) *origins_per_pass = VH_PASS;
    if (lag_tile) *lag_tile = Y.lag_tile;
    if (on_chip) *on_chip = Y.on_chip;
    if (lds_cells) *lds_cells = VH_LDS_CELLS;
    if (pass_splits) *pass_splits = Y.nsplit;
    if (pairs_per_flush) *pairs_per_flush = Y.pairs_per_flush;
    return MOLAR_HIP_OK;
}

int molar_hip_vanhove(molar_hip_ctx *c, const float *traj, size_t nframes, size_t frame_stride, size_t natoms, const uint64_t *idx, size_t n,
                      const uint32_t *labels, size_t ngroups, const uint64_t *lags, size_t nlags, size_t origin_stride, uint32_t dims, uint32_t flags, double lo,
                      double hi, size_t nbins, uint64_t *hist, uint64_t *outside, uint64_t *norigins, uint64_t *nvalid, uint32_t *bad) {
    return vanhove_run<float>(c, "vanhove", traj, nframes, frame_stride, natoms, idx, n, labels, ngroups, lags, nlags, origin_stride, dims, flags, lo, hi, nbins, hist,
                              outside, norigins, nvalid, bad);
}

int molar_hip_vanhove_f64(molar_hip_ctx *c, const double *traj, size_t nframes, size_t frame_stride, size_t natoms, const uint64_t *idx, size_t n,
                          const uint32_t *labels, size_t ngroups, const uint64_t *lags, size_t nlags, size_t origin_stride, uint32_t dims, uint32_t flags,
                          double lo, double hi, size_t nbins, uint64_t *hist, uint64_t *outside, uint64_t *norigins, uint64_t *nvalid, uint32_t *bad) {
    return vanhove_run<double>(c, "vanhove_f64", traj, nframes, frame_stride, natoms, idx, n, labels, ngroups, lags, nlags, origin_stride, dims, flags, lo, hi, nbins,
                               hist, outside, norigins, nvalid, bad);
}

}  // extern "C"
