// intcoord.hip - internal coordinates of a block of trajectory frames: the distance, the angle or the dihedral of every tuple
// of atoms in every frame, as a series, as histograms per group of tuples, as joint histograms of pairs of tuples (the
// Ramachandran map) and as a mean and a spread per tuple.  The definition is in molar_hip.h.
//
//   DISTANCE (A,B):     |B - A|
//   ANGLE (A,B,C):      u = A - B, v = C - B;  atan2(|u x v|, u . v)
//   DIHEDRAL (A,B,C,D): b1 = B - A, b2 = C - B, b3 = D - C, n1 = b1 x b2, n2 = b2 x b3;  atan2(|b2| (b1 . n2), n1 . n2)
//   every bond vector on its own through shortest_vector (boxmath.hpp) when pbc != 0; all of it in double.
//
// Stages, all on the context's stream:
//
//   boxes (one thread per box: the f64 PeriodicBox)  ->  prep: tuples, labels, pairs and pair labels in device memory judged
//   ->  64 bytes read back: the status
//   ->  series (a workgroup takes IC_TUPLES tuples and IC_FRAMES frames, a lane owns a tuple and walks its frames in order: the
//       value stored, binned with integer atomics into LDS when G * nbins cells fit and flushed once, else with integer
//       atomics into memory; the lane's partial sums and count of the chunk into the workspace [frame chunks][T])
//   ->  fold (one lane per tuple: the chunks in chunk order, then the mean and the spread)
//   ->  map (a lane owns a pair of tuples and recomputes its two values; the same two routes).
//
// Only integer atomics, and the f64 sums in a fixed order: the same call gives the same bits.
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "boxmath.hpp"
#include "common.hpp"
#include "traj_block.hpp"

using namespace mh;

struct molar_hip_intcoord_state {
    DevBuf in_frames, in_tuples, in_labels, in_boxes, in_pairs, in_plabels;   // host inputs staged here
    DevBuf boxes;                                                             // the f64 PeriodicBox of every box of the call
    DevBuf out_values, out_hist, out_map, out_mean, out_spread, out_valid;    // results on their way to host memory
    DevBuf ws;                                                                // the workspace molar_hip_intcoord_plan reports
};

namespace {

typedef unsigned long long u64;

constexpr uint32_t IC_WG = 256;                // threads of every workgroup here
constexpr uint32_t IC_TUPLES = 256;            // tuples (or pairs) per workgroup: one per lane
constexpr uint32_t IC_FRAMES = 64;             // frames per workgroup, walked in order by every lane
constexpr uint32_t IC_LDS_CELLS = 8192;        // G * nbins (G2 * map_bins^2) the on-chip route takes: 4 bytes per cell, 32 KiB
constexpr double IC_PI = 3.14159265358979323846;

// flags[0]: a tuple index not below natoms; [1]: a box matrix without an inverse; [3]: a box vector of zero length;
// [5]: a label not below ngroups; [6]: a pair entry not below ntuples; [7]: a pair label not below npair_groups
constexpr uint32_t IC_FLAG_WORDS = 16;

struct Layout {
    size_t chunks;                         // chunks of IC_FRAMES frames
    size_t off_flags, off_sum, off_n, bytes;
};

Layout make_layout(size_t F, size_t T, bool want_stats) {
    Layout Y{};
    Y.chunks = (F + IC_FRAMES - 1) / IC_FRAMES;
    Carve ws;
    ws.take(Y.off_flags, IC_FLAG_WORDS * 4);
    ws.take(Y.off_sum, want_stats ? Y.chunks * T * 16 : 0);
    ws.take(Y.off_n, want_stats ? Y.chunks * T * 4 : 0);
    Y.bytes = ws.bytes;
    return Y;
}

// One thread per box.
template <class Real>
__global__ void __launch_bounds__(64) ic_box_kernel(const Real *__restrict__ boxes, size_t nbox, BoxD *__restrict__ out, uint32_t *__restrict__ flags) {
    const size_t f = (size_t)blockIdx.x * 64u + threadIdx.x;
    if (f >= nbox) return;
    double m9[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) m9[q] = (double)boxes[f * 9 + q];
    const int bad = box_from_matrix_device(m9, out + f);
    if (bad == 1) flags[3] = 1u;
    if (bad == 2) flags[1] = 1u;
}

// What the host has not walked (a null pointer here: nothing to judge), grid-stride.
struct Prep {
    const uint64_t *tuples;
    size_t ntuple_entries, natoms;
    const uint32_t *labels;
    size_t T, G;
    const uint64_t *pairs;
    size_t npair_entries;
    const uint32_t *plabels;
    size_t P, G2;
};

__global__ void __launch_bounds__(IC_WG) ic_prep_kernel(Prep P, uint32_t *__restrict__ flags) {
    const size_t step = (size_t)gridDim.x * IC_WG, t0 = (size_t)blockIdx.x * IC_WG + threadIdx.x;
    if (P.tuples)
        for (size_t k = t0; k < P.ntuple_entries; k += step)
            if (P.tuples[k] >= P.natoms) flags[0] = 1u;
    if (P.labels)
        for (size_t k = t0; k < P.T; k += step)
            if (P.labels[k] >= P.G) flags[5] = 1u;
    if (P.pairs)
        for (size_t k = t0; k < P.npair_entries; k += step)
            if (P.pairs[k] >= P.T) flags[6] = 1u;
    if (P.plabels)
        for (size_t k = t0; k < P.P; k += step)
            if (P.plabels[k] >= P.G2) flags[7] = 1u;
}

__device__ __forceinline__ D3 cross3(D3 a, D3 b) { return D3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ double dot3(D3 a, D3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }

template <class Real>
struct Block {
    const Real *frames;
    size_t stride, F;
    const BoxD *boxes;            // null: no image is removed
    uint32_t box_step, pbc;
};

template <class Real>
__device__ __forceinline__ D3 ic_atom(const Real *p, uint64_t a, bool &fin) {
    const D3 x{(double)p[3 * a], (double)p[3 * a + 1], (double)p[3 * a + 2]};
    fin = fin && isfinite(x.x) && isfinite(x.y) && isfinite(x.z);
    return x;
}

// The value of tuple a[0 .. KIND) in the frame at p; false: invalid (a coordinate that is not finite, a degenerate
// configuration, or a result that is not finite under a box that is not).
template <int KIND, class Real>
__device__ __forceinline__ bool ic_value(const Real *p, const uint64_t *a, const BoxD *box, uint32_t pbc, double &val) {
    bool fin = true;
    D3 x[KIND];
#pragma unroll
    for (int j = 0; j < KIND; ++j) x[j] = ic_atom(p, a[j], fin);
    D3 b[KIND - 1];
#pragma unroll
    for (int j = 0; j + 1 < KIND; ++j) {
        // ANGLE: u = A - B, v = C - B; the others: the bonds in order
        b[j] = (KIND == 3 && j == 0) ? x[0] - x[1] : x[j + 1] - x[j];
        if (box) b[j] = shortest_vector(*box, b[j], pbc);
    }
    bool ok = fin;
    if constexpr (KIND == 2) {
        val = sqrt(norm2(b[0]));
    } else if constexpr (KIND == 3) {
        const D3 c = cross3(b[0], b[1]);
        if (norm2(b[0]) == 0.0 || norm2(b[1]) == 0.0) ok = false;
        val = atan2(sqrt(norm2(c)), dot3(b[0], b[1]));
    } else {
        const D3 n1 = cross3(b[0], b[1]), n2 = cross3(b[1], b[2]);
        if ((n1.x == 0.0 && n1.y == 0.0 && n1.z == 0.0) || (n2.x == 0.0 && n2.y == 0.0 && n2.z == 0.0)) ok = false;
        val = atan2(sqrt(norm2(b[1])) * dot3(b[0], n2), dot3(n1, n2));
    }
    return ok && isfinite(val);
}

// The bin of a valid value, -1: outside the range of a DISTANCE histogram.
template <int KIND>
__device__ __forceinline__ int32_t ic_bin(double v, double lo, double hi, uint32_t nbins) {
    double fb;
    if (KIND == 2) {
        if (!(v >= lo && v < hi)) return -1;
        fb = floor((v - lo) / (hi - lo) * (double)nbins);
    } else if (KIND == 3) {
        fb = floor(v / IC_PI * (double)nbins);
    } else {
        fb = floor((v + IC_PI) / (2.0 * IC_PI) * (double)nbins);
    }
    uint32_t bin = fb > 0.0 ? (uint32_t)fb : 0u;
    if (KIND == 4) {
        if (bin >= nbins) bin -= nbins;          // phi = pi: bin nbins mod nbins
    }
    if (bin > nbins - 1u) bin = nbins - 1u;       // theta = pi, or a product that rounds up to nbins
    return (int32_t)bin;
}

template <class Real>
struct Series {
    Block<Real> X;
    const uint64_t *tuples;
    size_t T;
    const uint32_t *labels;
    uint32_t nbins, cells;        // cells = G * nbins
    double lo, hi;
    uint32_t tblocks;             // workgroups along the tuples; blockIdx.x = chunk * tblocks + tuple block
    Real *values;                 // null: not wanted
    size_t ld;
    u64 *hist;                    // null: not wanted
    double *sum;                  // [chunks][T][2]; null: no statistics
    uint32_t *n;                  // [chunks][T]
};

template <class Real, int KIND, bool LDS>
__global__ void __launch_bounds__(IC_WG) ic_series_kernel(Series<Real> S) {
    __shared__ uint32_t sh[LDS ? IC_LDS_CELLS : 1];
    const uint32_t chunk = blockIdx.x / S.tblocks, tb = blockIdx.x - chunk * S.tblocks;
    if (LDS) {
        for (uint32_t i = threadIdx.x; i < S.cells; i += IC_WG) sh[i] = 0u;
        __syncthreads();
    }
    const size_t t = (size_t)tb * IC_TUPLES + threadIdx.x;
    const size_t f0 = (size_t)chunk * IC_FRAMES, f1 = f0 + IC_FRAMES < S.X.F ? f0 + IC_FRAMES : S.X.F;
    if (t < S.T) {
        uint64_t a[KIND];
#pragma unroll
        for (int j = 0; j < KIND; ++j) a[j] = S.tuples[t * KIND + j];
        const uint32_t base = (S.hist && S.labels ? S.labels[t] : 0u) * S.nbins;
        double s1 = 0.0, s2 = 0.0;
        uint32_t n = 0;
        for (size_t f = f0; f < f1; ++f) {
            const BoxD *box = S.X.boxes ? S.X.boxes + f * S.X.box_step : nullptr;
            double v;
            const bool ok = ic_value<KIND>(S.X.frames + f * S.X.stride, a, box, S.X.pbc, v);
            if (S.values) S.values[f * S.ld + t] = ok ? (Real)v : (Real)__builtin_nan("");
            if (!ok) continue;
            ++n;
            if (S.sum) {
                if (KIND == 4) {
                    double sn, cs;
                    sincos(v, &sn, &cs);
                    s1 += cs;
                    s2 += sn;
                } else {
                    s1 += v;
                    s2 += v * v;
                }
            }
            if (S.hist) {
                const int32_t bin = ic_bin<KIND>(v, S.lo, S.hi, S.nbins);
                if (bin >= 0) {
                    if (LDS) atomicAdd(&sh[base + (uint32_t)bin], 1u);
                    else atomicAdd(&S.hist[base + (uint32_t)bin], (u64)1);
                }
            }
        }
        if (S.sum) {
            const size_t o = (size_t)chunk * S.T + t;
            S.sum[2 * o] = s1;
            S.sum[2 * o + 1] = s2;
            S.n[o] = n;
        }
    }
    if (LDS) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < S.cells; i += IC_WG)
            if (sh[i]) atomicAdd(&S.hist[i], (u64)sh[i]);
    }
}

// One lane per tuple: the chunks in chunk order.  DISTANCE, ANGLE: mean = S1 / n, spread = sqrt(max(0, S2 / n - mean^2));
// DIHEDRAL: mean = atan2(S, C), spread = 1 - hypot(C, S) / n; n = 0: NaN.
template <class Real>
__global__ void __launch_bounds__(IC_WG) ic_fold_kernel(const double *__restrict__ sum, const uint32_t *__restrict__ cnt, size_t chunks, size_t T, uint32_t kind,
                                                        Real *__restrict__ mean, Real *__restrict__ spread, u64 *__restrict__ valid) {
    const size_t t = (size_t)blockIdx.x * IC_WG + threadIdx.x;
    if (t >= T) return;
    double s1 = 0.0, s2 = 0.0;
    u64 n = 0;
    for (size_t c = 0; c < chunks; ++c) {
        const size_t o = c * T + t;
        s1 += sum[2 * o];
        s2 += sum[2 * o + 1];
        n += cnt[o];
    }
    double m = __builtin_nan(""), s = __builtin_nan("");
    if (n) {
        const double dn = (double)n;
        if (kind == MOLAR_HIP_IC_DIHEDRAL) {
            m = atan2(s2, s1);
            s = 1.0 - hypot(s1, s2) / dn;
        } else {
            m = s1 / dn;
            s = sqrt(fmax(0.0, s2 / dn - m * m));
        }
    }
    if (mean) mean[t] = (Real)m;
    if (spread) spread[t] = (Real)s;
    if (valid) valid[t] = n;
}

template <class Real>
struct Map {
    Block<Real> X;
    const uint64_t *tuples, *pairs;
    size_t P;
    const uint32_t *plabels;
    uint32_t mb, cells;           // bins per side; cells = G2 * mb * mb
    double lo, hi;
    uint32_t pblocks;
    u64 *map;
};

template <class Real, int KIND, bool LDS>
__global__ void __launch_bounds__(IC_WG) ic_map_kernel(Map<Real> M) {
    __shared__ uint32_t sh[LDS ? IC_LDS_CELLS : 1];
    const uint32_t chunk = blockIdx.x / M.pblocks, pb = blockIdx.x - chunk * M.pblocks;
    if (LDS) {
        for (uint32_t i = threadIdx.x; i < M.cells; i += IC_WG) sh[i] = 0u;
        __syncthreads();
    }
    const size_t p = (size_t)pb * IC_TUPLES + threadIdx.x;
    const size_t f0 = (size_t)chunk * IC_FRAMES, f1 = f0 + IC_FRAMES < M.X.F ? f0 + IC_FRAMES : M.X.F;
    if (p < M.P) {
        const uint64_t t0 = M.pairs[2 * p], t1 = M.pairs[2 * p + 1];
        uint64_t a0[KIND], a1[KIND];
#pragma unroll
        for (int j = 0; j < KIND; ++j) {
            a0[j] = M.tuples[t0 * KIND + j];
            a1[j] = M.tuples[t1 * KIND + j];
        }
        const uint32_t base = (M.plabels ? M.plabels[p] : 0u) * M.mb * M.mb;
        for (size_t f = f0; f < f1; ++f) {
            const BoxD *box = M.X.boxes ? M.X.boxes + f * M.X.box_step : nullptr;
            const Real *x = M.X.frames + f * M.X.stride;
            double v0, v1;
            if (!ic_value<KIND>(x, a0, box, M.X.pbc, v0)) continue;
            if (!ic_value<KIND>(x, a1, box, M.X.pbc, v1)) continue;
            const int32_t b0 = ic_bin<KIND>(v0, M.lo, M.hi, M.mb), b1 = ic_bin<KIND>(v1, M.lo, M.hi, M.mb);
            if (b0 < 0 || b1 < 0) continue;
            const uint32_t cell = base + (uint32_t)b0 * M.mb + (uint32_t)b1;
            if (LDS) atomicAdd(&sh[cell], 1u);
            else atomicAdd(&M.map[cell], (u64)1);
        }
    }
    if (LDS) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < M.cells; i += IC_WG)
            if (sh[i]) atomicAdd(&M.map[i], (u64)sh[i]);
    }
}

template <class Real, int KIND>
void launch_series(const Series<Real> &S, bool lds, uint32_t grid, hipStream_t stream) {
    if (lds) hipLaunchKernelGGL((ic_series_kernel<Real, KIND, true>), dim3(grid), dim3(IC_WG), 0, stream, S);
    else hipLaunchKernelGGL((ic_series_kernel<Real, KIND, false>), dim3(grid), dim3(IC_WG), 0, stream, S);
}
template <class Real, int KIND>
void launch_map(const Map<Real> &M, bool lds, uint32_t grid, hipStream_t stream) {
    if (lds) hipLaunchKernelGGL((ic_map_kernel<Real, KIND, true>), dim3(grid), dim3(IC_WG), 0, stream, M);
    else hipLaunchKernelGGL((ic_map_kernel<Real, KIND, false>), dim3(grid), dim3(IC_WG), 0, stream, M);
}

// the spec and the groups alone
int check_spec(const char *who, const molar_hip_intcoord_spec *spec, size_t G, size_t G2) {
    if (!spec) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: the spec is null", who);
    if (spec->kind != MOLAR_HIP_IC_DISTANCE && spec->kind != MOLAR_HIP_IC_ANGLE && spec->kind != MOLAR_HIP_IC_DIHEDRAL)
        return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: kind = %u is not DISTANCE (2), ANGLE (3) or DIHEDRAL (4)", who, spec->kind);
    if (spec->reserved != 0) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: the reserved field of the spec is not zero", who);
    if (spec->kind == MOLAR_HIP_IC_DISTANCE) {
        if (!(std::isfinite(spec->lo) && std::isfinite(spec->hi))) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: the range is not finite", who);
        if (!(spec->lo < spec->hi)) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: lo = %g is not below hi = %g", who, spec->lo, spec->hi);
    }
    if (G >= 0x80000000ull || (unsigned __int128)G * spec->nbins >= 0x80000000ull)
        return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: 2^31 histogram cells (groups times nbins) or more", who);
    if (G2 >= 0x80000000ull || (unsigned __int128)G2 * spec->map_bins * spec->map_bins >= 0x80000000ull)
        return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: 2^31 map cells (pair groups times map_bins squared) or more", who);
    return 0;
}

template <class T>
int walk_below(const char *who, const char *name, const T *v, size_t count, size_t bound, const char *bound_name) {
    if (v && !is_device_ptr(v))
        for (size_t k = 0; k < count; ++k)
            if (v[k] >= bound)
                return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: %s[%zu] = %llu is not below %s = %zu", who, name, k, (unsigned long long)v[k], bound_name, bound);
    return 0;
}

template <class Real>
int intcoord_run(molar_hip_ctx *c, const char *who, const Real *frames, size_t F, size_t stride, size_t natoms, const uint64_t *tuples, size_t T,
                 const uint32_t *labels, size_t ngroups, const Real *boxes, size_t box_stride, uint8_t pbc, const molar_hip_intcoord_spec *spec,
                 const uint64_t *pairs, size_t npairs, const uint32_t *pair_labels, size_t npair_groups, Real *values, size_t ld, uint64_t *hist,
                 uint64_t *map, Real *mean, Real *spread, uint64_t *valid) {
    // the arguments are judged before the context is used
    if (!c) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "null context");
    const size_t G = labels ? ngroups : 1, G2 = pair_labels ? npair_groups : 1;
    if (G == 0) return fail(MOLAR_HIP_ERR_SIZES, "%s: labels and ngroups = 0", who);
    if (G2 == 0) return fail(MOLAR_HIP_ERR_SIZES, "%s: pair_labels and npair_groups = 0", who);
    MH_TRY(check_spec(who, spec, G, G2));
    const uint32_t kind = spec->kind;
    if (pbc > 7) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: pbc = %u is not a PbcDims byte", who, (unsigned)pbc);
    if (box_stride != 0 && box_stride != 9) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: box_stride = %zu is neither 0 nor 9", who, box_stride);
    if (hist && spec->nbins == 0) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: a histogram with nbins = 0", who);
    if (map && spec->map_bins == 0) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: a map with map_bins = 0", who);
    if (map && !pairs) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: a map without pairs", who);
    if (values && ld < T) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: ld = %zu is below ntuples = %zu", who, ld, T);
    if (T != 0 && !tuples) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: the tuples pointer is null", who);
    if (T != 0 && natoms == 0) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: %zu tuples out of natoms = 0", who, T);
    MH_TRY(check_stride(who, "the frame stride", F, stride, natoms));
    if (pbc != 0 && !boxes) return fail(MOLAR_HIP_ERR_NO_PBC, "%s: pbc operation without periodic box", who);
    const size_t chunks = (F + IC_FRAMES - 1) / IC_FRAMES, tblocks = (T + IC_TUPLES - 1) / IC_TUPLES, pblocks = (npairs + IC_TUPLES - 1) / IC_TUPLES;
    if (T >= 0x7FFFFF00ull || npairs >= 0x7FFFFF00ull || F >= 0x7FFFFFF0ull || chunks * tblocks >= 0x7FFFFFFFull || chunks * pblocks >= 0x7FFFFFFFull)
        return fail(MOLAR_HIP_ERR_TOO_LARGE, "%s: more than 2^31 tuples, pairs, frames or workgroups", who);
    if (F == 0 || T == 0) return MOLAR_HIP_OK;
    if (!frames) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: the frames pointer is null", who);
    const bool want_map = map != nullptr, want_stats = mean || spread || valid;
    // tuples, labels and pairs in host memory are walked here; those in device memory are judged by the prep kernel before one
    // is used as an address
    MH_TRY(check_index(who, "tuples", tuples, T * kind, natoms));
    MH_TRY(walk_below(who, "labels", labels, T, G, "ngroups"));
    if (want_map) {
        MH_TRY(walk_below(who, "pairs", pairs, npairs * 2, T, "ntuples"));
        MH_TRY(walk_below(who, "pair_labels", pair_labels, npairs, G2, "npair_groups"));
    }
    MH_HIP(hipSetDevice(c->device));

    const Layout Y = make_layout(F, T, want_stats);
    molar_hip_intcoord_state &Z = state_of(c->intcoord);
    MH_TRY(grow_exact(Z.ws, Y.bytes, who, "the workspace"));
    char *W = Z.ws.as<char>();
    uint32_t *flags = reinterpret_cast<uint32_t *>(W + Y.off_flags);
    double *sum_d = reinterpret_cast<double *>(W + Y.off_sum);
    uint32_t *n_d = reinterpret_cast<uint32_t *>(W + Y.off_n);
    const size_t hcells = G * spec->nbins, mcells = G2 * spec->map_bins * spec->map_bins;
    Real *values_d = nullptr, *mean_d = nullptr, *spread_d = nullptr;
    u64 *hist_d = nullptr, *map_d = nullptr, *valid_d = nullptr;
    u64 *hist_u = reinterpret_cast<u64 *>(hist), *map_u = reinterpret_cast<u64 *>(map), *valid_u = reinterpret_cast<u64 *>(valid);
    MH_TRY(out_buffer(values, F * T, Z.out_values, who, &values_d));
    MH_TRY(out_buffer(hist_u, hcells, Z.out_hist, who, &hist_d));
    MH_TRY(out_buffer(map_u, mcells, Z.out_map, who, &map_d));
    MH_TRY(out_buffer(mean, T, Z.out_mean, who, &mean_d));
    MH_TRY(out_buffer(spread, T, Z.out_spread, who, &spread_d));
    MH_TRY(out_buffer(valid_u, T, Z.out_valid, who, &valid_d));
    const bool use_box = pbc != 0;
    const size_t nbox = use_box ? (box_stride ? F : 1) : 0;
    if (use_box) MH_TRY(grow_exact(Z.boxes, nbox * sizeof(BoxD), who, "the boxes"));

    Block<Real> X{};
    X.stride = stride;
    X.F = F;
    X.boxes = use_box ? Z.boxes.as<BoxD>() : nullptr;
    X.box_step = box_stride ? 1u : 0u;
    X.pbc = pbc;
    const uint64_t *tuples_d = nullptr, *pairs_d = nullptr;
    const uint32_t *labels_d = nullptr, *plabels_d = nullptr;
    const Real *boxes_d = nullptr;
    MH_TRY(to_device(c, frames, (F - 1) * stride + natoms * 3, Z.in_frames, &X.frames));
    MH_TRY(to_device(c, tuples, T * kind, Z.in_tuples, &tuples_d));
    MH_TRY(to_device(c, labels, labels ? T : 0, Z.in_labels, &labels_d));
    MH_TRY(to_device(c, use_box ? boxes : nullptr, nbox * 9, Z.in_boxes, &boxes_d));
    MH_TRY(to_device(c, want_map ? pairs : nullptr, npairs * 2, Z.in_pairs, &pairs_d));
    MH_TRY(to_device(c, want_map ? pair_labels : nullptr, npairs, Z.in_plabels, &plabels_d));

    MH_HIP(hipMemsetAsync(flags, 0, IC_FLAG_WORDS * 4, c->stream));
    if (use_box) hipLaunchKernelGGL(ic_box_kernel<Real>, dim3((uint32_t)((nbox + 63) / 64)), dim3(64), 0, c->stream, boxes_d, nbox, Z.boxes.as<BoxD>(), flags);
    Prep P{};
    P.tuples = is_device_ptr(tuples) ? tuples_d : nullptr;
    P.ntuple_entries = T * kind;
    P.natoms = natoms;
    P.labels = is_device_ptr(labels) ? labels_d : nullptr;
    P.T = T;
    P.G = G;
    P.pairs = want_map && is_device_ptr(pairs) ? pairs_d : nullptr;
    P.npair_entries = npairs * 2;
    P.plabels = want_map && is_device_ptr(pair_labels) ? plabels_d : nullptr;
    P.P = npairs;
    P.G2 = G2;
    const bool judge = P.tuples || P.labels || P.pairs || P.plabels;
    if (judge) {
        const size_t items = std::max(P.ntuple_entries, want_map ? P.npair_entries : 0);
        hipLaunchKernelGGL(ic_prep_kernel, dim3((uint32_t)std::min<size_t>((items + IC_WG - 1) / IC_WG, 1024)), dim3(IC_WG), 0, c->stream, P, flags);
    }
    MH_HIP(hipGetLastError());
    if (use_box || judge) {
        // the one read-back: the status.  Nothing below runs, no index is used as an address and no output is touched after a
        // bad argument.
        uint32_t hf[IC_FLAG_WORDS];
        MH_TRY(read_back(c, hf, flags, sizeof hf));
        if (hf[0]) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: a tuple index is not below natoms = %zu", who, natoms);
        if (hf[5]) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: a label is not below ngroups = %zu", who, G);
        if (hf[6]) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: a pair entry is not below ntuples = %zu", who, T);
        if (hf[7]) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: a pair label is not below npair_groups = %zu", who, G2);
        if (hf[3]) return fail(MOLAR_HIP_ERR_ZERO_LENGTH_VECTOR, "%s: zero length box vector", who);
        if (hf[1]) return fail(MOLAR_HIP_ERR_INVERSE_FAILED, "%s: box matrix inverse failed", who);
    }

    const bool force_global = std::getenv("MOLAR_HIP_INTCOORD_GLOBAL") != nullptr;      // A/B runs and the tests of the switch
    if (values_d || hist_d || want_stats) {
        Series<Real> S{};
        S.X = X;
        S.tuples = tuples_d;
        S.T = T;
        S.labels = labels_d;
        S.nbins = spec->nbins;
        S.cells = (uint32_t)hcells;
        S.lo = spec->lo;
        S.hi = spec->hi;
        S.tblocks = (uint32_t)tblocks;
        S.values = values_d;
        S.ld = values_d == values ? ld : T;
        S.hist = hist_d;
        S.sum = want_stats ? sum_d : nullptr;
        S.n = n_d;
        const bool lds = hist_d && hcells <= IC_LDS_CELLS && !force_global;
        if (hist_d) MH_HIP(hipMemsetAsync(hist_d, 0, hcells * 8, c->stream));
        const uint32_t grid = (uint32_t)(chunks * tblocks);
        if (kind == MOLAR_HIP_IC_DISTANCE) launch_series<Real, 2>(S, lds, grid, c->stream);
        else if (kind == MOLAR_HIP_IC_ANGLE) launch_series<Real, 3>(S, lds, grid, c->stream);
        else launch_series<Real, 4>(S, lds, grid, c->stream);
        if (want_stats)
            hipLaunchKernelGGL(ic_fold_kernel<Real>, dim3((uint32_t)tblocks), dim3(IC_WG), 0, c->stream, sum_d, n_d, chunks, T, kind, mean_d, spread_d, valid_d);
    }
    if (want_map) {
        MH_HIP(hipMemsetAsync(map_d, 0, mcells * 8, c->stream));
        if (npairs) {
            Map<Real> M{};
            M.X = X;
            M.tuples = tuples_d;
            M.pairs = pairs_d;
            M.P = npairs;
            M.plabels = plabels_d;
            M.mb = spec->map_bins;
            M.cells = (uint32_t)mcells;
            M.lo = spec->lo;
            M.hi = spec->hi;
            M.pblocks = (uint32_t)pblocks;
            M.map = map_d;
            const bool lds = mcells <= IC_LDS_CELLS && !force_global;
            const uint32_t grid = (uint32_t)(chunks * pblocks);
            if (kind == MOLAR_HIP_IC_DISTANCE) launch_map<Real, 2>(M, lds, grid, c->stream);
            else if (kind == MOLAR_HIP_IC_ANGLE) launch_map<Real, 3>(M, lds, grid, c->stream);
            else launch_map<Real, 4>(M, lds, grid, c->stream);
        }
    }
    MH_HIP(hipGetLastError());
    bool wait = false;
    MH_TRY(copy_out_2d(c, values, ld, values_d, T, F, wait));
    MH_TRY(copy_out(c, hist_u, hist_d, hcells, wait));
    MH_TRY(copy_out(c, map_u, map_d, mcells, wait));
    MH_TRY(copy_out(c, mean, mean_d, T, wait));
    MH_TRY(copy_out(c, spread, spread_d, T, wait));
    MH_TRY(copy_out(c, valid_u, valid_d, T, wait));
    return finish_copies(c, wait);
}

}  // namespace

namespace mh {
void intcoord_release(molar_hip_ctx *c) {
    release_state(c->intcoord);
}
}  // namespace mh

extern "C" {

int molar_hip_intcoord_plan(size_t nframes, size_t ntuples, size_t ngroups, size_t npairs, size_t npair_groups, const molar_hip_intcoord_spec *spec,
                            int want_stats, size_t *workspace_bytes, uint32_t *frame_chunk, uint32_t *tuple_chunk, uint32_t *lds_cells) {
    (void)npairs;
    MH_TRY(check_spec("intcoord_plan", spec, ngroups ? ngroups : 1, npair_groups ? npair_groups : 1));
    const Layout Y = make_layout(nframes, ntuples, want_stats != 0);
    if (workspace_bytes) *workspace_bytes = (nframes == 0 || ntuples == 0) ? 0 : Y.bytes;
    if (frame_chunk) *frame_chunk = IC_FRAMES;
    if (tuple_chunk) *tuple_chunk = IC_TUPLES;
    if (lds_cells) *lds_cells = IC_LDS_CELLS;
    return MOLAR_HIP_OK;
}

int molar_hip_intcoord(molar_hip_ctx *c, const float *frames, size_t nframes, size_t frame_stride, size_t natoms, const uint64_t *tuples, size_t ntuples,
                       const uint32_t *labels, size_t ngroups, const float *boxes, size_t box_stride, uint8_t pbc, const molar_hip_intcoord_spec *spec,
                       const uint64_t *pairs, size_t npairs, const uint32_t *pair_labels, size_t npair_groups, float *values, size_t ld, uint64_t *hist,
                       uint64_t *map, float *mean, float *spread, uint64_t *valid) {
    return intcoord_run<float>(c, "intcoord", frames, nframes, frame_stride, natoms, tuples, ntuples, labels, ngroups, boxes, box_stride, pbc, spec, pairs,
                               npairs, pair_labels, npair_groups, values, ld, hist, map, mean, spread, valid);
}

int molar_hip_intcoord_f64(molar_hip_ctx *c, const double *frames, size_t nframes, size_t frame_stride, size_t natoms, const uint64_t *tuples,
                           size_t ntuples, const uint32_t *labels, size_t ngroups, const double *boxes, size_t box_stride, uint8_t pbc,
                           const molar_hip_intcoord_spec *spec, const uint64_t *pairs, size_t npairs, const uint32_t *pair_labels, size_t npair_groups,
                           double *values, size_t ld, uint64_t *hist, uint64_t *map, double *mean, double *spread, uint64_t *valid) {
    return intcoord_run<double>(c, "intcoord_f64", frames, nframes, frame_stride, natoms, tuples, ntuples, labels, ngroups, boxes, box_stride, pbc, spec,
                                pairs, npairs, pair_labels, npair_groups, values, ld, hist, map, mean, spread, valid);
}

}  // extern "C"
