// traj_block.hpp - what the analyses over a block of trajectory frames share (rmsd_matrix.hip, fluct.hip, msd.hip): a block of
// frames with a stride, natoms, an optional idx and an optional mass, host or device memory on either side.  Plain functions
// and two kernels, no state: the gather of a selection, the centring of every frame, the C layout of the f64 MFMA, the carving
// of a workspace, the staging of results, and the host checks of the selection.  (The per-context state's life, state_of / release_state, is in common.hpp.)
#pragma once

#include "common.hpp"

namespace mh {

// ---------------------------------------------------------------- device side

typedef double d4 __attribute__((ext_vector_type(4)));

// Atom k of a selection and its weight; P is anything with idx and mass members (null: 0 .. n-1, unit weights).  The record
// goes in by value: it is a kernel argument, nothing is copied once this is inlined, and through a reference the compiler
// orders fl_sums_kernel, fl_pack_kernel and msd_unwrap_kernel differently from the text written out.
template <class P, class K>
__device__ __forceinline__ uint64_t sel_atom(P p, K k) {
    return p.idx ? p.idx[k] : (uint64_t)k;
}
template <class P>
__device__ __forceinline__ double sel_weight(P p, uint64_t a) {
    return p.mass ? (double)p.mass[a] : 1.0;
}

// the fixed tree of a workgroup of 256 over NV values per thread, from values already in sh and behind a barrier; the result
// is in sh[v][0]
template <int NV>
__device__ __forceinline__ void tree256_sum(double (*sh)[256]) {
    for (uint32_t w = 128u; w > 0u; w >>= 1) {
        if (threadIdx.x < w)
#pragma unroll
            for (int v = 0; v < NV; ++v) sh[v][threadIdx.x] += sh[v][threadIdx.x + w];
        __syncthreads();
    }
}
template <int NV>
__device__ __forceinline__ void tree256(double (*sh)[256], const double *s) {
#pragma unroll
    for (int v = 0; v < NV; ++v) sh[v][threadIdx.x] = s[v];
    __syncthreads();
    tree256_sum<NV>(sh);
}

// One workgroup per frame: {sum w p / sum w, sum w}.  Thread t adds atoms t, t + 256, ... in that order, then the fixed tree:
// every frame's sum of the weights has the same bits.  flags[0]: an index is not below natoms.  In supplies frame(f), idx,
// mass, n and natoms.
template <class In>
__global__ void __launch_bounds__(256) tb_centre_kernel(In P, double *__restrict__ centre, uint32_t *__restrict__ flags) {
    __shared__ double sh[4][256];
    const size_t f = blockIdx.x;
    const auto *p = P.frame(f);
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (uint32_t k = threadIdx.x; k < P.n; k += 256u) {
        const uint64_t a = sel_atom(P, k);
        if (a >= P.natoms) {
            flags[0] = 1u;
            continue;
        }
        const double w = sel_weight(P, a);
        s[0] += w * (double)p[3 * a];
        s[1] += w * (double)p[3 * a + 1];
        s[2] += w * (double)p[3 * a + 2];
        s[3] += w;
    }
    tree256<4>(sh, s);
    if (threadIdx.x < 4u) centre[f * 4 + threadIdx.x] = threadIdx.x < 3u ? sh[threadIdx.x][0] / sh[3][0] : sh[3][0];
}

// The common origin of the mode without a fit: the centre of frame 0; should that frame hold a non-finite coordinate, the
// first centre that is finite (zeros when there is none), so that the other frames stay right.  (A template so that only
// the units that launch it carry it.)
template <class Index = size_t>
__global__ void tb_origin_kernel(const double *__restrict__ centre, Index F, double *__restrict__ origin) {
    double o[3] = {0.0, 0.0, 0.0};
    for (Index f = 0; f < F; ++f) {
        const double x = centre[f * 4], y = centre[f * 4 + 1], z = centre[f * 4 + 2];
        if (isfinite(x) && isfinite(y) && isfinite(z)) {
            o[0] = x;
            o[1] = y;
            o[2] = z;
            break;
        }
    }
    origin[0] = o[0];
    origin[1] = o[1];
    origin[2] = o[2];
}

// The C layout of v_mfma_f64_16x16x4_f64: register r of lane l holds the entry (row (l >> 4) + 4 r, column l & 15) of the tile;
// row0, col0: where the tile starts (added first, as the sites did: a sum of lane terms alone is associated otherwise and
// changes the fused kernels).
__device__ __forceinline__ size_t mfma_c_row(size_t row0, uint32_t lane, uint32_t r) { return row0 + (lane >> 4) + 4u * r; }
__device__ __forceinline__ size_t mfma_c_col(size_t col0, uint32_t lane) { return col0 + (lane & 15u); }

// ---------------------------------------------------------------- workspace layout

// Regions of a workspace one after the other, each rounded up to 256 bytes.
struct Carve {
    size_t bytes = 0;
    void take(size_t &off, size_t region) {
        off = bytes;
        bytes += (region + 255) & ~(size_t)255;
    }
};

// ksteps MFMA steps over (at the most) ks workgroups: steps per split and the splits that leaves, none of them empty.  How ks
// is bounded is the layout's own business.
struct Splits {
    uint32_t kper, ksplits;
};
inline Splits even_splits(uint32_t ksteps, size_t ks) {
    if (ks < 2) ks = 1;
    uint32_t kper = (uint32_t)((ksteps + ks - 1) / ks);
    if (kper == 0) kper = 1;
    return Splits{kper, ksteps ? (ksteps + kper - 1) / kper : 1u};
}

// ---------------------------------------------------------------- buffers and results

// A buffer of exactly `bytes` (no headroom: these are sized by a plan entry), MOLAR_HIP_ERR_TOO_LARGE when the device has not
// got them.
inline int grow_exact(DevBuf &b, size_t bytes, const char *who, const char *what) {
    if (bytes <= b.cap) return 0;
    b.release();
    void *p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess) {
        (void)hipGetLastError();
        return fail(MOLAR_HIP_ERR_TOO_LARGE, "%s: %s of %zu bytes cannot be allocated", who, what, bytes);
    }
    b.p = p;
    b.cap = bytes;
    return 0;
}

// a device destination as it is, a host destination through a staging buffer; a null destination stays null
template <class Real>
int out_buffer(Real *dst, size_t count, DevBuf &stage, const char *who, Real **dev) {
    *dev = dst;
    if (!dst || is_device_ptr(dst)) return 0;
    MH_TRY(grow_exact(stage, count * sizeof(Real), who, "a result"));
    *dev = stage.as<Real>();
    return 0;
}

// The copies of staged results to their host destinations (nothing for a null or a device destination), and their one wait.
template <class Real>
int copy_out(molar_hip_ctx *c, Real *dst, const Real *dev, size_t count, bool &wait) {
    if (!dst || dev == dst) return 0;
    MH_HIP(hipMemcpyAsync(dst, dev, count * sizeof(Real), hipMemcpyDeviceToHost, c->stream));
    wait = true;
    return 0;
}
template <class Real>
int copy_out_2d(molar_hip_ctx *c, Real *dst, size_t ld, const Real *dev, size_t cols, size_t rows, bool &wait) {
    if (!dst || dev == dst) return 0;
    MH_HIP(hipMemcpy2DAsync(dst, ld * sizeof(Real), dev, cols * sizeof(Real), cols * sizeof(Real), rows, hipMemcpyDeviceToHost, c->stream));
    wait = true;
    return 0;
}
inline int finish_copies(molar_hip_ctx *c, bool wait) {
    if (wait) MH_HIP(hipStreamSynchronize(c->stream));
    return 0;
}

// ---------------------------------------------------------------- host checks of a selection
// One function per check; each *_run calls them among its other checks, in the order that decides which error a bad call
// reports first.

// `count_name` atoms without an index are atoms 0 .. count-1 of the frame
inline int check_no_index(const char *who, const char *count_name, const uint64_t *idx, size_t count, size_t natoms) {
    if (!idx && count > natoms)
        return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: %s = %zu exceeds natoms = %zu and there is no index", who, count_name, count, natoms);
    return 0;
}

// (`which`: "the frame stride", or "a frame stride" of a call with two blocks)
inline int check_stride(const char *who, const char *which, size_t F, size_t stride, size_t natoms) {
    if (F > 1 && stride < natoms * 3) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: %s is below 3 * natoms = %zu", who, which, natoms * 3);
    return 0;
}

// an index in host memory is walked here; one in device memory is judged by the kernels (check_selection, msd.hip's flags)
inline int check_index(const char *who, const char *name, const uint64_t *idx, size_t count, size_t natoms) {
    if (idx && !is_device_ptr(idx))
        for (size_t k = 0; k < count; ++k)
            if (idx[k] >= natoms)
                return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: %s[%zu] = %llu is not below natoms = %zu", who, name, k, (unsigned long long)idx[k], natoms);
    return 0;
}

// The status check of the fitted analyses (rmsd_matrix.hip, fluct.hip): the index flag tb_centre_kernel raised and the sum of
// the selected weights, from two device buffers under one wait.
inline int check_selection(molar_hip_ctx *c, const uint32_t *index_flag_dev, const double *weight_sum_dev, const char *who, size_t natoms) {
    MH_TRY(ensure_pinned(c, 16));
    double *sum = static_cast<double *>(c->h_pinned);
    uint32_t *flag = reinterpret_cast<uint32_t *>(sum + 1);
    MH_HIP(hipMemcpyAsync(sum, weight_sum_dev, 8, hipMemcpyDeviceToHost, c->stream));
    MH_HIP(hipMemcpyAsync(flag, index_flag_dev, 4, hipMemcpyDeviceToHost, c->stream));
    MH_HIP(hipStreamSynchronize(c->stream));
    if (*flag) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: a selection index is not below natoms = %zu", who, natoms);
    if (*sum == 0.0) return fail(MOLAR_HIP_ERR_ZERO_MASS, "%s: the selected masses add up to zero", who);
    return 0;
}

}  // namespace mh
