// csr_kernels.hpp - small kernels that do not depend on the precision of the search that made the flags or the sorted entries:
// the block scan, the compaction of a flag array into ascending ids (`within` as a set, with the host function that launches
// it) and the last two steps of SearchConnectivity's CSR.  Included by search.hip (the block scan), by within.hip and
// search_f64.hip (the flags of the f32 and the f64 `within` set) and by connectivity.hip (the CSR of both precisions).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.hpp"

namespace {

template <class T>
__device__ __forceinline__ T block_exclusive_scan(T v, T *total) {
    __shared__ T wave_sums[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = (int)(blockDim.x >> 6);
    T inc = v;
    for (int off = 1; off < 64; off <<= 1) {
        T o = __shfl_up(inc, off, 64);
        if (lane >= off) inc += o;
    }
    if (lane == 63) wave_sums[wave] = inc;
    __syncthreads();
    T base = 0, tot = 0;
    for (int w = 0; w < nw; ++w) {
        if (w < wave) base += wave_sums[w];
        tot += wave_sums[w];
    }
    __syncthreads();
    *total = tot;
    return base + inc - v;
}

// off[r] = first sorted entry with row >= r, r = 0 .. nrows (off[nrows] = number of entries)
__global__ void __launch_bounds__(256) conn_offsets_kernel(const uint32_t *__restrict__ row_sorted, unsigned long long nent, uint32_t nrows,
                                                           unsigned long long *__restrict__ off) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r > nrows) return;
    unsigned long long lo = 0, hi = nent;
    while (lo < hi) {
        const unsigned long long mid = (lo + hi) >> 1;
        if (row_sorted[mid] < r) lo = mid + 1;
        else hi = mid;
    }
    off[r] = lo;
}

__global__ void __launch_bounds__(256) conn_widen_kernel(const uint32_t *__restrict__ nb_sorted, unsigned long long nent, unsigned long long *__restrict__ neigh) {
    const unsigned long long e = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    if (e < nent) neigh[e] = nb_sorted[e];
}

// flags -> count per tile of 2048 (8 flags per thread)
__global__ void __launch_bounds__(256) flag_tile_count_kernel(const uint8_t *__restrict__ flags, uint64_t n, uint32_t *__restrict__ tile_cnt) {
    __shared__ uint32_t part[4];
    const uint64_t i = ((uint64_t)blockIdx.x * 256u + threadIdx.x) * 8u;
    uint32_t v = 0;
    for (uint32_t k = 0; k < 8u; ++k) v += (i + k < n && flags[i + k]) ? 1u : 0u;
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if ((threadIdx.x & 63u) == 0u) part[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = (part[0] + part[1]) + (part[2] + part[3]);
}

// positions of the set flags, ascending, as u64
__global__ void __launch_bounds__(256) flag_compact_kernel(const uint8_t *__restrict__ flags, uint64_t n, const unsigned long long *__restrict__ tile_off,
                                                           unsigned long long *__restrict__ out) {
    const uint64_t i = ((uint64_t)blockIdx.x * 256u + threadIdx.x) * 8u;
    uint32_t f[8], v = 0;
    for (uint32_t k = 0; k < 8u; ++k) {
        f[k] = (i + k < n && flags[i + k]) ? 1u : 0u;
        v += f[k];
    }
    uint32_t tot;
    uint32_t at = block_exclusive_scan<uint32_t>(v, &tot);
    unsigned long long o = tile_off[blockIdx.x] + at;
    for (uint32_t k = 0; k < 8u; ++k)
        if (f[k]) out[o++] = i + k;
}

// The end of a within_fill of either precision: the `total` set flags as ascending u64 ids into the caller's array - device
// memory (`dev`) as it is, host memory through `stage`, complete when the call returns.  tile_off: the scanned tile counts.
static inline int flags_to_ids(molar_hip_ctx *c, const uint8_t *flags, uint64_t nflags, const unsigned long long *tile_off, uint64_t total,
                               mh::DevBuf &stage, uint64_t *ids, bool dev) {
    unsigned long long *dst = reinterpret_cast<unsigned long long *>(ids);
    if (!dev) {
        MH_TRY(stage.reserve((size_t)total * 8));
        dst = stage.as<unsigned long long>();
    }
    const uint64_t ntiles = (nflags + 2047) / 2048;
    hipLaunchKernelGGL(flag_compact_kernel, dim3((unsigned)ntiles), dim3(256), 0, c->stream, flags, nflags, tile_off, dst);
    MH_HIP(hipGetLastError());
    if (!dev) {
        MH_HIP(hipMemcpyAsync(ids, dst, (size_t)total * 8, hipMemcpyDeviceToHost, c->stream));
        MH_HIP(hipStreamSynchronize(c->stream));
    }
    return MOLAR_HIP_OK;
}

}  // namespace
