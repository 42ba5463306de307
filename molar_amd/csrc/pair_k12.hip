// pair_k12.hip - instantiates the connected-components kernels (cluster_kernel and the launches around it); see cluster_kernels.hpp.
#include "cluster_kernels.hpp"

namespace mh {
namespace pairk {

// ---------------------------------------------------------------- around the union kernel: one launch per step

__global__ void __launch_bounds__(256) cluster_init_kernel(uint32_t *__restrict__ parent, uint32_t np) {
    for (uint32_t p = blockIdx.x * 256u + threadIdx.x; p < np; p += gridDim.x * 256u) parent[p] = p;
}

// root[p] and the flag "p is a root"; flag has np + 1 entries (the last one 0: its rank is the number of components)
__global__ void __launch_bounds__(256) cluster_flatten_kernel(const uint32_t *__restrict__ parent, uint32_t np, uint32_t *__restrict__ root,
                                                              uint32_t *__restrict__ flag) {
    for (uint32_t p = blockIdx.x * 256u + threadIdx.x; p < np; p += gridDim.x * 256u) {
        uint32_t r = p, q;
        while ((q = parent[r]) != r) r = q;
        root[p] = r;
        flag[p] = r == p ? 1u : 0u;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) flag[np] = 0u;
}

// comp[p] = rank of p's root, sizes[comp] += 1 (sizes zeroed), iota[p] = p (the values of the members' sort)
__global__ void __launch_bounds__(256) cluster_label_kernel(const uint32_t *__restrict__ root, const uint32_t *__restrict__ rank, uint32_t np,
                                                            uint32_t *__restrict__ comp, uint32_t *__restrict__ sizes, uint32_t *__restrict__ iota) {
    for (uint32_t p = blockIdx.x * 256u + threadIdx.x; p < np; p += gridDim.x * 256u) {
        const uint32_t c = rank[root[p]];
        comp[p] = c;
        iota[p] = p;
        atomicAdd(&sizes[c], 1u);
    }
}

// frames form: the frame's number of components and its largest one, one add per component into the size histogram [np + 1]
__global__ void __launch_bounds__(256) cluster_frame_kernel(const uint32_t *__restrict__ flag, const uint32_t *__restrict__ rank,
                                                            const uint32_t *__restrict__ sizes, uint32_t np, uint32_t *__restrict__ ncomp,
                                                            uint32_t *__restrict__ largest, unsigned long long *__restrict__ hist) {
    for (uint32_t p = blockIdx.x * 256u + threadIdx.x; p < np; p += gridDim.x * 256u) {
        if (!flag[p]) continue;
        const uint32_t s = sizes[rank[p]];
        if (largest) atomicMax(largest, s);
        if (hist) atomicAdd(&hist[s], 1ull);
    }
    if (ncomp && blockIdx.x == 0 && threadIdx.x == 0) *ncomp = rank[np];
}

inline unsigned cluster_blocks(unsigned num_cus, uint32_t np) {
    const unsigned nb = (np + 255u) / 256u, cap = num_cus * 16u;
    return nb < cap ? (nb ? nb : 1u) : cap;
}

}  // namespace pairk

void launch_clusters(unsigned num_cus, hipStream_t stream, const pairk::SearchParams *dP, const pairk::SlotDesc *slot_desc, uint32_t nslots,
                     const pairk::ClusterArgs &A) {
    using namespace pairk;
    unsigned nblk = (nslots + (unsigned)CLUSTER_WAVES - 1u) / (unsigned)CLUSTER_WAVES;
    const unsigned cap = num_cus * 8u;
    if (nblk > cap) nblk = cap;
    if (nblk == 0u) return;
    if (A.stats) hipLaunchKernelGGL((cluster_kernel<true>), dim3(nblk), dim3(64 * CLUSTER_WAVES), 0, stream, dP, slot_desc, nslots, A);
    else hipLaunchKernelGGL((cluster_kernel<false>), dim3(nblk), dim3(64 * CLUSTER_WAVES), 0, stream, dP, slot_desc, nslots, A);
}

void launch_cluster_init(unsigned num_cus, hipStream_t stream, uint32_t *parent, uint32_t np) {
    hipLaunchKernelGGL(pairk::cluster_init_kernel, dim3(pairk::cluster_blocks(num_cus, np)), dim3(256), 0, stream, parent, np);
}

void launch_cluster_flatten(unsigned num_cus, hipStream_t stream, const uint32_t *parent, uint32_t np, uint32_t *root, uint32_t *flag) {
    hipLaunchKernelGGL(pairk::cluster_flatten_kernel, dim3(pairk::cluster_blocks(num_cus, np)), dim3(256), 0, stream, parent, np, root, flag);
}

void launch_cluster_label(unsigned num_cus, hipStream_t stream, const uint32_t *root, const uint32_t *rank, uint32_t np, uint32_t *comp,
                          uint32_t *sizes, uint32_t *iota) {
    hipLaunchKernelGGL(pairk::cluster_label_kernel, dim3(pairk::cluster_blocks(num_cus, np)), dim3(256), 0, stream, root, rank, np, comp, sizes, iota);
}

void launch_cluster_frame(unsigned num_cus, hipStream_t stream, const uint32_t *flag, const uint32_t *rank, const uint32_t *sizes, uint32_t np,
                          uint32_t *ncomp, uint32_t *largest, unsigned long long *hist) {
    hipLaunchKernelGGL(pairk::cluster_frame_kernel, dim3(pairk::cluster_blocks(num_cus, np)), dim3(256), 0, stream, flag, rank, sizes, np, ncomp,
                       largest, hist);
}

}  // namespace mh
