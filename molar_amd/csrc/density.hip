// density.hip - density profiles and maps of a block of trajectory frames: every selected atom of every frame is put into
// a bin of a regular grid by its position, and the bins' sums of weights per unit volume are averaged over the frames.
// The definition is in molar_hip.h.
//
//   BOX mode:  s = inv(box_f) p;  u_d = s_d (- c_d + 1/2 on a centred dimension), wrapped into [0, 1) on the periodic dimensions
//   LAB mode:  u_d = ((p_d - c_d) - lo_d) * (1 / (hi_d - lo_d))
//   b_d = min(floor(u_d nbins_d), nbins_d - 1);  an atom with a u_d outside [0, 1) is dropped and counted in outside[f]
//   I_f[g][b] = sum of q_k = llrint(w_k 2^S) over the atoms of group g in bin b of frame f          (integers)
//   density[g][b] = (1 / F) sum_f (double)I_f[g][b] * (2^-S / binvol_f)                              (frames in order)
//
// Stages, all on the context's stream:
//
//   boxes (one thread per frame: the inverse and the bin volume in double)
//   ->  prep: the indices, the labels and the weights judged, the largest |weight| by one integer max
//   ->  centre (one workgroup per frame: thread-strided partial sums and the fixed tree of 256, as tb_centre_kernel)
//   ->  64 bytes read back: the status and the largest |weight|, from which the host takes the weights' scale S
//   ->  per chunk of frames:  binning (a workgroup takes DN_ATOMS atoms of one frame; the histogram in LDS when all G * nb
//       cells fit, flushed cell by cell with integer atomics into the frame's buffer; else agent-scope integer atomics
//       straight into it)  ->  fold (one lane per cell: the frames of the chunk in order, the buffer cleared)
//   ->  the centres and bin volumes rounded to Real.
//
// Only integer atomics: no result depends on the order in which workgroups arrive, the same call gives the same bits.
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "boxmath.hpp"
#include "common.hpp"
#include "traj_block.hpp"

using namespace mh;

struct molar_hip_density_state {
    DevBuf in_frames, in_idx, in_weight, in_labels, in_boxes, in_cidx, in_cweight;   // host inputs staged here
    DevBuf ws;                                                                        // the workspace molar_hip_density_plan reports
};

namespace {

typedef unsigned long long u64;

constexpr uint32_t DN_WG = 256;                  // threads of every workgroup here
constexpr uint32_t DN_ATOMS = 8192;              // selected atoms of one frame per workgroup of the binning kernels
constexpr uint32_t DN_LDS_CELLS = 4096;          // G * nb the on-chip kernel takes: 4 + 8 bytes per cell, 48 KiB
constexpr uint32_t DN_MAX_REPLICAS = 16;         // copies of a small histogram in LDS, one per lane modulo
constexpr uint32_t DN_MAX_FRAMES = 64;           // frames per chunk at the most
constexpr size_t DN_FRAME_BYTES = (size_t)256 << 20;   // the integer buffers of a chunk of frames together, unless one frame's is larger
constexpr double DN_TWO_PI = 6.283185307179586476925286766559;

// flags[0]: an index not below natoms; [1]: a box matrix without an inverse; [2]: centre weights that add up to zero;
// [3]: a box vector of zero length; [4]: a selected weight that is not finite; [5]: a label not below ngroups;
// [6]: a centre weight that is negative or not finite; bytes 32 - 39: the bits of the largest |weight| as a double
constexpr uint32_t DN_FLAG_WORDS = 16;

struct DnBox {
    double inv[9];       // column-major inverse of the frame's box (BOX mode)
    double binvol;
};

// Where everything lives in the workspace, from the sizes alone (the plan entry and the call share it).
struct Layout {
    size_t cells;
    uint32_t frame_chunk;
    size_t off_flags, off_box, off_centre, off_outside, off_acc, off_count, off_dens, off_cout, off_bvout, off_sum, bytes;
};

Layout make_layout(size_t F, size_t G, size_t nb) {
    Layout Y{};
    Y.cells = G * nb;
    const size_t per_frame = Y.cells * 8;
    Y.frame_chunk = (uint32_t)std::max<size_t>(1, std::min<size_t>(DN_MAX_FRAMES, per_frame ? DN_FRAME_BYTES / per_frame : DN_MAX_FRAMES));
    Carve ws;
    ws.take(Y.off_flags, DN_FLAG_WORDS * 4);
    ws.take(Y.off_box, F * sizeof(DnBox));
    ws.take(Y.off_centre, F * 4 * 8);
    ws.take(Y.off_outside, F * 8);
    ws.take(Y.off_acc, per_frame);
    ws.take(Y.off_count, per_frame);
    ws.take(Y.off_dens, per_frame);
    ws.take(Y.off_cout, F * 3 * 8);
    ws.take(Y.off_bvout, F * 8);
    // min(F, frame_chunk) frames fit, and the region never shrinks when F or the cells grow (frame_chunk * per_frame alone would)
    ws.take(Y.off_sum, std::min(std::min<size_t>(F, DN_MAX_FRAMES) * per_frame, std::max(DN_FRAME_BYTES, per_frame)));
    Y.bytes = ws.bytes;
    return Y;
}

// One thread per frame.  BOX mode: the inverse of the frame's box as PeriodicBox::from_matrix forms it (its two errors
// raise flags[3] and flags[1]) and binvol = |det| / nb; LAB mode: the one bin volume of the call.
template <class Real>
__global__ void __launch_bounds__(64) dn_box_kernel(const Real *__restrict__ boxes, size_t box_stride, size_t F, uint32_t mode, double lab_binvol,
                                                    double nb, DnBox *__restrict__ out, uint32_t *__restrict__ flags) {
    const size_t f = (size_t)blockIdx.x * 64u + threadIdx.x;
    if (f >= F) return;
    DnBox B;
#pragma unroll
    for (int q = 0; q < 9; ++q) B.inv[q] = 0.0;
    B.binvol = lab_binvol;
    if (mode == MOLAR_HIP_DENSITY_BOX) {
        double m[9];
#pragma unroll
        for (int q = 0; q < 9; ++q) m[q] = (double)boxes[f * box_stride + q];
        bool ok = true;
        for (int k = 0; k < 3; ++k)
            if (sqrt(norm2(D3{m[3 * k], m[3 * k + 1], m[3 * k + 2]})) == 0.0) ok = false;
#pragma unroll
        for (int q = 0; q < 9; ++q) B.inv[q] = __builtin_nan("");
        if (!ok) flags[3] = 1u;
        else if (!inverse3(m, B.inv)) flags[1] = 1u;
        const double det = (m[0] * (m[4] * m[8] - m[5] * m[7]) - m[3] * (m[1] * m[8] - m[2] * m[7])) + m[6] * (m[1] * m[5] - m[2] * m[4]);
        B.binvol = fabs(det) / nb;
    }
    out[f] = B;
}

template <class Real>
struct Prep {
    const uint64_t *idx;
    size_t n, natoms;
    const Real *weight;
    const uint32_t *labels;       // null: none to judge here (one group, or labels the host has walked)
    uint32_t ngroups;
    const uint64_t *cidx;
    size_t ncentre;
    const Real *cweight;
};

// Grid-stride over the selection and the centre set: the flags above, and the largest |weight| of the selection - the bits
// of a non-negative finite double order as the numbers do, so one integer max per workgroup gives it.
template <class Real>
__global__ void __launch_bounds__(DN_WG) dn_prep_kernel(Prep<Real> P, uint32_t *__restrict__ flags) {
    __shared__ u64 sh[DN_WG];
    const size_t step = (size_t)gridDim.x * DN_WG, t0 = (size_t)blockIdx.x * DN_WG + threadIdx.x;
    u64 m = 0;
    for (size_t k = t0; k < P.n; k += step) {
        const uint64_t a = P.idx ? P.idx[k] : (uint64_t)k;
        if (a >= P.natoms) flags[0] = 1u;
        else if (P.weight) {
            const double w = fabs((double)P.weight[a]);
            if (!isfinite(w)) flags[4] = 1u;
            else m = max(m, (u64)__double_as_longlong(w));
        }
        if (P.labels && P.labels[k] >= P.ngroups) flags[5] = 1u;
    }
    for (size_t k = t0; k < P.ncentre; k += step) {
        const uint64_t a = P.cidx ? P.cidx[k] : (uint64_t)k;
        if (a >= P.natoms) flags[0] = 1u;
        else if (P.cweight) {
            const double w = (double)P.cweight[a];
            if (!(w >= 0.0) || !isfinite(w)) flags[6] = 1u;
        }
    }
    sh[threadIdx.x] = m;
    __syncthreads();
    for (uint32_t w = DN_WG / 2; w > 0u; w >>= 1) {
        if (threadIdx.x < w) sh[threadIdx.x] = max(sh[threadIdx.x], sh[threadIdx.x + w]);
        __syncthreads();
    }
    if (threadIdx.x == 0u && sh[0]) atomicMax(reinterpret_cast<u64 *>(flags + 8), sh[0]);
}

template <class Real>
struct Frames {
    const Real *frames;
    size_t stride, natoms;
};

// One workgroup per frame: the centre of the centre set on the masked dimensions.  Thread t adds atoms t, t + 256, ... in that
// order, then the fixed tree.  On a masked dimension that is periodic (BOX mode) the sums are of w sin(2 pi s) and
// w cos(2 pi s) and the centre is the circular mean; else of w s (BOX) or w p (LAB).  centre[f] = {c_x, c_y, c_z, W}, 0 on a
// dimension that is not masked.  flags[0], flags[2] as above.
template <class Real>
__global__ void __launch_bounds__(DN_WG) dn_centre_kernel(Frames<Real> X, const uint64_t *__restrict__ cidx, size_t nc, const Real *__restrict__ cweight,
                                                          const DnBox *__restrict__ boxes, uint32_t mode, uint32_t pbc, uint32_t cdims,
                                                          double *__restrict__ centre, uint32_t *__restrict__ flags) {
    __shared__ double sh[7][256];
    const size_t f = blockIdx.x;
    const Real *p = X.frames + f * X.stride;
    double inv[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) inv[q] = boxes[f].inv[q];
    double s[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (size_t k = threadIdx.x; k < nc; k += DN_WG) {
        const uint64_t a = cidx ? cidx[k] : (uint64_t)k;
        if (a >= X.natoms) {
            flags[0] = 1u;
            continue;
        }
        const double w = cweight ? (double)cweight[a] : 1.0;
        D3 v{(double)p[3 * a], (double)p[3 * a + 1], (double)p[3 * a + 2]};
        if (mode == MOLAR_HIP_DENSITY_BOX) v = mat_vec(inv, v);
        const double comp[3] = {v.x, v.y, v.z};
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            if (!(cdims >> d & 1u)) continue;
            if (mode == MOLAR_HIP_DENSITY_BOX && (pbc >> d & 1u)) {
                const double th = DN_TWO_PI * comp[d];
                s[2 * d] += w * sin(th);
                s[2 * d + 1] += w * cos(th);
            } else {
                s[2 * d] += w * comp[d];
            }
        }
        s[6] += w;
    }
    tree256<7>(sh, s);
    if (threadIdx.x == 0u) {
        const double W = sh[6][0];
        if (W == 0.0) flags[2] = 1u;
        for (int d = 0; d < 3; ++d) {
            double c = 0.0;
            if (cdims >> d & 1u) {
                if (mode == MOLAR_HIP_DENSITY_BOX && (pbc >> d & 1u)) c = atan2(-sh[2 * d][0], -sh[2 * d + 1][0]) / DN_TWO_PI + 0.5;
                else c = sh[2 * d][0] / W;
            }
            centre[f * 4 + d] = c;
        }
        centre[f * 4 + 3] = W;
    }
}

template <class Real>
struct Bin {
    Frames<Real> X;
    const uint64_t *idx;
    size_t n;
    const Real *weight;
    const uint32_t *labels;
    const DnBox *boxes;
    const double *centre;          // [F][4], or null: no centring
    uint32_t mode, pbc, cdims;
    uint32_t nbins[3];
    double lo[3], invw[3];         // LAB mode: lo_d and 1 / (hi_d - lo_d)
    uint32_t nb, cells, replicas;  // bins, G * nb, copies of the histogram in LDS (a power of two)
    int32_t S;
    size_t f0;                     // the first frame of the chunk
    u64 *sum;                      // [frames of the chunk][cells]: I_f as two's complement
    u64 *count;                    // [cells]
    u64 *outside;                  // [F]
};

// Workgroup (blockIdx.x, blockIdx.y): selected atoms [x DN_ATOMS, (x + 1) DN_ATOMS) of frame f0 + y, thread-strided so that
// the 12- or 24-byte gathers of a wave through idx are as coalesced as idx is.  The box row, the centre and the grid are the
// same for the whole workgroup (scalar registers).  LDS: the histogram of the workgroup on chip, lane l in copy
// l mod replicas, flushed with one integer atomic per non-zero quantity of a cell; else integer atomics straight into the
// frame's buffer.  Both add the same integers to the same cells.
template <class Real, bool LDS>
__global__ void __launch_bounds__(DN_WG) dn_bin_kernel(Bin<Real> B) {
    __shared__ u64 sh_sum[LDS ? DN_LDS_CELLS : 1];
    __shared__ uint32_t sh_cnt[LDS ? DN_LDS_CELLS : 1];
    __shared__ uint32_t sh_out;
    const uint32_t t = threadIdx.x;
    const size_t f = B.f0 + blockIdx.y;
    const size_t k0 = (size_t)blockIdx.x * DN_ATOMS, k1 = k0 + DN_ATOMS < B.n ? k0 + DN_ATOMS : B.n;
    if (LDS)
        for (uint32_t i = t; i < B.cells * B.replicas; i += DN_WG) {
            sh_sum[i] = 0;
            sh_cnt[i] = 0u;
        }
    if (t == 0u) sh_out = 0u;
    __syncthreads();

    double inv[9], c[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int q = 0; q < 9; ++q) inv[q] = B.boxes[f].inv[q];
    bool frame_ok = true;
    if (B.centre)
        for (int d = 0; d < 3; ++d) {
            c[d] = B.centre[f * 4 + d];
            if (!isfinite(c[d])) frame_ok = false;      // a centre that is not finite drops every atom of the frame
        }
    const bool box_mode = B.mode == MOLAR_HIP_DENSITY_BOX;
    const double scale = ldexp(1.0, B.S);
    const Real *p = B.X.frames + f * B.X.stride;
    u64 *fsum = B.sum + (size_t)blockIdx.y * B.cells;
    const uint32_t rep = (t & (B.replicas - 1u)) * B.cells;
    uint32_t dropped = 0;
    for (size_t k = k0 + t; k < k1; k += DN_WG) {
        const uint64_t a = B.idx ? B.idx[k] : (uint64_t)k;
        const D3 x{(double)p[3 * a], (double)p[3 * a + 1], (double)p[3 * a + 2]};
        double u[3];
        if (box_mode) {
            const D3 s = mat_vec(inv, x);
            u[0] = s.x;
            u[1] = s.y;
            u[2] = s.z;
        } else {
            u[0] = ((x.x - c[0]) - B.lo[0]) * B.invw[0];
            u[1] = ((x.y - c[1]) - B.lo[1]) * B.invw[1];
            u[2] = ((x.z - c[2]) - B.lo[2]) * B.invw[2];
        }
        bool in = frame_ok;
        uint32_t cell = 0;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            double v = u[d];
            bool ok;
            if (box_mode) {
                if (B.cdims >> d & 1u) v = (v - c[d]) + 0.5;
                if (B.pbc >> d & 1u) {
                    v -= floor(v);
                    ok = v >= 0.0 && v <= 1.0;          // 1 only by rounding of a tiny negative v: the last bin (below)
                } else {
                    ok = v >= 0.0 && v < 1.0;
                }
            } else {
                ok = v >= 0.0 && v < 1.0;
            }
            in = in && ok;
            const double fb = floor(v * (double)B.nbins[d]);
            uint32_t b = ok ? (uint32_t)fb : 0u;
            if (b > B.nbins[d] - 1u) b = B.nbins[d] - 1u;
            cell = cell * B.nbins[d] + b;
        }
        if (!in) {
            ++dropped;
            continue;
        }
        const uint32_t g = B.labels ? B.labels[k] : 0u;
        const long long q = B.weight ? llrint((double)B.weight[a] * scale) : 1ll;
        const uint32_t ci = g * B.nb + cell;
        if (LDS) {
            atomicAdd(&sh_cnt[rep + ci], 1u);
            atomicAdd(&sh_sum[rep + ci], (u64)q);
        } else {
            if (q) atomicAdd(&fsum[ci], (u64)q);
            atomicAdd(&B.count[ci], (u64)1);
        }
    }
    if (dropped) atomicAdd(&sh_out, dropped);
    __syncthreads();
    if (LDS)
        for (uint32_t i = t; i < B.cells; i += DN_WG) {
            u64 s = 0;
            uint32_t n = 0;
            for (uint32_t r = 0; r < B.replicas; ++r) {
                s += sh_sum[r * B.cells + i];
                n += sh_cnt[r * B.cells + i];
            }
            if (s) atomicAdd(&fsum[i], s);
            if (n) atomicAdd(&B.count[i], (u64)n);
        }
    if (t == 0u && sh_out) atomicAdd(&B.outside[f], (u64)sh_out);
}

// One lane per cell (g, b): the frames of the chunk in order into the cell's running sum, the buffer cleared behind it; the
// last chunk rounds the mean over the frames to Real.
template <class Real>
__global__ void __launch_bounds__(DN_WG) dn_fold_kernel(u64 *__restrict__ sum, uint32_t nf, size_t f0, size_t cells, const DnBox *__restrict__ boxes,
                                                        int32_t S, double *__restrict__ acc, Real *__restrict__ density, size_t F, int last) {
    const size_t i = (size_t)blockIdx.x * DN_WG + threadIdx.x;
    if (i >= cells) return;
    const double unit = ldexp(1.0, -S);
    double a = acc[i];
    for (uint32_t j = 0; j < nf; ++j) {
        const long long I = (long long)sum[(size_t)j * cells + i];
        sum[(size_t)j * cells + i] = 0;
        a += (double)I * (unit / boxes[f0 + j].binvol);
    }
    acc[i] = a;
    if (last && density) density[i] = (Real)(a / (double)F);
}

// One thread per frame: the centre used and the bin volume, rounded to Real.
template <class Real>
__global__ void __launch_bounds__(64) dn_out_kernel(const double *__restrict__ centre, const DnBox *__restrict__ boxes, size_t F, Real *__restrict__ cout,
                                                    Real *__restrict__ bvout) {
    const size_t f = (size_t)blockIdx.x * 64u + threadIdx.x;
    if (f >= F) return;
    for (int d = 0; d < 3; ++d) cout[f * 3 + d] = centre ? (Real)centre[f * 4 + d] : (Real)0;
    bvout[f] = (Real)boxes[f].binvol;
}

int ceil_log2(size_t n) {
    int c = 0;
    while (c < 63 && ((size_t)1 << c) < n) ++c;
    return c;
}

// the grid alone: the mode, the bins and the LAB range; *nb_out = nx ny nz
int check_grid(const char *who, const molar_hip_density_grid *grid, size_t *nb_out) {
    if (!grid) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: the grid is null", who);
    if (grid->mode != MOLAR_HIP_DENSITY_BOX && grid->mode != MOLAR_HIP_DENSITY_LAB)
        return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: grid mode = %u is neither BOX nor LAB", who, grid->mode);
    size_t nb = 1;
    for (int d = 0; d < 3; ++d) {
        if (grid->nbins[d] == 0) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: nbins[%d] is zero", who, d);
        if (grid->mode == MOLAR_HIP_DENSITY_LAB && !(grid->hi[d] > grid->lo[d]) )
            return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: hi[%d] = %g is not above lo[%d] = %g", who, d, grid->hi[d], d, grid->lo[d]);
        if (grid->mode == MOLAR_HIP_DENSITY_LAB && !(std::isfinite(grid->hi[d]) && std::isfinite(grid->lo[d])))
            return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: the range of dimension %d is not finite", who, d);
        nb *= grid->nbins[d];
        if (nb >= 0x80000000ull) return fail(MOLAR_HIP_ERR_TOO_LARGE, "%s: 2^31 bins or more", who);
    }
    if (grid->centre_dims > 7) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: centre_dims = %u is not a mask of x, y, z", who, grid->centre_dims);
    *nb_out = nb;
    return 0;
}

template <class T>
int copy_any(molar_hip_ctx *c, T *dst, const T *dev, size_t count, bool &wait) {
    if (!dst) return 0;
    if (!is_device_ptr(dst)) wait = true;
    MH_HIP(hipMemcpyAsync(dst, dev, count * sizeof(T), hipMemcpyDefault, c->stream));
    return 0;
}

template <class Real>
int density_run(molar_hip_ctx *c, const char *who, const Real *frames, size_t F, size_t stride, size_t natoms, const uint64_t *idx, size_t n,
                const Real *weight, const uint32_t *labels, size_t ngroups, const Real *boxes, size_t box_stride, uint8_t pbc,
                const molar_hip_density_grid *grid, const uint64_t *centre_idx, size_t ncentre, const Real *centre_weight, Real *density,
                uint64_t *count, uint64_t *outside, Real *centre, Real *binvol, int32_t *weight_scale_log2) {
    // the arguments are judged before the context is used
    if (!c) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "null context");
    if (n == 0) return fail(MOLAR_HIP_ERR_SIZES, "%s: empty selection", who);
    const size_t G = labels ? ngroups : 1;
    if (G == 0) return fail(MOLAR_HIP_ERR_SIZES, "%s: labels and ngroups = 0", who);
    size_t nb = 0;
    MH_TRY(check_grid(who, grid, &nb));
    if (pbc > 7) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: pbc = %u is not a PbcDims byte", who, (unsigned)pbc);
    if (box_stride != 0 && box_stride != 9) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: box_stride = %zu is neither 0 nor 9", who, box_stride);
    if (natoms == 0) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: a selection of %zu atoms out of natoms = 0", who, n);
    MH_TRY(check_no_index(who, "n", idx, n, natoms));
    MH_TRY(check_no_index(who, "ncentre", centre_idx, ncentre, natoms));
    MH_TRY(check_stride(who, "the frame stride", F, stride, natoms));
    const bool box_mode = grid->mode == MOLAR_HIP_DENSITY_BOX;
    if (box_mode && !boxes) return fail(MOLAR_HIP_ERR_NO_PBC, "%s: a grid in BOX mode without periodic box", who);
    if (n >= 0x7FFFFF00ull || ncentre >= 0x7FFFFF00ull || F >= 0x7FFFFFF0ull) return fail(MOLAR_HIP_ERR_TOO_LARGE, "%s: more than 2^31 atoms or frames", who);
    if (G >= 0x80000000ull || G * nb >= 0x80000000ull) return fail(MOLAR_HIP_ERR_TOO_LARGE, "%s: 2^31 cells (groups times bins) or more", who);
    if (F == 0) return MOLAR_HIP_OK;
    if (!frames) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: the frames pointer is null", who);
    MH_TRY(check_index(who, "idx", idx, n, natoms));
    MH_TRY(check_index(who, "centre_idx", centre_idx, ncentre, natoms));
    // labels in host memory are walked here; those in device memory are judged by the prep kernel before one is used as an address
    const bool labels_dev = is_device_ptr(labels);
    if (labels && !labels_dev)
        for (size_t k = 0; k < n; ++k)
            if (labels[k] >= G) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: labels[%zu] = %u is not below ngroups = %zu", who, k, labels[k], G);
    MH_HIP(hipSetDevice(c->device));

    const Layout Y = make_layout(F, G, nb);
    molar_hip_density_state &Z = state_of(c->density);
    MH_TRY(grow_exact(Z.ws, Y.bytes, who, "the workspace"));
    char *W = Z.ws.as<char>();
    uint32_t *flags = reinterpret_cast<uint32_t *>(W + Y.off_flags);
    DnBox *boxd = reinterpret_cast<DnBox *>(W + Y.off_box);
    double *centre_d = reinterpret_cast<double *>(W + Y.off_centre), *acc = reinterpret_cast<double *>(W + Y.off_acc);
    u64 *outside_d = reinterpret_cast<u64 *>(W + Y.off_outside), *count_d = reinterpret_cast<u64 *>(W + Y.off_count);
    u64 *sum_d = reinterpret_cast<u64 *>(W + Y.off_sum);
    Real *dens_d = reinterpret_cast<Real *>(W + Y.off_dens), *cout_d = reinterpret_cast<Real *>(W + Y.off_cout);
    Real *bvout_d = reinterpret_cast<Real *>(W + Y.off_bvout);

    Frames<Real> X{};
    X.stride = stride;
    X.natoms = natoms;
    const uint64_t *idx_d = nullptr, *cidx_d = nullptr;
    const Real *weight_d = nullptr, *cweight_d = nullptr, *boxes_d = nullptr;
    const uint32_t *labels_d = nullptr;
    const bool centring = ncentre != 0 && grid->centre_dims != 0;
    MH_TRY(to_device(c, frames, (F - 1) * stride + natoms * 3, Z.in_frames, &X.frames));
    MH_TRY(to_device(c, idx, idx ? n : 0, Z.in_idx, &idx_d));
    MH_TRY(to_device(c, weight, weight ? natoms : 0, Z.in_weight, &weight_d));
    MH_TRY(to_device(c, labels, labels ? n : 0, Z.in_labels, &labels_d));
    MH_TRY(to_device(c, box_mode ? boxes : nullptr, box_stride ? F * 9 : 9, Z.in_boxes, &boxes_d));
    MH_TRY(to_device(c, centring ? centre_idx : nullptr, ncentre, Z.in_cidx, &cidx_d));
    MH_TRY(to_device(c, centring ? centre_weight : nullptr, natoms, Z.in_cweight, &cweight_d));

    double lab_binvol = 1.0;
    if (!box_mode)
        for (int d = 0; d < 3; ++d) {
            const double wd = (grid->hi[d] - grid->lo[d]) / (double)grid->nbins[d];
            lab_binvol = d ? lab_binvol * wd : wd;
        }
    MH_HIP(hipMemsetAsync(flags, 0, DN_FLAG_WORDS * 4, c->stream));
    const uint32_t fblocks = (uint32_t)((F + 63) / 64);
    hipLaunchKernelGGL(dn_box_kernel<Real>, dim3(fblocks), dim3(64), 0, c->stream, boxes_d, box_stride, F, grid->mode, lab_binvol, (double)nb, boxd, flags);
    Prep<Real> P{};
    P.idx = idx_d;
    P.n = n;
    P.natoms = natoms;
    P.weight = weight_d;
    P.labels = labels_dev ? labels_d : nullptr;
    P.ngroups = (uint32_t)G;
    P.cidx = cidx_d;
    P.ncentre = centring ? ncentre : 0;
    P.cweight = cweight_d;
    const size_t prep_items = std::max(n, P.ncentre);
    hipLaunchKernelGGL(dn_prep_kernel<Real>, dim3((uint32_t)std::min<size_t>((prep_items + DN_WG - 1) / DN_WG, 1024)), dim3(DN_WG), 0, c->stream, P, flags);
    if (centring)
        hipLaunchKernelGGL(dn_centre_kernel<Real>, dim3((uint32_t)F), dim3(DN_WG), 0, c->stream, X, cidx_d, ncentre, cweight_d, boxd, grid->mode, (uint32_t)pbc,
                           grid->centre_dims, centre_d, flags);
    MH_HIP(hipGetLastError());
    // the one read-back: the status, and the largest |weight| the scale is taken from.  Nothing below runs, no label is used
    // as an address and no output is touched after a bad argument.
    uint32_t hf[DN_FLAG_WORDS];
    MH_TRY(read_back(c, hf, flags, sizeof hf));
    if (hf[0]) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: a selection index is not below natoms = %zu", who, natoms);
    if (hf[5]) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: a label is not below ngroups = %zu", who, G);
    if (hf[4]) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: a selected weight is not finite", who);
    if (hf[6]) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: a centre weight is negative or not finite", who);
    if (hf[3]) return fail(MOLAR_HIP_ERR_ZERO_LENGTH_VECTOR, "%s: zero length box vector", who);
    if (hf[1]) return fail(MOLAR_HIP_ERR_INVERSE_FAILED, "%s: box matrix inverse failed", who);
    if (hf[2]) return fail(MOLAR_HIP_ERR_ZERO_MASS, "%s: the weights of the centre set add up to zero", who);
    // S = 62 - ceil(log2 n) - e, e the smallest integer with max |w| < 2^e: n |q| < 2^62 whatever the bins
    int32_t S = 0;
    if (weight) {
        u64 bits;
        double wmax;
        memcpy(&bits, hf + 8, 8);
        memcpy(&wmax, &bits, 8);
        if (wmax == 0.0) {
            S = 52;
        } else {
            int e = 0;
            (void)std::frexp(wmax, &e);                    // wmax = m 2^e, 1/2 <= m < 1
            const int raw = 62 - ceil_log2(n) - e;
            if (raw < 0) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: %zu weights of up to %g do not fit an exact 64-bit sum", who, n, wmax);
            S = raw > 52 ? 52 : raw;
        }
    }
    if (weight_scale_log2) *weight_scale_log2 = S;

    const bool force_global = std::getenv("MOLAR_HIP_DENSITY_GLOBAL") != nullptr;      // A/B runs and the tests of the switch
    const bool lds = Y.cells <= DN_LDS_CELLS && !force_global;
    Bin<Real> B{};
    B.X = X;
    B.idx = idx_d;
    B.n = n;
    B.weight = weight_d;
    B.labels = labels_d;
    B.boxes = boxd;
    B.centre = centring ? centre_d : nullptr;
    B.mode = grid->mode;
    B.pbc = pbc;
    B.cdims = centring ? grid->centre_dims : 0u;
    for (int d = 0; d < 3; ++d) {
        B.nbins[d] = grid->nbins[d];
        B.lo[d] = box_mode ? 0.0 : grid->lo[d];
        B.invw[d] = box_mode ? 1.0 : 1.0 / (grid->hi[d] - grid->lo[d]);
    }
    B.nb = (uint32_t)nb;
    B.cells = (uint32_t)Y.cells;
    B.replicas = 1;
    while (lds && B.replicas < DN_MAX_REPLICAS && (size_t)B.replicas * 2 * Y.cells <= DN_LDS_CELLS) B.replicas *= 2;
    B.S = S;
    B.sum = sum_d;
    B.count = count_d;
    B.outside = outside_d;
    const uint32_t fc = (uint32_t)std::min<size_t>(Y.frame_chunk, F);
    MH_HIP(hipMemsetAsync(acc, 0, Y.cells * 8, c->stream));
    MH_HIP(hipMemsetAsync(count_d, 0, Y.cells * 8, c->stream));
    MH_HIP(hipMemsetAsync(outside_d, 0, F * 8, c->stream));
    MH_HIP(hipMemsetAsync(sum_d, 0, (size_t)fc * Y.cells * 8, c->stream));
    const uint32_t ablocks = (uint32_t)((n + DN_ATOMS - 1) / DN_ATOMS), cblocks = (uint32_t)((Y.cells + DN_WG - 1) / DN_WG);
    for (size_t f0 = 0; f0 < F; f0 += fc) {
        const uint32_t nf = (uint32_t)std::min<size_t>(fc, F - f0);
        B.f0 = f0;
        if (lds) hipLaunchKernelGGL((dn_bin_kernel<Real, true>), dim3(ablocks, nf), dim3(DN_WG), 0, c->stream, B);
        else hipLaunchKernelGGL((dn_bin_kernel<Real, false>), dim3(ablocks, nf), dim3(DN_WG), 0, c->stream, B);
        hipLaunchKernelGGL(dn_fold_kernel<Real>, dim3(cblocks), dim3(DN_WG), 0, c->stream, sum_d, nf, f0, Y.cells, boxd, S, acc, density ? dens_d : nullptr, F,
                           f0 + nf >= F ? 1 : 0);
    }
    if (centre || binvol)
        hipLaunchKernelGGL(dn_out_kernel<Real>, dim3(fblocks), dim3(64), 0, c->stream, centring ? centre_d : nullptr, boxd, F, cout_d, bvout_d);
    MH_HIP(hipGetLastError());
    bool wait = false;
    MH_TRY(copy_any(c, density, dens_d, Y.cells, wait));
    MH_TRY(copy_any(c, reinterpret_cast<u64 *>(count), count_d, Y.cells, wait));
    MH_TRY(copy_any(c, reinterpret_cast<u64 *>(outside), outside_d, F, wait));
    MH_TRY(copy_any(c, centre, cout_d, F * 3, wait));
    MH_TRY(copy_any(c, binvol, bvout_d, F, wait));
    return finish_copies(c, wait);
}

}  // namespace

namespace mh {
void density_release(molar_hip_ctx *c) {
    release_state(c->density);
}
}  // namespace mh

extern "C" {

int molar_hip_density_plan(size_t nframes, size_t n, size_t ngroups, const molar_hip_density_grid *grid, size_t *workspace_bytes,
                           uint32_t *frame_chunk, uint32_t *atom_chunk, uint32_t *lds_cells) {
    size_t nb = 0;
    MH_TRY(check_grid("density_plan", grid, &nb));
    const size_t G = ngroups ? ngroups : 1;
    if (G >= 0x80000000ull || G * nb >= 0x80000000ull) return fail(MOLAR_HIP_ERR_TOO_LARGE, "density_plan: 2^31 cells (groups times bins) or more");
    const Layout Y = make_layout(nframes, G, nb);
    if (workspace_bytes) *workspace_bytes = (nframes == 0 || n == 0) ? 0 : Y.bytes;
    if (frame_chunk) *frame_chunk = Y.frame_chunk;
    if (atom_chunk) *atom_chunk = DN_ATOMS;
    if (lds_cells) *lds_cells = DN_LDS_CELLS;
    return MOLAR_HIP_OK;
}

int molar_hip_density(molar_hip_ctx *c, const float *frames, size_t nframes, size_t frame_stride, size_t natoms, const uint64_t *idx, size_t n,
                      const float *weight, const uint32_t *labels, size_t ngroups, const float *boxes, size_t box_stride, uint8_t pbc,
                      const molar_hip_density_grid *grid, const uint64_t *centre_idx, size_t ncentre, const float *centre_weight, float *density,
                      uint64_t *count, uint64_t *outside, float *centre, float *binvol, int32_t *weight_scale_log2) {
    return density_run<float>(c, "density", frames, nframes, frame_stride, natoms, idx, n, weight, labels, ngroups, boxes, box_stride, pbc, grid, centre_idx,
                              ncentre, centre_weight, density, count, outside, centre, binvol, weight_scale_log2);
}

int molar_hip_density_f64(molar_hip_ctx *c, const double *frames, size_t nframes, size_t frame_stride, size_t natoms, const uint64_t *idx, size_t n,
                          const double *weight, const uint32_t *labels, size_t ngroups, const double *boxes, size_t box_stride, uint8_t pbc,
                          const molar_hip_density_grid *grid, const uint64_t *centre_idx, size_t ncentre, const double *centre_weight, double *density,
                          uint64_t *count, uint64_t *outside, double *centre, double *binvol, int32_t *weight_scale_log2) {
    return density_run<double>(c, "density_f64", frames, nframes, frame_stride, natoms, idx, n, weight, labels, ngroups, boxes, box_stride, pbc, grid,
                               centre_idx, ncentre, centre_weight, density, count, outside, centre, binvol, weight_scale_log2);
}

}  // extern "C"
