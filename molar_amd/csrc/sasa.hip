// sasa.hip - per-atom solvent-accessible surface area by Shrake-Rupley, fused: the neighbour filter and the point test of an
// atom run in one wave, and the pair list never goes through memory.  The definition (include/molar_hip.h) fixes
// every floating-point operation of the two compares, so the exposed-point counts are integers a CPU restatement reproduces.
//
//   bounds -> grid parameters -> cell keys + counts -> stable sort by cell -> records {x, y, z, R} in cell order
//          -> sasa_kernel (one wave per atom) -> fixed-order sum of the per-workgroup partial areas (sasa_sum_kernel)
//
// Everything, the grid's shape included, is decided on the device: a call enqueues and waits once, and the frames form
// queues frame after frame without a host round trip.  The grid only has to hand the kernel a superset of the neighbours
// (the kernel applies the definition's filter itself), so its arithmetic is double for both precisions and its edge carries
// a margin for the roundings of the bounds.
#include <algorithm>
#include <cmath>
#include <vector>

#include "common.hpp"
#include "stages.hpp"

using namespace mh;

struct molar_hip_sasa_state {
    DevBuf in_xyz, in_idx, in_vdw;                   // host inputs staged here
    DevBuf table[2];                                 // the point table, f32 / f64
    uint32_t table_np[2] = {0, 0};
    std::vector<double> h_table;                     // host side of the last table upload
    std::vector<float> h_table32;
    DevBuf bounds, gridp, err;                       // 7 ordered words; GridP; 1 word
    DevBuf key_in, key_out, val_in, val_out, cub_tmp;
    DevBuf cell_count, cell_start;                   // u32 [cap + 2]
    DevBuf rec;                                      // {x, y, z, R} per atom in cell order
    DevBuf partials, totals;                         // double per workgroup; double per frame
    DevBuf vpartials, vtotals;                       // the same for the volumes
    DevBuf out_areas, out_exposed, out_volumes;      // results of calls whose destinations are host memory
};

namespace {

constexpr uint32_t SASA_WAVES = 4;                   // atoms per workgroup
constexpr uint32_t SASA_CHUNK = 256;                 // neighbour entries a wave holds in LDS between two point passes
constexpr uint32_t SASA_MAX_POINTS = 4096;           // 64 lanes x 64 mask bits
constexpr uint32_t AXIS_CAP = 1024;                  // cells per axis
constexpr int SASA_VOL_Q = 4;                        // points per lane whose intervals the volume variant holds in registers

struct GridP {
    double lo[3];
    double inv_edge;
    uint32_t dims[3];
    uint32_t ncells;
};

template <class Real> struct Real4T;
template <> struct Real4T<float> { using type = float4; };
template <> struct Real4T<double> { using type = double4; };

// monotone map of finite floats onto unsigned words, 0 below every one of them
__host__ __device__ __forceinline__ uint32_t ord_of(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__host__ __device__ __forceinline__ float ord_back(uint32_t o) {
    const uint32_t u = (o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o;
    float f;
    memcpy(&f, &u, 4);
    return f;
}

template <class Real>
struct SasaIn {
    const Real *xyz;          // this frame
    const uint64_t *idx;      // or null: atoms 0 .. n-1
    const Real *vdw;          // n, selection order
    Real probe;
    uint32_t n;
    uint64_t natoms;
};

// position and radius of selected atom k; false: the atom takes no part (non-finite, R <= 0, index out of range)
template <class Real>
__device__ __forceinline__ bool load_atom(const SasaIn<Real> &S, uint32_t k, Real &x, Real &y, Real &z, Real &R, uint32_t *err) {
    const uint64_t a = S.idx ? S.idx[k] : (uint64_t)k;
    if (a >= S.natoms) {
        *err = 1u;
        return false;
    }
    x = S.xyz[3 * a];
    y = S.xyz[3 * a + 1];
    z = S.xyz[3 * a + 2];
    R = S.vdw[k] + S.probe;
    return isfinite(x) && isfinite(y) && isfinite(z) && isfinite(R) && R > (Real)0;
}

// bounds[0..2]: largest ord(-x), bounds[3..5]: largest ord(x), bounds[6]: largest ord(R); all zero before the launch
template <class Real>
__global__ void __launch_bounds__(256) sasa_bounds_kernel(SasaIn<Real> S, uint32_t *__restrict__ bounds, uint32_t *__restrict__ err) {
    uint32_t m[7] = {0, 0, 0, 0, 0, 0, 0};
    for (uint32_t k = blockIdx.x * 256u + threadIdx.x; k < S.n; k += gridDim.x * 256u) {
        Real x, y, z, R;
        if (!load_atom(S, k, x, y, z, R, err)) continue;
        // a double that overflows float becomes an infinity here: the bound stays a bound
        const float f[3] = {(float)x, (float)y, (float)z};
        for (int d = 0; d < 3; ++d) {
            m[d] = max(m[d], ord_of(-f[d]));
            m[3 + d] = max(m[3 + d], ord_of(f[d]));
        }
        m[6] = max(m[6], ord_of((float)R));
    }
    __shared__ uint32_t sh[4][7];
    for (int v = 0; v < 7; ++v) {
        uint32_t w = m[v];
        for (int off = 32; off > 0; off >>= 1) w = max(w, (uint32_t)__shfl_xor((int)w, off, 64));
        if ((threadIdx.x & 63u) == 0) sh[threadIdx.x >> 6][v] = w;
    }
    __syncthreads();
    if (threadIdx.x < 7u) {                          // seven atomics per workgroup
        const uint32_t w = max(max(sh[0][threadIdx.x], sh[1][threadIdx.x]), max(sh[2][threadIdx.x], sh[3][threadIdx.x]));
        if (w) atomicMax(&bounds[threadIdx.x], w);
    }
}

// One thread: the grid over the bounding box.  Edge >= 2 max R, widened by 2^-10 of itself for the rounding of the cell
// coordinate (at most AXIS_CAP cells per axis) and by 2^-20 of the largest coordinate for the float bounds; then enlarged
// until the grid has at most `cap` cells.
__global__ void sasa_grid_kernel(const uint32_t *__restrict__ bounds, uint32_t cap, GridP *__restrict__ G) {
    GridP g;
    g.lo[0] = g.lo[1] = g.lo[2] = 0.0;
    g.inv_edge = 0.0;
    g.dims[0] = g.dims[1] = g.dims[2] = 1u;
    g.ncells = 1u;
    if (bounds[6] != 0u) {
        double ext[3], maxabs = 0.0, extmax = 0.0;
        for (int d = 0; d < 3; ++d) {
            double lo = -(double)ord_back(bounds[d]), hi = (double)ord_back(bounds[3 + d]);
            // coordinates beyond float's range: bin them all at the rim (the filter in the kernel still decides)
            lo = fmax(lo, -3.0e38);
            hi = fmin(hi, 3.0e38);
            g.lo[d] = lo;
            ext[d] = hi - lo;
            extmax = fmax(extmax, ext[d]);
            maxabs = fmax(maxabs, fmax(fabs(lo), fabs(hi)));
        }
        double maxR = (double)ord_back(bounds[6]);
        maxR = fmin(maxR, 3.0e38);
        double edge = 2.0 * maxR * (1.0 + 0x1p-10) + maxabs * 0x1p-20;
        edge = fmax(edge, extmax / (double)(AXIS_CAP - 1u));
        for (int it = 0; it < 200; ++it) {
            unsigned long long prod = 1ull;
            for (int d = 0; d < 3; ++d) {
                const double c = floor(ext[d] / edge) + 1.0;
                g.dims[d] = (uint32_t)fmin(c, (double)AXIS_CAP);
                prod *= g.dims[d];
            }
            if (prod <= (unsigned long long)cap) {
                g.ncells = (uint32_t)prod;
                break;
            }
            edge *= 1.26;
            if (it == 199) {                       // not reached (1.26^199 * AXIS_CAP^-3 cells); one cell is always right
                g.dims[0] = g.dims[1] = g.dims[2] = 1u;
                g.ncells = 1u;
            }
        }
        g.inv_edge = 1.0 / edge;
    }
    *G = g;
}

__device__ __forceinline__ uint32_t cell_axis(double x, double lo, double inv_edge, uint32_t dim) {
    const double c = floor((x - lo) * inv_edge);
    if (!(c > 0.0)) return 0u;
    return c >= (double)dim ? dim - 1u : (uint32_t)c;
}

// key: the atom's cell, or `cap` for an atom that takes no part (sorted behind every cell); counts per key
template <class Real>
__global__ void __launch_bounds__(256) sasa_assign_kernel(SasaIn<Real> S, const GridP *__restrict__ Gp, uint32_t cap, uint32_t *__restrict__ key,
                                                          uint32_t *__restrict__ val, uint32_t *__restrict__ cell_count, uint32_t *__restrict__ err) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= S.n) return;
    const GridP G = *Gp;
    Real x, y, z, R;
    uint32_t cell = cap;
    if (load_atom(S, k, x, y, z, R, err)) {
        const uint32_t cx = cell_axis((double)x, G.lo[0], G.inv_edge, G.dims[0]);
        const uint32_t cy = cell_axis((double)y, G.lo[1], G.inv_edge, G.dims[1]);
        const uint32_t cz = cell_axis((double)z, G.lo[2], G.inv_edge, G.dims[2]);
        cell = (cz * G.dims[1] + cy) * G.dims[0] + cx;
    }
    key[k] = cell;
    val[k] = k;
    atomicAdd(&cell_count[cell], 1u);
}

// records in cell order; the atoms that take no part get their zeros here
template <class Real>
__global__ void __launch_bounds__(256) sasa_gather_kernel(SasaIn<Real> S, uint32_t cap, const uint32_t *__restrict__ key_sorted,
                                                          const uint32_t *__restrict__ val_sorted, typename Real4T<Real>::type *__restrict__ rec,
                                                          Real *__restrict__ areas, uint32_t *__restrict__ exposed) {
    const uint32_t s = blockIdx.x * 256u + threadIdx.x;
    if (s >= S.n) return;
    const uint32_t k = val_sorted[s];
    typename Real4T<Real>::type r;
    r.x = r.y = r.z = r.w = (Real)0;
    if (key_sorted[s] < cap) {
        const uint64_t a = S.idx ? S.idx[k] : (uint64_t)k;
        r.x = S.xyz[3 * a];
        r.y = S.xyz[3 * a + 1];
        r.z = S.xyz[3 * a + 2];
        r.w = S.vdw[k] + S.probe;
    } else {
        areas[k] = (Real)0;
        if (exposed) exposed[k] = 0u;
    }
    rec[s] = r;
}

// Points lane + 64 q of the wave's atom against the `count` entries {d, R_j^2} of its LDS chunk; bit q of `buried` is the
// point's state and is carried from chunk to chunk.  R_i * u_k does not depend on the neighbour and is formed once per
// point and chunk (the same multiplication, so the same value).  The entries are read four at a time so that their LDS
// reads are in flight together; the chunk is padded to a multiple of four with entries that bury nothing (R_j^2 = -1).
template <class Real>
__device__ __forceinline__ bool sasa_buries(const typename Real4T<Real>::type &nb, Real ax, Real ay, Real az) {
    const Real tx = ax - nb.x, ty = ay - nb.y, tz = az - nb.z;
    return (tx * tx + ty * ty) + tz * tz < nb.w;
}

template <class Real>
__device__ __forceinline__ void sasa_points_pass(typename Real4T<Real>::type *chunk, uint32_t count, const Real *__restrict__ table,
                                                 uint32_t npoints, uint32_t lane, Real Ri, unsigned long long &buried) {
    if (lane < 3u) {
        typename Real4T<Real>::type pad;
        pad.x = pad.y = pad.z = (Real)0;
        pad.w = (Real)-1;
        chunk[count + lane] = pad;
    }
    __builtin_amdgcn_wave_barrier();
    for (uint32_t q = 0, p = lane; q * 64u < npoints; ++q, p += 64u) {
        bool b = p >= npoints || ((buried >> q) & 1ull);
        if (__all(b)) continue;
        Real ax = (Real)0, ay = (Real)0, az = (Real)0;
        if (!b) {
            ax = Ri * table[3 * p];
            ay = Ri * table[3 * p + 1];
            az = Ri * table[3 * p + 2];
        }
        for (uint32_t e = 0; e < count; e += 4u) {
            // one address per read for the whole wave: LDS broadcasts
            const typename Real4T<Real>::type n0 = chunk[e], n1 = chunk[e + 1u], n2 = chunk[e + 2u], n3 = chunk[e + 3u];
            const bool h = sasa_buries<Real>(n0, ax, ay, az) | sasa_buries<Real>(n1, ax, ay, az) | sasa_buries<Real>(n2, ax, ay, az) |
                           sasa_buries<Real>(n3, ax, ay, az);
            b = b | h;
            if (__all(b)) break;
        }
        if (b && p < npoints) buried |= 1ull << q;
    }
}

// The volume variant's point work: a batch of SASA_VOL_Q points of the lane (directions u, surface points a = R_i u, the
// rays' intervals [lo, hi]) against the `count` entries of the chunk.  Per entry the radical plane's offset c once, then
// per point the burial compare of the areas (bit q of `bur`) and the cut of the ray's interval at t = c / (u . d); the
// definition's three cases.
template <class Real>
struct SasaVolBatch {
    Real u[SASA_VOL_Q][3], a[SASA_VOL_Q][3], lo[SASA_VOL_Q], hi[SASA_VOL_Q];
    uint32_t bur;
};

template <class Real>
__device__ __forceinline__ void sasa_vol_pass(const typename Real4T<Real>::type *chunk, uint32_t count, Real Ri2, uint32_t live, SasaVolBatch<Real> &B) {
    for (uint32_t e = 0; e < count; ++e) {
        const typename Real4T<Real>::type nb = chunk[e];            // one address for the whole wave: LDS broadcasts
        const Real dd = (nb.x * nb.x + nb.y * nb.y) + nb.z * nb.z;
        const Real c = ((dd + Ri2) - nb.w) * (Real)0.5;
#pragma unroll
        for (int q = 0; q < SASA_VOL_Q; ++q) {
            if ((uint32_t)q >= live) break;                           // wave-uniform: slots past the table's last q do no work
            B.bur |= (uint32_t)sasa_buries<Real>(nb, B.a[q][0], B.a[q][1], B.a[q][2]) << q;
            const Real al = (B.u[q][0] * nb.x + B.u[q][1] * nb.y) + B.u[q][2] * nb.z;
            const Real t = c / al;
            // selects, no branches: the lanes of a wave take different cases at every entry
            const Real hi = B.hi[q], lo = B.lo[q];
            B.hi[q] = ((al > (Real)0) & (t < hi)) ? t : (((al == (Real)0) & (c < (Real)0)) ? (Real)0 : hi);
            B.lo[q] = ((al < (Real)0) & (t > lo)) ? t : lo;
        }
    }
}

// One wave per atom.  WithVol = false: the exposed-point counts and areas.  WithVol = true: the same counts and areas (the
// same compares, so the same bits) and the volume of the atom's ball inside its power cell.  The volume variant cannot
// leave when every point is buried (a buried point still carries volume) and cannot keep the intervals of 64 points per
// lane, so it takes the points in batches of SASA_VOL_Q per lane with their intervals in registers, each batch against
// every neighbour: the chunk is read again per batch, and the cells are walked again per batch only for an atom whose
// neighbours overflowed the chunk.
template <class Real, bool WithVol>
__global__ void __launch_bounds__(64 * SASA_WAVES) sasa_kernel(const typename Real4T<Real>::type *__restrict__ rec, const uint32_t *__restrict__ key_sorted,
                                                               const uint32_t *__restrict__ val_sorted, const uint32_t *__restrict__ cell_start,
                                                               const GridP *__restrict__ Gp, uint32_t cap, uint32_t n, const Real *__restrict__ table,
                                                               uint32_t npoints, Real *__restrict__ areas, uint32_t *__restrict__ exposed,
                                                               double *__restrict__ partials, Real *__restrict__ volumes,
                                                               double *__restrict__ vpartials) {
    using R4 = typename Real4T<Real>::type;
    __shared__ R4 chunks[SASA_WAVES][SASA_CHUNK + 4];           // + the pad of sasa_points_pass
    __shared__ double wave_area[SASA_WAVES];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t s = blockIdx.x * SASA_WAVES + wave;
    double area_d = 0.0, vol_d = 0.0;
    // wave-uniform: the atoms that take part come first in cell order
    if (s < n && key_sorted[s] < cap) {
        R4 *chunk = chunks[wave];
        const uint32_t dx = Gp->dims[0], dy = Gp->dims[1], dz = Gp->dims[2];
        const uint32_t cell = key_sorted[s];
        const uint32_t cx = cell % dx, cy = (cell / dx) % dy, cz = cell / (dx * dy);
        const R4 me = rec[s];
        const Real Ri = me.w;
        // points this lane owns: lane + 64 q < npoints
        const uint32_t mine = npoints > lane ? (npoints - lane + 63u) / 64u : 0u;
        const unsigned long long full = mine >= 64u ? ~0ull : ((1ull << mine) - 1ull);
        unsigned long long buried = 0ull;
        double vsum = 0.0;
        // One nest for both variants.  The area variant runs it once and leaves when every point is buried; the volume variant
        // runs the part from the batch's set-up to its sums once per batch of points, the walk over the cells again only
        // while the neighbours do not fit the chunk (`fits`: later batches read the chunk as the first walk left it).
        const Real Ri2 = Ri * Ri;
        uint32_t count = 0, q0 = 0;
        bool done = false, fits = false;
        do {
            SasaVolBatch<Real> B;
            uint32_t flushes = 0u;
            const uint32_t live = min((uint32_t)SASA_VOL_Q, (npoints + 63u) / 64u - q0);      // slots of this batch that hold points
            if constexpr (WithVol) {
#pragma unroll
                for (int q = 0; q < SASA_VOL_Q; ++q) {
                    const uint32_t p = lane + 64u * (q0 + (uint32_t)q);
#pragma unroll
                    for (int d = 0; d < 3; ++d) {
                        B.u[q][d] = p < npoints ? table[3u * p + (uint32_t)d] : (Real)0;
                        B.a[q][d] = Ri * B.u[q][d];
                    }
                    B.lo[q] = (Real)0;
                    B.hi[q] = Ri;
                }
                B.bur = 0u;
                // a batch that walks the cells starts with an empty chunk; once the first walk has shown that every neighbour
                // fits (`fits`), no later batch walks: `count` and the chunk's entries stay as that walk left them
                if (!fits) count = 0;
                __builtin_amdgcn_wave_barrier();
            }
            const uint32_t x0 = cx > 0u ? cx - 1u : 0u, x1 = cx + 1u < dx ? cx + 1u : dx - 1u;
            for (uint32_t zz = (cz > 0u ? cz - 1u : 0u); zz <= (cz + 1u < dz ? cz + 1u : dz - 1u) && !done && !fits; ++zz) {
                for (uint32_t yy = (cy > 0u ? cy - 1u : 0u); yy <= (cy + 1u < dy ? cy + 1u : dy - 1u) && !done; ++yy) {
                    const uint32_t row = (zz * dy + yy) * dx;
                    const uint32_t t0 = cell_start[row + x0], t1 = cell_start[row + x1 + 1u];      // cells of one row are contiguous
                    for (uint32_t base = t0; base < t1; base += 64u) {
                        if (count + 64u > SASA_CHUNK) {
                            __builtin_amdgcn_wave_barrier();
                            if constexpr (WithVol) {
                                sasa_vol_pass<Real>(chunk, count, Ri2, live, B);
                                ++flushes;
                            } else {
                                sasa_points_pass<Real>(chunk, count, table, npoints, lane, Ri, buried);
                            }
                            __builtin_amdgcn_wave_barrier();
                            count = 0;
                            if constexpr (!WithVol) {
                                if (__all(buried == full)) {
                                    done = true;
                                    break;
                                }
                            }
                        }
                        const uint32_t t = base + lane;
                        bool hit = false;
                        R4 ent;
                        ent.x = ent.y = ent.z = ent.w = (Real)0;
                        if (t < t1 && t != s) {
                            const R4 o = rec[t];
                            const Real ddx = o.x - me.x, ddy = o.y - me.y, ddz = o.z - me.z;
                            const Real d2 = (ddx * ddx + ddy * ddy) + ddz * ddz;
                            const Real lim = Ri + o.w;
                            hit = d2 < lim * lim;
                            ent.x = ddx;
                            ent.y = ddy;
                            ent.z = ddz;
                            ent.w = o.w * o.w;
                        }
                        const unsigned long long mask = __builtin_amdgcn_ballot_w64(hit);
                        if (hit) {
                            const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
                            chunk[count + rank] = ent;
                        }
                        count += (uint32_t)__builtin_popcountll(mask);
                    }
                }
            }
            if (!done && count) {
                __builtin_amdgcn_wave_barrier();
                if constexpr (WithVol)
                    sasa_vol_pass<Real>(chunk, count, Ri2, live, B);
                else
                    sasa_points_pass<Real>(chunk, count, table, npoints, lane, Ri, buried);
            }
            if constexpr (WithVol) {
                if (q0 == 0u) fits = flushes == 0u;
#pragma unroll
                for (int q = 0; q < SASA_VOL_Q; ++q) {
                    // a point past the table has u = 0: its interval stays [0, R_i] or becomes [0, 0], its bit falls outside `full`
                    const bool own = lane + 64u * (q0 + (uint32_t)q) < npoints;
                    const double h = (double)(B.hi[q] < B.lo[q] ? B.lo[q] : B.hi[q]), l = (double)B.lo[q];
                    vsum += own ? (h * h) * h - (l * l) * l : 0.0;
                    buried |= (unsigned long long)((B.bur >> q) & 1u) << (q0 + (uint32_t)q);
                }
                q0 += (uint32_t)SASA_VOL_Q;
            }
        } while (WithVol && q0 * 64u < npoints);
        uint32_t ex = mine - (uint32_t)__builtin_popcountll(buried & full);
        for (int off = 32; off > 0; off >>= 1) ex += (uint32_t)__shfl_xor((int)ex, off, 64);
        if constexpr (WithVol)
            for (int off = 32; off > 0; off >>= 1) vsum += __shfl_xor(vsum, off, 64);
        if (lane == 0) {
            const double Rd = (double)Ri;
            const Real a = (Real)((((4.0 * 3.14159265358979323846) * (Rd * Rd)) * (double)ex) / (double)npoints);
            const uint32_t k = val_sorted[s];
            areas[k] = a;
            if (exposed) exposed[k] = ex;
            area_d = (double)a;
            if constexpr (WithVol) {
                const Real v = (Real)(((((4.0 * 3.14159265358979323846) / 3.0) * vsum)) / (double)npoints);
                volumes[k] = v;
                vol_d = (double)v;
            }
        }
    } else if constexpr (WithVol) {
        // an atom that takes no part: its area and count were zeroed with the records
        if (s < n && lane == 0) volumes[val_sorted[s]] = (Real)0;
    }
    if (lane == 0) wave_area[wave] = area_d;
    if constexpr (WithVol) {
        __shared__ double wave_vol[SASA_WAVES];
        if (lane == 0) wave_vol[wave] = vol_d;
        __syncthreads();
        if (threadIdx.x == 64) {
            double sum = 0.0;
            for (uint32_t w = 0; w < SASA_WAVES; ++w) sum += wave_vol[w];
            vpartials[blockIdx.x] = sum;
        }
    } else {
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        double sum = 0.0;
        for (uint32_t w = 0; w < SASA_WAVES; ++w) sum += wave_area[w];
        partials[blockIdx.x] = sum;
    }
}

// workgroup b adds in[4096 b .. 4096 b + 4095]: thread t takes t, t + 256, ... in that order, then a fixed tree.  Applied level
// by level until one value is left, so the total's summation order depends on the launch geometry alone.
constexpr uint32_t SUM_SPAN = 4096;
__global__ void __launch_bounds__(256) sasa_sum_kernel(const double *__restrict__ in, uint32_t count, double *__restrict__ out) {
    __shared__ double sh[256];
    const uint32_t base = blockIdx.x * SUM_SPAN + threadIdx.x;
    double sum = 0.0;
#pragma unroll
    for (uint32_t k = 0; k < SUM_SPAN / 256u; ++k) {
        const uint32_t i = base + k * 256u;
        sum += i < count ? in[i] : 0.0;
    }
    sh[threadIdx.x] = sum;
    __syncthreads();
    for (uint32_t w = 128u; w > 0u; w >>= 1) {
        if (threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = sh[0];
}

// u_k on the host in double (the definition's formula)
void sasa_table(uint32_t npoints, double *out) {
    const double golden = 3.14159265358979323846 * (3.0 - std::sqrt(5.0));
    for (uint32_t k = 0; k < npoints; ++k) {
        const double z = 1.0 - (double)(2u * k + 1u) / (double)npoints;
        const double r = std::sqrt(1.0 - z * z);
        const double phi = (double)k * golden;
        out[3 * k] = r * std::cos(phi);
        out[3 * k + 1] = r * std::sin(phi);
        out[3 * k + 2] = z;
    }
}

int check_npoints(const char *who, uint32_t npoints) {
    if (npoints < 1u || npoints > SASA_MAX_POINTS)
        return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: npoints %u outside 1..%u", who, npoints, SASA_MAX_POINTS);
    return 0;
}

template <class Real>
int ensure_table(molar_hip_ctx *c, molar_hip_sasa_state &Z, uint32_t npoints, const Real **out) {
    const int w = sizeof(Real) == 8 ? 1 : 0;
    if (Z.table_np[w] != npoints) {
        MH_HIP(hipStreamSynchronize(c->stream));      // the host vectors below may still feed an earlier upload
        Z.table_np[w] = 0;
        Z.h_table.resize((size_t)npoints * 3);
        sasa_table(npoints, Z.h_table.data());
        MH_TRY(Z.table[w].reserve((size_t)npoints * 3 * sizeof(Real)));
        const void *src = Z.h_table.data();
        if (w == 0) {
            Z.h_table32.assign(Z.h_table.begin(), Z.h_table.end());
            src = Z.h_table32.data();
        }
        MH_HIP(hipMemcpyAsync(Z.table[w].p, src, (size_t)npoints * 3 * sizeof(Real), hipMemcpyHostToDevice, c->stream));
        MH_HIP(hipStreamSynchronize(c->stream));
        Z.table_np[w] = npoints;
    }
    *out = Z.table[w].as<Real>();
    return 0;
}

// results to where the caller wants them: device destinations were written in place
int copy_out(molar_hip_ctx *c, void *dst, const void *src_dev, size_t bytes) {
    if (!dst || !bytes || dst == src_dev) return 0;
    MH_HIP(hipMemcpyAsync(dst, src_dev, bytes, is_device_ptr(dst) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c->stream));
    return 0;
}

template <class Real>
int sasa_run(molar_hip_ctx *c, const char *who, const Real *frames, size_t nframes, size_t frame_stride, size_t natoms, const uint64_t *idx,
             size_t n, const Real *vdw, Real probe, uint32_t npoints, Real *areas, uint32_t *exposed, double *totals, bool with_vol = false,
             Real *volumes = nullptr, double *vtotals = nullptr) {
    MH_CTX(c);
    MH_TRY(check_npoints(who, npoints));
    if (!(probe >= (Real)0) || !std::isfinite(probe)) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: probe radius %g is negative or not finite", who, (double)probe);
    if (!idx && n > natoms) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: n = %zu exceeds natoms = %zu and there is no index", who, n, natoms);
    const size_t nsel = idx ? n : (n ? n : natoms);
    if (nsel >= 0x7FFFFFFFull) return fail(MOLAR_HIP_ERR_TOO_LARGE, "%s: selection too large (%zu atoms)", who, nsel);
    if (nframes > 1 && frame_stride < natoms * 3) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: frame_stride %zu is below 3 * natoms", who, frame_stride);
    if (nframes == 0) return MOLAR_HIP_OK;
    if (!c->sasa) c->sasa = new molar_hip_sasa_state;
    molar_hip_sasa_state &Z = *c->sasa;
    MH_TRY(Z.totals.reserve(nframes * 8 + 8));
    if (with_vol) MH_TRY(Z.vtotals.reserve(nframes * 8 + 8));
    if (nsel == 0) {
        MH_HIP(hipMemsetAsync(Z.totals.p, 0, nframes * 8, c->stream));
        MH_TRY(copy_out(c, totals, Z.totals.p, nframes * 8));
        if (with_vol) MH_TRY(copy_out(c, vtotals, Z.totals.p, nframes * 8));
        MH_HIP(hipStreamSynchronize(c->stream));
        return MOLAR_HIP_OK;
    }
    if (!frames || !vdw) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: coordinates or radii pointer is null", who);
    const uint32_t ns = (uint32_t)nsel;
    const Real *table = nullptr;
    MH_TRY(ensure_table<Real>(c, Z, npoints, &table));

    SasaIn<Real> S{};
    const Real *d_frames = nullptr;
    MH_TRY(to_device(c, frames, (nframes - 1) * frame_stride + natoms * 3, Z.in_xyz, &d_frames));
    MH_TRY(to_device(c, idx, idx ? n : 0, Z.in_idx, &S.idx));
    MH_TRY(to_device(c, vdw, nsel, Z.in_vdw, &S.vdw));
    S.probe = probe;
    S.n = ns;
    S.natoms = natoms;

    // at most `cap` cells: twice the atoms; keys 0 .. cap
    const uint32_t cap = ns < 32u ? 64u : (ns > (1u << 24) ? (1u << 25) : 2u * ns);
    int end_bit = 1;
    while (end_bit < 32 && ((unsigned long long)cap >> end_bit)) ++end_bit;
    const uint32_t nblocks = (ns + SASA_WAVES - 1u) / SASA_WAVES, nb256 = (ns + 255u) / 256u;
    MH_TRY(Z.bounds.reserve(32));
    MH_TRY(Z.gridp.reserve(sizeof(GridP)));
    MH_TRY(Z.err.reserve(8));
    MH_TRY(Z.key_in.reserve((size_t)ns * 4));
    MH_TRY(Z.key_out.reserve((size_t)ns * 4));
    MH_TRY(Z.val_in.reserve((size_t)ns * 4));
    MH_TRY(Z.val_out.reserve((size_t)ns * 4));
    MH_TRY(Z.cell_count.reserve(((size_t)cap + 2) * 4));
    MH_TRY(Z.cell_start.reserve(((size_t)cap + 2) * 4));
    MH_TRY(Z.rec.reserve((size_t)ns * 4 * sizeof(Real)));
    // the workgroups' partial areas, and behind them the levels of their sum
    const uint32_t nlevel1 = (nblocks + SUM_SPAN - 1u) / SUM_SPAN;
    const size_t partials_bytes = ((size_t)nblocks + nlevel1 + nlevel1 / SUM_SPAN + 4) * 8;
    MH_TRY(Z.partials.reserve(partials_bytes));
    if (with_vol) MH_TRY(Z.vpartials.reserve(partials_bytes));
    // results: straight into device destinations, through the state's buffers otherwise
    const bool areas_dev = areas && is_device_ptr(areas), exposed_dev = exposed && is_device_ptr(exposed);
    Real *d_areas = areas;
    if (!areas_dev) {
        MH_TRY(Z.out_areas.reserve((areas ? nframes : 1) * (size_t)ns * sizeof(Real)));
        d_areas = Z.out_areas.as<Real>();
    }
    uint32_t *d_exposed = exposed;
    if (exposed && !exposed_dev) {
        MH_TRY(Z.out_exposed.reserve((size_t)ns * 4));
        d_exposed = Z.out_exposed.as<uint32_t>();
    }
    const bool volumes_dev = volumes && is_device_ptr(volumes);
    Real *d_volumes = volumes;
    if (with_vol && !volumes_dev) {
        MH_TRY(Z.out_volumes.reserve((volumes ? nframes : 1) * (size_t)ns * sizeof(Real)));
        d_volumes = Z.out_volumes.as<Real>();
    }
    MH_HIP(hipMemsetAsync(Z.err.p, 0, 4, c->stream));
    using R4 = typename Real4T<Real>::type;
    const uint32_t nbb = std::min<uint32_t>(nb256, (uint32_t)c->num_cus * 4u);
    for (size_t f = 0; f < nframes; ++f) {
        S.xyz = d_frames + f * frame_stride;
        Real *fa = areas ? d_areas + f * (size_t)ns : d_areas;
        MH_HIP(hipMemsetAsync(Z.bounds.p, 0, 32, c->stream));
        MH_HIP(hipMemsetAsync(Z.cell_count.p, 0, ((size_t)cap + 2) * 4, c->stream));
        hipLaunchKernelGGL(sasa_bounds_kernel<Real>, dim3(nbb), dim3(256), 0, c->stream, S, Z.bounds.as<uint32_t>(), Z.err.as<uint32_t>());
        hipLaunchKernelGGL(sasa_grid_kernel, dim3(1), dim3(1), 0, c->stream, Z.bounds.as<uint32_t>(), cap, Z.gridp.as<GridP>());
        hipLaunchKernelGGL(sasa_assign_kernel<Real>, dim3(nb256), dim3(256), 0, c->stream, S, Z.gridp.as<GridP>(), cap, Z.key_in.as<uint32_t>(),
                           Z.val_in.as<uint32_t>(), Z.cell_count.as<uint32_t>(), Z.err.as<uint32_t>());
        MH_TRY(device_sort_pairs_u32(c->stream, Z.cub_tmp, Z.key_in.as<uint32_t>(), Z.key_out.as<uint32_t>(), Z.val_in.as<uint32_t>(), Z.val_out.as<uint32_t>(), ns,
                                     end_bit));
        MH_TRY(device_exclusive_sum_u32(c, Z.cub_tmp, Z.cell_count.as<uint32_t>(), Z.cell_start.as<uint32_t>(), (size_t)cap + 2));
        hipLaunchKernelGGL(sasa_gather_kernel<Real>, dim3(nb256), dim3(256), 0, c->stream, S, cap, Z.key_out.as<uint32_t>(), Z.val_out.as<uint32_t>(),
                           Z.rec.as<R4>(), fa, d_exposed);
        if (with_vol) {
            Real *fv = volumes ? d_volumes + f * (size_t)ns : d_volumes;
            hipLaunchKernelGGL((sasa_kernel<Real, true>), dim3(nblocks), dim3(64 * SASA_WAVES), 0, c->stream, Z.rec.as<R4>(), Z.key_out.as<uint32_t>(),
                               Z.val_out.as<uint32_t>(), Z.cell_start.as<uint32_t>(), Z.gridp.as<GridP>(), cap, ns, table, npoints, fa, d_exposed,
                               Z.partials.as<double>(), fv, Z.vpartials.as<double>());
        } else {
            hipLaunchKernelGGL((sasa_kernel<Real, false>), dim3(nblocks), dim3(64 * SASA_WAVES), 0, c->stream, Z.rec.as<R4>(), Z.key_out.as<uint32_t>(),
                               Z.val_out.as<uint32_t>(), Z.cell_start.as<uint32_t>(), Z.gridp.as<GridP>(), cap, ns, table, npoints, fa, d_exposed,
                               Z.partials.as<double>(), (Real *)nullptr, (double *)nullptr);
        }
        // the areas' total, then the volumes': the same levels over each array of partial sums
        for (int pass = 0; pass < (with_vol ? 2 : 1); ++pass) {
            DevBuf &P = pass ? Z.vpartials : Z.partials;
            DevBuf &T = pass ? Z.vtotals : Z.totals;
            const double *src = P.as<double>();
            double *level = P.as<double>() + nblocks;
            for (uint32_t cnt = nblocks;;) {
                const uint32_t nb = (cnt + SUM_SPAN - 1u) / SUM_SPAN;
                double *dst = nb == 1u ? T.as<double>() + f : level;
                hipLaunchKernelGGL(sasa_sum_kernel, dim3(nb), dim3(256), 0, c->stream, src, cnt, dst);
                if (nb == 1u) break;
                src = dst;
                level += nb;
                cnt = nb;
            }
        }
        MH_HIP(hipGetLastError());
    }
    if (areas && !areas_dev) MH_TRY(copy_out(c, areas, d_areas, nframes * (size_t)ns * sizeof(Real)));
    if (exposed && !exposed_dev) MH_TRY(copy_out(c, exposed, d_exposed, (size_t)ns * 4));
    MH_TRY(copy_out(c, totals, Z.totals.p, nframes * 8));
    if (with_vol) {
        if (volumes && !volumes_dev) MH_TRY(copy_out(c, volumes, d_volumes, nframes * (size_t)ns * sizeof(Real)));
        MH_TRY(copy_out(c, vtotals, Z.vtotals.p, nframes * 8));
    }
    uint32_t bad_index = 0;
    MH_TRY(read_back(c, &bad_index, Z.err.p, 4));
    if (bad_index) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: a selection index is not below natoms = %zu", who, natoms);
    return MOLAR_HIP_OK;
}

template <class Real>
int sasa_points(const char *who, uint32_t npoints, Real *out_xyz) {
    MH_TRY(check_npoints(who, npoints));
    if (!out_xyz) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "%s: output pointer is null", who);
    std::vector<double> t((size_t)npoints * 3);
    sasa_table(npoints, t.data());
    for (size_t i = 0; i < t.size(); ++i) out_xyz[i] = (Real)t[i];
    return MOLAR_HIP_OK;
}

}  // namespace

namespace mh {
void sasa_release(molar_hip_ctx *c) {
    release_state(c->sasa);
}
}  // namespace mh

extern "C" {

int molar_hip_sasa_points(uint32_t npoints, float *out_xyz) { return sasa_points<float>("sasa_points", npoints, out_xyz); }

int molar_hip_sasa_points_f64(uint32_t npoints, double *out_xyz) { return sasa_points<double>("sasa_points_f64", npoints, out_xyz); }

int molar_hip_sasa(molar_hip_ctx *c, const float *xyz, size_t natoms, const uint64_t *idx, size_t n, const float *vdw, float probe,
                   uint32_t npoints, float *areas, uint32_t *exposed, double *total) {
    return sasa_run<float>(c, "sasa", xyz, 1, 0, natoms, idx, n, vdw, probe, npoints, areas, exposed, total);
}

int molar_hip_sasa_f64(molar_hip_ctx *c, const double *xyz, size_t natoms, const uint64_t *idx, size_t n, const double *vdw, double probe,
                       uint32_t npoints, double *areas, uint32_t *exposed, double *total) {
    return sasa_run<double>(c, "sasa_f64", xyz, 1, 0, natoms, idx, n, vdw, probe, npoints, areas, exposed, total);
}

int molar_hip_sasa_frames(molar_hip_ctx *c, const float *frames, size_t nframes, size_t frame_stride, size_t natoms, const uint64_t *idx,
                          size_t n, const float *vdw, float probe, uint32_t npoints, float *areas, double *totals) {
    return sasa_run<float>(c, "sasa_frames", frames, nframes, frame_stride, natoms, idx, n, vdw, probe, npoints, areas, nullptr, totals);
}

int molar_hip_sasa_vol(molar_hip_ctx *c, const float *xyz, size_t natoms, const uint64_t *idx, size_t n, const float *vdw, float probe,
                       uint32_t npoints, float *areas, uint32_t *exposed, double *total, float *volumes, double *total_volume) {
    return sasa_run<float>(c, "sasa_vol", xyz, 1, 0, natoms, idx, n, vdw, probe, npoints, areas, exposed, total, true, volumes, total_volume);
}

int molar_hip_sasa_vol_f64(molar_hip_ctx *c, const double *xyz, size_t natoms, const uint64_t *idx, size_t n, const double *vdw, double probe,
                           uint32_t npoints, double *areas, uint32_t *exposed, double *total, double *volumes, double *total_volume) {
    return sasa_run<double>(c, "sasa_vol_f64", xyz, 1, 0, natoms, idx, n, vdw, probe, npoints, areas, exposed, total, true, volumes, total_volume);
}

int molar_hip_sasa_vol_frames(molar_hip_ctx *c, const float *frames, size_t nframes, size_t frame_stride, size_t natoms, const uint64_t *idx,
                              size_t n, const float *vdw, float probe, uint32_t npoints, float *areas, double *totals, float *volumes,
                              double *total_volumes) {
    return sasa_run<float>(c, "sasa_vol_frames", frames, nframes, frame_stride, natoms, idx, n, vdw, probe, npoints, areas, nullptr, totals, true,
                           volumes, total_volumes);
}

}  // extern "C"
