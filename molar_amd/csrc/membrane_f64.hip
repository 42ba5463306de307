// membrane_f64.hip — the staged Membrane::compute (molar_membrane/src/lib.rs:410-454) for MolAR built with its `f64`
// feature (Float = f64, molar/src/aliases.rs:10-13; molar_membrane's own `f64 = ["molar/f64"]`).
//
// One iteration of Membrane::smooth (lib.rs:661-812) in double precision, with the contract of molar_hip_membrane_smooth:
//   k_membrane_fit64      one lane per lipid: local frame, patch markers into the frame (PBC shortest vector through
//                         boxmath64.hpp), 6x6 normal equations + Cholesky, Voronoi cell by half-plane clipping, curvatures,
//                         fitted normal, cell area, fitted patch points, marker moved onto the surface;
//   k_membrane_average64  one lane per lipid: the fitted images of its marker from every valid patch that contains it,
//                         added in the order of the reference's scatter loop (owner ascending, position in the patch).
// Plus the host-arithmetic twins of compute_initial_normals (lib.rs:456-505) and smooth_curvature (:584-621).
// The quadric fit is why this exists: the normal equations are poorly conditioned, and in f32 the Gaussian curvature of a
// flat-ish bilayer (~1e-3) is about as large as its own error.  Every operation is the reference's, in its order, in double,
// with no contraction (-ffp-contract=off).  The f32 kernels (membrane.hip) are untouched; the chained frame call is f32 only.
//
// LDS: a Voronoi vertex is 24 bytes here (two doubles, next, id) and a local point 32 (three doubles, id); the f32 layout
// (64 vertices + 60 points per lane, 64 lanes) would need 216 KB.  The f64 kernel keeps the same per-lane capacities
// (3456 bytes a lane) and runs 16 or 32 lanes per workgroup: 54 / 108 KB.  Patches too long for them use the lane's slices of
// `vwork` / `pwork` in HBM, as in the f32 kernel.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "boxmath64.hpp"
#include "common.hpp"
#include "stages.hpp"

namespace {

using namespace mh;

struct Vert64 {            // {x, y, ccw neighbour, id of the point that made the ccw edge}
    double x, y;
    uint32_t next;
    int32_t id;
};
struct Pt64 {              // a patch member in the lipid's local frame
    double x, y, z;
    uint32_t id, pad;
};
static_assert(sizeof(Vert64) == 24 && sizeof(Pt64) == 32, "LDS element sizes");

struct SmoothDev64 {
    uint32_t K;
    BoxD box;                  // by value (kernel arguments)
    const double *saved;       // [K][3] markers before the iteration
    double *head;              // [K][3] in/out
    double *normals;           // [K][3] in/out
    uint8_t *valid;            // [K] in/out
    const uint64_t *poff;      // [K+1]
    const uint64_t *pids;      // [E]
    double *coefs, *mean, *gauss, *pcurv, *pdirs, *area;
    uint32_t *nvert;
    uint64_t *neib;            // [E+4K]
    double *voro;              // [E+4K][3]
    double *fitted;            // [E][3]
    Vert64 *vwork;             // [E+4K] Voronoi vertices of the patches too long for LDS
    Pt64 *pwork;               // [E]    local points of those patches
    const uint32_t *rev_off;   // [K+1]  transpose of the patch CSR
    const uint32_t *rev_entry; // [E]    flat patch entry
    const uint32_t *rev_owner; // [E]    lipid owning that entry
};

__device__ __forceinline__ D3 cross(D3 a, D3 b) {
    return D3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}

// nalgebra try_inverse for 3x3 (closed form, column-major)
__device__ bool inverse3(const double *m, double *o) {
    const double m11 = m[0], m21 = m[1], m31 = m[2], m12 = m[3], m22 = m[4], m32 = m[5], m13 = m[6], m23 = m[7], m33 = m[8];
    const double mi1 = m22 * m33 - m32 * m23;
    const double mi2 = m21 * m33 - m31 * m23;
    const double mi3 = m21 * m32 - m31 * m22;
    const double det = (m11 * mi1 - m12 * mi2) + m13 * mi3;
    if (det == 0.0) return false;
    o[0] = mi1 / det;
    o[3] = (m13 * m32 - m33 * m12) / det;
    o[6] = (m12 * m23 - m22 * m13) / det;
    o[1] = -mi2 / det;
    o[4] = (m11 * m33 - m31 * m13) / det;
    o[7] = (m13 * m21 - m23 * m11) / det;
    o[2] = mi3 / det;
    o[5] = (m12 * m31 - m32 * m11) / det;
    o[8] = (m11 * m22 - m21 * m12) / det;
    return true;
}

// get_quad_coefs' solver (lib.rs:862): nalgebra Cholesky::new, then L y = b, L^T x = y.  a is column-major 6x6.
__device__ bool cholesky6_solve(double *a, double *b) {
    for (int j = 0; j < 6; ++j) {
        for (int k = 0; k < j; ++k) {
            const double factor = -a[k * 6 + j];
            for (int r = j; r < 6; ++r) a[j * 6 + r] = factor * a[k * 6 + r] + a[j * 6 + r];
        }
        const double diag = a[j * 6 + j];
        if (!(diag > 0.0)) return false;
        const double denom = __builtin_sqrt(diag);
        a[j * 6 + j] = denom;
        for (int r = j + 1; r < 6; ++r) a[j * 6 + r] /= denom;
    }
    for (int i = 0; i < 6; ++i) {
        const double coeff = b[i] / a[i * 6 + i];
        b[i] = coeff;
        for (int r = i + 1; r < 6; ++r) b[r] = (-coeff) * a[i * 6 + r] + b[r];
    }
    for (int i = 5; i >= 0; --i) {
        double dot = 0.0;
        for (int r = i + 1; r < 6; ++r) dot += a[i * 6 + r] * b[r];
        b[i] = (b[i] - dot) / a[i * 6 + i];
    }
    return true;
}

__device__ __forceinline__ double z_surf(double x, double y, const double *c) {   // lib.rs:870-879
    return ((((c[0] * x * x + c[1] * y * y) + c[2] * x * y) + c[3] * x) + c[4] * y) + c[5];
}

// a lane's vertices / points: in the workgroup's LDS, element-major (element v of lane l at [v * lanes + l]), or in the lane's
// HBM slice (stride 1)
template <class T>
struct Lane {
    T *p;
    uint32_t stride;
    __device__ __forceinline__ T &at(uint32_t i) const { return p[(size_t)i * stride]; }
};
__device__ __forceinline__ double vdist(const Lane<Vert64> &w, uint32_t i, double lx, double ly, double r2) {
    const Vert64 &q = w.at(i);
    return (lx * q.x + ly * q.y) - r2;     // line.pos.dot(pos) - r2  (voronoi_cell.rs:83-85)
}

// VoronoiCell::add_point (voronoi_cell.rs:107-205).  Returns false only where the reference would never return (no vertex on
// the inner side, e.g. NaN input) - the caller then drops the lipid.
__device__ bool voro_add_point(const Lane<Vert64> &w, uint32_t &nv, uint32_t &init, double px, double py, int32_t id) {
    const double TOL = 1e-10;
    const double lx = 0.5 * px, ly = 0.5 * py;
    const double r2 = lx * lx + ly * ly;
    uint32_t cur = init, guard = 0;
    double cur_d = vdist(w, cur, lx, ly, r2);
    while (cur_d >= TOL) {
        cur = w.at(cur).next;
        cur_d = vdist(w, cur, lx, ly, r2);
        if (++guard > nv) return false;
    }
    init = cur;
    uint32_t c1_in, c1_out, c2_in, c2_out;
    double c1_ind, c1_outd, c2_ind, c2_outd;
    for (;;) {
        const uint32_t nx = w.at(cur).next;
        if (nx == init) return true;               // every vertex is inside: nothing to cut
        const double nd = vdist(w, nx, lx, ly, r2);
        if (nd >= TOL) {
            c1_in = cur; c1_ind = cur_d; c1_out = nx; c1_outd = nd;
            cur = nx; cur_d = nd;
            break;
        }
        cur = nx; cur_d = nd;
    }
    guard = 0;
    for (;;) {
        const uint32_t nx = w.at(cur).next;
        const double nd = vdist(w, nx, lx, ly, r2);
        if (nd < TOL) {
            c2_out = cur; c2_outd = cur_d; c2_in = nx; c2_ind = nd;
            break;
        }
        cur = nx; cur_d = nd;
        if (++guard > nv) return false;
    }
    {   // cut #2 (:173-195)
        const Vert64 o = w.at(c2_out), in = w.at(c2_in);
        const double frac = c2_outd / (fabs(c2_ind) + c2_outd);
        const double x = (1.0 - frac) * o.x + frac * in.x;
        const double y = (1.0 - frac) * o.y + frac * in.y;
        if (c1_out != c2_out) {
            w.at(c2_out) = Vert64{x, y, o.next, o.id};
            w.at(c1_out).next = c2_out;
        } else {
            w.at(nv) = Vert64{x, y, c2_in, o.id};
            w.at(c1_out).next = nv;
            nv += 1;
        }
    }
    {   // cut #1 (:197-202)
        const Vert64 o = w.at(c1_out), in = w.at(c1_in);
        const double frac = c1_outd / (fabs(c1_ind) + c1_outd);
        w.at(c1_out) = Vert64{(1.0 - frac) * o.x + frac * in.x, (1.0 - frac) * o.y + frac * in.y, o.next, id};
    }
    return true;
}

// Eigenpairs of the symmetric 2x2 [[a, b], [b, c]]: descending eigenvalues, eigenvectors whose first non-zero component is
// positive (the convention of the f32 kernel; nalgebra's symmetric_eigen leaves order and sign open).
__device__ void eig2_sym(double a, double b, double c, double *w, double *v) {
    const double t = 0.5 * (a - c), m = 0.5 * (a + c);
    const double h = __builtin_sqrt(t * t + b * b);
    w[0] = m + h;
    w[1] = m - h;
    // both cases evaluated, then selected: a divergent if / else here makes the compiler put a VGPR copy ahead of an EXEC
    // restore (the pattern build.py's ISA audit refuses); the b == 0 case discards the other's values (0 / 0 included)
    double x = t >= 0.0 ? t + h : b, y = t >= 0.0 ? b : h - t;
    const double n = __builtin_sqrt(x * x + y * y);
    x /= n; y /= n;
    const bool flip = x < 0.0 || (x == 0.0 && y < 0.0);
    x = flip ? -x : x; y = flip ? -y : y;
    x = b == 0.0 ? (a >= c ? 1.0 : 0.0) : x;
    y = b == 0.0 ? (a >= c ? 0.0 : 1.0) : y;
    v[0] = x; v[1] = y;
    double x2 = -y, y2 = x;
    if (x2 < 0.0 || (x2 == 0.0 && y2 < 0.0)) { x2 = -x2; y2 = -y2; }
    v[2] = x2; v[3] = y2;
}

constexpr uint32_t VORO_LDS = 64;        // vertices per lane held in LDS
constexpr uint32_t PTS_LDS = 60;         // local points per lane held in LDS
constexpr size_t FIT64_LANE_BYTES = VORO_LDS * sizeof(Vert64) + PTS_LDS * sizeof(Pt64);      // 3456
constexpr uint32_t FIT64_MAX_LANES = 32;
constexpr size_t FIT64_LDS_BYTES = FIT64_LANE_BYTES * FIT64_MAX_LANES;                       // 108 KB
static_assert(FIT64_LDS_BYTES <= 160 * 1024, "gfx950 LDS");

__global__ __launch_bounds__(FIT64_MAX_LANES) void k_membrane_fit64(SmoothDev64 A) {
    extern __shared__ double fit64_lds[];
    const uint32_t lanes = blockDim.x;               // 16 or 32 (launch_fit64)
    const uint32_t i = blockIdx.x * lanes + threadIdx.x;
    if (i >= A.K || !A.valid[i]) return;
    const uint64_t p0 = A.poff[i];
    const uint32_t np = (uint32_t)(A.poff[i + 1] - p0);
    const uint64_t slot = p0 + 4ull * i;
    const D3 nrm = D3{A.normals[3 * i], A.normals[3 * i + 1], A.normals[3 * i + 2]};
    double to_lab[9], to_local[9];
    {   // get_to_lab_transform (lipid_molecule.rs:190-196)
        const D3 c0 = cross(nrm, D3{1.0, 0.0, 0.0});
        const D3 c1 = cross(nrm, c0);
        to_lab[0] = c0.x; to_lab[1] = c0.y; to_lab[2] = c0.z;
        to_lab[3] = c1.x; to_lab[4] = c1.y; to_lab[5] = c1.z;
        to_lab[6] = -nrm.x; to_lab[7] = -nrm.y; to_lab[8] = -nrm.z;
    }
    if (!inverse3(to_lab, to_local)) { A.valid[i] = 0; return; }
    const D3 c = D3{A.saved[3 * i], A.saved[3 * i + 1], A.saved[3 * i + 2]};
    const bool in_lds = np + 4u <= VORO_LDS && np <= PTS_LDS;
    Vert64 *lds_v = reinterpret_cast<Vert64 *>(fit64_lds);
    Pt64 *lds_p = reinterpret_cast<Pt64 *>(lds_v + (size_t)VORO_LDS * lanes);
    const Lane<Vert64> w = in_lds ? Lane<Vert64>{lds_v + threadIdx.x, lanes} : Lane<Vert64>{A.vwork + slot, 1u};
    const Lane<Pt64> pt = in_lds ? Lane<Pt64>{lds_p + threadIdx.x, lanes} : Lane<Pt64>{A.pwork + p0, 1u};
    double m[36], cf[6];
    for (int k = 0; k < 36; ++k) m[k] = 0.0;
    for (int k = 0; k < 6; ++k) cf[k] = 0.0;
    for (uint32_t q0 = 0; q0 < np; q0 += 2u) {   // local points + normal equations (lib.rs:685-689, 851-860), two gathers in flight
        uint32_t jj[2];
        D3 ss[2];
#pragma unroll
        for (uint32_t u = 0; u < 2u; ++u) jj[u] = (uint32_t)A.pids[p0 + (q0 + u < np ? q0 + u : np - 1u)];
#pragma unroll
        for (uint32_t u = 0; u < 2u; ++u) ss[u] = D3{A.saved[3 * jj[u]], A.saved[3 * jj[u] + 1], A.saved[3 * jj[u] + 2]};
        for (uint32_t u = 0; u < 2u; ++u) {
            if (q0 + u >= np) break;
            const D3 l = mat_vec(to_local, shortest_vector(A.box, ss[u] - c, MOLAR_HIP_PBC_FULL));
            pt.at(q0 + u) = Pt64{l.x, l.y, l.z, jj[u], 0u};
            const double pw[6] = {l.x * l.x, l.y * l.y, l.x * l.y, l.x, l.y, 1.0};
#pragma unroll
            for (int cc = 0; cc < 6; ++cc)
#pragma unroll
                for (int r = 0; r < 6; ++r) m[cc * 6 + r] += pw[r] * pw[cc];
#pragma unroll
            for (int r = 0; r < 6; ++r) cf[r] += pw[r] * l.z;
        }
    }
    if (!cholesky6_solve(m, cf)) { A.valid[i] = 0; return; }

    w.at(0) = Vert64{-10.0, -10.0, 1u, -1};     // VoronoiCell::new(-10, 10, -10, 10)  (voronoi_cell.rs:62-80)
    w.at(1) = Vert64{10.0, -10.0, 2u, -2};
    w.at(2) = Vert64{10.0, 10.0, 3u, -3};
    w.at(3) = Vert64{-10.0, 10.0, 0u, -4};
    uint32_t nv = 4, init = 0;
    for (uint32_t q = 0; q < np; ++q) {
        const Pt64 r = pt.at(q);
        if (!voro_add_point(w, nv, init, r.x, r.y, (int32_t)r.id)) { A.valid[i] = 0; return; }
    }
    uint32_t n_vert = 0, n_neib = 0;                 // direct neighbours (lib.rs:706-726)
    {
        uint32_t cur = init;
        do {
            const Vert64 v = w.at(cur);
            if (v.id >= 0) A.neib[slot + n_neib++] = (uint64_t)v.id;
            ++n_vert;
            cur = v.next;
        } while (cur != init);
    }
    if (n_neib < n_vert) { A.valid[i] = 0; return; }  // a wall vertex survived: open cell
    A.nvert[i] = n_vert;
#pragma unroll
    for (int k = 0; k < 6; ++k) A.coefs[6 * i + k] = cf[k];
    {   // compute_curvature_and_normal (lipid_molecule.rs:134-187)
        const double a = cf[0], b = cf[1], cq = cf[2], d = cf[3], e = cf[4];
        const double E = 1.0 + d * d, F = d * e, G = 1.0 + e * e;
        const double L = 2.0 * a, M = cq, N = 2.0 * b;
        const double Z = E * G - F * F;
        A.gauss[i] = (L * N - M * M) / Z;
        A.mean[i] = 0.5 * ((E * N - 2.0 * F * M) + G * L) / Z;
        const double gl = __builtin_sqrt((d * d + e * e) + 1.0);
        const D3 fn = mat_vec(to_lab, D3{d / gl, e / gl, -1.0 / gl});
        A.normals[3 * i] = fn.x; A.normals[3 * i + 1] = fn.y; A.normals[3 * i + 2] = fn.z;
        double ev[2], evec[4];
        eig2_sym((E * L - F * M) / Z, (G * M - F * L) / Z, (G * N - F * M) / Z, ev, evec);
        A.pcurv[2 * i] = ev[0]; A.pcurv[2 * i + 1] = ev[1];
        for (int k = 0; k < 2; ++k) {
            const D3 pd = mat_vec(to_lab, D3{evec[2 * k], evec[2 * k + 1], 0.0});
            A.pdirs[6 * i + 3 * k] = pd.x; A.pdirs[6 * i + 3 * k + 1] = pd.y; A.pdirs[6 * i + 3 * k + 2] = pd.z;
        }
    }
    {   // cell vertices on the fitted surface, lab frame, still relative to the marker; fan area (lib.rs:731-752)
        uint32_t cur = init;
        D3 first = D3{0.0, 0.0, 0.0}, prev = D3{0.0, 0.0, 0.0};
        double ar = 0.0;
        for (uint32_t k = 0; k < n_vert; ++k) {
            const Vert64 v = w.at(cur);
            const D3 p = mat_vec(to_lab, D3{v.x, v.y, z_surf(v.x, v.y, cf)});
            double *dst = A.voro + 3 * (slot + k);
            dst[0] = p.x; dst[1] = p.y; dst[2] = p.z;
            if (k == 0) first = p;
            else ar += 0.5 * __builtin_sqrt(norm2(cross(prev, p)));
            prev = p;
            cur = v.next;
        }
        ar += 0.5 * __builtin_sqrt(norm2(cross(prev, first)));
        A.area[i] = ar;
    }
    double *fp = A.fitted + 3 * p0;
    for (uint32_t q = 0; q < np; ++q) {              // fitted patch points (lib.rs:760-768)
        const Pt64 r = pt.at(q);
        const D3 s = D3{A.saved[3 * r.id], A.saved[3 * r.id + 1], A.saved[3 * r.id + 2]};
        const D3 t = mat_vec(to_lab, D3{0.0, 0.0, z_surf(r.x, r.y, cf) - r.z});
        fp[3 * q] = s.x + t.x;
        fp[3 * q + 1] = s.y + t.y;
        fp[3 * q + 2] = s.z + t.z;
    }
    if (fabs(cf[5]) > 0.5) { A.valid[i] = 0; return; }   // fitted surface too far from the marker (lib.rs:774-777)
    const D3 t = mat_vec(to_lab, D3{0.0, 0.0, cf[5]});
    A.head[3 * i] += t.x; A.head[3 * i + 1] += t.y; A.head[3 * i + 2] += t.z;
}

int launch_fit64(molar_hip_ctx *c, const SmoothDev64 &A) {
    static bool ready[64] = {};          // per device: the attribute belongs to the device's copy of the kernel
    const int dev = c->device & 63;
    if (!ready[dev]) {
        MH_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_membrane_fit64), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)FIT64_LDS_BYTES));
        ready[dev] = true;
    }
    // a wave's time is that of its slowest lane: 16 lipids to a workgroup (54 KB, two workgroups per CU) while that gives
    // every CU work, 32 (108 KB, one per CU) for larger sets
    const uint32_t cus = (uint32_t)std::max(c->num_cus, 1);
    const uint32_t lanes = A.K <= 16u * 2u * cus ? 16u : FIT64_MAX_LANES;
    hipLaunchKernelGGL(k_membrane_fit64, dim3((A.K + lanes - 1u) / lanes), dim3(lanes), FIT64_LANE_BYTES * lanes, c->stream, A);
    MH_HIP(hipGetLastError());
    return 0;
}

// lib.rs:781-809.  `fitted_head` holds the markers after k_membrane_fit64; the average is written to `head`.  The images of
// lipid i's marker are added in the reference's scatter order (rev_* lists them by owner ascending, then patch position).
__global__ __launch_bounds__(256) void k_membrane_average64(SmoothDev64 A, const double *fitted_head) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.K || !A.valid[i]) return;
    double n = 1.0;
    D3 s = D3{fitted_head[3 * i], fitted_head[3 * i + 1], fitted_head[3 * i + 2]};
    for (uint32_t r = A.rev_off[i]; r < A.rev_off[i + 1]; ++r) {
        if (!A.valid[A.rev_owner[r]]) continue;
        const double *p = A.fitted + 3ull * A.rev_entry[r];
        n += 1.0;
        s = s + D3{p[0], p[1], p[2]};
    }
    const D3 h = D3{s.x / n, s.y / n, s.z / n};
    A.head[3 * i] = h.x; A.head[3 * i + 1] = h.y; A.head[3 * i + 2] = h.z;
    const uint64_t slot = A.poff[i] + 4ull * i;
    const uint32_t nv = A.nvert[i];
    for (uint32_t k = 0; k < nv; ++k) {
        double *v = A.voro + 3 * (slot + k);
        v[0] += h.x; v[1] += h.y; v[2] += h.z;
    }
}

struct Blob {
    size_t size = 0;
    size_t take(size_t bytes) {
        const size_t at = size;
        size += (bytes + 15) & ~size_t(15);
        return at;
    }
};

}  // namespace

extern "C" int molar_hip_membrane_smooth_f64(molar_hip_ctx *c, const molar_hip_membrane_patches *P, const double *box9,
                                             molar_hip_membrane_state_f64 *S) {
    if (!c) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "null context");
    MH_HIP(hipSetDevice(c->device));
    if (!P || !S || !box9) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "membrane_smooth_f64: null argument");
    const size_t K = P->nlipids;
    if (K == 0) return MOLAR_HIP_OK;
    if (!P->patch_offsets || !S->head_markers || !S->normals || !S->valid)
        return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "membrane_smooth_f64: null array");
    if (K >= (1ull << 31)) return fail(MOLAR_HIP_ERR_TOO_LARGE, "membrane_smooth_f64: lipid ids must fit i32 (voronoi_cell.rs:17)");
    const size_t E = (size_t)P->patch_offsets[K];
    if (E && !P->patch_ids) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "membrane_smooth_f64: patch_ids missing");
    if (E >= (1ull << 32)) return fail(MOLAR_HIP_ERR_TOO_LARGE, "membrane_smooth_f64: %zu patch entries", E);
    if (P->patch_offsets[0] != 0) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "membrane_smooth_f64: patch_offsets[0] != 0");
    BoxD box;
    MH_TRY(box64_from_matrix(box9, &box));
    const size_t slots = E + 4 * K;

    // transpose of the patch CSR: for each lipid, the patch entries that point at it, ordered by
    // (owner lipid, position in the owner's patch) = the order of the reference's scatter loop
    std::vector<uint32_t> rev_off(K + 1, 0), rev_entry(E), rev_owner(E);
    for (size_t i = 0; i < K; ++i) {
        if (P->patch_offsets[i + 1] < P->patch_offsets[i]) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "membrane_smooth_f64: offsets not monotone");
        for (uint64_t q = P->patch_offsets[i]; q < P->patch_offsets[i + 1]; ++q) {
            if (P->patch_ids[q] >= K) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "membrane_smooth_f64: patch id %llu out of range", (unsigned long long)P->patch_ids[q]);
            rev_off[P->patch_ids[q] + 1]++;
        }
    }
    for (size_t i = 0; i < K; ++i) rev_off[i + 1] += rev_off[i];
    {
        std::vector<uint32_t> cursor(rev_off.begin(), rev_off.end() - 1);
        for (size_t i = 0; i < K; ++i)
            for (uint64_t q = P->patch_offsets[i]; q < P->patch_offsets[i + 1]; ++q) {
                const uint32_t at = cursor[P->patch_ids[q]]++;
                rev_entry[at] = (uint32_t)q;
                rev_owner[at] = (uint32_t)i;
            }
    }

    // one blob: [in/out state | inputs | device-only work]
    Blob L;
    const size_t o_head = L.take(K * 24), o_norm = L.take(K * 24), o_valid = L.take(K), o_coefs = L.take(K * 48),
                 o_mean = L.take(K * 8), o_gauss = L.take(K * 8), o_pcurv = L.take(K * 16), o_pdirs = L.take(K * 48),
                 o_area = L.take(K * 8), o_nvert = L.take(K * 4), o_neib = L.take(slots * 8), o_voro = L.take(slots * 24),
                 o_fitted = L.take(E * 24);
    const size_t io_bytes = L.size;
    const size_t o_poff = L.take((K + 1) * 8), o_pids = L.take(E * 8), o_roff = L.take((K + 1) * 4), o_rent = L.take(E * 4),
                 o_rown = L.take(E * 4);
    const size_t up_bytes = L.size;
    const size_t o_saved = L.take(K * 24), o_fh = L.take(K * 24), o_vwork = L.take(slots * sizeof(Vert64)),
                 o_pwork = L.take(E * sizeof(Pt64) + 32);
    MH_TRY(c->m_partials.reserve(L.size));
    MH_TRY(ensure_pinned(c, up_bytes));
    char *h = (char *)c->h_pinned, *d = c->m_partials.as<char>();
    auto put = [&](size_t off, const void *src, size_t bytes) {
        if (src) std::memcpy(h + off, src, bytes);
        else std::memset(h + off, 0, bytes);
    };
    put(o_head, S->head_markers, K * 24); put(o_norm, S->normals, K * 24); put(o_valid, S->valid, K);
    put(o_coefs, S->quad_coefs, K * 48); put(o_mean, S->mean_curv, K * 8); put(o_gauss, S->gauss_curv, K * 8);
    put(o_pcurv, S->princ_curvs, K * 16); put(o_pdirs, S->princ_dirs, K * 48); put(o_area, S->area, K * 8);
    put(o_nvert, S->nvert, K * 4); put(o_neib, S->neib_ids, slots * 8); put(o_voro, S->voro_vertexes, slots * 24);
    put(o_fitted, S->fitted_patch_points, E * 24);
    put(o_poff, P->patch_offsets, (K + 1) * 8); put(o_pids, P->patch_ids, E * 8);
    put(o_roff, rev_off.data(), (K + 1) * 4); put(o_rent, rev_entry.data(), E * 4); put(o_rown, rev_owner.data(), E * 4);
    {
        Prof span(c, 4);
        MH_HIP(hipMemcpyAsync(d, h, up_bytes, hipMemcpyHostToDevice, c->stream));
        MH_HIP(hipMemcpyAsync(d + o_saved, d + o_head, K * 24, hipMemcpyDeviceToDevice, c->stream));
        SmoothDev64 A;
        A.K = (uint32_t)K;
        A.box = box;
        A.saved = (const double *)(d + o_saved);
        A.head = (double *)(d + o_head); A.normals = (double *)(d + o_norm); A.valid = (uint8_t *)(d + o_valid);
        A.poff = (const uint64_t *)(d + o_poff); A.pids = (const uint64_t *)(d + o_pids);
        A.coefs = (double *)(d + o_coefs); A.mean = (double *)(d + o_mean); A.gauss = (double *)(d + o_gauss);
        A.pcurv = (double *)(d + o_pcurv); A.pdirs = (double *)(d + o_pdirs); A.area = (double *)(d + o_area);
        A.nvert = (uint32_t *)(d + o_nvert); A.neib = (uint64_t *)(d + o_neib); A.voro = (double *)(d + o_voro);
        A.fitted = (double *)(d + o_fitted); A.vwork = (Vert64 *)(d + o_vwork); A.pwork = (Pt64 *)(d + o_pwork);
        A.rev_off = (const uint32_t *)(d + o_roff); A.rev_entry = (const uint32_t *)(d + o_rent);
        A.rev_owner = (const uint32_t *)(d + o_rown);
        MH_TRY(launch_fit64(c, A));
        MH_HIP(hipMemcpyAsync(d + o_fh, d + o_head, K * 24, hipMemcpyDeviceToDevice, c->stream));
        hipLaunchKernelGGL(k_membrane_average64, dim3((uint32_t)((K + 255) / 256)), dim3(256), 0, c->stream, A,
                           (const double *)(d + o_fh));
        MH_HIP(hipGetLastError());
        MH_HIP(hipMemcpyAsync(h, d, io_bytes, hipMemcpyDeviceToHost, c->stream));
    }
    MH_HIP(hipStreamSynchronize(c->stream));
    auto get = [&](void *dst, size_t off, size_t bytes) {
        if (dst) std::memcpy(dst, h + off, bytes);
    };
    get(S->head_markers, o_head, K * 24); get(S->normals, o_norm, K * 24); get(S->valid, o_valid, K);
    get(S->quad_coefs, o_coefs, K * 48); get(S->mean_curv, o_mean, K * 8); get(S->gauss_curv, o_gauss, K * 8);
    get(S->princ_curvs, o_pcurv, K * 16); get(S->princ_dirs, o_pdirs, K * 48); get(S->area, o_area, K * 8);
    get(S->nvert, o_nvert, K * 4); get(S->neib_ids, o_neib, slots * 8); get(S->voro_vertexes, o_voro, slots * 24);
    get(S->fitted_patch_points, o_fitted, E * 24);
    return MOLAR_HIP_OK;
}

// host-only: f64, the reference's loop order (molar_membrane/src/lib.rs:456-505); the f32 twin is in measure.hip
extern "C" int molar_hip_membrane_initial_normals_f64(size_t K, const double *head, const double *tail, const uint64_t *poff,
                                                      const uint64_t *pids, const uint8_t *valid, double *normals) {
    if (!head || !tail || !poff || !normals) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "initial_normals_f64: null argument");
    if (poff[K] && !pids) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "initial_normals_f64: patch_ids missing");
    for (size_t i = 0; i < K; ++i) {
        if (poff[i + 1] < poff[i]) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "initial_normals_f64: offsets not monotone");
        for (uint64_t q = poff[i]; q < poff[i + 1]; ++q)
            if (pids[q] >= K) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "initial_normals_f64: patch id %llu out of range", (unsigned long long)pids[q]);
    }
    struct V { double x, y, z; };
    auto nrm = [](V a) { return std::sqrt((a.x * a.x + a.y * a.y) + a.z * a.z); };
    auto unit = [&](V a) { const double n = nrm(a); return V{a.x / n, a.y / n, a.z / n}; };
    // nalgebra Vector::angle (the two norms handed in: functions of one vector each) against FRAC_PI_2 (lib.rs:472-473, 494)
    const double half_pi = 1.57079632679489661923;
    auto within_half_pi = [&](V a, double n1, V b, double n2) {
        if (n1 == 0.0 || n2 == 0.0) return true;                // Vector::angle returns 0
        double cc = ((a.x * b.x + a.y * b.y) + a.z * b.z) / (n1 * n2);
        cc = cc < -1.0 ? -1.0 : (cc > 1.0 ? 1.0 : cc);
        return std::acos(cc) <= half_pi;
    };
    std::vector<V> thv(K), nv(K);
    std::vector<double> len(K);
    auto ok = [&](size_t i) { return !valid || valid[i]; };
    for (size_t i = 0; i < K; ++i) {
        thv[i] = V{0, 0, 0};
        nv[i] = V{normals[3 * i], normals[3 * i + 1], normals[3 * i + 2]};
        if (ok(i)) thv[i] = unit(V{head[3 * i] - tail[3 * i], head[3 * i + 1] - tail[3 * i + 1], head[3 * i + 2] - tail[3 * i + 2]});
    }
    for (int pass = 0; pass < 2; ++pass) {
        const std::vector<V> &src = pass == 0 ? thv : nv;   // pass 2 reads normals already updated for l < i
        for (size_t i = 0; i < K; ++i) len[i] = nrm(src[i]);
        for (size_t i = 0; i < K; ++i) {
            if (!ok(i)) continue;
            const V self = src[i];
            const double nself = len[i];
            V sum{0, 0, 0};
            for (uint64_t q = poff[i]; q < poff[i + 1]; ++q) {
                const V o = src[pids[q]];
                if (within_half_pi(o, len[pids[q]], self, nself)) { sum.x += o.x; sum.y += o.y; sum.z += o.z; }
            }
            sum.x += self.x; sum.y += self.y; sum.z += self.z;   // .chain(once(central))
            nv[i] = unit(sum);
            if (pass == 1) len[i] = nrm(nv[i]);                  // src aliases nv in pass 2: keep its norm current
        }
    }
    for (size_t i = 0; i < K; ++i) {
        normals[3 * i] = nv[i].x; normals[3 * i + 1] = nv[i].y; normals[3 * i + 2] = nv[i].z;
    }
    return MOLAR_HIP_OK;
}

// smooth_curvature (lib.rs:584-621) in f64: the shells of molar_hip_membrane_smooth_curvature (membrane.hip), sums in double
extern "C" int molar_hip_membrane_smooth_curvature_f64(size_t K, const uint8_t *valid, const uint64_t *patch_offsets,
                                                       const uint32_t *nvert, const uint64_t *neib_ids, size_t n_shells,
                                                       double *mean_curv, double *gauss_curv) {
    MH_TRY(check_shell_args(K, valid, patch_offsets, nvert, neib_ids, "membrane_smooth_curvature_f64"));
    if (!mean_curv || !gauss_curv) return fail(MOLAR_HIP_ERR_INVALID_ARGUMENT, "membrane_smooth_curvature_f64: null argument");
    if (n_shells < 1) return MOLAR_HIP_OK;                         // lib.rs:585-587
    const std::vector<double> mean(mean_curv, mean_curv + K), gauss(gauss_curv, gauss_curv + K);      // the values before smoothing (:589-590)
    std::vector<uint32_t> stamp(K, 0u), members, frontier;
    for (size_t i = 0; i < K; ++i) {
        if (!valid[i]) continue;
        nth_shell_of(i, n_shells, patch_offsets, nvert, neib_ids, K, stamp, members, frontier);
        double m = 0.0, g = 0.0;
        uint32_t n_valid = 0;
        for (uint32_t id : members) {
            if (!valid[id]) continue;
            m += mean[id];
            g += gauss[id];
            ++n_valid;
        }
        mean_curv[i] = (mean[i] + m) / (double)(n_valid + 1u);
        gauss_curv[i] = (gauss[i] + g) / (double)(n_valid + 1u);
    }
    return MOLAR_HIP_OK;
}
