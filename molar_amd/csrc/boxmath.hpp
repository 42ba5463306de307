// boxmath.hpp — PeriodicBox arithmetic shared by host API code and gfx950 kernels, in f32 and in f64 (MolAR built with its
// `f64` feature: Float = f64, aliases.rs:10-13).
//
// Restates molar/src/periodic_box.rs with the reference's operation order, once for both precisions; the whole
// library is compiled with -ffp-contract=off so no a*b+c here becomes an FMA (Rust never
// contracts).  nalgebra's 3-vector kernels as used by the reference:
//   M*v   : y_r = ((M_r0*v0) + M_r1*v1) + M_r2*v2
//   |v|^2 : ((x*x) + (y*y)) + (z*z)
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "common.hpp"
#include "linalg3.hpp"

namespace mh {

template <class R>
struct Vec3 {
    R x, y, z;
};
using V3 = Vec3<float>;
using D3 = Vec3<double>;

// PeriodicBox in f64 (periodic_box.rs:15-23 with Float = f64); molar_hip_box (molar_hip.h) is the f32 one.  A plain struct,
// not an instance of a template: its name is part of the mangled names of the kernels that take a `const BoxD *`.
struct BoxD {
    double m[9];       // column-major, columns a, b, c
    double inv[9];     // nalgebra try_inverse
    int32_t nshift;    // tric_corrections.len()
    double shifts[26 * 3];
};

#define MH_HD __host__ __device__ __forceinline__

MH_HD V3 v3(float x, float y, float z) { return V3{x, y, z}; }
template <class R> MH_HD Vec3<R> operator+(Vec3<R> a, Vec3<R> b) { return Vec3<R>{a.x + b.x, a.y + b.y, a.z + b.z}; }
template <class R> MH_HD Vec3<R> operator-(Vec3<R> a, Vec3<R> b) { return Vec3<R>{a.x - b.x, a.y - b.y, a.z - b.z}; }
template <class R> MH_HD R norm2(Vec3<R> v) { return (v.x * v.x + v.y * v.y) + v.z * v.z; }

// column-major 3x3: element (r,c) = m[c*3+r]
template <class R>
MH_HD Vec3<R> mat_vec(const R *m, Vec3<R> v) {
    return Vec3<R>{(m[0] * v.x + m[3] * v.y) + m[6] * v.z, (m[1] * v.x + m[4] * v.y) + m[7] * v.z,
                   (m[2] * v.x + m[5] * v.y) + m[8] * v.z};
}

// Rust f32::round / f64::round — half away from zero
MH_HD float round_away(float x) {
#ifdef __HIP_DEVICE_COMPILE__
    return __builtin_roundf(x);
#else
    return std::round(x);
#endif
}
MH_HD double round_away(double x) {
#ifdef __HIP_DEVICE_COMPILE__
    return __builtin_round(x);
#else
    return std::round(x);
#endif
}

// Rust f32::fract = x - trunc(x)
MH_HD float fract_rs(float x) {
#ifdef __HIP_DEVICE_COMPILE__
    return x - __builtin_truncf(x);
#else
    return x - std::trunc(x);
#endif
}

// Rust `f as usize` followed by .clamp(0, hi): saturating cast, NaN -> 0  (distance_search.rs:176-177)
MH_HD uint32_t floor_to_cell(float v, uint32_t dim) {
#ifdef __HIP_DEVICE_COMPILE__
    float f = __builtin_floorf(v);
#else
    float f = std::floor(v);
#endif
    if (!(f > 0.0f)) return 0u;
    if (f >= (float)dim) return dim - 1u;
    uint32_t u = (uint32_t)f;
    return u > dim - 1u ? dim - 1u : u;
}

// periodic_box.rs:286-318 (shortest_vector_dims), for molar_hip_box and BoxD.  `pbc` is the PbcDims byte; the triclinic
// candidate loop runs only for a non-empty shift list AND pbc == PBC_FULL (:304).
template <class B, class R>
MH_HD Vec3<R> shortest_vector(const B &b, Vec3<R> v, uint32_t pbc) {
    Vec3<R> f = mat_vec(b.inv, v);
    if (pbc & 1u) f.x -= round_away(f.x);
    if (pbc & 2u) f.y -= round_away(f.y);
    if (pbc & 4u) f.z -= round_away(f.z);
    const Vec3<R> start = mat_vec(b.m, f);
    if (b.nshift == 0 || pbc != MOLAR_HIP_PBC_FULL) return start;
    Vec3<R> best = start;
    R best2 = norm2(start);
    for (int k = 0; k < b.nshift; ++k) {
        const Vec3<R> cand = start + Vec3<R>{b.shifts[3 * k], b.shifts[3 * k + 1], b.shifts[3 * k + 2]};
        const R n2 = norm2(cand);
        if (n2 < best2) {
            best2 = n2;
            best = cand;
        }
    }
    return best;
}

// periodic_box.rs:322-330 (closest_image_dims)
template <class B, class R>
MH_HD Vec3<R> closest_image(const B &b, Vec3<R> p, Vec3<R> target, uint32_t pbc) {
    return target + shortest_vector(b, p - target, pbc);
}

// PeriodicBox::from_matrix (:156-176) + build_tric_corrections (:25-66) into a molar_hip_box (R = float) or a BoxD (double)
template <class R, class B>
inline int box_from_matrix(const R *m9, B *out) {
    using V = Vec3<R>;
    auto len = [](V v) { return std::sqrt(norm2(v)); };
    V col[3];
    for (int k = 0; k < 3; ++k) {
        col[k] = V{m9[3 * k], m9[3 * k + 1], m9[3 * k + 2]};
        if (len(col[k]) == R(0)) return fail(MOLAR_HIP_ERR_ZERO_LENGTH_VECTOR, "zero length box vector");
    }
    std::memcpy(out->m, m9, sizeof out->m);
    if (!inverse3(out->m, out->inv)) return fail(MOLAR_HIP_ERR_INVERSE_FAILED, "box matrix inverse failed");   // (:167-169)
    out->nshift = 0;
    const bool ortho = m9[3] == R(0) && m9[6] == R(0) && m9[1] == R(0) && m9[7] == R(0) && m9[2] == R(0) && m9[5] == R(0);
    if (ortho) return 0;
    const V a = col[0], b = col[1], c = col[2], na = V{-a.x, -a.y, -a.z};
    const R longest = std::fmax(std::fmax(std::fmax(len((a + b) + c), len((a + b) - c)), len((a - b) + c)), len((na + b) + c));
    const R half_diag = R(0.5) * longest, two = R(2) * half_diag, bound2 = two * two;
    for (int i = -1; i <= 1; ++i)
        for (int j = -1; j <= 1; ++j)
            for (int k = -1; k <= 1; ++k) {
                if (!i && !j && !k) continue;
                const R fi = (R)i, fj = (R)j, fk = (R)k;
                const V sft = (V{fi * a.x, fi * a.y, fi * a.z} + V{fj * b.x, fj * b.y, fj * b.z}) + V{fk * c.x, fk * c.y, fk * c.z};
                if (norm2(sft) < bound2) {
                    R *dst = out->shifts + 3 * out->nshift++;
                    dst[0] = sft.x; dst[1] = sft.y; dst[2] = sft.z;
                }
            }
    return 0;
}

// PeriodicBox::from_matrix in double on the device (box_from_matrix above, operation by operation, its two errors
// included); 0: a box, 1: a box vector of zero length, 2: a matrix without an inverse.
__device__ inline int box_from_matrix_device(const double *m9, BoxD *out) {
    D3 col[3];
    bool ok = true;
    for (int k = 0; k < 3; ++k) {
        col[k] = D3{m9[3 * k], m9[3 * k + 1], m9[3 * k + 2]};
        if (sqrt(norm2(col[k])) == 0.0) ok = false;
    }
    for (int q = 0; q < 9; ++q) {
        out->m[q] = m9[q];
        out->inv[q] = __builtin_nan("");
    }
    out->nshift = 0;
    if (!ok) return 1;
    if (!inverse3(out->m, out->inv)) return 2;
    const bool ortho = m9[3] == 0.0 && m9[6] == 0.0 && m9[1] == 0.0 && m9[7] == 0.0 && m9[2] == 0.0 && m9[5] == 0.0;
    if (ortho) return 0;
    const D3 a = col[0], b = col[1], c = col[2], na = D3{-a.x, -a.y, -a.z};
    const double longest = fmax(fmax(fmax(sqrt(norm2((a + b) + c)), sqrt(norm2((a + b) - c))), sqrt(norm2((a - b) + c))), sqrt(norm2((na + b) + c)));
    const double half_diag = 0.5 * longest, two = 2.0 * half_diag, bound2 = two * two;
    for (int i = -1; i <= 1; ++i)
        for (int j = -1; j <= 1; ++j)
            for (int k = -1; k <= 1; ++k) {
                if (!i && !j && !k) continue;
                const double fi = (double)i, fj = (double)j, fk = (double)k;
                const D3 sft = (D3{fi * a.x, fi * a.y, fi * a.z} + D3{fj * b.x, fj * b.y, fj * b.z}) + D3{fk * c.x, fk * c.y, fk * c.z};
                if (norm2(sft) < bound2) {
                    double *dst = out->shifts + 3 * out->nshift++;
                    dst[0] = sft.x;
                    dst[1] = sft.y;
                    dst[2] = sft.z;
                }
            }
    return 0;
}

inline int box64_from_matrix(const double *m9, BoxD *out) {
    if (!m9) return fail(MOLAR_HIP_ERR_NO_PBC, "pbc operation without periodic box");
    return box_from_matrix(m9, out);
}

}  // namespace mh
