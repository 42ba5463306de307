// linalg3.hpp — tiny dense kernels, usable from host code and from one GPU thread.
//  * symmetric Jacobi eigensolver in double (N = 3 for the inertia tensor, N = 4 for Horn's key matrix)
//  * optimal rotation from a 3x3 mass-weighted covariance via Horn's unit-quaternion method.
//  * nalgebra's closed-form 3x3 inverse, Rodrigues' rotation and the finish of Measure::inertia / principal_transform,
//    templates over the real type of the f32 and the f64 entries.
//
// The reference obtains the rotation as U diag(1,1,sign det(U V^T)) V^T from nalgebra's SVD
// (molar/src/measure.rs:626-642).  For a non-degenerate covariance that rotation is the unique
// maximiser of tr(R^T cov) over proper rotations, which is exactly what the dominant
// eigenvector of Horn's 4x4 matrix encodes, so both give the same matrix to rounding.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <utility>

namespace mh {

// nalgebra try_inverse for 3x3 (closed form, column-major: m11 m21 m31 | m12 m22 m32 | m13 m23 m33).  A singular matrix
// (det == 0) returns false and leaves `o` untouched, as try_inverse_mut leaves the matrix.
template <class R>
__host__ __device__ inline bool inverse3(const R *m, R *o) {
    const R m11 = m[0], m21 = m[1], m31 = m[2], m12 = m[3], m22 = m[4], m32 = m[5], m13 = m[6], m23 = m[7], m33 = m[8];
    const R mi1 = m22 * m33 - m32 * m23;
    const R mi2 = m21 * m33 - m31 * m23;
    const R mi3 = m21 * m32 - m31 * m22;
    const R det = (m11 * mi1 - m12 * mi2) + m13 * mi3;
    if (det == R(0)) return false;
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

// nalgebra Rotation3::from_axis_angle (Rodrigues' formula on a unit axis), column-major
template <class R>
inline void rotation_from_axis_angle(const R *unit_axis3, R angle, R *R9) {
    const R ux = unit_axis3[0], uy = unit_axis3[1], uz = unit_axis3[2];
    const R sn = std::sin(angle), cs = std::cos(angle), k = R(1) - cs;
    const R sqx = ux * ux, sqy = uy * uy, sqz = uz * uz;
    const R rot[9] = {sqx + (R(1) - sqx) * cs, ux * uy * k + uz * sn, ux * uz * k - uy * sn,
                      ux * uy * k - uz * sn, sqy + (R(1) - sqy) * cs, uy * uz * k + ux * sn,
                      ux * uz * k + uy * sn, uy * uz * k - ux * sn, sqz + (R(1) - sqz) * cs};
    for (int i = 0; i < 9; ++i) R9[i] = rot[i];
}

// do_principal_transform (measure.rs:646-649): Translation(cm) * Rotation(axes^-1) * Translation(-cm); a singular `axes`
// stays as it is (try_inverse_mut)
template <class R>
inline void principal_transform_from(const R *axes9, const R *cm, R *R9, R *t3) {
    if (!inverse3(axes9, R9))
        for (int i = 0; i < 9; ++i) R9[i] = axes9[i];
    for (int r = 0; r < 3; ++r) t3[r] = cm[r] + (((R9[r] * -cm[0]) + (R9[3 + r] * -cm[1])) + (R9[6 + r] * -cm[2]));
}

constexpr double JACOBI_TOL2 = 1e-26;      // jacobi_sym's default: ample for results stored in f32

// Cyclic Jacobi on a symmetric NxN (row-major a[N*N], destroyed).  w = eigenvalues,
// v = eigenvectors as COLUMNS (v[r*N+c]).
template <int N>
__host__ __device__ inline void jacobi_sym(double *a, double *w, double *v, double tol2 = JACOBI_TOL2) {
    // every loop over matrix indices is unrolled: on the GPU the two small matrices then live in registers (dynamic
    // indexing would put them in scratch memory, ~20 us per call for one lane)
#pragma unroll
    for (int i = 0; i < N * N; ++i) v[i] = 0.0;
#pragma unroll
    for (int i = 0; i < N; ++i) v[i * N + i] = 1.0;
    for (int sweep = 0; sweep < 60; ++sweep) {
        double off = 0.0, diag = 0.0;
#pragma unroll
        for (int p = 0; p < N; ++p) {
            diag += a[p * N + p] * a[p * N + p];
#pragma unroll
            for (int q = p + 1; q < N; ++q) off += a[p * N + q] * a[p * N + q];
        }
        // off-diagonal mass below 1e-13 of the diagonal (squared: 1e-26): eigenvectors good to ~1e-13, far below the f32
        // results they feed; every further sweep is ~2 us of dependent f64 divisions and square roots on one GPU lane
        // (tol2: callers with f64 results ask for 1e-34 - one or two sweeps more, the convergence is quadratic)
        if (off <= tol2 * diag || off < 1e-300) break;
#pragma unroll
        for (int p = 0; p < N - 1; ++p)
#pragma unroll
            for (int q = p + 1; q < N; ++q) {
                const double apq = a[p * N + q];
                if (apq == 0.0) continue;
                const double tau = (a[q * N + q] - a[p * N + p]) / (2.0 * apq);
                const double t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
                const double cs = 1.0 / sqrt(1.0 + t * t), sn = t * cs;
#pragma unroll
                for (int k = 0; k < N; ++k) {   // columns p,q
                    const double akp = a[k * N + p], akq = a[k * N + q];
                    a[k * N + p] = cs * akp - sn * akq;
                    a[k * N + q] = sn * akp + cs * akq;
                }
#pragma unroll
                for (int k = 0; k < N; ++k) {   // rows p,q
                    const double apk = a[p * N + k], aqk = a[q * N + k];
                    a[p * N + k] = cs * apk - sn * aqk;
                    a[q * N + k] = sn * apk + cs * aqk;
                }
#pragma unroll
                for (int k = 0; k < N; ++k) {
                    const double vkp = v[k * N + p], vkq = v[k * N + q];
                    v[k * N + p] = cs * vkp - sn * vkq;
                    v[k * N + q] = sn * vkp + cs * vkq;
                }
            }
    }
#pragma unroll
    for (int i = 0; i < N; ++i) w[i] = a[i * N + i];
}


// 3x3 determinant of the rows (r0,r1,r2) x columns (c0,c1,c2) of a row-major 4x4
__host__ __device__ inline double minor3(const double *a, int r0, int r1, int r2, int c0, int c1, int c2) {
    return a[r0 * 4 + c0] * (a[r1 * 4 + c1] * a[r2 * 4 + c2] - a[r1 * 4 + c2] * a[r2 * 4 + c1]) -
           a[r0 * 4 + c1] * (a[r1 * 4 + c0] * a[r2 * 4 + c2] - a[r1 * 4 + c2] * a[r2 * 4 + c0]) +
           a[r0 * 4 + c2] * (a[r1 * 4 + c0] * a[r2 * 4 + c1] - a[r1 * 4 + c1] * a[r2 * 4 + c0]);
}

// Dominant eigenvector of Horn's symmetric, traceless 4x4 matrix K without sweeping the whole spectrum: the largest root
// of the characteristic polynomial l^4 + c2 l^2 + c1 l + c0 (c2 = -tr(K^2)/2, c1 = -tr(K^3)/3, c0 = det K) by Newton's
// iteration from the Frobenius norm - an upper bound of every eigenvalue, and from above the iteration on a polynomial
// with only real roots descends monotonically onto the largest one - then a null vector of K - l I as the largest
// column of its adjugate.  ~4 us for one GPU lane against ~20 us for the Jacobi sweeps.  Returns false (the caller falls
// back to Jacobi) when the root is not simple to working precision: the residual |(K - l I) q| is checked, so a
// vector that passes IS the eigenvector to 1e-10 relative.
__host__ __device__ inline bool horn_dominant_eigenvector(const double *K, double &q0, double &qx, double &qy, double &qz) {
    double K2[16], f2 = 0.0, t3 = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < 4; ++k) s += K[i * 4 + k] * K[k * 4 + j];
            K2[i * 4 + j] = s;
        }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        f2 += K[i] * K[i];
        t3 += K2[i] * K[i];          // tr(K^3) = sum_ij (K^2)_ij K_ji, K symmetric
    }
    if (!(f2 > 0.0)) return false;
    const double det = K[0] * minor3(K, 1, 2, 3, 1, 2, 3) - K[1] * minor3(K, 1, 2, 3, 0, 2, 3) +
                       K[2] * minor3(K, 1, 2, 3, 0, 1, 3) - K[3] * minor3(K, 1, 2, 3, 0, 1, 2);
    const double c2 = -0.5 * f2, c1 = -t3 / 3.0, c0 = det;
    double l = sqrt(f2);
    bool converged = false;
    for (int it = 0; it < 60; ++it) {
        const double l2 = l * l;
        const double P = (l2 + c2) * l2 + (c1 * l + c0);
        const double dP = (4.0 * l2 + 2.0 * c2) * l + c1;
        if (!(dP > 0.0)) break;                   // at or beyond a multiple root
        const double step = P / dP;
        l -= step;
        if (fabs(step) <= 1e-15 * fabs(l)) {
            converged = true;
            break;
        }
    }
    if (!converged) return false;
    double A[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) A[i] = K[i];
#pragma unroll
    for (int i = 0; i < 4; ++i) A[i * 4 + i] -= l;
    // adjugate of the symmetric A, column by column: adj[i][j] = (-1)^(i+j) * minor(row j, column i removed)
    double best = -1.0;
    q0 = qx = qy = qz = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int r0 = j == 0 ? 1 : 0, r1 = j <= 1 ? 2 : 1, r2 = j <= 2 ? 3 : 2;     // rows without j
        const double v0 = minor3(A, r0, r1, r2, 1, 2, 3), v1 = minor3(A, r0, r1, r2, 0, 2, 3);
        const double v2 = minor3(A, r0, r1, r2, 0, 1, 3), v3 = minor3(A, r0, r1, r2, 0, 1, 2);
        const double sg = (j & 1) ? -1.0 : 1.0;
        const double e0 = sg * v0, e1 = -sg * v1, e2 = sg * v2, e3 = -sg * v3;
        const double nn = (e0 * e0 + e1 * e1) + (e2 * e2 + e3 * e3);
        if (nn > best) {
            best = nn;
            q0 = e0; qx = e1; qy = e2; qz = e3;
        }
    }
    if (!(best > 0.0)) return false;
    double res = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const double r = ((A[i * 4 + 0] * q0 + A[i * 4 + 1] * qx) + A[i * 4 + 2] * qy) + A[i * 4 + 3] * qz;
        res += r * r;
    }
    return res <= 1e-20 * f2 * best;
}

// Horn's key matrix of S[a][b] = sum w x1[a] x2[b] (row-major S[a*3+b]); its largest eigenvalue is the maximum of
// sum w (R x1) . x2 over proper rotations R, the same for S and for its transpose.
__host__ __device__ inline void horn_matrix(const double *S, double *K) {
    const double Sxx = S[0], Sxy = S[1], Sxz = S[2], Syx = S[3], Syy = S[4], Syz = S[5], Szx = S[6], Szy = S[7], Szz = S[8];
    const double Nm[16] = {(Sxx + Syy) + Szz, Syz - Szy,         Szx - Sxz,          Sxy - Syx,
                           Syz - Szy,         (Sxx - Syy) - Szz, Sxy + Syx,          Szx + Sxz,
                           Szx - Sxz,         Sxy + Syx,         (Syy - Sxx) - Szz,  Syz + Szy,
                           Sxy - Syx,         Szx + Sxz,         Syz + Szy,          (Szz - Sxx) - Syy};
#pragma unroll
    for (int i = 0; i < 16; ++i) K[i] = Nm[i];
}

// s + a b with the rounding errors of the product and of the sum collected in `err` (Ogita, Rump and Oishi's Dot2): the
// explicit fma gives the product's error exactly, and -ffp-contract=off keeps the rest as written
__host__ __device__ inline void dot2_step(double a, double b, double &s, double &err) {
    const double p = a * b, e = fma(a, b, -p);
    const double t = s + p, z = t - s;
    err += ((s - (t - z)) + (p - z)) + e;
    s = t;
}

// Rayleigh quotient v^T K v / v^T v of a symmetric 4x4 in twice the working precision: for an eigenvector good to d it
// is the eigenvalue to d^2 |K| plus a few 2^-53 of the eigenvalue itself, whatever the other eigenvalues are
__host__ __device__ inline double rayleigh4(const double *K, double v0, double v1, double v2, double v3) {
    const double v[4] = {v0, v1, v2, v3};
    double num = 0.0, nerr = 0.0, den = 0.0, derr = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        double y = 0.0, yerr = 0.0;
#pragma unroll
        for (int j = 0; j < 4; ++j) dot2_step(K[i * 4 + j], v[j], y, yerr);
        dot2_step(v[i], y, num, nerr);
        nerr += v[i] * yerr;
        dot2_step(v[i], v[i], den, derr);
    }
    return (num + nerr) / (den + derr);
}

// Largest eigenvalue of Horn's symmetric, traceless 4x4 matrix K, for callers that need no rotation: the
// Newton iteration of horn_dominant_eigenvector on the characteristic polynomial, accepted only where the root is well
// conditioned.  A rounding error e in the polynomial's value moves the root by e / P'(l), and both the coefficients and
// Horner's scheme carry a few 2^-53 of M = l^4 + |c2| l^2 + |c1| l + |c0|: the root is taken when M <= 2 l P'(l), which
// keeps it within a few 2^-53 of l (an isotropic covariance has M = 0.84 l P').  Multiple or close roots (planar and
// collinear selections, a mirror image) fail that test or the iteration itself and go to Jacobi sweeps at f64 working
// precision for the eigenvector, whatever the gaps.
__host__ __device__ inline double horn_lambda_max(const double *K) {
    double K2[16], f2 = 0.0, t3 = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < 4; ++k) s += K[i * 4 + k] * K[k * 4 + j];
            K2[i * 4 + j] = s;
        }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        f2 += K[i] * K[i];
        t3 += K2[i] * K[i];
    }
    if (f2 == 0.0) return 0.0;
    if (f2 > 0.0 && f2 <= 1.7976931348623157e308) {
        const double det = K[0] * minor3(K, 1, 2, 3, 1, 2, 3) - K[1] * minor3(K, 1, 2, 3, 0, 2, 3) +
                           K[2] * minor3(K, 1, 2, 3, 0, 1, 3) - K[3] * minor3(K, 1, 2, 3, 0, 1, 2);
        const double c2 = -0.5 * f2, c1 = -t3 / 3.0, c0 = det;
        double l = sqrt(f2);
        for (int it = 0; it < 60; ++it) {
            const double l2 = l * l;
            const double P = (l2 + c2) * l2 + (c1 * l + c0);
            const double dP = (4.0 * l2 + 2.0 * c2) * l + c1;
            if (!(dP > 0.0)) break;                   // at or beyond a multiple root
            const double step = P / dP;
            l -= step;
            if (fabs(step) <= 1e-15 * fabs(l)) {
                const double m2 = l * l;
                const double M = (m2 + fabs(c2)) * m2 + (fabs(c1) * l + fabs(c0));
                const double dQ = (4.0 * m2 + 2.0 * c2) * l + c1;
                if (M <= 2.0 * l * dQ) return l;
                break;
            }
        }
    }
    // Jacobi's own eigenvalues carry the roundings of every rotation (up to a hundred 2^-53 |K| were seen on two-atom
    // frames); its eigenvector is good to about as much, and the Rayleigh quotient on the untouched matrix squares that
    double A[16], w[4], v[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) A[i] = K[i];
    jacobi_sym<4>(A, w, v, 1e-34);
    double wb = w[0], q0 = v[0], q1 = v[4], q2 = v[8], q3 = v[12];
#pragma unroll
    for (int i = 1; i < 4; ++i)
        if (w[i] > wb) {
            wb = w[i];
            q0 = v[0 * 4 + i]; q1 = v[1 * 4 + i]; q2 = v[2 * 4 + i]; q3 = v[3 * 4 + i];
        }
    return rayleigh4(K, q0, q1, q2, q3);
}

// cov(r,c) = sum m * q2[r] * q1[c]  (measure.rs:621-623), column-major cov[c*3+r].
// Writes R (column-major) with q2 ~ R q1.  Returns false if cov holds a non-finite entry (NaN or +-inf: the callers
// report MOLAR_HIP_ERR_SVD) or if no unit quaternion comes out of the eigen-solve.
// precise: Jacobi only, swept to f64 working precision (the f64 Measure entries; the Newton path accepts an eigenvector
// with a 1e-10 relative residual, ample for f32 records only).
__host__ __device__ inline bool rotation_from_cov(const double *cov, double *R, bool precise = false) {
    for (int i = 0; i < 9; ++i)
        if (!(fabs(cov[i]) <= 1.7976931348623157e308)) return false;      // NaN or infinity
    // S[a][b] = sum m q1[a] q2[b] = cov(b,a)
    const double Sxx = cov[0 * 3 + 0], Sxy = cov[0 * 3 + 1], Sxz = cov[0 * 3 + 2];
    const double Syx = cov[1 * 3 + 0], Syy = cov[1 * 3 + 1], Syz = cov[1 * 3 + 2];
    const double Szx = cov[2 * 3 + 0], Szy = cov[2 * 3 + 1], Szz = cov[2 * 3 + 2];
    double Nm[16] = {Sxx + Syy + Szz, Syz - Szy,       Szx - Sxz,        Sxy - Syx,
                     Syz - Szy,       Sxx - Syy - Szz, Sxy + Syx,        Szx + Sxz,
                     Szx - Sxz,       Sxy + Syx,       -Sxx + Syy - Szz, Syz + Szy,
                     Sxy - Syx,       Szx + Sxz,       Syz + Szy,        -Sxx - Syy + Szz};
    double q0, qx, qy, qz;
    if (precise || !horn_dominant_eigenvector(Nm, q0, qx, qy, qz)) {
    double w[4], v[16];
    jacobi_sym<4>(Nm, w, v, precise ? 1e-34 : 1e-26);
    // eigenvector of the largest eigenvalue (first one wins ties); selected with static indices, see jacobi_sym
    double wb = w[0];
    q0 = v[0]; qx = v[4]; qy = v[8]; qz = v[12];
#pragma unroll
    for (int i = 1; i < 4; ++i)
        if (w[i] > wb) {
            wb = w[i];
            q0 = v[0 * 4 + i]; qx = v[1 * 4 + i]; qy = v[2 * 4 + i]; qz = v[3 * 4 + i];
        }
    }
    const double nq = sqrt(q0 * q0 + qx * qx + qy * qy + qz * qz);
    if (!(nq > 0.0) || !(nq <= 1.7976931348623157e308)) return false;
    q0 /= nq; qx /= nq; qy /= nq; qz /= nq;
    // column-major R
    R[0] = 1.0 - 2.0 * (qy * qy + qz * qz);
    R[1] = 2.0 * (qx * qy + q0 * qz);
    R[2] = 2.0 * (qx * qz - q0 * qy);
    R[3] = 2.0 * (qx * qy - q0 * qz);
    R[4] = 1.0 - 2.0 * (qx * qx + qz * qz);
    R[5] = 2.0 * (qy * qz + q0 * qx);
    R[6] = 2.0 * (qx * qz + q0 * qy);
    R[7] = 2.0 * (qy * qz - q0 * qx);
    R[8] = 1.0 - 2.0 * (qx * qx + qy * qy);
    return true;
}

// The finish of Measure::inertia (measure.rs:591-607) on the symmetric tensor T (stored in R, as the reference's Matrix3 is,
// before the eigen solve): ascending moments; axes col0, col1 normalised in R, col2 = col0 x col1.  tol2: see jacobi_sym
// (the f64 entries pass 1e-34).
template <class R>
inline void principal_axes(const R *T, double tol2, R *moments, R *axes9) {
    double A[9], w[3], V[9];
    for (int i = 0; i < 9; ++i) A[i] = T[i];
    jacobi_sym<3>(A, w, V, tol2);
    int ord[3] = {0, 1, 2};   // ascending moments (:594-601)
    for (int a = 0; a < 2; ++a)
        for (int q = a + 1; q < 3; ++q)
            if (w[ord[q]] < w[ord[a]]) std::swap(ord[a], ord[q]);
    for (int k = 0; k < 3; ++k) moments[k] = (R)w[ord[k]];
    // col0, col1 normalised, col2 = col0 x col1 (:603-607)
    R e[2][3];
    for (int k = 0; k < 2; ++k) {
        const R v[3] = {(R)V[0 * 3 + ord[k]], (R)V[1 * 3 + ord[k]], (R)V[2 * 3 + ord[k]]};
        const R nn = std::sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
        for (int d = 0; d < 3; ++d) e[k][d] = v[d] / nn;
    }
    const R c2[3] = {e[0][1] * e[1][2] - e[0][2] * e[1][1], e[0][2] * e[1][0] - e[0][0] * e[1][2],
                     e[0][0] * e[1][1] - e[0][1] * e[1][0]};
    for (int d = 0; d < 3; ++d) {
        axes9[0 * 3 + d] = e[0][d];
        axes9[1 * 3 + d] = e[1][d];
        axes9[2 * 3 + d] = c2[d];
    }
}

}  // namespace mh
