// icp_plane_rule.h -- the rule of lcd_register_icp_plane (include/lcd.h writes it down with the reference's line numbers) as functions the
// kernel (register_icp_plane.hip) and the host mirror (rtabmap_amd/host/RegistrationIcp.cpp) compile alike: the structural complexity of the
// normals, the decision between the two branches, the point-to-plane loop and its gated correspondences, and the low-complexity fallback
// around icp_rule.h's loop.  fp32, one rounded operation per statement, never contracted; only + - x / sqrt; the threshold, the gate's
// comparison and the variance are fp64.  What needs a cloud as a whole is a backend's, as in icp_rule.h; solve() drives either.  Internal.
#pragma once
#include "icp_rule.h"

namespace lcd {
namespace icpp {

using icp::compose;
using icp::finite;
using icp::invert;

constexpr int ST_LOW_COMPLEXITY = 4;         // lcd_icp_status, behind icp::ST_BELOW_RATIO
constexpr int STOP_SINGULAR = 5;             // lcd_icp_stop, behind icp::STOP_FEW_CORRESPONDENCES
constexpr int SUMS = 27;                     // 21 of A^T A's upper triangle, 6 of A^T b
// Cyclic Jacobi sweeps of the 3 x 3 covariance of the normals.  The matrix is the 4 x 4 of motion_rule_common.h with an empty last row and
// column, so a sweep is the three planes (0, 1), (0, 2), (1, 2) of that code.  The count is the 4 x 4's (4 was the smallest
// count two more sweeps did not change, the rule takes 5); a 3 x 3 has half the planes to a sweep and converges no slower, and
// tests/test_register_icp_plane_model.py checks that 6 and 7 sweeps change no bit of any eigenvalue over the test scans.
constexpr int SWEEPS = m3d::SWEEPS;

M3D_FN bool finite3(float x, float y, float z) { return finite(x) && finite(y) && finite(z); }

// step 1: R n with the rotation of a model
M3D_FN void rotate(const float m[12], float nx, float ny, float nz, float& x, float& y, float& z) {
    const float x0 = m[0] * nx, x1 = m[1] * ny, x2 = m[2] * nz;
    const float x01 = x0 + x1;
    x = x01 + x2;
    const float y0 = m[4] * nx, y1 = m[5] * ny, y2 = m[6] * nz;
    const float y01 = y0 + y1;
    y = y01 + y2;
    const float z0 = m[8] * nx, z1 = m[9] * ny, z2 = m[10] * nz;
    const float z01 = z0 + z1;
    z = z01 + z2;
}

M3D_FN float dot3(const float a[3], const float b[3]) {
    const float p0 = a[0] * b[0], p1 = a[1] * b[1], p2 = a[2] * b[2];
    const float p01 = p0 + p1;
    return p01 + p2;
}

// ---- step 2: the structural complexity of one side (util3d_surface.cpp:3164-3241)
struct Pca {
    float complexity;                        // third value x 3; 0 without a PCA
    float values[3], vectors[9];             // descending, the vectors as rows; zeros without a PCA
    bool has;                                // oi > 1
};

// the six products of a row's centred normal, in the order xx, xy, xz, yy, yz, zz
M3D_FN void cov_terms(const float n[3], const float mean[3], float e[6]) {
    const float dx = n[0] - mean[0], dy = n[1] - mean[1], dz = n[2] - mean[2];
    e[0] = dx * dx; e[1] = dx * dy; e[2] = dx * dz; e[3] = dy * dy; e[4] = dy * dz; e[5] = dz * dz;
}

// the mean over 2 oi rows of which oi are zero (:3221 hands cv::PCA the buffer's first 2 oi rows)
M3D_FN void pca_mean(int oi, const float sum[3], float mean[3]) {
    const float rows = (float)(2 * oi);
#pragma unroll
    for (int a = 0; a < 3; ++a) mean[a] = sum[a] / rows;
}

// The eigen decomposition of a symmetric 3 x 3 given as its upper triangle (xx, xy, xz, yy, yz, zz): SWEEPS sweeps of the cyclic Jacobi over
// the planes (0, 1), (0, 2), (1, 2).  The values are left on A's diagonal in no order, value k's vector in column k of V.  Step 2 here and the
// normals of scan_filter_rule.h call it.
M3D_FN void jacobi3(const float cov[6], float A[4][4], float V[4][4]) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) { A[r][c] = 0.0f; V[r][c] = r == c ? 1.0f : 0.0f; }
    A[0][0] = cov[0]; A[0][1] = cov[1]; A[0][2] = cov[2]; A[1][1] = cov[3]; A[1][2] = cov[4]; A[2][2] = cov[5];
    A[1][0] = cov[1]; A[2][0] = cov[2]; A[2][1] = cov[4];
#pragma unroll
    for (int sweep = 0; sweep < SWEEPS; ++sweep) {
        m3d::jacobi_rotate<0, 1>(A, V); m3d::jacobi_rotate<0, 2>(A, V); m3d::jacobi_rotate<1, 2>(A, V);
    }
}

// the covariance from the six sums over the oi rows that carry a normal and the oi zero rows' share, its eigenvalues and vectors
M3D_FN void pca_of(int oi, const float mean[3], const float C[6], Pca& p) {
    const float rows = (float)(2 * oi), zeros = (float)oi;
    float cov[6];
    const int ia[6] = {0, 0, 0, 1, 1, 2}, ib[6] = {0, 1, 2, 1, 2, 2};
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const float mm = mean[ia[k]] * mean[ib[k]];
        const float z = zeros * mm;
        const float s = C[k] + z;
        cov[k] = s / rows;
    }
    float A[4][4], V[4][4];
    jacobi3(cov, A, V);
    // descending, the lower index first among equals (a NaN stays where it is); values are selected, never an address
    float v0 = A[0][0], v1 = A[1][1], v2 = A[2][2];
    float e0[3] = {V[0][0], V[1][0], V[2][0]}, e1[3] = {V[0][1], V[1][1], V[2][1]}, e2[3] = {V[0][2], V[1][2], V[2][2]};
    auto swap_if = [](float& a, float& b, float x[3], float y[3]) {
        if (b > a) {
            const float t = a; a = b; b = t;
#pragma unroll
            for (int k = 0; k < 3; ++k) { const float u = x[k]; x[k] = y[k]; y[k] = u; }
        }
    };
    swap_if(v0, v1, e0, e1);
    swap_if(v1, v2, e1, e2);
    swap_if(v0, v1, e0, e1);
    p.values[0] = v0; p.values[1] = v1; p.values[2] = v2;
#pragma unroll
    for (int k = 0; k < 3; ++k) { p.vectors[k] = e0[k]; p.vectors[3 + k] = e1[k]; p.vectors[6 + k] = e2[k]; }
    p.complexity = v2 * 3.0f;
    p.has = true;
}

// one side's complexity from the backend's two sums
template <class B>
M3D_FN void pca_side(B& b, bool to_side, Pca& p) {
    p.complexity = 0.0f; p.has = false;
#pragma unroll
    for (int k = 0; k < 3; ++k) p.values[k] = 0.0f;
#pragma unroll
    for (int k = 0; k < 9; ++k) p.vectors[k] = 0.0f;
    float sum[3], mean[3], C[6];
    const int oi = b.normal_sums(to_side, sum);
    if (oi <= 1) return;
    pca_mean(oi, sum, mean);
    b.normal_cov(to_side, mean, C);
    pca_of(oi, mean, C, p);
}

// ---- step 4: the point-to-plane fit (pcl::registration::TransformationEstimationPointToPlaneLLS, uncentred as PCL's): the 27 products of one
// correspondence (s the source point, d the target point, n its normal)
M3D_FN void plane_terms(const float s[3], const float d[3], const float n[3], float out[SUMS]) {
    float a[6];
    const float yz = s[1] * n[2], zy = s[2] * n[1], zx = s[2] * n[0], xz = s[0] * n[2], xy = s[0] * n[1], yx = s[1] * n[0];
    a[0] = yz - zy; a[1] = zx - xz; a[2] = xy - yx;                    // s x n
    a[3] = n[0]; a[4] = n[1]; a[5] = n[2];
    const float nd = dot3(n, d), ns = dot3(n, s);
    const float b = nd - ns;
    int o = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = i; j < 6; ++j) out[o++] = a[i] * a[j];
#pragma unroll
    for (int i = 0; i < 6; ++i) out[o++] = a[i] * b;
}

// T from the 27 sums: x by LDL^T, then PCL's Rz(x2) Ry(x1) Rx(x0) without sines and cosines: the product of the three axis quaternions
// (1, 0, 0, c) (1, 0, b, 0) (1, a, 0, 0) with a = x0 / 2, b = x1 / 2, c = x2 / 2, which is (1 + abc, a - bc, b + ac, c - ab), normalised -- an
// exact rotation whose three angles are 2 atan(x / 2) = x - x^3 / 12, so it agrees with PCL's matrix to second order.  (The plain quaternion
// (1, a, b, c) agrees to first order only: measured against a float64 PCL-style ICP, its iterates left 2 of 24 room pairs in another fixed
// point, 6e-3 away)  The translation is (x3, x4, x5) as PCL sets it.
// false: a pivot that is not positive and finite, or a solution that is not finite
M3D_FN bool plane_fit(const float S[SUMS], float T[12]) {
    float x[6];
    if (!m3d::ldlt6_solve(S, x)) return false;
    const float a = 0.5f * x[0], b = 0.5f * x[1], c = 0.5f * x[2];
    const float ab = a * b, ac = a * c, bc = b * c;
    const float abc = ab * c;
    float q0 = 1.0f + abc, q1 = a - bc, q2 = b + ac, q3 = c - ab;
    float R[3][3];
    m3d::quat_rotation(q0, q1, q2, q3, R);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        T[4 * r] = R[r][0]; T[4 * r + 1] = R[r][1]; T[4 * r + 2] = R[r][2];
        T[4 * r + 3] = x[3 + r];
    }
    return true;
}

// Transform::to3DoF (:485-489) without the arc tangent: the rotation about z of (R00, R10), x and y kept
M3D_FN void to_3dof(float F[12]) {
    const float aa = F[0] * F[0], bb = F[4] * F[4];
    const float n2 = aa + bb;
    const float n = sqrtf(n2);
    float c = 1.0f, s = 0.0f;
    if (n != 0.0f && finite(n)) { c = F[0] / n; s = F[4] / n; }
    const float x = F[3], y = F[7];
    F[0] = c; F[1] = -s; F[2] = 0.0f; F[3] = x;
    F[4] = s; F[5] = c; F[6] = 0.0f; F[7] = y;
    F[8] = 0.0f; F[9] = 0.0f; F[10] = 1.0f; F[11] = 0.0f;
}

// step 5's gate (util3d_registration.cpp:268-289, pcl::getAngle3D): the cosine of the unit vectors against min_normal_cos in fp64
M3D_FN bool gate_passes(const float v1[3], const float v2[3], double min_normal_cos) {
    float u1[3], u2[3];
    const float s1 = dot3(v1, v1), s2 = dot3(v2, v2);
    const float r1 = sqrtf(s1), r2 = sqrtf(s2);
#pragma unroll
    for (int k = 0; k < 3; ++k) { u1[k] = s1 == 0.0f ? v1[k] : v1[k] / r1; u2[k] = s2 == 0.0f ? v2[k] : v2[k] / r2; }
    return (double)dot3(u1, u2) > min_normal_cos;
}

// step 6, strategy 1 (:789-832): the correction's translation limited to the well-constrained axes; F <- guess x [R_C | vp]^-1 x guess^-1
M3D_FN void limit_translation(float F[12], const float guess[12], const float vectors[9], bool has_vectors, bool second_too) {
    float Finv[12], Ginv[12], X[12], C[12];
    invert(F, Finv);
    invert(guess, Ginv);
    compose(Finv, guess, X);
    compose(Ginv, X, C);
    const float v[3] = {C[3], C[7], C[11]};
    float vp[3] = {0.0f, 0.0f, 0.0f};
    if (has_vectors) {
        const float a = dot3(v, vectors), b = dot3(v, vectors + 3);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float p = vectors[k] * a, q = vectors[3 + k] * b;
            vp[k] = second_too ? p + q : p;
        }
    }
    C[3] = vp[0]; C[7] = vp[1]; C[11] = vp[2];
    float Cinv[12], Y[12];
    invert(C, Cinv);
    compose(guess, Cinv, Y);
    compose(Y, Ginv, F);
}

struct Params {
    int max_iterations, max_laser_scans, strategy;
    bool force_3dof, gate;
    float epsilon, correspondence_ratio, min_complexity;
    double min_normal_cos;
};

struct Result : icp::Result {
    int32_t branch;
    float complexity, values[3], vectors[9], second;
};

// The backend is icp_rule.h's with, in addition:
//   int normal_sums(bool to_side, float sum[3])      the rows of a side whose normal is finite (oi), and SUM of their rotated normals
//   void normal_cov(bool to_side, const float mean[3], float C[6])   SUM of cov_terms over the same rows
//   void participate(bool with_normals)              fixes which rows take part (finite coordinates, and a finite normal for branch 0), stages Q
//   int rows_from(); int rows_to()                   rows with finite coordinates
//   bool fit_plane(float T[12])                      step 4 of branch 0 over the last correspond()
//   void register_normals(const float F[12])         the from-side's normals become F's rotation of the given ones
//   int reciprocal_gated(bool from_is_target, bool gate, double min_cos)   step 5: the reciprocal correspondences, out_match of those that
//                                                    pass the gate, returns their number
//   float median_first(int n)                        the d2 of rank n >> 1 among the first n reciprocal correspondences in source-row order
template <class B>
M3D_FN void solve(B& b, const Params& p, const float guess[12], Result& r) {
    icp::clear(r);
    r.status = icp::ST_OK; r.branch = 0; r.second = 1.0f;
    Pca pf, pt;
    pca_side(b, false, pf);
    pca_side(b, true, pt);
    const bool from_less = pf.complexity < pt.complexity;              // :530, :539: the to-side on equality
    r.complexity = from_less ? pf.complexity : pt.complexity;
#pragma unroll
    for (int k = 0; k < 3; ++k) r.values[k] = from_less ? pf.values[k] : pt.values[k];
#pragma unroll
    for (int k = 0; k < 9; ++k) r.vectors[k] = from_less ? pf.vectors[k] : pt.vectors[k];
    bool has_vectors = false;
    if (r.complexity < p.min_complexity) {
        if (r.complexity > 0.0f) {
            has_vectors = true;
            r.second = pf.values[1] < pt.values[1] ? pf.values[1] : pt.values[1];
        }
        if (p.strategy == 0) { r.status = ST_LOW_COMPLEXITY; return; }
        r.branch = 1;
    }
    b.participate(r.branch == 0);
    const int nf = b.n_from(), nt = b.n_to();
    if (nf == 0 || nt == 0) { r.status = icp::ST_EMPTY; return; }
    float F[12];
    int n;
    if (r.branch == 1) {
        if (!icp::loop(b, p.max_iterations, p.force_3dof, p.epsilon, F, r)) return;
        if (p.strategy == 1) limit_translation(F, guess, r.vectors, has_vectors, r.second >= p.min_complexity);
        b.set_registered(F);
        n = b.reciprocal(nf > nt);
        if (n >= icp::MIN_CORRESPONDENCES) r.variance = icp::VARIANCE_FACTOR * (double)b.median(n);
    } else {
#pragma unroll
        for (int k = 0; k < 12; ++k) F[k] = (k == 0 || k == 5 || k == 10) ? 1.0f : 0.0f;
        const float eps2 = p.epsilon * p.epsilon;
        float mse_prev = FLT_MAX;
        int stop;
        for (;;) {
            float sum_d2;
            const int c = b.correspond(sum_d2);
            if (c < icp::MIN_CORRESPONDENCES) { r.status = icp::ST_NOT_CONVERGED; r.stop = icp::STOP_FEW_CORRESPONDENCES; return; }
            const float mse = sum_d2 / (float)c;
            float T[12], G[12];
            if (!b.fit_plane(T)) { r.status = icp::ST_NOT_CONVERGED; r.stop = STOP_SINGULAR; return; }
            b.advance(T);
            compose(T, F, G);
#pragma unroll
            for (int k = 0; k < 12; ++k) F[k] = G[k];
            ++r.iterations;
            stop = icp::stop_of(T, r.iterations, p.max_iterations, eps2, mse, mse_prev);
            if (stop != icp::STOP_NONE) break;
            mse_prev = mse;
        }
        r.stop = stop;
        b.set_registered(F);                                           // the registered cloud and its normals are PCL's: before to3DoF
        b.register_normals(F);
        if (p.force_3dof) to_3dof(F);
        n = b.reciprocal_gated(nf > nt, p.gate, p.min_normal_cos);
        if (n >= 1) r.variance = icp::VARIANCE_FACTOR * (double)b.median_first(n);
    }
    r.n_correspondences = n;
    const int rf = b.rows_from(), rt = b.rows_to();
    icp::outputs(F, guess, n, rf > rt ? rf : rt, p.max_laser_scans, p.correspondence_ratio, r);
}

}  // namespace icpp
}  // namespace lcd
