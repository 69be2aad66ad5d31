// motion_pnp_rule.h -- the rule of lcd_estimate_motion_pnp (include/lcd.h writes it down with the reference's line numbers) as functions the
// kernel (motion_pnp.hip) and the host mirror (rtabmap_amd/host/Motion2D.cpp) compile alike.  fp32, one rounded operation per statement, never
// contracted; division and square root are IEEE; only + - x / sqrt.  The reference's thresholds, mean and variance are float here
// (util3d_motion_estimation.cpp:880-933); fp64 appears only where the reference has it: 1.1 x z (:200) and 2.1981 x median (:225).  What needs
// the correspondences as a whole is a backend's, as in motion_3d_rule.h; solve() and refine() drive either.  Internal.
#pragma once
#include "motion_3d_rule.h"                   // the sweep count of the shared three-point fit; motion_rule_common.h comes with it

namespace lcd {
namespace pnp {

using m3d::apply;
using m3d::bits_of;
using m3d::compose;
using m3d::finite;
using m3d::float_of;
using m3d::invert;
using m3d::mix;

constexpr int STEPS = 8;                     // Gauss-Newton steps of a fit (how the count was chosen)
constexpr int BISECT = 26;                   // halvings of a bracket in the minimal solver
constexpr int SUMS = 27;                     // 21 of J^T J's upper triangle, 6 of J^T r
constexpr int ST_OK = 0, ST_FEW_CORRESPONDENCES = 1, ST_NO_MODEL = 2, ST_BELOW_MIN_INLIERS = 3, ST_VARIANCE_REJECTED = 4;   // lcd_motion_pnp_status
constexpr double VARIANCE_FACTOR = 2.1981;   // util3d_motion_estimation.cpp:225, :229
constexpr float REFINE_SIGMA = 3.0f;         // util3d_motion_estimation.h:123

struct Camera {
    float fx, fy, cx, cy;
    int32_t width, height;
};

// the model a guess enters as (util3d_motion_estimation.cpp:121): (guess x local).inverse()
M3D_FN void model_of_guess(const float guess[12], bool has_local, const float local[12], float model[12]) {
    float g[12];
    if (has_local) compose(guess, local, g);
    else
        for (int k = 0; k < 12; ++k) g[k] = guess[k];
    invert(g, model);
}

// the pose a model leaves as (:154): (local x pnp).inverse()
M3D_FN void pose_of_model(const float model[12], bool has_local, const float local[12], float pose[12]) {
    float g[12];
    if (has_local) compose(local, model, g);
    else {
#pragma unroll
        for (int k = 0; k < 12; ++k) g[k] = model[k];
    }
    invert(g, pose);
}

// hypothesis h's four distinct correspondence indices among m (>= 1); false: not found within MAX_DRAWS draws
M3D_FN bool draw4(uint32_t seed, uint32_t h, uint32_t m, int& i0, int& i1, int& i2, int& i3) {
    const uint32_t base = mix(seed + h) * 4u;
    int got = 0;
    i0 = i1 = i2 = i3 = 0;
    for (int k = 0; k < m3d::MAX_DRAWS; ++k) {
        const int d = (int)(mix(base + (uint32_t)k) % m);
        if ((got > 0 && d == i0) || (got > 1 && d == i1) || (got > 2 && d == i2)) continue;
        i0 = got == 0 ? d : i0;
        i1 = got == 1 ? d : i1;
        i2 = got == 2 ? d : i2;
        i3 = got == 3 ? d : i3;
        if (++got == 4) return true;
    }
    return false;
}

// the squared reprojection error of p under a model; front: the point lies in front of the camera (Z > 0)
M3D_FN float reproj_sq(const float m[12], const Camera& k, float px, float py, float pz, float u, float v, bool& front) {
    float X, Y, Z;
    apply(m, px, py, pz, X, Y, Z);
    front = Z > 0.0f;
    const float xz = X / Z, yz = Y / Z;
    const float fxz = k.fx * xz, fyz = k.fy * yz;
    const float pu = fxz + k.cx, pv = fyz + k.cy;
    const float du = u - pu, dv = v - pv;
    const float uu = du * du, vv = dv * dv;
    return uu + vv;
}
// the reprojection error, unsquared
M3D_FN float reproj_error(const float m[12], const Camera& k, float px, float py, float pz, float u, float v, bool& front) {
    const float s = reproj_sq(m, k, px, py, pz, u, v, front);
    return sqrtf(s);
}
// an inlier under thr: in front, and the error <= thr (a NaN compares false; thr is finite)
M3D_FN bool is_inlier(float e, bool front, float thr) { return front && e <= thr; }

// ---- the minimal solver

// c[0] + c[1] x + .. + c[4] x^4 by Horner
M3D_FN float poly4(const float c[5], float x) {
    const float a3 = c[4] * x;
    const float b3 = a3 + c[3];
    const float a2 = b3 * x;
    const float b2 = a2 + c[2];
    const float a1 = b2 * x;
    const float b1 = a1 + c[1];
    const float a0 = b1 * x;
    return a0 + c[0];
}

M3D_FN float clamp01(float x) { return !(x > 0.0f) ? 0.0f : (x > 1.0f ? 1.0f : x); }

// a root of the polynomial in [lo, hi] when its signs at the ends differ: BISECT halvings, then the middle of what is left
M3D_FN bool bisect(const float c[5], float lo, float hi, float& root) {
    const float plo = poly4(c, lo), phi = poly4(c, hi);
    const bool neg_lo = plo < 0.0f;
    root = hi;
    if (neg_lo == (phi < 0.0f)) return false;
    float a = lo, b = hi;
    for (int k = 0; k < BISECT; ++k) {
        const float s = a + b;
        const float mid = 0.5f * s;
        const float pm = poly4(c, mid);
        const bool left = (pm < 0.0f) == neg_lo;
        a = left ? mid : a;
        b = left ? b : mid;
    }
    const float s = a + b;
    root = 0.5f * s;
    return true;
}

// the breakpoints 0 <= k1 <= k2 <= k3 <= 1 between which the quartic c is monotone on [0, 1]: the roots of its derivative there, found
// between the roots of its second derivative; a root that is absent is replaced by the right end of its bracket
M3D_FN void breakpoints(const float c[5], float& k1, float& k2, float& k3) {
    const float a2 = 12.0f * c[4], a1 = 6.0f * c[3], a0 = 2.0f * c[2];
    const float a11 = a1 * a1, a20 = a2 * a0;
    const float a204 = 4.0f * a20;
    const float disc = a11 - a204;
    const float sq = sqrtf(disc);                                      // NaN below zero: both roots become 0
    const float den = 2.0f * a2;
    const float na1 = -a1;
    const float n1 = na1 - sq, n2 = na1 + sq;
    const float r1 = n1 / den, r2 = n2 / den;
    const float c1 = clamp01(r1), c2 = clamp01(r2);
    const float qa = c1 < c2 ? c1 : c2, qb = c1 < c2 ? c2 : c1;
    const float d[5] = {c[1], 2.0f * c[2], 3.0f * c[3], 4.0f * c[4], 0.0f};
    (void)bisect(d, 0.0f, qa, k1);
    (void)bisect(d, qa, qb, k2);
    (void)bisect(d, qb, 1.0f, k3);
}

// P3P.  Object points P[0..2], unit bearings B[0..2]; the fourth correspondence (p4, u4, v4) picks among the solutions: the smallest error,
// the first found on ties; solutions in the order v = s3 / s1 ascending in (0, 1], then 1 / v ascending in (0, 1].  false: no solution.
M3D_FN bool p3p(const float P[3][3], const float B[3][3], float p4x, float p4y, float p4z, float u4, float v4, const Camera& cam, int sweeps,
                float best[12]) {
    // the triangle: collinear or coincident object points solve nothing
    float e1[3], e2[3], e3[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) { e1[a] = P[1][a] - P[0][a]; e2[a] = P[2][a] - P[0][a]; e3[a] = P[2][a] - P[1][a]; }
    const float cr0a = e1[1] * e2[2], cr0b = e1[2] * e2[1], cr1a = e1[2] * e2[0], cr1b = e1[0] * e2[2], cr2a = e1[0] * e2[1], cr2b = e1[1] * e2[0];
    const float cr0 = cr0a - cr0b, cr1 = cr1a - cr1b, cr2 = cr2a - cr2b;
    const float cr00 = cr0 * cr0, cr11 = cr1 * cr1, cr22 = cr2 * cr2;
    const float cr01 = cr00 + cr11;
    const float area2 = cr01 + cr22;
    if (!(area2 > 0.0f)) return false;
    float dd[3];                                                       // |P1 - P0|^2, |P2 - P0|^2, |P2 - P1|^2
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float* e = k == 0 ? e1 : k == 1 ? e2 : e3;
        const float x = e[0] * e[0], y = e[1] * e[1], z = e[2] * e[2];
        const float xy = x + y;
        dd[k] = xy + z;
    }
    const float c2 = dd[0], b2 = dd[1], a2 = dd[2];
    float cs[3];                                                       // B0.B1, B0.B2, B1.B2
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int i = k == 2 ? 1 : 0, j = k == 0 ? 1 : 2;
        const float x = B[i][0] * B[j][0], y = B[i][1] * B[j][1], z = B[i][2] * B[j][2];
        const float xy = x + y;
        cs[k] = xy + z;
    }
    const float cg = cs[0], cb = cs[1], ca = cs[2];
    // with u = s2 / s1 and v = s3 / s1: u = N(v) / D(v), and D^2 + N^2 - 2 cg N D = (c^2 / b^2) (1 - 2 cb v + v^2) D^2
    const float a2c2 = a2 - c2;
    const float K = a2c2 / b2, L = c2 / b2;
    const float Kcb = K * cb;
    const float Kcb2 = 2.0f * Kcb;
    const float n0 = K + 1.0f, n1 = -Kcb2, n2 = K - 1.0f;
    const float d0 = 2.0f * cg, ca2 = 2.0f * ca;
    const float d1 = -ca2;
    const float cb2 = 2.0f * cb;
    const float w1 = -cb2;
    const float n00 = n0 * n0, n01 = n0 * n1, n02 = n0 * n2, n11 = n1 * n1, n12 = n1 * n2, n22 = n2 * n2;
    const float n02_2 = 2.0f * n02;
    const float NN[5] = {n00, 2.0f * n01, n02_2 + n11, 2.0f * n12, n22};
    const float d00 = d0 * d0, d01 = d0 * d1, d11 = d1 * d1;
    const float DD[3] = {d00, 2.0f * d01, d11};
    const float n0d0 = n0 * d0, n0d1 = n0 * d1, n1d0 = n1 * d0, n1d1 = n1 * d1, n2d0 = n2 * d0, n2d1 = n2 * d1;
    const float ND[5] = {n0d0, n0d1 + n1d0, n1d1 + n2d0, n2d1, 0.0f};
    const float w1dd0 = w1 * DD[0], w1dd1 = w1 * DD[1], w1dd2 = w1 * DD[2];
    const float e2a = DD[2] + w1dd1;
    const float E[5] = {DD[0], DD[1] + w1dd0, e2a + DD[0], w1dd2 + DD[1], DD[2]};
    float Qc[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const float s = k < 3 ? NN[k] + DD[k] : NN[k];
        const float g = d0 * ND[k];
        const float sg = s - g;
        const float le = L * E[k];
        Qc[k] = sg - le;
    }
    bool has = false;
    float best_e = 0.0f;
#pragma unroll 1
    for (int pass = 0; pass < 2; ++pass) {
        float c[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) c[k] = pass ? Qc[4 - k] : Qc[k];
        float k1, k2, k3;
        breakpoints(c, k1, k2, k3);
#pragma unroll 1
        for (int seg = 0; seg < 4; ++seg) {
            const float lo = seg == 0 ? 0.0f : seg == 1 ? k1 : seg == 2 ? k2 : k3;
            const float hi = seg == 0 ? k1 : seg == 1 ? k2 : seg == 2 ? k3 : 1.0f;
            float x;
            if (!bisect(c, lo, hi, x)) continue;
            const float v = pass ? 1.0f / x : x;
            const float nv2 = n2 * v;
            const float nv21 = nv2 + n1;
            const float nv1 = nv21 * v;
            const float Nv = nv1 + n0;
            const float dv1 = d1 * v;
            const float Dv = dv1 + d0;
            const float u = Nv / Dv;
            const float wv1 = v + w1;
            const float wv2 = wv1 * v;
            const float Wv = wv2 + 1.0f;
            const float s1q = b2 / Wv;
            const float s1 = sqrtf(s1q);
            const float s2 = u * s1, s3 = v * s1;
            if (!(finite(s1) && finite(s2) && finite(s3) && s1 > 0.0f && s2 > 0.0f && s3 > 0.0f)) continue;
            float Q[3][3], model[12];
#pragma unroll
            for (int a = 0; a < 3; ++a) { Q[0][a] = s1 * B[0][a]; Q[1][a] = s2 * B[1][a]; Q[2][a] = s3 * B[2][a]; }
            m3d::fit3(P, Q, sweeps, model);
            bool front;
            const float e = reproj_error(model, cam, p4x, p4y, p4z, u4, v4, front);
            if (!front || !finite(e)) continue;
            if (!has || e < best_e) {
                has = true;
                best_e = e;
#pragma unroll
                for (int k = 0; k < 12; ++k) best[k] = model[k];
            }
        }
    }
    return has;
}

// the unit bearing of a pixel
M3D_FN void bearing(const Camera& k, float u, float v, float b[3]) {
    const float du = u - k.cx, dv = v - k.cy;
    const float x = du / k.fx, y = dv / k.fy;
    const float xx = x * x, yy = y * y;
    const float xy = xx + yy;
    const float n2 = xy + 1.0f;
    const float n = sqrtf(n2);
    b[0] = x / n; b[1] = y / n; b[2] = 1.0f / n;
}

// ---- the fit of an ordered set: Gauss-Newton on the pixel error, pose = unit quaternion + translation

// the quaternion of a rotation matrix (Shepperd): the largest of the four pivots, the lowest index on ties; not normalised
M3D_FN void quat_of_model(const float m[12], float q[4]) {
    const float r00 = m[0], r01 = m[1], r02 = m[2], r10 = m[4], r11 = m[5], r12 = m[6], r20 = m[8], r21 = m[9], r22 = m[10];
    const float t01 = r00 + r11, a1 = r00 - r11, a2 = r11 - r00;
    const float tr = t01 + r22, b1 = a1 - r22, b2 = a2 - r22, b3a = r22 - r00;
    const float b3 = b3a - r11;
    const float c0 = 1.0f + tr, c1 = 1.0f + b1, c2 = 1.0f + b2, c3 = 1.0f + b3;
    int pick = 0;
    float top = c0;
    if (c1 > top) { top = c1; pick = 1; }
    if (c2 > top) { top = c2; pick = 2; }
    if (c3 > top) { top = c3; pick = 3; }
    const float r = sqrtf(top);
    const float big = 0.5f * r, f = 0.5f / r;
    const float m21 = r21 - r12, m02 = r02 - r20, m10 = r10 - r01, p01 = r01 + r10, p02 = r02 + r20, p12 = r12 + r21;
    const float fm21 = m21 * f, fm02 = m02 * f, fm10 = m10 * f, fp01 = p01 * f, fp02 = p02 * f, fp12 = p12 * f;
    q[0] = pick == 0 ? big : pick == 1 ? fm21 : pick == 2 ? fm02 : fm10;
    q[1] = pick == 0 ? fm21 : pick == 1 ? big : pick == 2 ? fp01 : fp02;
    q[2] = pick == 0 ? fm02 : pick == 1 ? fp01 : pick == 2 ? big : fp12;
    q[3] = pick == 0 ? fm10 : pick == 1 ? fp02 : pick == 2 ? fp12 : big;
}

// model = [R(q / |q|) | t]; q comes back normalised
M3D_FN void model_of_pose(float q[4], const float t[3], float model[12]) {
    float R[3][3];
    m3d::quat_rotation(q[0], q[1], q[2], q[3], R);
#pragma unroll
    for (int r = 0; r < 3; ++r) { model[4 * r] = R[r][0]; model[4 * r + 1] = R[r][1]; model[4 * r + 2] = R[r][2]; model[4 * r + 3] = t[r]; }
}

// a set member's 27 terms under the model: J^T J's upper triangle row by row, then J^T r; J is the Jacobian of the predicted pixel with
// respect to (w, dt) in p' = dR(w) (R p) + t + dt, r = observed - predicted.  A member with Z <= 0 adds +0 everywhere.
M3D_FN void gn_terms(const float m[12], const Camera& k, float px, float py, float pz, float u, float v, float out[SUMS]) {
    const float mx0 = m[0] * px, mx1 = m[1] * py, mx2 = m[2] * pz;
    const float mx01 = mx0 + mx1;
    const float Mx = mx01 + mx2;
    const float my0 = m[4] * px, my1 = m[5] * py, my2 = m[6] * pz;
    const float my01 = my0 + my1;
    const float My = my01 + my2;
    const float mz0 = m[8] * px, mz1 = m[9] * py, mz2 = m[10] * pz;
    const float mz01 = mz0 + mz1;
    const float Mz = mz01 + mz2;
    const float X = Mx + m[3], Y = My + m[7], Z = Mz + m[11];
    if (!(Z > 0.0f)) {
#pragma unroll
        for (int i = 0; i < SUMS; ++i) out[i] = 0.0f;
        return;
    }
    const float iz = 1.0f / Z;
    const float x = X * iz, y = Y * iz;
    const float a = k.fx * iz, c = k.fy * iz;
    const float ax = a * x, cy = c * y;
    const float fxx = k.fx * x, fyy = k.fy * y;
    const float pu = fxx + k.cx, pv = fyy + k.cy;
    const float ru = u - pu, rv = v - pv;
    const float axMy = ax * My, aMz = a * Mz, axMx = ax * Mx, aMy = a * My;
    const float cMz = c * Mz, cyMy = cy * My, cyMx = cy * Mx, cMx = c * Mx;
    const float jv0 = cMz + cyMy;
    const float Ju[6] = {-axMy, aMz + axMx, -aMy, a, 0.0f, -ax};
    const float Jv[6] = {-jv0, cyMx, cMx, 0.0f, c, -cy};
    int o = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = i; j < 6; ++j) {
            const float p = Ju[i] * Ju[j], q = Jv[i] * Jv[j];
            out[o++] = p + q;
        }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const float p = Ju[i] * ru, q = Jv[i] * rv;
        out[o++] = p + q;
    }
}

// the 6 x 6 system of a Gauss-Newton step: motion_rule_common.h's LDL^T
M3D_FN bool gn_solve(const float S[SUMS], float delta[6]) { return m3d::ldlt6_solve(S, delta); }

// q <- (1, w / 2) (x) q (normalised by the next model_of_pose), t <- t + dt
M3D_FN void pose_update(float q[4], float t[3], const float delta[6]) {
    const float hx = 0.5f * delta[0], hy = 0.5f * delta[1], hz = 0.5f * delta[2];
    const float w = q[0], x = q[1], y = q[2], z = q[3];
    const float hxx = hx * x, hyy = hy * y, hzz = hz * z, hxw = hx * w, hyz = hy * z, hzy = hz * y;
    const float hxz = hx * z, hyw = hy * w, hzx = hz * x, hxy = hx * y, hyx = hy * x, hzw = hz * w;
    const float w1 = w - hxx, x1 = x + hxw, y1 = y - hxz, z1 = z + hxy;
    const float w2 = w1 - hyy, x2 = x1 + hyz, y2 = y1 + hyw, z2 = z1 - hyx;
    q[0] = w2 - hzz; q[1] = x2 - hzy; q[2] = y2 + hzx; q[3] = z2 + hzw;
    t[0] = t[0] + delta[3]; t[1] = t[1] + delta[4]; t[2] = t[2] + delta[5];
}

// uMean and uVariance (UMath.h:399-411, 489-502) over n >= 2 errors, then :933
M3D_FN float refined_threshold(const float* e, int n, float thr0) {
    float buf = 0.0f;
    for (int i = 0; i < n; ++i) buf = buf + e[i];
    const float mean = buf / (float)n;
    float sum = 0.0f;
    for (int i = 0; i < n; ++i) {
        const float d = e[i] - mean;
        const float dd = d * d;
        sum = sum + dd;
    }
    const float variance = sum / (float)(n - 1);
    const float sd = sqrtf(variance);
    const float s3 = REFINE_SIGMA * sd;
    return s3 < thr0 ? s3 : thr0;                                      // std::min(inlierThreshold, refineSigma * float(sqrt(variance)))
}

// ---- the covariance's inputs (util3d_motion_estimation.cpp:173-221)

// the squared distance between an inlier's object point and its point from the to-frame, and the cosine of the angle between the two
M3D_FN void cov_terms(const float pose[12], const float model[12], const float cam_pose[12], const Camera& k, float px, float py, float pz, float u,
                      float v, bool has_to, float tx, float ty, float tz, float& d2, float& cosine) {
    float nx, ny, nz;
    if (has_to && finite(tx) && finite(ty) && finite(tz)) {
        apply(pose, tx, ty, tz, nx, ny, nz);
    } else {
        float X, Y, Z;
        apply(model, px, py, pz, X, Y, Z);
        const float half_w = (float)(k.width / 2), half_h = (float)(k.height / 2);
        const float ccx = k.cx > 0.0f ? k.cx : half_w - 0.5f, ccy = k.cy > 0.0f ? k.cy : half_h - 0.5f;   // projectDepthTo3DRay (util3d.cpp:246-264)
        const float du = u - ccx, dv = v - ccy;
        const float rx = du / k.fx, ry = dv / k.fy;
        const double s = (double)Z * 1.1;
        const double sx = (double)rx * s, sy = (double)ry * s, sz = 1.0 * s;
        apply(cam_pose, (float)sx, (float)sy, (float)sz, nx, ny, nz);
    }
    const float dx = px - nx, dy = py - ny, dz = pz - nz;
    const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
    const float xy = xx + yy;
    d2 = xy + zz;
    const float a0 = px * nx, a1 = py * ny, a2 = pz * nz;
    const float a01 = a0 + a1;
    const float dot = a01 + a2;
    const float p0 = px * px, p1 = py * py, p2 = pz * pz;
    const float p01 = p0 + p1;
    const float pp = p01 + p2;
    const float q0 = nx * nx, q1 = ny * ny, q2 = nz * nz;
    const float q01 = q0 + q1;
    const float qq = q01 + q2;
    const float lp = sqrtf(pp), lq = sqrtf(qq);
    const float den = lp * lq;
    const float c = dot / den;
    cosine = !(den > 0.0f) || c != c ? 1.0f : c > 1.0f ? 1.0f : c < -1.0f ? -1.0f : c;
}

// the key a float sorts by as an unsigned integer, ascending
M3D_FN uint32_t order_key(float v) {
    const uint32_t b = bits_of(v);
    return (b & 0x80000000u) ? ~b : b | 0x80000000u;
}
M3D_FN float key_value(uint32_t k) { return float_of((k & 0x80000000u) ? k & 0x7fffffffu : ~k); }

struct Result {
    float transform[12];
    int32_t status, n_inliers, kind;
    double variance_lin, angle_cos;
};

// The backend B holds the correspondences, a current model and two index sets, `prev` and `next`.  Every call is made by all threads of a
// workgroup alike (the kernel) or by the one caller (the mirror), and returns the same value to each:
//   uint64_t ransac(float thr)     score the guess's model (candidate 0) and every hypothesis h (candidate h + 1); (count << 32) | ~candidate
//                                  of the best, 0 for none; on != 0 the model is that candidate's
//   void fit_prev()                the model becomes the fit of `prev` from the model: STEPS Gauss-Newton steps, LANES-lane sums; unchanged
//                                  when prev holds fewer than four
//   int select(float thr)          `next` = the correspondences that are inliers under thr, ascending; their errors are "the last selection"
//   float threshold(float thr0)    refined_threshold over the last selection's errors, in their order
//   void covariance(...)           over prev: kind 1 the two ranked elements, kind 2 the RMS reprojection
//   void swap_sets(); void clear_next(); int prev_n(); int next_n(); bool same_members(); const float* model()

// util3d::solvePnPRansac's refinement loop (util3d_motion_estimation.cpp:880-984), literally; afterwards the inliers are `next`
template <class B>
M3D_FN void refine(B& b, float thr0, int refine_iterations, int min_count) {
    float error_threshold = thr0;
    int it = 0;
    bool inlier_changed = false;
    int sizes[4] = {0, 0, 0, 0}, n_sizes = 0;                           // the last four of inliers_sizes, oldest first
    do {
        b.fit_prev();
        sizes[0] = sizes[1]; sizes[1] = sizes[2]; sizes[2] = sizes[3]; sizes[3] = b.prev_n(); ++n_sizes;
        const int found = b.select(error_threshold);
        if (found < min_count) {
            ++it;
            if (it >= refine_iterations) break;
            continue;
        }
        error_threshold = b.threshold(thr0);
        inlier_changed = false;
        b.swap_sets();
        if (b.next_n() != b.prev_n()) {
            if (n_sizes >= min_count && sizes[3] == sizes[1] && sizes[2] == sizes[0]) break;   // oscillating (:944: guarded by minInliersCount)
            inlier_changed = true;
            continue;
        }
        if (!b.same_members()) inlier_changed = true;
    } while (inlier_changed && ++it < refine_iterations);
}

// everything behind the correspondences: m of them
template <class B>
M3D_FN void solve(B& b, int m, int min_inliers, int refine_iterations, double reproj_error, int ratio, float max_variance, int kind, bool has_local,
                  const float local[12], Result& r) {
#pragma unroll
    for (int k = 0; k < 12; ++k) r.transform[k] = 0.0f;
    r.n_inliers = 0;
    r.kind = 0;
    r.variance_lin = 1.0;
    r.angle_cos = 1.0;
    if (m < min_inliers || m < 4) { r.status = ST_FEW_CORRESPONDENCES; return; }
    const float thr0 = (float)reproj_error;                            // util3d::solvePnPRansac takes a float
    const double thr0d = (double)thr0;
    const float thr_ransac = (float)(thr0d * thr0d);                   // solvepnp.cpp:253
    if (b.ransac(thr_ransac) == 0) { r.status = ST_NO_MODEL; return; }
    (void)b.select(thr_ransac);
    b.swap_sets();                                                     // prev = the best candidate's inliers
    b.clear_next();
    const int min_count = min_inliers < 4 ? 4 : min_inliers;           // :859-862
    if (b.prev_n() >= min_count && refine_iterations > 0) {
        refine(b, thr0, refine_iterations, min_count);
        b.swap_sets();                                                 // std::swap(inliers, new_inliers): the result is in prev again
    }
    const int n = b.prev_n();
    r.n_inliers = n;
    if (n < min_inliers) { r.status = ST_BELOW_MIN_INLIERS; return; }
    float pose[12];
    pose_of_model(b.model(), has_local, local, pose);
    double lin, cosine;
    b.covariance(kind, pose, ratio, lin, cosine);
    if (kind == 1 && max_variance > 0.0f && lin > (double)max_variance) { r.status = ST_VARIANCE_REJECTED; return; }
    r.kind = kind;
    r.variance_lin = lin;
    r.angle_cos = cosine;
#pragma unroll
    for (int k = 0; k < 12; ++k) r.transform[k] = pose[k];
    r.status = ST_OK;
}

}  // namespace pnp
}  // namespace lcd
