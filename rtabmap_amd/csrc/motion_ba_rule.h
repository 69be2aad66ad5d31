// motion_ba_rule.h -- the rule of lcd_refine_motion_ba (include/lcd.h writes it down with the reference's line numbers) as functions the kernel
// (motion_ba.hip) and the host mirror (rtabmap_amd/host/MotionBA.cpp) compile alike.  fp32, one rounded operation per statement, never
// contracted; division and square root are IEEE; only + - x / sqrt.  fp64 where the header says so: the disparity (OptimizerG2O.cpp:1880), the
// cost sums, the gain ratio and the damping factor, the normalised pixel coordinates (RegistrationVis.cpp:2154-2155).  What needs the points as
// a whole is a backend's, as in motion_pnp_rule.h; solve() drives either.  Internal.
#pragma once
#include "motion_pnp_rule.h"

namespace lcd {
namespace ba {

using m3d::apply;
using m3d::bits_of;
using m3d::compose;
using m3d::finite;
using m3d::float_of;
using m3d::invert;

constexpr int SUMS = 27;                     // 21 of the reduced camera system's upper triangle, 6 of its right-hand side
constexpr int STAGE1 = 5;                    // iterations of the first stage under a robust kernel (OptimizerG2O.cpp:1948)
constexpr int TRIALS = 10;                   // damping trials of an iteration
constexpr int PLANES = 17;                   // words of a point's state
constexpr int ST_OK = 0, ST_NO_INPUT = 1, ST_BAD_INLIER = 2, ST_DIVERGED = 3, ST_BELOW_MIN_INLIERS = 4, ST_MEAN_DISTANCE_REJECTED = 5,
              ST_DISTRIBUTION_REJECTED = 6;  // lcd_motion_ba_status
constexpr double LINEAR_EPSILON = 0.00000001, ANGULAR_EPSILON = 0.00000003;   // Registration.cpp:36-37
constexpr double CHI2_LIMIT = 1000000000000.0;                                // OptimizerG2O.cpp:1962, :2023
constexpr double GAIN_EPSILON = 1e-3, THIRD = 1.0 / 3.0;
constexpr float LAMBDA_SCALE = 1e-5f;

// a point's flags
constexpr uint32_t F_FROM = 1u, F_FROM_STEREO = 2u, F_TO_STEREO = 4u, F_FROM_OUT = 8u, F_TO_OUT = 16u, F_OUTLIER = 32u, F_TO_FINITE = 64u;

struct View {
    float fx, fy, cx, cy, b;                 // b: the baseline of a stereo edge
};

// what a pair's points share
struct Frame {
    float M1[12];                            // the fixed camera: inverse(local of the from-camera)
    View v1, v2;
    float info;                              // 1 / pixel_variance
    float delta, delta2, two_delta;          // the robust kernel; delta == 0: none
    float inf_lin, inf_ang;                  // the prior's information
};

struct Point {
    float p0[3], p[3], of[3], ot[3];         // the initial and the current estimate, the from- and the to-observation (u, v, u - disparity)
    uint32_t flags;
};

M3D_FN bool dfinite(double v) {
    uint64_t b;
    memcpy(&b, &v, 8);
    return (b & 0x7ff0000000000000ull) != 0x7ff0000000000000ull;
}

// the information of a prior variance (RegistrationVis.cpp:1893-1906): the floor, then 1 / v, as a float
inline float prior_information(double variance, double floor_) {
    const double v = variance <= floor_ ? floor_ : variance;
    const double i = 1.0 / v;
    return (float)i;
}

// An observation (RegistrationVis.cpp:1990-2017, OptimizerG2O.cpp:1859-1916): depth = z of inv_local(point), 0 without a point; a stereo edge
// iff the depth is finite and > 0 and the baseline > 0.  obs = (u, v, u - float(baseline x fx / depth)).  Returns whether the edge is stereo.
M3D_FN bool observe(const float inv_local[12], bool has_point, float px, float py, float pz, double baseline, float fx, float u, float v, float obs[3],
                    float& depth) {
    depth = 0.0f;
    if (has_point) {
        float x, y;
        apply(inv_local, px, py, pz, x, y, depth);
    }
    obs[0] = u; obs[1] = v; obs[2] = 0.0f;
    const bool stereo = finite(depth) && depth > 0.0f && baseline > 0.0;
    if (stereo) {
        const double bf = baseline * (double)fx;
        const double dd = bf / (double)depth;
        const float disparity = (float)dd;
        obs[2] = u - disparity;
    }
    return stereo;
}

// an edge under a model: the geometry the Jacobians need, the residual r = observed - projected, and chi2 = info x |r|^2
struct Proj {
    float Mx, My, Mz, a, c, ax, cy, axb;
    float r[3];
};
M3D_FN float edge(const float m[12], const View& k, bool stereo, const float p[3], const float obs[3], float info, Proj& g) {
    const float mx0 = m[0] * p[0], mx1 = m[1] * p[1], mx2 = m[2] * p[2];
    const float mx01 = mx0 + mx1;
    g.Mx = mx01 + mx2;
    const float my0 = m[4] * p[0], my1 = m[5] * p[1], my2 = m[6] * p[2];
    const float my01 = my0 + my1;
    g.My = my01 + my2;
    const float mz0 = m[8] * p[0], mz1 = m[9] * p[1], mz2 = m[10] * p[2];
    const float mz01 = mz0 + mz1;
    g.Mz = mz01 + mz2;
    const float X = g.Mx + m[3], Y = g.My + m[7], Z = g.Mz + m[11];
    const float iz = 1.0f / Z;
    const float x = X * iz, y = Y * iz;
    g.a = k.fx * iz; g.c = k.fy * iz;
    g.ax = g.a * x; g.cy = g.c * y;
    const float fxx = k.fx * x, fyy = k.fy * y;
    const float pu = fxx + k.cx, pv = fyy + k.cy;
    g.r[0] = obs[0] - pu; g.r[1] = obs[1] - pv;
    const float r00 = g.r[0] * g.r[0], r11 = g.r[1] * g.r[1];
    float s = r00 + r11;
    g.r[2] = 0.0f; g.axb = 0.0f;
    if (stereo) {
        const float Xb = X - k.b;
        const float xb = Xb * iz;
        const float fxb = k.fx * xb;
        const float pd = fxb + k.cx;
        g.r[2] = obs[2] - pd;
        g.axb = g.a * xb;
        const float r22 = g.r[2] * g.r[2];
        s = s + r22;
    }
    return info * s;
}

// Huber as IRLS: the weight and the cost of a chi2; delta == 0: no kernel
M3D_FN float huber_weight(float chi2, const Frame& f) {
    if (!(f.delta > 0.0f) || chi2 <= f.delta2) return 1.0f;
    const float s = sqrtf(chi2);
    return f.delta / s;
}
M3D_FN float huber_cost(float chi2, const Frame& f) {
    if (!(f.delta > 0.0f) || chi2 <= f.delta2) return chi2;
    const float s = sqrtf(chi2);
    const float a = f.two_delta * s;
    return a - f.delta2;
}

M3D_FN bool from_active(uint32_t flags) { return (flags & (F_FROM | F_FROM_OUT)) == F_FROM; }
M3D_FN bool to_active(uint32_t flags) { return (flags & F_TO_OUT) == 0u; }

// a point's robust cost under the moving camera's model, and the chi2 of its two edges (0 for an edge that is not active)
M3D_FN double point_cost(const Frame& f, const float m2[12], const Point& pt, float& chi_from, float& chi_to) {
    double cost = 0.0;
    chi_from = 0.0f; chi_to = 0.0f;
    Proj g;
    if (from_active(pt.flags)) {
        chi_from = edge(f.M1, f.v1, (pt.flags & F_FROM_STEREO) != 0u, pt.p, pt.of, f.info, g);
        const float c = huber_cost(chi_from, f);
        cost = cost + (double)c;
    }
    if (to_active(pt.flags)) {
        chi_to = edge(m2, f.v2, (pt.flags & F_TO_STEREO) != 0u, pt.p, pt.ot, f.info, g);
        const float c = huber_cost(chi_to, f);
        cost = cost + (double)c;
    }
    return cost;
}

// a point's part of the normal equations: its 3 x 3 block (upper triangle) and gradient, the 6 x 3 coupling to the moving camera, and its
// part of that camera's 6 x 6 block (upper triangle) and gradient
struct Blocks {
    float Hpp[6], bp[3], Hcp[18], Hcc[21], bc[6];
};

// the sum over an edge's rows of A_k B_k: two rows, the third with a stereo edge
M3D_FN float rows_dot(const float A[3], const float B[3], bool stereo) {
    const float p0 = A[0] * B[0], p1 = A[1] * B[1];
    float s = p0 + p1;
    if (stereo) {
        const float p2 = A[2] * B[2];
        s = s + p2;
    }
    return s;
}

// one edge into the blocks, weight W = info x the kernel's weight; `moving`: the edge of the camera that is estimated
M3D_FN void edge_blocks(const float m[12], const Proj& g, bool stereo, float W, bool moving, Blocks& B) {
    float Jp[3][3];                                                    // [parameter][row]
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float am = g.a * m[j], axm = g.ax * m[8 + j], cm = g.c * m[4 + j], cym = g.cy * m[8 + j], axbm = g.axb * m[8 + j];
        Jp[j][0] = am - axm;
        Jp[j][1] = cm - cym;
        Jp[j][2] = am - axbm;
    }
    int o = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = i; j < 3; ++j) {
            const float s = rows_dot(Jp[i], Jp[j], stereo);
            const float e = W * s;
            B.Hpp[o] = B.Hpp[o] + e;
            ++o;
        }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float s = rows_dot(Jp[i], g.r, stereo);
        const float e = W * s;
        B.bp[i] = B.bp[i] + e;
    }
    if (!moving) return;
    const float axMy = g.ax * g.My, aMz = g.a * g.Mz, axMx = g.ax * g.Mx, aMy = g.a * g.My;
    const float cMz = g.c * g.Mz, cyMy = g.cy * g.My, cyMx = g.cy * g.Mx, cMx = g.c * g.Mx;
    const float axbMy = g.axb * g.My, axbMx = g.axb * g.Mx;
    const float jv0 = cMz + cyMy;
    const float Jc[6][3] = {{-axMy, -jv0, -axbMy}, {aMz + axMx, cyMx, aMz + axbMx}, {-aMy, cMx, -aMy}, {g.a, 0.0f, g.a}, {0.0f, g.c, 0.0f},
                            {-g.ax, -g.cy, -g.axb}};
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const float s = rows_dot(Jc[i], Jp[j], stereo);
            const float e = W * s;
            B.Hcp[3 * i + j] = B.Hcp[3 * i + j] + e;
        }
    o = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = i; j < 6; ++j) {
            const float s = rows_dot(Jc[i], Jc[j], stereo);
            const float e = W * s;
            B.Hcc[o] = B.Hcc[o] + e;
            ++o;
        }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const float s = rows_dot(Jc[i], g.r, stereo);
        const float e = W * s;
        B.bc[i] = B.bc[i] + e;
    }
}

// a point's blocks under the moving camera's model; false (all zero): no active edge
M3D_FN bool point_blocks(const Frame& f, const float m2[12], const Point& pt, Blocks& B) {
#pragma unroll
    for (int i = 0; i < 6; ++i) { B.Hpp[i] = 0.0f; B.bc[i] = 0.0f; }
#pragma unroll
    for (int i = 0; i < 3; ++i) B.bp[i] = 0.0f;
#pragma unroll
    for (int i = 0; i < 18; ++i) B.Hcp[i] = 0.0f;
#pragma unroll
    for (int i = 0; i < 21; ++i) B.Hcc[i] = 0.0f;
    Proj g;
    const bool fa = from_active(pt.flags), ta = to_active(pt.flags);
    if (fa) {
        const bool stereo = (pt.flags & F_FROM_STEREO) != 0u;
        const float chi2 = edge(f.M1, f.v1, stereo, pt.p, pt.of, f.info, g);
        const float w = huber_weight(chi2, f);
        const float W = f.info * w;
        edge_blocks(f.M1, g, stereo, W, false, B);
    }
    if (ta) {
        const bool stereo = (pt.flags & F_TO_STEREO) != 0u;
        const float chi2 = edge(m2, f.v2, stereo, pt.p, pt.ot, f.info, g);
        const float w = huber_weight(chi2, f);
        const float W = f.info * w;
        edge_blocks(m2, g, stereo, W, true, B);
    }
    return fa || ta;
}

// the inverse of (Hpp + lambda I) by cofactors, upper triangle
M3D_FN void inv3(const float H[6], float lambda, float inv[6]) {
    const float a = H[0] + lambda, b = H[1], c = H[2], d = H[3] + lambda, e = H[4], f = H[5] + lambda;
    const float df = d * f, ee = e * e, ce = c * e, bf = b * f, be = b * e, cd = c * d, af = a * f, cc = c * c, bc = b * c, ae = a * e, ad = a * d, bb = b * b;
    const float c00 = df - ee, c01 = ce - bf, c02 = be - cd, c11 = af - cc, c12 = bc - ae, c22 = ad - bb;
    const float t0 = a * c00, t1 = b * c01, t2 = c * c02;
    const float t01 = t0 + t1;
    const float det = t01 + t2;
    inv[0] = c00 / det; inv[1] = c01 / det; inv[2] = c02 / det; inv[3] = c11 / det; inv[4] = c12 / det; inv[5] = c22 / det;
}
M3D_FN float sym3(const float s[6], int i, int j) { return s[i == 0 ? j : j == 0 ? i : i + j + 1]; }   // (0,0) (0,1) (0,2) (1,1) (1,2) (2,2)

// a point's 27 terms of the reduced camera system (the Schur complement of its block)
M3D_FN void point_terms(const Blocks& B, float lambda, float terms[SUMS]) {
    float inv[6], Y[6][3];
    inv3(B.Hpp, lambda, inv);
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float y0 = B.Hcp[3 * i] * sym3(inv, 0, a), y1 = B.Hcp[3 * i + 1] * sym3(inv, 1, a), y2 = B.Hcp[3 * i + 2] * sym3(inv, 2, a);
            const float y01 = y0 + y1;
            Y[i][a] = y01 + y2;
        }
    int o = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = i; j < 6; ++j) {
            const float y0 = Y[i][0] * B.Hcp[3 * j], y1 = Y[i][1] * B.Hcp[3 * j + 1], y2 = Y[i][2] * B.Hcp[3 * j + 2];
            const float y01 = y0 + y1;
            const float y012 = y01 + y2;
            terms[o] = B.Hcc[o] - y012;
            ++o;
        }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const float y0 = Y[i][0] * B.bp[0], y1 = Y[i][1] * B.bp[1], y2 = Y[i][2] * B.bp[2];
        const float y01 = y0 + y1;
        const float y012 = y01 + y2;
        terms[21 + i] = B.bc[i] - y012;
    }
}

// back-substitution: the point's step under the camera's step dc, and its part of the gain ratio's denominator
M3D_FN void point_step(const Blocks& B, float lambda, const float dc[6], float dp[3], double& scale) {
    float inv[6], v[3];
    inv3(B.Hpp, lambda, inv);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        float s = B.Hcp[a] * dc[0];
#pragma unroll
        for (int i = 1; i < 6; ++i) {
            const float p = B.Hcp[3 * i + a] * dc[i];
            s = s + p;
        }
        v[a] = B.bp[a] - s;
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float d0 = sym3(inv, a, 0) * v[0], d1 = sym3(inv, a, 1) * v[1], d2 = sym3(inv, a, 2) * v[2];
        const float d01 = d0 + d1;
        dp[a] = d01 + d2;
    }
    scale = 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double ld = (double)lambda * (double)dp[a];
        const double lb = ld + (double)B.bp[a];
        const double t = (double)dp[a] * lb;
        scale = scale + t;
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const double t = (double)dc[i] * (double)B.bc[i];
        scale = scale + t;
    }
}

// ---- the camera-to-camera edge: E = model x C0, C0 the camera's initial pose; error = (translation of E, twice the vector part of E's unit
// quaternion with w >= 0); information diag(inf_lin x 3, inf_ang x 3)
struct Prior {
    float e[6];
    float P[SUMS];                                                     // its part of the camera system: J^T W J's upper triangle, then -J^T W e
};
M3D_FN void prior_error(const float model[12], const float C0[12], float e[6], float q[4], float rt[3]) {
    float E[12];
    compose(model, C0, E);
    e[0] = E[3]; e[1] = E[7]; e[2] = E[11];
    pnp::quat_of_model(E, q);
    const float s0 = q[0] * q[0], s1 = q[1] * q[1], s2 = q[2] * q[2], s3 = q[3] * q[3];
    const float s01 = s0 + s1;
    const float s012 = s01 + s2;
    const float n2 = s012 + s3;
    const float n = sqrtf(n2);
    const float sn = q[0] < 0.0f ? -n : n;
    q[0] = q[0] / sn; q[1] = q[1] / sn; q[2] = q[2] / sn; q[3] = q[3] / sn;
    e[3] = 2.0f * q[1]; e[4] = 2.0f * q[2]; e[5] = 2.0f * q[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const float a = model[4 * r] * C0[3], b = model[4 * r + 1] * C0[7], c = model[4 * r + 2] * C0[11];
        const float ab = a + b;
        rt[r] = ab + c;
    }
}
M3D_FN double prior_cost(const Frame& f, const float e[6]) {
    const float t0 = e[0] * e[0], t1 = e[1] * e[1], t2 = e[2] * e[2], r0 = e[3] * e[3], r1 = e[4] * e[4], r2 = e[5] * e[5];
    const float t01 = t0 + t1, r01 = r0 + r1;
    const float st = t01 + t2, sr = r01 + r2;
    const float ct = f.inf_lin * st, cr = f.inf_ang * sr;
    const float c = ct + cr;
    return (double)c;
}
M3D_FN void prior_system(const Frame& f, const float model[12], const float C0[12], Prior& pr) {
    float q[4], rt[3];
    prior_error(model, C0, pr.e, q, rt);
    // rows: the error's six components; columns: (w, dt)
    const float J[6][6] = {{0.0f, rt[2], -rt[1], 1.0f, 0.0f, 0.0f}, {-rt[2], 0.0f, rt[0], 0.0f, 1.0f, 0.0f}, {rt[1], -rt[0], 0.0f, 0.0f, 0.0f, 1.0f},
                           {q[0], q[3], -q[2], 0.0f, 0.0f, 0.0f},   {-q[3], q[0], q[1], 0.0f, 0.0f, 0.0f},  {q[2], -q[1], q[0], 0.0f, 0.0f, 0.0f}};
    int o = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = i; j < 6; ++j) {
            float acc = 0.0f;
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                const float jj = J[k][i] * J[k][j];
                const float p = (k < 3 ? f.inf_lin : f.inf_ang) * jj;
                acc = acc + p;
            }
            pr.P[o++] = acc;
        }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        float acc = 0.0f;
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const float je = J[k][i] * pr.e[k];
            const float p = (k < 3 ? f.inf_lin : f.inf_ang) * je;
            acc = acc - p;
        }
        pr.P[21 + i] = acc;
    }
}

// thread 0's part of a trial: the 27 sums and the prior into the damped system, its solution, the new pose (q, t) and its part of the gain
// ratio's denominator.  false: no solution, q and t untouched
M3D_FN bool camera_step(const Frame& f, const float sums[SUMS], const Prior& pr, float lambda, float q[4], float t[3], float dc[6], double& scale) {
    float S[SUMS];
#pragma unroll
    for (int c = 0; c < SUMS; ++c) S[c] = sums[c] + pr.P[c];
    int o = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        S[o] = S[o] + lambda;
        o += 6 - i;
    }
    if (!m3d::ldlt6_solve(S, dc)) return false;
    pnp::pose_update(q, t, dc);
    scale = 0.0;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const double ld = (double)lambda * (double)dc[i];
        const double lb = ld + (double)pr.P[21 + i];
        const double tt = (double)dc[i] * lb;
        scale = scale + tt;
    }
    return true;
}

// the index of diagonal entry i in a 6 x 6 upper triangle stored row by row
M3D_FN int diag6(int i) { return i * 6 - (i * (i - 1)) / 2; }

// ---- the gates (RegistrationVis.cpp:2090-2188)

// the smaller eigenvalue of the symmetric 2 x 2 (a, b; b, c)
M3D_FN float small_eigenvalue(float a, float b, float c) {
    const float apc = a + c, amc = a - c;
    const float half = 0.5f * apc, d = 0.5f * amc;
    const float dd = d * d, bb = b * b;
    const float s = dd + bb;
    const float root = sqrtf(s);
    return half - root;
}
// the normalised pixel coordinate (:2154-2155): float((double(u) - double(c)) / double(size))
M3D_FN float normalised(float u, float c, int32_t size) {
    const double d = (double)u - (double)c;
    const double n = d / (double)size;
    return (float)n;
}

struct Params {
    int min_inliers, iterations;
    float max_mean_distance, min_distribution;
    bool distribution_valid;                                           // the to-camera isValidForReprojection (CameraModel.h:88)
    bool has_to_xyz;
    bool has_local;                                                    // of the to-camera
};
struct Result {
    float transform[12];
    int32_t status, n_inliers, n_outliers, lm_accepted;
    double chi2_before, chi2_after;
    float mean_distance, distribution;
};

// The backend B holds the points' state and the moving camera's pose.  Every call is made by all threads of a workgroup alike (the kernel) or
// by the one caller (the mirror), and returns the same value to each:
//   double cost()                          the robust cost of the state: the active edges' lane-and-tree sum in fp64, plus the prior's
//   float max_diagonal()                   the largest diagonal entry of the undamped normal equations
//   bool trial(lambda, F, scale)           saves the state, solves the damped system, moves pose and points; F the new cost, scale the
//                                          denominator delta^T (lambda delta + b); false: no solution, the state is unchanged
//   void restore()                         back to the saved state
//   void accept()                          the moved state is the state
//   void flag_outliers()                   OptimizerG2O.cpp:1968-2015 over the active edges
//   int survivors()                        compacts the ids of the points that are not outliers; their number
//   float mean_distance(int n, bool& any)  uMean over the survivors' finite to-points' depths
//   float distribution(int n)              the smaller eigenvalue over the survivors' normalised to-keypoints
//   const float* model()
template <class B>
M3D_FN void solve(B& b, int n, const Frame& f, const Params& p, const float transform0[12], const float local[12], Result& r) {
#pragma unroll
    for (int k = 0; k < 12; ++k) r.transform[k] = 0.0f;
    r.n_inliers = n; r.n_outliers = 0; r.lm_accepted = 0;
    r.chi2_before = 0.0; r.chi2_after = 0.0;
    r.mean_distance = 0.0f; r.distribution = 0.0f;
    r.status = ST_OK;
    if (p.iterations > 0) {
        const int stages = f.delta > 0.0f ? 2 : 1;
        double F = b.cost();
        r.chi2_before = F;
        bool diverged = false;
        for (int s = 0; s < stages && !diverged; ++s) {
            const int iters = s == 0 && stages == 2 ? STAGE1 : p.iterations;
            if (s > 0) F = b.cost();
            const float top = b.max_diagonal();
            float lambda = LAMBDA_SCALE * top, nu = 2.0f;
            for (int it = 0; it < iters; ++it) {
                bool accepted = false;
                for (int trial = 0; trial < TRIALS && !accepted; ++trial) {
                    double Fn = 0.0, scale = 0.0;
                    if (b.trial(lambda, Fn, scale)) {
                        const double gain = F - Fn;
                        const double den = scale + GAIN_EPSILON;
                        const double rho = gain / den;
                        if (rho > 0.0 && dfinite(Fn)) {
                            b.accept();
                            F = Fn;
                            const double t2 = 2.0 * rho;
                            const double t = t2 - 1.0;
                            const double tt = t * t;
                            const double ttt = tt * t;
                            const double alpha = 1.0 - ttt;
                            const double factor = alpha < THIRD ? THIRD : alpha;
                            const double l = (double)lambda * factor;
                            lambda = (float)l;
                            nu = 2.0f;
                            accepted = true;
                            ++r.lm_accepted;
                        } else {
                            b.restore();
                        }
                    }
                    if (!accepted) {
                        lambda = lambda * nu;
                        nu = nu * 2.0f;
                    }
                }
                if (!accepted) break;
            }
            r.chi2_after = F;
            if (F != F || (s > 0 && (F > CHI2_LIMIT || !dfinite(F)))) diverged = true;        // OptimizerG2O.cpp:1954, :1962
            else if (stages == 2) b.flag_outliers();
        }
        if (diverged || F > CHI2_LIMIT) { r.status = ST_DIVERGED; return; }                   // :2023
    }
    const int kept = b.survivors();
    r.n_outliers = n - kept;
    r.n_inliers = kept;
    if (kept < p.min_inliers) { r.status = ST_BELOW_MIN_INLIERS; return; }                    // RegistrationVis.cpp:2054
    if (kept > 0 && p.max_mean_distance > 0.0f && p.has_to_xyz) {
        bool any;
        const float mean = b.mean_distance(kept, any);
        if (any) {
            r.mean_distance = mean;
            if (mean > p.max_mean_distance) { r.status = ST_MEAN_DISTANCE_REJECTED; return; }
        }
    }
    if (kept > 0 && p.min_distribution > 0.0f && p.distribution_valid) {
        r.distribution = b.distribution(kept);
        if (r.distribution < p.min_distribution) { r.status = ST_DISTRIBUTION_REJECTED; return; }
    }
    if (p.iterations > 0) {
        pnp::pose_of_model(b.model(), p.has_local, local, r.transform);                       // OptimizerG2O.cpp:2049
    } else {
#pragma unroll
        for (int k = 0; k < 12; ++k) r.transform[k] = transform0[k];
    }
}

}  // namespace ba
}  // namespace lcd
