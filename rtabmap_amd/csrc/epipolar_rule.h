// epipolar_rule.h -- the rule of lcd_verify_epipolar (include/lcd.h writes it down with the reference's line numbers) as functions the kernel
// (epipolar.hip) and the host mirror (rtabmap_amd/host/EpipolarGeometryHip.cpp) compile alike.  fp32, one rounded operation per statement,
// never contracted; division and square root are IEEE; only + - x / sqrt.  The seven-point solver keeps its 7 x 9 matrix in statically
// indexed locals: every loop over it has constant bounds and is unrolled, and row and column exchanges are selects, so that a lane of the
// kernel holds the matrix in registers and nothing goes to a private segment (profiles/epipolar.txt).  Internal.
#pragma once
#include "motion_rule_common.h"

namespace lcd {
namespace epi {

using m3d::bits_of;
using m3d::finite;
using m3d::float_of;
using m3d::mix;

constexpr int BISECT = 26;                   // halvings of a bracket of the cubic
constexpr int MAX_DRAWS = 32;                // draws a hypothesis may use to find its seven distinct indices
constexpr int MIN_PAIRS = 8;                 // "more than 7" (util3d_correspondences.cpp:85)
constexpr int SUMS = 4;                      // the lane partials of a normalisation pass
constexpr int ST_OK = 0, ST_FEW_PAIRS = 1, ST_NO_MODEL = 2, ST_FEW_INLIERS = 3;   // lcd_epipolar_status
constexpr float SQRT2 = 1.41421356f;

M3D_FN float mag_of(float v) { return float_of(bits_of(v) & 0x7fffffffu); }

// T = [s 0 tx; 0 s ty; 0 0 1] of one image
struct Norm { float s, tx, ty; };

// the centroid from the sums of the coordinates
M3D_FN void centroid(float sum_u, float sum_v, int m, float& cx, float& cy) {
    const float fm = (float)m;
    cx = sum_u / fm;
    cy = sum_v / fm;
}
// a point's distance from the centroid
M3D_FN float distance(float u, float v, float cx, float cy) {
    const float dx = u - cx, dy = v - cy;
    const float xx = dx * dx, yy = dy * dy;
    const float dd = xx + yy;
    return sqrtf(dd);
}
// the normalisation from the centroid and the sum of the distances; false: the mean distance is 0 or not finite
M3D_FN bool normalisation(float cx, float cy, float sum_d, int m, Norm& n) {
    const float d = sum_d / (float)m;
    n.s = 0.0f; n.tx = 0.0f; n.ty = 0.0f;
    if (!(d > 0.0f) || !finite(d)) return false;
    const float s = SQRT2 / d;
    const float sx = s * cx, sy = s * cy;
    n.s = s; n.tx = -sx; n.ty = -sy;
    return true;
}
M3D_FN void normalise(const Norm& n, float u, float v, float& x, float& y) {
    const float a = n.s * u, b = n.s * v;
    x = a + n.tx;
    y = b + n.ty;
}

// hypothesis h's seven distinct correspondence indices among m (>= 1); false: not found within MAX_DRAWS draws
M3D_FN bool draw7(uint32_t seed, uint32_t h, uint32_t m, int idx[7]) {
    const uint32_t base = mix(seed + h) * 8u;
    int got = 0;
#pragma unroll
    for (int j = 0; j < 7; ++j) idx[j] = 0;
#pragma unroll 1
    for (int k = 0; k < MAX_DRAWS; ++k) {
        const int d = (int)(mix(base + (uint32_t)k) % m);
        bool dup = false;
#pragma unroll
        for (int j = 0; j < 7; ++j) dup = dup || (j < got && d == idx[j]);
        if (dup) continue;
#pragma unroll
        for (int j = 0; j < 7; ++j) idx[j] = got == j ? d : idx[j];
        if (++got == 7) return true;
    }
    return false;
}

// the row of one normalised correspondence: (x'x, x'y, x', y'x, y'y, y', x, y, 1), x the from-image's, x' the to-image's
M3D_FN void row_of(float x, float y, float xp, float yp, float r[9]) {
    r[0] = xp * x; r[1] = xp * y; r[2] = xp;
    r[3] = yp * x; r[4] = yp * y; r[5] = yp;
    r[6] = x; r[7] = y; r[8] = 1.0f;
}

// (a b - c d) style 3 x 3 determinant with a fixed cofactor order, row-major M
M3D_FN float det3(const float M[9]) {
    const float p0 = M[4] * M[8], q0 = M[5] * M[7];
    const float p1 = M[3] * M[8], q1 = M[5] * M[6];
    const float p2 = M[3] * M[7], q2 = M[4] * M[6];
    const float m0 = p0 - q0, m1 = p1 - q1, m2 = p2 - q2;
    const float t0 = M[0] * m0, t1 = M[1] * m1, t2 = M[2] * m2;
    const float t01 = t0 - t1;
    return t01 + t2;
}

// Gauss-Jordan elimination of the 7 x 9 matrix with complete pivoting, then the two null vectors: F1 with the free columns (1, 0), F2 with
// (0, 1).  false: a pivot that is 0 or not finite.
M3D_FN bool null_space(float A[7][9], float F1[9], float F2[9]) {
    int perm[9];
#pragma unroll
    for (int c = 0; c < 9; ++c) perm[c] = c;
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        // the largest magnitude of rows k .. 6, columns k .. 8: the lowest row, then the lowest column on ties; a NaN is never chosen
        float top = -1.0f;
        int pr = k, pc = k;
#pragma unroll
        for (int r = k; r < 7; ++r)
#pragma unroll
            for (int c = k; c < 9; ++c) {
                const float a = mag_of(A[r][c]);
                const bool more = a > top;
                top = more ? a : top;
                pr = more ? r : pr;
                pc = more ? c : pc;
            }
        // row pr <-> row k (the columns before k are zero in both), column pc <-> column k
#pragma unroll
        for (int r = k + 1; r < 7; ++r) {
            const bool sw = r == pr;
#pragma unroll
            for (int c = k; c < 9; ++c) {
                const float a = A[k][c], b = A[r][c];
                A[k][c] = sw ? b : a;
                A[r][c] = sw ? a : b;
            }
        }
#pragma unroll
        for (int c = k + 1; c < 9; ++c) {
            const bool sw = c == pc;
#pragma unroll
            for (int r = 0; r < 7; ++r) {
                const float a = A[r][k], b = A[r][c];
                A[r][k] = sw ? b : a;
                A[r][c] = sw ? a : b;
            }
            const int pa = perm[k], pb = perm[c];
            perm[k] = sw ? pb : pa;
            perm[c] = sw ? pa : pb;
        }
        const float piv = A[k][k];
        ok = ok && piv != 0.0f && finite(piv);                        // (a NaN is not finite)
#pragma unroll
        for (int c = k + 1; c < 9; ++c) A[k][c] = A[k][c] / piv;
        A[k][k] = 1.0f;
#pragma unroll
        for (int r = 0; r < 7; ++r) {
            if (r == k) continue;
            const float f = A[r][k];
#pragma unroll
            for (int c = k + 1; c < 9; ++c) {
                const float p = f * A[k][c];
                A[r][c] = A[r][c] - p;
            }
            A[r][k] = 0.0f;
        }
    }
    // in the permuted order the null vectors are (-A[.][7], 1, 0) and (-A[.][8], 0, 1); entry j belongs to column perm[j]
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        float f1 = 0.0f, f2 = 0.0f;
#pragma unroll
        for (int j = 0; j < 9; ++j) {
            const float v1 = j < 7 ? -A[j < 7 ? j : 0][7] : (j == 7 ? 1.0f : 0.0f);
            const float v2 = j < 7 ? -A[j < 7 ? j : 0][8] : (j == 8 ? 1.0f : 0.0f);
            const bool here = perm[j] == i;
            f1 = here ? v1 : f1;
            f2 = here ? v2 : f2;
        }
        F1[i] = f1; F2[i] = f2;
    }
    return ok;
}

// c[0] + c[1] x + c[2] x^2 + c[3] x^3 by Horner
M3D_FN float poly3(const float c[4], float x) {
    const float a2 = c[3] * x;
    const float b2 = a2 + c[2];
    const float a1 = b2 * x;
    const float b1 = a1 + c[1];
    const float a0 = b1 * x;
    return a0 + c[0];
}

// a root of the cubic in [lo, hi] when its signs at the ends differ: BISECT halvings, then the middle of what is left
M3D_FN bool bisect(const float c[4], float lo, float hi, float& root) {
    const float plo = poly3(c, lo), phi = poly3(c, hi);
    const bool neg_lo = plo < 0.0f;
    root = hi;
    if (neg_lo == (phi < 0.0f)) return false;
    float a = lo, b = hi;
#pragma unroll 1
    for (int k = 0; k < BISECT; ++k) {
        const float s = a + b;
        const float mid = 0.5f * s;
        const float pm = poly3(c, mid);
        const bool left = (pm < 0.0f) == neg_lo;
        a = left ? mid : a;
        b = left ? b : mid;
    }
    const float s = a + b;
    root = 0.5f * s;
    return true;
}

// the coefficients of det(x F1 + F2) from four determinants; false: c3 == 0 or a coefficient that is not finite
M3D_FN bool cubic_of(const float F1[9], const float F2[9], float c[4]) {
    float P[9], M[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) { P[i] = F1[i] + F2[i]; M[i] = F2[i] - F1[i]; }
    const float d0 = det3(F2), dp = det3(P), dm = det3(M), d3 = det3(F1);
    const float s = dp + dm, d = dp - dm;
    const float hs = 0.5f * s, hd = 0.5f * d;
    c[0] = d0;
    c[1] = hd - d3;
    c[2] = hs - d0;
    c[3] = d3;
    return c[3] != 0.0f && finite(c[0]) && finite(c[1]) && finite(c[2]) && finite(c[3]);
}

// the real roots of the cubic, ascending, found in the three brackets [-B, k1], [k1, k2], [k2, B]: k1 <= k2 are the roots of the derivative
// (closed form, clamped to [-B, B]; without two real ones both are B), B = 1 + max |c_i / c3|.  Returns their number; false through `ok`:
// B is not finite.
M3D_FN int cubic_roots(const float c[4], float roots[3], bool& ok) {
    const float q0 = c[0] / c[3], q1 = c[1] / c[3], q2 = c[2] / c[3];
    const float m0 = mag_of(q0), m1 = mag_of(q1), m2 = mag_of(q2);
    const float m01 = m0 > m1 ? m0 : m1;
    const float mx = m01 > m2 ? m01 : m2;
    const float B = 1.0f + mx;
    const float nB = -B;
    roots[0] = roots[1] = roots[2] = 0.0f;
    ok = finite(B);
    if (!ok) return 0;
    const float a = 3.0f * c[3], b = 2.0f * c[2];
    const float bb = b * b, ac = a * c[1];
    const float ac4 = 4.0f * ac;
    const float disc = bb - ac4;
    float k1 = B, k2 = B;
    if (disc > 0.0f) {
        const float sq = sqrtf(disc);
        const float den = 2.0f * a;
        const float nb = -b;
        const float n1 = nb - sq, n2 = nb + sq;
        const float r1 = n1 / den, r2 = n2 / den;
        const float lo = r1 < r2 ? r1 : r2, hi = r1 < r2 ? r2 : r1;
        const float lo1 = lo < nB ? nB : lo, hi1 = hi < nB ? nB : hi;
        k1 = lo1 > B ? B : lo1;
        k2 = hi1 > B ? B : hi1;
        k1 = k1 == k1 ? k1 : B;                                        // a NaN (inf - inf) counts as absent
        k2 = k2 == k2 ? k2 : B;
    }
    int n = 0;
    float x;
    if (bisect(c, nB, k1, x)) { roots[0] = x; n = 1; }
    if (bisect(c, k1, k2, x)) { roots[0] = n == 0 ? x : roots[0]; roots[1] = n == 1 ? x : roots[1]; ++n; }
    if (bisect(c, k2, B, x)) { roots[0] = n == 0 ? x : roots[0]; roots[1] = n == 1 ? x : roots[1]; roots[2] = n == 2 ? x : roots[2]; ++n; }
    return n;
}

// F = T'^T (F^ T): first G = F^ T, then T'^T G
M3D_FN void denormalise(const float Fn[9], const Norm& nf, const Norm& nt, float F[9]) {
    float G[9];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const float a = Fn[3 * r] * nf.tx, b = Fn[3 * r + 1] * nf.ty;
        const float ab = a + b;
        G[3 * r] = Fn[3 * r] * nf.s;
        G[3 * r + 1] = Fn[3 * r + 1] * nf.s;
        G[3 * r + 2] = ab + Fn[3 * r + 2];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float a = nt.tx * G[c], b = nt.ty * G[3 + c];
        const float ab = a + b;
        F[c] = nt.s * G[c];
        F[3 + c] = nt.s * G[3 + c];
        F[6 + c] = ab + G[6 + c];
    }
}

// Candidate c = 3 h + r: hypothesis h's r-th root.  at(plane, i): plane 0, 1 the from-keypoint (u, v), 2, 3 the to-keypoint (u', v') of
// correspondence i.  model[0 .. 8] = F row-major (denormalised), model[9 .. 11] = 0.  false: the candidate is invalid.
template <class At>
M3D_FN bool candidate(uint32_t seed, uint32_t c, int m, const Norm& nf, const Norm& nt, At at, float model[12]) {
    const uint32_t h = c / 3u;
    const int r = (int)(c - 3u * h);
    int idx[7];
    if (!draw7(seed, h, (uint32_t)m, idx)) return false;
    float A[7][9];
#pragma unroll
    for (int j = 0; j < 7; ++j) {
        float x, y, xp, yp;
        normalise(nf, at(0, idx[j]), at(1, idx[j]), x, y);
        normalise(nt, at(2, idx[j]), at(3, idx[j]), xp, yp);
        row_of(x, y, xp, yp, A[j]);
    }
    float F1[9], F2[9], cf[4], roots[3];
    if (!null_space(A, F1, F2)) return false;
    if (!cubic_of(F1, F2, cf)) return false;
    bool ok;
    const int n = cubic_roots(cf, roots, ok);
    if (!ok || r >= n) return false;
    const float x = r == 0 ? roots[0] : r == 1 ? roots[1] : roots[2];
    float Fn[9], F[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        const float p = x * F1[i];
        Fn[i] = p + F2[i];
    }
    denormalise(Fn, nf, nt, F);
#pragma unroll
    for (int i = 0; i < 9; ++i) model[i] = F[i];
    model[9] = 0.0f; model[10] = 0.0f; model[11] = 0.0f;
    return true;
}

// the squared distance of p' = (pu, pv) from the line F (u, v, 1)
M3D_FN float line_error(float f0, float f1, float f2, float f3, float f4, float f5, float f6, float f7, float f8, float u, float v, float pu, float pv) {
    const float x0 = f0 * u, x1 = f1 * v;
    const float x01 = x0 + x1;
    const float lx = x01 + f2;
    const float y0 = f3 * u, y1 = f4 * v;
    const float y01 = y0 + y1;
    const float ly = y01 + f5;
    const float z0 = f6 * u, z1 = f7 * v;
    const float z01 = z0 + z1;
    const float lz = z01 + f8;
    const float a = pu * lx, b = pv * ly;
    const float ab = a + b;
    const float d = ab + lz;
    const float dd = d * d;
    const float xx = lx * lx, yy = ly * ly;
    const float n = xx + yy;
    return dd / n;
}
// an inlier of F under thr2 = thr x thr: both distances <= thr2 (the larger of the two is the error; a NaN is no inlier)
M3D_FN bool is_inlier(const float F[12], float u, float v, float up, float vp, float thr2) {
    const float e1 = line_error(F[0], F[1], F[2], F[3], F[4], F[5], F[6], F[7], F[8], u, v, up, vp);
    const float e2 = line_error(F[0], F[3], F[6], F[1], F[4], F[7], F[2], F[5], F[8], up, vp, u, v);
    return e1 <= thr2 && e2 <= thr2;
}

// the returned matrix: unit Frobenius norm (the squares added in index order), the largest-magnitude entry (the lowest index on ties) positive
M3D_FN void unit_matrix(const float F[12], float out[9]) {
    float sum = 0.0f, top = -1.0f, lead = 0.0f;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        const float q = F[i] * F[i];
        sum = sum + q;
        const float a = mag_of(F[i]);
        const bool more = a > top;
        top = more ? a : top;
        lead = more ? F[i] : lead;
    }
    const float n = sqrtf(sum);
    const float sn = lead < 0.0f ? -n : n;
#pragma unroll
    for (int i = 0; i < 9; ++i) out[i] = F[i] / sn;
}

}  // namespace epi
}  // namespace lcd
