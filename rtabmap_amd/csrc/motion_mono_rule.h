// motion_mono_rule.h -- the rule of lcd_estimate_motion_mono (include/lcd.h writes it down with the reference's line numbers) as functions the
// kernel (motion_mono.hip) and the host mirror (rtabmap_amd/host/MotionMono.cpp) compile alike.  The five-point solver, the decomposition of E
// and the triangulation are fp64; the normalised coordinates, the scoring and everything behind the triangulated point are fp32.  One rounded
// operation per statement, never contracted; division and square root are IEEE; only + - x / sqrt.
//   The solver's arrays are too large for a lane's registers (the 10 x 20 constraint matrix alone is 1 600 bytes), so every indexed value
//   lives in a workspace of WS doubles that the caller provides through an accessor ws(e): the kernel gives each hypothesis of a chunk a
//   lane-interleaved column of LDS, the mirror a plain array.  Locals are scalars only: nothing goes to a private segment
//   (profiles/motion_mono.txt).  Internal.
#pragma once
#include "motion_rule_common.h"

namespace lcd {
namespace mono {

using m3d::bits_of;
using m3d::finite;
using m3d::float_of;
using m3d::mix;

constexpr int BISECT = 56;                   // halvings of a bracket of a polynomial (LCD_MONO_BISECT)
constexpr int MAX_DRAWS = 32;                // draws a hypothesis may use to find its five distinct indices
constexpr int MIN_PAIRS = 9;                 // "pairsFound > 8" (util3d_features.cpp:226)
constexpr int ROOTS = 10;                    // candidates per hypothesis: the degree of the polynomial in z
constexpr double VARIANCE_FACTOR = 2.1981;   // util3d_features.cpp:350, :374
constexpr int ST_OK = 0, ST_FEW_FEATURES = 1, ST_FEW_PAIRS = 2, ST_NO_MODEL = 3, ST_FEW_INLIERS = 4, ST_HIGH_VARIANCE = 5;   // lcd_motion_mono_status

// the workspace, in doubles
constexpr int WS = 256;
constexpr int WS_M = 0;                      // the 10 x 20 constraint matrix, row-major; before it the 5 x 9 matrix of the null space; behind it:
constexpr int WS_B = 0;                      //   B(z): three rows of 13 coefficients (x: z^0 .. z^3, y: z^0 .. z^3, 1: z^0 .. z^4)
constexpr int WS_MINOR = 40;                 //   a 2 x 2 minor of B(z): 8 coefficients
constexpr int WS_D = 60;                     //   the polynomial and its nine derivatives, 11 coefficients each
constexpr int WS_RA = 170, WS_RB = 181;      //   the roots of two successive derivatives
constexpr int WS_BASIS = 200;                // X, Y, Z, W: four null vectors of nine entries
constexpr int WS_T = 236;                    // tr(E E^T) / 2: ten quadratic coefficients
constexpr int WS_Q = 246;                    // a quadratic temporary

M3D_FN uint64_t dbits_of(double v) { uint64_t b; memcpy(&b, &v, 8); return b; }
M3D_FN double double_of(uint64_t b) { double v; memcpy(&v, &b, 8); return v; }
M3D_FN bool dfinite(double v) { return (dbits_of(v) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull; }
M3D_FN double dmag(double v) { return double_of(dbits_of(v) & 0x7fffffffffffffffull); }

// monomials.  Linear: x, y, z, 1.  Quadratic: x2 y2 z2 xy xz yz x y z 1.  Cubic, the ten that are eliminated first: x3 y3 x2y xy2 x2z x2 y2z
// y2 xyz xy | xz2 xz x yz2 yz y z3 z2 z 1.
M3D_FN int quad_index(int i, int j) {
    const int T[4][4] = {{0, 3, 4, 6}, {3, 1, 5, 7}, {4, 5, 2, 8}, {6, 7, 8, 9}};
    return T[i][j];
}
M3D_FN int cubic_index(int q, int l) {
    const int T[10][4] = {{0, 2, 4, 5}, {3, 1, 6, 7}, {10, 13, 16, 17}, {2, 3, 8, 9}, {4, 8, 10, 11}, {8, 6, 13, 14}, {5, 9, 11, 12}, {9, 7, 14, 15}, {11, 14, 17, 18}, {12, 15, 18, 19}};
    return T[q][l];
}

// the normalised coordinate (u - c) / f
M3D_FN float normalised(float u, float c, float f) {
    const float d = u - c;
    return d / f;
}
// threshold /= (fx + fy) / 2 in double (five-point.cpp:439), squared, as a float
M3D_FN float threshold2(double thr, float fx, float fy) {
    const double s = (double)fx + (double)fy;
    const double h = s / 2.0;
    const double t = thr / h;
    const double tt = t * t;
    return (float)tt;
}

// hypothesis h's five distinct correspondence indices among m (>= 1); false: not found within MAX_DRAWS draws
M3D_FN bool draw5(uint32_t seed, uint32_t h, uint32_t m, int idx[5]) {
    const uint32_t base = mix(seed + h) * 8u;
    int got = 0;
#pragma unroll
    for (int j = 0; j < 5; ++j) idx[j] = 0;
#pragma unroll 1
    for (int k = 0; k < MAX_DRAWS; ++k) {
        const int d = (int)(mix(base + (uint32_t)k) % m);
        bool dup = false;
#pragma unroll
        for (int j = 0; j < 5; ++j) dup = dup || (j < got && d == idx[j]);
        if (dup) continue;
#pragma unroll
        for (int j = 0; j < 5; ++j) idx[j] = got == j ? d : idx[j];
        if (++got == 5) return true;
    }
    return false;
}

// Gauss-Jordan elimination of the 5 x 9 matrix at WS_M (row-major) with complete pivoting, then the four null vectors into WS_BASIS: X has
// the free columns (1, 0, 0, 0), Y (0, 1, 0, 0), Z (0, 0, 1, 0), W (0, 0, 0, 1).  false: a pivot that is 0 or not finite.
template <class W>
M3D_FN bool null_space(W ws) {
    uint64_t perm = 0x876543210ull;                                    // four bits per column
#pragma unroll 1
    for (int k = 0; k < 5; ++k) {
        // the largest magnitude of rows k .. 4, columns k .. 8: the lowest row, then the lowest column on ties; a NaN is never chosen
        double top = -1.0;
        int pr = k, pc = k;
#pragma unroll 1
        for (int r = k; r < 5; ++r)
#pragma unroll 1
            for (int c = k; c < 9; ++c) {
                const double a = dmag(ws(WS_M + 9 * r + c));
                const bool more = a > top;
                top = more ? a : top;
                pr = more ? r : pr;
                pc = more ? c : pc;
            }
#pragma unroll 1
        for (int c = 0; c < 9; ++c) {
            const double a = ws(WS_M + 9 * k + c), b = ws(WS_M + 9 * pr + c);
            ws(WS_M + 9 * k + c) = b;
            ws(WS_M + 9 * pr + c) = a;
        }
#pragma unroll 1
        for (int r = 0; r < 5; ++r) {
            const double a = ws(WS_M + 9 * r + k), b = ws(WS_M + 9 * r + pc);
            ws(WS_M + 9 * r + k) = b;
            ws(WS_M + 9 * r + pc) = a;
        }
        const uint64_t pa = (perm >> (4 * k)) & 15ull, pb = (perm >> (4 * pc)) & 15ull;
        perm = perm ^ ((pa ^ pb) << (4 * k)) ^ ((pa ^ pb) << (4 * pc));
        const double piv = ws(WS_M + 9 * k + k);
        if (piv == 0.0 || !dfinite(piv)) return false;                 // (a NaN is not finite)
#pragma unroll 1
        for (int c = k + 1; c < 9; ++c) ws(WS_M + 9 * k + c) = ws(WS_M + 9 * k + c) / piv;
        ws(WS_M + 9 * k + k) = 1.0;
#pragma unroll 1
        for (int r = 0; r < 5; ++r) {
            if (r == k) continue;
            const double f = ws(WS_M + 9 * r + k);
#pragma unroll 1
            for (int c = k + 1; c < 9; ++c) {
                const double p = f * ws(WS_M + 9 * k + c);
                ws(WS_M + 9 * r + c) = ws(WS_M + 9 * r + c) - p;
            }
            ws(WS_M + 9 * r + k) = 0.0;
        }
    }
    // in the permuted order null vector b is (-A[.][5 + b], e_b); entry j belongs to column perm[j]
#pragma unroll 1
    for (int b = 0; b < 4; ++b)
#pragma unroll 1
        for (int j = 0; j < 9; ++j) {
            const int col = (int)((perm >> (4 * j)) & 15ull);
            const double v = j < 5 ? -ws(WS_M + 9 * j + 5 + b) : (j == 5 + b ? 1.0 : 0.0);
            ws(WS_BASIS + 9 * b + col) = v;
        }
    return true;
}

// coefficient k (x, y, z, 1) of E's entry e (row-major)
template <class W>
M3D_FN double e_coef(W ws, int e, int k) { return ws(WS_BASIS + 9 * k + e); }

// Q +- (entry ea) x (entry eb): linear times linear, the products in the order of the loops
template <class W>
M3D_FN void quad_mac(W ws, int ea, int eb, bool neg) {
#pragma unroll 1
    for (int i = 0; i < 4; ++i)
#pragma unroll 1
        for (int j = 0; j < 4; ++j) {
            const double p = e_coef(ws, ea, i) * e_coef(ws, eb, j);
            const int q = WS_Q + quad_index(i, j);
            ws(q) = neg ? ws(q) - p : ws(q) + p;
        }
}
template <class W>
M3D_FN void quad_zero(W ws) {
#pragma unroll 1
    for (int q = 0; q < 10; ++q) ws(WS_Q + q) = 0.0;
}
// row +- Q x (entry e): quadratic times linear
template <class W>
M3D_FN void cubic_mac(W ws, int row, int e, bool neg) {
#pragma unroll 1
    for (int q = 0; q < 10; ++q)
#pragma unroll 1
        for (int l = 0; l < 4; ++l) {
            const double p = ws(WS_Q + q) * e_coef(ws, e, l);
            const int c = WS_M + 20 * row + cubic_index(q, l);
            ws(c) = neg ? ws(c) - p : ws(c) + p;
        }
}

// the ten constraints on E = x X + y Y + z Z + W as rows of the 10 x 20 matrix: row 0 is det E, row 1 + 3 i + j the entry (i, j) of
// (E E^T - tr(E E^T) / 2) E
template <class W>
M3D_FN void constraints(W ws) {
#pragma unroll 1
    for (int c = 0; c < 200; ++c) ws(WS_M + c) = 0.0;
    // det E by the first row's cofactors
    quad_zero(ws); quad_mac(ws, 4, 8, false); quad_mac(ws, 5, 7, true); cubic_mac(ws, 0, 0, false);
    quad_zero(ws); quad_mac(ws, 3, 8, false); quad_mac(ws, 5, 6, true); cubic_mac(ws, 0, 1, true);
    quad_zero(ws); quad_mac(ws, 3, 7, false); quad_mac(ws, 4, 6, true); cubic_mac(ws, 0, 2, false);
    // T = tr(E E^T) / 2
    quad_zero(ws);
#pragma unroll 1
    for (int e = 0; e < 9; ++e) quad_mac(ws, e, e, false);
#pragma unroll 1
    for (int q = 0; q < 10; ++q) ws(WS_T + q) = 0.5 * ws(WS_Q + q);
#pragma unroll 1
    for (int i = 0; i < 3; ++i)
#pragma unroll 1
        for (int j = 0; j < 3; ++j)
#pragma unroll 1
            for (int k = 0; k < 3; ++k) {
                quad_zero(ws);
#pragma unroll 1
                for (int n = 0; n < 3; ++n) quad_mac(ws, 3 * i + n, 3 * k + n, false);
                if (k == i) {
#pragma unroll 1
                    for (int q = 0; q < 10; ++q) ws(WS_Q + q) = ws(WS_Q + q) - ws(WS_T + q);
                }
                cubic_mac(ws, 1 + 3 * i + j, 3 * k + j, false);
            }
}

// Gauss-Jordan elimination of the first ten columns of the 10 x 20 matrix, the pivot the largest magnitude of its column in rows k .. 9 (the
// lowest row on ties; a NaN is never chosen).  false: a pivot that is 0 or not finite.
template <class W>
M3D_FN bool eliminate(W ws) {
#pragma unroll 1
    for (int k = 0; k < 10; ++k) {
        double top = -1.0;
        int pr = k;
#pragma unroll 1
        for (int r = k; r < 10; ++r) {
            const double a = dmag(ws(WS_M + 20 * r + k));
            const bool more = a > top;
            top = more ? a : top;
            pr = more ? r : pr;
        }
#pragma unroll 1
        for (int c = k; c < 20; ++c) {
            const double a = ws(WS_M + 20 * k + c), b = ws(WS_M + 20 * pr + c);
            ws(WS_M + 20 * k + c) = b;
            ws(WS_M + 20 * pr + c) = a;
        }
        const double piv = ws(WS_M + 20 * k + k);
        if (piv == 0.0 || !dfinite(piv)) return false;
#pragma unroll 1
        for (int c = k + 1; c < 20; ++c) ws(WS_M + 20 * k + c) = ws(WS_M + 20 * k + c) / piv;
        ws(WS_M + 20 * k + k) = 1.0;
#pragma unroll 1
        for (int r = 0; r < 10; ++r) {
            if (r == k) continue;
            const double f = ws(WS_M + 20 * r + k);
#pragma unroll 1
            for (int c = k + 1; c < 20; ++c) {
                const double p = f * ws(WS_M + 20 * k + c);
                ws(WS_M + 20 * r + c) = ws(WS_M + 20 * r + c) - p;
            }
            ws(WS_M + 20 * r + k) = 0.0;
        }
    }
    return true;
}

// B(z): row r = (row 4 + 2 r) - z (row 5 + 2 r) of the eliminated matrix, whose leading monomials cancel; per row the coefficient of x (degree
// 3 in z), of y (degree 3) and the constant (degree 4), ascending in z
template <class W>
M3D_FN void b_rows(W ws) {
#pragma unroll 1
    for (int r = 0; r < 3; ++r) {
        const int a = WS_M + 20 * (4 + 2 * r), b = WS_M + 20 * (5 + 2 * r), o = WS_B + 13 * r;
        double v[13];
        v[0] = ws(a + 12); v[1] = ws(a + 11) - ws(b + 12); v[2] = ws(a + 10) - ws(b + 11); v[3] = -ws(b + 10);
        v[4] = ws(a + 15); v[5] = ws(a + 14) - ws(b + 15); v[6] = ws(a + 13) - ws(b + 14); v[7] = -ws(b + 13);
        v[8] = ws(a + 19); v[9] = ws(a + 18) - ws(b + 19); v[10] = ws(a + 17) - ws(b + 18); v[11] = ws(a + 16) - ws(b + 17); v[12] = -ws(b + 16);
#pragma unroll
        for (int k = 0; k < 13; ++k) ws(o + k) = v[k];                // (rows 0 and 1 of the matrix, which are dead)
    }
}

// dst[i + j] +- a[i] b[j], i < na, j < nb, the products in the order of the loops
template <class W>
M3D_FN void upoly_mac(W ws, int dst, int a, int na, int b, int nb, bool neg) {
#pragma unroll 1
    for (int i = 0; i < na; ++i)
#pragma unroll 1
        for (int j = 0; j < nb; ++j) {
            const double p = ws(a + i) * ws(b + j);
            ws(dst + i + j) = neg ? ws(dst + i + j) - p : ws(dst + i + j) + p;
        }
}

// det B(z), degree 10, by the first row's cofactors, into WS_D; then derivative k at WS_D + 11 k.  false: the leading coefficient is 0 or a
// coefficient is not finite.
template <class W>
M3D_FN bool det_polynomial(W ws) {
    const int x0 = WS_B, y0 = WS_B + 4, c0 = WS_B + 8, x1 = WS_B + 13, y1 = WS_B + 17, c1 = WS_B + 21, x2 = WS_B + 26, y2 = WS_B + 30, c2 = WS_B + 34;
#pragma unroll 1
    for (int k = 0; k < 110; ++k) ws(WS_D + k) = 0.0;
#pragma unroll 1
    for (int k = 0; k < 8; ++k) ws(WS_MINOR + k) = 0.0;
    upoly_mac(ws, WS_MINOR, y1, 4, c2, 5, false); upoly_mac(ws, WS_MINOR, c1, 5, y2, 4, true);
    upoly_mac(ws, WS_D, x0, 4, WS_MINOR, 8, false);
#pragma unroll 1
    for (int k = 0; k < 8; ++k) ws(WS_MINOR + k) = 0.0;
    upoly_mac(ws, WS_MINOR, x1, 4, c2, 5, false); upoly_mac(ws, WS_MINOR, c1, 5, x2, 4, true);
    upoly_mac(ws, WS_D, y0, 4, WS_MINOR, 8, true);
#pragma unroll 1
    for (int k = 0; k < 8; ++k) ws(WS_MINOR + k) = 0.0;
    upoly_mac(ws, WS_MINOR, x1, 4, y2, 4, false); upoly_mac(ws, WS_MINOR, y1, 4, x2, 4, true);
    upoly_mac(ws, WS_D, c0, 5, WS_MINOR, 7, false);
    bool ok = ws(WS_D + 10) != 0.0;
#pragma unroll 1
    for (int k = 0; k <= 10; ++k) ok = ok && dfinite(ws(WS_D + k));
    if (!ok) return false;
#pragma unroll 1
    for (int k = 1; k < 10; ++k)
#pragma unroll 1
        for (int i = 0; i + k <= 10; ++i) ws(WS_D + 11 * k + i) = ws(WS_D + 11 * (k - 1) + i + 1) * (double)(i + 1);
    return true;
}

// the polynomial of degree d at `at` by Horner
template <class W>
M3D_FN double horner(W ws, int at, int d, double z) {
    double v = ws(at + d);
#pragma unroll 1
    for (int i = d - 1; i >= 0; --i) {
        const double a = v * z;
        v = a + ws(at + i);
    }
    return v;
}

// a root in [lo, hi] when the signs at the ends differ: BISECT halvings, then the middle of what is left
template <class W>
M3D_FN bool bisect(W ws, int at, int d, double lo, double hi, double& root) {
    const double plo = horner(ws, at, d, lo), phi = horner(ws, at, d, hi);
    const bool neg_lo = plo < 0.0;
    root = hi;
    if (neg_lo == (phi < 0.0)) return false;
    double a = lo, b = hi;
#pragma unroll 1
    for (int k = 0; k < BISECT; ++k) {
        const double s = a + b;
        const double mid = 0.5 * s;
        const double pm = horner(ws, at, d, mid);
        const bool left = (pm < 0.0) == neg_lo;
        a = left ? mid : a;
        b = left ? b : mid;
    }
    const double s = a + b;
    root = 0.5 * s;
    return true;
}

// The real roots of the polynomial at WS_D, ascending, into WS_RA; returns their number, -1 when the bound is not finite.  B = 1 + max |c_i /
// c_10|.  From the derivative of degree 1 upwards: the roots of the derivative of degree d - 1 and -B, B are the ends of the brackets of the
// one of degree d.
template <class W>
M3D_FN int real_roots(W ws) {
    const double lead = ws(WS_D + 10);
    double mx = 0.0;
#pragma unroll 1
    for (int i = 0; i < 10; ++i) {
        const double q = ws(WS_D + i) / lead;
        const double a = dmag(q);
        mx = a > mx ? a : mx;
    }
    const double B = 1.0 + mx;
    if (!dfinite(B)) return -1;
    const double nB = -B;
    int n_prev = 0, from = WS_RA, into = WS_RB;
#pragma unroll 1
    for (int d = 1; d <= 10; ++d) {
        const int at = WS_D + 11 * (10 - d);
        int n = 0;
#pragma unroll 1
        for (int i = 0; i < d; ++i) {
            if (i > n_prev) continue;
            const double lo = i == 0 ? nB : ws(from + i - 1);
            const double hi = i == n_prev ? B : ws(from + i);
            double x;
            if (bisect(ws, at, d, lo, hi, x)) { ws(into + n) = x; ++n; }
        }
        const int t = from; from = into; into = t;
        n_prev = n;
    }
    // ten swaps: the last roots are where the first array began
    return n_prev;
}

// Candidate r of the sample whose normalised correspondences are (x1[j], y1[j]) -> (x2[j], y2[j]): solve(ws, ...) runs once per hypothesis and
// returns the number of real roots (0: an invalid hypothesis); model(ws, r, E) makes root r's matrix.
template <class W>
M3D_FN int solve(W ws, const float x1[5], const float y1[5], const float x2[5], const float y2[5]) {
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const double x = (double)x1[j], y = (double)y1[j], xp = (double)x2[j], yp = (double)y2[j];
        const int o = WS_M + 9 * j;
        ws(o) = xp * x; ws(o + 1) = xp * y; ws(o + 2) = xp;
        ws(o + 3) = yp * x; ws(o + 4) = yp * y; ws(o + 5) = yp;
        ws(o + 6) = x; ws(o + 7) = y; ws(o + 8) = 1.0;
    }
    if (!null_space(ws)) return 0;
    constraints(ws);
    if (!eliminate(ws)) return 0;
    b_rows(ws);
    if (!det_polynomial(ws)) return 0;
    const int n = real_roots(ws);
    return n < 0 ? 0 : n;
}

// root r (< the count solve returned): x and y from the largest cross product of the rows of B(z) (the lowest pair on ties, in the order
// (0, 1), (0, 2), (1, 2)), then E = ((x X + y Y) + z Z) + W.  false: x, y or an entry of E is not finite.
template <class W>
M3D_FN bool model(W ws, int r, double E[9]) {
    const double z = ws(WS_RA + r);
    double b[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        b[i][0] = horner(ws, WS_B + 13 * i, 3, z);
        b[i][1] = horner(ws, WS_B + 13 * i + 4, 3, z);
        b[i][2] = horner(ws, WS_B + 13 * i + 8, 4, z);
    }
    double top = -1.0, v0 = 0.0, v1 = 0.0, v2 = 0.0;
#pragma unroll
    for (int p = 0; p < 3; ++p) {
        const int i = p == 2 ? 1 : 0, j = p == 0 ? 1 : 2;
        const double a0 = b[i][1] * b[j][2], a1 = b[i][2] * b[j][1];
        const double b0 = b[i][2] * b[j][0], b1 = b[i][0] * b[j][2];
        const double c0 = b[i][0] * b[j][1], c1 = b[i][1] * b[j][0];
        const double cx = a0 - a1, cy = b0 - b1, cz = c0 - c1;
        const double xx = cx * cx, yy = cy * cy, zz = cz * cz;
        const double xy = xx + yy;
        const double n = xy + zz;
        const bool more = n > top;
        top = more ? n : top;
        v0 = more ? cx : v0; v1 = more ? cy : v1; v2 = more ? cz : v2;
    }
    const double x = v0 / v2, y = v1 / v2;
    bool ok = dfinite(x) && dfinite(y);
#pragma unroll
    for (int e = 0; e < 9; ++e) {
        const double px = x * ws(WS_BASIS + e), py = y * ws(WS_BASIS + 9 + e), pz = z * ws(WS_BASIS + 18 + e);
        const double s = px + py;
        const double t = s + pz;
        E[e] = t + ws(WS_BASIS + 27 + e);
        ok = ok && dfinite(E[e]);
    }
    return ok;
}

// computeError (five-point.cpp:375-401) with E rounded to fp32: (x2^T E x1)^2 / (((a + b) + c) + d); an inlier iff <= thr2 (a NaN is none)
M3D_FN float sampson(const float E[9], float x1, float y1, float x2, float y2) {
    const float p0 = E[0] * x1, p1 = E[1] * y1;
    const float p01 = p0 + p1;
    const float ex = p01 + E[2];
    const float q0 = E[3] * x1, q1 = E[4] * y1;
    const float q01 = q0 + q1;
    const float ey = q01 + E[5];
    const float r0 = E[6] * x1, r1 = E[7] * y1;
    const float r01 = r0 + r1;
    const float ez = r01 + E[8];
    const float s0 = E[0] * x2, s1 = E[3] * y2;
    const float s01 = s0 + s1;
    const float tx = s01 + E[6];
    const float u0 = E[1] * x2, u1 = E[4] * y2;
    const float u01 = u0 + u1;
    const float ty = u01 + E[7];
    const float d0 = x2 * ex, d1 = y2 * ey;
    const float d01 = d0 + d1;
    const float dot = d01 + ez;
    const float a = ex * ex, b = ey * ey, c = tx * tx, d = ty * ty;
    const float ab = a + b;
    const float abc = ab + c;
    const float den = abc + d;
    const float num = dot * dot;
    return num / den;
}
M3D_FN bool is_inlier(const float E[9], float x1, float y1, float x2, float y2, float thr2) { return sampson(E, x1, y1, x2, y2) <= thr2; }

// Horn's closed form: t t^T = tr(E E^T) / 2 I - E E^T, the column of the largest diagonal entry (the lowest on ties) over the root of that
// entry is b; C's row i is the cross product of E's rows i + 1 and i + 2 (cyclic); R1 = (C - [b]x E) / (b.b), R2 = (C + [b]x E) / (b.b); t = b
// / sqrt(b.b).  pose = R1 (9), R2 (9), t (3).  false: an entry that is not finite.
M3D_FN bool decompose(const double E[9], double pose[21]) {
    double G[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double a = E[3 * i] * E[3 * j], b = E[3 * i + 1] * E[3 * j + 1], c = E[3 * i + 2] * E[3 * j + 2];
            const double ab = a + b;
            G[3 * i + j] = ab + c;
        }
    const double t01 = G[0] + G[4];
    const double tr = t01 + G[8];
    const double h = 0.5 * tr;
    double M[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) M[i] = (i == 0 || i == 4 || i == 8) ? h - G[i] : -G[i];
    double top = M[0], c0 = M[0], c1 = M[3], c2 = M[6];
    if (M[4] > top) { top = M[4]; c0 = M[1]; c1 = M[4]; c2 = M[7]; }
    if (M[8] > top) { top = M[8]; c0 = M[2]; c1 = M[5]; c2 = M[8]; }
    const double root = sqrt(top);
    const double b0 = c0 / root, b1 = c1 / root, b2 = c2 / root;
    const double s0 = b0 * b0, s1 = b1 * b1, s2 = b2 * b2;
    const double s01 = s0 + s1;
    const double bb = s01 + s2;
    const double nb = sqrt(bb);
    double C[9], S[9];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int p = (i + 1) % 3, q = (i + 2) % 3;
        const double a0 = E[3 * p + 1] * E[3 * q + 2], a1 = E[3 * p + 2] * E[3 * q + 1];
        const double d0 = E[3 * p + 2] * E[3 * q], d1 = E[3 * p] * E[3 * q + 2];
        const double e0 = E[3 * p] * E[3 * q + 1], e1 = E[3 * p + 1] * E[3 * q];
        C[3 * i] = a0 - a1; C[3 * i + 1] = d0 - d1; C[3 * i + 2] = e0 - e1;
    }
    // S = [b]x E: row 0 = b1 E2. - b2 E1., row 1 = b2 E0. - b0 E2., row 2 = b0 E1. - b1 E0.
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const double a0 = b1 * E[6 + j], a1 = b2 * E[3 + j];
        const double d0 = b2 * E[j], d1 = b0 * E[6 + j];
        const double e0 = b0 * E[3 + j], e1 = b1 * E[j];
        S[j] = a0 - a1; S[3 + j] = d0 - d1; S[6 + j] = e0 - e1;
    }
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        const double m = C[i] - S[i], p = C[i] + S[i];
        pose[i] = m / bb;
        pose[9 + i] = p / bb;
        ok = ok && dfinite(pose[i]) && dfinite(pose[9 + i]);
    }
    pose[18] = b0 / nb; pose[19] = b1 / nb; pose[20] = b2 / nb;
    return ok && dfinite(pose[18]) && dfinite(pose[19]) && dfinite(pose[20]);
}

// the two depths that minimise |d2 x2 - (d1 R x1 + s t)|^2, s = +-1; false: the determinant is 0 or not finite
M3D_FN bool triangulate(const double R[9], const double t[3], bool minus, float fx1, float fy1, float fx2, float fy2, double& d1, double& d2) {
    const double x1 = (double)fx1, y1 = (double)fy1, x2 = (double)fx2, y2 = (double)fy2;
    double a[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double p = R[3 * i] * x1, q = R[3 * i + 1] * y1;
        const double pq = p + q;
        a[i] = pq + R[3 * i + 2];
    }
    const double t0 = minus ? -t[0] : t[0], t1 = minus ? -t[1] : t[1], t2 = minus ? -t[2] : t[2];
    const double aa0 = a[0] * a[0], aa1 = a[1] * a[1], aa2 = a[2] * a[2];
    const double aa01 = aa0 + aa1;
    const double aa = aa01 + aa2;
    const double bb0 = x2 * x2, bb1 = y2 * y2;
    const double bb01 = bb0 + bb1;
    const double bb = bb01 + 1.0;
    const double ab0 = a[0] * x2, ab1 = a[1] * y2;
    const double ab01 = ab0 + ab1;
    const double ab = ab01 + a[2];
    const double at0 = a[0] * t0, at1 = a[1] * t1, at2 = a[2] * t2;
    const double at01 = at0 + at1;
    const double at = at01 + at2;
    const double bt0 = x2 * t0, bt1 = y2 * t1;
    const double bt01 = bt0 + bt1;
    const double bt = bt01 + t2;
    const double m0 = aa * bb, m1 = ab * ab;
    const double det = m0 - m1;
    d1 = 0.0; d2 = 0.0;
    if (det == 0.0 || !dfinite(det)) return false;
    const double n0 = ab * bt, n1 = at * bb;
    const double num1 = n0 - n1;
    const double k0 = aa * bt, k1 = ab * at;
    const double num2 = k0 - k1;
    d1 = num1 / det;
    d2 = num2 / det;
    return true;
}
// recoverPose's three mask tests (five-point.cpp:530-538) with z = d1 in the first camera and d2 in the second
M3D_FN bool in_front(bool have, double d1, double d2, double dist) { return have && d1 > 0.0 && d1 < dist && d2 > 0.0 && d2 < dist; }
// configuration k of (R1, t), (R2, t), (R1, -t), (R2, -t) for one correspondence
M3D_FN bool config_test(const double pose[21], int k, float x1, float y1, float x2, float y2, double dist, double& d1) {
    double d2;
    const bool have = triangulate(pose + ((k & 1) ? 9 : 0), pose + 18, k >= 2, x1, y1, x2, y2, d1, d2);
    return in_front(have, d1, d2, dist);
}
// the >= cascade of five-point.cpp:609-642
M3D_FN int choose_config(int g1, int g2, int g3, int g4) {
    if (g1 >= g2 && g1 >= g3 && g1 >= g4) return 0;
    if (g2 >= g1 && g2 >= g3 && g2 >= g4) return 1;
    if (g3 >= g1 && g3 >= g2 && g3 >= g4) return 2;
    return 3;
}

// cameraTransform = local x inverse([R | t]) x inverse(local) (util3d_features.cpp:277-282), R and t rounded to fp32
M3D_FN void camera_transform(const double pose[21], int k, const float local[12], float out[12]) {
    float rt[12], inv[12], linv[12], a[12];
    const double* R = pose + ((k & 1) ? 9 : 0);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) rt[4 * i + j] = (float)R[3 * i + j];
        rt[4 * i + 3] = (float)(k >= 2 ? -pose[18 + i] : pose[18 + i]);
    }
    m3d::invert(rt, inv);
    m3d::invert(local, linv);
    m3d::compose(local, inv, a);
    m3d::compose(a, linv, out);
}
// the triangulated point d1 (x1, y1, 1) as floats, moved by local (:293)
M3D_FN void point_of(double d1, float x1, float y1, const float local[12], float p[3]) {
    const double px = d1 * (double)x1, py = d1 * (double)y1;
    m3d::apply(local, (float)px, (float)py, (float)d1, p[0], p[1], p[2]);
}
// findCorrespondences(.., 0)'s tests (util3d_correspondences.cpp:388-391)
M3D_FN bool usable(const float p[3], const float g[3]) {
    return finite(p[0]) && finite(p[1]) && finite(p[2]) && finite(g[0]) && finite(g[1]) && finite(g[2]) && (p[0] != 0.0f || p[1] != 0.0f || p[2] != 0.0f) &&
           (g[0] != 0.0f || g[1] != 0.0f || g[2] != 0.0f);
}
// uNormSquared(s p - g) (:341-346)
M3D_FN float scaled_error(const float p[3], const float g[3], float s) {
    const float x = p[0] * s, y = p[1] * s, z = p[2] * s;
    const float dx = x - g[0], dy = y - g[1], dz = z - g[2];
    const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
    const float xy = xx + yy;
    return xy + zz;
}
M3D_FN float norm3(float x, float y, float z) {
    const float xx = x * x, yy = y * y, zz = z * z;
    const float xy = xx + yy;
    const float n = xy + zz;
    return sqrtf(n);
}
// the key a float sorts by, ascending, NaNs of either sign last, and back
M3D_FN uint32_t order_key(float v) {
    const uint32_t b = bits_of(v);
    if ((b & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;
    return (b & 0x80000000u) ? ~b : b | 0x80000000u;
}
M3D_FN float key_value(uint32_t k) { return k == 0xffffffffu ? float_of(0x7fc00000u) : float_of((k & 0x80000000u) ? k & 0x7fffffffu : ~k); }
// the rank of errorSqrdDists[size >> ratio] (:349); the reference reads one past the end when the shift leaves size: the last is taken
M3D_FN int median_rank(int n, int ratio) {
    const int r = n >> ratio;
    return r < n ? r : n - 1;
}
M3D_FN float variance_of(float median) { return (float)(VARIANCE_FACTOR * (double)median); }
// Transform::isNull of a guess: all twelve 0, or a NaN
M3D_FN bool guess_is_null(const float g[12]) {
    bool zero = true, nan = false;
    for (int k = 0; k < 12; ++k) { zero = zero && g[k] == 0.0f; nan = nan || g[k] != g[k]; }
    return zero || nan;
}

}  // namespace mono
}  // namespace lcd
