// motion_rule_common.h -- what the rules of lcd_estimate_motion_3d (motion_3d_rule.h), lcd_estimate_motion_pnp (motion_pnp_rule.h) and
// lcd_register_icp (icp_rule.h, icp_plane_rule.h) share: the bit helpers, the id keys, the counter-based mix, the three-element sum in the order of the 256-lane
// sum, the rigid fit (Horn's quaternion by cyclic Jacobi), a rigid model applied, inverted and composed, and the 6 x 6 LDL^T solve.  fp32, one rounded operation
// per statement, never contracted; division and square root are IEEE.  Compiled for the kernels and for the host mirrors alike.  Internal.
#pragma once
#include <stdint.h>
#include <cmath>
#include <cstring>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define M3D_FN __host__ __device__ __forceinline__
#else
#define M3D_FN inline
#endif
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace lcd {
namespace m3d {

constexpr int LANES = 256;                   // the lanes of the summation order
constexpr int MAX_DRAWS = 16;                // draws a hypothesis may use to find its distinct indices
constexpr int MAX_ROWS = 8192;               // rows of a frame

M3D_FN uint32_t bits_of(float v) { uint32_t b; memcpy(&b, &v, 4); return b; }
M3D_FN float float_of(uint32_t b) { float v; memcpy(&v, &b, 4); return v; }
M3D_FN bool finite(float v) { return (bits_of(v) & 0x7f800000u) != 0x7f800000u; }

// the key a word id sorts by: ascending as a signed integer
M3D_FN uint32_t id_key(int32_t id) { return (uint32_t)id ^ 0x80000000u; }
M3D_FN int32_t key_id(uint32_t k) { return (int32_t)(k ^ 0x80000000u); }

M3D_FN uint32_t mix(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352du;
    x ^= x >> 15; x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

// the sum of three elements in the order of the LANES-lane sum: ((0 + e0) + (0 + e2)) + (0 + e1)
M3D_FN float sum3(float e0, float e1, float e2) {
    const float a = 0.0f + e0, b = 0.0f + e1, c = 0.0f + e2;
    const float ac = a + c;
    return ac + b;
}

// one Jacobi rotation of the symmetric A (both halves kept) in the plane (P, Q), accumulated into the columns of V
template <int P, int Q>
M3D_FN void jacobi_rotate(float A[4][4], float V[4][4]) {
    const float apq = A[P][Q];
    if (apq == 0.0f) return;
    const float diff = A[Q][Q] - A[P][P];
    const float den = 2.0f * apq;
    const float theta = diff / den;                                    // an overflow to +-inf runs through what follows and gives t = +-0
    const float mag = float_of(bits_of(theta) & 0x7fffffffu);
    const float th2 = theta * theta;
    const float th21 = th2 + 1.0f;
    const float root = sqrtf(th21);
    const float sum = mag + root;
    const float sgn = theta < 0.0f ? -1.0f : 1.0f;
    const float t = sgn / sum;
    const float t2 = t * t;
    const float t21 = t2 + 1.0f;
    const float croot = sqrtf(t21);
    const float c = 1.0f / croot;
    const float s = t * c;
    const float tapq = t * apq;
    A[P][P] = A[P][P] - tapq;
    A[Q][Q] = A[Q][Q] + tapq;
    A[P][Q] = 0.0f; A[Q][P] = 0.0f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (r == P || r == Q) continue;
        const float arp = A[r][P], arq = A[r][Q];
        const float c_arp = c * arp, s_arq = s * arq, s_arp = s * arp, c_arq = c * arq;
        const float np = c_arp - s_arq, nq = s_arp + c_arq;
        A[r][P] = np; A[P][r] = np;
        A[r][Q] = nq; A[Q][r] = nq;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float vrp = V[r][P], vrq = V[r][Q];
        const float c_vrp = c * vrp, s_vrq = s * vrq, s_vrp = s * vrp, c_vrq = c * vrq;
        V[r][P] = c_vrp - s_vrq;
        V[r][Q] = s_vrp + c_vrq;
    }
}

// the rotation of the quaternion (q0, q1, q2, q3) / |q|, |q| = sqrt(((q0 q0 + q1 q1) + q2 q2) + q3 q3); the unit quaternion comes back in q
M3D_FN void quat_rotation(float& q0, float& q1, float& q2, float& q3, float R[3][3]) {
    const float s0 = q0 * q0, s1 = q1 * q1, s2 = q2 * q2, s3 = q3 * q3;
    const float s01 = s0 + s1;
    const float s012 = s01 + s2;
    const float n2 = s012 + s3;
    const float n = sqrtf(n2);
    const float w = q0 / n, x = q1 / n, y = q2 / n, z = q3 / n;
    const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, xz = x * z, yz = y * z, wx = w * x, wy = w * y, wz = w * z;
    const float yy_zz = yy + zz, xx_zz = xx + zz, xx_yy2 = xx + yy;
    const float d0 = 2.0f * yy_zz, d1 = 2.0f * xx_zz, d2 = 2.0f * xx_yy2;
    const float xy_m = xy - wz, xy_p = xy + wz, xz_p = xz + wy, xz_m = xz - wy, yz_m = yz - wx, yz_p = yz + wx;
    R[0][0] = 1.0f - d0; R[0][1] = 2.0f * xy_m; R[0][2] = 2.0f * xz_p;
    R[1][0] = 2.0f * xy_p; R[1][1] = 1.0f - d1; R[1][2] = 2.0f * yz_m;
    R[2][0] = 2.0f * xz_m; R[2][1] = 2.0f * yz_p; R[2][2] = 1.0f - d2;
    q0 = w; q1 = x; q2 = y; q3 = z;
}

// the rigid fit from the two centroids and the nine sums S[3 a + b] of (p_a - cp_a) * (q_b - cq_b): model = row-major 3 x 4, R p + t ~ q
M3D_FN void horn_fit(const float cp[3], const float cq[3], const float S[9], int sweeps, float model[12]) {
    const float Sxx = S[0], Sxy = S[1], Sxz = S[2], Syx = S[3], Syy = S[4], Syz = S[5], Szx = S[6], Szy = S[7], Szz = S[8];
    float A[4][4], V[4][4];
    const float xx_yy = Sxx + Syy;
    A[0][0] = xx_yy + Szz;
    A[0][1] = Syz - Szy; A[0][2] = Szx - Sxz; A[0][3] = Sxy - Syx;
    const float xx_m_yy = Sxx - Syy;
    A[1][1] = xx_m_yy - Szz;
    A[1][2] = Sxy + Syx; A[1][3] = Szx + Sxz;
    const float yy_m_xx = Syy - Sxx;
    A[2][2] = yy_m_xx - Szz;
    A[2][3] = Syz + Szy;
    const float zz_m_xx = Szz - Sxx;
    A[3][3] = zz_m_xx - Syy;
    A[1][0] = A[0][1]; A[2][0] = A[0][2]; A[3][0] = A[0][3]; A[2][1] = A[1][2]; A[3][1] = A[1][3]; A[3][2] = A[2][3];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) V[r][c] = r == c ? 1.0f : 0.0f;
#pragma unroll
    for (int sweep = 0; sweep < sweeps; ++sweep) {
        jacobi_rotate<0, 1>(A, V); jacobi_rotate<0, 2>(A, V); jacobi_rotate<0, 3>(A, V);
        jacobi_rotate<1, 2>(A, V); jacobi_rotate<1, 3>(A, V); jacobi_rotate<2, 3>(A, V);
    }
    // the eigenvector of the largest diagonal entry, the lowest index on ties
    // (every entry is read before the choice: values are selected, never an address into V)
    const float v00 = V[0][0], v10 = V[1][0], v20 = V[2][0], v30 = V[3][0], v01 = V[0][1], v11 = V[1][1], v21 = V[2][1], v31 = V[3][1];
    const float v02 = V[0][2], v12 = V[1][2], v22 = V[2][2], v32 = V[3][2], v03 = V[0][3], v13 = V[1][3], v23 = V[2][3], v33 = V[3][3];
    const float a11 = A[1][1], a22 = A[2][2], a33 = A[3][3];
    float top = A[0][0], q0 = v00, q1 = v10, q2 = v20, q3 = v30;
    if (a11 > top) { top = a11; q0 = v01; q1 = v11; q2 = v21; q3 = v31; }
    if (a22 > top) { top = a22; q0 = v02; q1 = v12; q2 = v22; q3 = v32; }
    if (a33 > top) { top = a33; q0 = v03; q1 = v13; q2 = v23; q3 = v33; }
    float R[3][3];
    quat_rotation(q0, q1, q2, q3, R);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const float a = R[r][0] * cp[0], b = R[r][1] * cp[1], c = R[r][2] * cp[2];
        const float ab = a + b;
        const float abc = ab + c;
        model[4 * r] = R[r][0]; model[4 * r + 1] = R[r][1]; model[4 * r + 2] = R[r][2];
        model[4 * r + 3] = cq[r] - abc;
    }
}

// the fit of three correspondences P[i] -> Q[i], in the order given
M3D_FN void fit3(const float P[3][3], const float Q[3][3], int sweeps, float model[12]) {
    float cp[3], cq[3], S[9];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float sp = sum3(P[0][a], P[1][a], P[2][a]), sq = sum3(Q[0][a], Q[1][a], Q[2][a]);
        cp[a] = sp / 3.0f;
        cq[a] = sq / 3.0f;
    }
    float dp[3][3], dq[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int a = 0; a < 3; ++a) { dp[i][a] = P[i][a] - cp[a]; dq[i][a] = Q[i][a] - cq[a]; }
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            const float e0 = dp[0][a] * dq[0][b], e1 = dp[1][a] * dq[1][b], e2 = dp[2][a] * dq[2][b];
            S[3 * a + b] = sum3(e0, e1, e2);
        }
    horn_fit(cp, cq, S, sweeps, model);
}

// R p + t
M3D_FN void apply(const float m[12], float px, float py, float pz, float& x, float& y, float& z) {
    const float x0 = m[0] * px, x1 = m[1] * py, x2 = m[2] * pz;
    const float x01 = x0 + x1;
    const float x012 = x01 + x2;
    x = x012 + m[3];
    const float y0 = m[4] * px, y1 = m[5] * py, y2 = m[6] * pz;
    const float y01 = y0 + y1;
    const float y012 = y01 + y2;
    y = y012 + m[7];
    const float z0 = m[8] * px, z1 = m[9] * py, z2 = m[10] * pz;
    const float z01 = z0 + z1;
    const float z012 = z01 + z2;
    z = z012 + m[11];
}

// the inverse of a rigid model: R^T and -(R^T t)
M3D_FN void invert(const float m[12], float out[12]) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const float a = m[r] * m[3], b = m[4 + r] * m[7], c = m[8 + r] * m[11];
        const float ab = a + b;
        const float abc = ab + c;
        out[4 * r] = m[r]; out[4 * r + 1] = m[4 + r]; out[4 * r + 2] = m[8 + r];
        out[4 * r + 3] = -abc;
    }
}

// a x b for two rigid 3 x 4
M3D_FN void compose(const float a[12], const float b[12], float out[12]) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float p0 = a[4 * r] * b[c], p1 = a[4 * r + 1] * b[4 + c], p2 = a[4 * r + 2] * b[8 + c];
            const float p01 = p0 + p1;
            const float p012 = p01 + p2;
            out[4 * r + c] = c == 3 ? p012 + a[4 * r + 3] : p012;
        }
    }
}

// The 6 x 6 system A x = b by LDL^T without pivoting: S holds the 21 entries of A's upper triangle row by row, then the 6 of b; false (delta untouched): a pivot that is not positive and finite, or a solution that is not finite
M3D_FN bool ldlt6_solve(const float S[27], float delta[6]) {
    float A[6][6], Lm[6][6], d[6], w[6], z[6], x[6];
    int o = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = i; j < 6; ++j) { A[i][j] = S[o]; A[j][i] = S[o]; ++o; }
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        float acc = A[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) {
            w[k] = Lm[j][k] * d[k];
            const float p = Lm[j][k] * w[k];
            acc = acc - p;
        }
        if (!(acc > 0.0f) || !finite(acc)) return false;
        d[j] = acc;
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            float a = A[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) {
                const float p = Lm[i][k] * w[k];
                a = a - p;
            }
            Lm[i][j] = a / acc;
        }
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        float a = S[21 + i];
#pragma unroll
        for (int k = 0; k < i; ++k) {
            const float p = Lm[i][k] * z[k];
            a = a - p;
        }
        z[i] = a;
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {
        float a = z[i] / d[i];
#pragma unroll
        for (int k = i + 1; k < 6; ++k) {
            const float p = Lm[k][i] * x[k];
            a = a - p;
        }
        x[i] = a;
    }
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 6; ++i) ok = ok && finite(x[i]);
    if (!ok) return false;
#pragma unroll
    for (int i = 0; i < 6; ++i) delta[i] = x[i];
    return true;
}

}  // namespace m3d
}  // namespace lcd
