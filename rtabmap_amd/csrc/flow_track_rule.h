// flow_track_rule.h -- the rule of lcd_track_flow (include/lcd.h writes it down) as functions the kernels (flow_track.hip), the host entry's
// checks and the host mirror (rtabmap_amd/host/FlowTrack.cpp) compile alike.  The pyramid, the Scharr derivative, the fixed-point patch,
// the bounds tests and the x step are stereo_flow_rule.h's; this file adds only what the 2-D tracker does differently: the lane-tree order
// of every float sum, the step on both axes, the stop and the oscillation test on both axes, the start from a caller's position, minEig as
// the error, and the keep test of RegistrationVis.cpp:709-724.  One operation per statement, never contracted.  Internal.
#pragma once
#include <cmath>

#include "stereo_flow_rule.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace lcd {
namespace flow {

constexpr int LANES = 64;

// The sum of e(0) .. e(n - 1) in the engine's order (rtabmap_amd/host/LaneSum.h, laneTreeSum<64>): part p % 64 adds its terms in ascending
// p from +0, then the parts are added by the halving tree, the top half onto the bottom half.  The kernel's wave computes exactly this.
template <class F>
KP3D_FN float lane_tree_sum(int n, F e) {
    float part[LANES];
    for (int l = 0; l < LANES; ++l) part[l] = 0.0f;
    for (int p = 0; p < n; ++p) part[p % LANES] = part[p % LANES] + e(p);
    for (int s = LANES / 2; s >= 1; s >>= 1)
        for (int l = 0; l < s; ++l) part[l] = part[l] + part[l + s];
    return part[0];
}

// minEig of the scaled sums, as the stereo rule states it: sqrt and division correctly rounded fp32.  The stereo call only compares it with
// the threshold; this call hands it out (out_err), so the device takes sqrtf here and not the hardware's approximate root.
KP3D_FN float min_eig(float A11, float A12, float A22, int win_w, int win_h) {
    const float s = A22 + A11, d = A11 - A22;
    const float dd = d * d;
    const float f = 4.0f * A12;
    const float ff = f * A12;
    const float r = dd + ff;
    const float root = sqrtf(r);
    const float num = s - root;
    return num / (float)(2 * win_w * win_h);
}
// the stereo rule's two tests on D and minEig; *inv_d = 1.f / D where the level goes on
KP3D_FN bool solve(float A11, float A12, float A22, float eig, double min_eig_threshold, float* inv_d) {
    const float p = A11 * A22, q = A12 * A12;
    const float D = p - q;
    if ((double)eig < min_eig_threshold || D < stereo::FLT_EPS) return false;
    *inv_d = 1.0f / D;
    return true;
}

// delta of one iteration: x is the stereo rule's, y its counterpart
KP3D_FN void step(float A11, float A12, float A22, float b1, float b2, float inv_d, float* dx, float* dy) {
    *dx = stereo::delta_x(A12, A22, b1, b2, inv_d);
    const float p = A12 * b1, q = A11 * b2;
    const float n = p - q;
    *dy = n * inv_d;
}
KP3D_FN bool converged(float dx, float dy, double eps2) {
    const double x = (double)dx, y = (double)dy;
    const double xx = x * x, yy = y * y;
    return xx + yy <= eps2;
}
KP3D_FN bool oscillates(float dx, float dy, float prev_dx, float prev_dy) { return stereo::oscillates(dx, prev_dx) && stereo::oscillates(dy, prev_dy); }

// where the reference asserts or is undefined: a point, or with use_initial a start position, that is not finite or not inside int
KP3D_FN bool trackable(float ptx, float pty, int use_initial, float sx, float sy) {
    if (!kp3d::convertible(ptx) || !kp3d::convertible(pty)) return false;
    return !use_initial || (kp3d::convertible(sx) && kp3d::convertible(sy));
}

// RegistrationVis.cpp:709-724: the tracked corner is kept
KP3D_FN bool keep(const stereo::Track& T, int cols, int rows, int use_min_eigenvals, float error_threshold) {
    if (!T.status) return false;
    if (!kp3d::finite(T.rx) || T.rx < 0.0f || T.rx >= (float)cols) return false;
    if (!kp3d::finite(T.ry) || T.ry < 0.0f || T.ry >= (float)rows) return false;
    return use_min_eigenvals != 0 || T.err < error_threshold;
}

// ---- the tracker for one corner, the levels top down; I and J are the from and the to pyramid, (sx, sy) the start position where
// use_initial is set.  buf: win_w * win_h * 4 shorts.  This is the rule as a sequence; the kernel computes the same terms with a wave, a
// lane owning the part of the same number.
KP3D_FN stereo::Track track_point_2d(const stereo::Level* I, const stereo::Level* J, int levels, const stereo::Params& P, float ptx, float pty,
                                     int use_initial, float sx, float sy, short* buf) {
    using namespace stereo;
    Track T;
    T.status = 1; T.err = 0.0f;
    if (!trackable(ptx, pty, use_initial, sx, sy)) { T.rx = T.ry = kp3d::quiet_nan(); T.status = 0; return T; }
    const int ww = P.win_w, wh = P.win_h, n = ww * wh;
    const float hx = (float)(ww - 1) * 0.5f, hy = (float)(wh - 1) * 0.5f;
    short* Ib = buf; short* dxb = buf + n; short* dyb = buf + 2 * n; short* df = buf + 3 * n;
    float nx = 0.0f, ny = 0.0f;              // nextPts[ptidx]
    for (int level = levels - 1; level >= 0; --level) {
        const GlobalPx pi{I[level]}, pj{J[level]};
        const int cols = I[level].w, rows = I[level].h;
        const float scale = 1.0f / (float)(1 << level);
        float px = ptx * scale, py = pty * scale;
        float qx, qy;
        if (level == levels - 1) {
            if (use_initial) { qx = sx * scale; qy = sy * scale; }
            else { qx = px; qy = py; }
        } else { qx = nx * 2.0f; qy = ny * 2.0f; }
        nx = qx; ny = qy;
        px = px - hx; py = py - hy;
        const int ipx = floor_int(px), ipy = floor_int(py);
        if (outside(ipx, ipy, ww, wh, cols, rows)) {
            if (level == 0) T.status = 0;
            continue;
        }
        int iw[4];
        weights(px - (float)ipx, py - (float)ipy, iw);
        for (int y = 0; y < wh; ++y)
            for (int x = 0; x < ww; ++x) {
                const int iv = sample(pi, ipx, ipy, x, y, iw);
                int ix, iy;
                sample_deriv(pi, ipx, ipy, x, y, cols, rows, iw, ix, iy);
                Ib[y * ww + x] = (short)iv; dxb[y * ww + x] = (short)ix; dyb[y * ww + x] = (short)iy;
            }
        const float s11 = lane_tree_sum(n, [&](int p) { return (float)((int)dxb[p] * (int)dxb[p]); });
        const float s12 = lane_tree_sum(n, [&](int p) { return (float)((int)dxb[p] * (int)dyb[p]); });
        const float s22 = lane_tree_sum(n, [&](int p) { return (float)((int)dyb[p] * (int)dyb[p]); });
        const float A11 = s11 * FLT_SCALE, A12 = s12 * FLT_SCALE, A22 = s22 * FLT_SCALE;
        const float eig = min_eig(A11, A12, A22, ww, wh);
        if (P.use_min_eigenvals) T.err = eig;
        float inv_d;
        if (!flow::solve(A11, A12, A22, eig, P.min_eig_threshold, &inv_d)) {
            if (level == 0) T.status = 0;
            continue;
        }
        qx = qx - hx; qy = qy - hy;
        float prev_dx = 0.0f, prev_dy = 0.0f;
        for (int j = 0; j < P.iterations; ++j) {
            const int inx = floor_int(qx), iny = floor_int(qy);
            if (outside(inx, iny, ww, wh, cols, rows)) {
                if (level == 0) T.status = 0;
                break;
            }
            weights(qx - (float)inx, qy - (float)iny, iw);
            for (int y = 0; y < wh; ++y)
                for (int x = 0; x < ww; ++x) df[y * ww + x] = (short)(sample(pj, inx, iny, x, y, iw) - (int)Ib[y * ww + x]);
            const float sb1 = lane_tree_sum(n, [&](int p) { return (float)((int)df[p] * (int)dxb[p]); });
            const float sb2 = lane_tree_sum(n, [&](int p) { return (float)((int)df[p] * (int)dyb[p]); });
            const float b1 = sb1 * FLT_SCALE, b2 = sb2 * FLT_SCALE;
            float dx, dy;
            step(A11, A12, A22, b1, b2, inv_d, &dx, &dy);
            qx = qx + dx; qy = qy + dy;
            nx = qx + hx; ny = qy + hy;
            if (converged(dx, dy, P.eps2)) break;
            if (j > 0 && oscillates(dx, dy, prev_dx, prev_dy)) {
                const float half_x = dx * 0.5f, half_y = dy * 0.5f;
                nx = nx - half_x; ny = ny - half_y;
                break;
            }
            prev_dx = dx; prev_dy = dy;
        }
        if (T.status && level == 0 && !P.use_min_eigenvals) {           // the L1 error, as the stereo rule has it
            const float ex = nx - hx, ey = ny - hy;
            const int iex = floor_int(ex), iey = floor_int(ey);
            if (outside(iex, iey, ww, wh, cols, rows)) { T.status = 0; continue; }
            weights(ex - (float)iex, ey - (float)iey, iw);
            for (int y = 0; y < wh; ++y)
                for (int x = 0; x < ww; ++x) {
                    int diff = sample(pj, iex, iey, x, y, iw) - (int)Ib[y * ww + x];
                    if (diff < 0) diff = -diff;
                    df[y * ww + x] = (short)diff;
                }
            const float errval = lane_tree_sum(n, [&](int p) { return (float)(int)df[p]; });
            T.err = errval / (float)(32 * ww * wh);
        }
    }
    T.rx = nx; T.ry = ny;
    return T;
}

}  // namespace flow
}  // namespace lcd
