// scan_filter_rule.h -- the rule of lcd_filter_scans (include/lcd.h writes it down with the reference's line numbers) as functions the kernels
// (scan_filter.hip) and the host mirror (rtabmap_amd/host/ScanFilter.cpp) compile alike: which rows downsampling and the range keep, a
// coordinate's voxel cell and a voxel's index, the sums over a row's neighbours, the normal out of them, and the two flips.  fp32, one rounded
// operation per statement, never contracted; only + - x / sqrt and floor.  What needs a scan as a whole (the compaction, the sort by voxel,
// the neighbour search) is the caller's: the kernels do it as workgroups, the mirror as loops.  Internal.
#pragma once
#include "icp_plane_rule.h"

namespace lcd {
namespace scf {

using icp::dist2;
using icpp::finite3;
using m3d::finite;

constexpr int ST_OK = 0, ST_EMPTY = 1, ST_GRID_TOO_LARGE = 2, ST_TOO_MANY_ROWS = 3, ST_NO_ROOM = 4;   // lcd_scan_status
constexpr int MAX_K = 32;                    // LCD_SCAN_MAX_K
constexpr int MAX_SAMPLED = 16384;           // sampled rows of a scan
constexpr int MAX_NORMAL_ROWS = m3d::MAX_ROWS;   // rows that reach step 3
constexpr uint32_t QUIET_NAN = 0x7fc00000u;

struct Params {
    int32_t step, is_2d, k, normals;         // normals: k > 0 || radius > 0
    float range_min, range_max, voxel, radius, ground_up;
    float vp[3];
};

// ---- step 1
M3D_FN int step_of(int step, int64_t n) { return (step <= 1 || n <= (int64_t)step) ? 1 : step; }
// a sampled row stays iff its coordinates are finite and the range keeps it
M3D_FN bool stays(const Params& p, float x, float y, float z) {
    if (!finite3(x, y, z)) return false;
    if (!(p.range_min > 0.0f || p.range_max > 0.0f)) return true;
    const float xx = x * x, yy = y * y;
    float r = xx + yy;
    if (!p.is_2d) {
        const float zz = z * z;
        r = r + zz;
    }
    if (!finite(r)) return false;
    if (p.range_min > 0.0f) {
        const float lo = p.range_min * p.range_min;
        if (r < lo) return false;
    }
    if (p.range_max > 0.0f) {
        const float hi = p.range_max * p.range_max;
        if (r > hi) return false;
    }
    return true;
}

// ---- step 2
M3D_FN float inverse_leaf(float voxel) { return 1.0f / voxel; }
// false: the cell is beyond int32 (or no number)
M3D_FN bool cell_of(float x, float inv, int32_t& c) {
    const float u = x * inv;
    const float f = floorf(u);
    if (!(f >= -2147483648.0f && f < 2147483648.0f)) return false;
    c = (int32_t)f;
    return true;
}
// the grid's extent from the cell bounds; false: more than INT32_MAX voxels
M3D_FN bool grid_dims(const int32_t lo[3], const int32_t hi[3], int64_t d[3]) {
#pragma unroll
    for (int a = 0; a < 3; ++a) d[a] = (int64_t)hi[a] - (int64_t)lo[a] + 1;
    const int64_t limit = 2147483647;
    if (d[0] > limit || d[1] > limit || d[2] > limit) return false;
    const int64_t xy = d[0] * d[1];
    if (xy > limit) return false;
    return xy * d[2] <= limit;
}
M3D_FN int64_t voxel_index(const int32_t c[3], const int32_t lo[3], const int64_t d[3]) {
    return ((int64_t)c[0] - lo[0]) + ((int64_t)c[1] - lo[1]) * d[0] + ((int64_t)c[2] - lo[2]) * d[0] * d[1];
}

// ---- step 3: the sums over the neighbours of p, in the order they are offered
struct Acc { float S[3], SS[6]; };
M3D_FN void acc_clear(Acc& a) {
#pragma unroll
    for (int k = 0; k < 3; ++k) a.S[k] = 0.0f;
#pragma unroll
    for (int k = 0; k < 6; ++k) a.SS[k] = 0.0f;
}
M3D_FN void acc_add(Acc& a, float px, float py, float pz, float qx, float qy, float qz) {
    const float ux = qx - px, uy = qy - py, uz = qz - pz;
    a.S[0] = a.S[0] + ux; a.S[1] = a.S[1] + uy; a.S[2] = a.S[2] + uz;
    const float xx = ux * ux, xy = ux * uy, xz = ux * uz, yy = uy * uy, yz = uy * uz, zz = uz * uz;
    a.SS[0] = a.SS[0] + xx; a.SS[1] = a.SS[1] + xy; a.SS[2] = a.SS[2] + xz;
    a.SS[3] = a.SS[3] + yy; a.SS[4] = a.SS[4] + yz; a.SS[5] = a.SS[5] + zz;
}
// a neighbour's key in K mode: d2 is never negative, so the keys order as (d2, row)
M3D_FN uint64_t neighbour_key(float d2, int row) { return ((uint64_t)m3d::bits_of(d2) << 32) | (uint32_t)row; }
M3D_FN float radius2(float radius) { return radius * radius; }

// n is negated iff it points away from vp as seen from p
M3D_FN bool points_away(const float vp[3], float px, float py, float pz, const float n[3]) {
    const float vx = vp[0] - px, vy = vp[1] - py, vz = vp[2] - pz;
    const float a = vx * n[0], b = vy * n[1], c = vz * n[2];
    const float ab = a + b;
    return (ab + c) < 0.0f;
}
// the normal of p out of the sums over its n neighbours; three NaNs with fewer than three
M3D_FN void normal_of(const Acc& acc, int n, float px, float py, float pz, const float vp[3], float out[3]) {
    if (n < 3) {
#pragma unroll
        for (int k = 0; k < 3; ++k) out[k] = m3d::float_of(QUIET_NAN);
        return;
    }
    const float fn = (float)n;
    float m[3], cov[6];
#pragma unroll
    for (int a = 0; a < 3; ++a) m[a] = acc.S[a] / fn;
    const int ia[6] = {0, 0, 0, 1, 1, 2}, ib[6] = {0, 1, 2, 1, 2, 2};
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const float q = acc.SS[k] / fn;
        const float mm = m[ia[k]] * m[ib[k]];
        cov[k] = q - mm;
    }
    float A[4][4], V[4][4];
    icpp::jacobi3(cov, A, V);
    // the smallest value's vector, the lower index among equals; values are selected, never an address
    float best = A[0][0];
    float e[3] = {V[0][0], V[1][0], V[2][0]};
    if (A[1][1] < best) { best = A[1][1]; e[0] = V[0][1]; e[1] = V[1][1]; e[2] = V[2][1]; }
    if (A[2][2] < best) { best = A[2][2]; e[0] = V[0][2]; e[1] = V[1][2]; e[2] = V[2][2]; }
    const bool flip = points_away(vp, px, py, pz, e);
#pragma unroll
    for (int k = 0; k < 3; ++k) out[k] = flip ? -e[k] : e[k];
}

// ---- step 5 (adjustNormalsToViewPoint with the viewpoint (0, 0, 10))
M3D_FN void ground_up(float up, float px, float py, float pz, float n[3]) {
    const float vp[3] = {0.0f, 0.0f, 10.0f};
    if (points_away(vp, px, py, pz, n) || (n[2] < -up && pz < 10.0f)) {
#pragma unroll
        for (int k = 0; k < 3; ++k) n[k] = -n[k];
    }
}

}  // namespace scf
}  // namespace lcd
