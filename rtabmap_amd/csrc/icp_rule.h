// icp_rule.h -- the rule of lcd_register_icp (include/lcd.h writes it down with the reference's line numbers) as functions the kernel
// (register_icp.hip) and the host mirror (rtabmap_amd/host/RegistrationIcp.cpp) compile alike.  All point arithmetic is fp32, one rounded
// operation per statement, never contracted; division and square root are IEEE.  The correspondence threshold, its comparison and the variance
// are fp64.  What needs a cloud as a whole (the searches, the sums, the median) is a backend's: the kernel's works as a workgroup, the mirror's
// as a loop; solve() drives either.  How a backend finds a nearest neighbour is its own affair as long as it returns what nearer() defines.
// Internal.
#pragma once
#include <cfloat>

#include "motion_3d_rule.h"

namespace lcd {
namespace icp {

using m3d::apply;
using m3d::compose;
using m3d::finite;
using m3d::horn_fit;
using m3d::invert;

constexpr int ST_OK = 0, ST_EMPTY = 1, ST_NOT_CONVERGED = 2, ST_BELOW_RATIO = 3;                                   // lcd_icp_status
constexpr int STOP_NONE = 0, STOP_ITERATIONS = 1, STOP_TRANSFORM = 2, STOP_MSE = 3, STOP_FEW_CORRESPONDENCES = 4;  // lcd_icp_stop
constexpr int SEARCH_AUTO = 0, SEARCH_BRUTE = 1, SEARCH_GRID = 2;                                                  // lcd_icp_search
constexpr int MIN_CORRESPONDENCES = 3;       // pcl::Registration::min_number_correspondences_, and the guard of util3d_registration.cpp:352
constexpr float MSE_EPS = 1e-12f;            // pcl::registration::DefaultConvergenceCriteria::mse_threshold_absolute_
constexpr double VARIANCE_FACTOR = 2.1981;   // util3d_registration.cpp:355

// a row takes part iff its three coordinates are finite
M3D_FN bool takes_part(float x, float y, float z) { return finite(x) && finite(y) && finite(z); }

// the squared distance of step 2
M3D_FN float dist2(float px, float py, float pz, float cx, float cy, float cz) {
    const float dx = px - cx, dy = py - cy, dz = pz - cz;
    const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
    const float xy = xx + yy;
    return xy + zz;
}

// Step 2's order: the nearest row starts as (+inf, -1), rows are offered in ANY order, and (d2, row) replaces (best, best_row) iff this
// holds.  A NaN and +inf never win, so a row with no finite distance has no neighbour.
M3D_FN bool nearer(float d2, int row, float best, int best_row) { return d2 < best || (d2 == best && row < best_row); }

// a nearest row is a correspondence iff it exists and double(d2) <= thr2 (PCL drops distance > max_dist_sqr)
M3D_FN bool corresponds(int row, float d2, double thr2) { return row >= 0 && (double)d2 <= thr2; }

// ---- the grid form of the search: an IMPLEMENTATION of step 2, never part of the rule.  Only correspondences (double(d2) <= thr2) and step
// 8's reciprocal test reach an output, and both need a nearest row only where it lies within the threshold; so a search that looks at the
// 27 cells around a row returns the same outputs, provided no pair with double(d2) <= thr2 sits more than one cell apart on any axis.
// The cell is h = float(max_correspondence_distance) * CELL_MARGIN and a coordinate's cell is floor(x / h), for quotients below CELL_LIMIT in
// magnitude.  Why one cell is enough: d2 >= fl(dx * dx) (1 - 2^-23) and dx = fl(p - q), so |p - q| <= thr (1 + 2^-21); h >= thr
// CELL_MARGIN (1 - 2^-22); the two rounded quotients are each within 2^-24 x 2^16 of the real ones; so they differ by at most
// (1 + 2^-20) / CELL_MARGIN + 2^-7 = 0.949 < 1, and the floors of two numbers less than 1 apart differ by at most 1.  (IEEE division is
// monotone, so the order of the cells is the order of the coordinates.)  tests/test_register_icp_model.py checks this against brute force.
constexpr float CELL_MARGIN = 1.0625f;
constexpr float CELL_LIMIT = 65535.0f;       // cells -65535 .. 65534, their neighbours -65536 .. 65535: 17 bits an axis
constexpr int CELL_BITS = 17, CELL_BIAS = 1 << 16, ROW_BITS = 13;
constexpr uint64_t ROW_MASK = (1u << ROW_BITS) - 1;
static_assert(3 * CELL_BITS + ROW_BITS == 64 && (1 << ROW_BITS) == m3d::MAX_ROWS, "a key is three cells and a row");
// The target size from which AUTO takes the grid form.  Measured on one MI355X, one pair per call, 5 iterations, threshold 0.3 m, device time
// (profiles/register_icp.txt has both curves): the grid overtakes the brute form between 360 and 512 points on a 2-D scan (0.264 / 0.276 ms
// at 360, 0.331 / 0.320 at 512, 1.50 / 0.875 at 1081) and between 1536 and 2048 on a 3-D cloud (2.52 / 2.56 ms at 1536, 4.40 / 3.80 at 2048),
// whose 27 cells hold surfaces, not a line.  One constant between the two crossings: at 1024 a 3-D cloud pays 18 % (1.19 / 1.41 ms) until
// about 1600 points, and a 2-D scan of 512 .. 1023 forgoes up to 22 %.
constexpr int AUTO_GRID_ROWS = 1024;

M3D_FN float cell_size(double max_correspondence_distance) {
    const float t = max_correspondence_distance > (double)FLT_MAX ? m3d::float_of(0x7f800000u) : (float)max_correspondence_distance;
    return t * CELL_MARGIN;
}
// false: the coordinate does not fit the key's cell range (or h is 0 or the quotient a NaN)
M3D_FN bool cell_of(float x, float h, int& c) {
    const float u = x / h;
    const float mag = m3d::float_of(m3d::bits_of(u) & 0x7fffffffu);
    if (!(mag < CELL_LIMIT)) return false;
    c = (int)floorf(u);
    return true;
}
// x above y above z above the row: the three z-neighbours of a cell are one run of the sorted keys
M3D_FN uint64_t cell_key(int cx, int cy, int cz, uint64_t row) {
    const uint64_t x = (uint64_t)(cx + CELL_BIAS), y = (uint64_t)(cy + CELL_BIAS), z = (uint64_t)(cz + CELL_BIAS);
    return (((((x << CELL_BITS) | y) << CELL_BITS) | z) << ROW_BITS) | row;
}
M3D_FN bool key_of(float x, float y, float z, float h, uint64_t row, uint64_t& key) {
    int cx, cy, cz;
    if (!(cell_of(x, h, cx) && cell_of(y, h, cy) && cell_of(z, h, cz))) return false;
    key = cell_key(cx, cy, cz, row);
    return true;
}
// The nearest of the rows in the 27 cells around p, under nearer(): key_at(i) is the i-th of the n keys in ascending order, coords(row, x,
// y, z) a row's coordinates.  false: p's cell does not fit the range and the caller walks the whole cloud instead.
template <class KeyAt, class Coords>
M3D_FN bool grid_nearest(KeyAt key_at, int n, Coords coords, float px, float py, float pz, float h, float& best, int& row) {
    best = m3d::float_of(0x7f800000u);
    row = -1;
    int cx, cy, cz;
    if (!(cell_of(px, h, cx) && cell_of(py, h, cy) && cell_of(pz, h, cz))) return false;
    for (int ix = -1; ix <= 1; ++ix)
        for (int iy = -1; iy <= 1; ++iy) {
            const uint64_t lo = cell_key(cx + ix, cy + iy, cz - 1, 0), hi = cell_key(cx + ix, cy + iy, cz + 1, ROW_MASK);
            int a = 0, b = n;
            while (a < b) {
                const int mid = (a + b) >> 1;
                if (key_at(mid) < lo) a = mid + 1; else b = mid;
            }
            for (; a < n; ++a) {
                const uint64_t k = key_at(a);
                if (k > hi) break;
                const int r = (int)(k & ROW_MASK);
                float x, y, z;
                coords(r, x, y, z);
                const float d = dist2(px, py, pz, x, y, z);
                if (nearer(d, r, best, row)) { best = d; row = r; }
            }
        }
    return true;
}
// which form a target of `rows` participating rows is searched in
M3D_FN bool wants_grid(int search, int rows) { return search == SEARCH_GRID || (search == SEARCH_AUTO && rows >= AUTO_GRID_ROWS); }

// step 4, 2-D: the rotation about z and the translation in the plane
M3D_FN void fit_2d(const float cp[3], const float cq[3], const float S[9], float model[12]) {
    const float A = S[0] + S[4];             // Sxx + Syy
    const float B = S[1] - S[3];             // Sxy - Syx
    const float aa = A * A, bb = B * B;
    const float n2 = aa + bb;
    const float n = sqrtf(n2);
    float c = 1.0f, s = 0.0f;
    if (n != 0.0f && finite(n)) { c = A / n; s = B / n; }
    const float cx = c * cp[0], sy = s * cp[1], sx = s * cp[0], cy = c * cp[1];
    const float rx = cx - sy, ry = sx + cy;
    model[0] = c; model[1] = -s; model[2] = 0.0f; model[3] = cq[0] - rx;
    model[4] = s; model[5] = c; model[6] = 0.0f; model[7] = cq[1] - ry;
    model[8] = 0.0f; model[9] = 0.0f; model[10] = 1.0f; model[11] = 0.0f;
}

// step 4: T_k from the centroids and the nine sums
M3D_FN void fit(const float cp[3], const float cq[3], const float S[9], bool force_3dof, float model[12]) {
    if (force_3dof) fit_2d(cp, cq, S, model);
    else horn_fit(cp, cq, S, m3d::SWEEPS, model);
}

// step 6, behind the increment of `iterations`
M3D_FN int stop_of(const float T[12], int iterations, int max_iterations, float eps2, float mse, float mse_prev) {
    if (iterations >= max_iterations) return STOP_ITERATIONS;
    const float t01 = T[0] + T[5];
    const float tr = t01 + T[10];
    const float trm = tr - 1.0f;
    const float cosine = 0.5f * trm;
    const float rot_thr = 1.0f - eps2;
    const float xx = T[3] * T[3], yy = T[7] * T[7], zz = T[11] * T[11];
    const float xy = xx + yy;
    const float t2 = xy + zz;
    if (cosine >= rot_thr && t2 <= eps2) return STOP_TRANSFORM;
    const float diff = mse - mse_prev;
    const float mag = m3d::float_of(m3d::bits_of(diff) & 0x7fffffffu);
    if (mag < MSE_EPS) return STOP_MSE;
    return STOP_NONE;
}

struct Result {
    float transform[12], icp[12], correction[12];
    int32_t status, stop, iterations, n_correspondences;
    float ratio;
    double variance;
};

// The backend B holds the pair: the source's current cloud (at first the participating from-rows), the target Q and the per-row results of
// its searches.  Every call is made by all threads of a workgroup alike (the kernel) or by the one caller (the mirror), and returns the same
// value to each:
//   int n_from(); int n_to()              participating rows
//   int correspond(float& sum_d2)         step 3: nearest row in Q of every row of the current cloud; the number that are correspondences, and
//                                         SUM of their d2
//   void fit(int c, bool flat, float T[12])   step 4 over those correspondences
//   void advance(const float T[12])       the current cloud becomes T(current cloud)
//   void set_registered(const float F[12])    the current cloud becomes F(P_0)
//   int reciprocal(bool from_is_target)   step 8 over the current cloud and Q: writes out_match, returns the number of correspondences
//   float median(int n)                   the d2 of rank n >> 1 among the n correspondences of reciprocal()
// steps 3 to 6 over the backend's clouds: F, the iterations and the stop.  false: fewer than three correspondences in an iteration (r is final)
template <class B>
M3D_FN bool loop(B& b, int max_iterations, bool force_3dof, float epsilon, float F[12], Result& r) {
#pragma unroll
    for (int k = 0; k < 12; ++k) F[k] = (k == 0 || k == 5 || k == 10) ? 1.0f : 0.0f;
    const float eps2 = epsilon * epsilon;
    float mse_prev = FLT_MAX;
    int stop;
    for (;;) {
        float sum_d2;
        const int c = b.correspond(sum_d2);
        if (c < MIN_CORRESPONDENCES) { r.status = ST_NOT_CONVERGED; r.stop = STOP_FEW_CORRESPONDENCES; return false; }
        const float mse = sum_d2 / (float)c;
        float T[12], G[12];
        b.fit(c, force_3dof, T);
        b.advance(T);
        compose(T, F, G);
#pragma unroll
        for (int k = 0; k < 12; ++k) F[k] = G[k];
        ++r.iterations;
        stop = stop_of(T, r.iterations, max_iterations, eps2, mse, mse_prev);
        if (stop != STOP_NONE) break;
        mse_prev = mse;
    }
    r.stop = stop;
    return true;
}

// steps 9 and 10 from F, the number of correspondences kept and the ratio's denominator without max_laser_scans
M3D_FN void outputs(const float F[12], const float guess[12], int n, int larger, int max_laser_scans, float correspondence_ratio, Result& r) {
    r.ratio = (float)n / (float)(max_laser_scans > 0 ? max_laser_scans : larger);
    float Finv[12], X[12], Ginv[12], C[12];
    invert(F, Finv);
    compose(Finv, guess, X);
    invert(guess, Ginv);
    compose(Ginv, X, C);
#pragma unroll
    for (int k = 0; k < 12; ++k) { r.icp[k] = F[k]; r.correction[k] = C[k]; }
    if (r.ratio <= correspondence_ratio) { r.status = ST_BELOW_RATIO; return; }
#pragma unroll
    for (int k = 0; k < 12; ++k) r.transform[k] = X[k];
    r.status = ST_OK;
}

M3D_FN void clear(Result& r) {
#pragma unroll
    for (int k = 0; k < 12; ++k) { r.transform[k] = 0.0f; r.icp[k] = 0.0f; r.correction[k] = 0.0f; }
    r.stop = STOP_NONE; r.iterations = 0; r.n_correspondences = 0; r.ratio = 0.0f; r.variance = 1.0;
}

template <class B>
M3D_FN void solve(B& b, int max_iterations, bool force_3dof, int max_laser_scans, float epsilon, float correspondence_ratio, const float guess[12], Result& r) {
    clear(r);
    const int nf = b.n_from(), nt = b.n_to();
    if (nf == 0 || nt == 0) { r.status = ST_EMPTY; return; }
    float F[12];
    if (!loop(b, max_iterations, force_3dof, epsilon, F, r)) return;
    b.set_registered(F);
    const int n = b.reciprocal(nf > nt);
    r.n_correspondences = n;
    if (n >= MIN_CORRESPONDENCES) r.variance = VARIANCE_FACTOR * (double)b.median(n);
    outputs(F, guess, n, nf > nt ? nf : nt, max_laser_scans, correspondence_ratio, r);
}

}  // namespace icp
}  // namespace lcd
