// motion_3d_rule.h -- the rule of lcd_estimate_motion_3d (include/lcd.h writes it down with the reference's line numbers) as functions the
// kernel (motion_3d.hip) and the host mirror (rtabmap_amd/host/Motion3D.cpp) compile alike.  All point arithmetic is fp32, one rounded
// operation per statement, never contracted: no product is fused into a sum; division and square root are IEEE.  The threshold, the variance
// and the comparison against the threshold are fp64.  What needs the correspondences as a whole (sums over a set, the selection, the median,
// the hypotheses' scores) is a backend's: the kernel's works as a workgroup, the mirror's as a loop; solve() and refine() drive either.  Internal.
#pragma once
#include "motion_rule_common.h"

namespace lcd {
namespace m3d {

constexpr int SWEEPS = 5;                    // cyclic Jacobi sweeps of the 4 x 4 eigenproblem (how the count was chosen)
constexpr int ST_OK = 0, ST_FEW_CORRESPONDENCES = 1, ST_NO_MODEL = 2, ST_FEW_INLIERS = 3, ST_BELOW_MIN_INLIERS = 4;   // lcd_motion_3d_status
constexpr double VARIANCE_FACTOR = 2.1981;   // computeVariance: the factor in front of the median
constexpr double REFINE_SIGMA = 3.0;         // util3d_motion_estimation.cpp:783

// findCorrespondences' test (util3d_correspondences.cpp:388-392, maxDepth == 0)
M3D_FN bool keep_pair(float px, float py, float pz, float qx, float qy, float qz) {
    if (!(finite(px) && finite(py) && finite(pz) && finite(qx) && finite(qy) && finite(qz))) return false;
    return (px != 0.0f || py != 0.0f || pz != 0.0f) && (qx != 0.0f || qy != 0.0f || qz != 0.0f);
}

// hypothesis h's three distinct correspondence indices among m (>= 1); false: not found within MAX_DRAWS draws
M3D_FN bool draw3(uint32_t seed, uint32_t h, uint32_t m, int& i0, int& i1, int& i2) {
    const uint32_t base = mix(seed + h) * 3u;
    int got = 0;
    i0 = i1 = i2 = 0;
    for (int k = 0; k < MAX_DRAWS; ++k) {
        const int d = (int)(mix(base + (uint32_t)k) % m);
        if ((got > 0 && d == i0) || (got > 1 && d == i1)) continue;
        i0 = got == 0 ? d : i0;
        i1 = got == 1 ? d : i1;
        i2 = got == 2 ? d : i2;
        if (++got == 3) return true;
    }
    return false;
}

// the squared distance of R p + t from q
M3D_FN float dist2(const float m[12], float px, float py, float pz, float qx, float qy, float qz) {
    const float x0 = m[0] * px, x1 = m[1] * py, x2 = m[2] * pz;
    const float x01 = x0 + x1;
    const float x012 = x01 + x2;
    const float x = x012 + m[3];
    const float y0 = m[4] * px, y1 = m[5] * py, y2 = m[6] * pz;
    const float y01 = y0 + y1;
    const float y012 = y01 + y2;
    const float y = y012 + m[7];
    const float z0 = m[8] * px, z1 = m[9] * py, z2 = m[10] * pz;
    const float z01 = z0 + z1;
    const float z012 = z01 + z2;
    const float z = z012 + m[11];
    const float dx = x - qx, dy = y - qy, dz = z - qz;
    const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
    const float xy = xx + yy;
    return xy + zz;
}

M3D_FN double threshold_of(double inlier_distance, double variance) {
    const double sigma = REFINE_SIGMA * sqrt(variance);
    return sigma < inlier_distance ? sigma : inlier_distance;          // std::min(inlierThreshold, refineSigma * sqrt(variance))
}

struct Result {
    float transform[12];
    int32_t status, n_inliers;
    double variance;
};

// The backend B holds the correspondences, a current model and two index sets, `prev` and `next`.  Every call is made by all threads of a
// workgroup alike (the kernel) or by the one caller (the mirror), and returns the same value to each:
//   uint64_t ransac()          evaluate every hypothesis; (count << 32) | ~h of the best one, 0 for none; on != 0 the model is hypothesis h's
//   void fit_prev()            the model becomes the fit of `prev` (LANES-lane sums); unchanged when prev holds fewer than three
//   int select(double thr2)    `next` = the correspondences with (double)d2 < thr2, ascending; their d2 are "the last selection"
//   double variance()          VARIANCE_FACTOR x the element of rank (size >> 1) of the last selection's d2
//   void swap_sets(); void clear_next(); int prev_n(); int next_n(); bool same_members()
//   const float* model()

// transformFromXYZCorrespondences' refinement loop (util3d_registration.cpp:115-196), literally; afterwards the inliers are `next`
template <class B>
M3D_FN void refine(B& b, double inlier_distance, int refine_iterations) {
    double error_threshold = inlier_distance;
    int it = 0;
    bool inlier_changed = false;
    int sizes[4] = {0, 0, 0, 0}, n_sizes = 0;                           // the last four of inliers_sizes, oldest first
    do {
        b.fit_prev();
        sizes[0] = sizes[1]; sizes[1] = sizes[2]; sizes[2] = sizes[3]; sizes[3] = b.prev_n(); ++n_sizes;
        const int found = b.select(error_threshold * error_threshold);
        if (found == 0) {
            ++it;
            if (it >= refine_iterations) break;
            continue;
        }
        const double variance = b.variance();
        error_threshold = threshold_of(inlier_distance, variance);
        inlier_changed = false;
        b.swap_sets();
        if (b.next_n() != b.prev_n()) {
            if (n_sizes >= 4 && sizes[3] == sizes[1] && sizes[2] == sizes[0]) break;   // oscillating
            inlier_changed = true;
            continue;
        }
        if (!b.same_members()) inlier_changed = true;
    } while (inlier_changed && ++it < refine_iterations);
}

// everything behind the correspondences: m of them
template <class B>
M3D_FN void solve(B& b, int m, int min_inliers, int refine_iterations, double inlier_distance, Result& r) {
#pragma unroll
    for (int k = 0; k < 12; ++k) r.transform[k] = 0.0f;
    r.n_inliers = 0;
    r.variance = 1.0;
    if (m < min_inliers || m < 3) { r.status = ST_FEW_CORRESPONDENCES; return; }
    if (b.ransac() == 0) { r.status = ST_NO_MODEL; return; }
    (void)b.select(inlier_distance * inlier_distance);
    b.swap_sets();                                                     // prev = the best model's inliers
    b.clear_next();
    if (refine_iterations > 0) {
        refine(b, inlier_distance, refine_iterations);
        b.swap_sets();                                                 // std::swap(inliers, new_inliers): the result is in prev again
    }
    const int n = b.prev_n();
    if (n < 3) { r.status = ST_FEW_INLIERS; return; }
    r.n_inliers = n;
    r.variance = b.variance();
    if (n < min_inliers) { r.status = ST_BELOW_MIN_INLIERS; return; }
    float pose[12];
    invert(b.model(), pose);
#pragma unroll
    for (int k = 0; k < 12; ++k) r.transform[k] = pose[k];
    r.status = ST_OK;
}

}  // namespace m3d
}  // namespace lcd
