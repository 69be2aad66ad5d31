// Motion2D.cpp -- see Motion2D.h.
#include "Motion2D.h"

#include <algorithm>
#include <cmath>

#include "../csrc/motion_pnp_rule.h"
#include "LaneSum.h"
#include "MotionMirror.h"

namespace rtabmap_amd {

namespace {

namespace rule = lcd::pnp;
namespace common = lcd::m3d;

// the backend of rule::solve as a loop; X: the correspondences' coordinates, [planes][m] (from x, y, z, to u, v and, with points, to x, y, z)
struct CpuBackend : MirrorState {
    int m;
    const float* X;
    bool has_to;
    rule::Camera cam;
    uint32_t seed;
    int iterations, steps;
    float model0[12];
    std::vector<float> last_e;

    float at(int c, int i) const { return X[(size_t)c * m + i]; }
    bool inlier(const float model[12], int i, float thr, float& e) const {
        bool front;
        e = rule::reproj_error(model, cam, at(0, i), at(1, i), at(2, i), at(3, i), at(4, i), front);
        return rule::is_inlier(e, front, thr);
    }
    bool hypothesis(int h, float model[12]) const {
        int i[4];
        if (!rule::draw4(seed, (uint32_t)h, (uint32_t)m, i[0], i[1], i[2], i[3])) return false;
        float P[3][3], B[3][3];
        for (int k = 0; k < 3; ++k) {
            for (int a = 0; a < 3; ++a) P[k][a] = at(a, i[k]);
            rule::bearing(cam, at(3, i[k]), at(4, i[k]), B[k]);
        }
        return rule::p3p(P, B, at(0, i[3]), at(1, i[3]), at(2, i[3]), at(3, i[3]), at(4, i[3]), cam, common::SWEEPS, model);
    }
    bool candidate(int c, float model[12]) const {
        if (c > 0) return hypothesis(c - 1, model);
        for (int k = 0; k < 12; ++k) model[k] = model0[k];
        return true;
    }
    uint64_t ransac(float thr) {
        return bestCandidate(iterations + 1, m, cur, [&](int c, float* model) { return candidate(c, model); },
                             [&](const float* model, int i) { float e; return inlier(model, i, thr, e); });
    }
    void fit_prev() {
        const int n = (int)prev.size();
        if (n < 4) return;
        float q[4], t[3] = {cur[3], cur[7], cur[11]};
        rule::quat_of_model(cur, q);
        std::vector<float> terms((size_t)n * rule::SUMS);
        for (int s = 0; s < steps; ++s) {
            float model[12], S[rule::SUMS], delta[6];
            rule::model_of_pose(q, t, model);
            for (int i = 0; i < n; ++i) {
                const int j = prev[(size_t)i];
                rule::gn_terms(model, cam, at(0, j), at(1, j), at(2, j), at(3, j), at(4, j), &terms[(size_t)i * rule::SUMS]);
            }
            for (int k = 0; k < rule::SUMS; ++k) S[k] = laneTreeSum<common::LANES>(n, [&](int i) { return terms[(size_t)i * rule::SUMS + k]; });
            if (rule::gn_solve(S, delta)) rule::pose_update(q, t, delta);
        }
        rule::model_of_pose(q, t, cur);
    }
    int select(float thr) {
        return MirrorState::select(m, last_e, [&](int i, float& e) { return inlier(cur, i, thr, e); });
    }
    float threshold(float thr0) const { return rule::refined_threshold(last_e.data(), (int)last_e.size(), thr0); }
    void covariance(int kind, const float pose[12], int ratio, double& lin, double& cosine) const {
        const int n = (int)prev.size();
        lin = 1.0; cosine = 1.0;
        if (kind == 1) {
            float cam_pose[12];
            common::invert(cur, cam_pose);
            std::vector<uint32_t> kd((size_t)n), kc((size_t)n);
            for (int i = 0; i < n; ++i) {
                const int j = prev[(size_t)i];
                float d2, c;
                rule::cov_terms(pose, cur, cam_pose, cam, at(0, j), at(1, j), at(2, j), at(3, j), at(4, j), has_to, has_to ? at(5, j) : 0.0f,
                                has_to ? at(6, j) : 0.0f, has_to ? at(7, j) : 0.0f, d2, c);
                kd[(size_t)i] = rule::order_key(d2);
                kc[(size_t)i] = rule::order_key(c);
            }
            const int k = n / ratio;
            std::sort(kd.begin(), kd.end());
            std::sort(kc.begin(), kc.end());
            lin = rule::VARIANCE_FACTOR * (double)rule::key_value(kd[(size_t)k]);
            cosine = (double)rule::key_value(kc[(size_t)(n - 1 - k)]);
        } else {
            float err = 0.0f;                                          // :264-270, in the inliers' order
            for (int i = 0; i < n; ++i) {
                bool front;
                const int j = prev[(size_t)i];
                const float ee = rule::reproj_sq(cur, cam, at(0, j), at(1, j), at(2, j), at(3, j), at(4, j), front);
                err = err + ee;
            }
            const float mean = err / (float)n;
            lin = (double)sqrtf(mean);
        }
    }
};

const float IDENTITY[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};

}  // namespace

bool motion_pnp_cpu(const int32_t* fromIds, const float* fromXyz, int nFrom, const int32_t* toIds, const float* toPoints, const float* toXyz, int nTo,
                    const lcd_camera& camera, const float* guess, const MotionPnpParams& p, MotionPnpResult& out) {
    if (nFrom < 0 || nTo < 0 || nFrom > common::MAX_ROWS || nTo > common::MAX_ROWS || p.minInliers < 1 || p.iterations < 1 || p.iterations > 65535 ||
        p.refineIterations < 0 || p.varianceMedianRatio <= 1 || p.steps < 0 || !std::isfinite(p.reprojError) || !(p.reprojError > 0.0) ||
        !((float)p.reprojError > 0.0f) || !std::isfinite((float)((double)(float)p.reprojError * (double)(float)p.reprojError)) ||
        !(p.maxVariance >= 0.0f) || !std::isfinite(p.maxVariance))
        return false;
    if ((nFrom > 0 && (!fromIds || !fromXyz)) || (nTo > 0 && (!toIds || !toPoints))) return false;
    const std::map<int32_t, int> from = uniqueRows(fromIds, nFrom), to = uniqueRows(toIds, nTo);
    const bool has_to = toXyz != nullptr;
    const int planes = has_to ? 8 : 5;
    MotionPnpResult r;
    std::vector<float> coords[8];
    for (const auto& t : to) {                                         // util3d_motion_estimation.cpp:89-106
        const auto f = from.find(t.first);
        if (f == from.end()) continue;
        const float* q = fromXyz + (size_t)f->second * 3;
        if (!(common::finite(q[0]) && common::finite(q[1]) && common::finite(q[2]))) continue;
        r.matches.push_back(t.first);
        for (int a = 0; a < 3; ++a) coords[a].push_back(q[a]);
        coords[3].push_back(toPoints[(size_t)t.second * 2]);
        coords[4].push_back(toPoints[(size_t)t.second * 2 + 1]);
        if (has_to)
            for (int a = 0; a < 3; ++a) coords[5 + a].push_back(toXyz[(size_t)t.second * 3 + a]);
    }
    const int m = (int)r.matches.size();
    std::vector<float> X((size_t)m * planes);
    for (int c = 0; c < planes; ++c) std::copy(coords[c].begin(), coords[c].end(), X.begin() + (size_t)c * m);
    CpuBackend b;
    b.m = m; b.X = X.data(); b.has_to = has_to; b.seed = p.seed; b.iterations = p.iterations; b.steps = p.steps ? p.steps : rule::STEPS;
    b.cam = rule::Camera{camera.fx, camera.fy, camera.cx, camera.cy, camera.image_width, camera.image_height};
    const bool has_local = camera.has_local_transform != 0;
    rule::model_of_guess(guess ? guess : IDENTITY, has_local, camera.local_transform, b.model0);
    for (int k = 0; k < 12; ++k) b.cur[k] = 0.0f;
    const int kind = has_to || camera.image_width != 0 || camera.image_height != 0 ? 1 : 2;
    rule::Result res;
    rule::solve(b, m, p.minInliers, p.refineIterations, p.reprojError, p.varianceMedianRatio, p.maxVariance, kind, has_local, camera.local_transform, res);
    for (int k = 0; k < 12; ++k) r.transform[k] = res.transform[k];
    r.status = res.status;
    r.varianceKind = res.kind;
    r.varianceLin = res.variance_lin;
    r.angleCos = res.angle_cos;
    for (int j = 0; j < res.n_inliers; ++j) r.inliers.push_back(r.matches[(size_t)b.prev[(size_t)j]]);
    out = r;
    return true;
}

void motion_pnp_covariance(int varianceKind, double varianceLin, double angleCos, double* covariance) {
    for (int k = 0; k < 36; ++k) covariance[k] = k % 7 == 0 ? 1.0 : 0.0;
    if (varianceKind == 1) {
        const double ang = lcd::pnp::VARIANCE_FACTOR * std::acos(angleCos);
        for (int k = 0; k < 3; ++k) { covariance[7 * k] = varianceLin; covariance[7 * (k + 3)] = ang; }
    } else if (varianceKind == 2) {
        for (int k = 0; k < 6; ++k) covariance[7 * k] = varianceLin;
    }
}

Transform3D Motion2D::estimateMotion3DTo2D(lcd_engine* engine, const std::multimap<int, Point3f>& words3A, const std::multimap<int, Point2f>& words2B,
                                           const lcd_camera& camera, int minInliers, int iterations, double reprojError, int refineIterations,
                                           int varianceMedianRatio, float maxVariance, const Transform3D& guess,
                                           const std::multimap<int, Point3f>& words3B, double* covariance, std::vector<int>* matchesOut,
                                           std::vector<int>* inliersOut, uint32_t seed) {
    Transform3D transform;
    if (covariance) motion_pnp_covariance(0, 1.0, 1.0, covariance);
    if (matchesOut) matchesOut->clear();
    if (inliersOut) inliersOut->clear();
    std::vector<int32_t> fromIds, toIds;
    std::vector<float> fromXyz, toPoints, toXyz;
    for (const auto& w : words3A) {
        fromIds.push_back(w.first);
        fromXyz.push_back(w.second.x); fromXyz.push_back(w.second.y); fromXyz.push_back(w.second.z);
    }
    const float nan = std::nanf("");
    for (const auto& w : words2B) {
        toIds.push_back(w.first);
        toPoints.push_back(w.second.x); toPoints.push_back(w.second.y);
        if (words3B.empty()) continue;
        const auto range = words3B.equal_range(w.first);               // the unique map's entry (RegistrationVis.cpp:1704-1720)
        const bool one = range.first != range.second && std::next(range.first) == range.second;
        toXyz.push_back(one ? range.first->second.x : nan); toXyz.push_back(one ? range.first->second.y : nan); toXyz.push_back(one ? range.first->second.z : nan);
    }
    const int64_t fromOffsets[2] = {0, (int64_t)fromIds.size()}, toOffsets[2] = {0, (int64_t)toIds.size()};
    const size_t region = std::max<size_t>(toIds.size(), 1);
    std::vector<int32_t> matches(region), inliers(region);
    float t[12];
    int32_t status = 0, nMatches = 0, nInliers = 0, kind = 0;
    double lin = 1.0, cosine = 1.0;
    lcd_motion_pnp_args a;
    a.struct_size = (int32_t)sizeof a; a.n_pairs = 1; a.min_inliers = minInliers; a.iterations = iterations; a.refine_iterations = refineIterations;
    a.variance_median_ratio = varianceMedianRatio; a.seed = seed; a.max_variance = maxVariance; a.reproj_error = reprojError;
    a.from_word_ids = fromIds.data(); a.from_xyz = fromXyz.data(); a.to_word_ids = toIds.data(); a.to_points = toPoints.data();
    a.to_xyz = words3B.empty() ? nullptr : toXyz.data();
    a.from_offsets = fromOffsets; a.to_offsets = toOffsets; a.cameras = &camera; a.guesses = guess.isNull() ? nullptr : guess.data;
    a.out_transform = t; a.out_status = &status; a.out_n_matches = &nMatches; a.out_n_inliers = &nInliers;
    a.out_variance_lin = &lin; a.out_angle_cos = &cosine; a.out_variance_kind = &kind;
    a.out_matches = matches.data(); a.out_inliers = inliers.data();
    if (!engine || lcd_estimate_motion_pnp(engine, &a) != LCD_OK) return transform;
    if (covariance) motion_pnp_covariance(kind, lin, cosine, covariance);
    if (matchesOut) matchesOut->assign(matches.begin(), matches.begin() + nMatches);
    if (inliersOut) inliersOut->assign(inliers.begin(), inliers.begin() + nInliers);
    for (int k = 0; k < 12; ++k) transform.data[k] = t[k];
    return transform;
}

}  // namespace rtabmap_amd
