// MotionBA.cpp -- see MotionBA.h.
#include "MotionBA.h"

#include <algorithm>
#include <cmath>

#include "../csrc/motion_ba_rule.h"
#include "LaneSum.h"
#include "MotionMirror.h"

namespace rtabmap_amd {

namespace {

namespace rule = lcd::ba;
namespace common = lcd::m3d;

// SUM64: LaneSum.h's order in fp64
template <class F>
double laneTreeSum64(int n, F e) {
    double part[common::LANES];
    for (int l = 0; l < common::LANES; ++l) part[l] = 0.0;
    for (int i = 0; i < n; ++i) part[i % common::LANES] = part[i % common::LANES] + e(i);
    for (int s = common::LANES / 2; s >= 1; s >>= 1)
        for (int l = 0; l < s; ++l) part[l] = part[l] + part[l + s];
    return part[0];
}

// the backend of rule::solve as a loop
struct CpuBackend {
    rule::Frame f;
    float C0[12];
    float cur[12], moved[12];
    float q[4], t[3], q_saved[4], t_saved[3];
    std::vector<rule::Point> pts;
    std::vector<float> saved;                                          // [n x 3]
    std::vector<float> depth_to;
    std::vector<int32_t> ids, kept;
    float cx, cy;
    int32_t width, height;

    int n() const { return (int)pts.size(); }
    double cost_under(const float model[12]) const {
        const double points = laneTreeSum64(n(), [&](int i) { float a, b; return rule::point_cost(f, model, pts[(size_t)i], a, b); });
        float e[6], qe[4], rt[3];
        rule::prior_error(model, C0, e, qe, rt);
        return points + rule::prior_cost(f, e);
    }
    double cost() const { return cost_under(cur); }
    float max_diagonal() const {
        float top = 0.0f;
        std::vector<rule::Blocks> B((size_t)n());
        for (int i = 0; i < n(); ++i) {
            if (!rule::point_blocks(f, cur, pts[(size_t)i], B[(size_t)i])) continue;
            const float* H = B[(size_t)i].Hpp;
            top = H[0] > top ? H[0] : top; top = H[3] > top ? H[3] : top; top = H[5] > top ? H[5] : top;
        }
        rule::Prior pr;
        rule::prior_system(f, cur, C0, pr);
        for (int d = 0; d < 6; ++d) {
            const int o = rule::diag6(d);
            const float s = laneTreeSum<common::LANES>(n(), [&](int i) { return B[(size_t)i].Hcc[o]; });
            const float v = s + pr.P[o];
            top = v > top ? v : top;
        }
        return top;
    }
    bool trial(float lambda, double& F, double& scale) {
        const int m = n();
        std::vector<rule::Blocks> B((size_t)m);
        std::vector<char> active((size_t)m);
        std::vector<float> terms((size_t)m * rule::SUMS, 0.0f);
        for (int i = 0; i < m; ++i) {
            active[(size_t)i] = rule::point_blocks(f, cur, pts[(size_t)i], B[(size_t)i]) ? 1 : 0;
            if (active[(size_t)i]) rule::point_terms(B[(size_t)i], lambda, &terms[(size_t)i * rule::SUMS]);
        }
        float S[rule::SUMS], dc[6];
        for (int c = 0; c < rule::SUMS; ++c) S[c] = laneTreeSum<common::LANES>(m, [&](int i) { return terms[(size_t)i * rule::SUMS + c]; });
        rule::Prior pr;
        rule::prior_system(f, cur, C0, pr);
        for (int k = 0; k < 4; ++k) q_saved[k] = q[k];
        for (int k = 0; k < 3; ++k) t_saved[k] = t[k];
        double scale0 = 0.0;
        if (!rule::camera_step(f, S, pr, lambda, q, t, dc, scale0)) return false;
        lcd::pnp::model_of_pose(q, t, moved);
        std::vector<double> sc((size_t)m, 0.0);
        for (int i = 0; i < m; ++i) {
            rule::Point& p = pts[(size_t)i];
            for (int a = 0; a < 3; ++a) saved[(size_t)3 * i + a] = p.p[a];
            if (!active[(size_t)i]) continue;
            float dp[3];
            rule::point_step(B[(size_t)i], lambda, dc, dp, sc[(size_t)i]);
            for (int a = 0; a < 3; ++a) p.p[a] = p.p[a] + dp[a];
        }
        const double s = laneTreeSum64(m, [&](int i) { return sc[(size_t)i]; });
        scale = s + scale0;
        F = cost_under(moved);
        return true;
    }
    void restore() {
        for (int i = 0; i < n(); ++i)
            for (int a = 0; a < 3; ++a) pts[(size_t)i].p[a] = saved[(size_t)3 * i + a];
        for (int k = 0; k < 4; ++k) q[k] = q_saved[k];
        for (int k = 0; k < 3; ++k) t[k] = t_saved[k];
    }
    void accept() { for (int k = 0; k < 12; ++k) cur[k] = moved[k]; }
    void flag_outliers() {
        for (rule::Point& p : pts) {
            float cf, ct;
            (void)rule::point_cost(f, cur, p, cf, ct);
            uint32_t add = 0;
            if (rule::from_active(p.flags) && cf > f.delta) add |= rule::F_FROM_OUT;
            if (rule::to_active(p.flags) && ct > f.delta) add |= rule::F_TO_OUT;
            if (!add) continue;
            p.flags |= add | rule::F_OUTLIER;
            for (int a = 0; a < 3; ++a) p.p[a] = p.p0[a];
        }
    }
    int survivors() {
        kept.clear();
        for (int i = 0; i < n(); ++i) if (!(pts[(size_t)i].flags & rule::F_OUTLIER)) kept.push_back(i);
        return (int)kept.size();
    }
    float mean_distance(int count, bool& any) const {
        float sum = 0.0f;
        int used = 0;
        for (int j = 0; j < count; ++j) {
            const int i = kept[(size_t)j];
            if (!(pts[(size_t)i].flags & rule::F_TO_FINITE)) continue;
            sum = sum + depth_to[(size_t)i];
            ++used;
        }
        any = used > 0;
        return any ? sum / (float)used : 0.0f;
    }
    float distribution(int count) const {
        std::vector<float> x((size_t)count), y((size_t)count);
        for (int j = 0; j < count; ++j) {
            const rule::Point& p = pts[(size_t)kept[(size_t)j]];
            x[(size_t)j] = rule::normalised(p.ot[0], cx, width);
            y[(size_t)j] = rule::normalised(p.ot[1], cy, height);
        }
        const float nn = (float)count;
        const float sx = laneTreeSum<common::LANES>(count, [&](int j) { return x[(size_t)j]; });
        const float sy = laneTreeSum<common::LANES>(count, [&](int j) { return y[(size_t)j]; });
        const float mx = sx / nn, my = sy / nn;
        const float sxx = laneTreeSum<common::LANES>(count, [&](int j) { const float d = x[(size_t)j] - mx; return d * d; });
        const float sxy = laneTreeSum<common::LANES>(count, [&](int j) { const float d = x[(size_t)j] - mx, e = y[(size_t)j] - my; return d * e; });
        const float syy = laneTreeSum<common::LANES>(count, [&](int j) { const float e = y[(size_t)j] - my; return e * e; });
        const float a = sxx / nn, b = sxy / nn, c = syy / nn;
        return rule::small_eigenvalue(a, b, c);
    }
    const float* model() const { return cur; }
};

const float IDENTITY[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};

bool camera_ok(const lcd_camera& c) { return std::isfinite(c.fx) && std::isfinite(c.fy) && c.fx != 0.0f && c.fy != 0.0f; }

}  // namespace

bool motion_ba_cpu(const int32_t* fromIds, const float* fromXyz, const float* fromPoints, int nFrom, const int32_t* toIds, const float* toPoints,
                   const float* toXyz, int nTo, const int32_t* inliers, int nInliers, const float* transform, const double* priorVariance,
                   const lcd_camera& cameraFrom, const lcd_camera& cameraTo, const MotionBAParams& p, MotionBAResult& out) {
    const float info = (float)(1.0 / p.pixelVariance), delta = (float)p.robustDelta;
    if (nFrom < 0 || nTo < 0 || nFrom > common::MAX_ROWS || nTo > common::MAX_ROWS || p.iterations < 0 || p.iterations > 65535 || p.minInliers < 0 || !std::isfinite(p.pixelVariance) ||
        !(p.pixelVariance > 0.0) || !std::isfinite(info) || !(info > 0.0f) || !std::isfinite(p.robustDelta) || p.robustDelta < 0.0 || !std::isfinite(delta * delta) ||
        !std::isfinite(p.maxInliersMeanDistance) || p.maxInliersMeanDistance < 0.0f || !std::isfinite(p.minInliersDistribution) ||
        p.minInliersDistribution < 0.0f || !std::isfinite(p.baselineFrom) || !std::isfinite(p.baselineTo) || !camera_ok(cameraFrom) || !camera_ok(cameraTo))
        return false;
    if (priorVariance && (!std::isfinite(priorVariance[0]) || !std::isfinite(priorVariance[1]) || priorVariance[0] < 0.0 || priorVariance[1] < 0.0)) return false;
    if ((nFrom > 0 && (!fromIds || !fromXyz)) || (nTo > 0 && (!toIds || !toPoints || !inliers)) || !transform) return false;

    MotionBAResult r;
    for (int k = 0; k < 12; ++k) r.transform[k] = 0.0f;
    r.status = rule::ST_OK; r.nOutliers = 0; r.lmAccepted = 0; r.chi2Before = 0.0; r.chi2After = 0.0; r.inliersMeanDistance = 0.0f; r.inliersDistribution = 0.0f;
    const int n = nInliers;
    const int n_c = std::min(std::max(n, 0), nTo);
    auto pass = [&](int status) {
        r.status = status;
        r.inliers.assign(inliers, inliers + n_c);
        out = r;
        return true;
    };
    bool zero = true;
    for (int k = 0; k < 12; ++k) zero = zero && transform[k] == 0.0f;
    if (zero || n == 0) return pass(rule::ST_NO_INPUT);
    if (n < 0 || n > nTo) return pass(rule::ST_BAD_INLIER);

    CpuBackend b;
    const bool local_from = cameraFrom.has_local_transform != 0, local_to = cameraTo.has_local_transform != 0;
    float inv_local_to[12];
    common::invert(local_from ? cameraFrom.local_transform : IDENTITY, b.f.M1);
    common::invert(local_to ? cameraTo.local_transform : IDENTITY, inv_local_to);
    b.f.v1 = rule::View{cameraFrom.fx, cameraFrom.fy, cameraFrom.cx, cameraFrom.cy, (float)p.baselineFrom};
    b.f.v2 = rule::View{cameraTo.fx, cameraTo.fy, cameraTo.cx, cameraTo.cy, (float)p.baselineTo};
    b.f.info = info; b.f.delta = delta; b.f.delta2 = delta * delta; b.f.two_delta = 2.0f * delta;
    b.f.inf_lin = priorVariance ? rule::prior_information(priorVariance[0], rule::LINEAR_EPSILON) : 1.0f;
    b.f.inf_ang = priorVariance ? rule::prior_information(priorVariance[1], rule::ANGULAR_EPSILON) : 1.0f;
    b.cx = cameraTo.cx; b.cy = cameraTo.cy; b.width = cameraTo.image_width; b.height = cameraTo.image_height;

    const std::map<int32_t, int> from = uniqueRows(fromIds, nFrom), to = uniqueRows(toIds, nTo);
    for (int i = 0; i < n; ++i) {
        const auto fi = from.find(inliers[i]), ti = to.find(inliers[i]);
        if (fi == from.end() || ti == to.end()) return pass(rule::ST_BAD_INLIER);
        const float* P = fromXyz + (size_t)fi->second * 3;
        if (!(common::finite(P[0]) && common::finite(P[1]) && common::finite(P[2]))) return pass(rule::ST_BAD_INLIER);
        rule::Point pt;
        float depth;
        pt.flags = 0;
        for (int a = 0; a < 3; ++a) { pt.p0[a] = P[a]; pt.p[a] = P[a]; pt.of[a] = 0.0f; }
        if (fromPoints) {
            pt.flags |= rule::F_FROM;
            if (rule::observe(b.f.M1, true, P[0], P[1], P[2], p.baselineFrom, cameraFrom.fx, fromPoints[(size_t)fi->second * 2], fromPoints[(size_t)fi->second * 2 + 1],
                              pt.of, depth))
                pt.flags |= rule::F_FROM_STEREO;
        }
        const float* T = toXyz ? toXyz + (size_t)ti->second * 3 : nullptr;
        if (rule::observe(inv_local_to, T != nullptr, T ? T[0] : 0.0f, T ? T[1] : 0.0f, T ? T[2] : 0.0f, p.baselineTo, cameraTo.fx, toPoints[(size_t)ti->second * 2],
                          toPoints[(size_t)ti->second * 2 + 1], pt.ot, depth))
            pt.flags |= rule::F_TO_STEREO;
        if (T && common::finite(T[0]) && common::finite(T[1]) && common::finite(T[2])) pt.flags |= rule::F_TO_FINITE;
        b.pts.push_back(pt);
        b.depth_to.push_back(depth);
        b.ids.push_back(inliers[i]);
    }
    b.saved.assign((size_t)n * 3, 0.0f);
    if (local_to) common::compose(transform, cameraTo.local_transform, b.C0);
    else
        for (int k = 0; k < 12; ++k) b.C0[k] = transform[k];
    float m0[12];
    common::invert(b.C0, m0);
    lcd::pnp::quat_of_model(m0, b.q);
    b.t[0] = m0[3]; b.t[1] = m0[7]; b.t[2] = m0[11];
    lcd::pnp::model_of_pose(b.q, b.t, b.cur);

    rule::Params prm;
    prm.min_inliers = p.minInliers; prm.iterations = p.iterations; prm.max_mean_distance = p.maxInliersMeanDistance; prm.min_distribution = p.minInliersDistribution;
    prm.distribution_valid = cameraTo.fx > 0.0f && cameraTo.fy > 0.0f && cameraTo.cx > 0.0f && cameraTo.cy > 0.0f && cameraTo.image_width > 0 && cameraTo.image_height > 0;
    prm.has_to_xyz = toXyz != nullptr; prm.has_local = local_to;
    rule::Result res;
    rule::solve(b, n, b.f, prm, transform, local_to ? cameraTo.local_transform : IDENTITY, res);
    for (int k = 0; k < 12; ++k) r.transform[k] = res.transform[k];
    r.status = res.status; r.nOutliers = res.n_outliers; r.lmAccepted = res.lm_accepted; r.chi2Before = res.chi2_before; r.chi2After = res.chi2_after;
    r.inliersMeanDistance = res.mean_distance; r.inliersDistribution = res.distribution;
    if (res.status == rule::ST_DIVERGED) r.inliers.assign(inliers, inliers + n);
    else
        for (int j = 0; j < res.n_inliers; ++j) r.inliers.push_back(b.ids[(size_t)b.kept[(size_t)j]]);
    out = r;
    return true;
}

Transform3D MotionBA::refine(lcd_engine* engine, const std::multimap<int, Point3f>& words3A, const std::multimap<int, Point2f>& kptsA,
                             const std::multimap<int, Point2f>& kptsB, const std::multimap<int, Point3f>& words3B, const lcd_camera& cameraFrom,
                             const lcd_camera& cameraTo, const Transform3D& transform, std::vector<int>& inliers, int varianceKind, double varianceLin,
                             double angleCos, const MotionBAParams& p, MotionBAInfo* info) {
    Transform3D refined;
    std::vector<int32_t> fromIds, toIds;
    std::vector<float> fromXyz, fromPoints, toPoints, toXyz;
    const float nan = std::nanf("");
    for (const auto& w : words3A) {
        fromIds.push_back(w.first);
        fromXyz.push_back(w.second.x); fromXyz.push_back(w.second.y); fromXyz.push_back(w.second.z);
        if (kptsA.empty()) continue;
        const auto range = kptsA.equal_range(w.first);
        const bool one = range.first != range.second && std::next(range.first) == range.second;
        fromPoints.push_back(one ? range.first->second.x : nan); fromPoints.push_back(one ? range.first->second.y : nan);
    }
    for (const auto& w : kptsB) {
        toIds.push_back(w.first);
        toPoints.push_back(w.second.x); toPoints.push_back(w.second.y);
        if (words3B.empty()) continue;
        const auto range = words3B.equal_range(w.first);
        const bool one = range.first != range.second && std::next(range.first) == range.second;
        toXyz.push_back(one ? range.first->second.x : nan); toXyz.push_back(one ? range.first->second.y : nan); toXyz.push_back(one ? range.first->second.z : nan);
    }
    const int64_t fromOffsets[2] = {0, (int64_t)fromIds.size()}, toOffsets[2] = {0, (int64_t)toIds.size()};
    const size_t region = std::max<size_t>(toIds.size(), 1);
    if (inliers.size() > toIds.size()) return refined;
    std::vector<int32_t> in(region, 0), survivors(region, 0);
    std::copy(inliers.begin(), inliers.end(), in.begin());
    const int32_t nIn = (int32_t)inliers.size();
    double covariance[36];
    motion_pnp_covariance(varianceKind, varianceLin, angleCos, covariance);
    const double prior[2] = {covariance[0], covariance[21]};
    const double baselines[2] = {p.baselineFrom, p.baselineTo};
    float t[12], mean = 0.0f, distribution = 0.0f;
    int32_t status = 0, nInliers = 0, nOutliers = 0, accepted = 0;
    double before = 0.0, after = 0.0;
    lcd_motion_ba_args a;
    a.struct_size = (int32_t)sizeof a; a.n_pairs = 1; a.min_inliers = p.minInliers; a.iterations = p.iterations; a.pixel_variance = p.pixelVariance;
    a.robust_delta = p.robustDelta; a.default_baseline = 0.0; a.max_inliers_mean_distance = p.maxInliersMeanDistance;
    a.min_inliers_distribution = p.minInliersDistribution;
    a.from_word_ids = fromIds.data(); a.from_xyz = fromXyz.data(); a.from_points = kptsA.empty() ? nullptr : fromPoints.data();
    a.to_word_ids = toIds.data(); a.to_points = toPoints.data(); a.to_xyz = words3B.empty() ? nullptr : toXyz.data();
    a.inliers = in.data(); a.n_inliers = &nIn; a.transforms = transform.data; a.prior_variance = varianceKind == 0 ? nullptr : prior;
    a.from_offsets = fromOffsets; a.to_offsets = toOffsets; a.cameras_from = &cameraFrom; a.cameras_to = &cameraTo; a.baselines = baselines;
    a.out_transform = t; a.out_status = &status; a.out_inliers = survivors.data(); a.out_n_inliers = &nInliers; a.out_n_outliers = &nOutliers;
    a.out_chi2_before = &before; a.out_chi2_after = &after; a.out_lm_accepted = &accepted; a.out_inliers_mean_distance = &mean;
    a.out_inliers_distribution = &distribution;
    if (!engine || lcd_refine_motion_ba(engine, &a) != LCD_OK) return refined;
    inliers.assign(survivors.begin(), survivors.begin() + nInliers);
    if (info) { info->status = status; info->inliersMeanDistance = mean; info->inliersDistribution = distribution; }
    for (int k = 0; k < 12; ++k) refined.data[k] = t[k];
    return refined;
}

}  // namespace rtabmap_amd
