// MotionMono.cpp -- see MotionMono.h.
#include "MotionMono.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "../csrc/motion_mono_rule.h"
#include "MotionMirror.h"

namespace rtabmap_amd {

namespace rule = lcd::mono;
namespace common = lcd::m3d;

namespace {

struct PlainWs {
    double* p;
    double& operator()(int e) const { return p[e]; }
};

}  // namespace

bool motion_mono_cpu(const int32_t* fromIds, const float* fromPoints, const float* fromPoints3, int nFrom, const int32_t* toIds, const float* toPoints,
                     int nTo, const MotionMonoParams& p, MotionMonoResult& out) {
    if (nFrom < 0 || nTo < 0 || nFrom > common::MAX_ROWS || nTo > common::MAX_ROWS || p.minInliers < 1 || p.iterations < 1 || p.iterations > 65535 ||
        !std::isfinite(p.reprojThreshold) || !(p.reprojThreshold > 0.0) || !std::isfinite(p.distanceThreshold) || !(p.distanceThreshold > 0.0) ||
        p.varianceMedianRatio < 0 || p.varianceMedianRatio > 31 || !(p.maxVariance >= 0.0f) || !std::isfinite(p.maxVariance) || !std::isfinite(p.fx) ||
        !std::isfinite(p.fy) || p.fx == 0.0f || p.fy == 0.0f || !std::isfinite(p.cx) || !std::isfinite(p.cy))
        return false;
    const float thr2 = rule::threshold2(p.reprojThreshold, p.fx, p.fy);
    if (!(thr2 > 0.0f) || !std::isfinite(thr2)) return false;
    if ((nFrom > 0 && (!fromIds || !fromPoints)) || (nTo > 0 && (!toIds || !toPoints))) return false;
    const float identity[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    const float* local = p.hasLocalTransform ? p.localTransform : identity;
    MotionMonoResult r;
    for (int k = 0; k < 12; ++k) r.transform[k] = 0.0f;
    r.status = rule::ST_FEW_FEATURES;
    r.variance = 1.0;
    if (nFrom >= p.minInliers && nTo >= p.minInliers) {                // RegistrationVis.cpp:1594
        const std::map<int32_t, int> from = uniqueRows(fromIds, nFrom), to = uniqueRows(toIds, nTo);
        std::vector<float> coords[7];
        for (const auto& t : to) {
            if (t.first < 0) continue;
            const auto f = from.find(t.first);
            if (f == from.end()) continue;
            r.matches.push_back(t.first);
            coords[0].push_back(rule::normalised(fromPoints[(size_t)f->second * 2], p.cx, p.fx));
            coords[1].push_back(rule::normalised(fromPoints[(size_t)f->second * 2 + 1], p.cy, p.fy));
            coords[2].push_back(rule::normalised(toPoints[(size_t)t.second * 2], p.cx, p.fx));
            coords[3].push_back(rule::normalised(toPoints[(size_t)t.second * 2 + 1], p.cy, p.fy));
            for (int c = 0; c < 3; ++c) coords[4 + c].push_back(fromPoints3 ? fromPoints3[(size_t)f->second * 3 + c] : 0.0f);
        }
        const int m = (int)r.matches.size();
        r.status = rule::ST_FEW_PAIRS;
        if (m >= rule::MIN_PAIRS) {
            auto at = [&](int plane, int i) { return coords[plane][(size_t)i]; };
            double space[rule::WS];
            PlainWs ws{space};
            auto solve = [&](uint32_t h) {
                int idx[5];
                if (!rule::draw5(p.seed, h, (uint32_t)m, idx)) return 0;
                float x1[5], y1[5], x2[5], y2[5];
                for (int j = 0; j < 5; ++j) { x1[j] = at(0, idx[j]); y1[j] = at(1, idx[j]); x2[j] = at(2, idx[j]); y2[j] = at(3, idx[j]); }
                return rule::solve(ws, x1, y1, x2, y2);
            };
            auto inlier = [&](const float* e, int i) { return rule::is_inlier(e, at(0, i), at(1, i), at(2, i), at(3, i), thr2); };
            uint64_t best = 0;
            for (int h = 0; h < p.iterations; ++h) {
                const int n = solve((uint32_t)h);
                for (int c = 0; c < n; ++c) {
                    double E[9];
                    if (!rule::model(ws, c, E)) continue;
                    float e[9];
                    for (int k = 0; k < 9; ++k) e[k] = (float)E[k];
                    uint32_t count = 0;
                    for (int i = 0; i < m; ++i) count += inlier(e, i) ? 1u : 0u;
                    const uint64_t key = ((uint64_t)count << 32) | (uint32_t)~(uint32_t)(h * rule::ROOTS + c);
                    if (count > 0 && key > best) best = key;
                }
            }
            r.status = rule::ST_NO_MODEL;
            double E[9], P[21];
            bool have = best != 0;
            if (have) {
                const uint32_t c = ~(uint32_t)best, h = c / (uint32_t)rule::ROOTS;
                (void)solve(h);
                (void)rule::model(ws, (int)(c - h * (uint32_t)rule::ROOTS), E);
                have = rule::decompose(E, P);
            }
            if (have) {
                float e[9];
                for (int k = 0; k < 9; ++k) e[k] = (float)E[k];
                int cnt[4] = {0, 0, 0, 0};
                for (int i = 0; i < m; ++i) {
                    if (!inlier(e, i)) continue;
                    for (int k = 0; k < 4; ++k) {
                        double d1;
                        if (rule::config_test(P, k, at(0, i), at(1, i), at(2, i), at(3, i), p.distanceThreshold, d1)) ++cnt[k];
                    }
                }
                const int cfg = rule::choose_config(cnt[0], cnt[1], cnt[2], cnt[3]);
                std::vector<int> rows;
                for (int i = 0; i < m; ++i) {
                    double d1;
                    if (!inlier(e, i) || !rule::config_test(P, cfg, at(0, i), at(1, i), at(2, i), at(3, i), p.distanceThreshold, d1)) continue;
                    float q[3];
                    rule::point_of(d1, at(0, i), at(1, i), local, q);
                    rows.push_back(i);
                    r.inliers.push_back(r.matches[(size_t)i]);
                    r.points3.insert(r.points3.end(), q, q + 3);
                }
                float T[12];
                rule::camera_transform(P, cfg, local, T);
                // the scale and the variance (util3d_features.cpp:304-408)
                const bool hasGuess = p.hasGuess && !rule::guess_is_null(p.guess);
                float scale = 1.0f, variance = 1.0f;
                if (hasGuess) scale = rule::norm3(p.guess[3], p.guess[7], p.guess[11]) / rule::norm3(T[3], T[7], T[11]);
                if (fromPoints3) {
                    std::vector<int> usable;
                    auto guessOf = [&](int j, float g[3]) { for (int c = 0; c < 3; ++c) g[c] = at(4 + c, rows[(size_t)j]); };
                    for (int j = 0; j < (int)rows.size(); ++j) {
                        float g[3];
                        guessOf(j, g);
                        if (rule::usable(&r.points3[(size_t)j * 3], g)) usable.push_back(j);
                    }
                    const int n = (int)usable.size();
                    if (n > 0) {
                        const int rank = rule::median_rank(n, p.varianceMedianRatio);
                        const int rounds = hasGuess ? 1 : n;
                        std::vector<uint32_t> keys((size_t)n);
                        for (int c = 0; c < rounds; ++c) {
                            float s = scale;
                            if (!hasGuess) s = at(4, rows[(size_t)usable[(size_t)c]]) / r.points3[(size_t)usable[(size_t)c] * 3];
                            for (int q = 0; q < n; ++q) {
                                float g[3];
                                guessOf(usable[(size_t)q], g);
                                keys[(size_t)q] = rule::order_key(rule::scaled_error(&r.points3[(size_t)usable[(size_t)q] * 3], g, s));
                            }
                            std::vector<uint32_t> sorted(keys);
                            std::nth_element(sorted.begin(), sorted.begin() + rank, sorted.end());
                            const float var = rule::variance_of(rule::key_value(sorted[(size_t)rank]));
                            if (hasGuess || c == 0 || var < variance) { variance = var; scale = s; }
                        }
                    }
                }
                if (scale != 1.0f) {
                    T[3] = T[3] * scale; T[7] = T[7] * scale; T[11] = T[11] * scale;
                    for (size_t j = 0; j < rows.size(); ++j) {
                        float* q = &r.points3[j * 3];
                        if (common::finite(q[0]) && common::finite(q[1]) && common::finite(q[2])) { q[0] = q[0] * scale; q[1] = q[1] * scale; q[2] = q[2] * scale; }
                    }
                }
                r.variance = (double)variance;
                r.status = (int)rows.size() < p.minInliers ? rule::ST_FEW_INLIERS
                                                           : ((double)variance <= (double)p.maxVariance ? rule::ST_OK : rule::ST_HIGH_VARIANCE);
                if (r.status == rule::ST_OK) for (int k = 0; k < 12; ++k) r.transform[k] = T[k];
            }
        }
    }
    out = r;
    return true;
}

MotionMonoHip::MotionMonoHip(const ParametersMap& parameters) : _minInliers(20), _reprojThreshold(2.0), _varianceMedianRatio(4), _maxVariance(0.1f) {
    this->parseParameters(parameters);       // Parameters.h: Vis/MinInliers 20, Vis/PnPReprojError 2, Vis/PnPVarianceMedianRatio 4, Vis/EpipolarGeometryVar 0.1
}

void MotionMonoHip::parseParameters(const ParametersMap& parameters) {
    ParametersMap::const_iterator it;
    if ((it = parameters.find("Vis/MinInliers")) != parameters.end()) _minInliers = atoi(it->second.c_str());
    if ((it = parameters.find("Vis/PnPReprojError")) != parameters.end()) _reprojThreshold = (double)uStr2Float(it->second);
    if ((it = parameters.find("Vis/PnPVarianceMedianRatio")) != parameters.end()) _varianceMedianRatio = atoi(it->second.c_str());
    if ((it = parameters.find("Vis/EpipolarGeometryVar")) != parameters.end()) _maxVariance = uStr2Float(it->second);
}

bool MotionMonoHip::estimate(lcd_engine* engine, const std::vector<int>& wordIdsA, const std::vector<float>& pointsA, const std::vector<float>& points3A,
                             const std::vector<int>& wordIdsB, const std::vector<float>& pointsB, const lcd_camera& camera, const float* guess,
                             MotionMonoResult& out, uint32_t seed) const {
    if (!engine || pointsA.size() != wordIdsA.size() * 2 || pointsB.size() != wordIdsB.size() * 2 || (!points3A.empty() && points3A.size() != wordIdsA.size() * 3))
        return false;
    const int64_t fromOffsets[2] = {0, (int64_t)wordIdsA.size()}, toOffsets[2] = {0, (int64_t)wordIdsB.size()};
    const size_t region = std::max<size_t>(wordIdsB.size(), 1);
    std::vector<int32_t> matches(region), inliers(region);
    std::vector<float> points3(region * 3);
    MotionMonoResult r;
    int32_t st = 0, nMatches = 0, nInliers = 0;
    lcd_motion_mono_args a;
    a.struct_size = (int32_t)sizeof a; a.n_pairs = 1; a.min_inliers = _minInliers; a.iterations = 1000; a.seed = seed;
    a.variance_median_ratio = _varianceMedianRatio; a.reproj_threshold = _reprojThreshold; a.distance_threshold = 50.0; a.max_variance = _maxVariance;
    a.reserved = 0;
    a.from_word_ids = wordIdsA.data(); a.from_points = pointsA.data(); a.from_points3 = points3A.empty() ? nullptr : points3A.data();
    a.to_word_ids = wordIdsB.data(); a.to_points = pointsB.data();
    a.from_offsets = fromOffsets; a.to_offsets = toOffsets; a.cameras = &camera; a.guesses = guess;
    a.out_transform = r.transform; a.out_status = &st; a.out_n_matches = &nMatches; a.out_n_inliers = &nInliers; a.out_variance = &r.variance;
    a.out_matches = matches.data(); a.out_inliers = inliers.data(); a.out_points3 = points3.data();
    if (lcd_estimate_motion_mono(engine, &a) != LCD_OK) return false;
    r.status = st;
    r.matches.assign(matches.begin(), matches.begin() + nMatches);
    r.inliers.assign(inliers.begin(), inliers.begin() + nInliers);
    r.points3.assign(points3.begin(), points3.begin() + (size_t)nInliers * 3);
    out = r;
    return true;
}

}  // namespace rtabmap_amd
