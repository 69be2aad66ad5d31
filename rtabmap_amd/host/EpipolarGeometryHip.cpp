// EpipolarGeometryHip.cpp -- see EpipolarGeometryHip.h.
#include "EpipolarGeometryHip.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "../csrc/epipolar_rule.h"
#include "LaneSum.h"
#include "MotionMirror.h"

namespace rtabmap_amd {

namespace rule = lcd::epi;
namespace common = lcd::m3d;

bool epipolar_cpu(const int32_t* fromIds, const float* fromPoints, int nFrom, const int32_t* toIds, const float* toPoints, int nTo,
                  const EpipolarParams& p, EpipolarResult& out) {
    const float thr = (float)p.ransacParam1;
    const float thr2 = thr * thr;
    if (nFrom < 0 || nTo < 0 || nFrom > common::MAX_ROWS || nTo > common::MAX_ROWS || p.matchCountMin < 1 || p.iterations < 1 || p.iterations > 65535 ||
        !std::isfinite(p.ransacParam1) || !(thr > 0.0f) || !std::isfinite(thr) || !(thr2 > 0.0f) || !std::isfinite(thr2))
        return false;
    if ((nFrom > 0 && (!fromIds || !fromPoints)) || (nTo > 0 && (!toIds || !toPoints))) return false;
    const std::map<int32_t, int> from = uniqueRows(fromIds, nFrom), to = uniqueRows(toIds, nTo);
    EpipolarResult r;
    for (int k = 0; k < 9; ++k) r.fundamental[k] = 0.0f;
    std::vector<float> coords[4];
    for (const auto& t : to) {                                         // EpipolarGeometry.h:158-186
        if (t.first < 0) continue;
        const auto f = from.find(t.first);
        if (f == from.end()) continue;
        r.matches.push_back(t.first);
        coords[0].push_back(fromPoints[(size_t)f->second * 2]);
        coords[1].push_back(fromPoints[(size_t)f->second * 2 + 1]);
        coords[2].push_back(toPoints[(size_t)t.second * 2]);
        coords[3].push_back(toPoints[(size_t)t.second * 2 + 1]);
    }
    const int m = (int)r.matches.size();
    r.status = rule::ST_FEW_PAIRS;
    if (m >= p.matchCountMin && m >= rule::MIN_PAIRS) {
        auto at = [&](int plane, int i) { return coords[plane][(size_t)i]; };
        float sums[4];
        for (int c = 0; c < 4; ++c) sums[c] = laneTreeSum<common::LANES>(m, [&](int i) { return at(c, i); });
        float cfx, cfy, ctx, cty;
        rule::centroid(sums[0], sums[1], m, cfx, cfy);
        rule::centroid(sums[2], sums[3], m, ctx, cty);
        const float df = laneTreeSum<common::LANES>(m, [&](int i) { return rule::distance(at(0, i), at(1, i), cfx, cfy); });
        const float dt = laneTreeSum<common::LANES>(m, [&](int i) { return rule::distance(at(2, i), at(3, i), ctx, cty); });
        rule::Norm nf, nt;
        const bool okf = rule::normalisation(cfx, cfy, df, m, nf), okt = rule::normalisation(ctx, cty, dt, m, nt);
        r.status = rule::ST_NO_MODEL;
        if (okf && okt) {
            float cur[12];
            const uint64_t best = bestCandidate(3 * p.iterations, m, cur,
                [&](int c, float* model) { return rule::candidate(p.seed, (uint32_t)c, m, nf, nt, at, model); },
                [&](const float* model, int i) { return rule::is_inlier(model, at(0, i), at(1, i), at(2, i), at(3, i), thr2); });
            if (best) {
                for (int i = 0; i < m; ++i)
                    if (rule::is_inlier(cur, at(0, i), at(1, i), at(2, i), at(3, i), thr2)) r.inliers.push_back(r.matches[(size_t)i]);
                rule::unit_matrix(cur, r.fundamental);
                r.status = (int)r.inliers.size() >= p.matchCountMin ? rule::ST_OK : rule::ST_FEW_INLIERS;
            }
        }
    }
    out = r;
    return true;
}

EpipolarGeometryHip::EpipolarGeometryHip(const ParametersMap& parameters) : _matchCountMin(8), _ransacParam1(3.0), _ransacParam2(0.99) {
    this->parseParameters(parameters);       // Parameters.h: VhEp/MatchCountMin 8, VhEp/RansacParam1 3, VhEp/RansacParam2 0.99
}

void EpipolarGeometryHip::parseParameters(const ParametersMap& parameters) {
    ParametersMap::const_iterator it;
    if ((it = parameters.find("VhEp/MatchCountMin")) != parameters.end()) _matchCountMin = atoi(it->second.c_str());
    if ((it = parameters.find("VhEp/RansacParam1")) != parameters.end()) _ransacParam1 = (double)uStr2Float(it->second);
    if ((it = parameters.find("VhEp/RansacParam2")) != parameters.end()) _ransacParam2 = (double)uStr2Float(it->second);
}

bool EpipolarGeometryHip::findFFromWords(lcd_engine* engine, const std::vector<int>& wordIdsA, const std::vector<float>& pointsA,
                                         const std::vector<int>& wordIdsB, const std::vector<float>& pointsB, float fundamental[9],
                                         std::vector<unsigned char>& status, std::vector<int>* pairsOut, int* engineStatus, uint32_t seed) const {
    for (int k = 0; k < 9; ++k) fundamental[k] = 0.0f;
    status.clear();
    if (pairsOut) pairsOut->clear();
    if (engineStatus) *engineStatus = LCD_EPI_FEW_PAIRS;
    if (!engine || pointsA.size() != wordIdsA.size() * 2 || pointsB.size() != wordIdsB.size() * 2) return false;
    const int64_t fromOffsets[2] = {0, (int64_t)wordIdsA.size()}, toOffsets[2] = {0, (int64_t)wordIdsB.size()};
    const size_t region = std::max<size_t>(wordIdsB.size(), 1);
    std::vector<int32_t> matches(region), inliers(region);
    int32_t st = 0, nPairs = 0, nInliers = 0;
    lcd_epipolar_args a;
    a.struct_size = (int32_t)sizeof a; a.n_pairs = 1; a.match_count_min = _matchCountMin; a.iterations = 1000; a.seed = seed;
    a.ransac_threshold = _ransacParam1;
    a.from_word_ids = wordIdsA.data(); a.from_points = pointsA.data(); a.to_word_ids = wordIdsB.data(); a.to_points = pointsB.data();
    a.from_offsets = fromOffsets; a.to_offsets = toOffsets;
    a.out_fundamental = fundamental; a.out_status = &st; a.out_n_pairs = &nPairs; a.out_n_inliers = &nInliers;
    a.out_matches = matches.data(); a.out_inliers = inliers.data();
    if (lcd_verify_epipolar(engine, &a) != LCD_OK) return false;
    if (engineStatus) *engineStatus = st;
    if (pairsOut) pairsOut->assign(matches.begin(), matches.begin() + nPairs);
    status.assign((size_t)nPairs, 0);
    for (int i = 0, j = 0; i < nPairs && j < nInliers; ++i)           // both lists ascend
        if (matches[(size_t)i] == inliers[(size_t)j]) { status[(size_t)i] = 1; ++j; }
    return true;
}

bool EpipolarGeometryHip::check(lcd_engine* engine, const std::vector<int>& wordIdsA, const std::vector<float>& pointsA, const std::vector<int>& wordIdsB,
                                const std::vector<float>& pointsB, uint32_t seed) const {
    float f[9];
    std::vector<unsigned char> status;
    int st = LCD_EPI_FEW_PAIRS;
    if (!this->findFFromWords(engine, wordIdsA, pointsA, wordIdsB, pointsB, f, status, nullptr, &st, seed)) return false;
    return st == LCD_EPI_OK;
}

}  // namespace rtabmap_amd
