// RegistrationIcp.cpp -- see RegistrationIcp.h.
#include "RegistrationIcp.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <limits>

#include "../../include/lcd.h"
#include "../csrc/icp_plane_rule.h"

namespace rtabmap_amd {

namespace {

namespace rule = lcd::icp;
namespace plane = lcd::icpp;

// SUM over the rows 0 .. n - 1 that has(i) holds for: lane (i mod LANES) adds e(i) in ascending order from +0, a row without is skipped; then
// the halving tree
template <class H, class F>
float laneTreeSumIf(int n, H has, F e) {
    constexpr int LANES = lcd::m3d::LANES;
    float part[LANES];
    for (int l = 0; l < LANES; ++l) part[l] = 0.0f;
    for (int i = 0; i < n; ++i)
        if (has(i)) part[i % LANES] = part[i % LANES] + e(i);
    for (int s = LANES / 2; s >= 1; s >>= 1)
        for (int l = 0; l < s; ++l) part[l] = part[l] + part[l + s];
    return part[0];
}

struct Cloud {
    std::vector<float> xyz;                  // [n x 3]
    std::vector<char> part;                  // the rows that take part
    std::vector<int> nn;                     // the last search's nearest row in the other cloud, -1: none
    std::vector<float> d2;
    int n() const { return (int)part.size(); }
    const float* row(int i) const { return &xyz[(size_t)3 * i]; }
};

// step 2 for every row of q in c: brute force in the words of the rule, or -- where rule::wants_grid says so and every participating row of c
// fits the key's cell range -- over c's sorted cell keys, a row of q outside the range walking the whole cloud
void search(Cloud& q, const Cloud& c, int mode, float h) {
    const int rows = (int)std::count(c.part.begin(), c.part.end(), (char)1);
    bool grid = rule::wants_grid(mode, rows);
    std::vector<uint64_t> keys;
    for (int j = 0; grid && j < c.n(); ++j) {
        if (!c.part[(size_t)j]) continue;
        uint64_t k = 0;
        grid = rule::key_of(c.row(j)[0], c.row(j)[1], c.row(j)[2], h, (uint64_t)j, k);
        keys.push_back(k);
    }
    std::sort(keys.begin(), keys.end());
    for (int i = 0; i < q.n(); ++i) {
        float best = std::numeric_limits<float>::infinity();
        int row = -1;
        if (q.part[(size_t)i]) {
            const float* p = q.row(i);
            const bool found = grid && rule::grid_nearest([&](int a) { return keys[(size_t)a]; }, (int)keys.size(),
                                                          [&](int r, float& x, float& y, float& z) { x = c.row(r)[0]; y = c.row(r)[1]; z = c.row(r)[2]; },
                                                          p[0], p[1], p[2], h, best, row);
            for (int j = 0; !found && j < c.n(); ++j) {
                if (!c.part[(size_t)j]) continue;
                const float* t = c.row(j);
                const float d = rule::dist2(p[0], p[1], p[2], t[0], t[1], t[2]);
                if (rule::nearer(d, j, best, row)) { best = d; row = j; }
            }
        }
        q.nn[(size_t)i] = row; q.d2[(size_t)i] = best;
    }
}

// the backend of rule::solve as a loop
struct CpuBackend {
    Cloud from, to;                          // the source's current cloud, Q
    const float* raw_from;
    double thr2;
    int mode;                                // lcd_icp_search
    float h;                                 // the grid's cell
    std::vector<int> match;
    std::vector<uint32_t> keys;

    int count(const Cloud& c) const { return (int)std::count(c.part.begin(), c.part.end(), (char)1); }
    int n_from() const { return count(from); }
    int n_to() const { return count(to); }
    bool has(int i) const { return from.part[(size_t)i] && rule::corresponds(from.nn[(size_t)i], from.d2[(size_t)i], thr2); }
    int correspond(float& sum_d2) {
        search(from, to, mode, h);
        int c = 0;
        for (int i = 0; i < from.n(); ++i) c += has(i) ? 1 : 0;
        sum_d2 = laneTreeSumIf(from.n(), [&](int i) { return has(i); }, [&](int i) { return from.d2[(size_t)i]; });
        return c;
    }
    void fit(int c, bool flat, float T[12]) {
        const int n = from.n();
        auto h = [&](int i) { return has(i); };
        float cp[3], cq[3], S[9];
        for (int a = 0; a < 3; ++a) {
            const float sp = laneTreeSumIf(n, h, [&](int i) { return from.row(i)[a]; });
            const float sq = laneTreeSumIf(n, h, [&](int i) { return to.row(from.nn[(size_t)i])[a]; });
            cp[a] = sp / (float)c;
            cq[a] = sq / (float)c;
        }
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b)
                S[3 * a + b] = laneTreeSumIf(n, h, [&](int i) {
                    const float dp = from.row(i)[a] - cp[a], dq = to.row(from.nn[(size_t)i])[b] - cq[b];
                    return dp * dq;
                });
        rule::fit(cp, cq, S, flat, T);
    }
    void move(const float T[12], const float* src) {
        for (int i = 0; i < from.n(); ++i) {
            if (!from.part[(size_t)i]) continue;
            float x, y, z;
            rule::apply(T, src[(size_t)3 * i], src[(size_t)3 * i + 1], src[(size_t)3 * i + 2], x, y, z);
            from.xyz[(size_t)3 * i] = x; from.xyz[(size_t)3 * i + 1] = y; from.xyz[(size_t)3 * i + 2] = z;
        }
    }
    void advance(const float T[12]) { move(T, from.xyz.data()); }
    void set_registered(const float F[12]) { move(F, raw_from); }
    int reciprocal(bool from_is_target) {
        search(from, to, mode, h);
        search(to, from, mode, h);
        Cloud& src = from_is_target ? to : from;
        const Cloud& tgt = from_is_target ? from : to;
        keys.clear();
        for (int i = 0; i < src.n(); ++i) {
            const int row = src.nn[(size_t)i];
            if (!rule::corresponds(row, src.d2[(size_t)i], thr2) || tgt.nn[(size_t)row] != i) continue;
            keys.push_back(lcd::m3d::bits_of(src.d2[(size_t)i]));                  // non-negative: they order as integers
            if (from_is_target) match[(size_t)row] = i;
            else match[(size_t)i] = row;
        }
        return (int)keys.size();
    }
    float median(int n) {
        std::nth_element(keys.begin(), keys.begin() + (n >> 1), keys.end());
        return lcd::m3d::float_of(keys[(size_t)(n >> 1)]);
    }
};

// the backend of plane::solve as a loop: CpuBackend and the normals
struct CpuPlaneBackend : CpuBackend {
    std::vector<float> nrm_from, nrm_to;     // [n x 3]: the from-side's as given (behind register_normals: under F), the to-side's under the guess
    std::vector<char> nfin_from, nfin_to;    // the rows whose given normal is finite
    std::vector<char> cpart_from, cpart_to;  // the rows whose coordinates are finite
    const float* raw_nrm_from;
    std::vector<uint32_t> first;             // median_first()'s keys

    int rows_from() const { return (int)std::count(cpart_from.begin(), cpart_from.end(), (char)1); }
    int rows_to() const { return (int)std::count(cpart_to.begin(), cpart_to.end(), (char)1); }
    int normal_sums(bool to_side, float sum[3]) {
        const std::vector<float>& nrm = to_side ? nrm_to : nrm_from;
        const std::vector<char>& fin = to_side ? nfin_to : nfin_from;
        for (int a = 0; a < 3; ++a)
            sum[a] = laneTreeSumIf((int)fin.size(), [&](int i) { return fin[(size_t)i] != 0; }, [&](int i) { return nrm[(size_t)3 * i + a]; });
        return (int)std::count(fin.begin(), fin.end(), (char)1);
    }
    void normal_cov(bool to_side, const float mean[3], float C[6]) {
        const std::vector<float>& nrm = to_side ? nrm_to : nrm_from;
        const std::vector<char>& fin = to_side ? nfin_to : nfin_from;
        for (int k = 0; k < 6; ++k)
            C[k] = laneTreeSumIf((int)fin.size(), [&](int i) { return fin[(size_t)i] != 0; }, [&](int i) {
                float e[6];
                plane::cov_terms(&nrm[(size_t)3 * i], mean, e);
                return e[k];
            });
    }
    void participate(bool with_normals) {
        for (int i = 0; i < from.n(); ++i) from.part[(size_t)i] = cpart_from[(size_t)i] && (!with_normals || nfin_from[(size_t)i]) ? 1 : 0;
        for (int j = 0; j < to.n(); ++j) to.part[(size_t)j] = cpart_to[(size_t)j] && (!with_normals || nfin_to[(size_t)j]) ? 1 : 0;
    }
    bool fit_plane(float T[12]) {
        const int n = from.n();
        auto h = [&](int i) { return has(i); };
        float S[plane::SUMS];
        std::vector<float> E((size_t)n * plane::SUMS, 0.0f);
        for (int i = 0; i < n; ++i)
            if (has(i)) plane::plane_terms(from.row(i), to.row(from.nn[(size_t)i]), &nrm_to[(size_t)3 * from.nn[(size_t)i]], &E[(size_t)i * plane::SUMS]);
        for (int k = 0; k < plane::SUMS; ++k) S[k] = laneTreeSumIf(n, h, [&](int i) { return E[(size_t)i * plane::SUMS + k]; });
        for (int k = 0; k < 12; ++k) T[k] = 0.0f;
        return plane::plane_fit(S, T);
    }
    void register_normals(const float F[12]) {
        for (int i = 0; i < from.n(); ++i)
            plane::rotate(F, raw_nrm_from[3 * i], raw_nrm_from[3 * i + 1], raw_nrm_from[3 * i + 2], nrm_from[(size_t)3 * i], nrm_from[(size_t)3 * i + 1],
                          nrm_from[(size_t)3 * i + 2]);
    }
    int reciprocal_gated(bool from_is_target, bool gate, double min_cos) {
        search(from, to, mode, h);
        search(to, from, mode, h);
        Cloud& src = from_is_target ? to : from;
        const Cloud& tgt = from_is_target ? from : to;
        const std::vector<float>& nsrc = from_is_target ? nrm_to : nrm_from;
        const std::vector<float>& ntgt = from_is_target ? nrm_from : nrm_to;
        first.clear();
        int count = 0;
        for (int i = 0; i < src.n(); ++i) {
            const int row = src.nn[(size_t)i];
            if (!rule::corresponds(row, src.d2[(size_t)i], thr2) || tgt.nn[(size_t)row] != i) continue;
            first.push_back(lcd::m3d::bits_of(src.d2[(size_t)i]));
            if (gate && !plane::gate_passes(&ntgt[(size_t)3 * row], &nsrc[(size_t)3 * i], min_cos)) continue;
            ++count;
            if (from_is_target) match[(size_t)row] = i;
            else match[(size_t)i] = row;
        }
        first.resize((size_t)count);                                   // distances.resize(correspondencesOut), before the sort
        return count;
    }
    float median_first(int n) {
        std::nth_element(first.begin(), first.begin() + (n >> 1), first.end());
        return lcd::m3d::float_of(first[(size_t)(n >> 1)]);
    }
};

void fill(Cloud& c, const float* xyz, int n) {
    c.xyz.assign(xyz, xyz + (size_t)3 * n);
    c.part.resize((size_t)n); c.nn.assign((size_t)n, -1); c.d2.assign((size_t)n, 0.0f);
    for (int i = 0; i < n; ++i) c.part[(size_t)i] = rule::takes_part(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]) ? 1 : 0;
}

// What both mirrors do in front of their solve: the refusals of the parameters and arrays both have, then P_0, Q = guess(to-rows) and the
// search's parameters.  false: refused.
bool set_up(CpuBackend& b, const float* fromXyz, int nFrom, const float* toXyz, int nTo, const float guess[12], int maxIterations, int maxLaserScans,
            double maxCorrespondenceDistance, float epsilon, float correspondenceRatio, int search, bool deviceEntry) {
    const double thr2 = maxCorrespondenceDistance * maxCorrespondenceDistance;
    if (nFrom < 0 || nTo < 0 || nFrom > lcd::m3d::MAX_ROWS || nTo > lcd::m3d::MAX_ROWS || maxIterations < 1 || maxLaserScans < 0 ||
        (search != rule::SEARCH_AUTO && search != rule::SEARCH_BRUTE && search != rule::SEARCH_GRID) || !std::isfinite(maxCorrespondenceDistance) || !(maxCorrespondenceDistance > 0.0) ||
        !std::isfinite(thr2) || !std::isfinite(epsilon) || !(epsilon >= 0.0f) || !(correspondenceRatio >= 0.0f) || !(correspondenceRatio <= 1.0f) || !guess)
        return false;
    for (int k = 0; k < 12; ++k) if (!std::isfinite(guess[k])) return false;
    if ((nFrom > 0 && !fromXyz) || (nTo > 0 && !toXyz)) return false;
    fill(b.from, fromXyz, nFrom);
    fill(b.to, toXyz, nTo);
    if (!deviceEntry && (b.n_from() != nFrom || b.n_to() != nTo)) return false;
    for (int j = 0; j < nTo; ++j)
        rule::apply(guess, toXyz[3 * j], toXyz[3 * j + 1], toXyz[3 * j + 2], b.to.xyz[(size_t)3 * j], b.to.xyz[(size_t)3 * j + 1], b.to.xyz[(size_t)3 * j + 2]);
    b.raw_from = fromXyz; b.thr2 = thr2; b.mode = search; b.h = rule::cell_size(maxCorrespondenceDistance);
    b.match.assign((size_t)nFrom, -1);
    return true;
}

// the ten fields both results have, out of rule::Result or plane::Result
template <class R>
void common_result(const R& res, const CpuBackend& b, IcpResult& r) {
    for (int k = 0; k < 12; ++k) { r.transform[k] = res.transform[k]; r.icpTransform[k] = res.icp[k]; r.correction[k] = res.correction[k]; }
    r.status = res.status; r.stop = res.stop; r.iterations = res.iterations; r.correspondences = res.n_correspondences;
    r.ratio = res.ratio; r.variance = res.variance;
    r.match = b.match;
}

}  // namespace

float icp_cells(const float* x, int n, double maxCorrespondenceDistance, int* outCells) {
    const float h = rule::cell_size(maxCorrespondenceDistance);
    for (int i = 0; i < n; ++i)
        if (!rule::cell_of(x[i], h, outCells[i])) outCells[i] = std::numeric_limits<int>::min();
    return h;
}

bool register_icp_cpu(const float* fromXyz, int nFrom, const float* toXyz, int nTo, const float guess[12], int maxIterations, bool force3DoF,
                      int maxLaserScans, double maxCorrespondenceDistance, float epsilon, float correspondenceRatio, int search, bool deviceEntry,
                      IcpResult& out) {
    CpuBackend b;
    if (!set_up(b, fromXyz, nFrom, toXyz, nTo, guess, maxIterations, maxLaserScans, maxCorrespondenceDistance, epsilon, correspondenceRatio, search, deviceEntry)) return false;
    rule::Result res;
    rule::solve(b, maxIterations, force3DoF, maxLaserScans, epsilon, correspondenceRatio, guess, res);
    IcpResult r;
    common_result(res, b, r);
    out = r;
    return true;
}

bool register_icp_plane_cpu(const float* fromXyz, const float* fromNormals, int nFrom, const float* toXyz, const float* toNormals, int nTo,
                            const float guess[12], int maxIterations, bool force3DoF, int maxLaserScans, double maxCorrespondenceDistance, float epsilon,
                            float correspondenceRatio, float minComplexity, int lowComplexityStrategy, bool normalGate, double minNormalCos, int search,
                            bool deviceEntry, IcpPlaneResult& out) {
    if (!(minComplexity >= 0.0f) || !(minComplexity <= 1.0f) || lowComplexityStrategy < 0 || lowComplexityStrategy > 2 || (normalGate && !std::isfinite(minNormalCos)) ||
        (nFrom > 0 && !fromNormals) || (nTo > 0 && !toNormals))
        return false;
    CpuPlaneBackend b;
    if (!set_up(b, fromXyz, nFrom, toXyz, nTo, guess, maxIterations, maxLaserScans, maxCorrespondenceDistance, epsilon, correspondenceRatio, search, deviceEntry)) return false;
    b.cpart_from = b.from.part; b.cpart_to = b.to.part;
    b.nrm_from.assign(fromNormals, fromNormals + (size_t)3 * nFrom);
    b.nrm_to.resize((size_t)3 * nTo);
    b.nfin_from.resize((size_t)nFrom); b.nfin_to.resize((size_t)nTo);
    for (int i = 0; i < nFrom; ++i) b.nfin_from[(size_t)i] = plane::finite3(fromNormals[3 * i], fromNormals[3 * i + 1], fromNormals[3 * i + 2]) ? 1 : 0;
    for (int j = 0; j < nTo; ++j) {
        plane::rotate(guess, toNormals[3 * j], toNormals[3 * j + 1], toNormals[3 * j + 2], b.nrm_to[(size_t)3 * j], b.nrm_to[(size_t)3 * j + 1], b.nrm_to[(size_t)3 * j + 2]);
        b.nfin_to[(size_t)j] = plane::finite3(toNormals[3 * j], toNormals[3 * j + 1], toNormals[3 * j + 2]) ? 1 : 0;
    }
    b.raw_nrm_from = fromNormals;
    plane::Params p;
    p.max_iterations = maxIterations; p.max_laser_scans = maxLaserScans; p.strategy = lowComplexityStrategy; p.force_3dof = force3DoF; p.gate = normalGate;
    p.epsilon = epsilon; p.correspondence_ratio = correspondenceRatio; p.min_complexity = minComplexity; p.min_normal_cos = minNormalCos;
    plane::Result res;
    plane::solve(b, p, guess, res);
    IcpPlaneResult r;
    common_result(res, b, r);
    r.branch = res.branch; r.complexity = res.complexity; r.secondEigenvalue = res.second;
    for (int k = 0; k < 3; ++k) r.complexityValues[k] = res.values[k];
    for (int k = 0; k < 9; ++k) r.complexityVectors[k] = res.vectors[k];
    out = r;
    return true;
}

Transform3D RegistrationIcpHip::finish(const IcpResult& r, RegistrationInfoIcp& info) const {
    Transform3D transform;
    char msg[256];
    if (r.status == LCD_ICP_LOW_COMPLEXITY) {                          // :569-577
        snprintf(msg, sizeof msg, "Rejecting transform because too low complexity %f (Icp/PointToPlaneLowComplexityStrategy=0)", info.icpStructuralComplexity);
        info.rejectedMsg = msg;
        return transform;
    }
    if (r.status != LCD_ICP_OK && r.status != LCD_ICP_BELOW_RATIO) {   // :962: icpT is null or the loop did not converge
        snprintf(msg, sizeof msg, "Cannot compute transform (converged=false var=%f)", r.variance);
        info.rejectedMsg = msg;
        return transform;
    }
    // :858-862: pcl::getTranslationAndEulerAngles over the correction in the target's referential
    const float* c = r.correction;
    const float roll = std::atan2(c[9], c[10]), pitch = std::asin(-c[8]), yaw = std::atan2(c[4], c[0]);
    info.icpTranslation = std::max(std::fabs(c[3]), std::max(std::fabs(c[7]), std::fabs(c[11])));
    info.icpRotation = std::max(std::fabs(roll), std::max(std::fabs(pitch), std::fabs(yaw)));
    if ((maxTranslation > 0.0f && info.icpTranslation > maxTranslation) || (maxRotation > 0.0f && info.icpRotation > maxRotation)) {
        snprintf(msg, sizeof msg, "Cannot compute transform (ICP correction too large -> %f m %f rad, limits=%f m, %f rad)", info.icpTranslation,
                 info.icpRotation, maxTranslation, maxRotation);
        info.rejectedMsg = msg;
        return transform;
    }
    const double variance = r.variance / 10.0;                         // :898
    if (r.correspondences != 0) {                                      // :917-918
        for (int k = 0; k < 36; ++k) info.covariance[k] = 0.0;
        for (int k = 0; k < 3; ++k) { info.covariance[7 * k] = variance; info.covariance[7 * (k + 3)] = variance / 10.0; }
    }
    info.icpInliersRatio = r.ratio;
    info.icpCorrespondences = r.correspondences;
    if (r.status == LCD_ICP_BELOW_RATIO) {                             // :930
        snprintf(msg, sizeof msg, "Cannot compute transform (cor=%d corrRatio=%f/%f)", r.correspondences, r.ratio, correspondenceRatio);
        info.rejectedMsg = msg;
        return transform;
    }
    for (int k = 0; k < 12; ++k) transform.data[k] = r.transform[k];
    return transform;
}

Transform3D RegistrationIcpHip::computeTransformation(lcd_engine* engine, const std::vector<Point3f>& fromScan, const std::vector<Point3f>& toScan,
                                                      const Transform3D& guess, int maxLaserScans, RegistrationInfoIcp& info) const {
    info = RegistrationInfoIcp();
    if (fromScan.empty() || toScan.empty()) {                          // :972
        info.rejectedMsg = "Laser scans empty ?!?";
        return Transform3D();
    }
    static_assert(sizeof(Point3f) == 12, "a scan is handed over as [n x 3] floats");
    const int64_t fromOffsets[2] = {0, (int64_t)fromScan.size()}, toOffsets[2] = {0, (int64_t)toScan.size()};
    IcpResult r;
    r.match.assign(fromScan.size(), -1);
    int32_t status = 0, stop = 0, iterations = 0, correspondences = 0;
    lcd_icp_args a;
    a.struct_size = (int32_t)sizeof a; a.n_pairs = 1; a.max_iterations = maxIterations; a.force_3dof = force3DoF ? 1 : 0;
    a.max_laser_scans = maxLaserScans; a.search = LCD_ICP_SEARCH_AUTO;
    a.max_correspondence_distance = maxCorrespondenceDistance; a.epsilon = epsilon; a.correspondence_ratio = correspondenceRatio;
    a.from_xyz = &fromScan[0].x; a.to_xyz = &toScan[0].x; a.from_offsets = fromOffsets; a.to_offsets = toOffsets; a.guesses = guess.data;
    a.out_transform = r.transform; a.out_icp_transform = r.icpTransform; a.out_correction = r.correction;
    a.out_status = &status; a.out_stop = &stop; a.out_iterations = &iterations; a.out_n_correspondences = &correspondences;
    a.out_ratio = &r.ratio; a.out_variance = &r.variance; a.out_match = r.match.data();
    if (!engine || lcd_register_icp(engine, &a) != LCD_OK) {
        info.rejectedMsg = "the engine refused the call";
        return Transform3D();
    }
    r.status = status; r.stop = stop; r.iterations = iterations; r.correspondences = correspondences;
    return finish(r, info);
}

Transform3D RegistrationIcpHip::computeTransformation(lcd_engine* engine, const std::vector<Point3f>& fromScan, const std::vector<Point3f>& fromNormals,
                                                      bool fromIs2d, const std::vector<Point3f>& toScan, const std::vector<Point3f>& toNormals, bool toIs2d,
                                                      const Transform3D& guess, int maxLaserScans, RegistrationInfoIcp& info) const {
    // :510-524: point to plane is ignored for 2-D scans and needs normals on both sides
    if (!pointToPlane || fromIs2d || toIs2d || fromNormals.size() != fromScan.size() || toNormals.size() != toScan.size() || fromScan.empty() || toScan.empty())
        return computeTransformation(engine, fromScan, toScan, guess, maxLaserScans, info);
    info = RegistrationInfoIcp();
    const int64_t fromOffsets[2] = {0, (int64_t)fromScan.size()}, toOffsets[2] = {0, (int64_t)toScan.size()};
    IcpPlaneResult r;
    r.match.assign(fromScan.size(), -1);
    int32_t status = 0, stop = 0, iterations = 0, correspondences = 0, branch = 0;
    lcd_icp_plane_args a;
    a.struct_size = (int32_t)sizeof a; a.n_pairs = 1; a.max_iterations = maxIterations; a.force_3dof = force3DoF ? 1 : 0;
    a.max_laser_scans = maxLaserScans; a.search = LCD_ICP_SEARCH_AUTO;
    a.max_correspondence_distance = maxCorrespondenceDistance; a.epsilon = epsilon; a.correspondence_ratio = correspondenceRatio;
    a.min_complexity = pointToPlaneMinComplexity; a.low_complexity_strategy = pointToPlaneLowComplexityStrategy;
    a.normal_gate = maxRotation > 0.0f ? 1 : 0; a.reserved = 0;        // :268: maxCorrespondenceAngle <= 0 counts every correspondence
    a.min_normal_cos = std::cos((double)maxRotation);                  // angle < max  <=>  cosine > cos(max)
    a.from_xyz = &fromScan[0].x; a.to_xyz = &toScan[0].x; a.from_normals = &fromNormals[0].x; a.to_normals = &toNormals[0].x;
    a.from_offsets = fromOffsets; a.to_offsets = toOffsets; a.guesses = guess.data;
    a.out_transform = r.transform; a.out_icp_transform = r.icpTransform; a.out_correction = r.correction;
    a.out_status = &status; a.out_stop = &stop; a.out_iterations = &iterations; a.out_n_correspondences = &correspondences;
    a.out_ratio = &r.ratio; a.out_variance = &r.variance; a.out_match = r.match.data();
    a.out_branch = &branch; a.out_complexity = &r.complexity; a.out_complexity_values = r.complexityValues; a.out_complexity_vectors = r.complexityVectors;
    a.out_second_eigenvalue = &r.secondEigenvalue;
    if (!engine || lcd_register_icp_plane(engine, &a) != LCD_OK) {
        info.rejectedMsg = "the engine refused the call";
        return Transform3D();
    }
    r.status = status; r.stop = stop; r.iterations = iterations; r.correspondences = correspondences; r.branch = branch;
    info.icpStructuralComplexity = r.complexity;                       // :531
    return finish(r, info);
}

Transform3D RegistrationIcpHip::computeTransformation(lcd_engine* engine, const std::vector<Point3f>& fromScan, bool fromIs2d, int fromMaxPoints,
                                                      const std::vector<Point3f>& toScan, bool toIs2d, int toMaxPoints, const Transform3D& guess,
                                                      RegistrationInfoIcp& info, FilteredScans* filtered) const {
    info = RegistrationInfoIcp();
    FilteredScans fs;
    fs.fromScan = fromScan; fs.toScan = toScan;
    int maxFrom = fromMaxPoints > 0 ? fromMaxPoints : (int)fromScan.size(), maxTo = toMaxPoints > 0 ? toMaxPoints : (int)toScan.size();   // :363-364
    struct Side { const std::vector<Point3f>* raw; std::vector<Point3f>* xyz; std::vector<Point3f>* normals; bool is2d; int* maxScans; };
    std::vector<Side> sides;
    if (!fromScan.empty() && (filtersEnabled & 1)) sides.push_back(Side{&fromScan, &fs.fromScan, &fs.fromNormals, fromIs2d, &maxFrom});
    if (!toScan.empty() && (filtersEnabled & 2)) sides.push_back(Side{&toScan, &fs.toScan, &fs.toNormals, toIs2d, &maxTo});
    // one call for the sides that agree on 2-D, which is every pair but a mixed one
    for (size_t first = 0; first < sides.size();) {
        size_t last = first + 1;
        while (last < sides.size() && sides[last].is2d == sides[first].is2d) ++last;
        const int ns = (int)(last - first);
        const bool normals = pointToPlane && !sides[first].is2d && (pointToPlaneK > 0 || pointToPlaneRadius > 0.0f);
        std::vector<float> xyz;
        std::vector<int64_t> offsets(1, 0), outOffsets(1, 0);
        for (size_t s = first; s < last; ++s) {
            const std::vector<Point3f>& raw = *sides[s].raw;
            xyz.insert(xyz.end(), &raw[0].x, &raw[0].x + raw.size() * 3);
            offsets.push_back(offsets.back() + (int64_t)raw.size());
            outOffsets.push_back(outOffsets.back() + (int64_t)raw.size());                 // a scan never grows
        }
        std::vector<float> outXyz((size_t)outOffsets.back() * 3), outNormals(normals ? outXyz.size() : 0);
        int32_t count[2] = {0, 0}, stages[6], status[2] = {0, 0};
        lcd_scan_filter_args a;
        a.struct_size = (int32_t)sizeof a; a.n_scans = ns; a.downsampling_step = downsamplingStep; a.is_2d = sides[first].is2d ? 1 : 0;
        a.normal_k = normals ? pointToPlaneK : 0; a.reserved = 0; a.range_min = rangeMin; a.range_max = rangeMax; a.voxel_size = voxelSize;
        a.normal_radius = normals ? pointToPlaneRadius : 0.0f; a.ground_normals_up = normals ? pointToPlaneGroundNormalsUp : 0.0f;
        a.viewpoint[0] = a.viewpoint[1] = a.viewpoint[2] = 0.0f;
        a.xyz = xyz.data(); a.offsets = offsets.data(); a.out_offsets = outOffsets.data(); a.out_xyz = outXyz.data();
        a.out_normals = normals ? outNormals.data() : nullptr; a.out_count = count; a.out_stage_counts = stages; a.out_status = status;
        if (!engine || lcd_filter_scans(engine, &a) != LCD_OK) {
            info.rejectedMsg = "the engine refused the call";
            return Transform3D();
        }
        for (size_t s = first; s < last; ++s) {
            const size_t k = s - first, n = (size_t)count[k];
            const Point3f* px = reinterpret_cast<const Point3f*>(outXyz.data()) + outOffsets[k];
            sides[s].xyz->assign(px, px + n);
            if (normals) {
                const Point3f* pn = reinterpret_cast<const Point3f*>(outNormals.data()) + outOffsets[k];
                sides[s].normals->assign(pn, pn + n);
            }
            const float ratio = float(n) / float(sides[s].raw->size());                  // :404-405
            *sides[s].maxScans = int(float(*sides[s].maxScans) * ratio);
        }
        first = last;
    }
    fs.maxLaserScans = maxTo ? maxTo : maxFrom;                            // :879
    const Transform3D t = computeTransformation(engine, fs.fromScan, fs.fromNormals, fromIs2d, fs.toScan, fs.toNormals, toIs2d, guess, fs.maxLaserScans, info);
    if (filtered) *filtered = fs;
    return t;
}

}  // namespace rtabmap_amd
