// sanitize_epipolar.cpp -- epipolar_cpu (plain host code: the whole rule of lcd_verify_epipolar) driven from a stand-alone program, for a host-only
// AddressSanitizer / UndefinedBehaviorSanitizer run.  No engine is created and nothing touches a GPU.
//
//   g++ -std=c++17 -g -O1 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -Irtabmap_amd/host \
//       tools/sanitize_epipolar.cpp rtabmap_amd/host/EpipolarGeometryHip.cpp -o epipolar_asan
//   ./epipolar_asan
//
// Frames whose buffers end with their last row (a read past a frame is a heap overflow): 0 to 9 pairs, negative ids, ids that occur twice on
// one side or on both, ids of one side only, INT_MIN and INT_MAX ids, every keypoint at one position, collinear keypoints, NaN, infinite and
// huge coordinates, pairs that are all outliers, 1 / 85 / 86 / 300 iterations, 8192 rows, scenes times 2^-74 .. 2^+60, a hypothesis without seven
// distinct draws, every status, and the refused arguments.  Every result is checked against what the rule promises whatever the numbers are;
// exit status 0 and "ok" with the number of cases when all hold.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <set>
#include <vector>

#include "EpipolarGeometryHip.h"

// EpipolarGeometryHip.cpp's engine entry is linked but never called here
extern "C" int lcd_verify_epipolar(lcd_engine*, const lcd_epipolar_args*) { return 1; }

using rtabmap_amd::EpipolarParams;
using rtabmap_amd::EpipolarResult;
using rtabmap_amd::epipolar_cpu;

namespace {

struct Frame {
    std::vector<int32_t> ids;
    std::vector<float> uv;
    void add(int32_t id, float u, float v) { ids.push_back(id); uv.push_back(u); uv.push_back(v); }
    int n() const { return (int)ids.size(); }
};

int failures = 0, cases = 0;
bool seen[4] = {false, false, false, false};
void expect(bool ok, const char* what, int tag) {
    if (!ok) { std::printf("FAILED: %s (case %d)\n", what, tag); ++failures; }
}

// heap copies that end with the last element
bool run(const Frame& f, const Frame& t, const EpipolarParams& p, EpipolarResult& r) {
    std::vector<int32_t> fi(f.ids), ti(t.ids);
    std::vector<float> fp(f.uv), tp(t.uv);
    fi.shrink_to_fit(); ti.shrink_to_fit(); fp.shrink_to_fit(); tp.shrink_to_fit();
    return epipolar_cpu(fi.data(), fp.data(), f.n(), ti.data(), tp.data(), t.n(), p, r);
}

// unit_norm false: keypoints so small that the squares of the matrix' entries overflow, where the rule's division by the norm leaves zeros
void check(const Frame& f, const Frame& t, const EpipolarParams& p, int tag, bool unit_norm = true) {
    ++cases;
    EpipolarResult a, b;
    expect(run(f, t, p, a), "accepted", tag);
    expect(run(f, t, p, b), "accepted again", tag);
    expect(std::memcmp(a.fundamental, b.fundamental, sizeof a.fundamental) == 0 && a.status == b.status && a.matches == b.matches && a.inliers == b.inliers,
           "the same call gives the same bits", tag);
    expect(std::is_sorted(a.matches.begin(), a.matches.end()) && std::adjacent_find(a.matches.begin(), a.matches.end()) == a.matches.end(), "matches ascend", tag);
    expect(a.matches.empty() || a.matches.front() >= 0, "no negative id among the pairs", tag);
    expect(std::is_sorted(a.inliers.begin(), a.inliers.end()), "inliers in correspondence order", tag);
    const std::set<int> matches(a.matches.begin(), a.matches.end());
    bool sub = true;
    for (int id : a.inliers) sub = sub && matches.count(id) == 1;
    expect(sub, "inliers are pairs", tag);
    bool zero = true;
    for (float v : a.fundamental) zero = zero && v == 0.0f;
    expect(a.status >= 0 && a.status <= 3, "a status of the enum", tag);
    if (a.status >= 0 && a.status <= 3) seen[a.status] = true;
    const int m = (int)a.matches.size();
    expect((a.status == 1) == (m < p.matchCountMin || m < 8), "LCD_EPI_FEW_PAIRS iff m < match_count_min or m < 8", tag);
    if (a.status == 1 || a.status == 2) expect(a.inliers.empty() && zero, "no inliers and no matrix without a model", tag);
    if (a.status == 3) expect(!a.inliers.empty() && (int)a.inliers.size() < p.matchCountMin, "below match_count_min", tag);
    if (a.status == 0) expect((int)a.inliers.size() >= p.matchCountMin, "at least match_count_min", tag);
    if (a.status == 0 || a.status == 3) {
        double n2 = 0.0;
        for (float v : a.fundamental) n2 += (double)v * (double)v;
        expect(unit_norm ? std::fabs(n2 - 1.0) < 1e-3 : n2 == 0.0, unit_norm ? "a matrix of unit norm" : "a matrix of zeros", tag);
    }
}

// a scene under a small motion: m pairs, a fraction of them outliers, decoy ids around them
void scene(std::mt19937& rng, int m, double outliers, Frame& f, Frame& t) {
    std::uniform_real_distribution<float> U(0.0f, 1.0f);
    const float c = std::cos(0.15f), s = std::sin(0.15f), tx = 0.3f, ty = -0.05f, tz = 0.1f;
    for (int i = 0; i < m; ++i) {
        const float z = 1.0f + 7.0f * U(rng), u = 639.0f * U(rng), v = 479.0f * U(rng);
        const float X = (u - 319.5f) / 525.0f * z, Y = (v - 239.5f) / 525.0f * z;
        const float qx = c * X + s * z + tx, qy = Y + ty, qz = -s * X + c * z + tz;
        const bool out = U(rng) < outliers;
        f.add(i * 3, u, v);
        t.add(i * 3, out ? 639.0f * U(rng) : 525.0f * qx / qz + 319.5f, out ? 479.0f * U(rng) : 525.0f * qy / qz + 239.5f);
    }
    f.add(1 << 20, 1, 1); t.add(1 << 21, 5, 5);                            // one side only
    f.add(1 << 22, 1, 1); f.add(1 << 22, 2, 2); t.add(1 << 22, 5, 5);      // twice in from
    f.add(1 << 23, 1, 1); t.add(1 << 23, 5, 5); t.add(1 << 23, 6, 6);      // twice in to
    f.add(1 << 24, 1, 1); f.add(1 << 24, 2, 2); t.add(1 << 24, 5, 5); t.add(1 << 24, 6, 6);   // twice in both
    f.add(-5, 10, 10); t.add(-5, 20, 20);                                  // negative
}

}  // namespace

int main() {
    std::mt19937 rng(7);
    int tag = 0;
    EpipolarParams base;
    base.matchCountMin = 8; base.iterations = 60; base.ransacParam1 = 3.0; base.seed = 3;
    // 0 .. 9 pairs, three values of match_count_min
    for (int m = 0; m <= 9; ++m)
        for (int v = 0; v < 3; ++v) {
            Frame f, t;
            scene(rng, m, 0.0, f, t);
            EpipolarParams p = base;
            p.matchCountMin = 1 + v * 4;
            check(f, t, p, ++tag);
        }
    // iterations at the chunk edges of the device's scoring
    for (int it : {1, 85, 86, 300}) {
        Frame f, t;
        scene(rng, 120, 0.4, f, t);
        EpipolarParams p = base;
        p.iterations = it;
        check(f, t, p, ++tag);
    }
    {   // all outliers with a count that cannot be met; every keypoint at one position; collinear keypoints; empty frames
        Frame f, t;
        scene(rng, 60, 1.1, f, t);
        EpipolarParams p = base;
        p.matchCountMin = 40;
        check(f, t, p, ++tag);
        Frame e, et;
        for (int i = 0; i < 12; ++i) { e.add(i, 100, 100); et.add(i, 10.0f * i, 7.0f * i * i); }
        check(e, et, base, ++tag);
        Frame l, lt;
        for (int i = 0; i < 12; ++i) { l.add(i, 8.0f + 16.0f * i, 64); lt.add(i, 100.0f + 30.0f * i, 240.0f - 3.0f * i * i); }
        check(l, lt, base, ++tag);
        Frame none;
        check(none, lt, base, ++tag);
        check(l, none, base, ++tag);
        check(none, none, base, ++tag);
    }
    {   // NaN, infinite and huge coordinates; INT_MIN and INT_MAX ids
        const float bad[] = {NAN, INFINITY, -INFINITY, 3.0e38f, -3.0e38f, 1.0e19f, 1.0e-38f, 0.0f};
        for (float w : bad) {
            Frame f, t;
            scene(rng, 20, 0.2, f, t);
            f.uv[4] = w; t.uv[11] = w;
            f.add(INT_MIN, w, 1); t.add(INT_MIN, 10, w);
            f.add(INT_MAX, 1, w); t.add(INT_MAX, w, w);
            check(f, t, base, ++tag);
            Frame h, ht;                                                   // every coordinate the same bad value
            for (int i = 0; i < 9; ++i) { h.add(i, w, w); ht.add(i, w, w); }
            check(h, ht, base, ++tag);
        }
    }
    {   // 8192 rows a side
        Frame f, t;
        scene(rng, 8180, 0.3, f, t);
        f.ids.resize(8192); f.uv.resize(8192 * 2); t.ids.resize(8192); t.uv.resize(8192 * 2);
        EpipolarParams p = base;
        p.iterations = 10; p.matchCountMin = 20;
        check(f, t, p, ++tag);
    }
    // one scene times 2^k with the threshold scaled alike: squares that go subnormal (k <= -64), that vanish (-74) and that overflow (+60)
    for (int k : {-74, -70, -66, -64, -62, -20, 20, 55, 60}) {
        std::mt19937 same(11);
        Frame f, t;
        scene(same, 100, 0.4, f, t);
        for (float& w : f.uv) w = std::ldexp(w, k);
        for (float& w : t.uv) w = std::ldexp(w, k);
        EpipolarParams p = base;
        p.ransacParam1 = std::ldexp(3.0, k);
        check(f, t, p, ++tag, k > -62);
    }
    // one infinite coordinate among the pairs, either sign, either frame
    for (int side = 0; side < 2; ++side)
        for (float w : {INFINITY, -INFINITY}) {
            Frame f, t;
            scene(rng, 40, 0.0, f, t);
            (side ? t : f).uv[7] = w;
            check(f, t, base, ++tag);
        }
    {   // eight pairs: hypothesis 3 of seed 301 (seed + h = 304) does not find seven distinct indices in its 32 draws
        Frame f, t;
        scene(rng, 8, 0.0, f, t);
        EpipolarParams p = base;
        p.seed = 301;
        check(f, t, p, ++tag);
    }
    ++cases;
    expect(seen[0] && seen[1] && seen[2] && seen[3], "every status was met", ++tag);
    {   // refused arguments: the result stays untouched
        Frame f, t;
        scene(rng, 10, 0.0, f, t);
        EpipolarResult r;
        r.status = -7;
        auto refused = [&](EpipolarParams p, const char* what) {
            ++cases;
            expect(!run(f, t, p, r) && r.status == -7, what, ++tag);
        };
        EpipolarParams p = base;
        p.iterations = 0; refused(p, "iterations 0"); p = base;
        p.iterations = 65536; refused(p, "iterations 65536"); p = base;
        p.ransacParam1 = 0.0; refused(p, "ransac_threshold 0"); p = base;
        p.ransacParam1 = -1.0; refused(p, "ransac_threshold -1"); p = base;
        p.ransacParam1 = NAN; refused(p, "ransac_threshold NaN"); p = base;
        p.ransacParam1 = 1e-30; refused(p, "ransac_threshold whose square is 0 as a float"); p = base;
        p.ransacParam1 = 1e30; refused(p, "ransac_threshold whose square is not finite"); p = base;
        p.matchCountMin = 0; refused(p, "match_count_min 0");
        ++cases;
        expect(!epipolar_cpu(nullptr, f.uv.data(), 5, t.ids.data(), t.uv.data(), 5, base, r), "a null frame", ++tag);
        ++cases;
        expect(!epipolar_cpu(f.ids.data(), f.uv.data(), 5, t.ids.data(), nullptr, 5, base, r), "null keypoints", ++tag);
        ++cases;
        expect(!epipolar_cpu(f.ids.data(), f.uv.data(), 8193, t.ids.data(), t.uv.data(), 5, base, r), "8193 rows", ++tag);
    }
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("ok %d\n", cases);
    return 0;
}
