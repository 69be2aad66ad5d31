// sanitize_motion_mono.cpp -- motion_mono_cpu (plain host code: the whole rule of lcd_estimate_motion_mono) driven from a stand-alone program,
// for a host-only AddressSanitizer / UndefinedBehaviorSanitizer run.  No engine is created and nothing touches a GPU.
//
//   g++ -std=c++17 -g -O1 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -Irtabmap_amd/host \
//       tools/sanitize_motion_mono.cpp rtabmap_amd/host/MotionMono.cpp -o motion_mono_asan
//   ./motion_mono_asan
//
// Frames whose buffers end with their last row (a read past a frame is a heap overflow): 0 to 12 pairs, negative ids, ids that occur twice,
// ids of one side only, INT_MIN and INT_MAX ids, every keypoint at one position, the same keypoints in both frames, NaN, infinite and huge
// coordinates, pairs that are all outliers, 1 / 31 / 32 / 33 iterations, 8192 rows, cameras times 2^-60 .. 2^+60, with and without words3, a
// guess and a local transform, words3 of NaN, infinity and zeros, every shift of the median's rank, and the refused arguments.  Every result
// is checked against what the rule promises whatever the numbers are; exit status 0 and "ok" with the number of cases when all hold.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <set>
#include <vector>

#include "MotionMono.h"

// MotionMono.cpp's engine entry is linked but never called here
extern "C" int lcd_estimate_motion_mono(lcd_engine*, const lcd_motion_mono_args*) { return 1; }

using rtabmap_amd::MotionMonoParams;
using rtabmap_amd::MotionMonoResult;
using rtabmap_amd::motion_mono_cpu;

namespace {

struct Frame {
    std::vector<int32_t> ids;
    std::vector<float> uv, xyz;
    void add(int32_t id, float u, float v, float x = 1.0f, float y = 1.0f, float z = 1.0f) {
        ids.push_back(id); uv.push_back(u); uv.push_back(v); xyz.push_back(x); xyz.push_back(y); xyz.push_back(z);
    }
    int n() const { return (int)ids.size(); }
};

int failures = 0, cases = 0;
bool seen[6] = {false, false, false, false, false, false};
void expect(bool ok, const char* what, int tag) {
    if (!ok) { std::printf("FAILED: %s (case %d)\n", what, tag); ++failures; }
}

// heap copies that end with the last element
bool run(const Frame& f, const Frame& t, bool with3, const MotionMonoParams& p, MotionMonoResult& r) {
    std::vector<int32_t> fi(f.ids), ti(t.ids);
    std::vector<float> fp(f.uv), tp(t.uv), f3(f.xyz);
    fi.shrink_to_fit(); ti.shrink_to_fit(); fp.shrink_to_fit(); tp.shrink_to_fit(); f3.shrink_to_fit();
    return motion_mono_cpu(fi.data(), fp.data(), with3 ? f3.data() : nullptr, f.n(), ti.data(), tp.data(), t.n(), p, r);
}

void check(const Frame& f, const Frame& t, bool with3, const MotionMonoParams& p, int tag) {
    ++cases;
    MotionMonoResult a, b;
    expect(run(f, t, with3, p, a), "accepted", tag);
    expect(run(f, t, with3, p, b), "accepted again", tag);
    expect(std::memcmp(a.transform, b.transform, sizeof a.transform) == 0 && a.status == b.status && a.matches == b.matches && a.inliers == b.inliers &&
               std::memcmp(&a.variance, &b.variance, 8) == 0 && a.points3.size() == b.points3.size() &&
               (a.points3.empty() || std::memcmp(a.points3.data(), b.points3.data(), a.points3.size() * 4) == 0),
           "the same bits twice", tag);
    expect(a.status >= 0 && a.status <= 5, "a status of the enum", tag);
    if (a.status >= 0 && a.status <= 5) seen[a.status] = true;
    expect(std::is_sorted(a.matches.begin(), a.matches.end()) && std::adjacent_find(a.matches.begin(), a.matches.end()) == a.matches.end(), "matches ascend", tag);
    expect(std::is_sorted(a.inliers.begin(), a.inliers.end()), "inliers ascend", tag);
    expect(std::includes(a.matches.begin(), a.matches.end(), a.inliers.begin(), a.inliers.end()), "inliers are matches", tag);
    expect(a.points3.size() == a.inliers.size() * 3, "one point per inlier", tag);
    for (int id : a.matches) expect(id >= 0, "no negative id is paired", tag);
    bool zero = true;
    for (float v : a.transform) zero = zero && v == 0.0f;
    expect((a.status == 0) == !zero || (a.status == 0 && zero), "a transform for LCD_MONO_OK only", tag);
    if (a.status != 0) expect(zero, "twelve zeros without LCD_MONO_OK", tag);
    if (a.status == 1) expect(a.matches.empty(), "no join below min_inliers rows", tag);
    if (a.status <= 3 && a.status >= 1) expect(a.inliers.empty() && a.variance == 1.0, "nothing estimated", tag);
    if (a.status == 2) expect(a.matches.size() < 9, "FEW_PAIRS below nine", tag);
    if (a.status == 4) expect((int)a.inliers.size() < p.minInliers, "FEW_INLIERS below min_inliers", tag);
    if (a.status == 0) expect((int)a.inliers.size() >= p.minInliers && a.variance <= (double)p.maxVariance, "OK passes both gates", tag);
    if (a.status == 5) expect(!(a.variance <= (double)p.maxVariance), "HIGH_VARIANCE above max_variance", tag);
}

// a rigid scene seen twice: x2 ~ R x1 + t, f = 525
void scene(std::mt19937& rng, int m, double outliers, double noise, bool rotate_only, Frame& f, Frame& t, float fscale = 1.0f) {
    std::uniform_real_distribution<double> U(0.0, 1.0);
    std::normal_distribution<double> N(0.0, 1.0);
    const double a = 0.2 * (U(rng) - 0.5), b = 0.2 * (U(rng) - 0.5);
    const double R[9] = {std::cos(a), 0, std::sin(a), std::sin(a) * std::sin(b), std::cos(b), -std::cos(a) * std::sin(b), -std::sin(a) * std::cos(b), std::sin(b), std::cos(a) * std::cos(b)};
    const double T[3] = {rotate_only ? 0.0 : 0.4 * (U(rng) - 0.5), rotate_only ? 0.0 : 0.4 * (U(rng) - 0.5), rotate_only ? 0.0 : 0.4 * (U(rng) - 0.5)};
    const double fl = 525.0 * fscale;
    for (int i = 0; i < m; ++i) {
        const double z = 1.0 + 7.0 * U(rng), x = (U(rng) - 0.5) * z, y = (U(rng) - 0.5) * 0.8 * z;
        const double X = R[0] * x + R[1] * y + R[2] * z + T[0], Y = R[3] * x + R[4] * y + R[5] * z + T[1], Z = R[6] * x + R[7] * y + R[8] * z + T[2];
        f.add(100 + 3 * i, (float)(fl * x / z + 319.5 + noise * N(rng)), (float)(fl * y / z + 239.5 + noise * N(rng)), (float)x, (float)y, (float)z);
        if (U(rng) < outliers) t.add(100 + 3 * i, (float)(640 * U(rng)), (float)(480 * U(rng)));
        else t.add(100 + 3 * i, (float)(fl * X / Z + 319.5 + noise * N(rng)), (float)(fl * Y / Z + 239.5 + noise * N(rng)));
    }
}

MotionMonoParams params(int minInliers = 8, int iterations = 40, float fscale = 1.0f) {
    MotionMonoParams p;
    p.minInliers = minInliers; p.iterations = iterations; p.seed = 11; p.maxVariance = 100.0f;
    p.fx = 525.0f * fscale; p.fy = 525.0f * fscale; p.cx = 319.5f; p.cy = 239.5f;
    return p;
}

}  // namespace

int main() {
    std::mt19937 rng(5);
    int tag = 0;
    // 0 to 12 pairs, with and without words3
    for (int m = 0; m <= 12; ++m)
        for (int with3 = 0; with3 < 2; ++with3) {
            Frame f, t;
            scene(rng, m, 0.0, 0.0, false, f, t);
            for (int k = 0; k < 9; ++k) { f.add(9000 + k, 5.0f * k, 7.0f * k); t.add(9500 + k, 3.0f * k, 2.0f * k); }   // rows without a partner
            check(f, t, with3 != 0, params(), ++tag);
        }
    {
        Frame f, t, none;
        scene(rng, 7, 0.0, 0.0, false, f, t);
        check(f, t, true, params(), ++tag);                            // fewer rows than min_inliers
        check(none, none, false, params(), ++tag);
    }
    // ids: negative, twice on a side, extreme
    {
        Frame f, t;
        scene(rng, 40, 0.2, 0.3, false, f, t);
        f.add(-3, 10, 10); t.add(-3, 11, 11); f.add(INT_MIN, 1, 2); t.add(INT_MIN, 2, 1); f.add(INT_MAX, 20, 30); t.add(INT_MAX, 22, 33);
        f.add(100, 50, 50); t.add(103, 60, 60); f.add(0, 300, 200); t.add(0, 310, 205);
        check(f, t, true, params(), ++tag);
    }
    // degenerate keypoints
    {
        Frame f, t;
        for (int i = 0; i < 30; ++i) { f.add(i, 100, 100); t.add(i, 100, 100); }
        check(f, t, true, params(), ++tag);
        Frame g, u;
        scene(rng, 30, 0.0, 0.0, false, g, u);
        check(g, g, true, params(), ++tag);                            // the same keypoints in both frames
        Frame r1, r2;
        scene(rng, 30, 0.0, 0.0, true, r1, r2);
        check(r1, r2, true, params(), ++tag);                          // a pure rotation
    }
    for (float bad : {NAN, INFINITY, -INFINITY, 3e38f, -3e38f, 1e-40f}) {
        Frame f, t;
        scene(rng, 30, 0.1, 0.2, false, f, t);
        f.uv[6] = bad; t.uv[21] = bad; f.xyz[9] = bad;
        check(f, t, true, params(), ++tag);
        for (size_t i = 0; i < f.xyz.size(); ++i) f.xyz[i] = bad;
        check(f, t, true, params(), ++tag);
    }
    {
        Frame f, t;
        scene(rng, 30, 0.0, 0.0, false, f, t);
        std::fill(f.xyz.begin(), f.xyz.end(), 0.0f);
        check(f, t, true, params(), ++tag);
        Frame g, u;
        scene(rng, 40, 1.0, 0.0, false, g, u);                         // all outliers
        check(g, u, true, params(20), ++tag);
    }
    // iterations around the kernel's chunk; the gates; the shift
    for (int it : {1, 31, 32, 33}) {
        Frame f, t;
        scene(rng, 50, 0.3, 0.5, false, f, t);
        check(f, t, false, params(8, it), ++tag);
    }
    for (int ratio : {0, 1, 4, 6, 31})
        for (int guess = 0; guess < 2; ++guess) {
            Frame f, t;
            scene(rng, 50, 0.2, 0.3, false, f, t);
            MotionMonoParams p = params();
            p.varianceMedianRatio = ratio;
            p.hasGuess = guess != 0;
            const float g[12] = {1, 0, 0, 0.2f, 0, 1, 0, 0.1f, 0, 0, 1, -0.3f};
            std::copy(g, g + 12, p.guess);
            const float l[12] = {0, 0, 1, 0.1f, -1, 0, 0, 0, 0, -1, 0, 0.3f};
            p.hasLocalTransform = ratio == 4;
            std::copy(l, l + 12, p.localTransform);
            check(f, t, true, p, ++tag);
            p.maxVariance = 0.0f; check(f, t, true, p, ++tag);
            p.minInliers = 49; check(f, t, true, p, ++tag);
        }
    {
        MotionMonoParams p = params();
        p.hasGuess = true;                                             // twelve zeros, then a NaN: null
        Frame f, t;
        scene(rng, 30, 0.0, 0.1, false, f, t);
        check(f, t, true, p, ++tag);
        p.guess[5] = NAN;
        check(f, t, true, p, ++tag);
    }
    for (int k : {-60, -20, 20, 60}) {
        Frame f, t;
        const float s = std::ldexp(1.0f, k);
        scene(rng, 40, 0.2, 0.3, false, f, t, s);
        check(f, t, true, params(8, 40, s), ++tag);
    }
    {
        Frame f, t;
        scene(rng, 8192, 0.3, 0.3, false, f, t);
        check(f, t, false, params(8, 3), ++tag);
        Frame g, u;
        scene(rng, 600, 0.3, 0.3, false, g, u);
        check(g, u, true, params(8, 3), ++tag);
    }
    // the refused arguments
    {
        Frame f, t;
        scene(rng, 20, 0.0, 0.0, false, f, t);
        MotionMonoResult r;
        r.status = 77;
        const MotionMonoParams ok = params();
        auto refused = [&](MotionMonoParams p, const char* what) { ++cases; expect(!run(f, t, true, p, r) && r.status == 77, what, ++tag); };
        MotionMonoParams p = ok; p.iterations = 0; refused(p, "iterations 0");
        p = ok; p.iterations = 65536; refused(p, "iterations 65536");
        p = ok; p.minInliers = 0; refused(p, "min_inliers 0");
        p = ok; p.reprojThreshold = 0.0; refused(p, "threshold 0");
        p = ok; p.reprojThreshold = NAN; refused(p, "threshold NaN");
        p = ok; p.reprojThreshold = 1e-30; refused(p, "threshold whose square vanishes");
        p = ok; p.distanceThreshold = -1.0; refused(p, "distance -1");
        p = ok; p.varianceMedianRatio = 32; refused(p, "shift 32");
        p = ok; p.varianceMedianRatio = -1; refused(p, "shift -1");
        p = ok; p.maxVariance = NAN; refused(p, "max_variance NaN");
        p = ok; p.fx = 0.0f; refused(p, "fx 0");
        p = ok; p.cy = INFINITY; refused(p, "cy infinite");
        ++cases; expect(!motion_mono_cpu(nullptr, nullptr, nullptr, 3, t.ids.data(), t.uv.data(), t.n(), ok, r), "null from-arrays", ++tag);
        ++cases; expect(!motion_mono_cpu(f.ids.data(), f.uv.data(), nullptr, 8193, t.ids.data(), t.uv.data(), t.n(), ok, r), "8193 rows", ++tag);
    }
    for (int s = 0; s < 6; ++s) expect(seen[s], "every status is met", 1000 + s);
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("ok %d\n", cases);
    return 0;
}
