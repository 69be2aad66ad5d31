// sanitize_motion_3d.cpp -- motion3d_cpu (plain host code: the whole rule of lcd_estimate_motion_3d) driven from a stand-alone program, for a
// host-only AddressSanitizer / UndefinedBehaviorSanitizer run.  No engine is created and nothing touches a GPU.
//
//   g++ -std=c++17 -g -O1 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -Irtabmap_amd/host \
//       tools/sanitize_motion_3d.cpp rtabmap_amd/host/Motion3D.cpp -o motion_3d_asan
//   ./motion_3d_asan
//
// Frames whose buffers end with their last row (a read past a frame is a heap overflow): no rows, 2 and 3 correspondences, ids that occur
// twice on one side, ids of one side only, the extreme ids, NaN, infinite and zero points, pairs that are all outliers, exact pairs whose
// hypotheses all tie, a seed whose first hypothesis finds no three distinct indices, coordinates whose sums overflow to NaN models, every
// combination of 1 / 255 / 256 / 257 iterations with 0 / 1 / 5 refinement passes, 8192 rows, and the refused arguments.  Every result is
// checked against what the rule promises whatever the numbers are; exit status 0 and "ok" when all hold.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <set>
#include <vector>

#include "Motion3D.h"

// Motion3D.cpp's engine entry is linked but never called here
struct lcd_motion_3d_args;
extern "C" int lcd_estimate_motion_3d(lcd_engine*, const lcd_motion_3d_args*) { return 1; }

using rtabmap_amd::Motion3DResult;
using rtabmap_amd::motion3d_cpu;

namespace {

struct Frame {
    std::vector<int32_t> ids;
    std::vector<float> xyz;
    void add(int32_t id, float x, float y, float z) { ids.push_back(id); xyz.push_back(x); xyz.push_back(y); xyz.push_back(z); }
    int n() const { return (int)ids.size(); }
};

int failures = 0;
void expect(bool ok, const char* what, int tag) {
    if (!ok) { std::printf("FAILED: %s (case %d)\n", what, tag); ++failures; }
}

// heap copies that end with the last element
bool run(const Frame& f, const Frame& t, int minInliers, double dist, int iterations, int refine, uint32_t seed, Motion3DResult& r) {
    std::vector<int32_t> fi(f.ids), ti(t.ids);
    std::vector<float> fx(f.xyz), tx(t.xyz);
    fi.shrink_to_fit(); ti.shrink_to_fit(); fx.shrink_to_fit(); tx.shrink_to_fit();
    return motion3d_cpu(fi.data(), fx.data(), f.n(), ti.data(), tx.data(), t.n(), minInliers, dist, iterations, refine, seed, r);
}

void check(const Frame& f, const Frame& t, int minInliers, double dist, int iterations, int refine, uint32_t seed, int tag) {
    Motion3DResult a, b;
    expect(run(f, t, minInliers, dist, iterations, refine, seed, a), "accepted", tag);
    expect(run(f, t, minInliers, dist, iterations, refine, seed, b), "accepted again", tag);
    expect(std::memcmp(a.transform, b.transform, sizeof a.transform) == 0 && a.status == b.status && a.matches == b.matches && a.inliers == b.inliers &&
           std::memcmp(&a.variance, &b.variance, 8) == 0, "the same call gives the same bits", tag);
    expect(std::is_sorted(a.matches.begin(), a.matches.end()) && std::adjacent_find(a.matches.begin(), a.matches.end()) == a.matches.end(), "matches ascend", tag);
    for (int id : a.matches) {
        expect(std::count(f.ids.begin(), f.ids.end(), id) == 1 && std::count(t.ids.begin(), t.ids.end(), id) == 1, "a match is unique on both sides", tag);
    }
    size_t at = 0;                                                      // the inliers are a subsequence of the matches
    for (int id : a.inliers) {
        while (at < a.matches.size() && a.matches[at] != id) ++at;
        expect(at < a.matches.size(), "inliers in correspondence order", tag);
        ++at;
    }
    bool zero = true, finite = true;
    for (float v : a.transform) { zero = zero && v == 0.0f; finite = finite && std::isfinite(v); }
    const int m = (int)a.matches.size(), n = (int)a.inliers.size();
    expect(a.status >= 0 && a.status <= 4, "a status of the enum", tag);
    expect((a.status == 0) == !zero || (a.status == 0 && !finite), "a transform with LCD_M3D_OK and only then", tag);
    if (a.status == 1) expect(m < minInliers || m < 3, "few correspondences", tag);
    if (a.status != 1) expect(m >= minInliers && m >= 3, "enough correspondences", tag);
    if (a.status >= 1 && a.status <= 3) expect(n == 0 && a.variance == 1.0, "no inliers and variance 1 without a model", tag);
    if (a.status == 0) expect(n >= minInliers && n >= 3, "inliers >= min_inliers", tag);
    if (a.status == 4) expect(n >= 3 && n < minInliers, "3 <= inliers < min_inliers", tag);
    if (a.status == 0 || a.status == 4) expect(a.variance >= 0.0 && !std::isnan(a.variance), "a variance", tag);
}

Frame moved(const Frame& f, std::mt19937& rng, double outliers, float noise) {
    std::normal_distribution<float> g(0.0f, noise);
    std::uniform_real_distribution<float> u(-3.0f, 3.0f), p(0.0f, 1.0f);
    Frame t;
    for (int i = 0; i < f.n(); ++i) {
        const float x = f.xyz[3 * i], y = f.xyz[3 * i + 1], z = f.xyz[3 * i + 2];
        if (p(rng) < outliers) t.add(f.ids[i], u(rng), u(rng), u(rng));
        else t.add(f.ids[i], -y + 0.5f + g(rng), x - 0.25f + g(rng), z + 1.0f + g(rng));          // a quarter turn about z and a shift
    }
    return t;
}

Frame cloud(int n, std::mt19937& rng, int firstId) {
    std::uniform_real_distribution<float> u(-3.0f, 3.0f);
    Frame f;
    for (int i = 0; i < n; ++i) f.add(firstId + 3 * i, u(rng), u(rng), u(rng));
    return f;
}

void shuffle(Frame& f, std::mt19937& rng) {
    for (int i = f.n() - 1; i > 0; --i) {
        const int j = (int)(rng() % (uint32_t)(i + 1));
        std::swap(f.ids[i], f.ids[j]);
        for (int k = 0; k < 3; ++k) std::swap(f.xyz[3 * i + k], f.xyz[3 * j + k]);
    }
}

}  // namespace

int main() {
    std::mt19937 rng(7);
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    const int32_t lo = std::numeric_limits<int32_t>::min(), hi = std::numeric_limits<int32_t>::max();
    int tag = 0;
    const int iters[] = {1, 255, 256, 257}, refines[] = {0, 1, 5};

    // sizes around nothing, the guards, a wave and a workgroup; decoys of every kind
    for (int m : {0, 1, 2, 3, 5, 6, 63, 64, 65, 255, 256, 257, 600}) {
        Frame f = cloud(m, rng, -40);
        Frame t = moved(f, rng, 0.4, 0.01f);
        f.add(lo, 1, 2, 3); t.add(lo, -2 + 0.5f, 1 - 0.25f, 4);          // the extreme ids take part
        f.add(hi, 1, 1, 1); t.add(hi, -1 + 0.5f, 1 - 0.25f, 2);
        f.add(1000000, 1, 1, 1); f.add(1000000, 2, 2, 2); t.add(1000000, 1, 1, 1);      // twice in from
        f.add(1000001, 1, 1, 1); t.add(1000001, 1, 1, 1); t.add(1000001, 2, 2, 2);      // twice in to
        f.add(1000002, 1, 1, 1); t.add(1000003, 1, 1, 1);                                // one side only
        f.add(1000004, nan, 1, 1); t.add(1000004, 1, 1, 1);
        f.add(1000005, 1, 1, 1); t.add(1000005, 1, -inf, 1);
        f.add(1000006, 0, 0, 0); t.add(1000006, 1, 1, 1);
        f.add(1000007, 1, 1, 1); t.add(1000007, 0, -0.0f, 0);
        shuffle(f, rng); shuffle(t, rng);
        for (int it : iters)
            for (int rf : refines) check(f, t, 4, 0.1, it, rf, (uint32_t)(it + rf), ++tag);
        Motion3DResult r;
        run(f, t, 1, 0.1, 10, 0, 0, r);
        expect((int)r.matches.size() == m + 2, "the decoys take no part, the extreme ids do", tag);
    }
    // empty sides
    {
        Frame none, some = cloud(10, rng, 1);
        check(none, none, 1, 0.1, 5, 5, 0, ++tag);
        check(none, some, 1, 0.1, 5, 5, 0, ++tag);
        check(some, none, 1, 0.1, 5, 5, 0, ++tag);
    }
    // all outliers; thresholds tiny and huge
    {
        Frame f = cloud(40, rng, 1), t = moved(f, rng, 1.1, 0.0f);
        for (double d : {1e-30, 1e-3, 0.1, 10.0, 1e30}) for (int rf : refines) check(f, t, 10, d, 300, rf, 3, ++tag);
    }
    // exact pairs: every hypothesis ties; a seed whose hypothesis 0 is invalid among three correspondences
    {
        Frame f;
        for (int i = 0; i < 12; ++i) f.add(i + 1, (float)(i % 5 - 2), (float)(i % 3 + 1), (float)(i / 4 - 1));
        for (int rf : refines) check(f, f, 3, 0.1, 50, rf, 9, ++tag);
        Frame three;
        three.add(1, 1, 0, 0); three.add(2, 0, 2, 0); three.add(3, 0, 0, 3);
        Motion3DResult r;
        expect(run(three, three, 3, 0.1, 1, 0, 555, r) && r.status == 2, "seed 555: hypothesis 0 finds no three distinct indices among three", ++tag);
        expect(run(three, three, 3, 0.1, 2, 0, 555, r) && r.status == 0 && r.inliers.size() == 3, "... hypothesis 1 does", tag);
        for (uint32_t seed = 0; seed < 2000; ++seed) check(three, three, 3, 0.1, 3, 1, seed, ++tag);
    }
    // coordinates at the edge of fp32: sums that overflow, models of NaNs
    for (float scale : {1.0e15f, 4.4e18f, 1.0e19f, 3.0e38f}) {
        std::uniform_real_distribution<float> u(0.5f, 1.0f);
        Frame f, t;
        for (int i = 0; i < 64; ++i) {
            const float x = (rng() & 1 ? -1.0f : 1.0f) * u(rng) * scale, y = (rng() & 1 ? -1.0f : 1.0f) * u(rng) * scale, z = (rng() & 1 ? -1.0f : 1.0f) * u(rng) * scale;
            f.add(i + 1, x, y, z); t.add(i + 1, -y, x, z);
        }
        for (double d : {0.1, 1.0e15, 1.0e300}) for (int rf : refines) check(f, t, 3, d, 20, rf, 1, ++tag);
    }
    // denormal coordinates
    {
        Frame f = cloud(30, rng, 1);
        for (float& v : f.xyz) v *= 1.0e-42f;
        check(f, f, 3, 0.1, 30, 5, 1, ++tag);
        check(f, moved(f, rng, 0.3, 1.0e-44f), 3, 1.0e-40, 30, 5, 1, ++tag);
    }
    // the largest frames
    {
        Frame f = cloud(8192, rng, -5000), t = moved(f, rng, 0.3, 0.01f);
        shuffle(t, rng);
        check(f, t, 20, 0.1, 8, 5, 2, ++tag);
    }
    // refused arguments leave the result alone
    {
        Frame f = cloud(5, rng, 1);
        Motion3DResult r;
        r.status = -9;
        expect(!run(f, f, 0, 0.1, 10, 0, 0, r) && !run(f, f, 3, 0.1, 0, 0, 0, r) && !run(f, f, 3, 0.1, 65536, 0, 0, r) && !run(f, f, 3, 0.1, 10, -1, 0, r) &&
               !run(f, f, 3, 0.0, 10, 0, 0, r) && !run(f, f, 3, -1.0, 10, 0, 0, r) && !run(f, f, 3, (double)nan, 10, 0, 0, r) && !run(f, f, 3, (double)inf, 10, 0, 0, r),
               "refused", ++tag);
        expect(!run(cloud(8193, rng, 1), f, 3, 0.1, 10, 0, 0, r) && !run(f, cloud(8193, rng, 1), 3, 0.1, 10, 0, 0, r) && r.status == -9, "more than 8192 rows", tag);
        expect(!motion3d_cpu(nullptr, f.xyz.data(), 5, f.ids.data(), f.xyz.data(), 5, 3, 0.1, 10, 0, 0, r), "a null frame", tag);
    }
    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("ok: %d cases\n", tag);
    return 0;
}
