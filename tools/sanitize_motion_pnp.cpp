// sanitize_motion_pnp.cpp -- motion_pnp_cpu (plain host code: the whole rule of lcd_estimate_motion_pnp) driven from a stand-alone program, for a
// host-only AddressSanitizer / UndefinedBehaviorSanitizer run.  No engine is created and nothing touches a GPU.
//
//   g++ -std=c++17 -g -O1 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -Irtabmap_amd/host \
//       tools/sanitize_motion_pnp.cpp rtabmap_amd/host/Motion2D.cpp -o motion_pnp_asan
//   ./motion_pnp_asan
//
// Frames whose buffers end with their last row (a read past a frame is a heap overflow): 0 to 6 correspondences, ids that occur twice on one
// side, ids of one side only, INT_MIN and INT_MAX ids, collinear and coincident triples, every point behind the camera, NaN, infinite and huge
// coordinates in points and keypoints, pairs that are all outliers, with and without to_xyz, an image size, a local transform and a guess,
// every combination of 1 / 255 / 256 / 257 iterations with 0 / 1 / 5 refinement passes, 8192 rows, and the refused arguments.  Every result
// is checked against what the rule promises whatever the numbers are; exit status 0 and "ok" with the number of cases when all hold.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <set>
#include <vector>

#include "Motion2D.h"

// Motion2D.cpp's engine entry is linked but never called here
extern "C" int lcd_estimate_motion_pnp(lcd_engine*, const lcd_motion_pnp_args*) { return 1; }

using rtabmap_amd::MotionPnpParams;
using rtabmap_amd::MotionPnpResult;
using rtabmap_amd::motion_pnp_cpu;

namespace {

struct From {
    std::vector<int32_t> ids;
    std::vector<float> xyz;
    void add(int32_t id, float x, float y, float z) { ids.push_back(id); xyz.push_back(x); xyz.push_back(y); xyz.push_back(z); }
    int n() const { return (int)ids.size(); }
};
struct To {
    std::vector<int32_t> ids;
    std::vector<float> uv, xyz;
    void add(int32_t id, float u, float v, float x, float y, float z) {
        ids.push_back(id); uv.push_back(u); uv.push_back(v); xyz.push_back(x); xyz.push_back(y); xyz.push_back(z);
    }
    int n() const { return (int)ids.size(); }
};

int failures = 0, cases = 0;
void expect(bool ok, const char* what, int tag) {
    if (!ok) { std::printf("FAILED: %s (case %d)\n", what, tag); ++failures; }
}

lcd_camera camera(bool sized, bool local) {
    lcd_camera c = {};
    c.fx = 525.0f; c.fy = 525.0f; c.cx = 319.5f; c.cy = 239.5f;
    if (sized) { c.image_width = 640; c.image_height = 480; }
    if (local) {
        const float t[12] = {0, 0, 1, 0.1f, -1, 0, 0, 0.02f, 0, -1, 0, 0.3f};
        c.has_local_transform = 1;
        std::copy(t, t + 12, c.local_transform);
    }
    return c;
}

// heap copies that end with the last element
bool run(const From& f, const To& t, bool toXyz, const lcd_camera& cam, const float* guess, const MotionPnpParams& p, MotionPnpResult& r) {
    std::vector<int32_t> fi(f.ids), ti(t.ids);
    std::vector<float> fx(f.xyz), tp(t.uv), tx(t.xyz);
    fi.shrink_to_fit(); ti.shrink_to_fit(); fx.shrink_to_fit(); tp.shrink_to_fit(); tx.shrink_to_fit();
    std::vector<float> g;
    if (guess) g.assign(guess, guess + 12);
    return motion_pnp_cpu(fi.data(), fx.data(), f.n(), ti.data(), tp.data(), toXyz ? tx.data() : nullptr, t.n(), cam, guess ? g.data() : nullptr, p, r);
}

void check(const From& f, const To& t, bool toXyz, const lcd_camera& cam, const float* guess, const MotionPnpParams& p, int tag) {
    ++cases;
    MotionPnpResult a, b;
    expect(run(f, t, toXyz, cam, guess, p, a), "accepted", tag);
    expect(run(f, t, toXyz, cam, guess, p, b), "accepted again", tag);
    expect(std::memcmp(a.transform, b.transform, sizeof a.transform) == 0 && a.status == b.status && a.matches == b.matches && a.inliers == b.inliers &&
           std::memcmp(&a.varianceLin, &b.varianceLin, 8) == 0 && std::memcmp(&a.angleCos, &b.angleCos, 8) == 0 && a.varianceKind == b.varianceKind,
           "the same call gives the same bits", tag);
    expect(std::is_sorted(a.matches.begin(), a.matches.end()) && std::adjacent_find(a.matches.begin(), a.matches.end()) == a.matches.end(), "matches ascend", tag);
    const std::set<int> matches(a.matches.begin(), a.matches.end());
    bool sub = true;
    for (int id : a.inliers) sub = sub && matches.count(id) == 1;
    expect(sub, "inliers are matches", tag);
    bool zero = true;
    for (float v : a.transform) zero = zero && v == 0.0f;
    expect(a.status >= 0 && a.status <= 4, "a status of the enum", tag);
    expect((a.status == 0) == !zero || a.status == 0, "no transform without LCD_PNP_OK", tag);
    const int m = (int)a.matches.size();
    expect((a.status == 1) == (m < p.minInliers || m < 4), "LCD_PNP_FEW_CORRESPONDENCES iff m < min_inliers or m < 4", tag);
    if (a.status == 1 || a.status == 2) expect(a.inliers.empty(), "no inliers without a model", tag);
    if (a.status == 3) expect((int)a.inliers.size() < p.minInliers, "below min_inliers", tag);
    if (a.status == 0 || a.status == 4) expect((int)a.inliers.size() >= p.minInliers, "at least min_inliers", tag);
    if (a.status != 0) expect(a.varianceKind == 0 && a.varianceLin == 1.0 && a.angleCos == 1.0, "the covariance reset", tag);
    else expect(a.varianceKind == 1 || a.varianceKind == 2, "a covariance kind", tag);
    if (a.status == 0 && a.varianceKind == 1) expect(!(a.angleCos > 1.0) && !(a.angleCos < -1.0), "a cosine", tag);
    double cov[36];
    rtabmap_amd::motion_pnp_covariance(a.varianceKind, a.varianceLin, a.angleCos, cov);
}

// a scene under a small motion: m correspondences, a fraction of them outliers, decoy ids around them
void scene(std::mt19937& rng, int m, double outliers, From& f, To& t) {
    std::uniform_real_distribution<float> U(0.0f, 1.0f);
    const float c = std::cos(0.2f), s = std::sin(0.2f), tx = 0.1f, ty = -0.05f, tz = 0.2f;
    for (int i = 0; i < m; ++i) {
        const float z = 0.5f + 9.5f * U(rng), u = 639.0f * U(rng), v = 479.0f * U(rng);
        const float X = (u - 319.5f) / 525.0f * z, Y = (v - 239.5f) / 525.0f * z;
        const float px = c * (X - tx) + s * (z - tz), py = Y - ty, pz = -s * (X - tx) + c * (z - tz);       // R^T (C - t), R about y
        const bool out = U(rng) < outliers;
        f.add(i * 3 - m, px, py, pz);
        t.add(i * 3 - m, out ? 639.0f * U(rng) : u + U(rng) - 0.5f, out ? 479.0f * U(rng) : v + U(rng) - 0.5f, X, Y, i % 7 == 0 ? NAN : z);
    }
    f.add(1 << 20, 1, 1, 1); t.add(1 << 21, 5, 5, 1, 1, 1);                                                // one side only
    f.add(1 << 22, 1, 1, 1); f.add(1 << 22, 2, 2, 2); t.add(1 << 22, 5, 5, 1, 1, 1);                          // twice in from
    f.add(1 << 23, 1, 1, 1); t.add(1 << 23, 5, 5, 1, 1, 1); t.add(1 << 23, 6, 6, 1, 1, 1);                    // twice in to
    f.add(1 << 24, 1, INFINITY, 1); t.add(1 << 24, 5, 5, 1, 1, 1);                                         // a from-point that is not finite
}

}  // namespace

int main() {
    std::mt19937 rng(7);
    int tag = 0;
    MotionPnpParams base;
    base.minInliers = 4; base.iterations = 60; base.refineIterations = 5; base.varianceMedianRatio = 4; base.reprojError = 2.0; base.seed = 3;
    const float guess[12] = {0.98f, 0, 0.2f, 0.1f, 0, 1, 0, 0, -0.2f, 0, 0.98f, -0.1f};
    // 0 .. 6 correspondences, every covariance branch, with and without a guess
    for (int m = 0; m <= 6; ++m)
        for (int v = 0; v < 8; ++v) {
            From f; To t;
            scene(rng, m, 0.0, f, t);
            MotionPnpParams p = base;
            p.minInliers = 1 + (v % 3) * 2;
            check(f, t, v & 1, camera(v & 2, v & 4), v & 4 ? guess : nullptr, p, ++tag);
        }
    // iterations x refinement passes at the chunk edges
    for (int it : {1, 255, 256, 257})
        for (int rf : {0, 1, 5}) {
            From f; To t;
            scene(rng, 120, 0.4, f, t);
            MotionPnpParams p = base;
            p.iterations = it; p.refineIterations = rf; p.maxVariance = rf == 1 ? 1e-6f : 0.0f;
            check(f, t, it & 1, camera(rf == 5, rf == 1), nullptr, p, ++tag);
        }
    {   // all outliers; every point behind the camera; collinear and coincident triples
        From f; To t;
        scene(rng, 60, 1.1, f, t);
        check(f, t, true, camera(true, false), nullptr, base, ++tag);
        From b; To bt;
        for (int i = 0; i < 30; ++i) { b.add(i, 0.1f * i - 1, 0.05f * i, -2.0f - 0.1f * i); bt.add(i, 20.0f * i, 10.0f * i, 0, 0, 1); }
        check(b, bt, false, camera(false, false), nullptr, base, ++tag);
        From l; To lt;
        for (int i = 0; i < 12; ++i) { l.add(i, (float)i, 0, 4); lt.add(i, 100.0f + 30.0f * i, 240, (float)i, 0, 4); }
        check(l, lt, true, camera(true, false), nullptr, base, ++tag);
        From c; To ct;
        for (int i = 0; i < 12; ++i) { c.add(i, 1, 2, 3); ct.add(i, 320, 240, 1, 2, 3); }
        check(c, ct, true, camera(true, true), nullptr, base, ++tag);
    }
    {   // NaN, infinite and huge coordinates; INT_MIN and INT_MAX ids
        const float bad[] = {NAN, INFINITY, -INFINITY, 3.0e38f, -3.0e38f, 1.0e19f, 1.0e-38f, 0.0f};
        for (float w : bad) {
            From f; To t;
            scene(rng, 20, 0.2, f, t);
            f.xyz[4] = w; f.xyz[9] = w; t.uv[6] = w; t.uv[11] = w; t.xyz[12] = w;
            f.add(INT_MIN, w, 1, 2); t.add(INT_MIN, 10, w, 1, 1, w);
            f.add(INT_MAX, 1, 1, w); t.add(INT_MAX, w, w, w, w, w);
            check(f, t, true, camera(true, false), nullptr, base, ++tag);
            check(f, t, false, camera(false, true), guess, base, ++tag);
            From h; To ht;                                              // every coordinate the same bad value
            for (int i = 0; i < 8; ++i) { h.add(i, w, w, w); ht.add(i, w, w, w, w, w); }
            check(h, ht, true, camera(true, false), nullptr, base, ++tag);
        }
        const float wild[12] = {NAN, 1e30f, 0, INFINITY, 0, 0, 0, 0, 1, 1, 1, -INFINITY};
        From f; To t;
        scene(rng, 20, 0.2, f, t);
        check(f, t, true, camera(true, true), wild, base, ++tag);
    }
    {   // 8192 rows a side
        From f; To t;
        scene(rng, 8185, 0.3, f, t);
        f.ids.resize(8192); f.xyz.resize(8192 * 3); t.ids.resize(8192); t.uv.resize(8192 * 2); t.xyz.resize(8192 * 3);
        MotionPnpParams p = base;
        p.iterations = 20; p.refineIterations = 2; p.minInliers = 20;
        check(f, t, true, camera(true, false), nullptr, p, ++tag);
    }
    {   // refused arguments: the result stays untouched
        From f; To t;
        scene(rng, 10, 0.0, f, t);
        const lcd_camera cam = camera(false, false);
        MotionPnpResult r;
        r.status = -7;
        auto refused = [&](MotionPnpParams p, const char* what) {
            ++cases;
            expect(!run(f, t, true, cam, nullptr, p, r) && r.status == -7, what, ++tag);
        };
        MotionPnpParams p = base;
        p.iterations = 0; refused(p, "iterations 0"); p = base;
        p.iterations = 65536; refused(p, "iterations 65536"); p = base;
        p.reprojError = 0.0; refused(p, "reproj_error 0"); p = base;
        p.reprojError = NAN; refused(p, "reproj_error NaN"); p = base;
        p.reprojError = 1e-60; refused(p, "reproj_error that is 0 as a float"); p = base;
        p.reprojError = 1e30; refused(p, "reproj_error whose square is not finite"); p = base;
        p.refineIterations = -1; refused(p, "refine_iterations -1"); p = base;
        p.minInliers = 0; refused(p, "min_inliers 0"); p = base;
        p.varianceMedianRatio = 1; refused(p, "variance_median_ratio 1"); p = base;
        p.maxVariance = -1.0f; refused(p, "max_variance -1"); p = base;
        p.maxVariance = NAN; refused(p, "max_variance NaN"); p = base;
        p.steps = -1; refused(p, "steps -1");
        ++cases;
        expect(!motion_pnp_cpu(nullptr, f.xyz.data(), 5, t.ids.data(), t.uv.data(), nullptr, 5, cam, nullptr, base, r), "a null frame", ++tag);
        ++cases;
        expect(!motion_pnp_cpu(f.ids.data(), f.xyz.data(), 5, t.ids.data(), nullptr, nullptr, 5, cam, nullptr, base, r), "null keypoints", ++tag);
        ++cases;
        expect(!motion_pnp_cpu(f.ids.data(), f.xyz.data(), 8193, t.ids.data(), t.uv.data(), nullptr, 5, cam, nullptr, base, r), "8193 rows", ++tag);
    }
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("ok: %d cases\n", cases);
    return 0;
}
