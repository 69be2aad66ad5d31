// sanitize_motion_ba.cpp -- motion_ba_cpu (plain host code: the whole rule of lcd_refine_motion_ba) driven from a stand-alone program, for a
// host-only AddressSanitizer / UndefinedBehaviorSanitizer run.  No engine is created and nothing touches a GPU.
//
//   g++ -std=c++17 -g -O1 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -Irtabmap_amd/host \
//       tools/sanitize_motion_ba.cpp rtabmap_amd/host/MotionBA.cpp rtabmap_amd/host/Motion2D.cpp -o motion_ba_asan
//   ./motion_ba_asan
//
// Frames, inlier lists and transforms whose buffers end with their last element (a read past one is a heap overflow): 1 to 600 inliers, with
// and without from-keypoints, to-points, a prior, local transforms and baselines, planted outliers, no kernel, no iterations, each gate alone,
// NaN and huge keypoints, an id missing from a frame or twice in it, a from-point that is not finite, counts outside the region, a zero
// transform, 8192 rows, and every refused argument, the NULL pointers and negative row counts among them.  Every result is checked against what the rule promises whatever the numbers are, every
// status must occur; exit status 0 and "ok" with the number of cases when all hold.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <set>
#include <vector>

#include "MotionBA.h"

// the engine entries of MotionBA.cpp and Motion2D.cpp are linked but never called here
extern "C" int lcd_refine_motion_ba(lcd_engine*, const lcd_motion_ba_args*) { return 1; }
extern "C" int lcd_estimate_motion_pnp(lcd_engine*, const lcd_motion_pnp_args*) { return 1; }

using rtabmap_amd::MotionBAParams;
using rtabmap_amd::MotionBAResult;
using rtabmap_amd::motion_ba_cpu;

namespace {

int failures = 0, cases = 0;
int seen[7] = {0, 0, 0, 0, 0, 0, 0};
void expect(bool ok, const char* what, int tag) {
    if (!ok) { std::printf("FAILED: %s (case %d)\n", what, tag); ++failures; }
}

lcd_camera camera(bool local) {
    lcd_camera c = {};
    c.fx = 525.0f; c.fy = 525.0f; c.cx = 319.5f; c.cy = 239.5f; c.image_width = 640; c.image_height = 480;
    if (local) {
        const float t[12] = {0, 0, 1, 0.1f, -1, 0, 0, 0.02f, 0, -1, 0, 0.3f};
        c.has_local_transform = 1;
        std::copy(t, t + 12, c.local_transform);
    }
    return c;
}

struct Scene {
    std::vector<int32_t> fromIds, toIds, inliers;
    std::vector<float> fromXyz, fromUv, toUv, toXyz;
    float transform[12];
};

// two views of m points: the to-camera a little to the right of the from-camera and turned about y; `outliers` to-keypoints 40 px off; `extra`
// rows of one side only
Scene scene(std::mt19937& rng, int m, int outliers, int extra) {
    std::uniform_real_distribution<float> U(0.0f, 1.0f);
    std::normal_distribution<float> N(0.0f, 0.5f);
    Scene s;
    const float a = 0.05f, ca = std::cos(a), sa = std::sin(a), tx = 0.2f;
    // the to-camera's pose in the from-camera: rotation about y by a, translation (tx, 0, 0); its model is the inverse
    const float T[12] = {ca, 0, sa, tx, 0, 1, 0, 0, -sa, 0, ca, 0};
    for (int k = 0; k < 12; ++k) s.transform[k] = T[k];
    s.transform[3] += 0.01f; s.transform[7] -= 0.01f;
    for (int i = 0; i < m; ++i) {
        const float z = 2.0f + 6.0f * U(rng), x = (U(rng) - 0.5f) * z * 0.8f, y = (U(rng) - 0.5f) * z * 0.6f;
        const float dx = x - tx, cx = ca * dx - sa * z, cz = sa * dx + ca * z;        // R^T (p - t)
        s.fromIds.push_back(1000 + 3 * i); s.toIds.push_back(1000 + 3 * i); s.inliers.push_back(1000 + 3 * i);
        s.fromXyz.insert(s.fromXyz.end(), {x, y, z});
        s.fromUv.insert(s.fromUv.end(), {525.0f * x / z + 319.5f + N(rng), 525.0f * y / z + 239.5f + N(rng)});
        const float off = i < outliers ? 40.0f : 0.0f;
        s.toUv.insert(s.toUv.end(), {525.0f * cx / cz + 319.5f + N(rng) + off, 525.0f * y / cz + 239.5f + N(rng)});
        s.toXyz.insert(s.toXyz.end(), {cx, y, cz});
    }
    for (int e = 0; e < extra; ++e) {
        s.fromIds.push_back(-5 - e); s.fromXyz.insert(s.fromXyz.end(), {1.0f, 1.0f, 4.0f}); s.fromUv.insert(s.fromUv.end(), {10.0f, 20.0f});
        s.toIds.push_back(900000 + e); s.toUv.insert(s.toUv.end(), {30.0f, 40.0f}); s.toXyz.insert(s.toXyz.end(), {0.5f, 0.5f, 3.0f});
    }
    return s;
}

// heap copies that end with the last element
bool run(const Scene& s, bool fromUv, bool toXyz, const double* prior, const lcd_camera& cf, const lcd_camera& ct, const MotionBAParams& p, int nInliers,
         MotionBAResult& r) {
    std::vector<int32_t> fi(s.fromIds), ti(s.toIds), in(s.inliers);
    std::vector<float> fx(s.fromXyz), fu(s.fromUv), tu(s.toUv), tx(s.toXyz), tr(s.transform, s.transform + 12);
    std::vector<double> pv;
    if (prior) pv.assign(prior, prior + 2);
    in.resize(ti.size(), 0);                                           // the PnP's out_inliers: the to-region, zeros behind the ids
    ++cases;
    return motion_ba_cpu(fi.data(), fx.data(), fromUv ? fu.data() : nullptr, (int)fi.size(), ti.data(), tu.data(), toXyz ? tx.data() : nullptr, (int)ti.size(),
                         in.data(), nInliers, tr.data(), prior ? pv.data() : nullptr, cf, ct, p, r);
}

void check(const Scene& s, const MotionBAResult& r, int nInliers, const MotionBAParams& p, int tag) {
    expect(r.status >= 0 && r.status <= 6, "status in range", tag);
    if (r.status < 0 || r.status > 6) return;
    ++seen[r.status];
    bool zero = true;
    for (int k = 0; k < 12; ++k) { zero = zero && r.transform[k] == 0.0f; }
    expect((r.status == 0) == !zero, "a transform iff LCD_BA_OK", tag);
    size_t at = 0;                                                     // the survivors are a subsequence of the inliers (a count past the list takes its zeros along)
    for (int id : r.inliers) {
        if (nInliers > (int)s.inliers.size()) break;
        while (at < s.inliers.size() && s.inliers[at] != id) ++at;
        expect(at < s.inliers.size(), "survivors in input order", tag);
        ++at;
    }
    if (r.status == 0 || r.status >= 4) expect((int)r.inliers.size() + r.nOutliers == nInliers, "survivors + outliers = inliers", tag);
    if (r.status == 0) {
        for (int k = 0; k < 12; ++k) expect(std::isfinite(r.transform[k]), "finite transform", tag);
        expect((int)r.inliers.size() >= p.minInliers, "min_inliers holds", tag);
        if (p.iterations > 0) expect(r.chi2After <= r.chi2Before, "the cost did not grow", tag);
    }
    if (r.status == 4) expect((int)r.inliers.size() < p.minInliers, "below min_inliers", tag);
    if (r.status == 1 || r.status == 2) expect(r.nOutliers == 0 && r.lmAccepted == 0, "nothing refined", tag);
}

}  // namespace

int main() {
    std::mt19937 rng(7);
    int tag = 0;
    const double prior[2] = {1e-4, 4e-4}, floor_[2] = {0.0, 0.0};
    // ---- sizes x optional arrays x locals
    for (int m : {1, 2, 3, 4, 63, 64, 65, 255, 256, 257, 600})
        for (int v = 0; v < 8; ++v) {
            const Scene s = scene(rng, m, m / 10, v % 3);
            MotionBAParams p;
            p.minInliers = 1;
            if (v == 5) { p.baselineFrom = 0.0; p.baselineTo = -1.0; }
            if (v == 6) p.robustDelta = 0.0;
            if (v == 7) { p.iterations = 0; p.maxInliersMeanDistance = 100.0f; p.minInliersDistribution = 1e-6f; }
            MotionBAResult r;
            const bool ok = run(s, (v & 1) == 0, (v & 2) == 0, v == 3 ? nullptr : v == 4 ? floor_ : prior, camera(v == 2), camera(v >= 2 && v < 5), p, m, r);
            expect(ok, "accepted", ++tag);
            if (ok) check(s, r, m, p, tag);
        }
    // ---- the statuses
    {
        MotionBAParams p;
        p.minInliers = 20;
        MotionBAResult r;
        Scene s = scene(rng, 40, 4, 5);
        Scene z = s;
        std::fill(z.transform, z.transform + 12, 0.0f);
        expect(run(z, true, true, prior, camera(false), camera(false), p, 40, r) && r.status == 1 && r.inliers.size() == 40, "a zero transform passes through", ++tag);
        check(z, r, 40, p, tag);
        expect(run(s, true, true, prior, camera(false), camera(false), p, 0, r) && r.status == 1 && r.inliers.empty(), "no inliers", ++tag);
        check(s, r, 0, p, tag);
        for (int n : {-1, 46, 1 << 30}) {
            expect(run(s, true, true, prior, camera(false), camera(false), p, n, r) && r.status == 2, "a count outside the region", ++tag);
            check(s, r, n, p, tag);
        }
        Scene missing = s;
        missing.inliers[39] = 77;                                      // in neither frame
        expect(run(missing, true, true, prior, camera(false), camera(false), p, 40, r) && r.status == 2, "an id of no frame", ++tag);
        Scene twice = s;
        twice.toIds[41] = twice.inliers[3];                            // twice in the to-frame
        expect(run(twice, true, true, prior, camera(false), camera(false), p, 40, r) && r.status == 2, "an id twice in a frame", ++tag);
        Scene inf = s;
        inf.fromXyz[3 * 39 + 2] = std::numeric_limits<float>::infinity();
        expect(run(inf, true, true, prior, camera(false), camera(false), p, 40, r) && r.status == 2, "a from-point that is not finite", ++tag);
        check(inf, r, 40, p, tag);
        Scene nan = s;
        nan.toUv[2 * 39] = std::nanf("");
        expect(run(nan, true, true, prior, camera(false), camera(false), p, 40, r) && r.status == 3 && r.inliers.size() == 40, "a NaN keypoint diverges", ++tag);
        check(nan, r, 40, p, tag);
        Scene huge = s;
        huge.toUv[2 * 39] = 1e7f;
        MotionBAParams plain = p;
        plain.robustDelta = 0.0;
        expect(run(huge, true, true, prior, camera(false), camera(false), plain, 40, r) && r.status == 3, "a cost above 1e12 diverges", ++tag);
        check(huge, r, 40, plain, tag);
        Scene few = scene(rng, 24, 6, 0);
        expect(run(few, true, true, prior, camera(false), camera(false), p, 24, r) && r.status == 4, "below min_inliers behind the filtering", ++tag);
        check(few, r, 24, p, tag);
        MotionBAParams near = p;
        near.maxInliersMeanDistance = 1.0f;
        expect(run(s, true, true, prior, camera(false), camera(false), near, 40, r) && r.status == 5 && r.inliersMeanDistance > 1.0f, "the mean distance gate", ++tag);
        check(s, r, 40, near, tag);
        MotionBAParams wide = p;
        wide.minInliersDistribution = 10.0f;
        expect(run(s, true, true, prior, camera(false), camera(false), wide, 40, r) && r.status == 6 && r.inliersDistribution > 0.0f, "the distribution gate", ++tag);
        check(s, r, 40, wide, tag);
        lcd_camera unsized = camera(false);
        unsized.image_width = 0;
        expect(run(s, true, true, prior, camera(false), unsized, wide, 40, r) && r.status == 0 && r.inliersDistribution == 0.0f, "no image size: no distribution gate", ++tag);
        expect(run(s, true, false, prior, camera(false), camera(false), near, 40, r) && r.status == 0 && r.inliersMeanDistance == 0.0f, "no to-points: no distance gate", ++tag);
    }
    // ---- 8192 rows
    {
        const Scene s = scene(rng, 8192, 100, 0);
        MotionBAParams p;
        MotionBAResult r;
        expect(run(s, true, true, prior, camera(false), camera(true), p, 8192, r), "8192 rows", ++tag);
        check(s, r, 8192, p, tag);
    }
    // ---- the refusals
    {
        const Scene s = scene(rng, 30, 0, 2);
        MotionBAResult r;
        r.status = -7;
        const double inf = std::numeric_limits<double>::infinity(), nan = std::nan("");
        auto refused = [&](const MotionBAParams& p, const double* pv, const lcd_camera& cf, const lcd_camera& ct, const char* what) {
            expect(!run(s, true, true, pv, cf, ct, p, 30, r) && r.status == -7, what, ++tag);
        };
        const lcd_camera c = camera(false);
        MotionBAParams p;
        p = MotionBAParams(); p.iterations = -1; refused(p, prior, c, c, "iterations < 0");
        p = MotionBAParams(); p.iterations = 65536; refused(p, prior, c, c, "iterations > 65535");
        p = MotionBAParams(); p.minInliers = -1; refused(p, prior, c, c, "min_inliers < 0");
        for (double v : {0.0, -1.0, nan, inf, 1e-60, 1e60}) { p = MotionBAParams(); p.pixelVariance = v; refused(p, prior, c, c, "pixel_variance"); }
        for (double v : {-1.0, nan, inf, 1e30}) { p = MotionBAParams(); p.robustDelta = v; refused(p, prior, c, c, "robust_delta"); }
        for (float v : {-1.0f, std::nanf(""), std::numeric_limits<float>::infinity()}) {
            p = MotionBAParams(); p.maxInliersMeanDistance = v; refused(p, prior, c, c, "max_inliers_mean_distance");
            p = MotionBAParams(); p.minInliersDistribution = v; refused(p, prior, c, c, "min_inliers_distribution");
        }
        for (double v : {nan, inf}) {
            p = MotionBAParams(); p.baselineFrom = v; refused(p, prior, c, c, "baseline");
            p = MotionBAParams(); p.baselineTo = v; refused(p, prior, c, c, "baseline");
        }
        for (double v : {-1e-9, nan, inf}) {
            const double a[2] = {v, 1e-4}, b[2] = {1e-4, v};
            refused(MotionBAParams(), a, c, c, "linear prior variance");
            refused(MotionBAParams(), b, c, c, "angular prior variance");
        }
        for (float v : {0.0f, std::nanf(""), std::numeric_limits<float>::infinity()}) {
            lcd_camera bad = c;
            bad.fx = v; refused(MotionBAParams(), prior, bad, c, "fx of the from-camera");
            bad = c; bad.fy = v; refused(MotionBAParams(), prior, c, bad, "fy of the to-camera");
        }
        const Scene big = scene(rng, 10, 0, 8183);                     // 8193 rows a side
        expect(!run(big, true, true, prior, c, c, MotionBAParams(), 10, r) && r.status == -7, "more than 8192 rows", ++tag);
        // a NULL pointer where rows exist, a NULL transform, negative row counts
        std::vector<int32_t> fi(s.fromIds), ti(s.toIds), in(s.inliers);
        std::vector<float> fx(s.fromXyz), fu(s.fromUv), tu(s.toUv), tx(s.toXyz), tr(s.transform, s.transform + 12);
        in.resize(ti.size(), 0);
        const int nf = (int)fi.size(), nt = (int)ti.size();
        auto raw = [&](const int32_t* a, const float* b, int na, const int32_t* d, const float* e, int nd, const int32_t* l, const float* t, const char* what) {
            ++cases;
            expect(!motion_ba_cpu(a, b, fu.data(), na, d, e, tx.data(), nd, l, 30, t, prior, c, c, MotionBAParams(), r) && r.status == -7, what, ++tag);
        };
        raw(nullptr, fx.data(), nf, ti.data(), tu.data(), nt, in.data(), tr.data(), "null from ids");
        raw(fi.data(), nullptr, nf, ti.data(), tu.data(), nt, in.data(), tr.data(), "null from points");
        raw(fi.data(), fx.data(), nf, nullptr, tu.data(), nt, in.data(), tr.data(), "null to ids");
        raw(fi.data(), fx.data(), nf, ti.data(), nullptr, nt, in.data(), tr.data(), "null to keypoints");
        raw(fi.data(), fx.data(), nf, ti.data(), tu.data(), nt, nullptr, tr.data(), "null inliers");
        raw(fi.data(), fx.data(), nf, ti.data(), tu.data(), nt, in.data(), nullptr, "null transform");
        raw(fi.data(), fx.data(), -1, ti.data(), tu.data(), nt, in.data(), tr.data(), "negative from rows");
        raw(fi.data(), fx.data(), nf, ti.data(), tu.data(), -1, in.data(), tr.data(), "negative to rows");
    }
    for (int st = 0; st < 7; ++st) expect(seen[st] > 0, "every status occurs", 1000 + st);
    if (failures) { std::printf("%d failure(s) in %d cases\n", failures, cases); return 1; }
    std::printf("ok %d\n", cases);
    return 0;
}
