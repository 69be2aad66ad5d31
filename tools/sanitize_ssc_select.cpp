// sanitize_ssc_select.cpp -- FeatureSelect's two Kp/SSC forms (plain host code: the LCD_SELECT_SSC rule of lcd_select_features) driven from
// a stand-alone program, for a host-only AddressSanitizer / UndefinedBehaviorSanitizer run.  No engine is created and nothing touches a GPU.
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Irtabmap_amd/host \
//       tools/sanitize_ssc_select.cpp rtabmap_amd/host/FeatureSelect.cpp -o ssc_select_asan
//   ./ssc_select_asan
//
// Every buffer is allocated at its exact size, so a read behind a frame's last feature is a heap overflow.  Covered: random frames on
// images from 1 x 1 to 16384 x 16384 (uniform, all in one pixel, on the borders), n = maxKeypoints + 1, maxKeypoints 2 and 3, every refused
// argument, NaN / infinite / negative / denormal coordinates and responses, and maxKeypoints near INT_MAX (the products of exp2 are long
// long for that).  Each accepted result is checked against a restatement with the pairwise reading of the covering; exit status 0 and
// "ok" when all agree.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "FeatureSelect.h"

using rtabmap_amd::FeatureSelect;

static const float kInf = std::numeric_limits<float>::infinity(), kNaN = std::numeric_limits<float>::quiet_NaN();

static long long roundAway(double v) { return (long long)(v < 0 ? -std::floor(-v + 0.5) : std::floor(v + 0.5)); }

// the rule restated: signed order with ties to the lower index, the binary search, and the covering as "no earlier selected feature within
// 2 cells in both directions" by a plain quadratic loop
static std::vector<int> restated(const std::vector<float>& r, const std::vector<float>& p, int n, int maxKeypoints, int cols, int rows) {
    std::vector<int> order((size_t)n);
    for (int i = 0; i < n; ++i) order[(size_t)i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return r[(size_t)a] > r[(size_t)b]; });   // -0.0 == 0.0; no NaN here
    const float tol = 0.1f;
    const long long m = maxKeypoints - roundAway(maxKeypoints * tol);
    const long long exp1 = (long long)rows + cols + 2 * m;
    const long long exp2 = 4ll * cols + 4ll * m + 4ll * rows * m + (long long)rows * rows + (long long)cols * cols - 2ll * rows * cols + 4ll * rows * cols * m;
    const double exp3 = std::sqrt((double)exp2), exp4 = (double)(m - 1);
    const double s1 = -(double)roundAway((exp1 + exp3) / exp4), s2 = -(double)roundAway((exp1 - exp3) / exp4);
    long long high = (long long)(s1 > s2 ? s1 : s2), low = std::max(1ll, (long long)std::floor(std::sqrt((double)n / (double)m)));
    const float fm = (float)m;
    const long long kMin = roundAway(fm - fm * tol), kMax = roundAway(fm + fm * tol);
    long long prev = -1;
    std::vector<int> result;
    for (;;) {
        const long long width = low + (high - low) / 2;
        if (width == prev || low > high) break;
        result.clear();
        const double c = (double)width / 2.0;
        std::vector<long long> sr, sc;
        for (int k = 0; k < n; ++k) {
            const int i = order[(size_t)k];
            const long long row = (long long)std::floor((double)p[(size_t)2 * i + 1] / c), col = (long long)std::floor((double)p[(size_t)2 * i] / c);
            bool covered = false;
            for (size_t s = 0; s < sr.size() && !covered; ++s) covered = std::llabs(sr[s] - row) <= 2 && std::llabs(sc[s] - col) <= 2;
            if (covered) continue;
            sr.push_back(row); sc.push_back(col);
            result.push_back(i);
        }
        const long long size = (long long)result.size();
        if (size >= kMin && size <= kMax) break;
        if (size < kMin) high = width - 1; else low = width + 1;
        prev = width;
    }
    return result;
}

static int fail(const char* what, int it) { std::fprintf(stderr, "%s: mismatch at iteration %d\n", what, it); return 1; }

int main() {
    std::mt19937 rng(23);
    auto upto = [&](int n) { return n <= 0 ? 0 : (int)(rng() % (unsigned)n); };
    auto unit = [&]() { return (float)(rng() >> 8) / 16777216.0f; };
    const float pool[] = {0.0f, -0.0f, 1e-45f, -1e-45f, 0.5f, -0.5f, 1.0f, 1.0f, -1.0f, 7.25f, kInf, -3e38f};
    const int sides[] = {1, 2, 7, 16, 17, 33, 100, 480, 640, 16384};
    long checked = 0, refused = 0, above = 0, empty = 0;
    for (int it = 0; it < 6000; ++it) {
        const int n = it % 50 == 0 ? 0 : 1 + upto(it % 9 == 0 ? 400 : 60);
        int maxKeypoints = it % 5 == 0 ? n - 1 : it % 5 == 1 ? 2 + upto(2) : upto(n + 4) - 1;       // n = max + 1; 2 and 3; anything from -1 up
        int cols = sides[upto(10)], rows = sides[upto(10)];
        std::vector<float> r((size_t)n), p((size_t)2 * n);                                           // exact sizes: the last feature ends the buffer
        const int shape = it % 4;                                                                    // uniform, one pixel, borders, tied uniform
        const float px = unit() * (float)cols, py = unit() * (float)rows;
        for (int i = 0; i < n; ++i) {
            r[(size_t)i] = shape == 0 ? unit() * 100.0f - 30.0f : pool[upto(12)];
            float x = unit() * (float)cols, y = unit() * (float)rows;
            if (shape == 1) { x = px; y = py; }
            if (shape == 2 && i % 2) { const float edge[] = {0.0f, -0.0f, (float)cols, 1e-45f}; x = edge[upto(4)]; }
            if (shape == 2 && i % 3 == 0) { const float edge[] = {0.0f, (float)rows, 1e-40f}; y = edge[upto(3)]; }
            p[(size_t)2 * i] = x; p[(size_t)2 * i + 1] = y;
        }
        bool expectOk = maxKeypoints != 1;
        const bool cut = maxKeypoints > 0 && n > maxKeypoints;
        const int trouble = it % 7 == 0 && n > 0 ? 1 + upto(9) : 0;
        const float badCoord[] = {-0.5f, -1e-45f, kNaN, kInf, -kInf, (float)cols + 0.5f, 3e38f};
        bool nullPoints = false;
        switch (trouble) {
            case 1: r[(size_t)upto(n)] = kNaN; expectOk = false; break;                              // refused whether the frame is cut or not
            case 2: p[(size_t)2 * upto(n)] = badCoord[upto(7)]; if (cut) expectOk = false; break;
            case 3: p[(size_t)2 * upto(n) + 1] = -1.0f; if (cut) expectOk = false; break;
            case 4: cols = 0; if (cut) expectOk = false; break;
            case 5: rows = -3; if (cut) expectOk = false; break;
            case 6: cols = 16385; if (cut) expectOk = false; break;
            case 7: rows = INT_MAX; if (cut) expectOk = false; break;
            case 8: nullPoints = true; if (cut) expectOk = false; break;
            case 9: maxKeypoints = 1; expectOk = false; break;
            default: break;
        }
        if (trouble == 2 || trouble == 3)                                                            // a coordinate moved: does it still lie in [0, side]?
            for (int i = 0; i < n && cut; ++i)
                if (!(p[(size_t)2 * i] >= 0.0f && p[(size_t)2 * i] <= (float)cols && p[(size_t)2 * i + 1] >= 0.0f && p[(size_t)2 * i + 1] <= (float)rows)) expectOk = false;
        std::vector<int> kept(2, -5);
        std::vector<bool> inliers(3, true);
        const float* pp = nullPoints ? nullptr : p.data();
        const bool ok = FeatureSelect::limitKeypointsSSC(r.data(), pp, n, maxKeypoints, cols, rows, kept);
        const bool ok2 = FeatureSelect::limitKeypointsSSC(r.data(), pp, n, maxKeypoints, cols, rows, inliers);
        if (ok != expectOk || ok2 != expectOk) return fail("accepted / refused", it);
        if (!ok) {
            if (kept != std::vector<int>(2, -5) || inliers != std::vector<bool>(3, true)) return fail("outputs touched by a refusal", it);
            ++refused;
            continue;
        }
        std::vector<int> expected;
        if (cut) expected = restated(r, p, n, maxKeypoints, cols, rows);
        else for (int i = 0; i < n; ++i) expected.push_back(i);
        if (kept != expected) return fail("limitKeypointsSSC (compacting)", it);
        std::vector<bool> mask((size_t)n, false);
        for (int i : expected) mask[(size_t)i] = true;
        if (inliers != mask) return fail("limitKeypointsSSC (mask)", it);
        if (cut && (int)kept.size() > maxKeypoints) ++above;
        if (cut && kept.empty()) ++empty;
        checked += n;
    }
    // maxKeypoints near INT_MAX can only cut a frame of more features than a test holds: the scalars alone, through a frame that is not cut,
    // and the products of exp2 at the largest image -- 4 * 16384 * 16384 * m is 2^30 m -- through the largest max a small frame is cut by
    {
        std::vector<float> r(5, 1.0f), p(10, 0.0f);
        std::vector<int> kept;
        if (!FeatureSelect::limitKeypointsSSC(r.data(), p.data(), 5, INT_MAX, 16384, 16384, kept) || kept.size() != 5) return fail("INT_MAX, not cut", 0);
        std::vector<float> r2(4000), p2(8000);
        for (int i = 0; i < 4000; ++i) { r2[(size_t)i] = (float)(i % 97); p2[(size_t)2 * i] = unit() * 16384.0f; p2[(size_t)2 * i + 1] = unit() * 16384.0f; }
        if (!FeatureSelect::limitKeypointsSSC(r2.data(), p2.data(), 4000, 3999, 16384, 16384, kept)) return fail("16384 x 16384, 3999", 0);
        if (kept != restated(r2, p2, 4000, 3999, 16384, 16384)) return fail("16384 x 16384 against the restatement", 0);
        // all 4000 in one pixel of the largest image: the search walks down to width 1, where the mirror leaves the byte mask for its row lists
        for (int i = 0; i < 4000; ++i) { p2[(size_t)2 * i] = 16384.0f; p2[(size_t)2 * i + 1] = 16384.0f; }
        if (!FeatureSelect::limitKeypointsSSC(r2.data(), p2.data(), 4000, 2000, 16384, 16384, kept) || kept.size() != 1) return fail("one pixel at the far corner", 0);
    }
    if (refused < 100 || above < 10 || empty < 10) { std::fprintf(stderr, "the cases do not reach what they are for: %ld refused, %ld above max, %ld empty\n", refused, above, empty); return 1; }
    std::printf("ok: 6000 cases, %ld features, %ld refused, %ld above maxKeypoints, %ld empty\n", checked, refused, above, empty);
    return 0;
}
