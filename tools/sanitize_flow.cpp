// sanitize_flow.cpp -- flow_track_cpu (plain host code: the rule of lcd_track_flow) driven from a stand-alone program, for a host-only
// AddressSanitizer / UndefinedBehaviorSanitizer run.  No engine is created and nothing touches a GPU.
//
//   g++ -std=c++17 -g -O1 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -Irtabmap_amd/host \
//       tools/sanitize_flow.cpp rtabmap_amd/host/FlowTrack.cpp rtabmap_amd/host/Stereo.cpp -o flow_asan
//   ./flow_asan
//
// Random image pairs whose buffers end with their last pixel (a read of the border that is not reflected is a heap overflow), a pitch
// larger than the row, windows of 3 x 3 to 31 x 31, 0 to 8 levels, both error modes, with and without start positions, corners at, near
// and beyond every border, NaN, infinite and huge coordinates.  What the mirror answers is checked against what the rule promises without
// restating the tracker: a refusal writes nothing; the kept list is ascending and is exactly the corners with the status set, a finite
// track inside [0, width) x [0, height) and, with the L1 error, an error below the threshold; an untrackable corner has status 0, the
// track (NaN, NaN) and the error 0; without iterations a tracked corner stays at its start; two runs give the same bits.  Exit status 0
// and "ok" when all hold.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "FlowTrack.h"

using rtabmap_amd::FlowParams;
using rtabmap_amd::GrayImage;
using rtabmap_amd::flow_track_cpu;

namespace {

bool convertible(float v) { return v > -2147483648.0f && v < 2147483648.0f; }
bool sameBits(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }

}  // namespace

int main() {
    std::mt19937 rng(54321);
    auto uni = [&](double lo, double hi) { return std::uniform_real_distribution<double>(lo, hi)(rng); };
    long pairs = 0, corners = 0, tracked = 0, keptAll = 0, refused = 0;
    for (int round = 0; round < 400; ++round) {
        FlowParams fp;
        const int wins[][2] = {{16, 16}, {3, 3}, {8, 8}, {5, 13}, {31, 31}, {15, 3}};
        fp.winWidth = wins[round % 6][0]; fp.winHeight = wins[round % 6][1];
        const int maxLevel = round % 7 == 6 ? 8 : round % 5;
        fp.useMinEigenVals = round % 2 == 0;
        fp.iterations = round % 5 == 4 ? 3 : (round % 19 == 7 ? 0 : 30);
        fp.errorThreshold = round % 3 == 0 ? 2.0f : 20.0f;
        if (round % 11 == 0) fp.minEigThreshold = 0.0;
        const int w = fp.winWidth + 1 + (int)(rng() % 90), h = fp.winHeight + 1 + (int)(rng() % 60);
        const int pitchA = w + (round % 3 == 0 ? (int)(rng() % 9) : 0), pitchB = w + (round % 4 == 0 ? (int)(rng() % 5) : 0);
        // buffers that end with the last pixel
        std::vector<unsigned char> from((size_t)(h - 1) * pitchA + w), to((size_t)(h - 1) * pitchB + w);
        const int sx = (int)(rng() % 4), sy = (int)(rng() % 3);
        const int W = w + 8, H = h + 8;
        std::vector<double> scene((size_t)H * W);
        for (double& v : scene) v = uni(0, 255);
        for (int pass = 0; pass < 2; ++pass) {
            for (int y = 0; y < H; ++y)
                for (int x = 1; x + 1 < W; ++x) scene[(size_t)y * W + x] = (scene[(size_t)y * W + x - 1] + 2 * scene[(size_t)y * W + x] + scene[(size_t)y * W + x + 1]) / 4;
            for (int y = 1; y + 1 < H; ++y)
                for (int x = 0; x < W; ++x) scene[(size_t)y * W + x] = (scene[(size_t)(y - 1) * W + x] + 2 * scene[(size_t)y * W + x] + scene[(size_t)(y + 1) * W + x]) / 4;
        }
        std::fill(from.begin(), from.end(), 201); std::fill(to.begin(), to.end(), 77);
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) {
                from[(size_t)y * pitchA + x] = (unsigned char)scene[(size_t)y * W + x];
                to[(size_t)y * pitchB + x] = round % 13 == 5 ? (unsigned char)std::min(255, x * 3 + y) : (unsigned char)scene[(size_t)(y + sy) * W + x + sx];
            }
        const GrayImage ga{from.data(), pitchA, w, h}, gb{to.data(), pitchB, w, h};
        const int n = 48;
        std::vector<float> pts((size_t)n * 2), start((size_t)n * 2);
        const float hx = (fp.winWidth - 1) * 0.5f, hy = (fp.winHeight - 1) * 0.5f;
        for (int i = 0; i < n; ++i) {
            pts[2 * i] = (float)uni(-fp.winWidth - 2.0, w + fp.winWidth + 2.0); pts[2 * i + 1] = (float)uni(-fp.winHeight - 2.0, h + fp.winHeight + 2.0);
            if (i % 4 == 0) { pts[2 * i] = std::floor(pts[2 * i]); pts[2 * i + 1] = std::floor(pts[2 * i + 1]); }
            if (i % 9 == 0) pts[2 * i] = std::floor(pts[2 * i]) + 1.0f / 32768.0f;
        }
        // the window origin exactly at -win and at cols - 1 / rows - 1, and one pixel beyond
        const float edge[8][2] = {{-fp.winWidth + hx, h * 0.5f}, {-fp.winWidth + hx - 1.0f, h * 0.5f}, {w - 1 + hx, h * 0.5f}, {w + hx, h * 0.5f},
                                  {w * 0.5f, -fp.winHeight + hy}, {w * 0.5f, -fp.winHeight + hy - 1.0f}, {w * 0.5f, h - 1 + hy}, {w * 0.5f, h + hy}};
        for (int k = 0; k < 8; ++k) { pts[2 * (40 + k)] = edge[k][0]; pts[2 * (40 + k) + 1] = edge[k][1]; }
        for (int i = 0; i < n; ++i) {
            start[2 * i] = pts[2 * i] - sx + (float)uni(-1.5, 1.5); start[2 * i + 1] = pts[2 * i + 1] - sy + (float)uni(-1.5, 1.5);
            if (i % 7 == 3) { start[2 * i] = (float)uni(-60.0, w + 60.0); start[2 * i + 1] = (float)uni(-60.0, h + 60.0); }
            if (i % 10 == 1) { start[2 * i] = (float)w; start[2 * i + 1] = 0.0f; }                       // on the keep bounds
        }
        const bool useInitial = round % 3 == 1;
        const int wild = round % 17 == 3 ? 1 : (round % 17 == 9 ? 2 : 0);      // 1: refused, 2: served as the device entry serves it
        if (wild) {
            pts[6] = std::numeric_limits<float>::quiet_NaN(); pts[9] = std::numeric_limits<float>::infinity(); pts[20] = 1e20f;
            start[30] = -std::numeric_limits<float>::infinity(); start[33] = 3e9f;
        }
        ++pairs;
        std::vector<float> track((size_t)n * 2, -1.0f), err((size_t)n, -1.0f);
        std::vector<unsigned char> status((size_t)n, 9);
        std::vector<int> kept(1, 12345);
        const float* ini = useInitial ? start.data() : nullptr;
        const bool ok = flow_track_cpu(ga, gb, maxLevel, pts.data(), ini, n, fp, wild == 2, track.data(), status.data(), err.data(), kept);
        if (wild == 1) {
            if (ok || status[0] != 9 || track[0] != -1.0f || kept.size() != 1) { std::printf("round %d: wild corners not refused\n", round); return 1; }
            ++refused;
            continue;
        }
        if (!ok) { std::printf("round %d: refused\n", round); return 1; }
        size_t k = 0;
        for (int i = 0; i < n; ++i) {
            ++corners;
            const float x = track[2 * i], y = track[2 * i + 1];
            const bool can = convertible(pts[2 * i]) && convertible(pts[2 * i + 1]) && (!useInitial || (convertible(start[2 * i]) && convertible(start[2 * i + 1])));
            if (!can && (status[i] != 0 || !std::isnan(x) || !std::isnan(y) || err[i] != 0.0f)) { std::printf("round %d corner %d: an untrackable corner served\n", round, i); return 1; }
            if (status[i] > 1) { std::printf("round %d corner %d: status %d\n", round, i, status[i]); return 1; }
            if (fp.iterations == 0 && status[i]) {
                const float wx = useInitial ? start[2 * i] : pts[2 * i], wy = useInitial ? start[2 * i + 1] : pts[2 * i + 1];
                if (maxLevel == 0 && (!sameBits(x, wx) || !sameBits(y, wy))) { std::printf("round %d corner %d moved without an iteration\n", round, i); return 1; }
            }
            const bool want = status[i] && std::isfinite(x) && !(x < 0.0f) && !(x >= (float)w) && std::isfinite(y) && !(y < 0.0f) && !(y >= (float)h) &&
                              (fp.useMinEigenVals || err[i] < fp.errorThreshold);
            const bool got = k < kept.size() && kept[k] == i;
            if (want != got) { std::printf("round %d corner %d (%g, %g) -> (%.9g, %.9g) status %d err %g: kept %d / %d\n", round, i, pts[2 * i], pts[2 * i + 1], x, y, status[i], err[i], got, want); return 1; }
            if (got) ++k;
            tracked += status[i];
        }
        if (k != kept.size()) { std::printf("round %d: %zu kept entries not accounted for\n", round, kept.size() - k); return 1; }
        keptAll += (long)kept.size();
        // a second run, without the optional outputs, keeps the same corners
        std::vector<int> again;
        if (!flow_track_cpu(ga, gb, maxLevel, pts.data(), ini, n, fp, wild == 2, nullptr, nullptr, nullptr, again) || again != kept) { std::printf("round %d: the second run differs\n", round); return 1; }
    }
    // what the engine refuses
    {
        std::vector<unsigned char> img(40 * 24, 90);
        const GrayImage g{img.data(), 40, 40, 24};
        const float pt[2] = {20.0f, 12.0f};
        std::vector<int> kept;
        FlowParams bad[5];
        bad[0].winWidth = 2; bad[1].winHeight = 32; bad[2].winWidth = 40; bad[3].eps = std::numeric_limits<double>::quiet_NaN();
        bad[4].errorThreshold = std::numeric_limits<float>::quiet_NaN();
        for (const FlowParams& p : bad)
            if (flow_track_cpu(g, g, 3, pt, nullptr, 1, p, false, nullptr, nullptr, nullptr, kept)) { std::printf("a bad parameter served\n"); return 1; }
        FlowParams p;
        p.winWidth = p.winHeight = 5;
        if (flow_track_cpu(g, g, 9, pt, nullptr, 1, p, false, nullptr, nullptr, nullptr, kept) || flow_track_cpu(g, g, -1, pt, nullptr, 1, p, false, nullptr, nullptr, nullptr, kept)) return 1;
        const GrayImage narrow{img.data(), 39, 40, 24};
        if (flow_track_cpu(narrow, g, 3, pt, nullptr, 1, p, false, nullptr, nullptr, nullptr, kept)) { std::printf("a pitch below the row served\n"); return 1; }
        if (!flow_track_cpu(g, g, 3, pt, nullptr, 0, p, false, nullptr, nullptr, nullptr, kept) || !kept.empty()) return 1;
        refused += 8;
    }
    std::printf("ok: %ld image pairs, %ld corners (%ld tracked, %ld kept), %ld calls refused as the rule asks\n", pairs, corners, tracked, keptAll, refused);
    return keptAll > 1000 && tracked > keptAll ? 0 : 1;
}
