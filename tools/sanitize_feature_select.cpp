// sanitize_feature_select.cpp -- FeatureSelect's three functions (plain host code: the selection and expansion rule of lcd_select_features /
// lcd_expand_word_ids) driven from a stand-alone program, for a host-only AddressSanitizer / UndefinedBehaviorSanitizer run.  No engine is
// created and nothing touches a GPU.
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Irtabmap_amd/host \
//       tools/sanitize_feature_select.cpp rtabmap_amd/host/FeatureSelect.cpp -o feature_select_asan
//   ./feature_select_asan
//
// Random frames with every kind of entry the functions guard against (ties, both signs, both zeros, denormals, infinities, NaN, keypoints
// on cell edges, below zero, in the remainder strip and far outside, images not larger than the grid, indices and counts out of range,
// ids of every kind including INT_MIN) against a restatement with std::multimap; exit status 0 and "ok" when all agree.
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <map>
#include <random>
#include <vector>

#include "FeatureSelect.h"

using rtabmap_amd::FeatureSelect;

// the `keep` strongest of `members` by the reverse walk of a multimap over fabs(response); all of them when keep <= 0 or nothing is cut
static void walk(const std::vector<float>& r, const std::vector<int>& members, int keep, std::vector<int>& out) {
    if (keep <= 0 || (int)members.size() <= keep) { out.insert(out.end(), members.begin(), members.end()); return; }
    std::multimap<float, int> byResponse;
    for (int i : members) byResponse.insert(std::pair<float, int>(std::fabs(r[(size_t)i]), i));
    int k = 0;
    for (std::multimap<float, int>::reverse_iterator it = byResponse.rbegin(); it != byResponse.rend() && k < keep; ++it, ++k) out.push_back(it->second);
}

int main() {
    std::mt19937 rng(11);
    auto upto = [&](int n) { return n <= 0 ? 0 : (int)(rng() % (unsigned)n); };
    const float pool[] = {0.0f, -0.0f, 1e-45f, -1e-45f, 0.5f, -0.5f, 1.0f, 1.0f, -1.0f, 7.25f, std::numeric_limits<float>::infinity(), -3e38f};
    long checked = 0;
    for (int it = 0; it < 20000; ++it) {
        const int n = upto(40);
        const int maxKeypoints = upto(n + 6) - 2;
        const int gridRows = 1 + upto(4), gridCols = 1 + upto(4);
        const int width = it % 17 == 0 ? gridCols : 97 + upto(40), height = it % 19 == 0 ? gridRows - 1 : 61 + upto(40);
        std::vector<float> r((size_t)n), p((size_t)2 * n);
        for (float& v : r) v = pool[upto(12)];
        const bool withNaN = it % 7 == 0 && n > 0;
        if (withNaN) r[(size_t)upto(n)] = std::numeric_limits<float>::quiet_NaN();
        const int wild = it % 3 == 0 ? 8 : 0;                                   // one point in eight may leave the grid
        for (int i = 0; i < n; ++i) {
            p[(size_t)2 * i] = (float)upto(width > 0 ? width : 1) + (float)upto(4) * 0.25f;
            p[(size_t)2 * i + 1] = (float)upto(height > 0 ? height : 1) + (float)upto(4) * 0.25f;
            if (wild && upto(wild) == 0) {
                const float odd[] = {-0.5f, -1.5f, -1000.0f, 1e20f, -1e20f, std::numeric_limits<float>::quiet_NaN(), (float)width, (float)height};
                p[(size_t)2 * i + upto(2)] = odd[upto(8)];
            }
        }
        // ---- the inlier mask
        std::vector<bool> inliers(3, true);
        const bool ok = FeatureSelect::limitKeypoints(r.data(), p.data(), n, maxKeypoints, width, height, gridRows, gridCols, inliers);
        bool expectOk = !withNaN;
        std::vector<int> kept;
        const bool cut = maxKeypoints > 0 && n > maxKeypoints;
        std::vector<int> everything((size_t)n);
        for (int i = 0; i < n; ++i) everything[(size_t)i] = i;
        if (expectOk && !cut) kept = everything;
        else if (expectOk && gridRows * gridCols == 1) walk(r, everything, maxKeypoints, kept);
        else if (expectOk) {
            if (height <= gridRows || width <= gridCols) expectOk = false;
            else {
                const int rowSize = height / gridRows, colSize = width / gridCols;
                std::vector<std::vector<int> > cells((size_t)(gridRows * gridCols));
                for (int i = 0; i < n && expectOk; ++i) {
                    const int cellRow = FeatureSelect::toInt(p[(size_t)2 * i + 1]) / rowSize, cellCol = FeatureSelect::toInt(p[(size_t)2 * i]) / colSize;
                    if (cellRow < 0 || cellRow >= gridRows || cellCol < 0 || cellCol >= gridCols) expectOk = false;
                    else cells[(size_t)(cellRow * gridCols + cellCol)].push_back(i);
                }
                for (size_t c = 0; c < cells.size() && expectOk; ++c) walk(r, cells[c], maxKeypoints / (gridRows * gridCols), kept);
            }
        }
        std::vector<bool> expected((size_t)n, false);
        for (int i : kept) expected[(size_t)i] = true;
        if (ok != expectOk || (ok && inliers != expected) || (!ok && inliers != std::vector<bool>(3, true))) {
            std::fprintf(stderr, "limitKeypoints (mask): mismatch at iteration %d\n", it);
            return 1;
        }
        // ---- the compacting form
        std::vector<int> order(2, -5), expectedOrder;
        const bool ok2 = FeatureSelect::limitKeypoints(r.data(), n, maxKeypoints, order);
        if (cut) walk(r, everything, maxKeypoints, expectedOrder); else expectedOrder = everything;
        if (ok2 != !withNaN || (ok2 && order != expectedOrder) || (!ok2 && order != std::vector<int>(2, -5))) {
            std::fprintf(stderr, "limitKeypoints (compacting): mismatch at iteration %d\n", it);
            return 1;
        }
        // ---- the expansion
        const int count = upto(n + 3) - 1;                                      // -1 and n + 1: out of range
        std::vector<int> index, ids;
        bool inRange = count >= 0 && count <= n;
        for (int j = 0; j < count; ++j) {
            index.push_back(it % 5 == 0 ? upto(n + 2) - 1 : upto(n > 0 ? n : 1));
            const int kinds[] = {1 + upto(9000), -(1 + upto(30)), 0, INT_MIN, INT_MAX};
            ids.push_back(kinds[upto(5)]);
        }
        for (int j = 0; j < count && j < (int)index.size(); ++j) if (index[(size_t)j] < 0 || index[(size_t)j] >= n) inRange = false;
        const int first = it % 2 ? 0 : (it % 4 ? 500 : INT_MAX - 3);
        std::vector<int> all(1, 42);
        const bool ok3 = FeatureSelect::expandWordIds(n, index.data(), ids.data(), count, first, all);
        std::vector<long long> resolved((size_t)n, 0);
        for (int j = 0; j < count && inRange; ++j) {
            const long long w = ids[(size_t)j];
            long long id = w;
            if (w < 0) {
                id = 0;
                if (first > 0) {
                    id = (long long)first + (-(w + 1));
                    if (id > INT_MAX) id -= 4294967296ll;                       // the 32-bit sum wraps: not a word id
                }
            }
            if (id > 0) resolved[(size_t)index[(size_t)j]] = id;
        }
        std::vector<int> expectedAll;
        int neg = -1;
        for (int i = 0; i < n; ++i) expectedAll.push_back(resolved[(size_t)i] > 0 ? (int)resolved[(size_t)i] : neg--);
        if (ok3 != inRange || (ok3 && all != expectedAll) || (!ok3 && all != std::vector<int>(1, 42))) {
            std::fprintf(stderr, "expandWordIds: mismatch at iteration %d\n", it);
            return 1;
        }
        checked += n;
    }
    std::printf("ok: 20000 cases, %ld features\n", checked);
    return 0;
}
