// sanitize_guided_word_ids.cpp -- VWDictionaryHip::guidedWordIds (plain host code: the id bookkeeping behind lcd_match_guided) driven from a
// stand-alone program, for a host-only AddressSanitizer / UndefinedBehaviorSanitizer run.  No engine is created and nothing touches a GPU.
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Irtabmap_amd/host -Iinclude \
//       tools/sanitize_guided_word_ids.cpp rtabmap_amd/host/VWDictionaryHip.cpp -Lrtabmap_amd -llcd_hip -ldl -Wl,-rpath,$PWD/rtabmap_amd -o guided_ids_asan
//   ./guided_ids_asan
//
// Random inputs with every kind of entry the function guards against (corner indices and from-rows out of range, no corners, no rows, with
// and without original ids, a count array or none) against a restatement with std::map; exit status 0 and "ok" when all agree.
#include <cstdio>
#include <cstdlib>
#include <list>
#include <map>
#include <random>
#include <vector>

#include "VWDictionaryHip.h"

using rtabmap_amd::VWDictionaryHip;

int main() {
    std::mt19937 rng(7);
    auto upto = [&](int n) { return n <= 0 ? 0 : (int)(rng() % (unsigned)n); };
    long checked = 0;
    for (int it = 0; it < 20000; ++it) {
        const int rowsFrom = upto(12), rowsTo = upto(14);
        const int nCorners = upto(rowsFrom + 3);
        std::vector<int> orig;
        if (it % 2) for (int i = 0; i < rowsFrom; ++i) orig.push_back(3 + 5 * i + upto(3));
        std::vector<int> cornerRows((size_t)nCorners);
        for (int& r : cornerRows) r = upto(rowsFrom + 2) - 1;                    // -1 and rowsFrom: out of range
        std::vector<int32_t> toCorner((size_t)rowsTo), count((size_t)nCorners);
        for (int32_t& c : toCorner) c = upto(nCorners + 3) - 2;                  // -2, -1 and nCorners: out of range
        for (int32_t& c : count) c = upto(3);
        const bool withCount = it % 3 != 0;
        std::list<int> f, t, p;
        VWDictionaryHip::guidedWordIds(rowsFrom, orig, cornerRows, rowsTo ? toCorner.data() : nullptr, rowsTo, withCount ? count.data() : nullptr, f, t,
                                       it % 5 ? &p : nullptr);
        // the reference's bookkeeping, restated (:1104, :1158, :1189, :1257, :1308, :1349-1361)
        std::map<int, int> idOfRow;
        int newToId = rowsFrom;
        for (int i = 0; i < rowsFrom; ++i) idOfRow[i] = orig.empty() ? i : orig[(size_t)i];
        if (!orig.empty()) { newToId = 0; for (int v : orig) newToId = v > newToId ? v : newToId; newToId += 1; }
        std::vector<int> ef, et, ep;
        for (int i = 0; i < rowsFrom; ++i) ef.push_back(idOfRow[i]);
        for (int i = 0; i < rowsTo; ++i) {
            const int c = toCorner[(size_t)i];
            const int row = c >= 0 && c < nCorners ? cornerRows[(size_t)c] : -1;
            if (idOfRow.count(row)) et.push_back(idOfRow[row]); else et.push_back(newToId++);
        }
        if (withCount && it % 5)
            for (int c = 0; c < nCorners; ++c) if (count[(size_t)c] > 0 && idOfRow.count(cornerRows[(size_t)c])) ep.push_back(idOfRow[cornerRows[(size_t)c]]);
        if (std::vector<int>(f.begin(), f.end()) != ef || std::vector<int>(t.begin(), t.end()) != et || std::vector<int>(p.begin(), p.end()) != ep) {
            std::fprintf(stderr, "mismatch at iteration %d\n", it);
            return 1;
        }
        checked += rowsFrom + rowsTo + nCorners;
    }
    std::printf("ok: 20000 cases, %ld entries\n", checked);
    return 0;
}
