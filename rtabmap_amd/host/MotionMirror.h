// MotionMirror.h -- what the host mirrors of the motion rules (Motion3D.cpp, Motion2D.cpp) share: the unique-id rows of a frame, the backend's
// current model and two index sets with the selection into them, and the loop that scores the candidates.  Each CpuBackend derives from
// MirrorState and adds its rule, as the kernels' GroupBackend does from csrc/motion_group.cuh's Group.
#pragma once
#include <cstdint>
#include <map>
#include <utility>
#include <vector>

namespace rtabmap_amd {

// uMultimapToMapUnique (UStl.h:503-516): the rows whose id occurs once in their frame, by id
inline std::map<int32_t, int> uniqueRows(const int32_t* ids, int n) {
    std::map<int32_t, std::pair<int, int> > seen;                      // id -> (occurrences, row)
    for (int r = 0; r < n; ++r) { std::pair<int, int>& s = seen[ids[r]]; ++s.first; s.second = r; }
    std::map<int32_t, int> rows;
    for (const auto& s : seen) if (s.second.first == 1) rows[s.first] = s.second.second;
    return rows;
}

// what rule::solve and rule::refine ask of either backend about the model and the sets
struct MirrorState {
    float cur[12];
    std::vector<int> prev, next;

    // next = the i < m for which eval(i, value) holds, ascending, and their values beside them; returns their number
    template <class Eval>
    int select(int m, std::vector<float>& values, Eval eval) {
        next.clear();
        values.clear();
        for (int i = 0; i < m; ++i) { float v; if (eval(i, v)) { next.push_back(i); values.push_back(v); } }
        return (int)next.size();
    }
    void swap_sets() { prev.swap(next); }
    void clear_next() { next.clear(); }
    int prev_n() const { return (int)prev.size(); }
    int next_n() const { return (int)next.size(); }
    bool same_members() const { return prev == next; }
    const float* model() const { return cur; }
};

// Candidates 0 .. n_cand - 1 in turn: make(c, model) -> bool, its score the number of i < m with inlier(model, i); the best is the largest
// (count << 32 | ~c), so the earliest of the highest count.  Its model is made again into cur.  Returns the key, 0 when no candidate has an inlier.
template <class Make, class Inlier>
uint64_t bestCandidate(int n_cand, int m, float cur[12], Make make, Inlier inlier) {
    uint64_t best = 0;
    for (int c = 0; c < n_cand; ++c) {
        float model[12];
        if (!make(c, model)) continue;
        uint32_t count = 0;
        for (int i = 0; i < m; ++i) count += inlier(model, i) ? 1u : 0u;
        const uint64_t key = ((uint64_t)count << 32) | (uint32_t)~(uint32_t)c;
        if (count > 0 && key > best) best = key;
    }
    if (best) (void)make((int)~(uint32_t)best, cur);
    return best;
}

}  // namespace rtabmap_amd
