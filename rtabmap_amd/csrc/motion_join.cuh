// motion_join.cuh -- the unique-id join of two frames for motion_3d.hip, motion_pnp.hip and motion_ba.hip: both frames' 64-bit keys (id || row) sorted in LDS
// (compact_body.cuh's network), and the lookup of one side's sorted position in the other.  join_lookup's one caller is motion_group.cuh's join_compact,
// which walks a side and compacts the survivors; join_find_unique is motion_ba.hip's, which looks a list of ids up in both frames.  Device code only.  Internal.
#pragma once
#include "compact_body.cuh"
#include "motion_rule_common.h"

namespace lcd {

// keys[padded(0 .. p2 - 1)] = (id_key || row) of the frame's n rows, ascending, p2 the power of two >= max(n, 2), the tail all ones; ends
// behind a barrier
__device__ __forceinline__ void join_sort_keys(uint64_t* keys, const int32_t* ids, int n) {
    int p2 = 2;
    while (p2 < n) p2 <<= 1;
    for (int i = threadIdx.x; i < p2; i += blockDim.x) keys[padded(i)] = i < n ? ((uint64_t)m3d::id_key(ids[i]) << 32) | (uint32_t)i : ~0ull;
    __syncthreads();
    bitonic_sort(keys, p2);
}

// Position p (< na) of side A's sorted keys: true iff its id occurs once in A and exactly once in B (uMultimapToMapUnique on both sides, then
// the map lookup).  idk: the id's key; row_a, row_b: the rows in their frames.
__device__ __forceinline__ bool join_lookup(const uint64_t* keys_a, int na, const uint64_t* keys_b, int nb, int p, uint32_t& idk, uint32_t& row_a,
                                            uint32_t& row_b) {
    const uint64_t key = keys_a[padded(p)];
    idk = (uint32_t)(key >> 32);
    row_a = (uint32_t)key;
    row_b = 0;
    const bool unique = (p == 0 || (uint32_t)(keys_a[padded(p - 1)] >> 32) != idk) && (p + 1 >= na || (uint32_t)(keys_a[padded(p + 1)] >> 32) != idk);
    int lo = 0, hi = nb;                                               // the first B-key whose id is not below
    while (unique && lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((uint32_t)(keys_b[padded(mid)] >> 32) < idk) lo = mid + 1; else hi = mid;
    }
    if (!unique || lo >= nb) return false;
    const uint64_t bk = keys_b[padded(lo)];
    row_b = (uint32_t)bk;
    return (uint32_t)(bk >> 32) == idk && (lo + 1 >= nb || (uint32_t)(keys_b[padded(lo + 1)] >> 32) != idk);
}

// The row of the id with key idk among a frame's n sorted keys; false unless the id occurs exactly once (motion_ba.hip looks up a list of ids
// in both frames)
__device__ __forceinline__ bool join_find_unique(const uint64_t* keys, int n, uint32_t idk, uint32_t& row) {
    int lo = 0, hi = n;                                                // the first key whose id is not below
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((uint32_t)(keys[padded(mid)] >> 32) < idk) lo = mid + 1; else hi = mid;
    }
    row = 0;
    if (lo >= n) return false;
    const uint64_t k = keys[padded(lo)];
    row = (uint32_t)k;
    return (uint32_t)(k >> 32) == idk && (lo + 1 >= n || (uint32_t)(keys[padded(lo + 1)] >> 32) != idk);
}

}  // namespace lcd
