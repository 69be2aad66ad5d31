// top2_keys.cuh -- the two smallest 64-bit keys ((distance bits << 32) | row: a tie goes to the lower row) of a lane and of a wave; shared by
// the exact scans (knn2_kernels.hip), the exact redo (rowpar_body.cuh) and the re-rank (rerank_body.cuh).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lcd {
namespace {

__device__ __forceinline__ void top2_push(uint64_t& best, uint64_t& second, uint64_t k) {
    const uint64_t hi = best > k ? best : k;
    best = best < k ? best : k;
    second = second < hi ? second : hi;
}
__device__ __forceinline__ uint64_t shfl_xor_u64(uint64_t v, int m) {
    uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
    lo = __shfl_xor(lo, m, 64);
    hi = __shfl_xor(hi, m, 64);
    return ((uint64_t)hi << 32) | lo;
}
// 6-step butterfly: afterwards EVERY lane of the wave holds the wave's two smallest keys
__device__ __forceinline__ void wave_top2_reduce(uint64_t& best, uint64_t& second) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const uint64_t ob = shfl_xor_u64(best, m), os = shfl_xor_u64(second, m);
        top2_push(best, second, ob);
        top2_push(best, second, os);
    }
}

}  // namespace
}  // namespace lcd
