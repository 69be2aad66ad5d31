// dist_ref.cuh -- the reference's two distance functions, bit for bit (squared L2: rtflann L2 functor, dist.h:150-177, every product and sum
// individually rounded; Hamming: popcount(a ^ b), dist.h:555-579); shared by the exact scans and the same-frame distance kernels
// (knn2_kernels.hip), the pair matcher's distance blocks (pair_match.hip) and the guided matcher's candidates (guided_match.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lcd {
namespace {

// rtflann::L2<float>::operator() (dist.h:150-177), a = vocabulary row (wave-uniform), b = the lane's query
template <int DIM>
__device__ __forceinline__ float l2_ref(const float* __restrict__ row, const float (&q)[DIM]) {
    float res = 0.0f;
#pragma unroll
    for (int g = 0; g + 3 < DIM; g += 4) {
        const float d0 = __fsub_rn(row[g + 0], q[g + 0]);
        const float d1 = __fsub_rn(row[g + 1], q[g + 1]);
        const float d2 = __fsub_rn(row[g + 2], q[g + 2]);
        const float d3 = __fsub_rn(row[g + 3], q[g + 3]);
        float t = __fmul_rn(d0, d0);
        t = __fadd_rn(t, __fmul_rn(d1, d1));
        t = __fadd_rn(t, __fmul_rn(d2, d2));
        t = __fadd_rn(t, __fmul_rn(d3, d3));
        res = __fadd_rn(res, t);
    }
#pragma unroll
    for (int g = DIM & ~3; g < DIM; ++g) {
        const float d0 = __fsub_rn(row[g], q[g]);
        res = __fadd_rn(res, __fmul_rn(d0, d0));
    }
    return res;
}
// any dimension: the query is re-read from memory (L1-resident) -- correctness path for unusual descriptor sizes
__device__ __forceinline__ float l2_ref_dyn(const float* __restrict__ row, const float* __restrict__ q, int dim) {
    float res = 0.0f;
    int g = 0;
    for (; g + 3 < dim; g += 4) {
        const float d0 = __fsub_rn(row[g + 0], q[g + 0]);
        const float d1 = __fsub_rn(row[g + 1], q[g + 1]);
        const float d2 = __fsub_rn(row[g + 2], q[g + 2]);
        const float d3 = __fsub_rn(row[g + 3], q[g + 3]);
        float t = __fmul_rn(d0, d0);
        t = __fadd_rn(t, __fmul_rn(d1, d1));
        t = __fadd_rn(t, __fmul_rn(d2, d2));
        t = __fadd_rn(t, __fmul_rn(d3, d3));
        res = __fadd_rn(res, t);
    }
    for (; g < dim; ++g) {
        const float d0 = __fsub_rn(row[g], q[g]);
        res = __fadd_rn(res, __fmul_rn(d0, d0));
    }
    return res;
}

template <int W>
__device__ __forceinline__ uint32_t hamming_ref(const uint32_t* __restrict__ row, const uint32_t (&q)[W]) {
    uint32_t d = 0;
    // The bit counts of a row accumulate in the instruction itself (v_bcnt_u32_b32 d, x, d = popcount(x) + d), one chain per row.  Left
    // to the compiler the eight counts of a 256-bit row are summed as a tree -- eight v_bcnt_u32_b32 + three v_add3_u32
    // (tools/isa_loop_histogram.py: 94 VALU per trip of four rows, 82 this way; SURVEY.md 8d counts 16 per row: 8 xor + 8 counts); the
    // four rows of a trip keep four chains in flight.  An integer sum: the same number in any order.  Measured (round 5, same box,
    // 200 000 words x 500 descriptors): scan 77.6 -> 67.3 us, -13 % (profiles/r05_first_call.txt).
#pragma unroll
    for (int w = 0; w < W; ++w) {
        const uint32_t x = row[w] ^ q[w];
        asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(d) : "v"(x), "v"(d));
    }
    return d;
}
__device__ __forceinline__ uint32_t hamming_dyn(const uint32_t* __restrict__ row, const uint32_t* __restrict__ q, int w32) {
    uint32_t d = 0;
    for (int w = 0; w < w32; ++w) d += __popc(row[w] ^ q[w]);
    return d;
}

}  // namespace
}  // namespace lcd
