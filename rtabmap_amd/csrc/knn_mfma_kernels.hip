// knn_mfma_kernels.hip -- squared-L2 2-NN as a dense contraction on the matrix cores, with an exactness certificate.
//
// The reference's arithmetic, sum_k (v_k - q_k)^2 in rtflann's order (dist.h:150-177), costs 3 VALU ops per element and
// cannot use FMA.  Here the scan is split in two:
//
//   1. FILTER (MFMA): s(i, j) = |v_i|^2 + |q_j|^2 - 2 v_i . q_j for every (vocabulary row i, query j).  |v|^2 and |q|^2 ride
//      along as one extra f32 k-step (A = (|v_i|^2, 1), B = (1, |q_j|^2)) and the queries are pre-scaled by -2, so the
//      accumulator IS the approximate squared distance.  Every lane keeps a running top-3 of 32-bit keys (score bits | in-strip
//      row index) for the queries it sees -- no cross-lane traffic in the loop.  Two variants:
//        knn_bf16_filter_kernel  (default)  three bf16 MFMA chains per product on a hi/lo split of the operands
//                                           (v_mfma_f32_32x32x16_bf16, 16x the f32 rate), one vocabulary tile shared by the
//                                           four waves of a workgroup; the same launch also computes the same-frame distance matrix
//        knn_mfma_filter_kernel             v_mfma_f32_32x32x2_f32 -- f32 in, f32 accumulate: an exact fp32 FMA chain
//   2. RE-RANK (knn_mfma_rerank_kernel): per query the few kept keys that can still be a neighbour (filter score within
//      2 eps of the second best) are re-evaluated with the reference's own arithmetic (bit-exact distances, lower row wins
//      ties) and the two best are returned.  The result is PROVEN equal to the exact scan when every row the filter dropped
//      is certainly farther than the exact second neighbour:
//            bound - eps > d2_exact,
//      bound = the smallest filter score any dropped row can have (tracked through every merge level), eps = a bound on
//      |filter score - reference distance| (eps_for() / eps_bf16()).  Queries that fail the certificate (near-duplicate
//      clusters) are re-done exactly by rowpar_body.cuh (one lane per vocabulary row, the whole chip on each rejected
//      query), so the output is always the reference's bit-exact answer.
//
// MFMA operand layout (both variants): lane (row or query l&31, half l>>5) holds the contiguous elements [32h, 32h+32) of its
// row, i.e. a k-step multiplies the same element subset on both sides -- A and B use the same k permutation, which a dot
// product does not see.  D layout: lane holds query (l&31), 16 rows (reg&3) + 8*(reg>>2) + 4*(l>>5).
#include <hip/hip_ext.h>
#include "lcd_kernels.h"
#include "rowpar_body.cuh"
#include "shard_body.cuh"
#include "frame_tail_body.cuh"
#include "score_body.cuh"

#include <algorithm>
#include <cstdlib>

namespace lcd {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
constexpr int MF_BLOCK = 256;
constexpr int MF_WAVES = 4;
constexpr int MF_KEEP = 4;     // keys kept per (row block, query)

// Augmentation table of the vocabulary: aug[2r] = |row r|^2 (any summation order: the filter only needs it to ~dim ulps;
// +inf for tombstones), aug[2r + 1] = 1, plus a sentinel entry {+inf, 1} at r = n_rows for the padding rows of the last
// tile.  The MFMA filter reads aug[2 * min(row, n_rows) + half] with ONE unconditional load per lane.
__global__ void row_norm_kernel(const float* __restrict__ vocab, const int32_t* __restrict__ row_id, int first, int n, int dim,
                                float* __restrict__ aug, uint32_t* __restrict__ norm_max_bits) {
    const int r = first + blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= first + n) return;
    float s = __int_as_float(0x7f800000);
    if (row_id[r] != 0) {
        s = 0.0f;
        const float* v = vocab + (size_t)r * dim;
        for (int k = 0; k < dim; ++k) s = fmaf(v[k], v[k], s);
        atomicMax(norm_max_bits, __float_as_uint(s));
    }
    aug[2 * (size_t)r] = s;
    aug[2 * (size_t)r + 1] = 1.0f;
    if (r == first + n - 1) { aug[2 * (size_t)(r + 1)] = __int_as_float(0x7f800000); aug[2 * (size_t)(r + 1) + 1] = 1.0f; }
}
__global__ void norm_tombstone_kernel(float* __restrict__ aug, const int32_t* __restrict__ rows, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) aug[2 * (size_t)rows[i]] = __int_as_float(0x7f800000);
}

// bf16 split of the vocabulary for the bf16x3 filter: row r -> 256 bytes = 64 bf16 "hi" (the float rounded to bf16, RNE) then
// 64 bf16 "lo" (the exact remainder float - hi, rounded to bf16).  hi + lo carries ~17 significant bits of the float.
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef float f32x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void bf16_split2(float a, float b, uint32_t& hi, uint32_t& lo) {
    hi = __builtin_bit_cast(uint32_t, __builtin_convertvector((f32x2_t){a, b}, bf16x2_t));      // v_cvt_pk_bf16_f32
    const float ra = __fsub_rn(a, __uint_as_float(hi << 16)), rb = __fsub_rn(b, __uint_as_float(hi & 0xFFFF0000u));   // exact
    lo = __builtin_bit_cast(uint32_t, __builtin_convertvector((f32x2_t){ra, rb}, bf16x2_t));
}
// The fp16 filter (LCD_KNN_F16, one product per fp32 product: the operand format north_star names for the SURF distance GEMM): the SAME
// table layout with IEEE half "hi" (RNE, 11 significant bits) and half "lo" (the remainder, unused by the one-product filter) -- the
// matrix pipe runs v_mfma_f32_32x32x16_f16 at the bf16 rate, a third of the products, an eps of ~2^-10 (|q|^2 + |v|^2) instead of ~2^-14.
typedef _Float16 f16x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void f16_split2(float a, float b, uint32_t& hi, uint32_t& lo) {
    const f16x2_t h = __builtin_convertvector((f32x2_t){a, b}, f16x2_t);                          // v_cvt_pkrtz would truncate: this rounds to nearest even
    hi = __builtin_bit_cast(uint32_t, h);
    const f32x2_t back = __builtin_convertvector(h, f32x2_t);
    lo = __builtin_bit_cast(uint32_t, __builtin_convertvector((f32x2_t){__fsub_rn(a, back.x), __fsub_rn(b, back.y)}, f16x2_t));
}
template <int M> __device__ __forceinline__ void op_split2(float a, float b, uint32_t& hi, uint32_t& lo) {
    if (M == 1) f16_split2(a, b, hi, lo); else bf16_split2(a, b, hi, lo);
}
__device__ __forceinline__ void op_split2_rt(int f16, float a, float b, uint32_t& hi, uint32_t& lo) {
    if (f16) f16_split2(a, b, hi, lo); else bf16_split2(a, b, hi, lo);
}
__global__ void vocab_bf16_kernel(const float* __restrict__ vocab, int first, int n, uint32_t* __restrict__ bf, int f16) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;          // one thread per 4 floats of a 64-float row
    if (i >= n * 16) return;
    const int r = first + (i >> 4), c = i & 15;
    const float4 x = reinterpret_cast<const float4*>(vocab + (size_t)r * 64)[c];
    uint2 hi, lo;
    op_split2_rt(f16, x.x, x.y, hi.x, lo.x);
    op_split2_rt(f16, x.z, x.w, hi.y, lo.y);
    reinterpret_cast<uint2*>(bf + (size_t)r * 64)[c] = hi;
    reinterpret_cast<uint2*>(bf + (size_t)r * 64 + 32)[c] = lo;
}

// rows [first, first + n) that hold no word yet (capacity behind the vocabulary, filled by the device-side append): |row|^2 = +inf so
// that no filter ever ranks them, a zero bf16 split so that the product with them is finite
__global__ void vocab_tail_kernel(float* __restrict__ aug, uint32_t* __restrict__ bf, long long first, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;          // one thread per 16 bytes of the 256-byte split row
    if (i >= n * 16) return;
    const long long r = first + (i >> 4);
    const int c = (int)(i & 15);
    reinterpret_cast<uint4*>(bf + r * 64)[c] = make_uint4(0u, 0u, 0u, 0u);
    if (c == 0) { aug[2 * r] = __int_as_float(0x7f800000); aug[2 * r + 1] = 1.0f; }
}

// ------------------------------------------------------------------------------------------------ filter
// In-loop candidate key: 32 bits = the score's float bits with the low MF_IDX_BITS mantissa bits replaced by the
// candidate's position inside the wave's strip (tile-in-strip << 4 | accumulator register).  Scores are >= 0, so the keys
// strip (tile-in-strip << 4 | accumulator register).  Keys are compared as SIGNED integers: non-negative floats order like
// their bit patterns, and a score that rounding pushed slightly below zero (an exact duplicate of the query) sorts first,
// which is where it belongs; a top-3 update is one v_min_i32 and two v_med3_i32.  Truncation only LOWERS a key
// (by < 2^-16 relative): a dropped row's true score is >= its key >= the bound derived from kept keys, so the
// certificate stays valid; at most MF_STRIP_TILES tiles per wave strip keep the index in 7 bits.
constexpr int MF_IDX_BITS = 7;
constexpr int MF_STRIP_TILES = 1 << (MF_IDX_BITS - 4);
constexpr uint32_t MF_IDX_MASK = (1u << MF_IDX_BITS) - 1;
constexpr int32_t MF_KEY_NONE = 0x7FFFFFFF;

// sorted insertion into k0 <= k1 <= k2 from the OLD values only (three independent VALU, no dependent chain):
//   k0' = min(k0, k), k1' = med3(k0, k1, k), k2' = med3(k1, k2, k)
__device__ __forceinline__ int32_t med3_i32(int32_t a, int32_t b, int32_t c) {
    int32_t r;
    asm("v_med3_i32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
__device__ __forceinline__ void top3_push32(int32_t& k0, int32_t& k1, int32_t& k2, int32_t k) {
    const int32_t n2 = med3_i32(k1, k2, k);
    const int32_t n1 = med3_i32(k0, k1, k);
    k0 = min(k0, k);
    k1 = n1;
    k2 = n2;
}
// strip key of accumulator register r of strip tile tl: the score bits with the index in the low mantissa bits -- one v_and_or_b32
// (the index is wave-uniform)
// (the index is wave-uniform; the mask is kept in a VGPR the compiler cannot see through, or it would pick v_and + v_or with
// a literal)
__device__ __forceinline__ uint32_t strip_mask() {
    uint32_t m;
    asm("v_mov_b32 %0, 0xffffff80" : "=v"(m));
    static_assert(MF_IDX_BITS == 7, "literal above");
    return m;
}
__device__ __forceinline__ int32_t strip_key(float score, uint32_t mask, uint32_t idx) {
    return (int32_t)((__float_as_uint(score) & mask) | idx);
}
// strip key -> merge key (score bits << 32 | vocabulary row); a slightly negative score (rounding of a distance ~ 0) becomes +0
__device__ __forceinline__ uint64_t widen_key(int32_t k, int t_begin, int half) {
    if (k == MF_KEY_NONE) return KEY_NONE;
    const uint32_t idx = (uint32_t)k & MF_IDX_MASK, r = idx & 15u;
    const uint32_t row = (uint32_t)(t_begin + (int)(idx >> 4)) * 32u + (r & 3u) + 8u * (r >> 2) + 4u * (uint32_t)half;
    const uint32_t bits = k < 0 ? 0u : ((uint32_t)k & ~MF_IDX_MASK);
    return ((uint64_t)bits << 32) | row;
}

// A tile = 32 vocabulary rows x DIM floats (8 KB for DIM = 64).  It goes global -> LDS with the asynchronous LDS-DMA
// (global_load_lds, 16 B per lane, no staging VGPRs, fully coalesced: every instruction moves 1 KiB = 8 whole 128-B lines),
// then LDS -> VGPRs in MFMA operand order (lane (row l&31, half l>>5) gets the contiguous floats [KH*half, KH*half + KH) of
// its row).  The DMA writes LDS linearly (wave-uniform base + 16 * lane), so the bank-conflict fix is an XOR swizzle applied
// to the SOURCE address and to the read address alike (cdna_hip_programming.md rule 21): 16-B chunk c of row r lives at
// chunk position c ^ (r & 15).  A per-lane gather straight from global memory (row stride 256 B across lanes) touches 64
// lines per load and thrashes the 32 KiB L1: it made the kernel load-bound.
template <int KH>
__device__ __forceinline__ void dma_a_tile(const float* __restrict__ vocab, int n_rows, int t, int lane, float* __restrict__ lds_slot) {
    constexpr int DIM = 2 * KH;
    constexpr int CPR = DIM / 4;                          // 16-B chunks per row
    static_assert(CPR == 16 || CPR == 32, "swizzle written for 64- or 128-float rows");
#pragma unroll
    for (int i = 0; i < (32 * CPR) / 64; ++i) {           // 8 instructions for DIM = 64
        const int p = i * 64 + lane;                      // linear chunk position in the LDS slot
        const int r = p / CPR, cpos = p % CPR;
        const int c = cpos ^ (r & 15);                    // the global chunk that belongs at this position
        const int row = min(t * 32 + r, n_rows - 1);      // padding rows repeat the last row (their score is forced to +inf)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(vocab + (size_t)row * DIM + c * 4),
                                         (__attribute__((address_space(3))) void*)(lds_slot + i * 256), 16, 0, 0);
    }
}
template <int KH>
__device__ __forceinline__ void read_a_tile(const float* __restrict__ lds_slot, int col, int half, float (&a)[KH]) {
    constexpr int DIM = 2 * KH;
    const float* rowp = lds_slot + col * DIM;
#pragma unroll
    for (int v = 0; v < KH / 4; ++v) {
        const int c = half * (KH / 4) + v;                // chunk of the row this lane needs
        const float4 x = *reinterpret_cast<const float4*>(rowp + ((c ^ (col & 15)) << 2));
        a[4 * v + 0] = x.x; a[4 * v + 1] = x.y; a[4 * v + 2] = x.z; a[4 * v + 3] = x.w;
    }
}

// one 32-row tile against one 32-query group: 33 MFMAs
template <int KH>
__device__ __forceinline__ f32x16 mfma_group(const float (&a)[KH], float a_aug, const float (&b)[KH], float b_aug) {
    f32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#if LCD_MFMA_ABLATE == 2
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = a[r] * b[r] + a_aug * b_aug;
    return acc;
#endif
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a_aug, b_aug, acc, 0, 0, 0);
#pragma unroll
    for (int k = 0; k < KH; ++k) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[k], b[k], acc, 0, 0, 0);
    return acc;
}
// one 32-row tile against TWO 32-query groups with the two accumulator chains interleaved k-step by k-step: consecutive
// MFMAs are independent, so the matrix pipe never waits for a dependent accumulator
template <int KH>
__device__ __forceinline__ void mfma_pair(const float (&a)[KH], float a_aug, const float (&b0)[KH], float b0_aug, const float (&b1)[KH],
                                          float b1_aug, f32x16& acc0, f32x16& acc1) {
    const f32x16 z = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a_aug, b0_aug, z, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a_aug, b1_aug, z, 0, 0, 0);
#pragma unroll
    for (int k = 0; k < KH; ++k) {
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[k], b0[k], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[k], b1[k], acc1, 0, 0, 0);
    }
}

// acc[r] = approximate squared distance between the lane's query and row t*32 + (r&3) + 8*(r>>2) + 4*half
#ifndef LCD_MFMA_ABLATE
#define LCD_MFMA_ABLATE 0      // 1: skip the top-3 update (timing experiment only), 2: skip the MFMAs
#endif
__device__ __forceinline__ void push_group(const f32x16& acc, uint32_t tl, int32_t& k0, int32_t& k1, int32_t& k2) {
#if LCD_MFMA_ABLATE == 1
    asm volatile("" :: "v"(acc[0]), "v"(acc[5]), "v"(acc[10]), "v"(acc[15]));
    k0 = min(k0, __float_as_int(acc[3])); (void)tl; (void)k1; (void)k2;
    return;
#endif
    const uint32_t base = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tl << 4));
    const uint32_t mask = strip_mask();
#pragma unroll
    for (int r = 0; r < 16; ++r) top3_push32(k0, k1, k2, strip_key(acc[r], mask, base | (uint32_t)r));
}

// The bf16 / fp16 filters select GROUPS: the four accumulator registers 4g .. 4g + 3 of a lane are four CONSECUTIVE vocabulary rows
// (t * 32 + 8 g + 4 half + {0, 1, 2, 3}); the lane keeps the three groups with the smallest minimum -- one key per group (the minimum's bits,
// the index of the group's FIRST register), 6 VALU per four scores (v_min3_f32, v_min_f32, v_and_or_b32, v_med3_i32 x 2, v_min_i32)
// instead of 16.  Complete for the re-rank, which evaluates all four rows of a kept group exactly: every row of the true top-3 lies in a
// group whose minimum is <= that row's score, and a group WITHOUT such a row has a minimum >= the third-best row's score -- so the
// three groups with the smallest minima contain the three best rows, and the bound on what was dropped (the third kept key) holds as
// before.  (The filter loop was issue-bound 2:1 on exactly this selection: 354 instructions per 32-row tile against 768 matrix-pipe
// cycles with one fp16 product per fp32 product)
__device__ __forceinline__ float min4(float a, float b, float c, float d) { return fminf(fminf(fminf(a, b), c), d); }
__device__ __forceinline__ void push_group4(const f32x16& acc, uint32_t tl, int32_t& k0, int32_t& k1, int32_t& k2) {
#if LCD_MFMA_ABLATE == 1
    asm volatile("" :: "v"(acc[0]), "v"(acc[5]), "v"(acc[10]), "v"(acc[15]));
    k0 = min(k0, __float_as_int(acc[3])); (void)tl; (void)k1; (void)k2;
    return;
#endif
    const uint32_t base = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tl << 4));
    const uint32_t mask = strip_mask();
#pragma unroll
    for (int g = 0; g < 4; ++g) top3_push32(k0, k1, k2, strip_key(min4(acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]), mask, base | (uint32_t)(4 * g)));
}

// One software-pipeline step in explicit program order: the 66 MFMAs of a group pair (two interleaved accumulator chains)
// with the top-3 update of the PREVIOUS pair's 32 scores spread between them -- 4 MFMAs, then the update of one score of
// each pending accumulator (~14 VALU), sixteen times.  A wave issues in order and the compiler otherwise emits the MFMAs
// back to back and the VALU afterwards (measured: MFMA-busy 57 % of the wave cycles, VALU time additive), so the order is
// pinned with sched_barrier(0): the VALU then issues in the shadow of the 64-cycle MFMAs.
template <int KH>
__device__ __forceinline__ void mfma_pair_push(const float (&a)[KH], float a_aug, const float (&b0)[KH], float b0_aug, const float (&b1)[KH],
                                               float b1_aug, f32x16& c0, f32x16& c1, const f32x16& p0, const f32x16& p1, uint32_t tl,
                                               int32_t& k00, int32_t& k01, int32_t& k02, int32_t& k10, int32_t& k11, int32_t& k12) {
    static_assert(KH == 32, "interleave pattern written for 64-float rows");
    const f32x16 z = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    const uint32_t base = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tl << 4));
    const uint32_t mask = strip_mask();
    c0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a_aug, b0_aug, z, 0, 0, 0);
    c1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a_aug, b1_aug, z, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        c0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[2 * r], b0[2 * r], c0, 0, 0, 0);
        c1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[2 * r], b1[2 * r], c1, 0, 0, 0);
        c0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[2 * r + 1], b0[2 * r + 1], c0, 0, 0, 0);
        c1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[2 * r + 1], b1[2 * r + 1], c1, 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        top3_push32(k00, k01, k02, strip_key(p0[r], mask, base | (uint32_t)r));
        top3_push32(k10, k11, k12, strip_key(p1[r], mask, base | (uint32_t)r));
        __builtin_amdgcn_sched_barrier(0);
    }
}

// partial_keys [qpad][n_blocks][MF_KEEP] u64, partial_lmin [qpad][n_blocks] f32 bits (query-major: the re-rank wave of a query
// reads one contiguous run).
// MF_NG = 32-query column groups per wave (wave tile = MF_NG*32 queries x 32 rows): ONE wave per SIMD with four independent
// accumulator chains (A tiles reused 4x, the VALU top-3 update of one accumulator issues under the MFMAs of the next; two
// groups and two waves per SIMD measured the same).
constexpr int MF_NG = 4;
#ifdef LCD_MFMA_TIMING   // timing experiment only: per-wave timestamps (100 MHz) at kernel entry, loop entry, loop exit, kernel exit
__device__ unsigned long long g_mf_timing[4 * 4096];
#define MF_STAMP(i) do { if (lane == 0) g_mf_timing[4 * (((blockIdx.y * gridDim.x + blockIdx.x) & 1023) * MF_WAVES + wave) + (i)] = __builtin_amdgcn_s_memrealtime(); } while (0)
__device__ unsigned long long g_mf_timing2[8 * 4096];   // finer stamps inside one loop trip of the bf16 filter
#define MF_STAMP2(i) do { if (lane == 0 && (i) < 8) { g_mf_timing2[8 * (((blockIdx.y * gridDim.x + blockIdx.x) & 1023) * MF_WAVES + wave) + (i)] = __builtin_amdgcn_s_memrealtime(); } } while (0)
#else
#define MF_STAMP(i) do { } while (0)
#define MF_STAMP2(i) do { } while (0)
#endif

template <int DIM>
__global__ __launch_bounds__(MF_BLOCK, 1) void knn_mfma_filter_kernel(const float* __restrict__ vocab, const float* __restrict__ row_norm, int n_rows,
                                                                     const float* __restrict__ queries, int nq, int qpad, int tiles_per_block,
                                                                     uint64_t* __restrict__ partial_keys, uint32_t* __restrict__ partial_lmin) {
    constexpr int NG = MF_NG;
    constexpr int KH = DIM / 2;                    // floats of a row held by one lane
    constexpr int QW = NG * 32;                    // queries per wave / workgroup
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int col = lane & 31, half = lane >> 5;
    const int q0 = blockIdx.y * QW;
    MF_STAMP(0);

    // B operand: the NG 32-query groups, pre-scaled by -2 (exact), + |q|^2 for the extra k-step
    float b[NG][KH];
    float b_aug[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        const int qi = min(q0 + g * 32 + col, nq - 1);
        const float4* src = reinterpret_cast<const float4*>(queries + (size_t)qi * DIM + half * KH);
        float part = 0.0f;
#pragma unroll
        for (int v = 0; v < KH / 4; ++v) {
            const float4 x = src[v];
            b[g][4 * v + 0] = -2.0f * x.x; b[g][4 * v + 1] = -2.0f * x.y; b[g][4 * v + 2] = -2.0f * x.z; b[g][4 * v + 3] = -2.0f * x.w;
            part = fmaf(x.x, x.x, part); part = fmaf(x.y, x.y, part); part = fmaf(x.z, x.z, part); part = fmaf(x.w, x.w, part);
        }
        const float qn = part + __shfl_xor(part, 32, 64);          // both halves of the row
        b_aug[g] = half == 0 ? 1.0f : qn;                          // B[k0][j] = 1, B[k1][j] = |q_j|^2
    }

    const int tile0 = blockIdx.x * tiles_per_block;
    const int n_tiles = (n_rows + 31) / 32;
    const int tile1 = min(tile0 + tiles_per_block, n_tiles);
    const int per_wave = (tile1 - tile0 + MF_WAVES - 1) / MF_WAVES;
    const int t_begin = min(tile0 + wave * per_wave, tile1);
    const int t_end = min(t_begin + per_wave, tile1);

    // every lane keeps its three best keys per query group: a row the lane drops is no better than its third key
    int32_t k0[NG], k1[NG], k2[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) { k0[g] = MF_KEY_NONE; k1[g] = MF_KEY_NONE; k2[g] = MF_KEY_NONE; }
    // Software pipeline per wave: while tile t occupies the matrix pipe, the LDS-DMA of tile t+1 is in flight into the wave's
    // other LDS slot; it is waited for (vmcnt) and read back in operand order right before it is needed.  The two accumulator
    // chains of a group pair are interleaved (independent consecutive MFMAs); the VALU top-3 update of a pair is issued under
    // the MFMAs of the next pair.  Each wave owns its two slots: no workgroup barrier in the loop.
    __shared__ __attribute__((aligned(16))) float s_tile[MF_WAVES][2][32 * DIM];
    float a[KH];
    float aug = 0.0f;
    if (t_begin < t_end) {
        dma_a_tile<KH>(vocab, n_rows, t_begin, lane, s_tile[wave][0]);
        aug = row_norm[2 * (size_t)min(t_begin * 32 + col, n_rows) + half];
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        read_a_tile<KH>(s_tile[wave][0], col, half, a);
        dma_a_tile<KH>(vocab, n_rows, min(t_begin + 1, t_end - 1), lane, s_tile[wave][1]);        // prefetch tile t_begin + 1
        float aug_next = row_norm[2 * (size_t)min(min(t_begin + 1, t_end - 1) * 32 + col, n_rows) + half];
        f32x16 p0, p1;                                               // pending accumulators (previous pair)
        int pend_t = t_begin;
        MF_STAMP(1);
        mfma_pair<KH>(a, aug, b[0], b_aug[0], b[1], b_aug[1], p0, p1);
        for (int t = t_begin; t < t_end; ++t) {
#pragma unroll
            for (int gp = 1; gp < NG / 2; ++gp) {                    // remaining pairs of tile t
                f32x16 c0, c1;
                mfma_pair_push<KH>(a, aug, b[2 * gp], b_aug[2 * gp], b[2 * gp + 1], b_aug[2 * gp + 1], c0, c1, p0, p1,
                                   (uint32_t)(pend_t - t_begin), k0[2 * gp - 2], k1[2 * gp - 2], k2[2 * gp - 2], k0[2 * gp - 1],
                                   k1[2 * gp - 1], k2[2 * gp - 1]);
                p0 = c0; p1 = c1;
            }
            if (t + 1 >= t_end) break;
            // tile t+1 has landed in the other slot: operand order -> registers (the MFMAs that read `a` are already issued),
            // then start the DMA of tile t+2 into the slot just vacated
            const int cur = (t + 1 - t_begin) & 1;
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            read_a_tile<KH>(s_tile[wave][cur], col, half, a);
            aug = aug_next;
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");       // the slot reads above precede the DMA that overwrites the other slot's twin
            dma_a_tile<KH>(vocab, n_rows, min(t + 2, t_end - 1), lane, s_tile[wave][cur ^ 1]);
            aug_next = row_norm[2 * (size_t)min(min(t + 2, t_end - 1) * 32 + col, n_rows) + half];
            {
                f32x16 c0, c1;                                       // (t+1, pair 0) with the update of (t, last pair)
                mfma_pair_push<KH>(a, aug, b[0], b_aug[0], b[1], b_aug[1], c0, c1, p0, p1, (uint32_t)(t - t_begin), k0[NG - 2], k1[NG - 2],
                                   k2[NG - 2], k0[NG - 1], k1[NG - 1], k2[NG - 1]);
                p0 = c0; p1 = c1; pend_t = t + 1;
            }
        }
        // the last pending pair: the last pair of groups of the last tile
        push_group(p0, (uint32_t)(pend_t - t_begin), k0[NG - 2], k1[NG - 2], k2[NG - 2]);
        push_group(p1, (uint32_t)(pend_t - t_begin), k0[NG - 1], k1[NG - 1], k2[NG - 1]);
    }

    MF_STAMP(2);
    // workgroup merge: 8 partitions (4 waves x 2 halves) x top-3 per query -> top-MF_KEEP + the smallest partition third
    __shared__ uint64_t s_key[QW][MF_WAVES * 2][3];
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        s_key[g * 32 + col][wave * 2 + half][0] = widen_key(k0[g], t_begin, half);
        s_key[g * 32 + col][wave * 2 + half][1] = widen_key(k1[g], t_begin, half);
        s_key[g * 32 + col][wave * 2 + half][2] = widen_key(k2[g], t_begin, half);
    }
    __syncthreads();
    if (threadIdx.x < QW) {
        const int ql = threadIdx.x;
        uint64_t keep[MF_KEEP];
#pragma unroll
        for (int i = 0; i < MF_KEEP; ++i) keep[i] = KEY_NONE;
        uint32_t lmin = 0x7f800000u;                                 // +inf
        for (int p = 0; p < MF_WAVES * 2; ++p) {
#pragma unroll
            for (int e = 0; e < 3; ++e) {
                uint64_t k = s_key[ql][p][e];
                if (e == 2) lmin = min(lmin, (uint32_t)min(k >> 32, (uint64_t)0x7f800000u));   // rows hidden behind a partition's top-3
#pragma unroll
                for (int i = 0; i < MF_KEEP; ++i) {                  // sorted insertion
                    const uint64_t lo = keep[i] < k ? keep[i] : k;
                    k = keep[i] < k ? k : keep[i];
                    keep[i] = lo;
                }
            }
        }
        const int qi = q0 + ql;
        if (qi < qpad) {
#pragma unroll
            for (int i = 0; i < MF_KEEP; ++i) partial_keys[((size_t)qi * gridDim.x + blockIdx.x) * MF_KEEP + i] = keep[i];
            partial_lmin[(size_t)qi * gridDim.x + blockIdx.x] = lmin;
        }
    }
    MF_STAMP(3);
}


// ------------------------------------------------------------------------------------------------ bf16x3 / fp16 filter
// (the filter bodies, the same-frame distance matrix, the query pre-split and the shadow scores)
#include "bf16_filter_body.cuh"

template <int M>
__global__ __launch_bounds__(256) void knn_bf16_filter_kernel_p(const float* __restrict__ vocab_bf, const float* __restrict__ row_norm, int n_rows,
                                                                const float* __restrict__ queries, int nq, int qpad, int tiles_per_block, int n_blocks,
                                                                int px, StripRecord* __restrict__ records, SelfdistJob sd) {
    extern __shared__ __attribute__((aligned(16))) float s_dyn_p[];
    knn_bf16_filter_body_p<M>(s_dyn_p, (int)blockIdx.x, vocab_bf, row_norm, n_rows, queries, nq, qpad, tiles_per_block, n_blocks, px, records, sd);
}

template <int M>
__global__ __launch_bounds__(MF_WAVES * 64) void knn_bf16_filter_kernel(const float* __restrict__ vocab_bf, const float* __restrict__ row_norm,
                                                                      int n_rows, const float* __restrict__ queries, int nq, int qpad,
                                                                      int tiles_per_block, int n_blocks, StripRecord* __restrict__ records,
                                                                      SelfdistJob sd) {
    extern __shared__ __attribute__((aligned(16))) float s_dyn_f[];
    knn_bf16_filter_body<M>(s_dyn_f, (int)blockIdx.x, vocab_bf, row_norm, n_rows, queries, nq, qpad, tiles_per_block, n_blocks, records, sd);
}

// ------------------------------------------------------------------------------------------------ re-rank + certificate
// (the error bounds of the filters, knn_mfma_rerank_body)
#include "rerank_body.cuh"

template <int DIM, int KEEP, bool LAST_KEY_BOUNDS, bool BF16>
__global__ __launch_bounds__(MF_BLOCK) void knn_mfma_rerank_kernel(KeptKeys<BF16> kk, int n_blocks, int nq,
                                                                   const float* __restrict__ vocab, const float* __restrict__ queries,
                                                                   const int32_t* __restrict__ row_id,
                                                                   const uint32_t* __restrict__ norm_max_bits,
                                                                   int32_t* __restrict__ out_row, int32_t* __restrict__ out_word,
                                                                   float* __restrict__ out_dist, int32_t* __restrict__ fail_list,
                                                                   int32_t* __restrict__ fail_count, CandBits cb, int f16, int n_rows) {
    knn_mfma_rerank_body<DIM, KEEP, LAST_KEY_BOUNDS, BF16>((int)blockIdx.x, kk, n_blocks, nq, vocab, queries, row_id,
                                                          norm_max_bits, out_row, out_word, out_dist, fail_list, fail_count, cb, nullptr, nullptr,
                                                          n_rows, nullptr, 0, f16);
}

// ------------------------------------------------------------------------------------------------ rows of 128 and 256 floats
// (the stateless bf16x3 / fp16 filter, its re-rank and its redo: knn_wide_filter_kernel, knn_wide_rerank_kernel, knn_wide_rowpar_kernel)
#include "wide_filter_body.cuh"

// ------------------------------------------------------------------------------------------------ software-pipelined frames
// Consecutive frames of a device-resident stream overlap INSIDE two launches instead of across streams: the 2-NN stage of frame t
// does not depend on the index stage of frame t - 1 (lcd_frame_dev never changes the vocabulary), so
//   launch A(t) = matrix-core filter of frame t  +  ONE workgroup running the whole tail of frame t - 1 (decision loop, retirements,
//                 registration, idf) + the redo workgroups of frame t - 1: the tail is a single-workgroup latency chain that used
//                 to sit alone on the critical path of every frame; here it hides behind the filter;
//   launch B(t) = exact re-rank of frame t  +  TF-IDF scoring of frame t - 1: two groups of small latency-bound workgroups that fill
//                 each other's stalls.
// Two dependent launches per frame on ONE stream, no events, no second host thread; the data each part reads was written by the
// previous launch (A -> B -> A ...).  The per-frame scratch exists twice (see engine.h).
struct FilterArgs {
    const float* vocab_bf; const float* row_norm; int n_rows; const float* queries; int nq, qpad, tiles_per_block, n_blocks;
    StripRecord* records; SelfdistJob sd; const int32_t* n_lo;
    const uint4* qsplit; const float* qnorm;                           // pre-split queries (non-persistent pipelined launch)
    int delay;                                                         // PipeOpts::filter_delay (timing experiments)
    const float* sh_bf; const float* sh_norm; int sh_rows; float* sh_x; int sh_ld;   // shadow scores (shadow_scores_body): the operand rows of the frame before, the score matrix
};
struct RerankArgs {
    KeptKeys<true> kk; int n_blocks, nq; const float* vocab; const float* queries; const int32_t* row_id;
    const uint32_t* norm_max_bits; int32_t* out_row; int32_t* out_word; float* out_dist; int32_t* fail_list; int32_t* fail_count; CandBits cb;
    const int32_t* n_lo; const int32_t* n_hi; int plan_rows;
    int stage_rows;                                                    // rows the launch's dynamic LDS stages (0: none)
    int f16;                                                           // the filter multiplied fp16 operands (one product): eps_f16
    const float* pend_desc; const uint32_t* pend_list; int32_t pend_first_id;   // the rows a deferred append writes in this launch, as descriptors
    const float* cross; int cross_ld;                                  // this frame's distances to every descriptor of pend_desc (CrossJob of the previous pair), or NULL
    const uint32_t* sh_mask; int sh_q; const float* sh_x; int sh_ld;   // shadow scores (knn_mfma_rerank_body): sh_q == 0: none
};
constexpr int PIPE_BLOCK = 256;     // workgroup size of both fused launches (the filter's and the re-rank's)

// workgroup 0 is the decision loop of the previous frame, workgroup 1 the retirement + registration of the frame before that (dispatched
// first: they are the longest single workgroups of the launch); the redo helpers of the decision loop come LAST -- they have nothing
// to do unless the certificate rejected a query, and in front they would each hold a compute unit's LDS while they find out
struct TailRoles { int has_resolve, has_register, n_redo, n_filter_wgs, n_q_wgs, n_sh_wgs; };
#ifdef LCD_B_TIMING   // timing experiment only: start / end of every workgroup of launch A (100 MHz)
__device__ unsigned long long g_a_timing[2 * 4096];
#define A_STAMP(i) do { __builtin_amdgcn_s_barrier(); if (threadIdx.x == 0 && blockIdx.x < 4096) g_a_timing[2 * blockIdx.x + (i)] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define A_STAMP(i) do { } while (0)
#endif
// grid order: decision loop, registration, filter workgroups (+ distance tiles), query pre-split workgroups, redo helpers
template <bool PERSISTENT, int M>
__device__ __forceinline__ void frame_a_body(float* s_dyn, const FilterArgs& f, int px, const TailRoles& tr, const ResolveArgs& r, const FwArgs& a,
                                             const RetireArgs& ret, const QSplitArgs& qs) {
    const int bid = (int)blockIdx.x;
    const int n_front = tr.has_resolve + tr.has_register;
    A_STAMP(0);
    if (bid < tr.has_resolve) { frame_resolve_part<PIPE_BLOCK>((uint32_t*)s_dyn, r, 0, 1 + tr.n_redo); A_STAMP(1); return; }
    if (bid < n_front) { frame_register_part<PIPE_BLOCK>((uint32_t*)s_dyn, a, ret); A_STAMP(1); return; }
    const int after_strips = n_front + tr.n_filter_wgs;
    if (bid >= after_strips && bid < after_strips + tr.n_sh_wgs) {      // the shadow scores of this frame against the frame before it (non-persistent launches)
        if constexpr (!PERSISTENT) shadow_scores_body<M>(s_dyn, bid - after_strips, f.sh_bf, f.sh_norm, f.sh_rows, f.qsplit, f.qnorm, f.nq, f.qpad, f.sh_x, f.sh_ld);
        A_STAMP(1);
        return;
    }
    const int after_filter = after_strips + tr.n_sh_wgs;
    if (bid >= after_filter && bid < after_filter + tr.n_q_wgs) { qsplit_body(qs, bid - after_filter); A_STAMP(1); return; }
    if (bid >= after_filter + tr.n_q_wgs) { frame_resolve_part<PIPE_BLOCK>((uint32_t*)s_dyn, r, bid - after_filter - tr.n_q_wgs + 1, 1 + tr.n_redo); A_STAMP(1); return; }
    for (int i = 0; i < f.delay; ++i) __builtin_amdgcn_s_sleep(1);      // (0 unless "filter_delay" is set)
    if constexpr (PERSISTENT)
        knn_bf16_filter_body_p<M>(s_dyn, bid - n_front, f.vocab_bf, f.row_norm, f.n_rows, f.queries, f.nq, f.qpad, f.tiles_per_block, f.n_blocks, px,
                               f.records, f.sd, f.n_lo);
    else
        knn_bf16_filter_body_q<M>(s_dyn, bid - n_front, f.vocab_bf, f.row_norm, f.n_rows, f.qsplit, f.qnorm, f.nq, f.qpad, f.tiles_per_block, f.n_blocks,
                               f.records, f.sd, f.n_lo);
    A_STAMP(1);
}
// two workgroups per compute unit: 66 KB of LDS each, and a register budget of two waves per SIMD
template <int M>
__global__ __launch_bounds__(PIPE_BLOCK, 2) void frame_a_kernel(FilterArgs f, TailRoles tr, ResolveArgs r, FwArgs a, RetireArgs ret, QSplitArgs qs) {
    extern __shared__ __attribute__((aligned(16))) float s_dyn_a[];
    frame_a_body<false, M>(s_dyn_a, f, 0, tr, r, a, ret, qs);
}
// the same launch over a vocabulary of more strips than compute units: persistent filter workgroups (knn_bf16_filter_body_p)
template <int M>
__global__ __launch_bounds__(PIPE_BLOCK) void frame_a_kernel_p(FilterArgs f, int px, TailRoles tr, ResolveArgs r, FwArgs a, RetireArgs ret, QSplitArgs qs) {
    extern __shared__ __attribute__((aligned(16))) float s_dyn_ap[];
    frame_a_body<true, M>(s_dyn_ap, f, px, tr, r, a, ret, qs);
}
#ifdef LCD_B_TIMING   // timing experiment only: start / end of every workgroup of launch B (100 MHz)
__device__ unsigned long long g_b_timing[2 * 4096];
__device__ unsigned g_b_role[4096];                                    // 0 re-rank, 1 row writer, 2 sealed bucket, 3 open bucket (tools/launch_b_tail.py)
#define B_ROLE(r) do { if (threadIdx.x == 0 && blockIdx.x < 4096) g_b_role[blockIdx.x] = (r); } while (0)
#ifdef LCD_RR_ACKSTAMP   // the end stamp waits for every wave's requests to be acknowledged (rerank_body.cuh)
#define B_STAMP(i) do { if (i) asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); __builtin_amdgcn_s_barrier(); if (threadIdx.x == 0 && blockIdx.x < 4096) g_b_timing[2 * blockIdx.x + (i)] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define B_STAMP(i) do { __builtin_amdgcn_s_barrier(); if (threadIdx.x == 0 && blockIdx.x < 4096) g_b_timing[2 * blockIdx.x + (i)] = __builtin_amdgcn_s_memrealtime(); } while (0)
#endif
#else
#define B_STAMP(i) do { } while (0)
#define B_ROLE(r) do { } while (0)
#endif
constexpr int PIPE_B_BLOCK = 512;   // workgroup size of launch B: eight waves per sealed bucket, two queries per re-rank workgroup
constexpr uint32_t PIPE_B_STAGE_ROWS = 160;   // pending rows a re-rank workgroup stages in LDS at a time
constexpr int APPEND_SPLIT_BUCKETS = 1024;    // sealed buckets (x 256 signatures) from which a deferred append's row writers get a launch of their own
static_assert(PIPE_B_BLOCK == 2 * MF_BLOCK, "the re-rank halves");
// WITH_APPEND: the workgroups that write a deferred append's rows ride in this launch.  Their mere presence changes the register
// allocation of the whole kernel: the scoring branch, which holds everything in registers without them, then parks ~14 values in scratch
// memory and reloads them inside its latency chain (launch B at 10^6 signatures: 47 -> 62 us; compile-time evidence: the kernel's scratch
// accesses by source file, tools/store_wait_audit.py's sibling in DESIGN 7a).  A memory of >= APPEND_SPLIT_BUCKETS sealed buckets
// therefore launches the row writers as a kernel of their own behind launch B (one more launch, ~4 us, against ~15 us of scoring).
// n_wr > 0: workgroups [n_rerank_wgs, n_rerank_wgs + n_wr) belong to the re-rank role but only write the appended rows (rows_only above);
// the re-rank workgroups proper then write none
template <bool WITH_APPEND>
__global__ __launch_bounds__(PIPE_B_BLOCK, 6) void frame_b_kernel(RerankArgs k, int n_rerank_wgs, ScoreArgs A, int n_score_wgs, AppendRowsArgs app, int n_wr) {
    int bid = (int)blockIdx.x;
    B_STAMP(0);
    const bool rows_only = !WITH_APPEND && n_wr > 0 && bid >= n_rerank_wgs && bid < n_rerank_wgs + n_wr;
    const int wr_index = bid - n_rerank_wgs;
    if (!WITH_APPEND && n_wr > 0 && bid >= n_rerank_wgs + n_wr) bid -= n_wr;            // the scoring workgroups follow
    if (WITH_APPEND && bid >= n_rerank_wgs + n_score_wgs) {              // the rows the decision loop of launch A published (deferred append)
        extern __shared__ __attribute__((aligned(16))) float s_dyn_b2[];
        append_rows_body<PIPE_B_BLOCK>(app, bid - n_rerank_wgs - n_score_wgs, app.ap.lds_bytes >= 1024 ? s_dyn_b2 : nullptr, (app.ap.lds_bytes / 256) & ~3);
        B_STAMP(1);
        return;
    }
    if (bid < n_rerank_wgs || rows_only) {                               // (a multiple of 8: see launch_frame_b)
        B_ROLE(rows_only ? 1u : 0u);
        // consecutive query pairs on one XCD: eight queries share a 128-byte line of the block-major candidate records
        const int pair = rows_only ? 0 : (bid & 7) * (n_rerank_wgs >> 3) + (bid >> 3);
        if (2 * pair >= k.nq) return;
        extern __shared__ __attribute__((aligned(16))) float s_dyn_b[];
        const bool wr_any = !WITH_APPEND && app.ap.enabled && app.ap.defer_rows;
        knn_mfma_rerank_body<64, BF_KEEP, false, true, 2>(2 * pair, k.kk, k.n_blocks, k.nq, k.vocab, k.queries, k.row_id, k.norm_max_bits, k.out_row,
                                                          k.out_word, k.out_dist, k.fail_list, k.fail_count, k.cb, k.n_lo, k.n_hi, k.plan_rows,
                                                          s_dyn_b, k.stage_rows, k.f16, k.pend_desc, k.pend_list, k.pend_first_id, k.cross, k.cross_ld
                                                          , app, wr_any && (n_wr == 0 || rows_only), rows_only ? wr_index : pair, n_wr > 0 ? n_wr : (k.nq + 1) / 2
                                                          , rows_only, k.sh_mask, k.sh_q, k.sh_x, k.sh_ld);
        B_STAMP(1);
        return;
    }
    const int g = bid - n_rerank_wgs;
    B_ROLE(g < A.n_closed_pad ? 2u : 3u);
    if (g < A.n_closed_pad) {                                            // consecutive buckets on one XCD: they share directory lines
        const int b = (g & 7) * (A.n_closed_pad >> 3) + (g >> 3);
        if (b < A.n_closed) score_sealed_body<PIPE_B_BLOCK>(A, b);
    } else score_open_body<PIPE_B_BLOCK>(A, g - A.n_closed_pad);
    B_STAMP(1);
}

__global__ __launch_bounds__(PIPE_B_BLOCK) void append_rows_kernel(AppendRowsArgs app) {
    extern __shared__ __attribute__((aligned(16))) float s_dyn_ar[];
    append_rows_body<PIPE_B_BLOCK>(app, (int)blockIdx.x, app.ap.lds_bytes >= 1024 ? s_dyn_ar : nullptr, (app.ap.lds_bytes / 256) & ~3);
}

// ------------------------------------------------------------------------------------------------ row-parallel exact scan
// rowpar_body.cuh; stand-alone launch for the paths without a fused frame tail
__global__ __launch_bounds__(MF_BLOCK) void knn_rowpar_kernel(RowparArgs a, int32_t* __restrict__ fail_count) {
    rowpar_body<64, MF_BLOCK>(a, (int)blockIdx.x, (int)gridDim.x, fail_count);
}
// shard_merge_kernel + the bit rows of selfdist_l2_kernel for a frame whose distance matrix exists already (lcd_kernels.h): wave w of a workgroup
// owns query 4 * blockIdx.x + w; its lanes read the same records (one request), then the query's row of the (symmetric) matrix
__global__ __launch_bounds__(256) void shard_merge_bits_kernel(ShardMergeJob mj, CandBits cb) {
    const int lane = threadIdx.x & 63;
    const int qi = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (qi >= cb.nq) return;                                         // (wave-uniform)
    const ShardMerged m = shard_merge_one(mj.cand, mj.world, mj.rank, cb.nq, qi, mj.by_word);
    const bool v0 = m.dist[0] >= 0.0f && m.word[0] != 0, v1 = m.dist[1] >= 0.0f && m.word[1] != 0;   // cand_threshold(), knn2_kernels.hip
    const float thr = (cb.have_index && v0 && v1) ? m.dist[1] : __int_as_float(0x7f800000);
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < 2; ++j) { mj.out_word[2 * qi + j] = m.word[j]; mj.out_dist[2 * qi + j] = m.dist[j]; mj.out_wslot[2 * qi + j] = m.wslot[j]; }
    }
    cand_bits_row(cb, qi, thr, lane, 64);
}
// A sharded search's last launch: the exact redo, then the rank's candidate records (shard_pack_kernel's work -- one launch of ~4.7 us less per
// frame and rank).  Nothing to redo (the usual frame): every workgroup sees that and packs its stride of the records; the counters are zero
// already.  A redo: the last workgroup to arrive, which merged and knows every result final, packs all records and zeroes the counters
// ([0] rejected queries, [1] arrivals, [3] done) -- every other workgroup has read [0] and taken its ticket by then.
__global__ __launch_bounds__(MF_BLOCK) void knn_rowpar_pack_kernel(RowparArgs a, int32_t* __restrict__ fail_count, ShardPackArgs p) {
    const int st = rowpar_body<64, MF_BLOCK>(a, (int)blockIdx.x, (int)gridDim.x, fail_count);
    if (st == 0) {
        for (int i = (int)blockIdx.x * MF_BLOCK + (int)threadIdx.x; i < p.q2; i += (int)gridDim.x * MF_BLOCK) shard_pack_one(p, i);
    } else if (st == 2) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");            // (the redone queries' slots were written by this workgroup's other waves)
        for (int i = (int)threadIdx.x; i < p.q2; i += MF_BLOCK) shard_pack_one(p, i);
        if (threadIdx.x < 4 && threadIdx.x != 2) fail_count[threadIdx.x] = 0;
    }
}

}  // namespace
}  // namespace lcd
#ifdef LCD_B_TIMING
extern "C" int lcd_debug_a_timing(unsigned long long* out, int n_words) {
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(lcd::g_a_timing), (size_t)n_words * 8);
}
extern "C" int lcd_debug_rr_timing(unsigned long long* out, int n_words) {
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(lcd::g_rr_timing), (size_t)n_words * 8);
}
extern "C" int lcd_debug_rr_tail(unsigned long long* out, int n_words) {
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(lcd::g_rr_tail), (size_t)n_words * 8);
}
extern "C" int lcd_debug_b_role(unsigned* out, int n_words) {
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(lcd::g_b_role), (size_t)n_words * 4);
}
extern "C" int lcd_debug_b_timing(unsigned long long* out, int n_words) {
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(lcd::g_b_timing), (size_t)n_words * 8);
}
#endif
#ifdef LCD_MFMA_TIMING
extern "C" int lcd_debug_mfma_timing(unsigned long long* out, int n_words) {
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(lcd::g_mf_timing), (size_t)n_words * 8);
}
extern "C" int lcd_debug_mfma_timing2(unsigned long long* out, int n_words) {
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(lcd::g_mf_timing2), (size_t)n_words * 8);
}
#endif
namespace lcd {

// ================================================================================================ host side
bool knn_mfma_supported(int dtype, int dim) { return dtype == 0 && dim == 64; }

MfmaPlan knn_mfma_plan(int q, int n_rows) {
    MfmaPlan p;
    p.q = q;
    p.qpad = (q + 63) / 64 * 64;
    p.n_rows = n_rows;
    const int n_tiles = (n_rows + 31) / 32;
    const int qw = MF_NG * 32;
    const int qgroups = (q + qw - 1) / qw;
    // waves to fill the chip: 256 CUs x 4 SIMDs x 1 wave -> workgroups of 4 waves
    int nb = (256 + qgroups - 1) / qgroups;
    if (nb > (n_tiles + MF_WAVES - 1) / MF_WAVES) nb = (n_tiles + MF_WAVES - 1) / MF_WAVES;   // at least one tile per wave
    if (nb < 1) nb = 1;
    nb = (nb + 7) / 8 * 8;
    int tpb = (n_tiles + nb - 1) / nb;
    tpb = (tpb + MF_WAVES - 1) / MF_WAVES * MF_WAVES;               // equal strips for the 4 waves
    if (tpb < MF_WAVES) tpb = MF_WAVES;
    if (tpb > MF_STRIP_TILES * MF_WAVES) tpb = MF_STRIP_TILES * MF_WAVES;   // the in-loop keys index at most 8 tiles per wave
    p.tiles_per_block = tpb;
    p.n_blocks = n_tiles > 0 ? (n_tiles + tpb - 1) / tpb : 0;
    return p;
}
size_t knn_mfma_partial_bytes(const MfmaPlan& p) {
    const size_t nb = (size_t)(p.n_blocks > 0 ? p.n_blocks : 1);
    return nb * MF_KEEP * p.qpad * sizeof(uint64_t) + nb * p.qpad * sizeof(uint32_t);
}

hipError_t launch_row_norms(const void* vocab, const int32_t* row_id, int first, int n, int dim, float* norm, uint32_t* norm_max_bits,
                            hipStream_t s) {
    if (n <= 0) return hipSuccess;
    row_norm_kernel<<<(n + 255) / 256, 256, 0, s>>>((const float*)vocab, row_id, first, n, dim, norm, norm_max_bits);
    return hipGetLastError();
}
hipError_t launch_vocab_tail(float* norm, void* bf, long long first, long long n, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    vocab_tail_kernel<<<(unsigned)((n * 16 + 255) / 256), 256, 0, s>>>(norm, (uint32_t*)bf, first, n);
    return hipGetLastError();
}
hipError_t launch_norm_tombstone(float* norm, const int32_t* rows, int n, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    norm_tombstone_kernel<<<(n + 255) / 256, 256, 0, s>>>(norm, rows, n);
    return hipGetLastError();
}

__global__ void fail_count_reset_kernel(int32_t* __restrict__ fail_count) {
    if (threadIdx.x < 4 && threadIdx.x != 2) fail_count[threadIdx.x] = 0;
}

hipError_t launch_knn_mfma(int dim, const void* vocab, const float* row_norm, const uint32_t* norm_max_bits, const int32_t* row_id,
                           const void* queries, const MfmaPlan& p, void* partial, int32_t* out_row, int32_t* out_word, float* out_dist,
                           int32_t* fail_list, int32_t* fail_count, hipStream_t s, hipEvent_t ev_begin, hipEvent_t ev_end, bool reset_count,
                           const CandBits* cb) {
    if (p.q == 0) return hipSuccess;
    uint64_t* pk = (uint64_t*)partial;
    uint32_t* pl = (uint32_t*)(pk + (size_t)(p.n_blocks > 0 ? p.n_blocks : 1) * MF_KEEP * p.qpad);
    hipError_t e = hipSuccess;
    if (reset_count) {   // [0] rejected queries, [1] arrival counter of the row-parallel redo (the fused frame tail leaves them zeroed)
        // ... and [3], the "redo done" flag: a stand-alone redo (knn_rowpar_kernel) leaves it raised, and the decision workgroup of a fused frame
        // tail that found it raised would not wait for ITS redo ([2], the running maximum of the error ratio, stays).  One launch for the
        // three words (two hipMemsetAsync calls were two fill kernels in front of every stand-alone search)
        fail_count_reset_kernel<<<1, 64, 0, s>>>(fail_count);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (p.n_blocks > 0) {
        dim3 grid(p.n_blocks, (p.q + MF_NG * 32 - 1) / (MF_NG * 32));
        if (ev_begin) { e = hipEventRecord(ev_begin, s); if (e != hipSuccess) return e; }
        knn_mfma_filter_kernel<64><<<grid, MF_BLOCK, 0, s>>>((const float*)vocab, row_norm, p.n_rows, (const float*)queries, p.q, p.qpad,
                                                              p.tiles_per_block, pk, pl);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
        if (ev_end) { e = hipEventRecord(ev_end, s); if (e != hipSuccess) return e; }
    }
    if (dim != 64) return hipErrorInvalidValue;
    const KeptKeys<false> kk{pk, pl};
    knn_mfma_rerank_kernel<64, MF_KEEP, true, false><<<p.q, MF_BLOCK, 0, s>>>(kk, p.n_blocks, p.q, (const float*)vocab,
                                                                                   (const float*)queries, row_id, norm_max_bits, out_row,
                                                                                   out_word, out_dist, fail_list, fail_count,
                                                                                   cb ? *cb : CandBits{}, 0, p.n_rows);
    return hipGetLastError();
}

// ---- bf16x3 filter
// compute units the launch plans are made for: the device's own count (lcd_create asks hipDeviceProp_t; 256 on MI355X, also the value the
// plans are tested with on a machine without a device)
static int g_plan_cus = 256;
void knn_set_compute_units(int cus) { if (cus >= 16 && cus <= 4096) g_plan_cus = cus; }
int knn_selfdist_wgs(int q) { return selfdist_tiles(q); }
// other_wgs: workgroups of the same launch that run for about as long as a filter workgroup (distance-matrix tiles, the frame tail's
// two workgroups).  Every workgroup of the launch holds a whole compute unit's LDS: 256 strips + 2 tail workgroups used to leave two
// strips for a second round -- a 12 us workgroup each, the launch took twice as long as its filter.
MfmaPlan knn_bf16_plan(int q, int n_rows, int other_wgs) {
    MfmaPlan p;
    p.q = q;
    p.qpad = (q + 63) / 64 * 64;
    p.n_rows = n_rows;
    p.other_wgs = other_wgs > 0 && other_wgs < g_plan_cus / 2 ? other_wgs : 0;
    const int n_tiles = (n_rows + 31) / 32;
    const int qchunks = (q + BF_QB - 1) / BF_QB;
    const int cus = g_plan_cus - p.other_wgs;
    const int per_q = cus / qchunks > 0 ? cus / qchunks : 1;         // workgroups (4 waves, one per SIMD, a whole compute unit's LDS) per block of 512 queries
    // tiles per workgroup when every compute unit gets one; more than a strip holds (the in-loop keys index 8 tiles): the workgroups
    // are persistent and walk `rounds` equal strips each -- so that a vocabulary a little larger than 256 x 8 tiles does not run as
    // one full round plus a nearly empty one
    int w = (n_tiles + per_q - 1) / per_q;
    if (w < 1) w = 1;
    const int rounds = (w + MF_STRIP_TILES - 1) / MF_STRIP_TILES;
    int tpb = (w + rounds - 1) / rounds;
    if (tpb < 1) tpb = 1;
    if (tpb > MF_STRIP_TILES) tpb = MF_STRIP_TILES;
    p.tiles_per_block = tpb;
    p.n_blocks = n_tiles > 0 ? (n_tiles + tpb - 1) / tpb : 0;
    return p;
}
// StripRecord [n_blocks][qpad].  The floor of ONE block is load-bearing: the re-rank's record requests carry no condition, a thread without a
// block asks for block max(n_blocks - 1, 0) (knn_mfma_rerank_body, the up-front requests) -- with no block at all that is block 0 of this buffer.
size_t knn_bf16_partial_bytes(const MfmaPlan& p) {
    const size_t nb = (size_t)(p.n_blocks > 0 ? p.n_blocks : 1);
    static_assert(sizeof(StripRecord) == 16, "one 16-byte request per (block, query)");
    return nb * p.qpad * sizeof(StripRecord);
}
hipError_t launch_vocab_bf16(const void* vocab, int first, int n, int dim, void* bf, hipStream_t s, int f16) {
    if (n <= 0) return hipSuccess;
    if (dim != 64) return hipErrorInvalidValue;
    vocab_bf16_kernel<<<(n * 16 + 255) / 256, 256, 0, s>>>((const float*)vocab, first, n, (uint32_t*)bf, f16);
    return hipGetLastError();
}
// Persistent filter workgroups per block of 512 queries, or 0: the one-strip kernel (every strip gets its own workgroup; up to one
// workgroup per compute unit that is the faster launch).  MfmaPlan::filter_units (lcd_set_option "filter_units") overrides the
// number of compute units to plan for: tests shorten it to walk many strips per workgroup.
static int bf16_persistent_px(const MfmaPlan& p) {
    const int cus = p.filter_units >= 0 ? p.filter_units : g_plan_cus - p.other_wgs;
    const int qchunks = (p.q + BF_QB - 1) / BF_QB;
    if (p.one_strip || cus <= 0 || qchunks <= 0 || p.n_blocks * qchunks <= (p.filter_units >= 0 ? g_plan_cus : cus)) return 0;
    const int px_max = cus / qchunks > 0 ? cus / qchunks : 1;
    const int rounds = (p.n_blocks + px_max - 1) / px_max;
    return (p.n_blocks + rounds - 1) / rounds;                          // equal shares: ceil(strips / rounds) workgroups of <= rounds strips
}
bool knn_bf16_persistent(const MfmaPlan& p) { return p.q > 0 && bf16_persistent_px(p) > 0; }   // which kernel the launch will be (profile labels)
// The plan of a pipelined frame's filter (launch A, pre-split queries: 66 KB of LDS per workgroup, so two share a compute unit).
//   up to one strip per compute unit the distance tiles leave free: one workgroup per strip, alone on its compute unit;
//   up to TWO strips per compute unit: still one workgroup per strip, in pairs -- a pair runs its tiles at 2.2 us each instead of
//     1.24, but starts and ends once per strip instead of walking two strips one after the other (59 000 words: 34.1 us per
//     frame against 38.0 with persistent workgroups, 80 000 words: 39.0 against 41.6);
//   beyond: persistent workgroups (146 KB of LDS, one per compute unit; the two tail workgroups need units of their own then).
MfmaPlan knn_bf16_plan_pipelined(int q, int n_rows, int n_tile_wgs, int filter_units) {
    MfmaPlan p = knn_bf16_plan(q, n_rows, n_tile_wgs);
    p.filter_units = filter_units;
    if (bf16_persistent_px(p) == 0) return p;
    if (filter_units >= 0) {                                            // (tests: a fixed number of persistent workgroups)
        p = knn_bf16_plan(q, n_rows, 2 + n_tile_wgs);
        p.filter_units = filter_units;
        return p;
    }
    const int n_tiles = (n_rows + 31) / 32;
    const int qchunks = (q + BF_QB - 1) / BF_QB;
    const int slots = (2 * (g_plan_cus - p.other_wgs) - 16) / qchunks;         // strips that can be resident at once (16: the two tails, the pre-split, redo helpers)
    if (slots > 0 && n_tiles <= slots * MF_STRIP_TILES) {
        int tpb = (n_tiles + slots - 1) / slots;
        if (tpb < 1) tpb = 1;
        p.tiles_per_block = tpb;
        p.n_blocks = (n_tiles + tpb - 1) / tpb;
        p.one_strip = 1;
        return p;
    }
    p = knn_bf16_plan(q, n_rows, 2 + n_tile_wgs);
    p.filter_units = filter_units;
    return p;
}
hipError_t launch_knn_bf16(int dim, const void* vocab, const void* vocab_bf, const float* row_norm, const uint32_t* norm_max_bits,
                           const int32_t* row_id, const void* queries, const MfmaPlan& p, void* partial, int32_t* out_row, int32_t* out_word,
                           float* out_dist, int32_t* fail_list, int32_t* fail_count, hipStream_t s, hipEvent_t ev_begin, hipEvent_t ev_end,
                           bool reset_count, const CandBits* cb, bool with_selfdist, hipStream_t s_rerank, hipEvent_t ev_bridge) {
    if (p.q == 0) return hipSuccess;
    if (dim != 64) return hipErrorInvalidValue;
    if (!s_rerank || !ev_bridge) s_rerank = s;
    StripRecord* records = (StripRecord*)partial;
    hipError_t e = hipSuccess;
    if (reset_count) {
        // ... and [3], the "redo done" flag: a stand-alone redo (knn_rowpar_kernel) leaves it raised, and the decision workgroup of a fused frame
        // tail that found it raised would not wait for ITS redo ([2], the running maximum of the error ratio, stays).  One launch for the
        // three words (two hipMemsetAsync calls were two fill kernels in front of every stand-alone search)
        fail_count_reset_kernel<<<1, 64, 0, s>>>(fail_count);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (p.n_blocks > 0) {
        static const hipError_t attr0 = hipFuncSetAttribute(reinterpret_cast<const void*>(&knn_bf16_filter_kernel<0>),
                                                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)BF_LDS_BYTES);
        static const hipError_t attr1 = hipFuncSetAttribute(reinterpret_cast<const void*>(&knn_bf16_filter_kernel<1>),
                                                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)BF_LDS_BYTES);
        (void)attr0; (void)attr1;
        SelfdistJob sd;
        if (with_selfdist && cb) {                                    // the same-frame distance matrix rides along
            sd.queries = (const float*)queries; sd.nq = p.q; sd.out = const_cast<float*>(cb->selfdist); sd.ld = cb->ld; sd.n_tiles = sd.n_self = selfdist_tiles(p.q);
        }
        const int grid = sd.n_tiles + p.n_blocks * ((p.q + BF_QB - 1) / BF_QB);
        const int px = bf16_persistent_px(p);
        if (ev_begin) { e = hipEventRecord(ev_begin, s); if (e != hipSuccess) return e; }
        if (px > 0) {
            static const hipError_t attrp0 = hipFuncSetAttribute(reinterpret_cast<const void*>(&knn_bf16_filter_kernel_p<0>),
                                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)BF_LDS_BYTES_P);
            static const hipError_t attrp1 = hipFuncSetAttribute(reinterpret_cast<const void*>(&knn_bf16_filter_kernel_p<1>),
                                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)BF_LDS_BYTES_P);
            (void)attrp0; (void)attrp1;
            const int gp = sd.n_tiles + px * ((p.q + BF_QB - 1) / BF_QB);
            auto kern = p.f16 ? knn_bf16_filter_kernel_p<1> : knn_bf16_filter_kernel_p<0>;
            kern<<<gp, 256, BF_LDS_BYTES_P, s>>>((const float*)vocab_bf, row_norm, p.n_rows, (const float*)queries, p.q, p.qpad, p.tiles_per_block,
                                                 p.n_blocks, px, records, sd);
        } else {
            auto kern = p.f16 ? knn_bf16_filter_kernel<1> : knn_bf16_filter_kernel<0>;
            kern<<<grid, 256, BF_LDS_BYTES, s>>>((const float*)vocab_bf, row_norm, p.n_rows, (const float*)queries, p.q, p.qpad, p.tiles_per_block,
                                                 p.n_blocks, records, sd);
        }
        e = hipGetLastError();
        if (e != hipSuccess) return e;
        if (ev_end) { e = hipEventRecord(ev_end, s); if (e != hipSuccess) return e; }
    }
    if (s_rerank != s) {                                             // the re-rank of this frame on its own stream: the next frame's
        e = hipEventRecord(ev_bridge, s);                             // filter does not have to wait for it
        if (e != hipSuccess) return e;
        e = hipStreamWaitEvent(s_rerank, ev_bridge, 0);
        if (e != hipSuccess) return e;
    }
    const KeptKeys<true> kk{records, p.tiles_per_block};
    knn_mfma_rerank_kernel<64, BF_KEEP, false, true><<<p.q, MF_BLOCK, 0, s_rerank>>>(
        kk, p.n_blocks, p.q, (const float*)vocab, (const float*)queries, row_id, norm_max_bits, out_row, out_word, out_dist, fail_list,
        fail_count, cb ? *cb : CandBits{}, p.f16, p.n_rows);
    return hipGetLastError();
}

hipError_t launch_shard_merge_bits(const ShardMergeJob& mj, const CandBits& cb, hipStream_t s) {
    if (cb.nq <= 0) return hipSuccess;
    if (!mj.cand || !cb.selfdist || !cb.bits || (cb.bw & 1) || cb.ld % 64 != 0) return hipErrorInvalidValue;
    shard_merge_bits_kernel<<<(cb.nq + 3) / 4, 256, 0, s>>>(mj, cb);
    return hipGetLastError();
}

size_t knn_rowpar_partial_bytes(int n_rows, int q) { return (size_t)(q > 0 ? q : 1) * ((n_rows + MF_BLOCK - 1) / MF_BLOCK + 1) * 2 * sizeof(uint64_t); }

hipError_t launch_knn_rowpar(int dim, const void* vocab, const int32_t* row_id, int n_rows, const void* queries, const int32_t* fail_list,
                             int32_t* fail_count, void* partial, int32_t* out_row, int32_t* out_word, float* out_dist, hipStream_t s,
                             const CandBits* cb, const ShardPackArgs* pack) {
    if (dim != 64 || n_rows <= 0) return hipErrorInvalidValue;
    RowparArgs a;
    a.enabled = 1; a.vocab = (const float*)vocab; a.row_id = row_id; a.n_rows = n_rows; a.queries = (const float*)queries;
    a.fail_list = fail_list; a.partial = (unsigned long long*)partial; a.out_row = out_row; a.out_word = out_word; a.out_dist = out_dist;
    if (cb) a.cb = *cb;
    const int nb = (n_rows + MF_BLOCK - 1) / MF_BLOCK;
    if (pack) knn_rowpar_pack_kernel<<<nb, MF_BLOCK, 0, s>>>(a, fail_count, *pack);
    else knn_rowpar_kernel<<<nb, MF_BLOCK, 0, s>>>(a, fail_count);
    return hipGetLastError();
}

// ---- rows of 128 and 256 floats (wide_filter_body.cuh)
bool knn_wide_mfma_supported(int dtype, int dim) { return dtype == 0 && (dim == 128 || dim == 256); }

// One workgroup (eight waves of up to 256 VGPRs: one per compute unit) per block of queries and compute unit; the rows are cut into equal shares
// of at most WD_SHARE_TILES 32-row tiles (one record each), a workgroup takes one or several and walks each in strips of MF_STRIP_TILES.
// units > 0: plan for that many compute units (lcd_set_option "filter_units").  false: no such plan.
bool knn_wide_mfma_plan(int q, int n_rows, int dim, int units, WidePlan* out) {
    if (!out || q <= 0 || n_rows <= 0 || !knn_wide_mfma_supported(0, dim)) return false;
    WidePlan p;
    p.q = q;
    p.qpad = (int)(((long long)q + 63) / 64 * 64);
    if (p.qpad <= 0) return false;
    p.n_rows = n_rows;
    p.dim = dim;
    p.group_q = wide_group_q(dim);
    p.n_qblocks = (p.qpad + p.group_q - 1) / p.group_q;
    if (p.n_qblocks > 65535) return false;                              // grid.y
    const int cus = units > 0 ? units : g_plan_cus;
    const int target = std::max(1, cus / p.n_qblocks);
    const int n_tiles = (int)(((long long)n_rows + 31) / 32);
    // tiles per workgroup when every compute unit gets one; more than a share holds: every workgroup walks `rounds` equal shares
    const int w = (n_tiles + target - 1) / target;
    const int rounds = (w + WD_SHARE_TILES - 1) / WD_SHARE_TILES;
    p.tiles_per_block = (int)(((long long)n_tiles + (long long)target * rounds - 1) / ((long long)target * rounds));
    p.n_blocks = (n_tiles + p.tiles_per_block - 1) / p.tiles_per_block;
    p.n_wgs = std::min(p.n_blocks, target);
    if (knn_wide_partial_bytes(p) > 0x7FFFFFFFull) return false;
    *out = p;
    return true;
}
size_t knn_wide_partial_bytes(const WidePlan& p) {
    const size_t nb = (size_t)(p.n_blocks > 0 ? p.n_blocks : 1);
    return nb * BF_KEEP * p.qpad * sizeof(uint64_t) + nb * p.qpad * sizeof(uint32_t);
}

template <int DIM, int M>
static hipError_t launch_wide_filter(const WidePlan& p, const float* vocab, const int32_t* row_id, const float* queries, const ShareRecords& rec,
                                     uint32_t* norm_max_bits, hipStream_t s) {
    // (per launch, checked: <256, 0> needs more than the 64 KB a kernel gets unasked, and the attribute belongs to the current device)
    const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(&knn_wide_filter_kernel<DIM, M>),
                                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)WideShape<DIM, M>::LDS_BYTES);
    if (attr != hipSuccess) return attr;
    knn_wide_filter_kernel<DIM, M><<<dim3(p.n_wgs, p.n_qblocks), WD_BLOCK, WideShape<DIM, M>::LDS_BYTES, s>>>(vocab, row_id, p.n_rows, queries, p.q, p.qpad,
                                                                                                             p.tiles_per_block, p.n_blocks, rec, norm_max_bits);
    return hipGetLastError();
}

hipError_t launch_knn_wide(const WidePlan& p, int f16, const void* vocab, const int32_t* row_id, const void* queries, void* partial, void* partial_redo,
                           uint32_t* norm_max_bits, int32_t* out_row, int32_t* out_word, float* out_dist, int32_t* fail_list, int32_t* fail_count,
                           hipStream_t s, hipEvent_t ev_begin, hipEvent_t ev_end, bool reset_count) {
    if (p.q == 0) return hipSuccess;
    if (!knn_wide_mfma_supported(0, p.dim) || p.n_blocks <= 0 || p.n_rows <= 0) return hipErrorInvalidValue;
    ShareRecords rec;
    rec.keys = (uint64_t*)partial;
    rec.bound = (uint32_t*)(rec.keys + (size_t)p.n_blocks * BF_KEEP * p.qpad);
    const float* v = (const float*)vocab; const float* qq = (const float*)queries;
    knn_wide_reset_kernel<<<1, 64, 0, s>>>(fail_count, reset_count ? 1 : 0, norm_max_bits);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (ev_begin) { e = hipEventRecord(ev_begin, s); if (e != hipSuccess) return e; }
    if (p.dim == 128) e = f16 ? launch_wide_filter<128, 1>(p, v, row_id, qq, rec, norm_max_bits, s) : launch_wide_filter<128, 0>(p, v, row_id, qq, rec, norm_max_bits, s);
    else e = f16 ? launch_wide_filter<256, 1>(p, v, row_id, qq, rec, norm_max_bits, s) : launch_wide_filter<256, 0>(p, v, row_id, qq, rec, norm_max_bits, s);
    if (e != hipSuccess) return e;
    if (ev_end) { e = hipEventRecord(ev_end, s); if (e != hipSuccess) return e; }
    if (p.dim == 128)
        knn_wide_rerank_kernel<128><<<p.q, MF_BLOCK, 0, s>>>(rec, p.n_blocks, p.q, p.qpad, v, qq, row_id, p.n_rows, norm_max_bits, out_row, out_word, out_dist,
                                                             fail_list, fail_count, f16);
    else
        knn_wide_rerank_kernel<256><<<p.q, MF_BLOCK, 0, s>>>(rec, p.n_blocks, p.q, p.qpad, v, qq, row_id, p.n_rows, norm_max_bits, out_row, out_word, out_dist,
                                                             fail_list, fail_count, f16);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    // the queries the certificate rejected are redone exactly (usually none: every workgroup leaves at once)
    RowparArgs a;
    a.enabled = 1; a.vocab = v; a.row_id = row_id; a.n_rows = p.n_rows; a.queries = qq;
    a.fail_list = fail_list; a.partial = (unsigned long long*)partial_redo; a.out_row = out_row; a.out_word = out_word; a.out_dist = out_dist;
    const int nb = (p.n_rows + MF_BLOCK - 1) / MF_BLOCK;
    if (p.dim == 128) knn_wide_rowpar_kernel<128><<<nb, MF_BLOCK, 0, s>>>(a, fail_count);
    else knn_wide_rowpar_kernel<256><<<nb, MF_BLOCK, 0, s>>>(a, fail_count);
    return hipGetLastError();
}

// ---- software-pipelined frames (see frame_a_kernel / frame_b_kernel)
int pipe_block_size() { return PIPE_BLOCK; }
int pipe_b_block_size() { return PIPE_B_BLOCK; }

size_t knn_qsplit_bytes(int q) { return (size_t)((q + 63) / 64 * 64) * 256; }

// lcd_set_option "cross_frame_tiles" = 1: launch A also computes the frame's distances to the frame before it, and the re-rank reads its
// pending rows' distances there instead of staging the rows.  Built, bit-identical (tests/test_gpu_append_dev.py), and NOT the default:
// measured on one box with the kernel trace of the driver's command (profiles/r05_ab_notes.txt 9), launch B 19.7 -> 17.5 us while every
// frame creates ~150 words, but the 64 extra tiles share compute units with the filter strips -- launch A 14.2 -> 15.3 us there and
// 13.3 -> 15.0 us once frames mostly revisit (where launch B gains nothing): 0.0417 -> 0.0412 ms per frame over the driver's 20 steps,
// 0.0409 -> 0.0412 over 200, and the filter launch is the one the roofline is quoted on.

hipError_t launch_frame_a(const PipeKnn* kp, const QSplitArgs* qsp, const TailLaunch* resolve, const TailLaunch* reg, hipStream_t s, hipEvent_t ev_begin,
                          hipEvent_t ev_end, const PipeOpts& opt) {
    static const hipError_t attr0 = hipFuncSetAttribute(reinterpret_cast<const void*>(&frame_a_kernel<0>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                        (int)BF_LDS_BYTES_Q);
    static const hipError_t attr1 = hipFuncSetAttribute(reinterpret_cast<const void*>(&frame_a_kernel<1>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                        (int)BF_LDS_BYTES_Q);
    (void)attr0; (void)attr1;
    FilterArgs f{};
    MfmaPlan p;
    p.q = 0; p.qpad = 0; p.n_rows = 0; p.tiles_per_block = 1; p.n_blocks = 0;
    if (kp) {
        const PipeKnn& k = *kp;
        p = k.plan;
        if (p.n_shadow > 0 && k.sh_bf && k.sh_norm && k.sh_rows > 0 && k.sh_x) { f.sh_bf = (const float*)k.sh_bf; f.sh_norm = k.sh_norm; f.sh_rows = k.sh_rows; f.sh_x = k.sh_x; f.sh_ld = k.sh_ld; }
        f.vocab_bf = (const float*)k.vocab_bf; f.row_norm = k.row_norm; f.n_rows = p.n_rows; f.queries = (const float*)k.queries; f.nq = p.q; f.qpad = p.qpad;
        f.tiles_per_block = p.tiles_per_block; f.n_blocks = p.n_blocks; f.records = (StripRecord*)k.partial; f.n_lo = k.n_lo;
        f.qsplit = (const uint4*)k.qsplit; f.qnorm = k.qnorm;
        if (k.cb.selfdist) {                                          // the same-frame distance matrix rides along
            f.sd.queries = (const float*)k.queries; f.sd.nq = p.q; f.sd.out = const_cast<float*>(k.cb.selfdist); f.sd.ld = k.cb.ld; f.sd.n_tiles = f.sd.n_self = selfdist_tiles(p.q);
        }
        if (opt.cross_frames && k.cross && k.cross_cols && k.cross_ncols > 0 && p.q > 0) {   // ... and so do this frame's distances to the frame before it
            f.sd.queries = (const float*)k.queries; f.sd.nq = p.q;
            f.sd.other = (const float*)k.cross_cols; f.sd.n_other = k.cross_ncols; f.sd.xout = k.cross; f.sd.xld = k.cross_ld;
            f.sd.n_tiles += ((p.q + 63) / 64) * ((k.cross_ncols + 63) / 64);
        }
    }
    f.delay = opt.filter_delay;
    const int px = p.q > 0 ? bf16_persistent_px(p) : 0;
    if (px == 0 && p.q > 0 && (!f.qsplit || !f.qnorm)) return hipErrorInvalidValue;      // the one-strip launch reads pre-split queries
    if (p.n_shadow > 0 && (px > 0 || !f.sh_x)) return hipErrorInvalidValue;   // shadow scores: one-strip launches with the rows at hand only (the engine plans them so)
    TailRoles tr;
    tr.n_filter_wgs = p.q > 0 ? f.sd.n_tiles + (px > 0 ? px : p.n_blocks) * ((p.q + BF_QB - 1) / BF_QB) : 0;
    tr.n_sh_wgs = (p.q > 0 && p.n_shadow > 0) ? ((f.sh_rows + 31) / 32) * ((p.q + BF_QB - 1) / BF_QB) : 0;
    tr.has_resolve = resolve ? 1 : 0; tr.has_register = reg ? 1 : 0; tr.n_redo = resolve ? resolve->n_redo : 0;
    QSplitArgs qs{};
    if (qsp) { qs = *qsp; qs.n_wgs = std::min((qs.qpad * 8 + PIPE_BLOCK - 1) / PIPE_BLOCK, 32); if (qs.n_wgs < 1) qs.n_wgs = 1; }   // one item per thread up to 1 024 descriptors
    tr.n_q_wgs = qsp ? qs.n_wgs : 0;
    const int grid = tr.n_filter_wgs + tr.n_sh_wgs + tr.has_resolve + tr.has_register + tr.n_redo + tr.n_q_wgs;
    if (grid == 0) return hipSuccess;
    const size_t lds = px > 0 ? BF_LDS_BYTES_P : BF_LDS_BYTES_Q;
    if ((resolve && resolve->shmem_resolve > lds) || (reg && reg->shmem + (size_t)reg->a.n * 4 > lds)) return hipErrorInvalidValue;   // (+ the word slots parked in LDS)
    ResolveArgs r{}; FwArgs a{}; RetireArgs ret{};
    if (resolve) { r = resolve->r; r.ap.lds_bytes = (int)lds; }        // what the decision loop's tables leave of it stages the frame's new rows
    if (reg) { a = reg->a; ret = reg->ret; }
    // ev_begin / ev_end: the launch's own start and end time stamps (hipExtLaunchKernel attaches the two events to the dispatch; a pair
    // of hipEventRecord around it costs the stream ~10 us of barrier packets -- and measures the gap in front of the kernel with it)
    const bool timed = ev_begin != nullptr && ev_end != nullptr;
    const bool f16 = kp ? p.f16 != 0 : opt.f16 != 0;                    // (no filter: the variant the handle's filter launches keep hot)
    if (px > 0) {
        static const hipError_t attrp0 = hipFuncSetAttribute(reinterpret_cast<const void*>(&frame_a_kernel_p<0>),
                                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)BF_LDS_BYTES_P);
        static const hipError_t attrp1 = hipFuncSetAttribute(reinterpret_cast<const void*>(&frame_a_kernel_p<1>),
                                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)BF_LDS_BYTES_P);
        (void)attrp0; (void)attrp1;
        auto kern = f16 ? frame_a_kernel_p<1> : frame_a_kernel_p<0>;
        if (timed) hipExtLaunchKernelGGL(kern, dim3(grid), dim3(PIPE_BLOCK), (uint32_t)BF_LDS_BYTES_P, s, ev_begin, ev_end, 0u, f, px, tr, r, a, ret, qs);
        else kern<<<grid, PIPE_BLOCK, BF_LDS_BYTES_P, s>>>(f, px, tr, r, a, ret, qs);
    } else {
        auto kern = f16 ? frame_a_kernel<1> : frame_a_kernel<0>;
        if (timed) hipExtLaunchKernelGGL(kern, dim3(grid), dim3(PIPE_BLOCK), (uint32_t)BF_LDS_BYTES_Q, s, ev_begin, ev_end, 0u, f, tr, r, a, ret, qs);
        else kern<<<grid, PIPE_BLOCK, BF_LDS_BYTES_Q, s>>>(f, tr, r, a, ret, qs);
    }
    return hipGetLastError();
}


static long long g_b_routes[8];                                        // see lcd_debug_launch_b_routes
hipError_t launch_frame_b(const PipeKnn* k, const ScoreArgs* score, int score_wgs, hipStream_t s, hipEvent_t ev_begin, hipEvent_t ev_end,
                          const AppendRowsArgs* app, const PipeOpts& opt) {
    RerankArgs rk{};
    int n_rerank = 0;
    if (k) {
        const MfmaPlan& p = k->plan;
        rk.kk.records = (const StripRecord*)k->partial; rk.kk.tiles_per_block = p.tiles_per_block;
        rk.n_blocks = p.n_blocks; rk.nq = p.q; rk.vocab = (const float*)k->vocab; rk.queries = (const float*)k->queries; rk.row_id = k->row_id;
        rk.norm_max_bits = k->norm_max_bits; rk.out_row = k->out_row; rk.out_word = k->out_word; rk.out_dist = k->out_dist;
        rk.fail_list = k->fail_list; rk.fail_count = k->fail_count; rk.cb = k->cb; rk.n_lo = k->n_lo; rk.n_hi = k->n_hi; rk.plan_rows = p.n_rows; rk.f16 = p.f16;
        n_rerank = ((p.q + 1) / 2 + 7) & ~7;                          // two queries per workgroup; padded to the XCD count (frame_b_kernel)
    }
    ScoreArgs A{};
    if (score) A = *score; else score_wgs = 0;
    AppendRowsArgs ar{};
    int n_app = 0;
    if (app && app->ap.enabled && app->ap.defer_rows) { ar = *app; n_app = ar.n_wgs = APPEND_ROW_WGS; }
    if (n_rerank + score_wgs + n_app == 0) return hipSuccess;
    // frames that append their words on the device: 40 KB of dynamic LDS stage 160 pending rows per re-rank workgroup (three workgroups
    // of launch B share a compute unit: 3 x (40 + 10) KB of its 160 KB); the workgroups that write appended rows stage them there too
    const uint32_t dyn = ((k && k->n_hi) || n_app) ? PIPE_B_STAGE_ROWS * 256u : 0u;   // (the workgroup's two queries lie in the body's static LDS)
    rk.stage_rows = (dyn && k && k->n_hi) ? (int)PIPE_B_STAGE_ROWS : 0;
    ar.ap.lds_bytes = (int)(PIPE_B_STAGE_ROWS * 256u);
    if (k && n_app) { rk.pend_desc = ar.ap.descriptors; rk.pend_list = ar.ap.list_out; rk.pend_first_id = ar.ap.first_id; }   // k's pending rows ARE the rows being written
    // ... and their distances to k's queries were computed by launch A of this pair (selfdist_tile's cross-frame tiles), if it knew both frames
    if (k && n_app && opt.cross_frames && k->cross && k->cross_cols == (const void*)ar.ap.descriptors) { rk.cross = k->cross; rk.cross_ld = k->cross_ld; }
    // Who writes the rows of the deferred append: the re-rank workgroups (they hold the rows in their staging area) -- no third branch in the
    // kernel, whose presence makes the scoring branch spill: launch B 15.4 -> 13.8 us once frames create few words.  While frames create
    // ~150 words each (the driver's 20 steps) the two ways are within box-to-box noise of each other (0.0387 against 0.0380 ms per frame
    // on one box, 0.0418 against 0.0427 on another), and choosing per launch by the expected number of new rows lost to both (the second
    // kernel variant is loaded in the middle of the stream): profiles/r05_ab_notes.txt 6.  "append_from_rerank" = 0 keeps round 4's eight
    // row-writer workgroups for A/B runs.
    const bool writers = opt.append_from_rerank == 0;
    if (!writers && k && n_app > 0 && k->n_hi && k->plan.q > 0 && rk.stage_rows >= 4) n_app = 0;   // the re-rank workgroups write the rows (`ar` stays filled in: they get it);
                                                                                      // without re-rank workgroups or a staging area the writers stay
    // shadow rows: the filter of launch A ranked the descriptors of the frame whose rows are written here; the re-rank needs that frame's new-word mask
    const bool shadow = k && k->plan.n_shadow > 0 && k->sh_mask && k->sh_x && k->sh_q > 0 && app && app->ap.enabled && app->ap.defer_rows && rk.pend_desc && !rk.cross;
    if (k && k->plan.n_shadow > 0 && !shadow) return hipErrorInvalidValue;          // (launch A wrote scores nobody reads: the engine plans the two together)
    if (shadow) { rk.sh_mask = k->sh_mask; rk.sh_q = k->sh_q; rk.sh_x = k->sh_x; rk.sh_ld = k->sh_ld; }
    // round 6: rows written by n_wr extra workgroups of the re-rank role instead of by the re-rank workgroups themselves ("row_writer_wgs");
    // with shadow rows the re-rank workgroups stage nothing they could write, so the writers are not optional
    const int n_wr = (!writers && n_app == 0 && k && app && app->ap.enabled && app->ap.defer_rows && k->n_hi && k->plan.q > 0 && rk.stage_rows >= 4 && !rk.cross &&
                      (opt.row_writer_wgs > 0 || shadow)) ? (opt.row_writer_wgs > 0 ? opt.row_writer_wgs : 16) : 0;
    if (shadow && n_wr == 0) return hipErrorInvalidValue;
    if (k && n_rerank > 0) {                                         // (tests: lcd_debug_launch_b_routes)
        g_b_routes[0] += 1; g_b_routes[1] += shadow ? 1 : 0; g_b_routes[2] += n_wr > 0 ? 1 : 0; g_b_routes[3] += rk.cross ? 1 : 0;
        g_b_routes[4] += (rk.pend_list && !shadow && !rk.cross && rk.stage_rows >= 4) ? 1 : 0;
        g_b_routes[5] += (!writers && n_app == 0 && n_wr == 0 && rk.pend_list) ? 1 : 0; g_b_routes[6] = n_wr; g_b_routes[7] = n_rerank;
    }
    const bool split = n_app > 0 && score && score->n_closed >= (opt.append_split_buckets >= 0 ? opt.append_split_buckets : APPEND_SPLIT_BUCKETS);   // (see frame_b_kernel)
    if (split || n_app == 0) {
        if (n_rerank + score_wgs > 0) {
            if (ev_begin != nullptr && ev_end != nullptr)
                hipExtLaunchKernelGGL(frame_b_kernel<false>, dim3(n_rerank + n_wr + score_wgs), dim3(PIPE_B_BLOCK), dyn, s, ev_begin, ev_end, 0u, rk, n_rerank, A, score_wgs, ar, n_wr);
            else frame_b_kernel<false><<<n_rerank + n_wr + score_wgs, PIPE_B_BLOCK, dyn, s>>>(rk, n_rerank, A, score_wgs, ar, n_wr);
        }
        if (n_app > 0) append_rows_kernel<<<n_app, PIPE_B_BLOCK, PIPE_B_STAGE_ROWS * 256u, s>>>(ar);
        return hipGetLastError();
    }
    if (ev_begin != nullptr && ev_end != nullptr)
        hipExtLaunchKernelGGL(frame_b_kernel<true>, dim3(n_rerank + score_wgs + n_app), dim3(PIPE_B_BLOCK), dyn, s, ev_begin, ev_end, 0u, rk, n_rerank, A, score_wgs, ar, 0);
    else frame_b_kernel<true><<<n_rerank + score_wgs + n_app, PIPE_B_BLOCK, dyn, s>>>(rk, n_rerank, A, score_wgs, ar, 0);
    return hipGetLastError();
}

}  // namespace lcd

// Which routes the launches B of this process were given through the re-rank role since the last reset (tests; host-side counts of what each launch was
// set up for -- whether rows were pending at all is the device's to know --, nothing is read from the device): out8[0] launches with re-rank workgroups, of which [1] with shadow scores (the new words of the frame before as candidates of one row each),
// [2] with row-writer workgroups of the re-rank role, [3] with the pending rows' distances from the cross-frame tiles, [4] with the pending rows staged and
// scanned by every re-rank workgroup, [5] with the rows written by the re-rank workgroups themselves; [6] writer workgroups and [7] re-rank workgroups (two
// queries each, padded to a multiple of eight) of the latest such launch.
extern "C" int lcd_debug_launch_b_routes(long long* out8, int reset) {
    if (out8) for (int i = 0; i < 8; ++i) out8[i] = lcd::g_b_routes[i];
    if (reset) for (int i = 0; i < 8; ++i) lcd::g_b_routes[i] = 0;
    return 0;
}

// The launch plan of a pipelined frame's filter for a vocabulary of n_rows and q descriptors, as the engine makes it (tests; no device
// needed): out[0] tiles per workgroup, [1] strips, [2] persistent workgroups per block of 512 queries (0: one workgroup per strip),
// [3] distance-tile workgroups riding in the launch, [4] query blocks
extern "C" int lcd_debug_frame_plan(int q, int n_rows, int new_words_compared, int* out) {
    if (q <= 0 || n_rows <= 0 || !out) return -1;
    const int tiles = new_words_compared ? lcd::knn_selfdist_wgs(q) : 0;
    const lcd::MfmaPlan p = lcd::knn_bf16_plan_pipelined(q, n_rows, tiles, -1);
    out[0] = p.tiles_per_block; out[1] = p.n_blocks; out[2] = lcd::bf16_persistent_px(p); out[3] = tiles; out[4] = (q + lcd::BF_QB - 1) / lcd::BF_QB;
    return 0;
}

// The launch plan of the wide-row matrix-core filter for q queries over n_rows rows of dim floats (128 or 256), as run_knn2_raw makes it for a
// handle whose "filter_units" is `units` (0, -1: the device's compute units) -- tests; no device needed:
// out9[0] tiles (32 rows) per share, [1] shares (one record per share and query), [2] query blocks (grid.y), [3] queries per block, [4] qpad,
// [5] bytes of the partial records / 4, [6] tiles per strip (the key's index bits), [7] strips per share, [8] workgroups along the rows
// (grid.x; workgroup x takes shares x, x + [8], ...).
// -1: no such plan (another row length, arguments the handle does not admit, or records beyond an int)
extern "C" int lcd_debug_wide_mfma_plan(int q, int n_rows, int dim, int units, int* out9) {
    lcd::WidePlan p;
    if (!out9 || !lcd::knn_wide_mfma_plan(q, n_rows, dim, units, &p)) return -1;
    out9[0] = p.tiles_per_block; out9[1] = p.n_blocks; out9[2] = p.n_qblocks; out9[3] = p.group_q; out9[4] = p.qpad;
    out9[5] = (int)(lcd::knn_wide_partial_bytes(p) / 4); out9[6] = lcd::MF_STRIP_TILES;
    out9[7] = (p.tiles_per_block + lcd::MF_STRIP_TILES - 1) / lcd::MF_STRIP_TILES; out9[8] = p.n_wgs;
    return 0;
}

#ifdef LCD_SCORE_TIMING   // timing experiment only: the phase stamps of the scoring workgroups of launch B (this translation unit's copy)
extern "C" int lcd_debug_score_timing_pipe(unsigned long long* out, int n_words) {
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(lcd::g_score_timing), (size_t)n_words * 8);
}
#endif

#ifdef LCD_TAIL_TIMING   // timing experiment only: the stamps of the tail that ran inside the fused filter launch (this translation unit's copy)
extern "C" int lcd_debug_tail_timing_pipe(unsigned long long* out) {
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(lcd::g_tail_timing), 64) != hipSuccess) return -2;
    if (hipMemcpyFromSymbol(out + 8, HIP_SYMBOL(lcd::g_resolve_timing), 64) != hipSuccess) return -3;
    return (int)hipMemcpyFromSymbol(out + 16, HIP_SYMBOL(lcd::g_sweep_timing), 256);
}
#endif
