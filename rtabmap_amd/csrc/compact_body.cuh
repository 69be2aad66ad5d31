// compact_body.cuh -- what the per-frame kernels of feature_select.hip, keypoints_3d.hip, keypoints_3d_stereo.hip and flow_track.hip and the motion kernels (motion_3d.hip and
// motion_pnp.hip, through motion_join.cuh's sort and motion_group.cuh's compaction and selection) share: the ballot scan that compacts a
// workgroup's flags in thread order, the gather of rows behind an index list, and the bitonic sort of 64-bit keys in LDS.  Device code only.
// Internal.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lcd {

// exclusive rank of this thread's flag among the workgroup's flags in thread order, and their total (two barriers; wsum: one int per wave)
__device__ __forceinline__ int block_rank(bool flag, int* wsum, int& total) {
    const unsigned long long m = __ballot(flag);
    const int in_wave = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    const int wave = threadIdx.x >> 6, n_waves = blockDim.x >> 6;
    if ((threadIdx.x & 63) == 0) wsum[wave] = __popcll(m);
    __syncthreads();
    int before = 0, all = 0;
    for (int w = 0; w < n_waves; ++w) {
        const int v = wsum[w];
        if (w < wave) before += v;
        all += v;
    }
    __syncthreads();
    total = all;
    return before + in_wave;
}

// dst row j = src row idx[j], j < count (count x bytes / sizeof(V) fits an int: at most 16384 x 128), `bytes` per row in pieces of V; src, dst
// and idx are the frame's own
template <typename V>
__device__ __forceinline__ void gather_rows(const void* src, void* dst, const int32_t* idx, int count, int bytes) {
    const int per = bytes / (int)sizeof(V);
    const V* s = reinterpret_cast<const V*>(src);
    V* d = reinterpret_cast<V*>(dst);
    const int total = count * per;
    for (int e = threadIdx.x; e < total; e += blockDim.x) {
        const int j = e / per, c = e - j * per;
        d[(size_t)j * per + c] = s[(size_t)idx[j] * per + c];
    }
}

// the same for the frame that starts at feature `first` of [N x bytes] arrays
template <typename V>
__device__ __forceinline__ void gather_rows(const void* src, void* dst, const int32_t* idx, int64_t first, int count, int bytes) {
    gather_rows<V>((const char*)src + first * bytes, (char*)dst + first * bytes, idx, count, bytes);
}

// What the depth stage and the stereo stage do behind their index list (which the workgroup has just written: the caller's barrier lies in
// front): the frame's kept rows of `bytes` bytes each, [first, first + count) of dst from the rows idx names of src, in chunks whose element
// counter fits an int; vec: 16 or 4, the widest copy the addresses and sizes allow
__device__ __forceinline__ void gather_kept_rows(const void* src_all, void* dst_all, const int32_t* idx, int64_t first, int count, int bytes, int vec) {
    constexpr int CHUNK = 16384;
    const char* src = (const char*)src_all + first * bytes;
    for (int c0 = 0; c0 < count; c0 += CHUNK) {
        const int c = min(count - c0, CHUNK);
        char* dst = (char*)dst_all + (first + c0) * bytes;
        if (vec == 16) gather_rows<uint4>(src, dst, idx + c0, c, bytes);
        else gather_rows<uint32_t>(src, dst, idx + c0, c, bytes);
    }
}

// Where key i lies in LDS: one spare slot behind every eight keys.  The network's threads walk the keys with strides of 8, 64, 512, .. keys
// between neighbouring lanes; unpadded, those land on the same banks (64 banks of 4 bytes: 32 keys) up to sixteen lanes deep.
__host__ __device__ __forceinline__ int padded(int i) { return i + (i >> 3); }

// M consecutive steps of a bitonic network's level k in one round trip through LDS: the strides j, j/2, .., j >> (M - 1).  A thread takes the
// 2^M keys that differ only in those M index bits (they meet nobody else during these steps), orders them in registers and puts them back.
template <int M>
__device__ __forceinline__ void bitonic_pass(uint64_t* keys, int p2, int k, int j) {
    const int j_lo = j >> (M - 1);
    for (int g = threadIdx.x; g < (p2 >> M); g += blockDim.x) {
        const int base = ((g & ~(j_lo - 1)) << M) | (g & (j_lo - 1));
        const bool ascending = (base & k) == 0;                        // the same for the 2^M keys: their indices differ below bit k
        uint64_t e[1 << M];
#pragma unroll
        for (int a = 0; a < (1 << M); ++a) e[a] = keys[padded(base + a * j_lo)];
#pragma unroll
        for (int b = M - 1; b >= 0; --b) {
#pragma unroll
            for (int a = 0; a < (1 << M); ++a) {
                if ((a >> b) & 1) continue;
                const uint64_t x = e[a], y = e[a | (1 << b)];
                const bool swap = (x > y) == ascending;
                e[a] = swap ? y : x;
                e[a | (1 << b)] = swap ? x : y;
            }
        }
#pragma unroll
        for (int a = 0; a < (1 << M); ++a) keys[padded(base + a * j_lo)] = e[a];
    }
}

// keys[padded(0 .. p2 - 1)] ascending, p2 a power of two >= 2: the whole network, three steps to a round trip through LDS; ends behind a barrier
__device__ __forceinline__ void bitonic_sort(uint64_t* keys, int p2) {
    for (int k = 2; k <= p2; k <<= 1) {                                // the strides k/2 .. 1 of level k, three to a round trip through LDS
        int j = k >> 1;
        for (; j >= 4; j >>= 3) { bitonic_pass<3>(keys, p2, k, j); __syncthreads(); }
        if (j == 2) bitonic_pass<2>(keys, p2, k, 2);
        else if (j == 1) bitonic_pass<1>(keys, p2, k, 1);
        if (j) __syncthreads();
    }
}

}  // namespace lcd
