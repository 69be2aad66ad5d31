// compact_body.cuh -- what the per-frame kernels of feature_select.hip and keypoints_3d.hip share: the ballot scan that compacts a
// workgroup's flags in thread order, and the gather of rows behind an index list.  Device code only.  Internal.
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

}  // namespace lcd
