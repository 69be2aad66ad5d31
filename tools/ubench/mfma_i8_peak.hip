// Micro-benchmark: sustained rate of v_mfma_i32_32x32x32_i8 on this box (1, 2 or 4 independent accumulator chains per wave, 1 or 2 waves
// per SIMD), and the same chain with the two-smallest update of knn2_hamming_mfma_kernel (v_min, v_max, v_min per accumulator register) after
// every 8 products.  The denominator of that kernel's roofline fraction.  hipcc --offload-arch=gfx950 -O3
#include <hip/hip_runtime.h>
#include <cstdio>
typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

template <int CHAINS, bool TOP2>
__global__ __launch_bounds__(256) void k(int* out, int iters, int a0, int b0) {
    v16i acc[CHAINS];
    for (int c = 0; c < CHAINS; ++c) for (int r = 0; r < 16; ++r) acc[c][r] = (int)(threadIdx.x + c);
    v4i a, b;
    for (int j = 0; j < 4; ++j) { a[j] = a0 + (int)threadIdx.x * (j + 1); b[j] = b0 - (int)threadIdx.x * (j + 3); }
    unsigned best = ~0u, second = ~0u;
    for (int i = 0; i < iters; ++i) {
#pragma unroll
        for (int c = 0; c < CHAINS; ++c) {
#pragma unroll
            for (int u = 0; u < 8; ++u) acc[c] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b, acc[c], 0, 0, 0);
            if (TOP2) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const unsigned key = (unsigned)acc[c][r], hi = max(best, key);
                    best = min(best, key);
                    second = min(second, hi);
                }
            }
        }
    }
    int s = (int)(best + second);
    for (int c = 0; c < CHAINS; ++c) for (int r = 0; r < 16; ++r) s += acc[c][r];
    out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}

template <int CHAINS, bool TOP2>
void run(int blocks, const char* label) {
    int* out; hipMalloc(&out, (size_t)blocks * 256 * 4);
    const int iters = 4000;
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    k<CHAINS, TOP2><<<blocks, 256>>>(out, 10, 1, 2);
    hipDeviceSynchronize();
    hipEventRecord(e0);
    k<CHAINS, TOP2><<<blocks, 256>>>(out, iters, 1, 2);
    hipEventRecord(e1);
    hipDeviceSynchronize();
    float ms; hipEventElapsedTime(&ms, e0, e1);
    const double mfmas = (double)blocks * 4 * iters * 8 * CHAINS;
    const double ops = mfmas * 32 * 32 * 32 * 2;
    printf("%-52s blocks=%4d chains=%d  %.3f ms  %.1f TOP/s  (%.1f cycles/MFMA/SIMD at 2.4 GHz)\n", label, blocks, CHAINS, ms, ops / ms / 1e9,
           ms * 1e-3 * 2.4e9 / (mfmas / 1024.0));
    hipFree(out);
}
int main() {
    run<1, false>(256, "1 wave/SIMD, 1 dependent chain");
    run<4, false>(256, "1 wave/SIMD, 4 chains");
    run<1, false>(512, "2 waves/SIMD, 1 chain each");
    run<4, false>(512, "2 waves/SIMD, 4 chains each");
    run<4, true>(256, "1 wave/SIMD, 4 chains + two-smallest update");
    run<4, true>(512, "2 waves/SIMD, 4 chains + two-smallest update");
    return 0;
}
