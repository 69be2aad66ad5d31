// knn_hamming_mfma.hip -- exact Hamming 2-NN of binary descriptors on the gfx950 matrix cores (LCD_KNN_HAMMING_MFMA, u8 handles).
//
// Replaces knn2_hamming_kernel (knn2_kernels.hip) for the main vocabulary of a u8 handle in this mode; it writes the same partial keys
// [n_blocks][2][qpad], (hamming << 32) | row, so knn2_merge_kernel / knn2_merge_selfdist_hamming_kernel consume them unchanged.
//
// The arithmetic.  Hamming distance is an integer dot product, and v_mfma_i32_32x32x32_i8 computes integer dot products exactly.  A bit of a
// vocabulary row becomes the byte +127 (set) or -127 (clear), a bit of a query the byte -127 (set) or +127 (clear): over B = 32 * w32 bits
//     dot = sum(q_byte * v_byte) = 127^2 * (differing - equal) = KM * (2 * hamming - B),          KM = 127 * 127 = 16129.
// The accumulator does not start at zero but at   C[row] = KM * B + (row - row0)   (row0: the workgroup's first row), so one chain of w32
// MFMAs leaves, per (row, query),
//     key = KM * (2 * hamming) + (row - row0),
// which orders like (hamming, row) as long as a workgroup covers fewer than KM rows: the sort key of the two-smallest update, lower row first on
// equal distance, comes out of the matrix pipe finished.  A row that is no row (row_id == 0: tombstones, rows behind the device's row count)
// starts at KEY_DEAD + KM * B instead and ends at or above KEY_DEAD = KM * (2 * B + 1) whatever its bytes hold; a live key is below it.  All of
// it fits 32 bits for every row length the engine admits (B <= 32768: KM * (4 * B + 1) < 2^31).  What is left per pair on the VALU is the
// two-smallest update (v_min, v_max, v_min): 3 instructions instead of the ~20 of the xor / bit-count scan.  Nothing is approximate: no
// filter, no certificate, no re-rank.  Zero padding of a row (dim 61 -> 64 bytes) is 'equal bits' on both operands.
//
// Mapping, rows of W = 2, 4, 8, 16 dwords (knn2_hamming_mfma_kernel<W, QT, CHUNK_TILES>): a workgroup of four waves walks a strip of rows in chunks
// of 64 (32 at W = 16: the two LDS buffers stay at 32 KB).
//   * Vocabulary: the packed rows stay as they are in memory.  The workgroup expands a chunk bit -> byte ONCE into LDS, in the order the A
//     operand wants it (one ds_read_b128 per lane and K step, consecutive lanes 16 bytes apart), and all four waves read it from there;
//     the chunk after it is fetched from memory before the products of this one are issued, and expanded into the other LDS buffer behind them
//     (two buffers: one barrier per chunk).
//   * Queries: a wave keeps QT tiles of 32 queries expanded in registers for the whole kernel (QT * W * 4 VGPRs; 512 queries of 256 bits are
//     4 tiles x 32 VGPRs on each of the four waves).  Every row tile read from LDS meets all of them.
//   * One dword of a row is one K = 32 step: lanes 0-31 take its low 16 bits, lanes 32-63 its high 16.  Both operands go through the same
//     expansion, so the K order inside a step cannot matter.
//   * C/D: the query is on the lane (column = lane & 31), the 16 registers are rows (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5) of the tile;
//     each lane keeps a running (best, second) per query tile, the two lane halves are merged once at the end.
// Any other row length (knn2_hamming_mfma_dyn_kernel): a runtime K loop, both operands expanded from memory as they are needed, a wave per
// row tile; the correctness path, as knn2_hamming_dyn_kernel is for the scan.
#include "lcd_kernels.h"
#include "top2_keys.cuh"

#include <algorithm>

namespace lcd {
namespace {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));
typedef uint32_t v4u __attribute__((ext_vector_type(4)));

constexpr int BLOCK = 256;
constexpr int WAVES = 4;
constexpr uint32_t KM = 127u * 127u;             // one differing bit more moves the key by 2 * KM; rows of a workgroup are told apart below KM
constexpr int MAX_BLOCK_ROWS = 16128;            // < KM, a multiple of every chunk
constexpr int PLAN_UNIT = 64;                    // a workgroup's strip is a multiple of this many rows (a multiple of every chunk)

// 16 bits -> 16 bytes (4 dwords, bit j in byte j): set -> +127 and clear -> -127 (NEG = false, vocabulary), the opposite signs for NEG (queries).
// (nibble * 0x00408102) puts bit i of the nibble at bit 8 * i + 1: the four shifted copies do not overlap, and the factor fits v_mul_u32_u24
template <bool NEG>
__device__ __forceinline__ v4i expand16(uint32_t bits) {
    v4i r;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t two = __umul24((bits >> (4 * j)) & 0xFu, 0x00408102u) & 0x02020202u;   // 2 in the byte of every set bit
        r[j] = (int)(NEG ? 0x7F7F7F7Fu + two : 0x81818181u - two);                            // 0x7F = +127, 0x81 = -127: no carry between bytes
    }
    return r;
}

__device__ __forceinline__ void top2_push32(uint32_t& best, uint32_t& second, uint32_t k) {
    const uint32_t hi = max(best, k);
    best = min(best, k);
    second = min(second, hi);
}
__device__ __forceinline__ void top2_push_tile(uint32_t& best, uint32_t& second, const v16i& acc) {
#pragma unroll
    for (int i = 0; i < 16; ++i) top2_push32(best, second, (uint32_t)acc[i]);
}

// the key of the matrix pipe -> the key of the merges
__device__ __forceinline__ uint64_t decode_key(uint32_t k, uint32_t key_dead, int row0) {
    if (k >= key_dead) return KEY_NONE;
    const uint32_t twice = k / KM;
    return ((uint64_t)(twice >> 1) << 32) | (uint32_t)(row0 + (int)(k - twice * KM));
}
// the two halves of the wave hold different rows for the same query: merged, the low half stores
__device__ __forceinline__ void halves_merge_store(uint32_t best, uint32_t second, int lane, uint32_t key_dead, int row0, int qi, int qpad,
                                                   uint64_t* __restrict__ partial) {
    const uint32_t ob = __shfl_xor(best, 32, 64), os = __shfl_xor(second, 32, 64);
    top2_push32(best, second, ob);
    top2_push32(best, second, os);
    if (lane < 32) {
        partial[((size_t)blockIdx.x * 2 + 0) * qpad + qi] = decode_key(best, key_dead, row0);
        partial[((size_t)blockIdx.x * 2 + 1) * qpad + qi] = decode_key(second, key_dead, row0);
    }
}

// ------------------------------------------------------------------------------------------------ rows of W dwords, queries in registers
// grid.x = row blocks, grid.y = groups of WAVES * QT * 32 queries.  Query tile t of the group belongs to wave t % WAVES.
// CHUNK_TILES = 32-row tiles expanded per barrier (two LDS buffers of CHUNK_TILES * W KiB).
template <int W, int QT, int CHUNK_TILES>
__global__ __launch_bounds__(BLOCK, 2) void knn2_hamming_mfma_kernel(const uint32_t* __restrict__ vocab, const int32_t* __restrict__ row_id, int n_rows,
                                                                     const uint32_t* __restrict__ queries, int nq, int qpad, int rows_per_block,
                                                                     uint64_t* __restrict__ partial) {
    constexpr int CHUNK_ROWS = 32 * CHUNK_TILES;
    static_assert(PLAN_UNIT % CHUNK_ROWS == 0, "a strip is whole chunks");
    constexpr int ITEMS = CHUNK_ROWS * W;                             // packed dwords of a chunk
    constexpr int PER = (ITEMS + BLOCK - 1) / BLOCK;                  // ... per thread
    constexpr uint32_t BITS = 32u * W;
    constexpr uint32_t BASE_LIVE = KM * BITS, KEY_DEAD = KM * (2u * BITS + 1u), BASE_DEAD = KEY_DEAD + KM * BITS;
    // [buffer][tile][K step][lane half][row of the tile] fragments of 16 bytes, and the accumulator start of every row
    __shared__ v4i s_a[2][CHUNK_TILES * W * 64];
    __shared__ __attribute__((aligned(16))) uint32_t s_base[2][CHUNK_ROWS];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5;
    const int q_first = blockIdx.y * (WAVES * QT * 32);
    const int n_tiles = min(WAVES * QT, (min(nq, qpad) - q_first + 31) / 32);   // query tiles of this group (>= 1)
    const int row0 = blockIdx.x * rows_per_block;
    const int row1 = min(row0 + rows_per_block, n_rows);
    const int n_chunks = (row1 - row0 + CHUNK_ROWS - 1) / CHUNK_ROWS;

    // the wave's queries: tile wave + WAVES * t, lane -> query (lane & 31), K step k -> its half of dword k
    v4i qf[QT][W];
#pragma unroll
    for (int t = 0; t < QT; ++t) {
        const int qi = q_first + (wave + WAVES * t) * 32 + (lane & 31);
        const uint32_t* src = queries + (size_t)min(qi, nq - 1) * W;  // lanes behind the last query repeat it; their keys are never read
#pragma unroll
        for (int k = 0; k < W; ++k) qf[t][k] = expand16<true>((src[k] >> (16 * half)) & 0xFFFFu);
    }

    // staging: item = (tile, K step, row of the tile), row fastest
    uint32_t st[PER];
    int32_t st_id = 0;
    auto fetch = [&](int chunk) {
        const int r_first = row0 + chunk * CHUNK_ROWS;
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int it = tid + u * BLOCK;
            const int r = r_first + (it / (32 * W)) * 32 + (it & 31), k = (it >> 5) % W;
            st[u] = (ITEMS % BLOCK == 0 || it < ITEMS) ? vocab[(size_t)min(r, n_rows - 1) * W + k] : 0u;   // behind the strip: clamped, the row is dead below
        }
        if (tid < CHUNK_ROWS) { const int r = r_first + tid; st_id = r < row1 ? row_id[r] : 0; }
    };
    auto expand = [&](int chunk, int buf) {
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int it = tid + u * BLOCK;
            if (ITEMS % BLOCK == 0 || it < ITEMS) {
                const int frag = (it / (32 * W)) * (W * 64) + ((it >> 5) % W) * 64 + (it & 31);
                s_a[buf][frag] = expand16<false>(st[u] & 0xFFFFu);
                s_a[buf][frag + 32] = expand16<false>(st[u] >> 16);
            }
        }
        if (tid < CHUNK_ROWS) s_base[buf][tid] = st_id != 0 ? BASE_LIVE + (uint32_t)(chunk * CHUNK_ROWS + tid) : BASE_DEAD;
    };

    uint32_t best[QT], second[QT];
#pragma unroll
    for (int t = 0; t < QT; ++t) { best[t] = ~0u; second[t] = ~0u; }

    if (n_chunks > 0) { fetch(0); expand(0, 0); }
    __syncthreads();
    for (int c = 0; c < n_chunks; ++c) {
        const int buf = c & 1;
        if (c + 1 < n_chunks) fetch(c + 1);
#pragma unroll
        for (int tt = 0; tt < CHUNK_TILES; ++tt) {
            if (wave >= n_tiles) break;                                // a wave without queries only stages
            // the 16 rows of this lane's accumulator registers: (i & 3) + 8 * (i >> 2) + 4 * half
            v16i base;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const v4u b = *reinterpret_cast<const v4u*>(&s_base[buf][tt * 32 + 8 * g + 4 * half]);
                base[4 * g + 0] = (int)b[0]; base[4 * g + 1] = (int)b[1]; base[4 * g + 2] = (int)b[2]; base[4 * g + 3] = (int)b[3];
            }
            v4i a[W];
#pragma unroll
            for (int k = 0; k < W; ++k) a[k] = s_a[buf][tt * (W * 64) + k * 64 + lane];
#pragma unroll
            for (int t = 0; t < QT; ++t) {
                if (wave + WAVES * t >= n_tiles) break;
                v16i acc = base;
#pragma unroll
                for (int k = 0; k < W; ++k) acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[k], qf[t][k], acc, 0, 0, 0);
                top2_push_tile(best[t], second[t], acc);
            }
        }
        if (c + 1 < n_chunks) expand(c + 1, buf ^ 1);
        __syncthreads();
    }
#pragma unroll
    for (int t = 0; t < QT; ++t) {
        const int tile = wave + WAVES * t;
        if (tile >= n_tiles) break;
        const int qi = q_first + tile * 32 + (lane & 31);
        if (qi < qpad) halves_merge_store(best[t], second[t], lane, KEY_DEAD, row0, qi, qpad, partial);
    }
}

// ------------------------------------------------------------------------------------------------ any row length: runtime K loop
// grid.x = row blocks, grid.y = groups of 64 queries (two tiles per wave); wave w of the workgroup takes row tiles w, w + WAVES, ... of the block
__global__ __launch_bounds__(BLOCK) void knn2_hamming_mfma_dyn_kernel(const uint32_t* __restrict__ vocab, const int32_t* __restrict__ row_id, int n_rows,
                                                                      int w32, const uint32_t* __restrict__ queries, int nq, int qpad,
                                                                      int rows_per_block, uint64_t* __restrict__ partial) {
    __shared__ uint32_t s_key[WAVES][2][2][64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int half = lane >> 5;
    const uint32_t bits = 32u * (uint32_t)w32;
    const uint32_t base_live = KM * bits, key_dead = KM * (2u * bits + 1u), base_dead = key_dead + KM * bits;
    const int row0 = blockIdx.x * rows_per_block;
    const int row1 = min(row0 + rows_per_block, n_rows);
    const uint32_t* qsrc[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) qsrc[t] = queries + (size_t)min(blockIdx.y * 64 + t * 32 + (lane & 31), nq - 1) * w32;
    uint32_t best[2] = {~0u, ~0u}, second[2] = {~0u, ~0u};
    for (int tile0 = row0 + wave * 32; tile0 < row1; tile0 += WAVES * 32) {
        v16i base;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int r = tile0 + (i & 3) + 8 * (i >> 2) + 4 * half;
            const bool live = r < row1 && row_id[min(r, n_rows - 1)] != 0;
            base[i] = (int)(live ? base_live + (uint32_t)(r - row0) : base_dead);
        }
        const uint32_t* vsrc = vocab + (size_t)min(tile0 + (lane & 31), n_rows - 1) * w32;   // behind the last row: clamped, the row is dead above
        v16i acc[2] = {base, base};
        for (int k = 0; k < w32; ++k) {
            const v4i a = expand16<false>((vsrc[k] >> (16 * half)) & 0xFFFFu);
#pragma unroll
            for (int t = 0; t < 2; ++t)
                acc[t] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, expand16<true>((qsrc[t][k] >> (16 * half)) & 0xFFFFu), acc[t], 0, 0, 0);
        }
#pragma unroll
        for (int t = 0; t < 2; ++t) top2_push_tile(best[t], second[t], acc[t]);
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) { s_key[wave][t][0][lane] = best[t]; s_key[wave][t][1][lane] = second[t]; }
    __syncthreads();
    if (wave < 2) {                                                  // wave t merges query tile t of the four waves
        uint32_t b = ~0u, s = ~0u;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) { top2_push32(b, s, s_key[w][wave][0][lane]); top2_push32(b, s, s_key[w][wave][1][lane]); }
        const int qi = blockIdx.y * 64 + wave * 32 + (lane & 31);
        halves_merge_store(b, s, lane, key_dead, row0, qi, qpad, partial);
    }
}

int g_cus = 256;

}  // namespace

// ================================================================================================ host side
bool knn_hamming_mfma_fixed(int w32) { return w32 == 2 || w32 == 4 || w32 == 8 || w32 == 16; }

HammingMfmaPlan knn_hamming_mfma_plan(int q, int n_rows, int dim_bytes, int units) {
    HammingMfmaPlan p;
    p.q = q;
    p.qpad = (q + 63) / 64 * 64;
    p.n_rows = n_rows;
    p.w32 = dim_bytes / 4;
    const bool fixed = knn_hamming_mfma_fixed(p.w32);
    p.group_q = fixed ? (p.w32 == 16 ? WAVES * 2 * 32 : WAVES * 4 * 32) : 64;
    const int groups = (p.qpad + p.group_q - 1) / p.group_q;
    const int unit = fixed ? PLAN_UNIT : WAVES * 32;                // rows a workgroup takes in one step
    // two workgroups per compute unit (one wave of each on every SIMD: the products of one run beside the key updates of the other)
    const int cus = units > 0 ? units : g_cus;                      // (tests: a fixed number of workgroups, whatever the device)
    const int target = std::max(1, (int)((2 * (long long)cus + groups - 1) / groups));
    long long rpb = ((long long)n_rows + target - 1) / target;
    rpb = (rpb + unit - 1) / unit * unit;
    if (rpb < unit) rpb = unit;
    if (rpb > MAX_BLOCK_ROWS) rpb = MAX_BLOCK_ROWS;                   // the key tells the rows of a workgroup apart below KM
    p.rows_per_block = (int)rpb;
    p.n_blocks = n_rows > 0 ? (int)(((long long)n_rows + rpb - 1) / rpb) : 0;
    return p;
}
KnnPlan knn_hamming_mfma_merge_plan(const HammingMfmaPlan& p) {
    KnnPlan k;
    k.q = p.q; k.qpad = p.qpad; k.n_rows = p.n_rows; k.rows_per_block = p.rows_per_block; k.n_blocks = p.n_blocks;
    return k;
}
size_t knn_hamming_mfma_partial_bytes(const HammingMfmaPlan& p) { return (size_t)(p.n_blocks > 0 ? p.n_blocks : 1) * 2 * p.qpad * sizeof(uint64_t); }
void knn_hamming_mfma_set_compute_units(int cus) { if (cus > 0) g_cus = cus; }

hipError_t launch_knn2_hamming_mfma(const void* vocab, const int32_t* row_id, const void* queries, const HammingMfmaPlan& p, uint64_t* partial,
                                    hipStream_t s) {
    if (p.n_blocks == 0 || p.q == 0) return hipSuccess;
    if (p.w32 < 1 || p.w32 > 1024 || p.rows_per_block > MAX_BLOCK_ROWS) return hipErrorInvalidValue;   // the 32-bit key: B <= 32768 bits, rows < KM
    const uint32_t* v = (const uint32_t*)vocab; const uint32_t* qq = (const uint32_t*)queries;
    dim3 grid(p.n_blocks, (p.qpad + p.group_q - 1) / p.group_q), block(BLOCK);
    switch (knn_hamming_mfma_fixed(p.w32) ? p.w32 : 0) {
        case 2: knn2_hamming_mfma_kernel<2, 4, 2><<<grid, block, 0, s>>>(v, row_id, p.n_rows, qq, p.q, p.qpad, p.rows_per_block, partial); break;
        case 4: knn2_hamming_mfma_kernel<4, 4, 2><<<grid, block, 0, s>>>(v, row_id, p.n_rows, qq, p.q, p.qpad, p.rows_per_block, partial); break;
        case 8: knn2_hamming_mfma_kernel<8, 4, 2><<<grid, block, 0, s>>>(v, row_id, p.n_rows, qq, p.q, p.qpad, p.rows_per_block, partial); break;
        case 16: knn2_hamming_mfma_kernel<16, 2, 1><<<grid, block, 0, s>>>(v, row_id, p.n_rows, qq, p.q, p.qpad, p.rows_per_block, partial); break;
        default: knn2_hamming_mfma_dyn_kernel<<<grid, block, 0, s>>>(v, row_id, p.n_rows, p.w32, qq, p.q, p.qpad, p.rows_per_block, partial); break;
    }
    return hipGetLastError();
}

}  // namespace lcd

// The launch plan of the matrix-core Hamming 2-NN for q queries over n_rows rows of dim_bytes (padded to whole dwords, as the handle pads its
// rows), as scan_partial makes it for a handle whose "filter_units" is `units` (0, -1: the device's compute units) -- tests; no device needed:
// out6[0] rows per workgroup, [1] workgroups along the rows (grid.x), [2] query groups (grid.y), [3] rows of a chunk of the chosen
// instantiation (the runtime-K kernel: the 128 rows its four waves take in one step), [4] qpad, [5] bytes of the partial keys / 16.
// -1: no such plan (arguments the handle does not admit, or partial keys beyond an int)
extern "C" int lcd_debug_hamming_mfma_plan(int q, int n_rows, int dim_bytes, int units, int* out6) {
    if (q <= 0 || n_rows <= 0 || dim_bytes <= 0 || dim_bytes > 4096 || !out6) return -1;
    const lcd::HammingMfmaPlan p = lcd::knn_hamming_mfma_plan(q, n_rows, (dim_bytes + 3) / 4 * 4, units);
    const size_t bytes = lcd::knn_hamming_mfma_partial_bytes(p);
    if (bytes > 0x7FFFFFFFull) return -1;
    out6[0] = p.rows_per_block; out6[1] = p.n_blocks; out6[2] = (p.qpad + p.group_q - 1) / p.group_q;
    out6[3] = lcd::knn_hamming_mfma_fixed(p.w32) ? (p.w32 == 16 ? 32 : 64) : lcd::WAVES * 32;
    out6[4] = p.qpad; out6[5] = (int)(bytes / 16);
    return 0;
}
