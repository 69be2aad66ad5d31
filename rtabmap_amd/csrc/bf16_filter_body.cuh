// bf16_filter_body.cuh -- the bf16x3 / fp16 matrix-core distance filter (device code): the one-strip body, the body over pre-split
// queries and the shadow scores of a pipelined frame's launch A, the persistent body, and the same-frame distance matrix and query
// pre-split that ride in the same launches.  A section of knn_mfma_kernels.hip, which includes it once, inside namespace lcd::{anonymous},
// behind the tile, key and time-stamp helpers it uses (dma_a_tile, read_a_tile, push_group4, widen_key, op_split2, MF_STAMP, ...): not a
// stand-alone header.
#pragma once

// ------------------------------------------------------------------------------------------------ bf16x3 filter
// The same filter with the contraction on the bf16 matrix pipe (v_mfma_f32_32x32x16_bf16, 16x the f32 MFMA rate): every float
// is split hi + lo (two bf16), and q . v ~ qh.vh + qh.vl + ql.vh -- three bf16 MFMA chains accumulated in fp32 into the SAME
// accumulator that the f32 augmentation step (|v|^2 + |q|^2, exact) initialised.  The neglected ql.vl and the bf16 rounding of
// the lo parts cost < 2^-16 relative to |q||v|, which eps_bf16() adds to the certificate -- the result stays the exact scan's.
//
// Workgroup = 4 waves x 128 queries (512 queries) against ONE shared strip of vocabulary tiles: a tile (32 rows x {hi, lo} =
// 8 KiB) is brought in once by LDS-DMA (each wave issues a quarter), double-buffered, one barrier per tile, and read by all four
// waves -- the vocabulary crosses L2 -> LDS once per 512 queries.  The queries are staged the same way (coalesced DMA, then
// operand order), split on the fly, and stay in registers for the whole kernel.
constexpr int BF_KEEP = 2;                       // keys kept per (row block, query); the third best is the block's bound
constexpr int BF_QW = 128;                       // queries per wave
constexpr int BF_NG = BF_QW / 32;                // 32-query groups per wave: four accumulator chains, four waves, one per SIMD (eight waves of
                                                 // two groups, two per SIMD, measured equal)
constexpr int BF_QB = BF_QW * MF_WAVES;          // queries per workgroup
constexpr int BF_TILE_F = 32 * 64;               // floats (dwords) per staged tile
constexpr size_t BF_LDS_BYTES = (size_t)(MF_WAVES * 4 + 2) * BF_TILE_F * 4 + (size_t)MF_STRIP_TILES * 64 * 4;   // + the strip's augmentation entries
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));

// DMA instructions [i0, i1) of the 8 that move one 32-row x 256-byte tile (same swizzle as dma_a_tile)
// HI (round 6, the fp16 filter): only the row's first 128-byte line -- the "hi" operands, the only ones the one-product filter multiplies -- is
// requested: the lanes whose chunk lies in the "lo" line sit the instruction out.  Same instruction count (the waits that count instructions
// stay valid), same LDS layout (the lo positions are simply never written or read), HALF the bytes: the opening burst of launch A -- every
// strip asks for its whole strip in the first microsecond -- is 6.3 MB instead of 12.5 MB at 49 000 words.
template <bool HI = false>
__device__ __forceinline__ void dma_tile_part(const float* __restrict__ base, int n_rows, int t, int lane, float* __restrict__ lds_slot,
                                              int i0, int i1) {
    for (int i = i0; i < i1; ++i) {
        const int p = i * 64 + lane;
        const int r = p >> 4, cpos = p & 15;
        const int c = cpos ^ (r & 15);
        if (HI && c >= 8) continue;
        const int row = min(t * 32 + r, n_rows - 1);
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(base + (size_t)row * 64 + c * 4),
                                         (__attribute__((address_space(3))) void*)(lds_slot + i * 256), 16, 0, 0);
    }
}
typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));
template <int M>
__device__ __forceinline__ f32x16 bf_mfma(const uint4& a, const uint4& b, const f32x16& c) {
    if (M == 1) return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8_t, a), __builtin_bit_cast(f16x8_t, b), c, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), c, 0, 0, 0);
}
// One 32-row tile against two 32-query groups: 2 x (1 f32 augmentation step + 12 bf16 steps), the two accumulator chains
// interleaved; with PUSH the top-3 update of the previous pair's 32 scores is spread between the steps.
// M = 0: bf16, three products per fp32 product (hi.hi + hi.lo + lo.hi); M = 1: fp16, the hi.hi product alone.
template <bool PUSH, int M>
__device__ __forceinline__ void bf_pair(const uint4 (&ah)[4], const uint4 (&al)[4], float a_aug, const uint4 (&bh0)[4], const uint4 (&bl0)[4],
                                        float b0_aug, const uint4 (&bh1)[4], const uint4 (&bl1)[4], float b1_aug, f32x16& c0, f32x16& c1,
                                        const f32x16& p0, const f32x16& p1, uint32_t tl, int32_t& k00, int32_t& k01, int32_t& k02,
                                        int32_t& k10, int32_t& k11, int32_t& k12) {
    const f32x16 z = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    const uint32_t base = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tl << 4));
    const uint32_t mask = strip_mask();
    c0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a_aug, b0_aug, z, 0, 0, 0);
    c1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a_aug, b1_aug, z, 0, 0, 0);
#pragma unroll
    for (int st = 0; st < 12; ++st) {
        const int s = st / 3, term = st % 3;                        // (hi, hi), (hi, lo), (lo, hi)
        const uint4& a = term == 2 ? al[s] : ah[s];
#if LCD_MFMA_ABLATE != 3      // 4 / 5: only the (hi, hi) / the (hi, hi) + (hi, lo) products -- the MFMA count of a one- / two-product filter (timing only)
        if ((M == 0 && LCD_MFMA_ABLATE < 4) || term == 0 || (LCD_MFMA_ABLATE == 5 && term == 1)) c0 = bf_mfma<M>(a, term == 1 ? bl0[s] : bh0[s], c0);
#endif
        if (PUSH && LCD_MFMA_ABLATE == 1) asm volatile("" :: "v"(p0[st]), "v"(p1[st]));   // keep the ablated chains alive
        if (PUSH && LCD_MFMA_ABLATE != 1) {                         // one MFMA, then the VALU that fits in its 32-cycle shadow
            __builtin_amdgcn_sched_barrier(0);
            if (st < 4) top3_push32(k00, k01, k02, strip_key(min4(p0[4 * st], p0[4 * st + 1], p0[4 * st + 2], p0[4 * st + 3]), mask, base | (uint32_t)(4 * st)));   // group st of the previous pair
            __builtin_amdgcn_sched_barrier(0);
        }
#if LCD_MFMA_ABLATE != 3
        if ((M == 0 && LCD_MFMA_ABLATE < 4) || term == 0 || (LCD_MFMA_ABLATE == 5 && term == 1)) c1 = bf_mfma<M>(a, term == 1 ? bl1[s] : bh1[s], c1);
#endif
        if (PUSH && LCD_MFMA_ABLATE != 1) {
            __builtin_amdgcn_sched_barrier(0);
            if (st < 4) top3_push32(k10, k11, k12, strip_key(min4(p1[4 * st], p1[4 * st + 1], p1[4 * st + 2], p1[4 * st + 3]), mask, base | (uint32_t)(4 * st)));
            __builtin_amdgcn_sched_barrier(0);
        }
    }
}

// Eight 16-byte LDS reads + the wait for them, as ONE inline-assembly statement the compiler does not see as LDS traffic (see the
// filter loop).
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void lds_read8_b128(const uint32_t (&addr)[8], uint4 (&out)[8], uint32_t addr32, float& out32) {
    u32x4_t v0, v1, v2, v3, v4, v5, v6, v7;
    asm volatile(
        "ds_read_b128 %0, %9\n\tds_read_b128 %1, %10\n\tds_read_b128 %2, %11\n\tds_read_b128 %3, %12\n\t"
        "ds_read_b128 %4, %13\n\tds_read_b128 %5, %14\n\tds_read_b128 %6, %15\n\tds_read_b128 %7, %16\n\t"
        "ds_read_b32 %8, %17\n\t"
        "s_waitcnt lgkmcnt(0)"
        : "=&v"(v0), "=&v"(v1), "=&v"(v2), "=&v"(v3), "=&v"(v4), "=&v"(v5), "=&v"(v6), "=&v"(v7), "=&v"(out32)
        : "v"(addr[0]), "v"(addr[1]), "v"(addr[2]), "v"(addr[3]), "v"(addr[4]), "v"(addr[5]), "v"(addr[6]), "v"(addr[7]), "v"(addr32)
        : "memory");
    out[0] = __builtin_bit_cast(uint4, v0); out[1] = __builtin_bit_cast(uint4, v1); out[2] = __builtin_bit_cast(uint4, v2);
    out[3] = __builtin_bit_cast(uint4, v3); out[4] = __builtin_bit_cast(uint4, v4); out[5] = __builtin_bit_cast(uint4, v5);
    out[6] = __builtin_bit_cast(uint4, v6); out[7] = __builtin_bit_cast(uint4, v7);
}
// the same for the "hi" operands alone (the fp16 filter): four 16-byte reads
__device__ __forceinline__ void lds_read4_b128(const uint32_t (&addr)[8], uint4 (&out)[8], uint32_t addr32, float& out32) {
    u32x4_t v0, v1, v2, v3;
    asm volatile(
        "ds_read_b128 %0, %5\n\tds_read_b128 %1, %6\n\tds_read_b128 %2, %7\n\tds_read_b128 %3, %8\n\t"
        "ds_read_b32 %4, %9\n\t"
        "s_waitcnt lgkmcnt(0)"
        : "=&v"(v0), "=&v"(v1), "=&v"(v2), "=&v"(v3), "=&v"(out32)
        : "v"(addr[0]), "v"(addr[1]), "v"(addr[2]), "v"(addr[3]), "v"(addr32)
        : "memory");
    out[0] = __builtin_bit_cast(uint4, v0); out[1] = __builtin_bit_cast(uint4, v1); out[2] = __builtin_bit_cast(uint4, v2);
    out[3] = __builtin_bit_cast(uint4, v3);
    out[4] = out[5] = out[6] = out[7] = make_uint4(0u, 0u, 0u, 0u);     // ("lo": never multiplied by the one-product filter)
}
template <int M>
__device__ __forceinline__ void lds_read_ops(const uint32_t (&addr)[8], uint4 (&out)[8], uint32_t addr32, float& out32) {
    if (M == 1) lds_read4_b128(addr, out, addr32, out32); else lds_read8_b128(addr, out, addr32, out32);
}
// third smallest of two sorted triples (K: the 64-bit merge keys, or the 32-bit record keys below)
template <class K>
__device__ __forceinline__ K third_of_two_triples(K a0, K a1, K a2, K b0, K b1, K b2) {
    const K x = a1 > b0 ? a1 : b0, y = a0 > b1 ? a0 : b1;
    K m = a2 < b2 ? a2 : b2;
    m = m < x ? m : x;
    return m < y ? m : y;
}
// The two halves of a query's rows meet (lanes l and l ^ 32 hold the sorted triples of the same query): the best two of the six keys and the
// third, the bound on everything dropped.
__device__ __forceinline__ uint32_t shfl_xor_key(uint32_t v, int m) { return (uint32_t)__shfl_xor((int)v, m, 64); }
__device__ __forceinline__ uint64_t shfl_xor_key(uint64_t v, int m) { return shfl_xor_u64(v, m); }
template <class K>
__device__ __forceinline__ void merge_halves(K a0, K a1, K a2, K& m0, K& m1, K& third) {
    const K b0 = shfl_xor_key(a0, 32), b1 = shfl_xor_key(a1, 32), b2 = shfl_xor_key(a2, 32);
    m0 = a0 < b0 ? a0 : b0;
    const K hx = a0 < b0 ? b0 : a0, lx = a1 < b1 ? a1 : b1;
    m1 = hx < lx ? hx : lx;
    third = third_of_two_triples(a0, a1, a2, b0, b1, b2);
}

// ---- what a filter hands to the re-rank: one record per (row block, query), block-major ([n_blocks][qpad]: the filter's lanes own consecutive
// queries of ONE block, so its records leave as full lines -- a wave's 32 queries make one 512-byte write; query-major they were 16-byte
// pieces of 112 000 different lines per frame, and the write-back of those partial lines at the end of the launch was a third of launch
// A's wall time).  The record type is the filter's:
//   StripRecord  (the 64-float filters, whose block is ONE strip): 16 bytes, stored with one instruction and fetched with one request.  The two
//                kept keys stay 32-bit strip keys; the block's first tile follows from the block index, and the half of the tile's rows the
//                key's lane held travels in bit 0 of the index -- the filters select 4-row groups (push_group4, bf_pair: index 4 st), so the
//                index's two low bits are free and the score keeps every bit it has in a strip key.  record_key() writes a key,
//                record_widen() -- the one place that calls widen_key for these filters -- rebuilds the merge key on the reader's side.
//   ShareRecords (the 128- / 256-float filter, wide_filter_body.cuh): a share is up to FOUR strips; strip, tile and group fill the index's
//                seven bits, so no bit is left for the half: that filter keeps two 64-bit merge keys and the bound in arrays of their own.
struct __attribute__((aligned(16))) StripRecord { uint32_t key[BF_KEEP]; uint32_t bound; uint32_t spare; };
static_assert(sizeof(StripRecord) == 16 && BF_KEEP == 2, "one 16-byte store, one 16-byte request");
constexpr uint32_t REC_KEY_NONE = (uint32_t)MF_KEY_NONE;
constexpr uint32_t REC_HALF_BIT = 1u;
static_assert((MF_IDX_MASK & 3u) == 3u && REC_HALF_BIT < 4u, "the group index leaves the two low index bits free");
// strip key of a 4-row group (lane half `half`) -> record key.  A slightly negative score (rounding of a distance ~ 0) becomes +0 HERE, so that
// record keys compare (unsigned) exactly as the merge keys they widen to: score bits, then tile, group and half = score bits, then row.
__device__ __forceinline__ uint32_t record_key(int32_t k, int half) {
    if (k == MF_KEY_NONE) return REC_KEY_NONE;
    return (k < 0 ? ((uint32_t)k & MF_IDX_MASK) : (uint32_t)k) | (half ? REC_HALF_BIT : 0u);
}
// record key -> merge key (score bits << 32 | the group's first vocabulary row); tile0: the first tile of the record's block
__device__ __forceinline__ uint64_t record_widen(uint32_t k, int tile0) {
    if (k == REC_KEY_NONE) return KEY_NONE;
    return widen_key((int32_t)(k & ~REC_HALF_BIT), tile0, (int)(k & REC_HALF_BIT));
}
// the score bits of a record key (KEY_NONE -> +inf), without the row
__device__ __forceinline__ uint32_t record_score(uint32_t k) { return k == REC_KEY_NONE ? 0x7f800000u : min(k & ~MF_IDX_MASK, 0x7f800000u); }
struct ShareRecords { uint64_t* keys; uint32_t* bound; };        // keys [n_blocks][qpad][BF_KEEP], bound [n_blocks][qpad] f32 bits

// ---- same-frame distance matrix, computed by extra workgroups of the filter launch (independent of the 2-NN; a launch of its own
// costs more than the work).  One workgroup = one 64 x 64 tile of the upper triangle of D[r][c] = |q_r - q_c|^2 in the reference's
// arithmetic (dist.h:150-177; (a - b)^2 == (b - a)^2 bit for bit, so the mirrored tile is a copy).  Both 64-query tiles are staged
// in LDS (16-byte chunks XOR-swizzled by the row so that lanes with different queries read conflict-free); a thread owns a 4 x 4 block
// of the tile (rows ty + 16 m, columns tx + 16 n), so a 16-byte LDS read feeds four outputs.  64 x 64 and not 32 x 32: every workgroup
// of the launch holds a whole compute unit's LDS, and 500 descriptors are 36 tiles -- which fit on the compute units the 192 filter
// workgroups leave free -- instead of 136, which did not (the launch then ran in two rounds: 23 us instead of 15).
struct SelfdistJob {
    const float* queries = nullptr;    // [nq x 64]
    int nq = 0;
    float* out = nullptr;              // [nq x ld]
    int ld = 0;
    int n_tiles = 0;                   // workgroups: n_self + the cross-frame tiles; 0 = no job
    int n_self = 0;                    // T (T + 1) / 2, T = ceil(nq / 64): the tiles of the upper triangle of the same-frame matrix (0: not asked for)
    // cross-frame tiles (round 5): X[r][c] = |q_r - o_c|^2 against the descriptors of the frame BEFORE this one, ceil(nq / 64) x ceil(n_other / 64)
    // full tiles.  The rows that frame appends to the vocabulary ARE descriptors of it, and this frame's re-rank (launch B of the same pair) has to
    // scan them exactly -- they are not in the filter's snapshot.  With this matrix that scan is one gathered read per pending row instead of
    // 38 KB of rows staged through LDS by each of 250 workgroups (+9.6 MB per launch) and ~150 distances per query.
    const float* other = nullptr; int n_other = 0;
    float* xout = nullptr; int xld = 0;
};
inline int selfdist_tiles(int q) { const int T = (q + 63) / 64; return T * (T + 1) / 2; }
__device__ __forceinline__ void selfdist_tile(const SelfdistJob& sd, int k, float* __restrict__ lds) {
    const int T = (sd.nq + 63) / 64;
    const bool xj = k >= sd.n_self;                    // uniform: a cross-frame tile
    const float* __restrict__ colsrc = xj ? sd.other : sd.queries;
    const int ncol = xj ? sd.n_other : sd.nq;
    float* __restrict__ out = xj ? sd.xout : sd.out;
    const int ld = xj ? sd.xld : sd.ld;
    int ti = 0, tj;
    if (xj) {
        const int Tc = (ncol + 63) / 64;
        ti = (k - sd.n_self) / Tc; tj = (k - sd.n_self) % Tc;
    } else {
        int rem = k;
        while (rem >= T - ti) { rem -= T - ti; ++ti; }
        tj = ti + rem;
    }
    const int tid = threadIdx.x;
    const bool act = tid < 256;                        // the tile is the work of 256 threads; a larger workgroup's other threads idle
    float* sA = lds;                   // rows of tile ti   [64][64] swizzled
    float* sB = lds + 4096;            // rows of tile tj
    float* sT = lds + 8192;            // [64][65] transposed result
    if (act) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int e = tid + u * 256;                   // float4 index within a tile: row e / 16, chunk e % 16
            const int r = e >> 4, c = e & 15;
            const int ra = min(ti * 64 + r, sd.nq - 1), rb = min(tj * 64 + r, ncol - 1);
            const float4 a = reinterpret_cast<const float4*>(sd.queries + (size_t)ra * 64)[c];
            const float4 b = reinterpret_cast<const float4*>(colsrc + (size_t)rb * 64)[c];
            *reinterpret_cast<float4*>(sA + r * 64 + ((c ^ (r & 15)) << 2)) = a;
            *reinterpret_cast<float4*>(sB + r * 64 + ((c ^ (r & 15)) << 2)) = b;
        }
    }
    __syncthreads();
    const int tx = tid & 15, ty = (tid >> 4) & 15;     // columns tx + 16 n of tile tj; rows ty + 16 m of tile ti
    if (act) {
        float res[4][4];
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int n = 0; n < 4; ++n) res[m][n] = 0.0f;
#pragma unroll 2
        for (int g = 0; g < 16; ++g) {
            float4 a[4], b[4];
#pragma unroll
            for (int m = 0; m < 4; ++m) { const int r = ty + 16 * m; a[m] = *reinterpret_cast<const float4*>(sA + r * 64 + ((g ^ (r & 15)) << 2)); }
#pragma unroll
            for (int n = 0; n < 4; ++n) { const int c = tx + 16 * n; b[n] = *reinterpret_cast<const float4*>(sB + c * 64 + ((g ^ (c & 15)) << 2)); }
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
                for (int n = 0; n < 4; ++n) {
                    const float d0 = __fsub_rn(a[m].x, b[n].x), d1 = __fsub_rn(a[m].y, b[n].y), d2 = __fsub_rn(a[m].z, b[n].z), d3 = __fsub_rn(a[m].w, b[n].w);
                    float t = __fmul_rn(d0, d0);
                    t = __fadd_rn(t, __fmul_rn(d1, d1));
                    t = __fadd_rn(t, __fmul_rn(d2, d2));
                    t = __fadd_rn(t, __fmul_rn(d3, d3));
                    res[m][n] = __fadd_rn(res[m][n], t);
                }
        }
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                const int r = ti * 64 + ty + 16 * m, c = tj * 64 + tx + 16 * n;
                if (r < sd.nq && c < ncol) out[(size_t)r * ld + c] = res[m][n];
                sT[(ty + 16 * m) * 65 + tx + 16 * n] = res[m][n];
            }
    }
    if (xj || ti == tj) return;                        // uniform
    __syncthreads();
    if (act) {
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int n = 0; n < 4; ++n) {              // mirrored tile: D[tj*64 + x][ti*64 + y] = D[ti*64 + y][tj*64 + x]
                const int x = ty + 16 * m, y = tx + 16 * n;
                const int r = tj * 64 + x, cc = ti * 64 + y;
                if (r < sd.nq && cc < sd.nq) sd.out[(size_t)r * sd.ld + cc] = sT[y * 65 + x];
            }
    }
}

// ---- the pieces the filter bodies below share (one strip per workgroup, pre-split queries, persistent, and in part the shadow scores).
// Those that fill operands or store keys work on ONE query group (one-dimensional arrays, scalars), the loop over the groups stays with the
// caller, and the A-operand read of a tile is left in each body on purpose: written over the bodies' [BF_NG][4] arrays, or around that
// read, the same text compiles to different tile loops and register counts (profiles/refactor_filter_helpers_isa.txt).

// LDS address of 16-byte chunk `chunk` of the tile row that starts at `row_base` (XOR swizzle, see dma_a_tile)
__device__ __forceinline__ uint32_t a_chunk_addr(uint32_t row_base, int chunk, int col) { return row_base + ((((uint32_t)chunk) ^ (uint32_t)(col & 15)) << 4); }

// B operands of one 32-query group from the wave's staging area: -2 q split hi/lo in operand order (lane (query l&31, half l>>5) holds
// floats [32h, 32h + 32) of its query: k-step s multiplies elements 32h + 8s .. + 8 -- A uses the same k permutation), + |q|^2 for the
// augmentation step
template <int M>
__device__ __forceinline__ void split_query_group(const float* s_q, int col, int half, uint4 (&bh)[4], uint4 (&bl)[4], float& b_aug) {
    constexpr int KH = 32;
    float x[KH];
    read_a_tile<KH>(s_q, col, half, x);
    float part = 0.0f;
#pragma unroll
    for (int k = 0; k < KH; ++k) part = fmaf(x[k], x[k], part);
    const float qn = part + __shfl_xor(part, 32, 64);
    b_aug = half == 0 ? 1.0f : qn;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        op_split2<M>(-2.0f * x[8 * s + 0], -2.0f * x[8 * s + 1], bh[s].x, bl[s].x);
        op_split2<M>(-2.0f * x[8 * s + 2], -2.0f * x[8 * s + 3], bh[s].y, bl[s].y);
        op_split2<M>(-2.0f * x[8 * s + 4], -2.0f * x[8 * s + 5], bh[s].z, bl[s].z);
        op_split2<M>(-2.0f * x[8 * s + 6], -2.0f * x[8 * s + 7], bh[s].w, bl[s].w);
    }
}

// One tile against the wave's four query groups.  Two accumulator pairs take turns (no copies): groups 0,1 are computed into (x0, x1)
// while the pending scores of groups 2,3 of the previous tile (p0, p1) are pushed, then groups 2,3 into (p0, p1) while (x0, x1) are
// pushed.  `first`: the strip's first tile, nothing is pending.  tl = the tile's index in the strip.
template <int M>
__device__ __forceinline__ void tile_trip(bool first, uint32_t tl, const uint4 (&ah)[4], const uint4 (&al)[4], float aug, const uint4 (&bh)[BF_NG][4],
                                          const uint4 (&bl)[BF_NG][4], const float (&b_aug)[BF_NG], f32x16& p0, f32x16& p1, int32_t (&k0)[BF_NG],
                                          int32_t (&k1)[BF_NG], int32_t (&k2)[BF_NG]) {
    f32x16 x0, x1;
    if (first) bf_pair<false, M>(ah, al, aug, bh[0], bl[0], b_aug[0], bh[1], bl[1], b_aug[1], x0, x1, p0, p1, 0u, k0[2], k1[2], k2[2], k0[3], k1[3], k2[3]);
    else bf_pair<true, M>(ah, al, aug, bh[0], bl[0], b_aug[0], bh[1], bl[1], b_aug[1], x0, x1, p0, p1, tl - 1u, k0[2], k1[2], k2[2], k0[3], k1[3], k2[3]);
    bf_pair<true, M>(ah, al, aug, bh[2], bl[2], b_aug[2], bh[3], bl[3], b_aug[3], p0, p1, x0, x1, tl, k0[0], k1[0], k2[0], k0[1], k1[1], k2[1]);
}
// behind a strip's last tile (index tlast): the scores tile_trip left pending
__device__ __forceinline__ void flush_pending(const f32x16& p0, const f32x16& p1, uint32_t tlast, int32_t (&k0)[BF_NG], int32_t (&k1)[BF_NG],
                                              int32_t (&k2)[BF_NG]) {
    push_group4(p0, tlast, k0[BF_NG - 2], k1[BF_NG - 2], k2[BF_NG - 2]);
    push_group4(p1, tlast, k0[BF_NG - 1], k1[BF_NG - 1], k2[BF_NG - 1]);
}

// The two halves of a query's rows meet in registers: best two of the six keys, and the third as the bound on everything this workgroup
// dropped for the query (qi; row block bx) -- one StripRecord, records[bx][qi], one 16-byte store.
__device__ __forceinline__ void merge_store_keys(int32_t k0, int32_t k1, int32_t k2, int half, int qi, int qpad, int bx, StripRecord* __restrict__ records) {
    uint32_t m0, m1, third;
    merge_halves(record_key(k0, half), record_key(k1, half), record_key(k2, half), m0, m1, third);
    if (half == 0 && qi < qpad)
        *reinterpret_cast<uint4*>(records + (size_t)bx * qpad + qi) = make_uint4(m0, m1, record_score(third), 0u);
}

// The one-strip filter.  Grid (1-D): n_blocks x ceil(nq / 512) filter workgroups first, then sd.n_tiles distance-matrix workgroups.
template <int M>
__device__ __forceinline__ void knn_bf16_filter_body(float* s_dyn, int bid, const float* __restrict__ vocab_bf, const float* __restrict__ row_norm,
                                                     int n_rows, const float* __restrict__ queries, int nq, int qpad,
                                                     int tiles_per_block, int n_blocks, StripRecord* __restrict__ records, const SelfdistJob& sd,
                                                     const int32_t* __restrict__ n_lo = nullptr) {
    // n_lo: the number of rows this search may see, on the device (a pipelined handle appends the previous frames' new words while
    // this launch runs: rows at or beyond n_lo[0] -- up to n_rows, the host's upper bound -- are masked with an infinite |row|^2)
    // (n_rows itself may be an ESTIMATE below the device's count -- the launch plan of a growing vocabulary: nothing at or beyond it is
    // ranked either, the re-rank scans from min(n_rows, n_lo[0]) on)
    const int lo_rows = min(n_lo ? n_lo[0] : 0x7fffffff, n_rows);
    constexpr int NG = BF_NG;
    constexpr int KH = 32;
    constexpr int NW = MF_WAVES;                   // waves per workgroup
    constexpr int QW = BF_QW;                      // queries per wave
    constexpr int DPW = 8 / NW;                    // DMA instructions of a tile issued by one wave
    // the filter workgroups come FIRST in the grid: a workgroup holds a whole compute unit's LDS, workgroups are dispatched in index order,
    // and the (short) distance-matrix tiles in front used to take 136 of the 256 compute units at the start of the launch -- a third of the
    // filter workgroups then began only when a tile, or another filter workgroup, had finished (entry spread 0 .. 12 us for a 12 us workgroup)
    const int n_fwg = n_blocks * ((nq + BF_QB - 1) / BF_QB);
    if (bid >= n_fwg) { selfdist_tile(sd, bid - n_fwg, s_dyn); return; }
    const int fb = bid;
    const int bx = fb % n_blocks, by = fb / n_blocks;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int col = lane & 31, half = lane >> 5;
    const int q0 = by * BF_QB + wave * QW;
    float* s_q = s_dyn + (size_t)wave * NG * BF_TILE_F;             // this wave's query staging (prologue only)
    float* s_tile = s_dyn + (size_t)NW * NG * BF_TILE_F;      // [2] vocabulary tiles shared by the workgroup
    float* s_aug = s_tile + 2 * BF_TILE_F;                    // [MF_STRIP_TILES][64] augmentation entries of the strip, per lane
    MF_STAMP(0);

    const int tile0 = bx * tiles_per_block;
    const int n_tiles = (n_rows + 31) / 32;
    const int tile1 = min(tile0 + tiles_per_block, n_tiles);

    // Everything the prologue needs is put in flight at once: the wave's query groups, its share of the first TWO vocabulary tiles
    // and the augmentation entries of every tile of the strip.  The strip's other tiles follow as soon as the query staging area
    // is free (below): the whole strip is requested long before it is needed -- with one tile of look-ahead the loop ran at the
    // memory LATENCY (a tile trip is shorter than a round trip to HBM), not at the matrix rate.
#pragma unroll
    for (int g = 0; g < NG; ++g) dma_a_tile<KH>(queries, nq, q0 / 32 + g, lane, s_q + g * BF_TILE_F);
    float augs[MF_STRIP_TILES];
#pragma unroll
    for (int i = 0; i < MF_STRIP_TILES; ++i) {
        const int t = min(tile0 + i, max(tile1 - 1, tile0));
        augs[i] = row_norm[2 * (size_t)min(t * 32 + col, n_rows) + half];
    }
    if (tile0 < tile1) {
        dma_tile_part<M == 1>(vocab_bf, n_rows, tile0, lane, s_tile, DPW * wave, DPW * wave + DPW);
        dma_tile_part<M == 1>(vocab_bf, n_rows, min(tile0 + 1, tile1 - 1), lane, s_tile + BF_TILE_F, DPW * wave, DPW * wave + DPW);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (wave == 0) {                                                 // the loop takes them from LDS: a VMEM load there would wait behind the whole prefetch
#pragma unroll
        for (int i = 0; i < MF_STRIP_TILES; ++i) {
            const int t = min(tile0 + i, max(tile1 - 1, tile0));
            s_aug[i * 64 + lane] = (half == 0 && t * 32 + col >= lo_rows) ? __int_as_float(0x7f800000) : augs[i];
        }
    }

    uint4 bh[NG][4], bl[NG][4];
    float b_aug[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) split_query_group<M>(s_q + g * BF_TILE_F, col, half, bh[g], bl[g], b_aug[g]);

    int32_t k0[NG], k1[NG], k2[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) { k0[g] = MF_KEY_NONE; k1[g] = MF_KEY_NONE; k2[g] = MF_KEY_NONE; }
    f32x16 p0, p1;                                                   // pending accumulators (groups NG-2, NG-1 of the previous tile)
    // every wave has its queries in registers (and the first two tiles have landed for everybody): the staging area now takes
    // tiles 2.. of the strip, all requested at once
    __syncthreads();
    for (int t = tile0 + 2; t < tile1; ++t)
        dma_tile_part<M == 1>(vocab_bf, n_rows, t, lane, s_dyn + (size_t)(t - tile0 - 2) * BF_TILE_F, DPW * wave, DPW * wave + DPW);
    MF_STAMP(1);
    for (int t = tile0; t < tile1; ++t) {
        const int ti = t - tile0;
        MF_STAMP2(ti);
        if (ti == 2) {                                               // tiles 2.. : one wait and one barrier for all of them
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
        }
        // A operands: hi chunks 4h .. 4h+3 and lo chunks 8+4h .. 8+4h+3 of row `col` (16-byte chunks, XOR-swizzled).  The reads
        // are issued as inline assembly: the compiler orders every LDS read it knows of behind ALL outstanding LDS-DMA
        // (s_waitcnt vmcnt(0)), which would serialise the loop behind the strip's prefetch.
        uint4 ah[4], al[4];
        float aug;
        {
            const float* slot = ti < 2 ? s_tile + ti * BF_TILE_F : s_dyn + (size_t)(ti - 2) * BF_TILE_F;
            const uint32_t base = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const void*)(slot + col * 64);
            uint32_t addr[8];
            uint4 av[8];
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                addr[v] = a_chunk_addr(base, 4 * half + v, col);
                addr[4 + v] = a_chunk_addr(base, 8 + 4 * half + v, col);
            }
            lds_read_ops<M>(addr, av, (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const void*)(s_aug + ti * 64 + lane), aug);
#pragma unroll
            for (int v = 0; v < 4; ++v) { ah[v] = av[v]; al[v] = av[4 + v]; }
        }
        tile_trip<M>(t == tile0, (uint32_t)ti, ah, al, aug, bh, bl, b_aug, p0, p1, k0, k1, k2);
    }
    if (tile0 < tile1) flush_pending(p0, p1, (uint32_t)(tile1 - 1 - tile0), k0, k1, k2);
    MF_STAMP(2);
#pragma unroll
    for (int g = 0; g < NG; ++g) merge_store_keys(k0[g], k1[g], k2[g], half, q0 + g * 32 + col, qpad, bx, records);
    MF_STAMP(3);
}

// ------------------------------------------------------------------------------------------------ pre-split queries (pipelined frames)
// Every strip's workgroup of the body above stages the SAME 512 queries through 128 KB of LDS and splits them into bf16 operands --
// 192 times per frame, and the staging area is what makes a filter workgroup own a whole compute unit's LDS.  A pipelined handle
// knows a frame one launch before its filter runs: the launch that carries the previous frame's filter also converts the new
// frame's queries ONCE (qsplit_body, a handful of small workgroups) into MFMA operand order in global memory:
//     qsplit[(((query / 32) * 4 + s) * 2 + kind) * 64 + lane]   uint4 = eight bf16 of  -2 q[32 * (lane >> 5) + 8 s .. + 8)  (kind 0: hi, 1: lo)
//     qnorm[query] = |q|^2
// so that the filter's prologue is 32 coalesced 16-byte loads per lane straight into the registers the operands live in, its LDS holds
// only the strip (8 tiles + augmentation entries = 66 KB) and TWO workgroups share a compute unit.
constexpr size_t BF_LDS_BYTES_Q = (size_t)MF_STRIP_TILES * BF_TILE_F * 4 + (size_t)MF_STRIP_TILES * 64 * 4;

__device__ __forceinline__ void qsplit_item(const QSplitArgs& qs, int t, const float4& a, const float4& b, uint32_t nm_seen) {
    const int qi = t >> 3, h = (t >> 2) & 1, sx = t & 3;
    uint4 hi, lo;
    op_split2_rt(qs.f16, -2.0f * a.x, -2.0f * a.y, hi.x, lo.x);
    op_split2_rt(qs.f16, -2.0f * a.z, -2.0f * a.w, hi.y, lo.y);
    op_split2_rt(qs.f16, -2.0f * b.x, -2.0f * b.y, hi.z, lo.z);
    op_split2_rt(qs.f16, -2.0f * b.z, -2.0f * b.w, hi.w, lo.w);
    const size_t base = ((size_t)(qi >> 5) * 4 + sx) * 2;
    qs.qsplit[(base + 0) * 64 + h * 32 + (qi & 31)] = hi;
    qs.qsplit[(base + 1) * 64 + h * 32 + (qi & 31)] = lo;
    float part = fmaf(b.w, b.w, fmaf(b.z, b.z, fmaf(b.y, b.y, fmaf(b.x, b.x, fmaf(a.w, a.w, fmaf(a.z, a.z, fmaf(a.y, a.y, a.x * a.x)))))));
    part += __shfl_xor(part, 1, 64);
    part += __shfl_xor(part, 2, 64);
    part += __shfl_xor(part, 4, 64);
    if ((t & 7) == 0) qs.qnorm[qi] = part;
    if (qs.shadow_bf) {                                                  // the descriptor as a ROW of an operand table (vocab_bf16_kernel's layout): floats [32 h + 8 sx, + 8)
        uint4 rh, rl;
        op_split2_rt(qs.f16, a.x, a.y, rh.x, rl.x);
        op_split2_rt(qs.f16, a.z, a.w, rh.y, rl.y);
        op_split2_rt(qs.f16, b.x, b.y, rh.z, rl.z);
        op_split2_rt(qs.f16, b.z, b.w, rh.w, rl.w);
        uint4* row = reinterpret_cast<uint4*>(qs.shadow_bf + (size_t)qi * 64);
        row[4 * h + sx] = rh;
        row[8 + 4 * h + sx] = rl;
        if ((t & 7) == 0) {                                              // padding rows (they repeat the last descriptor) never rank: |row|^2 = +inf
            qs.shadow_norm[2 * (size_t)qi] = qi < qs.nq ? part : __int_as_float(0x7f800000);
            qs.shadow_norm[2 * (size_t)qi + 1] = 1.0f;
            if (t == 0) { qs.shadow_norm[2 * (size_t)qs.qpad] = __int_as_float(0x7f800000); qs.shadow_norm[2 * (size_t)qs.qpad + 1] = 1.0f; }   // the sentinel
        }
        // the filter's error bound is made from the largest |row|^2 the filter may have multiplied: these rows are among them from the next launch on
        // (a running maximum: raising it early only widens the bound); one atomic per wave that holds something above what the maximum was seen
        // to be (nm_seen, running_max_seen): the frames of a stream have norms alike, so after the first ones hardly any wave does
        float nm = qi < qs.nq ? part : 0.0f;
#pragma unroll
        for (int m = 32; m >= 8; m >>= 1) nm = fmaxf(nm, __shfl_xor(nm, m, 64));
        if (qs.norm_max_bits && (threadIdx.x & 63) == 0 && nm > 0.0f && __float_as_uint(nm) > nm_seen) atomicMax(qs.norm_max_bits, __float_as_uint(nm));
    }
}
// One item = eight floats of one query.  A thread's items are READ first and written afterwards: loads and stores share one in-order
// counter, so a second trip's loads behind a first trip's stores wait for a store round trip that carries no data (round 4's stamps:
// the eight two-trip workgroups took 17 us, the longest chain of launch A).  Frames of up to 1 024 descriptors get one item per thread.
__device__ __forceinline__ void qsplit_body(const QSplitArgs& qs, int wg) {
    const int n_items = qs.qpad * 8, stride = qs.n_wgs * (int)blockDim.x;   // (qpad * 8 is a multiple of 64: a wave's lanes take part together)
    const uint32_t nm_seen = qs.shadow_bf ? running_max_seen(qs.norm_max_bits) : 0u;
    for (int t0 = wg * (int)blockDim.x + (int)threadIdx.x; t0 < n_items; t0 += 2 * stride) {
        const int t1 = t0 + stride;
        const bool two = t1 < n_items;
        const int tt = two ? t1 : t0;
        const float4* s0 = reinterpret_cast<const float4*>(qs.queries + (size_t)min(t0 >> 3, qs.nq - 1) * 64 + 32 * ((t0 >> 2) & 1) + 8 * (t0 & 3));   // padding repeats the last query
        const float4* s1 = reinterpret_cast<const float4*>(qs.queries + (size_t)min(tt >> 3, qs.nq - 1) * 64 + 32 * ((tt >> 2) & 1) + 8 * (tt & 3));
        const float4 a0 = s0[0], b0 = s0[1], a1 = s1[0], b1 = s1[1];
        qsplit_item(qs, t0, a0, b0, nm_seen);
        if (two) qsplit_item(qs, t1, a1, b1, nm_seen);
    }
}

// B operands of 32-query group `grp` straight from the table into the registers they live in
__device__ __forceinline__ void load_group_presplit(const uint4* qsplit, const float* qnorm, int grp, int qpad, int lane, int col, int half,
                                                    uint4 (&bh)[4], uint4 (&bl)[4], float& b_aug) {
#pragma unroll
    for (int sx = 0; sx < 4; ++sx) {
        const size_t base = ((size_t)grp * 4 + sx) * 2;
        bh[sx] = qsplit[(base + 0) * 64 + lane];
        bl[sx] = qsplit[(base + 1) * 64 + lane];
    }
    const float qn = qnorm[min(grp * 32 + col, qpad - 1)];
    b_aug = half == 0 ? 1.0f : qn;
}

// the filter body over pre-split queries: as knn_bf16_filter_body (one strip per workgroup), without the query staging
template <int M>
__device__ __forceinline__ void knn_bf16_filter_body_q(float* s_dyn, int bid, const float* __restrict__ vocab_bf, const float* __restrict__ row_norm,
                                                       int n_rows, const uint4* qsplit, const float* qnorm, int nq, int qpad,
                                                       int tiles_per_block, int n_blocks, StripRecord* __restrict__ records, const SelfdistJob& sd,
                                                       const int32_t* __restrict__ n_lo) {
    constexpr int NG = BF_NG;
    constexpr int NW = MF_WAVES;
    constexpr int QW = BF_QW;
    constexpr int DPW = 8 / NW;
    // the rows this search may see (see knn_bf16_filter_body), through the scalar cache: a vector load would sit in the same in-order
    // queue as the strip's requests below, and its first use would wait for all of them
    int lo_rows = 0x7fffffff;
    if (n_lo) asm volatile("s_load_dword %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(lo_rows) : "s"(n_lo) : "memory");
    lo_rows = min(lo_rows, n_rows);                                       // (the plan's n_rows may be an estimate below the device's count)
    const int n_fwg = n_blocks * ((nq + BF_QB - 1) / BF_QB);
    if (bid >= n_fwg) { selfdist_tile(sd, bid - n_fwg, s_dyn); return; }
    const int bx = bid % n_blocks, by = bid / n_blocks;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int col = lane & 31, half = lane >> 5;
    const int q0 = by * BF_QB + wave * QW;
    float* s_aug = s_dyn + (size_t)MF_STRIP_TILES * BF_TILE_F;          // [MF_STRIP_TILES][64]
    MF_STAMP(0);
    const int tile0 = bx * tiles_per_block;
    const int n_tiles = (n_rows + 31) / 32;
    const int tile1 = min(tile0 + tiles_per_block, n_tiles);
    // First what the loop needs to start -- two tiles, the augmentation entries, the query operands -- and, once that has arrived, the
    // rest of the strip, which lands while the first two tiles are multiplied.  (Requested all at once and awaited in front of the loop,
    // the strip cost 3.6 us per workgroup: every workgroup of the launch asks at the same moment, so the last byte of anybody's strip
    // arrives when the whole vocabulary has crossed the fabric.  Requested all at once and awaited tile by tile is not expressible:
    // the compiler waits for EVERY outstanding request at the first use of an operand register while LDS-DMA is in flight.)
    const int tile_last = max(tile1 - 1, tile0);
    dma_tile_part<M == 1>(vocab_bf, n_rows, tile0, lane, s_dyn, DPW * wave, DPW * wave + DPW);
    dma_tile_part<M == 1>(vocab_bf, n_rows, min(tile0 + 1, tile_last), lane, s_dyn + BF_TILE_F, DPW * wave, DPW * wave + DPW);
    // the augmentation entries of the strip go straight to LDS as well, two tiles per wave (the mask of rows that do not exist yet
    // is patched into them below)
    static_assert(MF_STRIP_TILES == 2 * NW, "two augmentation rows per wave");
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int i = 2 * wave + j;
        const int t = min(tile0 + i, tile_last);
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(row_norm + 2 * (size_t)min(t * 32 + col, n_rows) + half),
                                         (__attribute__((address_space(3))) void*)(s_aug + i * 64), 4, 0, 0);
    }
    uint4 bh[NG][4], bl[NG][4];
    float b_aug[NG];
    const int grp0 = q0 >> 5;
    const int n_grp = qpad >> 5;
#pragma unroll
    for (int g = 0; g < NG; ++g)                                        // (a wave beyond the padded queries repeats the last group: its keys are not written)
        load_group_presplit(qsplit, qnorm, min(grp0 + g, n_grp - 1), qpad, lane, col, half, bh[g], bl[g], b_aug[g]);
    // (a use of the youngest request here: the compiler waits for it -- and with it for everything older -- at this point, and knows
    // from then on that the operand registers are complete; left alone it would wait at their first use, behind the requests below)
    asm volatile("" : "+v"(b_aug[NG - 1]) : : "memory");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    for (int t = tile0 + 2; t < tile1; ++t)
        dma_tile_part<M == 1>(vocab_bf, n_rows, t, lane, s_dyn + (size_t)(t - tile0) * BF_TILE_F, DPW * wave, DPW * wave + DPW);
    if ((tile0 + MF_STRIP_TILES) * 32 > lo_rows) {                       // (rare: the strip reaches rows that are being appended while this launch runs)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int i = 2 * wave + j;
            if (half == 0 && (tile0 + i) * 32 + col >= lo_rows)
                asm volatile("ds_write_b32 %0, %1" ::"v"((uint32_t)(uintptr_t)(__attribute__((address_space(3))) void*)(s_aug + i * 64 + lane)),
                             "v"(__int_as_float(0x7f800000)) : "memory");
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
    __builtin_amdgcn_s_barrier();                                        // every wave's share of tiles 0, 1 and the augmentation entries are in LDS
    MF_STAMP(1);
    int32_t k0[NG], k1[NG], k2[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) { k0[g] = MF_KEY_NONE; k1[g] = MF_KEY_NONE; k2[g] = MF_KEY_NONE; }
    f32x16 p0, p1;
    for (int t = tile0; t < tile1; ++t) {
        const int ti = t - tile0;
        if (ti == 2) {                                                   // tiles 2.. : one wait and one barrier for all of them
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
        }
        uint4 ah[4], al[4];
        float aug;
        {
            const float* slot = s_dyn + (size_t)ti * BF_TILE_F;
            const uint32_t base = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const void*)(slot + col * 64);
            uint32_t addr[8];
            uint4 av[8];
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                addr[v] = a_chunk_addr(base, 4 * half + v, col);
                addr[4 + v] = a_chunk_addr(base, 8 + 4 * half + v, col);
            }
            lds_read_ops<M>(addr, av, (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const void*)(s_aug + ti * 64 + lane), aug);
#pragma unroll
            for (int v = 0; v < 4; ++v) { ah[v] = av[v]; al[v] = av[4 + v]; }
        }
        tile_trip<M>(t == tile0, (uint32_t)ti, ah, al, aug, bh, bl, b_aug, p0, p1, k0, k1, k2);
    }
    if (tile0 < tile1) flush_pending(p0, p1, (uint32_t)(tile1 - 1 - tile0), k0, k1, k2);
    MF_STAMP(2);
#pragma unroll
    for (int g = 0; g < NG; ++g) merge_store_keys(k0[g], k1[g], k2[g], half, q0 + g * 32 + col, qpad, bx, records);
    MF_STAMP(3);
}

// ------------------------------------------------------------------------------------------------ shadow scores (round 6)
// The words frame t-2 is about to create (its decision loop rides in THIS launch) are not rows of the vocabulary when the filter of frame t-1 runs
// beside it -- but they are descriptors of frame t-2, and that frame's query pre-split left ALL its descriptors as rows of an operand table (256 B
// each, the layout of vocab_bf; QSplitArgs::shadow_bf).  One workgroup per 32-row tile of that table multiplies it with the frame's 512 pre-split
// queries exactly as a filter strip does (the same MFMA chains on top of |v|^2 + |q|^2: the same error bound) and -- instead of selecting -- writes
// every score: x[query][descriptor], ld floats per query.  Launch B's re-rank, which knows by then which of those descriptors became words, reads
// its query's row, keeps the words' scores at or below its threshold and evaluates them exactly with its other candidates (knn_mfma_rerank_body):
// nobody stages or scans the ~150 new rows any more (250 workgroups x 38 KB and ~4.5 us of the re-rank's chain in round 5).
template <int M>
__device__ __forceinline__ void shadow_scores_body(float* s_dyn, int wg, const float* __restrict__ sh_bf, const float* __restrict__ sh_norm, int sh_rows,
                                                   const uint4* qsplit, const float* qnorm, int nq, int qpad, float* __restrict__ x, int ld) {
    constexpr int NG = BF_NG, NW = MF_WAVES, QW = BF_QW, DPW = 8 / NW;
    const int n_tiles = (sh_rows + 31) / 32;
    const int t = wg % n_tiles, by = wg / n_tiles;                       // tile of the table, block of 512 queries
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int col = lane & 31, half = lane >> 5;
    const int q0 = by * BF_QB + wave * QW;
    float* s_aug = s_dyn + (size_t)BF_TILE_F;
    dma_tile_part<M == 1>(sh_bf, sh_rows, t, lane, s_dyn, DPW * wave, DPW * wave + DPW);
    if (wave == 0)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(sh_norm + 2 * (size_t)min(t * 32 + col, sh_rows) + half),
                                         (__attribute__((address_space(3))) void*)s_aug, 4, 0, 0);
    uint4 bh[NG][4], bl[NG][4];
    float b_aug[NG];
    const int grp0 = q0 >> 5, n_grp = qpad >> 5;
#pragma unroll
    for (int g = 0; g < NG; ++g) load_group_presplit(qsplit, qnorm, min(grp0 + g, n_grp - 1), qpad, lane, col, half, bh[g], bl[g], b_aug[g]);
    asm volatile("" : "+v"(b_aug[NG - 1]) : : "memory");               // (pins the wait, see knn_bf16_filter_body_q)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    uint4 ah[4], al[4];
    float aug;
    {
        const uint32_t base = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const void*)(s_dyn + col * 64);
        uint32_t addr[8];
        uint4 av[8];
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            addr[v] = a_chunk_addr(base, 4 * half + v, col);
            addr[4 + v] = a_chunk_addr(base, 8 + 4 * half + v, col);
        }
        lds_read_ops<M>(addr, av, (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const void*)(s_aug + lane), aug);
#pragma unroll
        for (int v = 0; v < 4; ++v) { ah[v] = av[v]; al[v] = av[4 + v]; }
    }
    __builtin_amdgcn_s_barrier();                                        // every wave has its operands: the tile's LDS is free (the scores cross it below)
    f32x16 c[NG];
    int32_t kd0 = MF_KEY_NONE, kd1 = MF_KEY_NONE, kd2 = MF_KEY_NONE, kd3 = MF_KEY_NONE, kd4 = MF_KEY_NONE, kd5 = MF_KEY_NONE;   // (bf_pair<false> touches no keys)
    const f32x16 none = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    bf_pair<false, M>(ah, al, aug, bh[0], bl[0], b_aug[0], bh[1], bl[1], b_aug[1], c[0], c[1], none, none, 0u, kd0, kd1, kd2, kd3, kd4, kd5);
    bf_pair<false, M>(ah, al, aug, bh[2], bl[2], b_aug[2], bh[3], bl[3], b_aug[3], c[2], c[3], none, none, 0u, kd0, kd1, kd2, kd3, kd4, kd5);
    // Accumulator register r of lane (col, half) is row (r & 3) + 8 (r >> 2) + 4 half of the tile for query col of the group: stored straight from
    // the registers a query's 128 bytes would leave as eight 16-byte pieces of four different instructions (partial lines: the workgroups ended at
    // 11.4-12 us, 5 us of it waiting for those stores to be acknowledged).  So the scores cross LDS once -- each wave its own 128 queries x 32 rows
    // = 16 KB, 16-byte chunk k of a query at position k ^ (query & 7): no bank conflicts either way -- and leave as whole 128-byte lines, eight
    // queries per instruction.  (The barrier in front of the MFMAs has seen every wave finish reading the tile: its LDS is free.)
    float* xs = s_dyn + (size_t)wave * (QW * 32);
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        const int ql = g * 32 + col;
#pragma unroll
        for (int m = 0; m < 4; ++m)
            *reinterpret_cast<float4*>(xs + (size_t)ql * 32 + (((2 * m + half) ^ (ql & 7)) << 2)) = make_float4(c[g][4 * m], c[g][4 * m + 1], c[g][4 * m + 2], c[g][4 * m + 3]);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                   // (the wave reads back what the wave wrote: no barrier)
#pragma unroll 4
    for (int it = 0; it < QW / 8; ++it) {
        const int ql = it * 8 + (lane >> 3), ck = lane & 7;
        const int qi = q0 + ql;
        const float4 v = *reinterpret_cast<const float4*>(xs + (size_t)ql * 32 + ((ck ^ (ql & 7)) << 2));
        if (qi < nq) *reinterpret_cast<float4*>(x + (size_t)qi * ld + t * 32 + 4 * ck) = v;
    }
}

// ------------------------------------------------------------------------------------------------ persistent variant
// Vocabularies of more than BF_PX strips (> ~60k words): a workgroup keeps its queries in registers and walks several strips
// (strip bx0, bx0 + px, ...) instead of staging and splitting the same 512 queries once per strip -- with one workgroup per compute
// unit (146 KB of LDS each) the strips of the non-persistent launch ran in ceil(strips / 256) rounds of prologue + loop + epilogue.
// LDS holds two strips: the one being multiplied and the next one, requested (LDS-DMA, augmentation entries included) as soon as
// the strip before it has been read by every wave.  Strip 0 uses the slots of the one-strip kernel (tiles 0,1 behind the query
// staging area, tiles 2.. in it), odd strips slots 8..15, even strips >= 2 slots 0..7.
constexpr size_t BF_LDS_BYTES_P = (size_t)(MF_WAVES * 4 + 2) * BF_TILE_F * 4 + (size_t)2 * MF_STRIP_TILES * 64 * 4;
// every tile of strip `bx` + its augmentation entries (wave 0): a FIXED number of DMA instructions per wave, so that the wait in
// front of the strip before it can name how many may stay in flight
// the augmentation entry of a column that is not a visible row
__device__ const float g_aug_inf[2] = {__builtin_inff(), 1.0f};
template <int M>
__device__ __forceinline__ void bf_request_strip(const float* __restrict__ vocab_bf, const float* __restrict__ row_norm, int n_rows, int bx,
                                                 int tiles_per_block, int n_tiles, int lane, int wave, int col, int half, float* slots, float* aug_dst) {
    constexpr int DPW = 8 / MF_WAVES;
    const int tile0 = bx * tiles_per_block;
    const int tile1 = min(tile0 + tiles_per_block, n_tiles);
#pragma unroll
    for (int i = 0; i < MF_STRIP_TILES; ++i) {
        const int t = min(tile0 + i, max(tile1 - 1, tile0));
        dma_tile_part<M == 1>(vocab_bf, n_rows, t, lane, slots + (size_t)i * BF_TILE_F, DPW * wave, DPW * wave + DPW);
    }
    if (wave == 0) {
#pragma unroll
        for (int i = 0; i < MF_STRIP_TILES; ++i) {
            const int t = min(tile0 + i, max(tile1 - 1, tile0));
            // (columns at or beyond n_rows read a constant {+inf, 1}: the table's own entry behind the last visible row is where the
            // appender of the previous frame -- a workgroup of this same launch on a pipelined handle -- writes its first row's norm)
            const float* src = t * 32 + col >= n_rows ? g_aug_inf + half : row_norm + 2 * (size_t)(t * 32 + col) + half;
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                             (__attribute__((address_space(3))) void*)(aug_dst + i * 64), 4, 0, 0);
        }
    }
}
// everything issued before the newest strip request has arrived (vector memory operations of gfx9 complete in issue order)
__device__ __forceinline__ void bf_wait_all_but_request(int wave) {
    constexpr int DPW = 8 / MF_WAVES;
    if (wave == 0) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(MF_STRIP_TILES * DPW + MF_STRIP_TILES) : "memory");
    else asm volatile("s_waitcnt vmcnt(%0)" :: "n"(MF_STRIP_TILES * DPW) : "memory");
}
// a barrier that waits for this wave's LDS traffic only (__syncthreads() would also wait for the strip in flight)
__device__ __forceinline__ void bf_lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
template <int M>
__device__ __forceinline__ void knn_bf16_filter_body_p(float* s_dyn, int bid, const float* __restrict__ vocab_bf, const float* __restrict__ row_norm,
                                                       int n_rows, const float* __restrict__ queries, int nq, int qpad,
                                                       int tiles_per_block, int n_blocks, int px, StripRecord* __restrict__ records, const SelfdistJob& sd,
                                                       const int32_t* __restrict__ n_lo = nullptr) {
    if (n_lo) n_rows = min(n_rows, max(n_lo[0], 1));                 // rows the search may see (see knn_bf16_filter_body); the sentinel entry follows them
    constexpr int NG = BF_NG;
    constexpr int KH = 32;
    constexpr int NW = MF_WAVES;
    constexpr int QW = BF_QW;
    constexpr int DPW = 8 / NW;
    const int n_fwg = px * ((nq + BF_QB - 1) / BF_QB);                // filter workgroups first, distance-matrix tiles behind them (see above)
    if (bid >= n_fwg) { selfdist_tile(sd, bid - n_fwg, s_dyn); return; }
    const int fb = bid;
    const int bx0 = fb % px, by = fb / px;
    const int n_my = (n_blocks - bx0 + px - 1) / px;                 // strips of this workgroup: bx0, bx0 + px, ...
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int col = lane & 31, half = lane >> 5;
    const int q0 = by * BF_QB + wave * QW;
    float* s_q = s_dyn + (size_t)wave * NG * BF_TILE_F;
    float* s_tile = s_dyn + (size_t)NW * NG * BF_TILE_F;
    float* s_aug = s_tile + 2 * BF_TILE_F;                           // [2][MF_STRIP_TILES][64]
    const int n_tiles = (n_rows + 31) / 32;
    // ---- prologue: as the one-strip kernel, for strip bx0
    {
        const int tile0 = bx0 * tiles_per_block;
        const int tile1 = min(tile0 + tiles_per_block, n_tiles);
#pragma unroll
        for (int g = 0; g < NG; ++g) dma_a_tile<KH>(queries, nq, q0 / 32 + g, lane, s_q + g * BF_TILE_F);
        float augs[MF_STRIP_TILES];
#pragma unroll
        for (int i = 0; i < MF_STRIP_TILES; ++i) {
            const int t = min(tile0 + i, max(tile1 - 1, tile0));
            augs[i] = t * 32 + col >= n_rows ? g_aug_inf[half] : row_norm[2 * (size_t)(t * 32 + col) + half];
        }
        if (tile0 < tile1) {
            dma_tile_part<M == 1>(vocab_bf, n_rows, tile0, lane, s_tile, DPW * wave, DPW * wave + DPW);
            dma_tile_part<M == 1>(vocab_bf, n_rows, min(tile0 + 1, tile1 - 1), lane, s_tile + BF_TILE_F, DPW * wave, DPW * wave + DPW);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (wave == 0) {
#pragma unroll
            for (int i = 0; i < MF_STRIP_TILES; ++i) s_aug[i * 64 + lane] = augs[i];
        }
    }
    uint4 bh[NG][4], bl[NG][4];
    float b_aug[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) split_query_group<M>(s_q + g * BF_TILE_F, col, half, bh[g], bl[g], b_aug[g]);
    __syncthreads();                                                 // every wave has its queries in registers: the staging area is free
    {
        const int tile0 = bx0 * tiles_per_block;
        const int tile1 = min(tile0 + tiles_per_block, n_tiles);
        for (int t = tile0 + 2; t < tile1; ++t)
            dma_tile_part<M == 1>(vocab_bf, n_rows, t, lane, s_dyn + (size_t)(t - tile0 - 2) * BF_TILE_F, DPW * wave, DPW * wave + DPW);
    }
    if (n_my > 1) bf_request_strip<M>(vocab_bf, row_norm, n_rows, bx0 + px, tiles_per_block, n_tiles, lane, wave, col, half,
                                   s_dyn + (size_t)8 * BF_TILE_F, s_aug + MF_STRIP_TILES * 64);
    // ---- the strips
    for (int s = 0; s < n_my; ++s) {
        const int bx = bx0 + s * px;
        const int tile0 = bx * tiles_per_block;
        const int tile1 = min(tile0 + tiles_per_block, n_tiles);
        if (s > 0) {
            // strip s was requested one strip ago; behind it only the request of strip s + 1 (a fixed number of instructions) may
            // still be in flight
            if (s + 1 < n_my) bf_wait_all_but_request(wave); else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            bf_lds_barrier();
        }
        int32_t k0[NG], k1[NG], k2[NG];
#pragma unroll
        for (int g = 0; g < NG; ++g) { k0[g] = MF_KEY_NONE; k1[g] = MF_KEY_NONE; k2[g] = MF_KEY_NONE; }
        f32x16 p0, p1;
        const float* aug_s = s_aug + (s & 1) * (MF_STRIP_TILES * 64);
        for (int t = tile0; t < tile1; ++t) {
            const int ti = t - tile0;
            if (s == 0 && ti == 2) {                                 // strip 0, tiles 2.. : one wait and one barrier for all of them
                if (n_my > 1) bf_wait_all_but_request(wave); else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                bf_lds_barrier();
            }
            uint4 ah[4], al[4];
            float aug;
            {
                const float* slot = s == 0 ? (ti < 2 ? s_tile + ti * BF_TILE_F : s_dyn + (size_t)(ti - 2) * BF_TILE_F)
                                           : s_dyn + (size_t)(((s & 1) ? 8 : 0) + ti) * BF_TILE_F;
                const uint32_t base = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const void*)(slot + col * 64);
                uint32_t addr[8];
                uint4 av[8];
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    addr[v] = a_chunk_addr(base, 4 * half + v, col);
                    addr[4 + v] = a_chunk_addr(base, 8 + 4 * half + v, col);
                }
                lds_read_ops<M>(addr, av, (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const void*)(aug_s + ti * 64 + lane), aug);
#pragma unroll
                for (int v = 0; v < 4; ++v) { ah[v] = av[v]; al[v] = av[4 + v]; }
            }
            tile_trip<M>(t == tile0, (uint32_t)ti, ah, al, aug, bh, bl, b_aug, p0, p1, k0, k1, k2);
        }
        if (tile0 < tile1) flush_pending(p0, p1, (uint32_t)(tile1 - 1 - tile0), k0, k1, k2);
#pragma unroll
        for (int g = 0; g < NG; ++g) merge_store_keys(k0[g], k1[g], k2[g], half, q0 + g * 32 + col, qpad, bx, records);
        if (s + 2 < n_my) {                                          // strip s is read by every wave: its slots take strip s + 2
            bf_lds_barrier();
            bf_request_strip<M>(vocab_bf, row_norm, n_rows, bx0 + (s + 2) * px, tiles_per_block, n_tiles, lane, wave, col, half,
                             s_dyn + (size_t)((s & 1) ? 8 : 0) * BF_TILE_F, s_aug + (s & 1) * (MF_STRIP_TILES * 64));
        }
    }
}
