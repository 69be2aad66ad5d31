// wide_filter_body.cuh -- the matrix-core 2-NN of 128- and 256-float rows (SIFT, extended SURF, SuperPoint): the stateless bf16x3 / fp16 distance
// filter, its exact re-rank with the completeness certificate, and the exact redo.  A section of knn_mfma_kernels.hip, which includes it once,
// inside namespace lcd::{anonymous}, behind the key helpers, the filter helpers and rerank_body.cuh (op_split2, bf_mfma, strip_key, push_group4,
// widen_key, third_of_two_triples, eps_bf16, eps_f16, l2_term4, RR_MAX_CAND): not a stand-alone header.
//
// What differs from the 64-float filter (bf16_filter_body.cuh):
//   * STATELESS.  The handle keeps no operand table and no norm table for wide rows: the filter reads the fp32 rows and row_id only.  A workgroup
//     brings a 32-row tile in with coalesced 16-byte loads, converts it ONCE into matrix-core operands in LDS (op_split2<M>) and sums |v|^2 of its
//     rows on the way (an fp32 FMA chain per 16-lane group, any order: inside the dim * u norm term eps_* charge); the eight waves read the
//     operands from there.  The next tile is fetched in front of the products of this one and converted into the other LDS buffer behind them:
//     one barrier per tile.  Appending, rebuilding and tombstoning rows therefore need nothing from this path.
//   * A row that is no row (row_id == 0: a tombstone, or a row behind the device's own count when the search is planned for an upper bound; rows
//     behind the vocabulary in the last tile) may hold any bits.  Its operands are SELECTED to zero and its |v|^2 to +inf in front of every
//     arithmetic instruction: its score is +inf, and it stays out of the norm maximum.
//   * The maximum of |v|^2 over the live rows, which the certificate's eps needs, is collected here (one atomicMax on the float's bits per wave)
//     into a scratch word the search's reset kernel zeroes.
//   * Queries.  A wave keeps NG = 256 / DIM groups of 32 queries as operands in registers (128 VGPRs for bf16x3, 64 for fp16, at either row
//     length); a workgroup of eight waves takes 512 queries of 128 floats or 256 queries of 256 floats.
//   * The K loop: DIM / 16 steps of v_mfma_f32_32x32x16_bf16 / _f16 on top of the exact fp32 augmentation step |q|^2 + |v|^2 (as bf_pair).  Lane
//     (row or query l & 31, half l >> 5) holds floats [DIM / 2 * half, + DIM / 2) of its row; step s multiplies elements 8 s .. 8 s + 7 of that
//     half on both sides.
//   * The rows are cut into shares of at most WD_SHARE_TILES tiles, one record (BF_KEEP = 2 keys and a bound per query) each; a workgroup walks a
//     share in strips of MF_STRIP_TILES tiles (the in-loop key has 7 index bits): behind every strip the lane's three keys are widened to 64 bits
//     and merged into a running triple.  A vocabulary of more shares than compute units gives every workgroup several (share blockIdx.x,
//     + gridDim.x, ...): the queries stay in registers.  1024 rows per record keep the records small (20 bytes per query and 1024 rows) and the
//     bound tight enough (tests/test_certificate_model.py's model at that size rejects a few queries in a hundred).
// Records: ShareRecords (bf16_filter_body.cuh) -- keys [n_blocks][qpad][BF_KEEP] u64 merge keys, bound [n_blocks][qpad] f32 bits.  NOT the 16-byte
// StripRecord of the 64-float filters: a share is up to four strips, and strip (2 bits), tile (3) and group (2) fill the seven index bits of a
// 32-bit key -- the half of the tile's rows a lane held, which the reader needs for the row, would cost the score a bit.
#pragma once

constexpr int WD_WAVES = 8;
constexpr int WD_BLOCK = WD_WAVES * 64;
constexpr int WD_SHARE_TILES = 32;               // tiles of a share: four strips, 1024 rows per record
constexpr int WD_SLOT = 66;                      // uint4 of one (K step, hi / lo) operand slot: 64 lanes + 32 bytes that spread the conversion's writes over the banks
template <int DIM, int M> struct WideShape {
    static_assert(DIM == 128 || DIM == 256, "rows of 128 or 256 floats");
    static constexpr int NG = 256 / DIM;         // 32-query groups per wave
    static constexpr int QB = WD_WAVES * NG * 32;   // queries per workgroup
    static constexpr int STEPS = DIM / 16;       // K steps
    static constexpr int KINDS = M == 0 ? 2 : 1; // hi and lo operands (bf16x3), hi alone (fp16)
    static constexpr int U = DIM / 64;           // 16-byte chunks of a tile a thread converts: 16 lanes per row
    static constexpr int TILE_U4 = STEPS * KINDS * WD_SLOT;   // uint4 of one tile's operands
    static constexpr size_t LDS_BYTES = 2 * (size_t)TILE_U4 * 16 + 2 * 32 * 4;   // two tiles + their rows' |v|^2
};
inline int wide_group_q(int dim) { return WD_WAVES * (256 / dim) * 32; }

// three smallest of a sorted triple and three more keys
__device__ __forceinline__ void top3_merge64(uint64_t& r0, uint64_t& r1, uint64_t& r2, uint64_t a0, uint64_t a1, uint64_t a2) {
    const uint64_t in[3] = {a0, a1, a2};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        uint64_t k = in[i];
        uint64_t lo = r0 < k ? r0 : k; k = r0 < k ? k : r0; r0 = lo;
        lo = r1 < k ? r1 : k; k = r1 < k ? k : r1; r1 = lo;
        r2 = r2 < k ? r2 : k;
    }
}

template <int DIM, int M>
__global__ __launch_bounds__(WD_BLOCK) void knn_wide_filter_kernel(const float* __restrict__ vocab, const int32_t* __restrict__ row_id, int n_rows,
                                                                   const float* __restrict__ queries, int nq, int qpad, int tiles_per_block,
                                                                   int n_blocks, ShareRecords rec, uint32_t* __restrict__ norm_max_bits) {
    typedef WideShape<DIM, M> S;
    constexpr int NG = S::NG, STEPS = S::STEPS, KINDS = S::KINDS, U = S::U;
    extern __shared__ __attribute__((aligned(16))) float s_dyn_w[];
    uint4* s_op = reinterpret_cast<uint4*>(s_dyn_w);                                  // [2][STEPS][KINDS][WD_SLOT]
    float* s_norm = s_dyn_w + 2 * (size_t)S::TILE_U4 * 4;                            // [2][32]: |v|^2 of the tile's rows, +inf for a row that is none

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int col = lane & 31, half = lane >> 5;
    const int q0 = (int)blockIdx.y * S::QB + wave * (NG * 32);
    const bool active = q0 < nq;                                                     // (uniform) a wave without queries only converts tiles
    const int n_tiles = (int)(((long long)n_rows + 31) / 32);

    // the wave's queries as B operands: -2 q split hi / lo, + |q|^2 for the augmentation step (lanes behind the last query repeat it)
    uint4 bh[NG][STEPS], bl[NG][M == 0 ? STEPS : 1];
    float b_aug[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        const int qi = min(q0 + g * 32 + col, nq - 1);
        const float4* src = reinterpret_cast<const float4*>(queries + (size_t)qi * DIM + half * (DIM / 2));
        float part = 0.0f;
#pragma unroll
        for (int s = 0; s < STEPS; ++s) {
            const float4 x = src[2 * s], y = src[2 * s + 1];
            part = fmaf(x.x, x.x, part); part = fmaf(x.y, x.y, part); part = fmaf(x.z, x.z, part); part = fmaf(x.w, x.w, part);
            part = fmaf(y.x, y.x, part); part = fmaf(y.y, y.y, part); part = fmaf(y.z, y.z, part); part = fmaf(y.w, y.w, part);
            uint4 hi, lo;
            op_split2<M>(-2.0f * x.x, -2.0f * x.y, hi.x, lo.x);
            op_split2<M>(-2.0f * x.z, -2.0f * x.w, hi.y, lo.y);
            op_split2<M>(-2.0f * y.x, -2.0f * y.y, hi.z, lo.z);
            op_split2<M>(-2.0f * y.z, -2.0f * y.w, hi.w, lo.w);
            bh[g][s] = hi;
            if constexpr (M == 0) bl[g][s] = lo;
        }
        const float qn = part + __shfl_xor(part, 32, 64);
        b_aug[g] = half == 0 ? 1.0f : qn;
    }

    // conversion: thread -> (row tid >> 4 of the tile, chunks (tid & 15) + 16 u of the row): a wave's load is four rows x 256 contiguous bytes
    const int c_row = tid >> 4, c_lane = tid & 15;
    float4 st[U];
    bool st_live = false;
    float wmax = 0.0f;
    auto fetch = [&](int t) {
        const int r = t * 32 + c_row;
        const int rc = min(r, n_rows - 1);
        st_live = r < n_rows && row_id[rc] != 0;
        const float4* src = reinterpret_cast<const float4*>(vocab + (size_t)rc * DIM);
#pragma unroll
        for (int u = 0; u < U; ++u) st[u] = src[c_lane + 16 * u];
    };
    auto convert = [&](int buf) {
        uint2* op2 = reinterpret_cast<uint2*>(s_op + (size_t)buf * S::TILE_U4);
        float part = 0.0f;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            float4 x = st[u];
            x.x = st_live ? x.x : 0.0f; x.y = st_live ? x.y : 0.0f; x.z = st_live ? x.z : 0.0f; x.w = st_live ? x.w : 0.0f;   // selected, not multiplied
            part = fmaf(x.x, x.x, part); part = fmaf(x.y, x.y, part); part = fmaf(x.z, x.z, part); part = fmaf(x.w, x.w, part);
            uint2 hi, lo;
            op_split2<M>(x.x, x.y, hi.x, lo.x);
            op_split2<M>(x.z, x.w, hi.y, lo.y);
            const int f0 = 4 * (c_lane + 16 * u);                                    // the chunk's first float
            const int h = f0 / (DIM / 2), within = f0 % (DIM / 2);
            const int s = within >> 3, e4 = (within >> 2) & 1;
            const int slot = (s * KINDS) * WD_SLOT + h * 32 + c_row;
            op2[2 * slot + e4] = hi;
            if constexpr (M == 0) op2[2 * (slot + WD_SLOT) + e4] = lo;
        }
#pragma unroll
        for (int m = 8; m >= 1; m >>= 1) part += __shfl_xor(part, m, 64);
        if (c_lane == 0) s_norm[buf * 32 + c_row] = st_live ? part : __int_as_float(0x7f800000);
        wmax = fmaxf(wmax, st_live ? part : 0.0f);
    };

    // share bx of the rows: tiles [bx * tiles_per_block, + tiles_per_block), one record per query; a workgroup takes shares blockIdx.x, + gridDim.x, ...
    for (int bx = blockIdx.x; bx < n_blocks; bx += gridDim.x) {
    const int tile0 = bx * tiles_per_block;
    const int tile1 = min(tile0 + tiles_per_block, n_tiles);
    const int nt = tile1 - tile0;
    int32_t k0[NG], k1[NG], k2[NG];
    uint64_t r0[NG], r1[NG], r2[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) { k0[g] = MF_KEY_NONE; k1[g] = MF_KEY_NONE; k2[g] = MF_KEY_NONE; r0[g] = KEY_NONE; r1[g] = KEY_NONE; r2[g] = KEY_NONE; }

    // (every wave is behind the last tile's barrier of the share before: both buffers are free)
    if (nt > 0) { fetch(tile0); convert(0); }
    __syncthreads();
    for (int ti = 0; ti < nt; ++ti) {
        const int buf = ti & 1;
        if (ti + 1 < nt) fetch(tile0 + ti + 1);
        const int tl = ti & (MF_STRIP_TILES - 1);                                    // the tile's index in its strip
        if (active) {
            const uint4* op = s_op + (size_t)buf * S::TILE_U4;
            const float a_aug = half == 0 ? s_norm[buf * 32 + col] : 1.0f;
            const f32x16 z = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
            f32x16 acc[NG];
#pragma unroll
            for (int g = 0; g < NG; ++g) acc[g] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_aug, b_aug[g], z, 0, 0, 0);
#pragma unroll
            for (int s = 0; s < STEPS; ++s) {
                const uint4 ah = op[(s * KINDS) * WD_SLOT + lane];
                uint4 al = ah;
                if constexpr (M == 0) al = op[(s * KINDS + 1) * WD_SLOT + lane];
#pragma unroll
                for (int g = 0; g < NG; ++g) {
                    acc[g] = bf_mfma<M>(ah, bh[g][s], acc[g]);
                    if constexpr (M == 0) {
                        acc[g] = bf_mfma<M>(ah, bl[g][s], acc[g]);
                        acc[g] = bf_mfma<M>(al, bh[g][s], acc[g]);
                    }
                }
            }
#pragma unroll
            for (int g = 0; g < NG; ++g) push_group4(acc[g], (uint32_t)tl, k0[g], k1[g], k2[g]);
            if (tl == MF_STRIP_TILES - 1 || ti == nt - 1) {                          // the strip ends: its keys join the workgroup's running triple
                const int strip_tile0 = tile0 + ti - tl;
#pragma unroll
                for (int g = 0; g < NG; ++g) {
                    top3_merge64(r0[g], r1[g], r2[g], widen_key(k0[g], strip_tile0, half), widen_key(k1[g], strip_tile0, half), widen_key(k2[g], strip_tile0, half));
                    k0[g] = MF_KEY_NONE; k1[g] = MF_KEY_NONE; k2[g] = MF_KEY_NONE;
                }
            }
        }
        if (ti + 1 < nt) convert(buf ^ 1);
        __syncthreads();
    }

    // the two halves of a query's rows meet: best two of the six keys, the third as the bound on everything dropped in this share
    if (active) {
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            const int qi = q0 + g * 32 + col;
            uint64_t m0, m1, third;
            merge_halves(r0[g], r1[g], r2[g], m0, m1, third);
            if (half == 0 && qi < qpad) {
                uint64_t* dst = rec.keys + ((size_t)bx * qpad + qi) * BF_KEEP;
                dst[0] = m0;
                dst[1] = m1;
                rec.bound[(size_t)bx * qpad + qi] = (uint32_t)min(third >> 32, (uint64_t)0x7f800000u);
            }
        }
    }
    }

    // the largest |v|^2 this workgroup multiplied (live rows only)
#pragma unroll
    for (int m = 32; m >= 16; m >>= 1) wmax = fmaxf(wmax, __shfl_xor(wmax, m, 64));
    if (lane == 0 && wmax > 0.0f && blockIdx.y == 0) atomicMax(norm_max_bits, __float_as_uint(wmax));
}

// The search's reset: the certificate counters a stand-alone redo leaves raised ([0] rejected, [1] arrivals, [3] done; [2], the running maximum
// of the error ratio, stays) and the norm maximum the filter collects.
__global__ void knn_wide_reset_kernel(int32_t* __restrict__ fail_count, int reset_count, uint32_t* __restrict__ norm_max_bits) {
    if (reset_count && threadIdx.x < 4 && threadIdx.x != 2) fail_count[threadIdx.x] = 0;
    if (threadIdx.x == 4) norm_max_bits[0] = 0u;
}

// ------------------------------------------------------------------------------------------------ re-rank + certificate
// One workgroup per query: the logic of knn_mfma_rerank_body without pending rows, shadow scores, staging and row writers.  Pass 1 finds tau (the
// second smallest kept score) and the bound (the smallest score any workgroup of the filter dropped); every kept key at or below
// tau (1 + 2^-15) + 2 eps has ALL FOUR rows of its group evaluated exactly -- one lane per row, the reference's terms chained left to right
// (l2_term4: the bits are the scan's by construction); the two best with ties to the lower row are the answer, accepted iff
// bound - eps > exact second distance.  eps is eps_bf16 / eps_f16 at DIM with the filter's own norm maximum.  Anything else -- more than
// RR_MAX_CAND candidate rows, a measured error of half of eps, fp16 operands out of range -- sends the query to the exact redo.
template <int DIM>
__global__ __launch_bounds__(MF_BLOCK) void knn_wide_rerank_kernel(ShareRecords rec, int n_blocks, int nq, int qpad, const float* __restrict__ vocab,
                                                                   const float* __restrict__ queries, const int32_t* __restrict__ row_id, int n_rows,
                                                                   const uint32_t* __restrict__ norm_max_bits, int32_t* __restrict__ out_row,
                                                                   int32_t* __restrict__ out_word, float* __restrict__ out_dist,
                                                                   int32_t* __restrict__ fail_list, int32_t* __restrict__ fail_count, int f16) {
    constexpr uint32_t INF = 0x7f800000u;
    constexpr int RR_KEYS = RR_MAX_CAND / 4;
    __shared__ float4 s_q[DIM / 4];
    __shared__ float s_qn;
    __shared__ uint32_t s_a0[MF_WAVES], s_a1[MF_WAVES], s_bound[MF_WAVES];
    __shared__ int s_ncand;
    __shared__ uint64_t s_cand[RR_KEYS], s_exact[RR_MAX_CAND];
    __shared__ float s_err[MF_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int qi = blockIdx.x;
    const int n_keys = n_blocks * BF_KEEP;
    auto key_at = [&](int c) -> uint64_t { return rec.keys[((size_t)(c / BF_KEEP) * qpad + qi) * BF_KEEP + (c % BF_KEEP)]; };

    // the query and |q|^2 (DIM / 4 <= 64 lanes of wave 0)
    {
        float part = 0.0f;
        if (tid < DIM / 4) {
            const float4 q4 = reinterpret_cast<const float4*>(queries + (size_t)qi * DIM)[tid];
            s_q[tid] = q4;
            part = fmaf(q4.w, q4.w, fmaf(q4.z, q4.z, fmaf(q4.y, q4.y, q4.x * q4.x)));
        }
        if (wave == 0) {
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) part += __shfl_xor(part, m, 64);
            if (lane == 0) s_qn = part;
        }
    }
    const float vn_max = __uint_as_float(norm_max_bits[0]);
    const uint32_t err_seen = running_max_seen(reinterpret_cast<const uint32_t*>(fail_count) + 2);   // (as knn_mfma_rerank_body: the atomic below is for a ratio above it)

    // ---- pass 1: tau and the bound on dropped rows
    uint32_t a0 = INF, a1 = INF, bound = INF;
    for (int c = tid; c < n_keys; c += MF_BLOCK) {
        const uint32_t sc = min((uint32_t)(key_at(c) >> 32), INF);                   // KEY_NONE -> +inf
        const uint32_t h = max(a0, sc);
        a0 = min(a0, sc);
        a1 = min(a1, h);
    }
    for (int b = tid; b < n_blocks; b += MF_BLOCK) bound = min(bound, rec.bound[(size_t)b * qpad + qi]);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const uint32_t o0 = (uint32_t)__shfl_xor((int)a0, m, 64), o1 = (uint32_t)__shfl_xor((int)a1, m, 64);
        a1 = min(max(a0, o0), min(a1, o1));
        a0 = min(a0, o0);
        bound = min(bound, (uint32_t)__shfl_xor((int)bound, m, 64));
    }
    if (lane == 0) { s_a0[wave] = a0; s_a1[wave] = a1; s_bound[wave] = bound; }
    if (tid == 0) s_ncand = 0;
    __syncthreads();
    a0 = s_a0[0]; a1 = s_a1[0]; bound = s_bound[0];
#pragma unroll
    for (int wi = 1; wi < MF_WAVES; ++wi) {
        const uint32_t o0 = s_a0[wi], o1 = s_a1[wi];
        a1 = min(max(a0, o0), min(a1, o1));
        a0 = min(a0, o0);
        bound = min(bound, s_bound[wi]);
    }
    const float qn = s_qn;
    const float eps = f16 ? eps_f16(DIM, qn, vn_max) : eps_bf16(DIM, qn, vn_max);
    const float tau = __uint_as_float(a1);
    const float thr = tau + (2.0f * eps + tau * 3.0517578e-5f);                      // +inf when fewer than two finite keys exist

    // ---- pass 2: the keys at or below the threshold
    for (int c = tid; c < n_keys; c += MF_BLOCK) {
        const uint64_t key = key_at(c);
        const uint32_t sc = (uint32_t)(key >> 32);
        if (key != KEY_NONE && sc < INF && __uint_as_float(sc) <= thr) {
            const int slot = atomicAdd(&s_ncand, 1);
            if (slot < RR_KEYS) s_cand[slot] = key;
        }
    }
    __syncthreads();
    const int n_keys_in = s_ncand;
    const bool overflow = n_keys_in > RR_KEYS;
    const int n_cand = overflow ? 0 : n_keys_in * 4;                                 // candidate ROWS: slot i is row (i & 3) of key i >> 2

    // ---- exact distances: one lane per candidate row (waves 0 and 1; the four rows of a key are four neighbouring lanes)
    float err_ratio = 0.0f;
    if (tid < RR_MAX_CAND) {                                                         // (whole waves: the shuffles below find their lanes)
        const bool have = tid < n_cand;
        const uint64_t key = have ? s_cand[tid >> 2] : 0ull;
        const uint32_t row = (uint32_t)key + (uint32_t)(tid & 3);
        const bool live = have && row < (uint32_t)n_rows && row_id[row] != 0;        // a tombstone, a row that does not exist (yet): no candidate
        float res = __int_as_float(0x7f800000);
        if (live) {
            const float4* src = reinterpret_cast<const float4*>(vocab + (size_t)row * DIM);
            res = 0.0f;
#pragma unroll 8
            for (int c = 0; c < DIM / 4; ++c) res = __fadd_rn(res, l2_term4(src[c], s_q[c]));
        }
        float gmin = res;                                                            // the filter's score of a key is its group's minimum
        gmin = fminf(gmin, __shfl_xor(gmin, 1, 64));
        gmin = fminf(gmin, __shfl_xor(gmin, 2, 64));
        if (have && (tid & 3) == 0 && gmin < __int_as_float(0x7f800000)) err_ratio = fabsf(__uint_as_float((uint32_t)(key >> 32)) - gmin) / eps;
        s_exact[tid] = live ? (((uint64_t)__float_as_uint(res) << 32) | row) : KEY_NONE;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) err_ratio = fmaxf(err_ratio, __shfl_xor(err_ratio, m, 64));
    if (lane == 0) s_err[wave] = err_ratio;
    __syncthreads();

    // ---- top-2 (ties go to the lower row: the key carries it), results and certificate
    if (wave == 0) {
        uint64_t best = KEY_NONE, second = KEY_NONE;
        for (int i = lane; i < n_cand; i += 64) top2_push(best, second, s_exact[i]);
        wave_top2_reduce(best, second);
        if (lane == 0) {
            err_ratio = s_err[0];
#pragma unroll
            for (int wi = 1; wi < MF_WAVES; ++wi) err_ratio = fmaxf(err_ratio, s_err[wi]);
            const uint64_t win[2] = {best, second};
            int32_t wout[2] = {0, 0};
#pragma unroll
            for (int j = 0; j < 2; ++j) if (win[j] != KEY_NONE) wout[j] = row_id[(uint32_t)win[j]];
            // certificate: every row the filter dropped is strictly farther than the exact second neighbour
            bool ok = !overflow;
            if (ok && bound < INF) {                                                 // something finite was dropped
                if (second == KEY_NONE) ok = false;
                else ok = __uint_as_float(bound) - eps > __uint_as_float((uint32_t)(second >> 32));
            }
            // the premise is |filter score - exact distance| <= eps for every row; on the re-ranked candidates that error was just measured: half
            // the budget used up anywhere means the bound is no longer trusted for this query
            if (!(err_ratio < 0.5f)) ok = false;
            // fp16 operands hold magnitudes up to 65504: descriptors far outside that (the filter multiplies -2 q) go to the exact redo
            if (f16 && !(qn < 1.0e8f && vn_max < 1.0e8f)) ok = false;
            if (err_ratio > 0.0f && eps > 0.0f && err_ratio < __int_as_float(0x7f800000) && __float_as_uint(err_ratio) > err_seen)
                atomicMax(reinterpret_cast<uint32_t*>(fail_count) + 2, __float_as_uint(err_ratio));   // fail_count[2]: max |score - distance| / eps
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                out_row[2 * qi + j] = win[j] == KEY_NONE ? -1 : (int32_t)(uint32_t)win[j];
                out_word[2 * qi + j] = wout[j];
                out_dist[2 * qi + j] = win[j] == KEY_NONE ? -1.0f : __uint_as_float((uint32_t)(win[j] >> 32));
            }
            if (!ok) fail_list[atomicAdd(fail_count, 1)] = qi;
        }
    }
}

// ------------------------------------------------------------------------------------------------ exact redo
// rowpar_body.cuh at the wide row lengths: a lane holds its row in DIM registers, the listed queries are looped over.  Launched behind every
// re-rank; it leaves at once when nothing was rejected.
template <int DIM>
__global__ __launch_bounds__(MF_BLOCK) void knn_wide_rowpar_kernel(RowparArgs a, int32_t* __restrict__ fail_count) {
    rowpar_body<DIM, MF_BLOCK>(a, (int)blockIdx.x, (int)gridDim.x, fail_count);
}
