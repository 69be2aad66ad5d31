// motion_group.cuh -- what the one-workgroup-per-pair RANSAC kernels of motion_3d.hip and motion_pnp.hip share, each piece once: the LDS carve, the
// compaction behind the join (motion_join.cuh), the staging of the coordinate planes, the chunked scoring of candidates, the halving tree, the
// selection, the radix select and the two index sets; and, for their host entries, the launch plan and the refusals both make.  A kernel's
// GroupBackend derives from Group and adds its rule: how a candidate is made, what an inlier is, the fit.  Callables are passed by value and
// everything is inlined: each kernel compiles to what it did with its own copy (profiles/motion_group.txt).  Internal.
#pragma once
#include "engine_impl.h"
#include "motion_join.cuh"

#include <algorithm>

namespace lcd {

constexpr int BLOCK = m3d::LANES, WAVES = BLOCK / 64;
constexpr int MAX_ROWS = m3d::MAX_ROWS;
constexpr int MODEL_FLOATS = BLOCK * 12;
// what the scoring and the fits keep in the carve beside the coordinates: the chunk's models and `sums` rows of lane partials
constexpr size_t group_fixed_bytes(int sums) { return (size_t)(MODEL_FLOATS + BLOCK * sums) * 4; }
inline size_t key_bytes(int p_max) { return (size_t)2 * padded(p_max) * 8; }
constexpr size_t LDS_LIMIT = (size_t)2 * (MAX_ROWS + (MAX_ROWS >> 3)) * 8;   // key_bytes(MAX_ROWS): 144 KiB of the 160 KiB a workgroup may have

// The sort keys of both frames in the carve, the lookup and the compaction in ascending id, one pass of 256 positions of the walked side at a
// time.  load(row_walked, row_other, c) fills the correspondence's planes and says whether it is kept.  The ids go to out_matches[0 .. m), zeros
// behind them; plane k < planes to gx[k * n_walked + position].  Returns m, behind a barrier: the keys are dead, the coordinates written.
template <int MAX_PLANES, class Load>
__device__ __forceinline__ int join_compact(unsigned char* smem, int p_max, const int32_t* ids_other, int n_other, const int32_t* ids_walked, int n_walked,
                                            int planes, int32_t* out_matches, float* gx, int* wsum, Load load) {
    const int tid = threadIdx.x;
    uint64_t* keys_o = reinterpret_cast<uint64_t*>(smem);
    uint64_t* keys_w = keys_o + padded(p_max);
    join_sort_keys(keys_o, ids_other, n_other);
    join_sort_keys(keys_w, ids_walked, n_walked);
    int m = 0;
    for (int base = 0; base < n_walked; base += BLOCK) {
        const int p = base + tid;
        bool keep = false;
        uint32_t idk = 0;
        float c[MAX_PLANES];
#pragma unroll
        for (int k = 0; k < MAX_PLANES; ++k) c[k] = 0.0f;
        if (p < n_walked) {
            uint32_t row_w, row_o;
            if (join_lookup(keys_w, n_walked, keys_o, n_other, p, idk, row_w, row_o)) keep = load(row_w, row_o, c);
        }
        int total;
        const int pos = m + block_rank(keep, wsum, total);
        if (keep) {
            out_matches[pos] = m3d::key_id(idk);
#pragma unroll
            for (int k = 0; k < MAX_PLANES; ++k)
                if (k < planes) gx[(size_t)k * n_walked + pos] = c[k];
        }
        m += total;
    }
    for (int i = m + tid; i < n_walked; i += BLOCK) out_matches[i] = 0;
    __syncthreads();
    return m;
}

// the workgroup's state behind the join; every method is called by all 256 threads and returns the same value to each
struct Group {
    int m, tid;
    const float* X;                          // coordinate c of correspondence i: X[c * stride + i]; LDS or the scratch
    int stride;
    float* models; float* red;               // the carve: [BLOCK x 12], [sums x BLOCK]
    int* valid; int* hist; int* wsum; unsigned long long* best; float* cur;
    int32_t* prev; int32_t* next;            // the two index sets, `rows` words each
    int n_prev, n_next, n_last;

    // The carve, the kernel's static LDS (wsum[WAVES], valid[BLOCK], hist[256], best, cur[12]: declared by each kernel one by one -- as one
    // struct they cost motion_3d_kernel six VGPRs and a wave of occupancy) and the sets, then the coordinates: gx's `planes` planes of `rows`
    // floats move into the carve behind red when m <= stage_cap; larger pairs read them from the scratch through the same pointer.
    __device__ __forceinline__ void init(int m_, unsigned char* smem, int sums, int* wsum_, int* valid_, int* hist_, unsigned long long* best_, float* cur_,
                                         int32_t* sets, const float* gx, int planes, int rows, int stage_cap) {
        m = m_; tid = threadIdx.x;
        models = reinterpret_cast<float*>(smem); red = models + MODEL_FLOATS;
        valid = valid_; hist = hist_; wsum = wsum_; best = best_; cur = cur_;
        prev = sets; next = sets + rows;
        n_prev = n_next = n_last = 0;
        if (m <= stage_cap) {
            float* lx = red + BLOCK * sums;
            for (int e = tid; e < planes * m; e += BLOCK) { const int k = e / m, i = e - k * m; lx[e] = gx[(size_t)k * rows + i]; }
            X = lx; stride = m;
            __syncthreads();
        } else {
            X = gx; stride = rows;
        }
    }
    // Candidates 0 .. n_cand - 1 in chunks of 256: thread tid makes its model (make(c, model) -> bool), each wave scores candidates in turn with
    // a ballot count of inlier(model, i), lane 0 raises the maximum (count << 32 | ~c).  The winner's model is made again into cur.  Returns
    // the maximum, 0 when no candidate has an inlier.
    template <class Make, class Inlier>
    __device__ __forceinline__ unsigned long long ransac(int n_cand, Make make, Inlier inlier) {
        const int lane = tid & 63, wave = tid >> 6;
        if (tid == 0) *best = 0ull;
        __syncthreads();
        for (int c0 = 0; c0 < n_cand; c0 += BLOCK) {
            const int c = c0 + tid;
            float model[12];
            const bool ok = c < n_cand && make((uint32_t)c, model);
            valid[tid] = ok ? 1 : 0;
            if (ok) {
#pragma unroll
                for (int k = 0; k < 12; ++k) models[tid * 12 + k] = model[k];
            }
            __syncthreads();
            const int nc = min(BLOCK, n_cand - c0);
            for (int j = wave; j < nc; j += WAVES) {
                if (!valid[j]) continue;
                float w[12];
#pragma unroll
                for (int k = 0; k < 12; ++k) w[k] = models[j * 12 + k];
                uint32_t count = 0;
                for (int i0 = 0; i0 < m; i0 += 64) {
                    const int i = i0 + lane;
                    const bool in = i < m && inlier(w, i);
                    count += (uint32_t)__popcll(__ballot(in));
                }
                if (lane == 0 && count > 0) atomicMax(best, ((unsigned long long)count << 32) | (uint32_t)~(uint32_t)(c0 + j));
            }
            __syncthreads();
        }
        const unsigned long long key = *best;
        if (key && tid == 0) {
            float model[12];
            (void)make(~(uint32_t)key, model);
#pragma unroll
            for (int k = 0; k < 12; ++k) cur[k] = model[k];
        }
        __syncthreads();
        return key;
    }
    // red[c * BLOCK + tid] = part[c], then the halving tree; the sums are red[c * BLOCK]; ends behind a barrier
    template <int C>
    __device__ __forceinline__ void tree(const float part[C]) {
#pragma unroll
        for (int c = 0; c < C; ++c) red[c * BLOCK + tid] = part[c];
        __syncthreads();
        for (int s = BLOCK / 2; s >= 1; s >>= 1) {
            if (tid < s) {
#pragma unroll
                for (int c = 0; c < C; ++c) red[c * BLOCK + tid] = red[c * BLOCK + tid] + red[c * BLOCK + tid + s];
            }
            __syncthreads();
        }
    }
    // next = the correspondences for which eval(i, value) holds, ascending, and their values beside them; returns their number
    template <class Eval>
    __device__ __forceinline__ int select(float* values, Eval eval) {
        int count = 0;
        for (int base = 0; base < m; base += BLOCK) {
            const int i = base + tid;
            float v = 0.0f;
            bool in = false;
            if (i < m) in = eval(i, v);
            int total;
            const int pos = count + block_rank(in, wsum, total);
            if (in) { next[pos] = i; values[pos] = v; }
            count += total;
        }
        n_next = n_last = count;
        __syncthreads();                                               // the set and its values are read by other threads
        return count;
    }
    // the key of rank `rank` among keys[0 .. n): radix select, eight bits a pass
    __device__ __forceinline__ uint32_t ranked(const uint32_t* keys, int n, int rank) {
        uint32_t prefix = 0;
        for (int shift = 24; shift >= 0; shift -= 8) {
            hist[tid] = 0;
            __syncthreads();
            for (int i = tid; i < n; i += BLOCK) {
                const uint32_t b = keys[i];
                if ((((uint64_t)b ^ prefix) >> (shift + 8)) == 0) atomicAdd(&hist[(b >> shift) & 255u], 1);
            }
            __syncthreads();
            int before = 0, digit = 255;
            for (int d = 0; d < 256; ++d) {
                const int c = hist[d];
                if (rank < before + c) { digit = d; break; }
                before += c;
            }
            rank -= before;
            prefix |= (uint32_t)digit << shift;
            __syncthreads();
        }
        return prefix;
    }
    __device__ __forceinline__ void swap_sets() {
        int32_t* p = prev; prev = next; next = p;
        const int n = n_prev; n_prev = n_next; n_next = n;
    }
    __device__ __forceinline__ void clear_next() { n_next = 0; }
    __device__ __forceinline__ int prev_n() const { return n_prev; }
    __device__ __forceinline__ int next_n() const { return n_next; }
    __device__ __forceinline__ bool same_members() const {            // (sizes are equal)
        int differs = 0;
        for (int i = tid; i < n_prev; i += BLOCK) differs |= prev[i] != next[i];
        return !__syncthreads_or(differs);
    }
    __device__ __forceinline__ const float* model() const { return cur; }
    // out_inliers[0 .. rows): the ids of prev's first n_inliers members, zeros behind them
    __device__ __forceinline__ void write_inliers(int32_t* out_inliers, const int32_t* out_matches, int rows, int n_inliers) const {
        for (int j = tid; j < rows; j += BLOCK) out_inliers[j] = j < n_inliers ? out_matches[prev[j]] : 0;
    }
};

// ---- the host entries' part

template <auto Kernel>
void allow_large_lds() {
    static const bool once = [] {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_LIMIT) != hipSuccess) (void)hipGetLastError();
        return true;
    }();
    (void)once;
}

struct GroupPlan {
    int p_max;                               // keys per side the LDS carve holds (a power of two >= every frame)
    int stage_cap;                           // correspondences whose coordinates fit the carve behind the fixed part
    size_t lds;
};
inline GroupPlan group_plan(int n_max, int m_max, size_t fixed, size_t per) {
    GroupPlan p;
    p.p_max = 64;
    while (p.p_max < n_max) p.p_max <<= 1;
    p.lds = std::max(key_bytes(p.p_max), std::min(fixed + per * m_max, LDS_LIMIT));
    p.stage_cap = (int)((p.lds - fixed) / per);
    return p;
}

// the refusals both entries make, in their order; bad(code, text) records one and returns its code.  LCD_OK: none applies.
template <class Bad>
int refuse_pairs(const lcd_engine* h, int n_pairs, Bad bad) {
    if (n_pairs < 0) return bad(LCD_ERR_INVALID, "negative n_pairs");
    if (n_pairs > 65535) return bad(LCD_ERR_UNSUPPORTED, "more than 65535 pairs per call");
    if (h->shard_append || h->shard_first || h->shard_block) return bad(LCD_ERR_UNSUPPORTED, "not offered on the handles of a sharded vocabulary");
    return LCD_OK;
}
// n_max: the most rows of a frame; m_max: the most correspondences a pair can have
template <class Bad>
int refuse_offsets(int np, const int64_t* fo, const int64_t* to, Bad bad, int& n_max, int& m_max) {
    if (!fo || !to || fo[0] != 0 || to[0] != 0) return bad(LCD_ERR_INVALID, "offsets missing or not starting at 0");
    for (int i = 0; i < np; ++i) if (fo[i + 1] < fo[i] || to[i + 1] < to[i]) return bad(LCD_ERR_INVALID, "decreasing offsets");
    n_max = m_max = 0;
    for (int i = 0; i < np; ++i) {
        const int64_t nf = fo[i + 1] - fo[i], nt = to[i + 1] - to[i];
        if (nf > MAX_ROWS || nt > MAX_ROWS) return bad(LCD_ERR_UNSUPPORTED, "more than 8192 rows on a side of a pair");
        n_max = std::max(n_max, (int)std::max(nf, nt));
        m_max = std::max(m_max, (int)std::min(nf, nt));
    }
    return LCD_OK;
}

}  // namespace lcd
