// pair_match.hip -- lcd_match_pairs / lcd_match_pairs_dev: the descriptors of two frames matched in one stateless call, for any number
// of frame pairs (reference RegistrationVis.cpp:1383-1504: the verification step behind the loop-closure hypothesis and every proximity
// candidate).  Two matchers, both made of what the engine already computes bit-exactly:
//   dictionary mode  == the temporary two-frame VWDictionary (:1482-1503): addNewWords(from) -> update() -> addNewWords(to);
//   cross-check mode == cv::BFMatcher(crossCheck = true).match(to, from) (:1451-1453), by the rule include/lcd.h writes down.
//
// Two launches per group of pairs, no host round trip between them and nothing read back in between (not even how many words the
// from-frame created):
//   launch 1, pair_dist_kernel: a linear grid over the tiles of every distance block of every pair -- to x from, plus from x from and
//     to x to when new words are compared together.  A tile is selfdist_*_kernel's (knn2_kernels.hip): 64 lanes own 64 rows of one side, the
//     four waves walk eight rows each of the other, whose address is wave-uniform; the arithmetic is dist_ref.cuh's, the reference's.
//   launch 2, pair_match_kernel: ONE workgroup per pair (the decision loop is a latency chain, resolve_kernels.hip) runs
//     dictionary:  (1) the from-frame's decision loop on an empty vocabulary (resolve_body; no index: every earlier new word is a candidate,
//                  one shared all-ones bit row), (2) the to-rows' 2-NN over the from-rows that became words -- the to x from block under
//                  the from-frame's new-word mask, keys (distance bits << 32 | vocabulary row) as everywhere, row = rank of the word --
//                  and the to-frame's candidate bit rows from its thresholds, (3) the to-frame's decision loop (resolve_body again);
//     cross-check: the row arg-min with (distance bits << 32 | from-row) keys, a 64-bit atomicMin per from-row over the to-rows that
//                  chose it with (distance bits << 32 | to-row) keys, then the filter.
// Nothing of the engine is read or written: the scratch is StatelessScratch's (stateless_scratch.h), which is why the call does not drain a pipelined handle.
#include "engine_impl.h"
#include "dist_ref.cuh"
#include "resolve_body.cuh"
#include "top2_keys.cuh"

#include <vector>

static_assert(sizeof(lcd_match_args) == 96, "lcd_match_args: the layout include/lcd.h documents (LP64)");

namespace lcd {
namespace {

constexpr int DBLOCK = 256;                  // launch 1: four waves
constexpr int TILE_A = 32;                   // rows of side A per tile (eight per wave)
constexpr int TILE_B = 64;                   // rows of side B per tile (one per lane)
constexpr int MAX_SIDE = 8192;               // rows on one side of a pair (the decision loop's limit, launch_resolve)

// one distance block of one pair: dist[out + r * ld + c] = distance(A row r, B row c)
struct TileJob {
    int64_t tile_first;                      // the block's first tile in the launch's linear grid
    int64_t a_row, b_row;                    // first row of A / B among the concatenated from- / to-rows
    int64_t out;                             // floats into the distance scratch
    int32_t na, nb, ld;
    int32_t sides;                           // bit 0: A are to-rows, bit 1: B are to-rows
};
struct PairJob {
    int64_t from_row, to_row;                // the pair's first from- / to-row (also where its outputs start)
    int64_t d_tf, d_ff, d_tt;                // floats into the distance scratch: to x from, from x from, to x to
    int64_t small;                           // 4-byte words into the per-pair scratch (even: the keys are 8 bytes)
    int32_t nf, nt;
};

__host__ __device__ inline int ld_of(int n) { return (n + 63) / 64 * 64; }           // leading dimension of a block with n columns (prepare_resolve's)
__host__ __device__ inline int64_t even(int64_t n) { return (n + 1) & ~(int64_t)1; }
// the per-pair scratch, in words.  dictionary: knn_word[2 nt] | knn_dist[2 nt] | rank[nf] | id_of_rank[nf] | n_new[2] | bits[nt x ld_of(nt) / 32]
//                                  cross-check: nn_key[nt] (8 bytes each) | back[nf] (8 bytes each)
__host__ __device__ inline int64_t small_words(int mode, int nf, int nt, bool together) {
    if (mode == LCD_MATCH_CROSS_CHECK) return 2 * ((int64_t)nt + nf);
    return 4 * (int64_t)nt + 2 * even(nf) + 2 + (together ? (int64_t)nt * (ld_of(nt) / 32) : 0);
}

// ------------------------------------------------------------------------------------------------ launch 1: the distance blocks
// DTYPE 0: squared L2 over K floats, 1: Hamming over K dwords; K == 0: any row length (kdyn), the correctness path as *_dyn_kernel is for the scans
template <int DTYPE, int K>
__global__ __launch_bounds__(DBLOCK) void pair_dist_kernel(const void* __restrict__ from, const void* __restrict__ to, const TileJob* __restrict__ jobs,
                                                           int n_jobs, int kdyn, float* __restrict__ dist) {
    const int64_t t = blockIdx.x;
    int lo = 0, hi = n_jobs - 1;                                      // the block this tile belongs to: the last one that starts at or before it
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (jobs[mid].tile_first <= t) lo = mid; else hi = mid - 1;
    }
    const TileJob J = jobs[lo];
    const int k = K ? K : kdyn;                                       // dwords per row
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int tiles_a = (J.na + TILE_A - 1) / TILE_A;
    const int local = (int)(t - J.tile_first);
    const int ta = local % tiles_a, tb = local / tiles_a;
    const uint32_t* A = (const uint32_t*)((J.sides & 1) ? to : from) + (size_t)J.a_row * k;
    const uint32_t* B = (const uint32_t*)((J.sides & 2) ? to : from) + (size_t)J.b_row * k;
    const int c = tb * TILE_B + lane;
    if (tb * TILE_B >= J.nb) return;                                  // (never: the grid holds exactly the tiles of the blocks)
    const uint32_t* qsrc = B + (size_t)min(c, J.nb - 1) * k;          // lanes behind the block's last column: clamped, never stored
    const int r0 = ta * TILE_A + wave * (TILE_A / 4);
    const int r1 = min(r0 + TILE_A / 4, J.na);
    float* out = dist + J.out;
    if constexpr (K != 0 && DTYPE == 0) {
        float q[K];
#pragma unroll
        for (int g = 0; g < K / 4; ++g) {
            const float4 v = reinterpret_cast<const float4*>(qsrc)[g];
            q[4 * g + 0] = v.x; q[4 * g + 1] = v.y; q[4 * g + 2] = v.z; q[4 * g + 3] = v.w;
        }
        for (int r = r0; r < r1; ++r) {
            const float d = l2_ref<K>(reinterpret_cast<const float*>(A + (size_t)r * K), q);
            if (c < J.nb) out[(size_t)r * J.ld + c] = d;
        }
    } else if constexpr (K != 0) {
        uint32_t q[K];
#pragma unroll
        for (int g = 0; g < K / 4; ++g) {
            const uint4 v = reinterpret_cast<const uint4*>(qsrc)[g];
            q[4 * g + 0] = v.x; q[4 * g + 1] = v.y; q[4 * g + 2] = v.z; q[4 * g + 3] = v.w;
        }
        for (int r = r0; r < r1; ++r) {
            const float d = (float)hamming_ref<K>(A + (size_t)r * K, q);
            if (c < J.nb) out[(size_t)r * J.ld + c] = d;
        }
    } else {
        for (int r = r0; r < r1; ++r) {
            float d;
            if (DTYPE == 0) d = l2_ref_dyn(reinterpret_cast<const float*>(A + (size_t)r * k), reinterpret_cast<const float*>(qsrc), k);
            else d = (float)hamming_dyn(A + (size_t)r * k, qsrc, k);
            if (c < J.nb) out[(size_t)r * J.ld + c] = d;
        }
    }
}

hipError_t launch_pair_dist(int dtype, int kdim, const void* from, const void* to, const TileJob* jobs, int n_jobs, int64_t n_tiles, float* dist,
                            hipStream_t s) {
    if (n_tiles <= 0) return hipSuccess;
    if (n_tiles > 0x7fffffffll) return hipErrorInvalidValue;
    const dim3 grid((unsigned)n_tiles), block(DBLOCK);
    if (dtype == LCD_F32) {
        if (kdim == 64) pair_dist_kernel<0, 64><<<grid, block, 0, s>>>(from, to, jobs, n_jobs, kdim, dist);
        else if (kdim == 128) pair_dist_kernel<0, 128><<<grid, block, 0, s>>>(from, to, jobs, n_jobs, kdim, dist);
        else pair_dist_kernel<0, 0><<<grid, block, 0, s>>>(from, to, jobs, n_jobs, kdim, dist);
    } else {
        const int w32 = kdim / 4;
        if (w32 == 8) pair_dist_kernel<1, 8><<<grid, block, 0, s>>>(from, to, jobs, n_jobs, w32, dist);
        else if (w32 == 16) pair_dist_kernel<1, 16><<<grid, block, 0, s>>>(from, to, jobs, n_jobs, w32, dist);
        else pair_dist_kernel<1, 0><<<grid, block, 0, s>>>(from, to, jobs, n_jobs, w32, dist);
    }
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ launch 2: one workgroup per pair
struct MatchArgs {
    const PairJob* pairs; const float* dist; uint32_t* small; const uint32_t* ones;
    int mode, flags; float nndr;
    const int32_t* from_ids;                                          // dictionary mode, may be NULL
    int32_t* out_from; int32_t* out_to;                               // dictionary mode
    int32_t* out_match; float* out_dist;                              // cross-check mode (out_dist may be NULL)
};

__device__ __forceinline__ void dictionary_pair(const MatchArgs& a, const PairJob& P, uint32_t* rs) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nf = P.nf, nt = P.nt;
    const bool together = (a.flags & LCD_Q_NEW_WORDS_COMPARED) != 0;
    uint32_t* sm = a.small + P.small;
    int32_t* knn_word = reinterpret_cast<int32_t*>(sm);
    float* knn_dist = reinterpret_cast<float*>(sm + 2 * (size_t)nt);
    int32_t* rank = reinterpret_cast<int32_t*>(sm + 4 * (size_t)nt);                 // vocabulary row of from-row j (-1: it is no word)
    int32_t* id_of_rank = rank + even(nf);
    int32_t* n_new = id_of_rank + even(nf);
    uint32_t* bits = reinterpret_cast<uint32_t*>(n_new + 2);
    int32_t* out_from = a.out_from + P.from_row;
    int32_t* out_to = a.out_to + P.to_row;
    const int ldf = ld_of(nf), ldt = ld_of(nt);
    __shared__ int s_max_id;
    int n_words = 0, base = 0;                                        // vocabulary rows the to-frame searches, _lastWordId behind the from-frame

    // ---- (1) the from-frame: addNewWords on an empty dictionary, or addWord(id, row) per row
    if (nf > 0 && a.from_ids) {
        const int32_t* ids = a.from_ids + P.from_row;
        if (tid == 0) s_max_id = 0;
        __syncthreads();
        for (int j = tid; j < nf; j += RBLOCK) {
            const int32_t id = ids[j];
            int r = 0;                                                // update() appends _notIndexedWords, a std::set: ascending id
            for (int k = 0; k < nf; ++k) { const int32_t o = ids[k]; r += (o < id || (o == id && k < j)) ? 1 : 0; }
            rank[j] = r; id_of_rank[r] = id; out_from[j] = id;
            atomicMax(&s_max_id, id);
        }
        __syncthreads();
        n_words = nf; base = s_max_id;
    } else if (nf > 0) {
        // no index (have_index 0): every threshold is +inf, every bit row all ones -- one shared row, stride 0
        const uint32_t* mask = resolve_body<RBLOCK>(rs, nf, a.flags, a.nndr, 0, nullptr, nullptr, a.dist + P.d_ff, ldf, together ? a.ones : nullptr, 0,
                                                    out_from, n_new, nullptr, nullptr, nullptr, WsRuns());
        const int mw = (nf + 63) / 64 * 2;
        const uint32_t* prefix = rs + 2 * mw;
        for (int j = tid; j < nf; j += RBLOCK) {                      // (the thread that wrote out_from[j])
            const bool is_new = (mask[j >> 5] >> (j & 31)) & 1u;
            const int r = is_new ? new_rank(mask, prefix, j) : -1;
            rank[j] = r;
            if (is_new) id_of_rank[r] = r + 1;                        // ++_lastWordId from 0, descriptor order
            out_from[j] = -out_from[j];                               // -(k + 1), own or matched: word k + 1
        }
        n_words = (int)prefix[mw]; base = n_words;
        __syncthreads();
    }
    if (nt <= 0) return;                                              // if(descriptorsTo.rows)

    // ---- (2) the to-rows' 2-NN over the words (only when there are two: VWDictionary.cpp:1015) and their candidate bit rows
    const int have_index = n_words >= 2 ? 1 : 0;
    if (have_index) {
        for (int i = wave; i < nt; i += RBLOCK / 64) {
            const float* row = a.dist + P.d_tf + (size_t)i * ldf;
            uint64_t b = KEY_NONE, s = KEY_NONE;
            for (int j = lane; j < nf; j += 64) {
                const int r = rank[j];
                if (r >= 0) top2_push(b, s, ((uint64_t)__float_as_uint(row[j]) << 32) | (uint32_t)r);
            }
            wave_top2_reduce(b, s);
            if (lane == 0) {
                knn_word[2 * i] = b != KEY_NONE ? id_of_rank[(uint32_t)b] : 0;
                knn_dist[2 * i] = b != KEY_NONE ? __uint_as_float((uint32_t)(b >> 32)) : -1.0f;
                knn_word[2 * i + 1] = s != KEY_NONE ? id_of_rank[(uint32_t)s] : 0;
                knn_dist[2 * i + 1] = s != KEY_NONE ? __uint_as_float((uint32_t)(s >> 32)) : -1.0f;
            }
        }
        __syncthreads();
        if (together) {
            // bit j of row i = dist(j, i) < distance of i's second neighbour (cand_threshold, knn2_kernels.hip); only the words the
            // decision loop reads (j < i) are written
            const int bw = ldt / 32;
            const float* tt = a.dist + P.d_tt;
            for (int w = 0; (w << 5) < nt; ++w) {
                for (int i = (w << 5) + tid; i < nt; i += RBLOCK) {
                    const bool v0 = knn_dist[2 * i] >= 0.0f && knn_word[2 * i] != 0, v1 = knn_dist[2 * i + 1] >= 0.0f && knn_word[2 * i + 1] != 0;
                    const float thr = (v0 && v1) ? knn_dist[2 * i + 1] : __int_as_float(0x7f800000);
                    uint32_t word = 0;
                    const int jn = min(32, nt - (w << 5));
                    for (int u = 0; u < jn; ++u) word |= (tt[(size_t)((w << 5) + u) * ldt + i] < thr ? 1u : 0u) << u;
                    bits[(size_t)i * bw + w] = word;
                }
            }
            __syncthreads();
        }
    }

    // ---- (3) the to-frame's decision loop
    resolve_body<RBLOCK>(rs, nt, a.flags, a.nndr, have_index, knn_word, knn_dist, a.dist + P.d_tt, ldt,
                         together ? (have_index ? bits : a.ones) : nullptr, have_index ? ldt / 32 : 0, out_to, n_new, nullptr, nullptr, nullptr, WsRuns());
    for (int i = tid; i < nt; i += RBLOCK) {                          // (the thread that wrote out_to[i])
        const int w = out_to[i];
        out_to[i] = w > 0 ? w : base - w;                             // -(k + 1): the k-th new word of the to-frame, id base + k + 1
    }
}

__device__ __forceinline__ void cross_check_pair(const MatchArgs& a, const PairJob& P) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nf = P.nf, nt = P.nt;
    unsigned long long* nn_key = reinterpret_cast<unsigned long long*>(a.small + P.small);   // (distance bits << 32) | nn(i)
    unsigned long long* back = nn_key + nt;                                                  // (distance bits << 32) | back(j)
    int32_t* out_match = a.out_match + P.to_row;
    float* out_dist = a.out_dist ? a.out_dist + P.to_row : nullptr;
    const int ldf = ld_of(nf);
    for (int j = tid; j < nf; j += RBLOCK) back[j] = KEY_NONE;
    for (int i = wave; i < nt; i += RBLOCK / 64) {
        const float* row = a.dist + P.d_tf + (size_t)i * ldf;
        uint64_t b = KEY_NONE;
        for (int j = lane; j < nf; j += 64) {
            const uint64_t k = ((uint64_t)__float_as_uint(row[j]) << 32) | (uint32_t)j;
            b = b < k ? b : k;
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) { const uint64_t o = shfl_xor_u64(b, m); b = b < o ? b : o; }
        if (lane == 0) {
            nn_key[i] = b;
            if (out_dist) out_dist[i] = b != KEY_NONE ? __uint_as_float((uint32_t)(b >> 32)) : -1.0f;
        }
    }
    __syncthreads();
    for (int i = tid; i < nt; i += RBLOCK) {
        const unsigned long long k = nn_key[i];
        if (k != KEY_NONE) atomicMin(&back[(uint32_t)k], (k & 0xFFFFFFFF00000000ull) | (uint32_t)i);
    }
    __syncthreads();
    for (int i = tid; i < nt; i += RBLOCK) {
        const unsigned long long k = nn_key[i];
        int m = -1;
        if (k != KEY_NONE && (uint32_t)back[(uint32_t)k] == (uint32_t)i) m = (int)(uint32_t)k;
        out_match[i] = m;
    }
}

__global__ __launch_bounds__(RBLOCK) void pair_match_kernel(MatchArgs a) {
    __shared__ uint32_t rs[3 * (MAX_SIDE / 32) + 2];                  // resolve_body: two masks and the prefix sums of a frame of up to MAX_SIDE descriptors
    const PairJob P = a.pairs[blockIdx.x];
    if (a.mode == LCD_MATCH_CROSS_CHECK) cross_check_pair(a, P);
    else dictionary_pair(a, P, rs);
}

}  // namespace
}  // namespace lcd

using namespace lcd;

namespace {

int match_pairs(lcd_engine* h, const lcd_match_args* a, bool on_device) {
    const char* who = on_device ? "lcd_match_pairs_dev" : "lcd_match_pairs";
    auto bad = [&](int code, const char* what) { return h->fail(code, std::string(who) + ": " + what); };
    // ---- everything that can be refused is refused before anything is enqueued or written
    if (!a || a->struct_size != (int32_t)sizeof(lcd_match_args)) return bad(LCD_ERR_INVALID, "null arguments or wrong struct_size");
    if (a->mode != LCD_MATCH_DICTIONARY && a->mode != LCD_MATCH_CROSS_CHECK) return bad(LCD_ERR_INVALID, "unknown mode");
    if (a->n_pairs < 0) return bad(LCD_ERR_INVALID, "negative n_pairs");
    if (a->n_pairs > 65535) return bad(LCD_ERR_UNSUPPORTED, "more than 65535 pairs per call");
    if (on_device && rows_padded(h)) return bad(LCD_ERR_UNSUPPORTED, "the handle's rows are padded: a [n x dim] device buffer is not what the kernels walk");
    if (a->n_pairs == 0) return LCD_OK;
    const int np = a->n_pairs;
    const bool dict = a->mode == LCD_MATCH_DICTIONARY;
    const int64_t* fo = a->from_offsets; const int64_t* to = a->to_offsets;
    if (!fo || !to || fo[0] != 0 || to[0] != 0) return bad(LCD_ERR_INVALID, "offsets missing or not starting at 0");
    for (int p = 0; p < np; ++p) if (fo[p + 1] < fo[p] || to[p + 1] < to[p]) return bad(LCD_ERR_INVALID, "decreasing offsets");
    for (int p = 0; p < np; ++p)
        if (fo[p + 1] - fo[p] > MAX_SIDE || to[p + 1] - to[p] > MAX_SIDE) return bad(LCD_ERR_UNSUPPORTED, "more than 8192 rows on one side of a pair");
    const int64_t nfrom = fo[np], nto = to[np];
    if ((nfrom > 0 && !a->from) || (nto > 0 && !a->to)) return bad(LCD_ERR_INVALID, "null rows");
    // (an output of zero rows is not needed)
    if (dict && ((nfrom > 0 && !a->out_from_word_ids) || (nto > 0 && !a->out_to_word_ids))) return bad(LCD_ERR_INVALID, "dictionary mode needs out_from_word_ids and out_to_word_ids");
    if (!dict && nto > 0 && !a->out_to_match) return bad(LCD_ERR_INVALID, "cross-check mode needs out_to_match");
    if (dict && !(a->flags & ::LCD_Q_INCREMENTAL)) return bad(LCD_ERR_INVALID, "dictionary mode needs LCD_Q_INCREMENTAL (a fixed dictionary without indexed words matches nothing)");
    const bool with_ids = dict && a->from_word_ids != nullptr;
    if (with_ids && !on_device) {
        std::vector<int32_t> s;
        for (int p = 0; p < np; ++p) {
            s.assign(a->from_word_ids + fo[p], a->from_word_ids + fo[p + 1]);
            std::sort(s.begin(), s.end());
            if (!s.empty() && s.front() <= 0) return bad(LCD_ERR_INVALID, "from_word_ids must be > 0");
            if (std::adjacent_find(s.begin(), s.end()) != s.end()) return bad(LCD_ERR_INVALID, "from_word_ids repeat within a pair");
        }
    }
    if (nfrom == 0 && nto == 0) return LCD_OK;
    const bool together = dict && (a->flags & ::LCD_Q_NEW_WORDS_COMPARED);
    StatelessScratch& S = h->pairs;
    hipStream_t st = h->stream;

    // ---- host entry: rows and ids to the device, results back at the end (one synchronisation)
    const void* d_from = a->from; const void* d_to = a->to; const int32_t* d_ids = with_ids ? a->from_word_ids : nullptr;
    int32_t* d_out_a = dict ? a->out_from_word_ids : a->out_to_match;      // per from-row (dictionary) / per to-row (cross-check)
    void* d_out_b = dict ? (void*)a->out_to_word_ids : (void*)a->out_to_dist;
    HostStage stage(S, host_row_bytes(h), (size_t)h->row_bytes, on_device);
    stage.in_rows(d_from, nfrom); stage.in_rows(d_to, nto);
    stage.in(d_ids, (size_t)nfrom * 4);
    stage.out(d_out_a, (size_t)(dict ? nfrom : nto) * 4); stage.out(d_out_b, (size_t)nto * 4);    // (cross-check without out_to_dist: null stays null)
    LCD_HIP(h, stage.commit(st, &h->bytes_device));
    MatchArgs m;
    LCD_HIP(h, S.ones_row(&m.ones, MAX_SIDE / 8, st, &h->bytes_device));

    // ---- consecutive groups of pairs whose distance blocks fit the budget (a single pair always does)
    auto dist_floats = [&](int nf, int nt) {
        int64_t n = (int64_t)nt * ld_of(nf);
        if (together) n += (int64_t)nf * ld_of(nf) + (int64_t)nt * ld_of(nt);
        return n;
    };
    const int64_t budget = (S.budget_bytes > 0 ? S.budget_bytes : (256ll << 20)) / 4;
    std::vector<PairJob> pj; std::vector<TileJob> tj;
    for (int p0 = 0; p0 < np;) {
        pj.clear(); tj.clear();
        int64_t floats = 0, words = 0, tiles = 0;
        int p = p0;
        for (; p < np; ++p) {
            const int nf = (int)(fo[p + 1] - fo[p]), nt = (int)(to[p + 1] - to[p]);
            const int64_t need = dist_floats(nf, nt);
            if (p > p0 && floats + need > budget) break;
            PairJob J;
            J.from_row = fo[p]; J.to_row = to[p]; J.nf = nf; J.nt = nt; J.small = words;
            J.d_tf = floats; J.d_ff = J.d_tf + (int64_t)nt * ld_of(nf); J.d_tt = J.d_ff + (together ? (int64_t)nf * ld_of(nf) : 0);
            auto block = [&](int64_t a_row, int na, int64_t b_row, int nb, int64_t out, int sides) {
                if (na <= 0 || nb <= 0) return;
                TileJob T;
                T.tile_first = tiles; T.a_row = a_row; T.b_row = b_row; T.out = out; T.na = na; T.nb = nb; T.ld = ld_of(nb); T.sides = sides;
                tiles += (int64_t)((na + TILE_A - 1) / TILE_A) * ((nb + TILE_B - 1) / TILE_B);
                tj.push_back(T);
            };
            block(to[p], nt, fo[p], nf, J.d_tf, 1);
            if (together) { block(fo[p], nf, fo[p], nf, J.d_ff, 0); block(to[p], nt, to[p], nt, J.d_tt, 3); }
            floats += need;
            words += even(small_words(a->mode, nf, nt, together));
            pj.push_back(J);
        }
        const size_t pj_bytes = pj.size() * sizeof(PairJob), tj_bytes = tj.size() * sizeof(TileJob);
        LCD_HIP(h, dreserve(h, S.d_dist, (size_t)std::max<int64_t>(floats, 1) * 4));
        LCD_HIP(h, dreserve(h, S.d_small, (size_t)std::max<int64_t>(words, 2) * 4));
        LCD_HIP(h, S.upload_table(&m.pairs, st, &h->bytes_device, pj.data(), pj_bytes, tj.data(), tj_bytes));
        const TileJob* d_tiles = (const TileJob*)((const char*)m.pairs + pj_bytes);   // the tile jobs follow the pair jobs
        LCD_HIP(h, launch_pair_dist(h->dtype, h->kdim, d_from, d_to, d_tiles, (int)tj.size(), tiles, S.d_dist.as<float>(), st));
        m.dist = S.d_dist.as<float>(); m.small = S.d_small.as<uint32_t>();
        m.mode = a->mode; m.flags = a->flags; m.nndr = a->nndr_ratio; m.from_ids = d_ids;
        m.out_from = dict ? d_out_a : nullptr; m.out_to = dict ? (int32_t*)d_out_b : nullptr;
        m.out_match = dict ? nullptr : d_out_a; m.out_dist = dict ? nullptr : (float*)d_out_b;
        pair_match_kernel<<<dim3((unsigned)pj.size()), dim3(RBLOCK), 0, st>>>(m);
        LCD_HIP(h, hipGetLastError());
        p0 = p;
    }
    LCD_HIP(h, stage.finish(st));
    return LCD_OK;
}

}  // namespace

extern "C" {

int lcd_match_pairs(lcd_engine* h, const lcd_match_args* a) { return stateless_entry(h, "lcd_match_pairs", match_pairs, a, false); }
int lcd_match_pairs_dev(lcd_engine* h, const lcd_match_args* a) { return stateless_entry(h, "lcd_match_pairs", match_pairs, a, true); }

}  // extern "C"
