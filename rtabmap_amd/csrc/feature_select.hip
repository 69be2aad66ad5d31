// feature_select.hip -- lcd_select_features / lcd_expand_word_ids and their _dev forms: the quantisation glue of Memory::createSignature
// (reference Memory.cpp:5941-6059) for a caller whose extractor leaves responses, positions and descriptors in device memory.  The selection
// is Feature2D::limitKeypoints (Features2d.cpp:293-516) by the rule include/lcd.h writes down, the expansion puts the word ids back onto all
// features and numbers the ones without a word -1, -2, ... (:6029-6059).  Any number of frames per call, one launch each:
//   feature_select_kernel: one workgroup per frame.  A frame that is not cut writes the identity.  A cut frame builds one 64-bit key per
//     feature in LDS -- cell || the complement of (masked response bits || index) -- and sorts them ascending (bitonic, padded to a power of
//     two with all-ones keys, three steps of the network per round trip through LDS): the cells follow each other, the strongest feature
//     of a cell first.  A feature's rank within its cell is its position minus the position where its cell starts; "selected" is
//     rank < limit.  BY_RESPONSE writes the sorted prefix; KEEP_ORDER sets one bit per selected feature and compacts the bits in feature
//     order with a ballot scan.  Rows and the caller's payload are gathered behind the index list with 16-byte copies where addresses and
//     sizes allow, 4-byte copies otherwise.
//   expand_word_ids_kernel: one workgroup per frame; the resolved ids are scattered into an LDS image of the frame, then a ballot scan over
//     "has no word" in feature order hands out -1, -2, ...
//   ssc_select_kernel: a call with LCD_SELECT_SSC (Kp/SSC, util2d::SSC's square covering) launches this kernel INSTEAD, one workgroup per
//     frame as well.  A cut frame sorts (complement of the mapped response bits || index), keeps the sorted indices as 16-bit words and
//     runs the reference's binary search over the width with wave-uniform scalars.  An iteration: all threads compute the cell of every
//     sorted position and clear an open-addressed table of SELECTED cells (the reference's byte mask is never built); wave 0 walks the
//     sorted list 64 features at a time -- each lane probes the 25 cells around its own in the table (the covering by all earlier
//     batches), the survivors resolve the conflicts among themselves in priority order over the ballot of the living, the rest insert
//     their cells -- and leaves one bit per sorted position.  The last evaluated iteration's bits are the result whichever way the search
//     ends; they are compacted in sorted order (BY_RESPONSE) or scattered to feature order first (KEEP_ORDER).
// Nothing of the engine is read or written: the job table and the host entries' staging are StatelessScratch's (stateless_scratch.h), as for lcd_match_pairs and lcd_match_guided.
#include "engine_impl.h"
#include "compact_body.cuh"
#include "ssc_rule.h"

#include <cmath>
#include <vector>

static_assert(sizeof(lcd_select_args) == 120, "lcd_select_args: the layout include/lcd.h documents (LP64)");
static_assert(sizeof(lcd_expand_args) == 64, "lcd_expand_args: the layout include/lcd.h documents (LP64)");

namespace lcd {
namespace {

constexpr int MAX_FEATURES = 16384;          // features in one frame: 128 KiB of 64-bit keys (144 KiB with their padding) in one workgroup's LDS
constexpr int MAX_CELLS = 1024;
constexpr int IDX_BITS = 14;                 // an index within a frame
constexpr int STRENGTH_BITS = 31 + IDX_BITS; // masked response bits || index
constexpr uint64_t STRENGTH_MASK = (1ull << STRENGTH_BITS) - 1;
constexpr int SMALL_BLOCK = 256, BIG_BLOCK = 1024;
constexpr int SMALL_FRAME = 2048;            // the largest frame a call of 256-thread workgroups serves
constexpr int MAX_WAVES = BIG_BLOCK / 64;

struct FrameJob {
    int64_t first;                           // the frame's first feature in every array
    int32_t n;                               // the frame's region; with n_in / n_features the device knows how much of it is the frame
    int32_t row_size, col_size;              // pixels per grid cell (1 where the frame is not cut)
    int32_t pad;
};

struct SelectArgs {
    const FrameJob* jobs;
    int order, max_features, grid_rows, grid_cols;
    int p_max;                               // keys the LDS carve holds (a power of two >= every cut frame)
    int row_bytes, row_vec, aux_bytes, aux_vec;   // *_vec: 16 or 4, the widest copy the addresses and sizes allow
    const float* response; const float2* points; const void* rows; const void* aux;
    const int32_t* n_in;                     // may be null: per frame, how many features of the region are the frame (clamped)
    int32_t* out_count; int32_t* out_index; void* out_rows; void* out_aux;
};

// a frame of a call with LCD_SELECT_SSC: what util2d.cpp:2299-2319 computes from max_features and the image size (ssc::plan)
struct SscJob {
    int64_t first;
    int32_t n;
    int32_t m, high, k_min, k_max;           // low needs n: the device's
    int32_t cols, rows;                      // the image (1 x 1 where the frame's region is not cut)
    int32_t pad;
};

struct ExpandArgs {
    const FrameJob* jobs;
    const int32_t* count; const int32_t* index; const int32_t* word_ids; const int32_t* first_new_word_id;
    const int32_t* n_features;               // may be null: as SelectArgs::n_in
    int32_t* out_word_ids;
};

extern __shared__ __attribute__((aligned(16))) unsigned char fs_smem[];

// what every frame ends with: -1 behind the selected indices to the end of the region, the count, the rows and the payload behind the list
__device__ __forceinline__ void finish_frame(const SelectArgs& a, int64_t first, int region, int32_t* out_index, int count) {
    const int tid = threadIdx.x, T = blockDim.x;
    for (int i = count + tid; i < region; i += T) out_index[i] = -1;
    if (tid == 0) a.out_count[blockIdx.x] = count;
    if (!a.rows && !a.aux) return;
    __syncthreads();                                                   // the index list is read back by the threads that gather
    if (a.rows) {
        if (a.row_vec == 16) gather_rows<uint4>(a.rows, a.out_rows, out_index, first, count, a.row_bytes);
        else gather_rows<uint32_t>(a.rows, a.out_rows, out_index, first, count, a.row_bytes);
    }
    if (a.aux) {
        if (a.aux_vec == 16) gather_rows<uint4>(a.aux, a.out_aux, out_index, first, count, a.aux_bytes);
        else gather_rows<uint32_t>(a.aux, a.out_aux, out_index, first, count, a.aux_bytes);
    }
}

__global__ __launch_bounds__(BIG_BLOCK) void feature_select_kernel(SelectArgs a) {
    const FrameJob J = a.jobs[blockIdx.x];
    const int n = a.n_in ? min(max(a.n_in[blockIdx.x], 0), J.n) : J.n, tid = threadIdx.x, T = blockDim.x;
    const int n_cells = a.grid_rows * a.grid_cols;
    uint64_t* keys = reinterpret_cast<uint64_t*>(fs_smem);
    uint32_t* sel = reinterpret_cast<uint32_t*>(fs_smem + (size_t)padded(a.p_max) * 8);   // one bit per feature
    int32_t* cell_start = reinterpret_cast<int32_t*>(sel + a.p_max / 32);             // [n_cells + 1]: the last entry is "outside the grid"
    int* wsum = cell_start + n_cells + 1;
    int32_t* out_index = a.out_index + J.first;
    const bool cut = a.max_features > 0 && n > a.max_features;
    int count = n;

    if (!cut) {
        for (int i = tid; i < n; i += T) out_index[i] = i;             // the reference does not sort what it does not cut
    } else {
        int p2 = 2;
        while (p2 < n) p2 <<= 1;                                       // <= p_max
        const bool grid = n_cells > 1;
        for (int i = tid; i < p2; i += T) {
            uint64_t key = ~0ull;                                      // padding sorts last
            if (i < n) {
                uint32_t cell = 0;
                if (grid) {
                    const float2 p = a.points[J.first + i];
                    const int cr = __float2int_rz(p.y) / J.row_size, cc = __float2int_rz(p.x) / J.col_size;   // int(y) / rowSize: both truncate toward zero
                    const bool inside = cr >= 0 && cr < a.grid_rows && cc >= 0 && cc < a.grid_cols;
                    cell = inside ? (uint32_t)(cr * a.grid_cols + cc) : (uint32_t)n_cells;
                }
                const uint64_t strength = ((uint64_t)(__float_as_uint(a.response[J.first + i]) & 0x7fffffffu) << IDX_BITS) | (uint32_t)i;
                key = ((uint64_t)cell << STRENGTH_BITS) | (STRENGTH_MASK - strength);
            }
            keys[padded(i)] = key;
        }
        for (int w = tid; w < (n + 31) / 32; w += T) sel[w] = 0u;
        __syncthreads();
        bitonic_sort(keys, p2);
        for (int p = tid; p < n; p += T) {
            const int c = (int)(keys[padded(p)] >> STRENGTH_BITS);
            if (p == 0 || (int)(keys[padded(p - 1)] >> STRENGTH_BITS) != c) cell_start[c] = p;
        }
        __syncthreads();
        const int limit = grid ? a.max_features / n_cells : a.max_features;          // perCell == 0: the whole cell stays
        const bool by_response = a.order == LCD_SELECT_BY_RESPONSE;
        for (int p = tid; p < n; p += T) {
            const uint64_t key = keys[padded(p)];
            const int c = (int)(key >> STRENGTH_BITS);
            const int i = (int)((STRENGTH_MASK - (key & STRENGTH_MASK)) & ((1u << IDX_BITS) - 1));
            const bool chosen = c < n_cells && (limit <= 0 || p - cell_start[c] < limit);
            if (!chosen) continue;
            if (by_response) out_index[p] = i;                                        // (1 x 1 grid: the position is the rank)
            else atomicOr(&sel[i >> 5], 1u << (i & 31));
        }
        __syncthreads();
        if (by_response) {
            count = a.max_features;
        } else {
            count = 0;
            for (int base = 0; base < n; base += T) {
                const int i = base + tid;
                const bool flag = i < n && ((sel[i >> 5] >> (i & 31)) & 1u);
                int total;
                const int pos = count + block_rank(flag, wsum, total);
                if (flag) out_index[pos] = i;
                count += total;
            }
        }
    }
    finish_frame(a, J.first, J.n, out_index, count);
}

// ---- LCD_SELECT_SSC
constexpr uint32_t SSC_EMPTY = ssc::NO_CELL;                           // no cell has row and column 65535

__device__ __forceinline__ uint32_t ssc_slot(uint32_t cell, int shift) { return (cell * 0x9E3779B1u) >> shift; }

// is `cell` among the selected cells?  (the table is never full: twice as many slots as sorted positions)
__device__ __forceinline__ bool ssc_selected(const volatile uint32_t* table, uint32_t mask, int shift, uint32_t cell) {
    for (uint32_t s = ssc_slot(cell, shift);; s = (s + 1) & mask) {
        const uint32_t v = table[s];
        if (v == cell) return true;
        if (v == SSC_EMPTY) return false;
    }
}

// One iteration's greedy covering, by ONE wave: bit p of `plane` = sorted position p is selected; returns how many are.  cells[p] is the
// cell of sorted position p or NO_CELL; the table is all SSC_EMPTY on entry.  The walk ends as soon as more than `stop_above` are selected:
// the caller passes Kmax where "too many" is all the search will ever ask of this iteration (its bits are then incomplete).
__device__ __forceinline__ int ssc_walk(const uint32_t* cells, uint32_t* table, uint32_t mask, int shift, uint32_t* plane, int n, int stop_above) {
    const int lane = threadIdx.x & 63;
    int size = 0;
    for (int base = 0; base < n; base += 64) {
        const int p = base + lane;
        const uint32_t cell = p < n ? cells[p] : ssc::NO_CELL;
        const int row = (int)(cell >> 16), col = (int)(cell & 0xffffu);
        bool alive = cell != ssc::NO_CELL;
        if (alive) {                                                   // covered by an earlier batch?
            for (int dr = -2; dr <= 2 && alive; ++dr) {
                const int r = row + dr;
                if (r < 0) continue;
                for (int dc = -2; dc <= 2; ++dc) {
                    const int c = col + dc;                            // (at most 32770: stays in its 16 bits)
                    if (c >= 0 && ssc_selected(table, mask, shift, ((uint32_t)r << 16) | (uint32_t)c)) { alive = false; break; }
                }
            }
        }
        // ... or by a lane before it in this batch that stays selected: only lanes that are alive when their turn comes are broadcast
        unsigned long long live = __ballot(alive), todo = live;
        while (todo) {
            const int l = __ffsll((long long)todo) - 1;
            const uint32_t first = (uint32_t)__builtin_amdgcn_readlane((int)cell, l);
            const int fr = (int)(first >> 16), fc = (int)(first & 0xffffu);
            if (alive && lane > l && abs(row - fr) <= 2 && abs(col - fc) <= 2) alive = false;
            live = __ballot(alive);
            todo = l == 63 ? 0ull : live & ~((2ull << l) - 1ull);
        }
        if (alive) {
            uint32_t s = ssc_slot(cell, shift);
            while (atomicCAS(&table[s], SSC_EMPTY, cell) != SSC_EMPTY) s = (s + 1) & mask;
        }
        if (lane == 0) { plane[base >> 5] = (uint32_t)live; plane[(base >> 5) + 1] = (uint32_t)(live >> 32); }
        size += __popcll(live);
        if (size > stop_above) break;
        __threadfence_block();                                         // the next batch probes what this one inserted
    }
    return size;
}

__global__ __launch_bounds__(BIG_BLOCK) void ssc_select_kernel(SelectArgs a, const SscJob* jobs, int p_max) {
    const SscJob J = jobs[blockIdx.x];
    const int n = a.n_in ? min(max(a.n_in[blockIdx.x], 0), J.n) : J.n, tid = threadIdx.x, T = blockDim.x;
    // LDS: the sort's keys; behind the sort they give way to the sorted indices, the cells and the table of selected cells
    uint64_t* keys = reinterpret_cast<uint64_t*>(fs_smem);
    uint16_t* sorted = reinterpret_cast<uint16_t*>(fs_smem);                              // [p_max]: feature of sorted position p
    uint32_t* cells = reinterpret_cast<uint32_t*>(fs_smem + (size_t)p_max * 2);           // [p_max]
    uint32_t* table = reinterpret_cast<uint32_t*>(fs_smem + (size_t)p_max * 6);           // [2 p_max]; at the end the KEEP_ORDER bits
    uint32_t* plane = reinterpret_cast<uint32_t*>(fs_smem + (size_t)p_max * 14);          // [p_max / 32]
    int* wsum = reinterpret_cast<int*>(plane + p_max / 32);
    __shared__ int s_size;
    int32_t* out_index = a.out_index + J.first;
    const bool cut = a.max_features > 0 && n > a.max_features;
    int count = n;

    if (!cut) {
        for (int i = tid; i < n; i += T) out_index[i] = i;
    } else {
        int p2 = 64;
        while (p2 < n) p2 <<= 1;                                       // <= p_max
        for (int i = tid; i < p2; i += T) {
            uint64_t key = ~0ull;                                      // padding sorts last
            if (i < n) key = ((uint64_t)(~ssc::mapped_bits(__float_as_uint(a.response[J.first + i]))) << IDX_BITS) | (uint32_t)i;
            keys[padded(i)] = key;
        }
        __syncthreads();
        bitonic_sort(keys, p2);
        // keys -> 16-bit indices in place, ascending: the words chunk k writes lie below the keys of every later chunk
        for (int base = 0; base < p2; base += T) {
            const int p = base + tid;
            const uint64_t key = p < p2 ? keys[padded(p)] : 0ull;
            __syncthreads();
            if (p < p2) sorted[p] = (uint16_t)(key & ((1u << IDX_BITS) - 1));
        }
        for (int w = tid; w < p2 / 32; w += T) plane[w] = 0u;         // the search may end before its first iteration: nothing selected
        const uint32_t mask = 2u * (uint32_t)p2 - 1u;
        const int shift = __clz(2 * p2) + 1;                           // 32 - log2(2 p2)
        int low = ssc::low_of(n, J.m), high = J.high, prev_width = -1;
        count = 0;
        for (;;) {                                                     // every scalar here is the same for the whole workgroup
            const int width = low + (high - low) / 2;
            if (width == prev_width || low > high) break;              // the previous iteration's bits stand
            const double c = (double)width / 2.0;
            const int last_row = ssc::last_cell(J.rows, c), last_col = ssc::last_cell(J.cols, c);
            __syncthreads();                                           // sorted[] is written; the last iteration's walk is over
            for (int p = tid; p < n; p += T) {
                const float2 pt = a.points[J.first + sorted[p]];
                cells[p] = ssc::cell_of(pt.x, pt.y, c, last_row, last_col);
            }
            for (int s = tid; s < 2 * p2; s += T) table[s] = SSC_EMPTY;
            __syncthreads();
            // "Too many" sets low = width + 1.  Unless the search then stops (the same width again, or low > high), another iteration replaces
            // this one's result, and the walk may end at Kmax + 1 selected.
            const int next_low = width + 1, next_width = next_low + (high - next_low) / 2;
            const bool last_if_many = next_width == width || next_low > high;
            if (tid < 64) {
                const int size = ssc_walk(cells, table, mask, shift, plane, n, last_if_many ? 0x7fffffff : J.k_max);
                if (tid == 0) s_size = size;
            }
            __syncthreads();
            count = s_size;
            if (count >= J.k_min && count <= J.k_max) break;
            if (count < J.k_min) high = width - 1;
            else low = width + 1;
            prev_width = width;
        }
        __syncthreads();
        const bool by_response = a.order == LCD_SELECT_BY_RESPONSE;
        const uint32_t* bits = plane;                                  // BY_RESPONSE: the sorted positions' bits are the output's order
        if (!by_response) {                                            // KEEP_ORDER: one bit per FEATURE
            for (int w = tid; w < p2 / 32; w += T) table[w] = 0u;
            __syncthreads();
            for (int p = tid; p < n; p += T)
                if ((plane[p >> 5] >> (p & 31)) & 1u) { const int i = sorted[p]; atomicOr(&table[i >> 5], 1u << (i & 31)); }
            __syncthreads();
            bits = table;
        }
        count = 0;
        for (int base = 0; base < n; base += T) {
            const int i = base + tid;
            const bool flag = i < n && ((bits[i >> 5] >> (i & 31)) & 1u);
            int total;
            const int pos = count + block_rank(flag, wsum, total);
            if (flag) out_index[pos] = by_response ? (int)sorted[i] : i;
            count += total;
        }
    }
    finish_frame(a, J.first, J.n, out_index, count);
}

__global__ __launch_bounds__(BIG_BLOCK) void expand_word_ids_kernel(ExpandArgs a, int n_max) {
    const FrameJob J = a.jobs[blockIdx.x];
    const int n = a.n_features ? min(max(a.n_features[blockIdx.x], 0), J.n) : J.n, tid = threadIdx.x, T = blockDim.x;
    int32_t* all = reinterpret_cast<int32_t*>(fs_smem);                // the frame's resolved ids, 0 = no word
    int* wsum = all + n_max;
    const int count = min(max(a.count[blockIdx.x], 0), n);
    const int32_t first_id = a.first_new_word_id ? a.first_new_word_id[blockIdx.x] : 0;
    for (int i = tid; i < n; i += T) all[i] = 0;
    __syncthreads();
    for (int j = tid; j < count; j += T) {
        const int32_t i = a.index[J.first + j];
        if (i < 0 || i >= n) continue;                                 // (the host entry refuses it)
        const int32_t w = a.word_ids[J.first + j];
        int32_t id = w;
        if (w < 0) id = first_id > 0 ? (int32_t)((uint32_t)first_id + (uint32_t)(-(w + 1))) : 0;   // the code -(k+1): first + k
        if (id > 0) all[i] = id;
    }
    __syncthreads();
    int negatives = 0;
    for (int base = 0; base < n; base += T) {
        const int i = base + tid;
        const int32_t id = i < n ? all[i] : 1;
        int total;
        const int rank = negatives + block_rank(id <= 0, wsum, total);
        if (i < n) a.out_word_ids[J.first + i] = id > 0 ? id : -(rank + 1);
        negatives += total;
    }
    for (int i = n + tid; i < J.n; i += T) a.out_word_ids[J.first + i] = 0;   // behind the frame, to the end of the region
}

inline size_t select_lds(int p_max, int n_cells) { return ((size_t)padded(p_max) * 8 + (size_t)p_max / 8 + (size_t)(n_cells + 1) * 4 + MAX_WAVES * 4 + 15) & ~(size_t)15; }
inline size_t ssc_lds(int p_max) { return ((size_t)p_max * 14 + (size_t)p_max / 8 + MAX_WAVES * 4 + 15) & ~(size_t)15; }   // (the keys, 9 p_max bytes, fit below)
inline size_t expand_lds(int n_max) { return ((size_t)n_max * 4 + MAX_WAVES * 4 + 15) & ~(size_t)15; }

// the largest frames need more than the default 64 KiB of dynamic LDS.  (Not motion_group.cuh's allow_large_lds<kernel>: that sets one
// limit for every kernel, these three each need their own.)
void allow_large_lds() {
    static const bool once = [] {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(&feature_select_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)select_lds(MAX_FEATURES, MAX_CELLS)) != hipSuccess) (void)hipGetLastError();
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(&ssc_select_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)ssc_lds(ssc::MAX_FEATURES)) != hipSuccess) (void)hipGetLastError();
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(&expand_word_ids_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)expand_lds(MAX_FEATURES)) != hipSuccess) (void)hipGetLastError();
        return true;
    }();
    (void)once;
}

}  // namespace
}  // namespace lcd

using namespace lcd;

namespace {

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// offsets, the limits every entry shares; *n_max: the largest frame
int check_frames(lcd_engine* h, const char* who, int32_t n_frames, const int64_t* off, int* n_max) {
    auto bad = [&](int code, const char* what) { return h->fail(code, std::string(who) + ": " + what); };
    if (n_frames < 0) return bad(LCD_ERR_INVALID, "negative n_frames");
    if (n_frames > 65535) return bad(LCD_ERR_UNSUPPORTED, "more than 65535 frames per call");
    if (h->shard_append || h->shard_first || h->shard_block) return bad(LCD_ERR_UNSUPPORTED, "not offered on the handles of a sharded vocabulary");
    *n_max = 0;
    if (n_frames == 0) return LCD_OK;
    if (!off || off[0] != 0) return bad(LCD_ERR_INVALID, "offsets missing or not starting at 0");
    for (int f = 0; f < n_frames; ++f) if (off[f + 1] < off[f]) return bad(LCD_ERR_INVALID, "decreasing offsets");
    for (int f = 0; f < n_frames; ++f) {
        if (off[f + 1] - off[f] > MAX_FEATURES) return bad(LCD_ERR_UNSUPPORTED, "more than 16384 features in a frame");
        *n_max = std::max(*n_max, (int)(off[f + 1] - off[f]));
    }
    return LCD_OK;
}

// int(v) as the device converts it: toward zero, saturating, NaN -> 0
inline int to_int_rz(float v) {
    if (std::isnan(v)) return 0;
    if (v >= 2147483648.0f) return 2147483647;
    if (v <= -2147483648.0f) return -2147483647 - 1;
    return (int)v;
}

int select_features(lcd_engine* h, const lcd_select_args* a, bool on_device) {
    const char* who = on_device ? "lcd_select_features_dev" : "lcd_select_features";
    auto bad = [&](int code, const char* what) { return h->fail(code, std::string(who) + ": " + what); };
    // ---- everything that can be refused is refused before anything is enqueued or written
    if (!a || a->struct_size != (int32_t)sizeof(lcd_select_args)) return bad(LCD_ERR_INVALID, "null arguments or wrong struct_size");
    if (a->order != LCD_SELECT_KEEP_ORDER && a->order != LCD_SELECT_BY_RESPONSE) return bad(LCD_ERR_INVALID, "unknown order");
    if (a->grid_rows < 1 || a->grid_cols < 1) return bad(LCD_ERR_INVALID, "grid_rows and grid_cols are >= 1");
    if ((int64_t)a->grid_rows * a->grid_cols > MAX_CELLS) return bad(LCD_ERR_UNSUPPORTED, "more than 1024 grid cells");
    const bool grid = a->grid_rows * a->grid_cols > 1;
    if (grid && a->order == LCD_SELECT_BY_RESPONSE) return bad(LCD_ERR_INVALID, "LCD_SELECT_BY_RESPONSE has no grid variant");
    const bool by_ssc = (a->flags & LCD_SELECT_SSC) != 0;              // the other bits are ignored
    if (by_ssc && grid) return bad(LCD_ERR_INVALID, "LCD_SELECT_SSC with a grid above 1 x 1: the reference indexes its mask outside its bounds");
    if (by_ssc && a->max_features == 1) return bad(LCD_ERR_INVALID, "LCD_SELECT_SSC with max_features == 1: the reference divides by zero");
    if (a->aux_bytes < 0 || a->aux_bytes > 64 || a->aux_bytes % 4) return bad(LCD_ERR_INVALID, "aux_bytes is a multiple of 4, 0..64");
    int n_max = 0;
    if (int rc = check_frames(h, who, a->n_frames, a->offsets, &n_max)) return rc;
    const bool with_rows = a->rows != nullptr, with_aux = a->aux != nullptr && a->aux_bytes > 0;
    if (on_device && with_rows && rows_padded(h)) return bad(LCD_ERR_UNSUPPORTED, "the handle's rows are padded: a [n x dim] device buffer is not what the kernel walks");
    if (a->n_frames == 0) return LCD_OK;
    const int nf = a->n_frames;
    const int64_t* off = a->offsets;
    const int64_t N = off[nf];
    if (!a->out_count) return bad(LCD_ERR_INVALID, "null out_count");
    if (N > 0 && (!a->response || !a->out_index)) return bad(LCD_ERR_INVALID, "null response or out_index");
    if (N > 0 && ((with_rows && !a->out_rows) || (with_aux && !a->out_aux))) return bad(LCD_ERR_INVALID, "rows or aux without an output");
    if (N > 0 && grid && (!a->points || !a->image_size)) return bad(LCD_ERR_INVALID, "a grid needs points and image sizes");
    // the host entry knows n_in: what it checks per feature ends where the frame ends
    auto frame_n = [&](int f) { const int64_t r = off[f + 1] - off[f]; return !on_device && a->n_in ? std::min<int64_t>(std::max<int64_t>(a->n_in[f], 0), r) : r; };
    std::vector<FrameJob> jobs((size_t)(by_ssc ? 0 : nf));
    std::vector<SscJob> ssc_jobs((size_t)(by_ssc ? nf : 0));
    int cut_max = 0;
    for (int f = 0; f < nf && by_ssc; ++f) {
        SscJob& J = ssc_jobs[(size_t)f];
        J.first = off[f]; J.n = (int32_t)(off[f + 1] - off[f]); J.m = 2; J.high = 0; J.k_min = J.k_max = 0; J.cols = J.rows = 1; J.pad = 0;
        if (!(a->max_features > 0 && J.n > a->max_features)) continue;
        if (!a->points || !a->image_size) return bad(LCD_ERR_INVALID, "LCD_SELECT_SSC needs points and image sizes");
        if (J.n > ssc::MAX_FEATURES) return bad(LCD_ERR_UNSUPPORTED, "more than 8192 features in a frame cut under LCD_SELECT_SSC");
        cut_max = std::max(cut_max, (int)J.n);
        J.cols = a->image_size[2 * f]; J.rows = a->image_size[2 * f + 1];
        if (J.cols < 1 || J.rows < 1) return bad(LCD_ERR_INVALID, "LCD_SELECT_SSC: an image side < 1");
        if (J.cols > ssc::MAX_SIDE || J.rows > ssc::MAX_SIDE) return bad(LCD_ERR_UNSUPPORTED, "LCD_SELECT_SSC: an image side above 16384");
        ssc::Plan plan;
        if (!ssc::plan(a->max_features, J.cols, J.rows, plan)) return bad(LCD_ERR_INVALID, "LCD_SELECT_SSC: max_features outside what the reference's scalars hold");
        J.m = plan.m; J.high = plan.high; J.k_min = plan.k_min; J.k_max = plan.k_max;
    }
    for (int f = 0; f < nf && !by_ssc; ++f) {
        FrameJob& J = jobs[(size_t)f];
        J.first = off[f]; J.n = (int32_t)(off[f + 1] - off[f]); J.row_size = J.col_size = 1; J.pad = 0;
        if (!(a->max_features > 0 && J.n > a->max_features)) continue;
        cut_max = std::max(cut_max, (int)J.n);
        if (!grid) continue;
        const int32_t width = a->image_size[2 * f], height = a->image_size[2 * f + 1];
        if (height <= a->grid_rows || width <= a->grid_cols) return bad(LCD_ERR_INVALID, "the image is not larger than the grid");
        J.row_size = height / a->grid_rows; J.col_size = width / a->grid_cols;
    }
    if (!on_device) {
        for (int f = 0; f < nf; ++f)
            for (int64_t i = off[f]; i < off[f] + frame_n(f); ++i) if (std::isnan(a->response[i])) return bad(LCD_ERR_INVALID, "a NaN response has no place in the order");
        for (int f = 0; f < nf && by_ssc; ++f) {
            if (!(a->max_features > 0 && frame_n(f) > a->max_features)) continue;
            const float w = (float)ssc_jobs[(size_t)f].cols, hgt = (float)ssc_jobs[(size_t)f].rows;
            for (int64_t i = off[f]; i < off[f] + frame_n(f); ++i) {
                const float x = a->points[2 * i], y = a->points[2 * i + 1];
                if (!(x >= 0.0f && x <= w && y >= 0.0f && y <= hgt)) return bad(LCD_ERR_INVALID, "LCD_SELECT_SSC: a keypoint outside the image");   // NaN compares false
            }
        }
        if (grid)
            for (int f = 0; f < nf; ++f) {
                const FrameJob& J = jobs[(size_t)f];
                if (!(a->max_features > 0 && frame_n(f) > a->max_features)) continue;
                for (int64_t i = off[f]; i < off[f] + frame_n(f); ++i) {
                    const int cr = to_int_rz(a->points[2 * i + 1]) / J.row_size, cc = to_int_rz(a->points[2 * i]) / J.col_size;
                    if (cr < 0 || cr >= a->grid_rows || cc < 0 || cc >= a->grid_cols) return bad(LCD_ERR_INVALID, "a keypoint outside the grid");
                }
            }
    }
    StatelessScratch& S = h->pairs;
    hipStream_t st = h->stream;

    SelectArgs g;
    g.order = a->order; g.max_features = a->max_features; g.grid_rows = a->grid_rows; g.grid_cols = a->grid_cols;
    const bool with_points = grid || (by_ssc && cut_max > 0);
    g.p_max = 64;
    while (g.p_max < cut_max) g.p_max <<= 1;
    g.row_bytes = h->row_bytes; g.aux_bytes = a->aux_bytes;
    g.response = a->response; g.points = (const float2*)a->points; g.rows = with_rows ? a->rows : nullptr; g.aux = with_aux ? a->aux : nullptr;
    g.n_in = a->n_in;
    g.out_count = a->out_count; g.out_index = a->out_index; g.out_rows = a->out_rows; g.out_aux = a->out_aux;

    // ---- host entry: everything to the device, results back at the end (one synchronisation)
    HostStage stage(S, host_row_bytes(h), (size_t)h->row_bytes, on_device);
    const size_t aux_bytes = with_aux ? (size_t)N * a->aux_bytes : 0;
    stage.in(g.response, (size_t)N * 4); stage.in(g.points, with_points ? (size_t)N * 8 : 0);
    stage.in_rows(g.rows, N); stage.in(g.aux, aux_bytes);
    stage.in(g.n_in, (size_t)nf * 4);                                  // optional: null stays null
    stage.out(g.out_count, (size_t)nf * 4); stage.out(g.out_index, (size_t)N * 4);
    const int o_rows = stage.out_kept(g.out_rows, with_rows ? (size_t)N * h->row_bytes : 0);     // handed out below: only what each frame selected
    const int o_aux = stage.out_kept(g.out_aux, aux_bytes);
    LCD_HIP(h, stage.commit(st, &h->bytes_device));
    g.row_vec = g.rows && g.row_bytes % 16 == 0 && aligned16(g.rows) && aligned16(g.out_rows) ? 16 : 4;
    g.aux_vec = g.aux && g.aux_bytes % 16 == 0 && aligned16(g.aux) && aligned16(g.out_aux) ? 16 : 4;

    allow_large_lds();
    const int block = n_max > SMALL_FRAME ? BIG_BLOCK : SMALL_BLOCK;
    if (by_ssc) {
        const SscJob* d_jobs = nullptr;
        g.jobs = nullptr;
        LCD_HIP(h, S.upload_table(&d_jobs, st, &h->bytes_device, ssc_jobs.data(), ssc_jobs.size() * sizeof(SscJob)));
        ssc_select_kernel<<<dim3((unsigned)nf), dim3((unsigned)block), ssc_lds(g.p_max), st>>>(g, d_jobs, g.p_max);
    } else {
        LCD_HIP(h, S.upload_table(&g.jobs, st, &h->bytes_device, jobs.data(), jobs.size() * sizeof(FrameJob)));
        feature_select_kernel<<<dim3((unsigned)nf), dim3((unsigned)block), select_lds(g.p_max, a->grid_rows * a->grid_cols), st>>>(g);
    }
    LCD_HIP(h, hipGetLastError());
    LCD_HIP(h, stage.finish(st));
    stage.hand_out_rows(o_rows, a->out_count, off, nf);                // only what the frame wrote: the rest of its region stays as it was
    stage.hand_out(o_aux, a->out_count, off, nf, (size_t)a->aux_bytes);
    return LCD_OK;
}

int expand_word_ids(lcd_engine* h, const lcd_expand_args* a, bool on_device) {
    const char* who = on_device ? "lcd_expand_word_ids_dev" : "lcd_expand_word_ids";
    auto bad = [&](int code, const char* what) { return h->fail(code, std::string(who) + ": " + what); };
    if (!a || a->struct_size != (int32_t)sizeof(lcd_expand_args)) return bad(LCD_ERR_INVALID, "null arguments or wrong struct_size");
    int n_max = 0;
    if (int rc = check_frames(h, who, a->n_frames, a->offsets, &n_max)) return rc;
    if (a->n_frames == 0) return LCD_OK;
    const int nf = a->n_frames;
    const int64_t* off = a->offsets;
    const int64_t N = off[nf];
    if (!a->count) return bad(LCD_ERR_INVALID, "null count");
    if (N > 0 && (!a->index || !a->word_ids || !a->out_word_ids)) return bad(LCD_ERR_INVALID, "null index, word_ids or out_word_ids");
    if (!on_device)
        for (int f = 0; f < nf; ++f) {
            const int64_t region = off[f + 1] - off[f];
            const int64_t n = a->n_features ? std::min<int64_t>(std::max<int64_t>(a->n_features[f], 0), region) : region;
            if (a->count[f] < 0 || a->count[f] > n) return bad(LCD_ERR_INVALID, "count outside its frame");
            for (int64_t j = off[f]; j < off[f] + a->count[f]; ++j)
                if (a->index[j] < 0 || a->index[j] >= n) return bad(LCD_ERR_INVALID, "an index entry outside its frame");
        }
    if (N == 0) return LCD_OK;
    StatelessScratch& S = h->pairs;
    hipStream_t st = h->stream;
    std::vector<FrameJob> jobs((size_t)nf);
    for (int f = 0; f < nf; ++f) jobs[(size_t)f] = FrameJob{off[f], (int32_t)(off[f + 1] - off[f]), 1, 1, 0};

    ExpandArgs g;
    g.count = a->count; g.index = a->index; g.word_ids = a->word_ids; g.first_new_word_id = a->first_new_word_id; g.out_word_ids = a->out_word_ids;
    g.n_features = a->n_features;
    HostStage stage(S, host_row_bytes(h), (size_t)h->row_bytes, on_device);
    stage.in(g.count, (size_t)nf * 4); stage.in(g.index, (size_t)N * 4); stage.in(g.word_ids, (size_t)N * 4);
    stage.in(g.first_new_word_id, (size_t)nf * 4); stage.in(g.n_features, (size_t)nf * 4);      // optional: null stays null
    stage.out(g.out_word_ids, (size_t)N * 4);
    LCD_HIP(h, stage.commit(st, &h->bytes_device));
    LCD_HIP(h, S.upload_table(&g.jobs, st, &h->bytes_device, jobs.data(), jobs.size() * sizeof(FrameJob)));
    allow_large_lds();
    const int block = n_max > SMALL_FRAME ? BIG_BLOCK : SMALL_BLOCK;
    expand_word_ids_kernel<<<dim3((unsigned)nf), dim3((unsigned)block), expand_lds(n_max), st>>>(g, n_max);
    LCD_HIP(h, hipGetLastError());
    LCD_HIP(h, stage.finish(st));
    return LCD_OK;
}

}  // namespace

extern "C" {

int lcd_select_features(lcd_engine* h, const lcd_select_args* a) { return stateless_entry(h, "lcd_select_features", select_features, a, false); }
int lcd_select_features_dev(lcd_engine* h, const lcd_select_args* a) { return stateless_entry(h, "lcd_select_features", select_features, a, true); }
int lcd_expand_word_ids(lcd_engine* h, const lcd_expand_args* a) { return stateless_entry(h, "lcd_expand_word_ids", expand_word_ids, a, false); }
int lcd_expand_word_ids_dev(lcd_engine* h, const lcd_expand_args* a) { return stateless_entry(h, "lcd_expand_word_ids", expand_word_ids, a, true); }

}  // extern "C"
