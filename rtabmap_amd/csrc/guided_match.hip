// guided_match.hip -- lcd_match_guided / lcd_match_guided_dev: the descriptors of two frames matched under a guess transform, in one
// stateless call for any number of frame pairs (reference RegistrationVis.cpp:1078-1365: what the verification runs whenever the caller has
// a guess -- proximity detection, the local loop closures in time, odometry refining, the graph's re-registration).  The caller has
// projected the from-frame's 3-D points into the to-image; a descriptor is compared only with the descriptors whose keypoints lie within
// `radius` pixels of the projection, by the rule include/lcd.h writes down.  The to x from distance block is never formed.
//
// One launch (and one fill in front of it) for the whole batch:
//   guided_match_kernel: a linear grid over (pair, block of QBLOCK queries), the pair found by binary search in the job table as
//     pair_dist_kernel finds its block (pair_match.hip).  The workgroup stages the pair's target points in LDS (at most 8192 x 8 B); each
//     of its four waves then takes one query at a time: it walks the target points 64 at a time, applies the window test (rtflann's
//     L2_Simple, every operation rounded), and appends the hits behind a ballot to its own LDS list.  Whenever the list holds 64 entries,
//     and once more at the end, it is drained with one lane per candidate: the query's descriptor is wave-uniform, the lane gathers its
//     target's row and computes the whole distance alone -- dist_ref.cuh's arithmetic, the reference's summation order -- and keeps its two
//     smallest keys (distance bits << 32 | target index: the lowest index wins ties, top2_keys.cuh).  A wave reduction ends the query.
//   the first-come rule (projected-to-frame): out_to_owner is filled with 0xFF bytes in front of the launch and every decision is an
//     unsigned 32-bit atomicMin of the corner index on its to-row: a row nobody chose still reads -1.
// Nothing of the engine is read or written: job tables and staged rows are StatelessScratch's (stateless_scratch.h), as for lcd_match_pairs.
#include "engine_impl.h"
#include "dist_ref.cuh"
#include "top2_keys.cuh"

#include <cmath>
#include <vector>

static_assert(sizeof(lcd_guided_args) == 120, "lcd_guided_args: the layout include/lcd.h documents (LP64)");

namespace lcd {
namespace {

constexpr int GBLOCK = 256;                  // four waves
constexpr int GWAVES = GBLOCK / 64;
constexpr int QBLOCK = 16;                   // queries per workgroup (four per wave, one at a time)
constexpr int MAX_SIDE = 8192;               // rows or corners on one side of a pair (the staged target points: 64 KiB of LDS)
constexpr int LIST = 128;                    // a wave's candidate list: fewer than 64 left over + at most 64 appended

struct GuidedJob {
    int64_t from_row, to_row, corner_row;    // the pair's first from-row / to-row / corner (also where its outputs start)
    int32_t nf, nt, nc;
    int32_t block_first;                     // the pair's first workgroup in the launch's linear grid
};

struct GuidedArgs {
    const GuidedJob* jobs; int n_jobs;
    int direction, nn_type, kdyn;            // kdyn: dwords per row
    float r2, nndr;
    const void* from; const void* to;
    const float2* corners; const int32_t* corner_from_row; const float2* to_points;
    int32_t* out_count; int32_t* out_match; float* out_dist; uint32_t* out_to_owner;
};

// the distances of up to 64 listed targets against the wave's query: lane l owns list entry l
template <int DTYPE, int K>
__device__ __forceinline__ void drain(const GuidedArgs& a, const GuidedJob& P, const uint32_t* __restrict__ qd, const uint32_t* list, int m, int lane,
                                      uint64_t& best, uint64_t& second) {
    if (lane >= m) return;
    const int k = K ? K : a.kdyn;
    const uint32_t t = list[lane];
    const uint32_t* row;
    if (a.direction == LCD_GUIDED_PROJECTED_TO_FRAME) row = (const uint32_t*)a.to + (size_t)(P.to_row + t) * k;
    else row = (const uint32_t*)a.from + (size_t)(P.from_row + a.corner_from_row[P.corner_row + t]) * k;   // (a listed corner's from-row is in range)
    float d;
    if constexpr (K != 0 && DTYPE == 0) {
        float v[K];
#pragma unroll
        for (int g = 0; g < K / 4; ++g) {
            const float4 x = reinterpret_cast<const float4*>(row)[g];
            v[4 * g + 0] = x.x; v[4 * g + 1] = x.y; v[4 * g + 2] = x.z; v[4 * g + 3] = x.w;
        }
        d = l2_ref<K>(reinterpret_cast<const float*>(qd), v);
    } else if constexpr (K != 0) {
        uint32_t v[K];
#pragma unroll
        for (int g = 0; g < K / 4; ++g) {
            const uint4 x = reinterpret_cast<const uint4*>(row)[g];
            v[4 * g + 0] = x.x; v[4 * g + 1] = x.y; v[4 * g + 2] = x.z; v[4 * g + 3] = x.w;
        }
        d = (float)hamming_ref<K>(qd, v);
    } else if constexpr (DTYPE == 0) {
        d = l2_ref_dyn(reinterpret_cast<const float*>(qd), reinterpret_cast<const float*>(row), k);
    } else {
        d = (float)hamming_dyn(qd, row, k);
    }
    top2_push(best, second, ((uint64_t)__float_as_uint(d) << 32) | t);
}

// what one lane wrote to the wave's list is read by another: LDS operations of a wave run in order, the compiler is told not to move them
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// DTYPE 0: squared L2 over K floats, 1: Hamming over K dwords; K == 0: any row length (kdyn), as pair_dist_kernel
template <int DTYPE, int K>
__global__ __launch_bounds__(GBLOCK) void guided_match_kernel(GuidedArgs a) {
    __shared__ float2 s_pts[MAX_SIDE];
    __shared__ uint32_t s_list[GWAVES][LIST];
    const int b = blockIdx.x;
    int lo = 0, hi = a.n_jobs - 1;                                    // the pair this workgroup belongs to: the last one that starts at or before it
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.jobs[mid].block_first <= b) lo = mid; else hi = mid - 1;
    }
    const GuidedJob P = a.jobs[lo];
    const bool p2f = a.direction == LCD_GUIDED_PROJECTED_TO_FRAME;
    const int k = K ? K : a.kdyn;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nq = p2f ? P.nc : P.nt, n_tgt = p2f ? P.nt : P.nc;
    const int q0 = (b - P.block_first) * QBLOCK, q1 = min(q0 + QBLOCK, nq);
    const float qnan = __int_as_float(0x7fc00000);

    // ---- the pair's target points; a corner whose from-row is out of range is in no window (a NaN point)
    for (int i = tid; i < n_tgt; i += GBLOCK) {
        float2 p;
        if (p2f) p = a.to_points[P.to_row + i];
        else {
            p = a.corners[P.corner_row + i];
            const int32_t r = a.corner_from_row[P.corner_row + i];
            if (r < 0 || r >= P.nf) p = make_float2(qnan, qnan);
        }
        s_pts[i] = p;
    }
    __syncthreads();

    uint32_t* list = s_list[wave];
    for (int q = q0 + wave; q < q1; q += GWAVES) {
        float2 qp;
        const uint32_t* qd;
        bool valid = true;
        if (p2f) {
            const int32_t r = a.corner_from_row[P.corner_row + q];
            valid = r >= 0 && r < P.nf;                               // (the host entry refuses it; here: an empty window, nothing dereferenced)
            qp = a.corners[P.corner_row + q];
            qd = (const uint32_t*)a.from + (size_t)(P.from_row + (valid ? r : 0)) * k;
        } else {
            qp = a.to_points[P.to_row + q];
            qd = (const uint32_t*)a.to + (size_t)(P.to_row + q) * k;
        }
        int count = 0, n_list = 0;
        uint64_t best = KEY_NONE, second = KEY_NONE;
        for (int base = 0; base < n_tgt && valid; base += 64) {
            const int t = base + lane;
            bool in = false;
            if (t < n_tgt) {
                const float2 p = s_pts[t];
                const float dx = __fsub_rn(qp.x, p.x), dy = __fsub_rn(qp.y, p.y);
                in = __fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)) < a.r2;         // strict, false for NaN
            }
            const unsigned long long mask = __ballot(in);
            if (mask == 0) continue;
            const int pos = n_list + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
            if (in) list[pos] = (uint32_t)t;
            const int n = __popcll(mask);
            n_list += n; count += n;
            if (n_list >= 64) {                                       // LDS stays bounded however wide the window is
                wave_lds_sync();
                drain<DTYPE, K>(a, P, qd, list, 64, lane, best, second);
                n_list -= 64;
                const uint32_t rest = lane < n_list ? list[64 + lane] : 0u;
                wave_lds_sync();
                if (lane < n_list) list[lane] = rest;
            }
        }
        wave_lds_sync();
        int match = -1;
        float d1 = -1.0f, d2 = -1.0f;
        if (count == 1) {
            match = (int)list[0];                                     // no descriptor comparison (:1150-1153, :1303-1306)
        } else if (count >= 2) {
            drain<DTYPE, K>(a, P, qd, list, n_list, lane, best, second);
            wave_top2_reduce(best, second);
            d1 = __uint_as_float((uint32_t)(best >> 32));
            d2 = __uint_as_float((uint32_t)(second >> 32));
            if (a.nn_type == LCD_GUIDED_NEAREST || d1 < __fmul_rn(a.nndr, d2)) match = (int)(uint32_t)best;
        }
        wave_lds_sync();                                              // list[0] is read before the next query appends
        if (lane == 0) {
            const int64_t o = (p2f ? P.corner_row : P.to_row) + q;
            a.out_count[o] = count;
            a.out_match[o] = match;
            if (a.out_dist) { a.out_dist[2 * o] = d1; a.out_dist[2 * o + 1] = d2; }
            if (p2f && match >= 0) atomicMin(&a.out_to_owner[P.to_row + match], (uint32_t)q);   // addedWordsTo: the first corner keeps the row
        }
    }
}

hipError_t launch_guided(int dtype, int kdim, const GuidedArgs& a, int64_t n_blocks, hipStream_t s) {
    if (n_blocks <= 0) return hipSuccess;
    if (n_blocks > 0x7fffffffll) return hipErrorInvalidValue;
    const dim3 grid((unsigned)n_blocks), block(GBLOCK);
    GuidedArgs g = a;
    if (dtype == LCD_F32) {
        g.kdyn = kdim;
        if (kdim == 64) guided_match_kernel<0, 64><<<grid, block, 0, s>>>(g);
        else if (kdim == 128) guided_match_kernel<0, 128><<<grid, block, 0, s>>>(g);
        else guided_match_kernel<0, 0><<<grid, block, 0, s>>>(g);
    } else {
        g.kdyn = kdim / 4;
        if (g.kdyn == 8) guided_match_kernel<1, 8><<<grid, block, 0, s>>>(g);
        else if (g.kdyn == 16) guided_match_kernel<1, 16><<<grid, block, 0, s>>>(g);
        else guided_match_kernel<1, 0><<<grid, block, 0, s>>>(g);
    }
    return hipGetLastError();
}

}  // namespace
}  // namespace lcd

using namespace lcd;

namespace {

int match_guided(lcd_engine* h, const lcd_guided_args* a, bool on_device) {
    const char* who = on_device ? "lcd_match_guided_dev" : "lcd_match_guided";
    auto bad = [&](int code, const char* what) { return h->fail(code, std::string(who) + ": " + what); };
    // ---- everything that can be refused is refused before anything is enqueued or written
    if (!a || a->struct_size != (int32_t)sizeof(lcd_guided_args)) return bad(LCD_ERR_INVALID, "null arguments or wrong struct_size");
    if (a->direction != LCD_GUIDED_PROJECTED_TO_FRAME && a->direction != LCD_GUIDED_FRAME_TO_PROJECTED) return bad(LCD_ERR_INVALID, "unknown direction");
    if (a->nn_type != LCD_GUIDED_RATIO && a->nn_type != LCD_GUIDED_NEAREST) return bad(LCD_ERR_INVALID, "unknown nn_type");
    if (!std::isfinite(a->radius) || !(a->radius > 0.0f)) return bad(LCD_ERR_INVALID, "radius must be finite and > 0");
    if (a->n_pairs < 0) return bad(LCD_ERR_INVALID, "negative n_pairs");
    if (a->n_pairs > 65535) return bad(LCD_ERR_UNSUPPORTED, "more than 65535 pairs per call");
    if (h->shard_append || h->shard_first || h->shard_block) return bad(LCD_ERR_UNSUPPORTED, "not offered on the handles of a sharded vocabulary");
    if (on_device && rows_padded(h)) return bad(LCD_ERR_UNSUPPORTED, "the handle's rows are padded: a [n x dim] device buffer is not what the kernel walks");
    if (a->n_pairs == 0) return LCD_OK;
    const int np = a->n_pairs;
    const bool p2f = a->direction == LCD_GUIDED_PROJECTED_TO_FRAME;
    const int64_t* fo = a->from_offsets; const int64_t* to = a->to_offsets; const int64_t* co = a->corner_offsets;
    if (!fo || !to || !co || fo[0] != 0 || to[0] != 0 || co[0] != 0) return bad(LCD_ERR_INVALID, "offsets missing or not starting at 0");
    for (int p = 0; p < np; ++p)
        if (fo[p + 1] < fo[p] || to[p + 1] < to[p] || co[p + 1] < co[p]) return bad(LCD_ERR_INVALID, "decreasing offsets");
    for (int p = 0; p < np; ++p)
        if (fo[p + 1] - fo[p] > MAX_SIDE || to[p + 1] - to[p] > MAX_SIDE || co[p + 1] - co[p] > MAX_SIDE)
            return bad(LCD_ERR_UNSUPPORTED, "more than 8192 rows or corners on one side of a pair");
    const int64_t nfrom = fo[np], nto = to[np], ncor = co[np];
    const int64_t nquery = p2f ? ncor : nto;
    if ((nfrom > 0 && !a->from) || (nto > 0 && (!a->to || !a->to_points)) || (ncor > 0 && (!a->corners || !a->corner_from_row)))
        return bad(LCD_ERR_INVALID, "null rows, points or corners");
    // (an output of zero entries is not needed)
    if ((nquery > 0 && (!a->out_count || !a->out_match)) || (p2f && nto > 0 && !a->out_to_owner)) return bad(LCD_ERR_INVALID, "null output");
    if (!on_device)
        for (int p = 0; p < np; ++p) {
            const int64_t nf = fo[p + 1] - fo[p];
            for (int64_t c = co[p]; c < co[p + 1]; ++c)
                if (a->corner_from_row[c] < 0 || a->corner_from_row[c] >= nf) return bad(LCD_ERR_INVALID, "corner_from_row outside the pair's from-rows");
        }
    if (nquery == 0 && !(p2f && nto > 0)) return LCD_OK;
    StatelessScratch& S = h->pairs;
    hipStream_t st = h->stream;

    GuidedArgs g;
    g.n_jobs = np; g.direction = a->direction; g.nn_type = a->nn_type; g.kdyn = 0;
    g.r2 = a->radius * a->radius; g.nndr = a->nndr_ratio;
    g.from = a->from; g.to = a->to;
    g.corners = (const float2*)a->corners; g.corner_from_row = a->corner_from_row; g.to_points = (const float2*)a->to_points;
    g.out_count = a->out_count; g.out_match = a->out_match; g.out_dist = a->out_dist; g.out_to_owner = (uint32_t*)a->out_to_owner;

    // ---- host entry: rows, points and corners to the device, results back at the end (one synchronisation)
    HostStage stage(S, host_row_bytes(h), (size_t)h->row_bytes, on_device);
    stage.in_rows(g.from, nfrom); stage.in_rows(g.to, nto);
    stage.in(g.corners, (size_t)ncor * 8); stage.in(g.corner_from_row, (size_t)ncor * 4);
    stage.in(g.to_points, (size_t)nto * 8);
    stage.out(g.out_count, (size_t)nquery * 4); stage.out(g.out_match, (size_t)nquery * 4);
    stage.out(g.out_dist, (size_t)nquery * 8);                         // optional: null stays null
    stage.out(g.out_to_owner, p2f ? (size_t)nto * 4 : 0);              // the first-come rule's alone: no other direction touches it
    LCD_HIP(h, stage.commit(st, &h->bytes_device));

    // ---- the job table: one entry per pair
    std::vector<GuidedJob> jobs((size_t)np);
    int64_t blocks = 0;
    for (int p = 0; p < np; ++p) {
        GuidedJob& J = jobs[(size_t)p];
        J.from_row = fo[p]; J.to_row = to[p]; J.corner_row = co[p];
        J.nf = (int32_t)(fo[p + 1] - fo[p]); J.nt = (int32_t)(to[p + 1] - to[p]); J.nc = (int32_t)(co[p + 1] - co[p]);
        J.block_first = (int32_t)blocks;
        blocks += ((p2f ? J.nc : J.nt) + QBLOCK - 1) / QBLOCK;       // at most 65535 x 512
    }
    LCD_HIP(h, S.upload_table(&g.jobs, st, &h->bytes_device, jobs.data(), jobs.size() * sizeof(GuidedJob)));

    if (p2f && nto > 0) LCD_HIP(h, hipMemsetAsync(g.out_to_owner, 0xFF, (size_t)nto * 4, st));      // -1: nobody's
    LCD_HIP(h, launch_guided(h->dtype, h->kdim, g, blocks, st));
    LCD_HIP(h, stage.finish(st));
    return LCD_OK;
}

}  // namespace

extern "C" {

int lcd_match_guided(lcd_engine* h, const lcd_guided_args* a) { return stateless_entry(h, "lcd_match_guided", match_guided, a, false); }
int lcd_match_guided_dev(lcd_engine* h, const lcd_guided_args* a) { return stateless_entry(h, "lcd_match_guided", match_guided, a, true); }

}  // extern "C"
