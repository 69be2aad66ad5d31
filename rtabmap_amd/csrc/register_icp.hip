// register_icp.hip -- lcd_register_icp and its _dev form: the point-to-point branch of RegistrationIcp::computeTransformationImpl (reference
// RegistrationIcp.cpp:662-971 with Icp/Strategy = 0, util3d::icp at util3d_registration.cpp:384-434, computeVarianceAndCorrespondences at
// :327-360) for a caller who holds both scans in device memory.  The rule is include/lcd.h's; its arithmetic and its control flow are
// icp_rule.h's, compiled here for the device and in host/RegistrationIcp.cpp for the mirror.
//   register_icp_kernel: one launch per call, one workgroup of 256 threads per pair, in phases behind barriers.
//     (a) which rows take part (one bit a row, in LDS); Q = guess(to-rows) to the call's scratch; the source's current cloud = the from-rows.
//     (b) the target of a search is staged in LDS once and stays there while it does not move: three planes of floats, a row that takes no
//         part and the padding as +inf (no distance to them is ever the smallest).  A search is brute force: thread t owns the queries t,
//         t + 256, ..; it walks the whole target in ascending row order, four rows per 16-byte LDS read that every lane makes at the same
//         address (a broadcast, no bank conflict), and keeps the first smallest d2 -- icp::nearer in ascending order.  In the grid form
//         (icp::wants_grid: asked for, or AUTO from icp::AUTO_GRID_ROWS rows on) the planes' place holds the target's 64-bit keys (cell x, y,
//         z above the row), sorted once by compact_body.cuh's network; a query binary-searches the nine runs of three z-neighbours around
//         its cell and reads the candidates' coordinates from the scratch.  A target with a row beyond the key's cell range is staged in
//         the brute form instead, and a query beyond it walks the target in the scratch: the outputs are the same bit for bit.
//     (c) the loop: the thread that searched a row adds it to the lane partials of the rule's SUM (lane = row mod 256 = the thread), the
//         halving tree is Group::tree, thread 0 makes the fit, every thread moves its own rows.
//     (d) step 8: the registered cloud against Q (still staged), then Q against the registered cloud (staged over Q), the reciprocal test per
//         row, the median by the radix select (Group::ranked) over the d2 bit patterns, a row that is no correspondence as all ones.
//     (e) outputs.
// Nothing of the engine is read or written: the job table is StatelessScratch's, the per-row scratch its d_small.
#include "icp_rule.h"
#include "motion_group.cuh"

#include <cmath>
#include <vector>

static_assert(sizeof(lcd_icp_args) == 160, "lcd_icp_args: the layout include/lcd.h documents (LP64)");
static_assert(LCD_ICP_OK == lcd::icp::ST_OK && LCD_ICP_EMPTY == lcd::icp::ST_EMPTY && LCD_ICP_NOT_CONVERGED == lcd::icp::ST_NOT_CONVERGED &&
              LCD_ICP_BELOW_RATIO == lcd::icp::ST_BELOW_RATIO, "lcd_icp_status");
static_assert(LCD_ICP_STOP_NONE == lcd::icp::STOP_NONE && LCD_ICP_STOP_ITERATIONS == lcd::icp::STOP_ITERATIONS && LCD_ICP_STOP_TRANSFORM == lcd::icp::STOP_TRANSFORM &&
              LCD_ICP_STOP_MSE == lcd::icp::STOP_MSE && LCD_ICP_STOP_FEW_CORRESPONDENCES == lcd::icp::STOP_FEW_CORRESPONDENCES, "lcd_icp_stop");
static_assert(LCD_ICP_SEARCH_AUTO == lcd::icp::SEARCH_AUTO && LCD_ICP_SEARCH_BRUTE == lcd::icp::SEARCH_BRUTE && LCD_ICP_SEARCH_GRID == lcd::icp::SEARCH_GRID, "lcd_icp_search");

namespace lcd {
namespace {

constexpr int SUMS = 9;                                                  // rows of lane partials: a fit's nine products
constexpr int SCRATCH_WORDS = 5;                                         // per row of either side: three coordinates, the nearest row, its d2
constexpr int MASK_WORDS = MAX_ROWS / 32;
static_assert(MASK_WORDS == BLOCK, "a thread clears one word of each participation mask");
// the carve, every part a multiple of 16 bytes (the target's planes are read 16 bytes at a time): red, hist, the two masks, cur, planes
constexpr size_t OFF_HIST = (size_t)SUMS * BLOCK * 4, OFF_MASK_F = OFF_HIST + 256 * 4, OFF_MASK_T = OFF_MASK_F + MASK_WORDS * 4;
constexpr size_t OFF_CUR = OFF_MASK_T + MASK_WORDS * 4, OFF_PLANES = OFF_CUR + 16 * 4;
static_assert(OFF_PLANES % 16 == 0, "the planes start on a 16-byte boundary");
inline int plane_stride(int n_max) { return std::max((n_max + 3) & ~3, 4); }
inline int key_slots(int n_max) { int p2 = 2; while (p2 < n_max) p2 <<= 1; return padded(p2); }      // the grid form's sorted keys take the planes' place
inline size_t lds_bytes(int n_max) { return OFF_PLANES + std::max((size_t)3 * plane_stride(n_max) * 4, (size_t)key_slots(n_max) * 8); }
static_assert(OFF_PLANES + (size_t)3 * MAX_ROWS * 4 <= LDS_LIMIT && (size_t)(MAX_ROWS + MAX_ROWS / 8) * 8 <= (size_t)3 * MAX_ROWS * 4, "8192 rows of a target fit the carve, as planes and as keys");

struct IcpJob {
    int64_t first_from, first_to;            // the pair's first row in the from- / to-arrays
    int32_t n_from, n_to;
    float guess[12];
};
static_assert(sizeof(IcpJob) == 72, "the job table");

struct IcpArgs {
    const IcpJob* jobs;
    int max_iterations, force_3dof, max_laser_scans, search;
    float epsilon, correspondence_ratio, cell;            // cell: icp::cell_size of the call
    double thr2;
    int stride;                              // floats between the target's planes in LDS (a multiple of 4 >= every side)
    int64_t n_from_all;                      // Nf: the to-side's scratch starts behind the from-side's
    const float* from_xyz; const float* to_xyz;
    uint32_t* scratch;                       // [SCRATCH_WORDS x (Nf + Nt)] words
    float* out_transform; float* out_icp_transform; float* out_correction;
    int32_t* out_status; int32_t* out_stop; int32_t* out_iterations; int32_t* out_n_correspondences;
    float* out_ratio; double* out_variance; int32_t* out_match;
};

extern __shared__ __attribute__((aligned(16))) unsigned char icp_smem[];

__device__ __forceinline__ bool bit_of(const uint32_t* mask, int i) { return (mask[i >> 5] >> (i & 31)) & 1u; }

// one side of the pair in the scratch: planes [3][n], the nearest row in the other side, its d2
struct Side {
    int n;
    float* xyz; int32_t* nn; float* d2;
    const uint32_t* mask;                    // LDS: the rows that take part
    __device__ __forceinline__ void carve(uint32_t* base, int n_, const uint32_t* mask_) {
        n = n_; mask = mask_;
        xyz = reinterpret_cast<float*>(base); nn = reinterpret_cast<int32_t*>(base) + (size_t)3 * n; d2 = xyz + (size_t)4 * n;
    }
};

// the backend of icp::solve as a workgroup: every method is called by all 256 threads and returns the same value to each.  Of Group only the
// reductions are used -- tree() and ranked() -- and only what they touch is set: tid, red, hist, cur.  The RANSAC's members (models, valid,
// wsum, best, X, m, the two index sets) stay unset and nothing here may call the methods that read them.
struct GroupBackend : Group {
    Side from, to;
    int np_from, np_to;                      // participating rows
    const float* raw_from;                   // the pair's from-rows as given: P_0
    float* planes; int stride;               // LDS: the staged target, brute form
    uint64_t* keys64; int n_sorted;          // LDS, in the planes' place: the staged target's cell keys ascending, grid form
    bool staged_from, grid;                  // which side is staged, and in which form
    const float* txyz; const uint32_t* tmask; int tn;   // the staged side's planes in the scratch, its mask, its rows
    int search_mode; float cell;
    double thr2;
    float csum[6];                           // the six coordinate sums of the last correspond()
    int32_t* out_match;
    const uint32_t* keys; int n_keys;        // reciprocal()'s d2 bit patterns

    __device__ __forceinline__ int n_from() const { return np_from; }
    __device__ __forceinline__ int n_to() const { return np_to; }

    // the staged target becomes side s; ends behind a barrier, and begins with one: nobody reads the planes any more
    __device__ __forceinline__ void stage(bool is_from) {
        __syncthreads();
        const Side s = is_from ? from : to;
        staged_from = is_from; txyz = s.xyz; tmask = s.mask; tn = s.n;
        const int rows = is_from ? np_from : np_to;
        grid = icp::wants_grid(search_mode, rows);
        if (grid) {                                                    // keys of the participating rows, all ones for the rest, sorted
            int p2 = 2;
            while (p2 < s.n) p2 <<= 1;
            int outside = 0;
            for (int j = tid; j < p2; j += BLOCK) {
                uint64_t k = ~0ull;
                if (j < s.n && bit_of(s.mask, j) && !icp::key_of(s.xyz[j], s.xyz[(size_t)s.n + j], s.xyz[(size_t)2 * s.n + j], cell, (uint64_t)j, k)) outside = 1;
                keys64[padded(j)] = k;
            }
            if (!__syncthreads_or(outside)) {
                bitonic_sort(keys64, p2);
                n_sorted = rows;
                return;
            }
            grid = false;                                              // a row beyond the key's cell range: this target is searched in the brute form
        }
        const float inf = m3d::float_of(0x7f800000u);
        const int n4 = (s.n + 3) & ~3;
        for (int j = tid; j < n4; j += BLOCK) {
            const bool in = j < s.n && bit_of(s.mask, j);
            planes[j] = in ? s.xyz[j] : inf;
            planes[stride + j] = in ? s.xyz[(size_t)s.n + j] : inf;
            planes[2 * stride + j] = in ? s.xyz[(size_t)2 * s.n + j] : inf;
        }
        __syncthreads();
    }
    // coordinate a of the staged target's row
    __device__ __forceinline__ float target(int a, int row) const { return grid ? txyz[(size_t)a * tn + row] : planes[a * stride + row]; }
    // The nearest staged row (n_target of them) of every row of q, to q.nn / q.d2; a row that takes no part gets (-1, +inf).
    // In the grid form "nearest" is among the 27 cells around the row, which is the same row wherever it is a correspondence (icp_rule.h).
    // each(i, live, row, d2, px, py, pz) is called for every trip of every thread, also for i >= q.n (live = false).
    template <class Each>
    __device__ __forceinline__ void search(const Side& q, int n_target, Each each) {
        const float inf = m3d::float_of(0x7f800000u);
        const int n4 = (n_target + 3) & ~3;
        const float4* X = reinterpret_cast<const float4*>(planes);
        const float4* Y = reinterpret_cast<const float4*>(planes + stride);
        const float4* Z = reinterpret_cast<const float4*>(planes + 2 * stride);
        for (int base = 0; base < q.n; base += BLOCK) {
            const int i = base + tid;
            const bool live = i < q.n && bit_of(q.mask, i);
            float px = 0.0f, py = 0.0f, pz = 0.0f, best = inf;
            int row = -1;
            if (live) {
                px = q.xyz[i]; py = q.xyz[(size_t)q.n + i]; pz = q.xyz[(size_t)2 * q.n + i];
            }
            if (live && grid) {
                const float* tx = txyz;
                const bool found = icp::grid_nearest([&](int a) __attribute__((always_inline)) { return keys64[padded(a)]; }, n_sorted,
                                                     [&](int r, float& x, float& y, float& z) __attribute__((always_inline)) {
                                                         x = tx[r]; y = tx[(size_t)tn + r]; z = tx[(size_t)2 * tn + r];
                                                     }, px, py, pz, cell, best, row);
                if (!found) {                                          // the row's own cell is beyond the range: it walks the whole target
                    for (int j = 0; j < tn; ++j) {
                        if (!bit_of(tmask, j)) continue;
                        const float d = icp::dist2(px, py, pz, tx[j], tx[(size_t)tn + j], tx[(size_t)2 * tn + j]);
                        if (d < best) { best = d; row = j; }
                    }
                }
            } else if (live) {
                for (int j = 0; j < n4; j += 4) {
                    const float4 x = X[j >> 2], y = Y[j >> 2], z = Z[j >> 2];
                    const float d0 = icp::dist2(px, py, pz, x.x, y.x, z.x), d1 = icp::dist2(px, py, pz, x.y, y.y, z.y);
                    const float d2 = icp::dist2(px, py, pz, x.z, y.z, z.z), d3 = icp::dist2(px, py, pz, x.w, y.w, z.w);
                    if (d0 < best) { best = d0; row = j; }
                    if (d1 < best) { best = d1; row = j + 1; }
                    if (d2 < best) { best = d2; row = j + 2; }
                    if (d3 < best) { best = d3; row = j + 3; }
                }
            }
            if (i < q.n) { q.nn[i] = row; q.d2[i] = best; }
            each(i, live, row, best, px, py, pz);
        }
    }
    __device__ __forceinline__ int correspond(float& sum_d2) {
        float part[7];
#pragma unroll
        for (int c = 0; c < 7; ++c) part[c] = 0.0f;
        int count = 0;
        search(from, to.n, [&](int, bool live, int row, float d2, float px, float py, float pz) __attribute__((always_inline)) {
            const bool has = live && icp::corresponds(row, d2, thr2);
            if (has) {
                part[0] = part[0] + px; part[1] = part[1] + py; part[2] = part[2] + pz;
                part[3] = part[3] + target(0, row); part[4] = part[4] + target(1, row); part[5] = part[5] + target(2, row);
                part[6] = part[6] + d2;
            }
            count += __syncthreads_count(has);
        });
        tree<7>(part);
#pragma unroll
        for (int c = 0; c < 6; ++c) csum[c] = red[c * BLOCK];
        sum_d2 = red[6 * BLOCK];
        __syncthreads();
        return count;
    }
    __device__ __forceinline__ void fit(int c, bool flat, float T[12]) {
        float cen[6], part[9];
#pragma unroll
        for (int k = 0; k < 6; ++k) cen[k] = csum[k] / (float)c;
#pragma unroll
        for (int k = 0; k < 9; ++k) part[k] = 0.0f;
        for (int i = tid; i < from.n; i += BLOCK) {
            const int row = from.nn[i];
            if (!bit_of(from.mask, i) || !icp::corresponds(row, from.d2[i], thr2)) continue;
            float dp[3], dq[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) { dp[a] = from.xyz[(size_t)a * from.n + i] - cen[a]; dq[a] = target(a, row) - cen[3 + a]; }
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int b = 0; b < 3; ++b) {
                    const float e = dp[a] * dq[b];
                    part[3 * a + b] = part[3 * a + b] + e;
                }
        }
        tree<9>(part);
        if (tid == 0) {
            float S[9], model[12];
#pragma unroll
            for (int k = 0; k < 9; ++k) S[k] = red[k * BLOCK];
            icp::fit(cen, cen + 3, S, flat, model);
#pragma unroll
            for (int k = 0; k < 12; ++k) cur[k] = model[k];
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 12; ++k) T[k] = cur[k];
    }
    // a thread moves the rows it owns (t, t + 256, ..): the rows it searches for, so no barrier stands between the two
    __device__ __forceinline__ void advance(const float T[12]) {
        for (int i = tid; i < from.n; i += BLOCK) {
            if (!bit_of(from.mask, i)) continue;
            float x, y, z;
            icp::apply(T, from.xyz[i], from.xyz[(size_t)from.n + i], from.xyz[(size_t)2 * from.n + i], x, y, z);
            from.xyz[i] = x; from.xyz[(size_t)from.n + i] = y; from.xyz[(size_t)2 * from.n + i] = z;
        }
    }
    __device__ __forceinline__ void set_registered(const float F[12]) {
        for (int i = tid; i < from.n; i += BLOCK) {
            if (!bit_of(from.mask, i)) continue;
            float x, y, z;
            icp::apply(F, raw_from[(size_t)3 * i], raw_from[(size_t)3 * i + 1], raw_from[(size_t)3 * i + 2], x, y, z);
            from.xyz[i] = x; from.xyz[(size_t)from.n + i] = y; from.xyz[(size_t)2 * from.n + i] = z;
        }
    }
    __device__ __forceinline__ int reciprocal(bool from_is_target) {
        auto nothing = [](int, bool, int, float, float, float, float) __attribute__((always_inline)) {};
        search(from, to.n, nothing);                                   // Q is still staged
        stage(true);                                                   // (its first barrier also publishes the registered cloud)
        search(to, from.n, nothing);
        __syncthreads();                                               // both sides' nearest rows are read by other threads
        const Side& src = from_is_target ? to : from;
        const Side& tgt = from_is_target ? from : to;
        int count = 0;                                                 // (out_match is all -1 so far)
        for (int base = 0; base < src.n; base += BLOCK) {
            const int i = base + tid;
            bool keep = false;
            int row = -1;
            if (i < src.n) {
                row = src.nn[i];
                keep = icp::corresponds(row, src.d2[i], thr2) && tgt.nn[row] == i;
                if (!keep) reinterpret_cast<uint32_t*>(src.d2)[i] = 0xffffffffu;
                if (from_is_target) { if (keep) out_match[row] = i; }
                else out_match[i] = keep ? row : -1;
            }
            count += __syncthreads_count(keep);
        }
        keys = reinterpret_cast<const uint32_t*>(src.d2); n_keys = src.n;
        return count;
    }
    // non-negative floats order as their bit patterns; what is no correspondence sorts behind every one
    __device__ __forceinline__ float median(int n) { return m3d::float_of(ranked(keys, n_keys, n >> 1)); }
};

__global__ __launch_bounds__(BLOCK) void register_icp_kernel(IcpArgs a) {
    const int tid = threadIdx.x;
    const IcpJob J = a.jobs[blockIdx.x];
    const int nf = J.n_from, nt = J.n_to;
    uint32_t* mask_f = reinterpret_cast<uint32_t*>(icp_smem + OFF_MASK_F);
    uint32_t* mask_t = reinterpret_cast<uint32_t*>(icp_smem + OFF_MASK_T);
    const float* raw_from = a.from_xyz + J.first_from * 3;
    const float* raw_to = a.to_xyz + J.first_to * 3;

    GroupBackend b;
    b.tid = tid;
    b.red = reinterpret_cast<float*>(icp_smem);
    b.hist = reinterpret_cast<int*>(icp_smem + OFF_HIST);
    b.cur = reinterpret_cast<float*>(icp_smem + OFF_CUR);
    b.planes = reinterpret_cast<float*>(icp_smem + OFF_PLANES); b.stride = a.stride;
    b.keys64 = reinterpret_cast<uint64_t*>(icp_smem + OFF_PLANES); b.search_mode = a.search; b.cell = a.cell;
    b.thr2 = a.thr2; b.raw_from = raw_from; b.out_match = a.out_match + J.first_from;
    b.from.carve(a.scratch + (size_t)SCRATCH_WORDS * J.first_from, nf, mask_f);
    b.to.carve(a.scratch + (size_t)SCRATCH_WORDS * (a.n_from_all + J.first_to), nt, mask_t);

    // ---- (a) the rows that take part, Q and P_0
    mask_f[tid] = 0u; mask_t[tid] = 0u;
    __syncthreads();
    for (int i = tid; i < nf; i += BLOCK) {
        const float x = raw_from[(size_t)3 * i], y = raw_from[(size_t)3 * i + 1], z = raw_from[(size_t)3 * i + 2];
        b.from.xyz[i] = x; b.from.xyz[(size_t)nf + i] = y; b.from.xyz[(size_t)2 * nf + i] = z;
        if (icp::takes_part(x, y, z)) atomicOr(&mask_f[i >> 5], 1u << (i & 31));
        b.out_match[i] = -1;
    }
    for (int j = tid; j < nt; j += BLOCK) {
        const float x = raw_to[(size_t)3 * j], y = raw_to[(size_t)3 * j + 1], z = raw_to[(size_t)3 * j + 2];
        float qx, qy, qz;
        icp::apply(J.guess, x, y, z, qx, qy, qz);
        b.to.xyz[j] = qx; b.to.xyz[(size_t)nt + j] = qy; b.to.xyz[(size_t)2 * nt + j] = qz;
        if (icp::takes_part(x, y, z)) atomicOr(&mask_t[j >> 5], 1u << (j & 31));
    }
    __syncthreads();
    b.np_from = b.np_to = 0;
    for (int w = 0; w < MASK_WORDS; ++w) { b.np_from += __popc(mask_f[w]); b.np_to += __popc(mask_t[w]); }

    // ---- (b) .. (d): the rule's own control flow, Q staged for the loop
    b.stage(false);
    icp::Result r;
    icp::solve(b, a.max_iterations, a.force_3dof != 0, a.max_laser_scans, a.epsilon, a.correspondence_ratio, J.guess, r);

    // ---- (e) outputs
    if (tid == 0) {
        const size_t p = blockIdx.x;
#pragma unroll
        for (int k = 0; k < 12; ++k) {
            a.out_transform[p * 12 + k] = r.transform[k];
            a.out_icp_transform[p * 12 + k] = r.icp[k];
            a.out_correction[p * 12 + k] = r.correction[k];
        }
        a.out_status[p] = r.status;
        a.out_stop[p] = r.stop;
        a.out_iterations[p] = r.iterations;
        a.out_n_correspondences[p] = r.n_correspondences;
        a.out_ratio[p] = r.ratio;
        a.out_variance[p] = r.variance;
    }
}

}  // namespace
}  // namespace lcd

using namespace lcd;

namespace {

int register_icp(lcd_engine* h, const lcd_icp_args* a, bool on_device) {
    const char* who = on_device ? "lcd_register_icp_dev" : "lcd_register_icp";
    auto bad = [&](int code, const char* what) { return h->fail(code, std::string(who) + ": " + what); };
    // ---- everything that can be refused is refused before anything is enqueued or written
    if (!a || a->struct_size != (int32_t)sizeof(lcd_icp_args)) return bad(LCD_ERR_INVALID, "null arguments or wrong struct_size");
    if (a->max_iterations < 1) return bad(LCD_ERR_INVALID, "max_iterations is >= 1");
    if (a->max_laser_scans < 0) return bad(LCD_ERR_INVALID, "max_laser_scans is >= 0");
    if (a->search != LCD_ICP_SEARCH_AUTO && a->search != LCD_ICP_SEARCH_BRUTE && a->search != LCD_ICP_SEARCH_GRID) return bad(LCD_ERR_INVALID, "search is an lcd_icp_search");
    const double thr2 = a->max_correspondence_distance * a->max_correspondence_distance;
    if (!std::isfinite(a->max_correspondence_distance) || !(a->max_correspondence_distance > 0.0) || !std::isfinite(thr2))
        return bad(LCD_ERR_INVALID, "max_correspondence_distance is finite and > 0, squared too");
    if (!std::isfinite(a->epsilon) || !(a->epsilon >= 0.0f)) return bad(LCD_ERR_INVALID, "epsilon is finite and >= 0");
    if (!(a->correspondence_ratio >= 0.0f) || !(a->correspondence_ratio <= 1.0f)) return bad(LCD_ERR_INVALID, "correspondence_ratio is in [0, 1]");
    if (const int rc = refuse_pairs(h, a->n_pairs, bad)) return rc;
    if (a->n_pairs == 0) return LCD_OK;
    const int np = a->n_pairs;
    const int64_t* fo = a->from_offsets;
    const int64_t* to = a->to_offsets;
    int n_max, m_max;
    if (const int rc = refuse_offsets(np, fo, to, bad, n_max, m_max)) return rc;
    const int64_t Nf = fo[np], Nt = to[np];
    if (!a->guesses) return bad(LCD_ERR_INVALID, "null guesses");
    for (int64_t k = 0; k < (int64_t)np * 12; ++k) if (!std::isfinite(a->guesses[k])) return bad(LCD_ERR_INVALID, "a guess that is not finite");
    if (!a->out_transform || !a->out_icp_transform || !a->out_correction || !a->out_status || !a->out_stop || !a->out_iterations ||
        !a->out_n_correspondences || !a->out_ratio || !a->out_variance) return bad(LCD_ERR_INVALID, "a null per-pair output");
    if (Nf > 0 && (!a->from_xyz || !a->out_match)) return bad(LCD_ERR_INVALID, "null from-rows or out_match");
    if (Nt > 0 && !a->to_xyz) return bad(LCD_ERR_INVALID, "null to-rows");
    if (!on_device) {
        for (int64_t k = 0; k < Nf * 3; ++k) if (!std::isfinite(a->from_xyz[k])) return bad(LCD_ERR_INVALID, "a from-row that is not finite");
        for (int64_t k = 0; k < Nt * 3; ++k) if (!std::isfinite(a->to_xyz[k])) return bad(LCD_ERR_INVALID, "a to-row that is not finite");
    }

    StatelessScratch& S = h->pairs;
    hipStream_t st = h->stream;
    std::vector<IcpJob> jobs((size_t)np);
    for (int i = 0; i < np; ++i) {
        IcpJob& j = jobs[(size_t)i];
        j.first_from = fo[i]; j.first_to = to[i]; j.n_from = (int32_t)(fo[i + 1] - fo[i]); j.n_to = (int32_t)(to[i + 1] - to[i]);
        for (int k = 0; k < 12; ++k) j.guess[k] = a->guesses[(size_t)12 * i + k];
    }

    IcpArgs g;
    g.max_iterations = a->max_iterations; g.force_3dof = a->force_3dof; g.max_laser_scans = a->max_laser_scans;
    g.search = a->search; g.cell = icp::cell_size(a->max_correspondence_distance);
    g.epsilon = a->epsilon; g.correspondence_ratio = a->correspondence_ratio; g.thr2 = thr2;
    g.stride = plane_stride(n_max); g.n_from_all = Nf;
    g.from_xyz = a->from_xyz; g.to_xyz = a->to_xyz;
    g.out_transform = a->out_transform; g.out_icp_transform = a->out_icp_transform; g.out_correction = a->out_correction;
    g.out_status = a->out_status; g.out_stop = a->out_stop; g.out_iterations = a->out_iterations; g.out_n_correspondences = a->out_n_correspondences;
    g.out_ratio = a->out_ratio; g.out_variance = a->out_variance; g.out_match = a->out_match;

    // ---- host entry: everything to the device, results back at the end (one synchronisation)
    HostStage stage(S, host_row_bytes(h), (size_t)h->row_bytes);
    if (!on_device) {
        const int i_f = stage.add_in(a->from_xyz, (size_t)Nf * 12), i_t = stage.add_in(a->to_xyz, (size_t)Nt * 12);
        const int o_t = stage.add_out(a->out_transform, (size_t)np * 48), o_i = stage.add_out(a->out_icp_transform, (size_t)np * 48);
        const int o_c = stage.add_out(a->out_correction, (size_t)np * 48), o_v = stage.add_out(a->out_variance, (size_t)np * 8);
        const int o_s = stage.add_out(a->out_status, (size_t)np * 4), o_p = stage.add_out(a->out_stop, (size_t)np * 4);
        const int o_n = stage.add_out(a->out_iterations, (size_t)np * 4), o_k = stage.add_out(a->out_n_correspondences, (size_t)np * 4);
        const int o_r = stage.add_out(a->out_ratio, (size_t)np * 4), o_m = stage.add_out(a->out_match, (size_t)Nf * 4);
        LCD_HIP(h, stage.commit(st, &h->bytes_device));
        g.from_xyz = stage.in<float>(i_f); g.to_xyz = stage.in<float>(i_t);
        g.out_transform = stage.out<float>(o_t); g.out_icp_transform = stage.out<float>(o_i); g.out_correction = stage.out<float>(o_c);
        g.out_variance = stage.out<double>(o_v); g.out_status = stage.out<int32_t>(o_s); g.out_stop = stage.out<int32_t>(o_p);
        g.out_iterations = stage.out<int32_t>(o_n); g.out_n_correspondences = stage.out<int32_t>(o_k); g.out_ratio = stage.out<float>(o_r);
        g.out_match = stage.out<int32_t>(o_m);
    }
    LCD_HIP(h, dreserve(h, S.d_small, (size_t)std::max<int64_t>(Nf + Nt, 1) * SCRATCH_WORDS * 4));
    g.scratch = S.d_small.as<uint32_t>();
    LCD_HIP(h, S.upload_table(&g.jobs, st, &h->bytes_device, jobs.data(), jobs.size() * sizeof(IcpJob)));
    allow_large_lds<&register_icp_kernel>();
    register_icp_kernel<<<dim3((unsigned)np), dim3(BLOCK), lds_bytes(n_max), st>>>(g);
    LCD_HIP(h, hipGetLastError());
    if (!on_device) LCD_HIP(h, stage.finish(st));
    return LCD_OK;
}

}  // namespace

extern "C" {

int lcd_register_icp(lcd_engine* h, const lcd_icp_args* a) { return stateless_entry(h, "lcd_register_icp", register_icp, a, false); }
int lcd_register_icp_dev(lcd_engine* h, const lcd_icp_args* a) { return stateless_entry(h, "lcd_register_icp", register_icp, a, true); }

}  // extern "C"
