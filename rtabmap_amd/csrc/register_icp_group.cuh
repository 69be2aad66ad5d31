// register_icp_group.cuh -- what the one-workgroup-per-pair registration kernels of register_icp.hip and register_icp_plane.hip share, each piece
// once: the job table's row, a side of the pair in the call's scratch, and the backend of icp::solve as a workgroup -- the staging of a search's
// target in LDS in both forms, the two searches, the sums of a point-to-point fit, the reciprocal test and the median.  A kernel sets the
// backend's pointers into its own carve.  Everything is inlined.  Behind the backend, the frame of the two host entries: the refusals both
// make, the job table's fill, the ten outputs both have and their staging.  Internal.
#pragma once
#include "icp_rule.h"
#include "motion_group.cuh"

#include <cmath>
#include <vector>

namespace lcd {

constexpr int SCRATCH_WORDS = 5;                                         // per row of either side: three coordinates, the nearest row, its d2
constexpr int MASK_WORDS = MAX_ROWS / 32;
static_assert(MASK_WORDS == BLOCK, "a thread clears one word of each participation mask");
inline int plane_stride(int n_max) { return std::max((n_max + 3) & ~3, 4); }
inline int key_slots(int n_max) { int p2 = 2; while (p2 < n_max) p2 <<= 1; return padded(p2); }      // the grid form's sorted keys take the planes' place

struct IcpJob {
    int64_t first_from, first_to;            // the pair's first row in the from- / to-arrays
    int32_t n_from, n_to;
    float guess[12];
};
static_assert(sizeof(IcpJob) == 72, "the job table");

// the ten outputs both calls have, as the kernel arguments of either embed them
struct IcpOutputs {
    float* out_transform; float* out_icp_transform; float* out_correction;
    int32_t* out_status; int32_t* out_stop; int32_t* out_iterations; int32_t* out_n_correspondences;
    float* out_ratio; double* out_variance; int32_t* out_match;
};
// thread 0's write of pair p's result (icp::Result or icpp::Result: the fields of the same names); out_match is the backend's
template <class R>
__device__ __forceinline__ void write_result(const IcpOutputs& o, size_t p, const R& r) {
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        o.out_transform[p * 12 + k] = r.transform[k];
        o.out_icp_transform[p * 12 + k] = r.icp[k];
        o.out_correction[p * 12 + k] = r.correction[k];
    }
    o.out_status[p] = r.status;
    o.out_stop[p] = r.stop;
    o.out_iterations[p] = r.iterations;
    o.out_n_correspondences[p] = r.n_correspondences;
    o.out_ratio[p] = r.ratio;
    o.out_variance[p] = r.variance;
}


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

    // The coordinate half of a kernel's first phase, one trip over either side: the from-rows as given to the scratch planes (P_0), Q =
    // guess(to-rows) likewise, one bit a row that takes part into the masks (cleared by the kernel, behind a barrier), out_match = -1.
    // from_row(i) / to_row(j) are called in the same trip by the thread that owns the row (the plane kernel's normals).  Ends behind a barrier.
    template <class FromRow, class ToRow>
    __device__ __forceinline__ void load_rows(const float* raw_to, const float guess[12], uint32_t* mask_f, uint32_t* mask_t, FromRow from_row, ToRow to_row) {
        const int nf = from.n, nt = to.n;
        for (int i = tid; i < nf; i += BLOCK) {
            const float x = raw_from[(size_t)3 * i], y = raw_from[(size_t)3 * i + 1], z = raw_from[(size_t)3 * i + 2];
            from.xyz[i] = x; from.xyz[(size_t)nf + i] = y; from.xyz[(size_t)2 * nf + i] = z;
            if (icp::takes_part(x, y, z)) atomicOr(&mask_f[i >> 5], 1u << (i & 31));
            from_row(i);
            out_match[i] = -1;
        }
        for (int j = tid; j < nt; j += BLOCK) {
            const float x = raw_to[(size_t)3 * j], y = raw_to[(size_t)3 * j + 1], z = raw_to[(size_t)3 * j + 2];
            float qx, qy, qz;
            icp::apply(guess, x, y, z, qx, qy, qz);
            to.xyz[j] = qx; to.xyz[(size_t)nt + j] = qy; to.xyz[(size_t)2 * nt + j] = qz;
            if (icp::takes_part(x, y, z)) atomicOr(&mask_t[j >> 5], 1u << (j & 31));
            to_row(j);
        }
        __syncthreads();
    }

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

// ---- the host frame of the two entries, over either argument struct of include/lcd.h (the fields of the same names)

// the parameters both calls have; *thr2: the squared distance.  An entry's own parameter refusals follow this.
template <class A, class Bad>
int refuse_icp_params(const A* a, Bad bad, double* thr2) {
    if (a->max_iterations < 1) return bad(LCD_ERR_INVALID, "max_iterations is >= 1");
    if (a->max_laser_scans < 0) return bad(LCD_ERR_INVALID, "max_laser_scans is >= 0");
    if (a->search != LCD_ICP_SEARCH_AUTO && a->search != LCD_ICP_SEARCH_BRUTE && a->search != LCD_ICP_SEARCH_GRID) return bad(LCD_ERR_INVALID, "search is an lcd_icp_search");
    *thr2 = a->max_correspondence_distance * a->max_correspondence_distance;
    if (!std::isfinite(a->max_correspondence_distance) || !(a->max_correspondence_distance > 0.0) || !std::isfinite(*thr2))
        return bad(LCD_ERR_INVALID, "max_correspondence_distance is finite and > 0, squared too");
    if (!std::isfinite(a->epsilon) || !(a->epsilon >= 0.0f)) return bad(LCD_ERR_INVALID, "epsilon is finite and >= 0");
    if (!(a->correspondence_ratio >= 0.0f) || !(a->correspondence_ratio <= 1.0f)) return bad(LCD_ERR_INVALID, "correspondence_ratio is in [0, 1]");
    return LCD_OK;
}

// what an entry adds to the null checks: whether one of its own arrays is null, and its texts for a side's arrays
struct IcpOwnArrays {
    bool null_output, null_from, null_to;
    const char* from_text; const char* to_text;
};
// the pairs of a call that nothing refused; np == 0: nothing to do
struct IcpPairs {
    int np = 0, n_max = 0;
    int64_t Nf = 0, Nt = 0;
    std::vector<IcpJob> jobs;
};
// pairs, offsets, guesses, null outputs, null rows and the host form's finite rows, then the job table
template <class A, class Bad>
int refuse_icp_pairs(const lcd_engine* h, const A* a, bool on_device, Bad bad, const IcpOwnArrays& own, IcpPairs& c) {
    if (const int rc = refuse_pairs(h, a->n_pairs, bad)) return rc;
    if (a->n_pairs == 0) return LCD_OK;
    const int np = a->n_pairs;
    const int64_t* fo = a->from_offsets;
    const int64_t* to = a->to_offsets;
    int m_max;
    if (const int rc = refuse_offsets(np, fo, to, bad, c.n_max, m_max)) return rc;
    c.Nf = fo[np]; c.Nt = to[np];
    if (!a->guesses) return bad(LCD_ERR_INVALID, "null guesses");
    for (int64_t k = 0; k < (int64_t)np * 12; ++k) if (!std::isfinite(a->guesses[k])) return bad(LCD_ERR_INVALID, "a guess that is not finite");
    if (!a->out_transform || !a->out_icp_transform || !a->out_correction || !a->out_status || !a->out_stop || !a->out_iterations ||
        !a->out_n_correspondences || !a->out_ratio || !a->out_variance || own.null_output) return bad(LCD_ERR_INVALID, "a null per-pair output");
    if (c.Nf > 0 && (!a->from_xyz || own.null_from || !a->out_match)) return bad(LCD_ERR_INVALID, own.from_text);
    if (c.Nt > 0 && (!a->to_xyz || own.null_to)) return bad(LCD_ERR_INVALID, own.to_text);
    if (!on_device) {                                                  // (a normal that is not finite is legal: the reference produces such normals)
        for (int64_t k = 0; k < c.Nf * 3; ++k) if (!std::isfinite(a->from_xyz[k])) return bad(LCD_ERR_INVALID, "a from-row that is not finite");
        for (int64_t k = 0; k < c.Nt * 3; ++k) if (!std::isfinite(a->to_xyz[k])) return bad(LCD_ERR_INVALID, "a to-row that is not finite");
    }
    c.jobs.resize((size_t)np);
    for (int i = 0; i < np; ++i) {
        IcpJob& j = c.jobs[(size_t)i];
        j.first_from = fo[i]; j.first_to = to[i]; j.n_from = (int32_t)(fo[i + 1] - fo[i]); j.n_to = (int32_t)(to[i + 1] - to[i]);
        for (int k = 0; k < 12; ++k) j.guess[k] = a->guesses[(size_t)12 * i + k];
    }
    c.np = np;
    return LCD_OK;
}

template <class A>
IcpOutputs icp_outputs(const A* a) {
    return IcpOutputs{a->out_transform, a->out_icp_transform, a->out_correction, a->out_status, a->out_stop, a->out_iterations,
                      a->out_n_correspondences, a->out_ratio, a->out_variance, a->out_match};
}
// the two coordinate inputs and the ten outputs of a call, bound for the host form
inline void stage_icp(HostStage& stage, const IcpPairs& c, const float*& from_xyz, const float*& to_xyz, IcpOutputs& o) {
    const size_t np = (size_t)c.np;
    stage.in(from_xyz, (size_t)c.Nf * 12); stage.in(to_xyz, (size_t)c.Nt * 12);
    stage.out(o.out_transform, np * 48); stage.out(o.out_icp_transform, np * 48); stage.out(o.out_correction, np * 48);
    stage.out(o.out_variance, np * 8); stage.out(o.out_status, np * 4); stage.out(o.out_stop, np * 4);
    stage.out(o.out_iterations, np * 4); stage.out(o.out_n_correspondences, np * 4); stage.out(o.out_ratio, np * 4);
    stage.out(o.out_match, (size_t)c.Nf * 4);
}

}  // namespace lcd
