// motion_3d.hip -- lcd_estimate_motion_3d and its _dev form: util3d::estimateMotion3DTo3D (reference util3d_motion_estimation.cpp:730-807,
// RegistrationVis.cpp:1823-1871 with Vis/EstimationType = 0) for a caller who holds both frames' word ids and 3-D points in device memory.
// The rule is include/lcd.h's; its arithmetic and its control flow (solve, refine) are motion_3d_rule.h's, compiled here for the device and
// in host/Motion3D.cpp for the mirror.
//   motion_3d_kernel: one launch per call, one workgroup of 256 threads per pair, in phases behind barriers.  The phases' machinery is
//   motion_group.cuh's, shared with motion_pnp.hip; what is written here is what the 3-D rule puts into it:
//     (a) join (join_compact): the from-frame's ids are walked, the predicate is m3d::keep_pair, the six coordinates (one plane each) go to
//         the call's scratch and, when they fit beside the hypotheses, into LDS (Group::init).
//     (b) hypotheses in chunks of 256 (Group::ransac): thread h draws and solves its three-point fit (the Jacobi sweeps fully unrolled); an
//         inlier is a correspondence whose squared distance is below the threshold's square.
//     (c) selection, refinement and median: the sums of a fit are the rule's (Group::tree), the median is the radix select (Group::ranked)
//         over the bit patterns of the last selection's d2, the loop's scalars are the same in every thread.
//     (d) outputs.
// Nothing of the engine is read or written: the job table is StatelessScratch's, the per-row scratch its d_small.
#include "motion_3d_rule.h"
#include "motion_group.cuh"

#include <cmath>
#include <vector>

static_assert(sizeof(lcd_motion_3d_args) == 136, "lcd_motion_3d_args: the layout include/lcd.h documents (LP64)");
static_assert(LCD_M3D_OK == lcd::m3d::ST_OK && LCD_M3D_FEW_CORRESPONDENCES == lcd::m3d::ST_FEW_CORRESPONDENCES && LCD_M3D_NO_MODEL == lcd::m3d::ST_NO_MODEL &&
              LCD_M3D_FEW_INLIERS == lcd::m3d::ST_FEW_INLIERS && LCD_M3D_BELOW_MIN_INLIERS == lcd::m3d::ST_BELOW_MIN_INLIERS, "lcd_motion_3d_status");
static_assert(LCD_M3D_SWEEPS == lcd::m3d::SWEEPS, "the sweep count include/lcd.h documents");

namespace lcd {
namespace {

constexpr int SUMS = 9;                                                  // rows of lane partials: a fit's nine products
constexpr size_t FIXED_BYTES = group_fixed_bytes(SUMS);
constexpr int SCRATCH_WORDS = 9;                                         // per from-row: six coordinates, d2, two index sets

struct M3dJob {
    int64_t first_from, first_to;            // the pair's first row in the from- / to-arrays
    int32_t n_from, n_to;
};
static_assert(sizeof(M3dJob) == 24, "the job table");

struct M3dArgs {
    const M3dJob* jobs;
    int min_inliers, iterations, refine_iterations;
    uint32_t seed;
    double inlier_distance;
    int p_max;                               // keys per side the LDS carve holds (a power of two >= every frame)
    int stage_cap;                           // correspondences whose coordinates fit the carve behind the fixed part
    const int32_t* from_ids; const float* from_xyz; const int32_t* to_ids; const float* to_xyz;
    uint32_t* scratch;                       // [SCRATCH_WORDS x Nf] words; a pair's part starts at SCRATCH_WORDS x first_from
    float* out_transform; int32_t* out_status; int32_t* out_n_matches; int32_t* out_n_inliers; double* out_variance;
    int32_t* out_matches; int32_t* out_inliers;
};

extern __shared__ __attribute__((aligned(16))) unsigned char m3_smem[];

// the backend of m3d::solve as a workgroup: every method is called by all 256 threads and returns the same value to each
struct GroupBackend : Group {
    uint32_t seed;
    int iterations;
    double thr2;
    float* d2;

    __device__ __forceinline__ bool hypothesis(uint32_t h, float model[12]) const {
        int i0, i1, i2;
        if (!m3d::draw3(seed, h, (uint32_t)m, i0, i1, i2)) return false;
        float P[3][3], Q[3][3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            P[0][a] = X[a * stride + i0]; Q[0][a] = X[(3 + a) * stride + i0];
            P[1][a] = X[a * stride + i1]; Q[1][a] = X[(3 + a) * stride + i1];
            P[2][a] = X[a * stride + i2]; Q[2][a] = X[(3 + a) * stride + i2];
        }
        m3d::fit3(P, Q, m3d::SWEEPS, model);
        return true;
    }
    __device__ __forceinline__ float distance(const float model[12], int i) const {
        return m3d::dist2(model, X[i], X[stride + i], X[2 * stride + i], X[3 * stride + i], X[4 * stride + i], X[5 * stride + i]);
    }
    __device__ __forceinline__ unsigned long long ransac() {
        return Group::ransac(iterations, [&](uint32_t h, float* model) __attribute__((always_inline)) { return hypothesis(h, model); },
                             [&](const float* w, int i) __attribute__((always_inline)) { return (double)distance(w, i) < thr2; });
    }
    __device__ __forceinline__ void fit_prev() {
        const int n = n_prev;
        if (n < 3) return;
        float part[9];
#pragma unroll
        for (int c = 0; c < 6; ++c) part[c] = 0.0f;
        for (int i = tid; i < n; i += BLOCK) {
            const int idx = prev[i];
#pragma unroll
            for (int c = 0; c < 6; ++c) part[c] = part[c] + X[c * stride + idx];
        }
        tree<6>(part);
        float cen[6];
#pragma unroll
        for (int c = 0; c < 6; ++c) cen[c] = red[c * BLOCK] / (float)n;
        __syncthreads();
#pragma unroll
        for (int c = 0; c < 9; ++c) part[c] = 0.0f;
        for (int i = tid; i < n; i += BLOCK) {
            const int idx = prev[i];
            float dp[3], dq[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) { dp[a] = X[a * stride + idx] - cen[a]; dq[a] = X[(3 + a) * stride + idx] - cen[3 + a]; }
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
            for (int c = 0; c < 9; ++c) S[c] = red[c * BLOCK];
            m3d::horn_fit(cen, cen + 3, S, m3d::SWEEPS, model);
#pragma unroll
            for (int k = 0; k < 12; ++k) cur[k] = model[k];
        }
        __syncthreads();
    }
    __device__ __forceinline__ int select(double t2) {
        float w[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) w[k] = cur[k];
        return Group::select(d2, [&](int i, float& d) __attribute__((always_inline)) { d = distance(w, i); return (double)d < t2; });
    }
    // the median of the last selection's d2: non-negative floats order as their bit patterns
    __device__ __forceinline__ double variance() {
        return m3d::VARIANCE_FACTOR * (double)m3d::float_of(ranked(reinterpret_cast<const uint32_t*>(d2), n_last, n_last >> 1));
    }
};

__global__ __launch_bounds__(BLOCK) void motion_3d_kernel(M3dArgs a) {
    __shared__ int wsum[WAVES];
    __shared__ int valid[BLOCK];
    __shared__ int hist[256];
    __shared__ unsigned long long best;
    __shared__ float cur[12];
    const M3dJob J = a.jobs[blockIdx.x];
    const int nf = J.n_from, nt = J.n_to;
    uint32_t* scratch = a.scratch + (size_t)SCRATCH_WORDS * J.first_from;
    float* gx = reinterpret_cast<float*>(scratch);                     // [6][nf]
    int32_t* out_matches = a.out_matches + J.first_from;

    // ---- (a) join: walk the from-frame's ids
    const int m = join_compact<6>(m3_smem, a.p_max, a.to_ids + J.first_to, nt, a.from_ids + J.first_from, nf, 6, out_matches, gx, wsum,
                                  [&](uint32_t row_f, uint32_t row_t, float* c) __attribute__((always_inline)) {
        const float* pf = a.from_xyz + (J.first_from + (int64_t)row_f) * 3;
        const float* pt = a.to_xyz + (J.first_to + (int64_t)row_t) * 3;
        c[0] = pf[0]; c[1] = pf[1]; c[2] = pf[2]; c[3] = pt[0]; c[4] = pt[1]; c[5] = pt[2];
        return m3d::keep_pair(c[0], c[1], c[2], c[3], c[4], c[5]);
    });

    GroupBackend b;
    b.seed = a.seed; b.iterations = a.iterations; b.thr2 = a.inlier_distance * a.inlier_distance;
    b.d2 = gx + (size_t)6 * nf;
    b.init(m, m3_smem, SUMS, wsum, valid, hist, &best, cur, reinterpret_cast<int32_t*>(scratch) + (size_t)7 * nf, gx, 6, nf, a.stage_cap);

    // ---- (b), (c): the rule's own control flow
    m3d::Result r;
    m3d::solve(b, m, a.min_inliers, a.refine_iterations, a.inlier_distance, r);

    // ---- (d) outputs
    b.write_inliers(a.out_inliers + J.first_from, out_matches, nf, r.n_inliers);
    if (threadIdx.x == 0) {
        float* t = a.out_transform + (size_t)blockIdx.x * 12;
#pragma unroll
        for (int k = 0; k < 12; ++k) t[k] = r.transform[k];
        a.out_status[blockIdx.x] = r.status;
        a.out_n_matches[blockIdx.x] = m;
        a.out_n_inliers[blockIdx.x] = r.n_inliers;
        a.out_variance[blockIdx.x] = r.variance;
    }
}

}  // namespace
}  // namespace lcd

using namespace lcd;

namespace {

int estimate_motion_3d(lcd_engine* h, const lcd_motion_3d_args* a, bool on_device) {
    const char* who = on_device ? "lcd_estimate_motion_3d_dev" : "lcd_estimate_motion_3d";
    auto bad = [&](int code, const char* what) { return h->fail(code, std::string(who) + ": " + what); };
    // ---- everything that can be refused is refused before anything is enqueued or written
    if (!a || a->struct_size != (int32_t)sizeof(lcd_motion_3d_args)) return bad(LCD_ERR_INVALID, "null arguments or wrong struct_size");
    if (a->iterations < 1) return bad(LCD_ERR_INVALID, "iterations is >= 1");
    if (a->iterations > 65535) return bad(LCD_ERR_UNSUPPORTED, "more than 65535 iterations");
    if (!std::isfinite(a->inlier_distance) || !(a->inlier_distance > 0.0)) return bad(LCD_ERR_INVALID, "inlier_distance is finite and > 0");
    if (a->refine_iterations < 0 || a->min_inliers < 1) return bad(LCD_ERR_INVALID, "refine_iterations is >= 0 and min_inliers >= 1");
    if (const int rc = refuse_pairs(h, a->n_pairs, bad)) return rc;
    if (a->n_pairs == 0) return LCD_OK;
    const int np = a->n_pairs;
    const int64_t* fo = a->from_offsets;
    const int64_t* to = a->to_offsets;
    int n_max, m_max;
    if (const int rc = refuse_offsets(np, fo, to, bad, n_max, m_max)) return rc;
    const int64_t Nf = fo[np], Nt = to[np];
    if (!a->out_transform || !a->out_status || !a->out_n_matches || !a->out_n_inliers || !a->out_variance) return bad(LCD_ERR_INVALID, "a null per-pair output");
    if (Nf > 0 && (!a->from_word_ids || !a->from_xyz || !a->out_matches || !a->out_inliers)) return bad(LCD_ERR_INVALID, "null from-arrays or id outputs");
    if (Nt > 0 && (!a->to_word_ids || !a->to_xyz)) return bad(LCD_ERR_INVALID, "null to-arrays");

    StatelessScratch& S = h->pairs;
    hipStream_t st = h->stream;
    std::vector<M3dJob> jobs((size_t)np);
    for (int i = 0; i < np; ++i) jobs[(size_t)i] = M3dJob{fo[i], to[i], (int32_t)(fo[i + 1] - fo[i]), (int32_t)(to[i + 1] - to[i])};

    M3dArgs g;
    g.min_inliers = a->min_inliers; g.iterations = a->iterations; g.refine_iterations = a->refine_iterations; g.seed = a->seed;
    g.inlier_distance = a->inlier_distance;
    const GroupPlan plan = group_plan(n_max, m_max, FIXED_BYTES, 24);
    g.p_max = plan.p_max; g.stage_cap = plan.stage_cap;
    g.from_ids = a->from_word_ids; g.from_xyz = a->from_xyz; g.to_ids = a->to_word_ids; g.to_xyz = a->to_xyz;
    g.out_transform = a->out_transform; g.out_status = a->out_status; g.out_n_matches = a->out_n_matches; g.out_n_inliers = a->out_n_inliers;
    g.out_variance = a->out_variance; g.out_matches = a->out_matches; g.out_inliers = a->out_inliers;

    // ---- host entry: everything to the device, results back at the end (one synchronisation)
    HostStage stage(S, host_row_bytes(h), (size_t)h->row_bytes, on_device);
    stage.in(g.from_ids, (size_t)Nf * 4); stage.in(g.from_xyz, (size_t)Nf * 12);
    stage.in(g.to_ids, (size_t)Nt * 4); stage.in(g.to_xyz, (size_t)Nt * 12);
    stage.out(g.out_transform, (size_t)np * 48); stage.out(g.out_status, (size_t)np * 4);
    stage.out(g.out_n_matches, (size_t)np * 4); stage.out(g.out_n_inliers, (size_t)np * 4);
    stage.out(g.out_variance, (size_t)np * 8);
    stage.out(g.out_matches, (size_t)Nf * 4); stage.out(g.out_inliers, (size_t)Nf * 4);
    LCD_HIP(h, stage.commit(st, &h->bytes_device));
    LCD_HIP(h, dreserve(h, S.d_small, (size_t)std::max<int64_t>(Nf, 1) * SCRATCH_WORDS * 4));
    g.scratch = S.d_small.as<uint32_t>();
    LCD_HIP(h, S.upload_table(&g.jobs, st, &h->bytes_device, jobs.data(), jobs.size() * sizeof(M3dJob)));
    allow_large_lds<&motion_3d_kernel>();
    motion_3d_kernel<<<dim3((unsigned)np), dim3(BLOCK), plan.lds, st>>>(g);
    LCD_HIP(h, hipGetLastError());
    LCD_HIP(h, stage.finish(st));
    return LCD_OK;
}

}  // namespace

extern "C" {

int lcd_estimate_motion_3d(lcd_engine* h, const lcd_motion_3d_args* a) { return stateless_entry(h, "lcd_estimate_motion_3d", estimate_motion_3d, a, false); }
int lcd_estimate_motion_3d_dev(lcd_engine* h, const lcd_motion_3d_args* a) { return stateless_entry(h, "lcd_estimate_motion_3d", estimate_motion_3d, a, true); }

}  // extern "C"
