// motion_pnp.hip -- lcd_estimate_motion_pnp and its _dev form: util3d::estimateMotion3DTo2D (reference util3d_motion_estimation.cpp:59-289,
// :843-986, RegistrationVis.cpp:1676-1819 with Vis/EstimationType = 1) for a caller who holds the from-frame's word ids and 3-D points and
// the to-frame's word ids and keypoints in device memory.  The rule is include/lcd.h's; its arithmetic and its control flow (solve, refine)
// are motion_pnp_rule.h's, compiled here for the device and in host/Motion2D.cpp for the mirror.
//   motion_pnp_kernel: one launch per call, one workgroup of 256 threads per pair, in phases behind barriers.  The phases' machinery is
//   motion_group.cuh's, shared with motion_3d.hip; what is written here is what the PnP rule puts into it:
//     (a) join (join_compact): the to-frame's ids are walked, the from-point's finiteness is tested, the coordinates (one plane each: from
//         x, y, z, to u, v and, with to_xyz, to x, y, z) go to the call's scratch and, when they fit beside the candidates, into LDS
//         (Group::init).
//     (b) candidates in chunks of 256 (Group::ransac): candidate 0 is the guess's model, h + 1 hypothesis h, P3P and the fourth point; an
//         inlier is pnp::is_inlier of the reprojection error.
//     (c) selection and refinement: a fit's 27 sums per Gauss-Newton step are 256 lane partials and the halving tree (Group::tree), the
//         6 x 6 system is thread 0's; mean and variance of a selection's errors are thread 0's walk in the reference's order.
//     (d) covariance inputs: per inlier the squared distance and the cosine as ordered keys, two radix selects (Group::ranked); or thread
//         0's RMS sum.
//     (e) outputs.
// Nothing of the engine is read or written: the job table is StatelessScratch's, the per-row scratch its d_small.
#include "motion_group.cuh"
#include "motion_pnp_rule.h"

#include <cmath>
#include <vector>

static_assert(sizeof(lcd_motion_pnp_args) == 184, "lcd_motion_pnp_args: the layout include/lcd.h documents (LP64)");
static_assert(LCD_PNP_OK == lcd::pnp::ST_OK && LCD_PNP_FEW_CORRESPONDENCES == lcd::pnp::ST_FEW_CORRESPONDENCES && LCD_PNP_NO_MODEL == lcd::pnp::ST_NO_MODEL &&
              LCD_PNP_BELOW_MIN_INLIERS == lcd::pnp::ST_BELOW_MIN_INLIERS && LCD_PNP_VARIANCE_REJECTED == lcd::pnp::ST_VARIANCE_REJECTED, "lcd_motion_pnp_status");
static_assert(LCD_PNP_STEPS == lcd::pnp::STEPS && LCD_PNP_BISECT == lcd::pnp::BISECT, "the counts include/lcd.h documents");

namespace lcd {
namespace {

constexpr size_t FIXED_BYTES = group_fixed_bytes(pnp::SUMS);
constexpr int MAX_PLANES = 8;
constexpr int SCRATCH_WORDS = MAX_PLANES + 3;                            // per to-row: the coordinate planes, the errors / distance keys, two index sets

struct PnpJob {
    int64_t first_from, first_to;            // the pair's first row in the from- / to-arrays
    int32_t n_from, n_to;
    float fx, fy, cx, cy;
    int32_t width, height;
    int32_t has_local, kind;                 // kind: the covariance branch (1 or 2)
    float model0[12], local[12];
};
static_assert(sizeof(PnpJob) == 152, "the job table");

struct PnpArgs {
    const PnpJob* jobs;
    int min_inliers, iterations, refine_iterations, ratio;
    uint32_t seed;
    float max_variance;
    double reproj_error;
    int p_max;                               // keys per side the LDS carve holds (a power of two >= every frame)
    int stage_cap;                           // correspondences whose coordinates fit the carve behind the fixed part
    int planes;                              // 8 with to_xyz, 5 without
    const int32_t* from_ids; const float* from_xyz; const int32_t* to_ids; const float* to_points; const float* to_xyz;
    uint32_t* scratch;                       // [SCRATCH_WORDS x Nt] words; a pair's part starts at SCRATCH_WORDS x first_to
    float* out_transform; int32_t* out_status; int32_t* out_n_matches; int32_t* out_n_inliers; double* out_variance_lin; double* out_angle_cos;
    int32_t* out_variance_kind; int32_t* out_matches; int32_t* out_inliers;
};

extern __shared__ __attribute__((aligned(16))) unsigned char pnp_smem[];

// the backend of pnp::solve as a workgroup: every method is called by all 256 threads and returns the same value to each
struct GroupBackend : Group {
    bool has_to;
    pnp::Camera cam;
    const float* model0;
    uint32_t seed;
    int iterations;
    double* bcast;
    float* err;

    __device__ __forceinline__ bool candidate(uint32_t c, float model[12]) const {
        if (c == 0) {
#pragma unroll
            for (int k = 0; k < 12; ++k) model[k] = model0[k];
            return true;
        }
        int i0, i1, i2, i3;
        if (!pnp::draw4(seed, c - 1u, (uint32_t)m, i0, i1, i2, i3)) return false;
        float P[3][3], B[3][3];
#pragma unroll
        for (int a = 0; a < 3; ++a) { P[0][a] = X[a * stride + i0]; P[1][a] = X[a * stride + i1]; P[2][a] = X[a * stride + i2]; }
        pnp::bearing(cam, X[3 * stride + i0], X[4 * stride + i0], B[0]);
        pnp::bearing(cam, X[3 * stride + i1], X[4 * stride + i1], B[1]);
        pnp::bearing(cam, X[3 * stride + i2], X[4 * stride + i2], B[2]);
        return pnp::p3p(P, B, X[i3], X[stride + i3], X[2 * stride + i3], X[3 * stride + i3], X[4 * stride + i3], cam, m3d::SWEEPS, model);
    }
    __device__ __forceinline__ float error(const float model[12], int i, bool& front) const {
        return pnp::reproj_error(model, cam, X[i], X[stride + i], X[2 * stride + i], X[3 * stride + i], X[4 * stride + i], front);
    }
    __device__ __forceinline__ bool inlier(const float model[12], int i, float thr, float& e) const {
        bool front;
        e = error(model, i, front);
        return pnp::is_inlier(e, front, thr);
    }
    __device__ __forceinline__ unsigned long long ransac(float thr) {
        return Group::ransac(iterations + 1, [&](uint32_t c, float* model) __attribute__((always_inline)) { return candidate(c, model); },
                             [&](const float* w, int i) __attribute__((always_inline)) { float e; return inlier(w, i, thr, e); });
    }
    __device__ __forceinline__ void fit_prev() {
        const int n = n_prev;
        if (n < 4) return;
        float q[4], t[3] = {cur[3], cur[7], cur[11]};                  // thread 0's are the pose
        {
            float w[12];
#pragma unroll
            for (int k = 0; k < 12; ++k) w[k] = cur[k];
            pnp::quat_of_model(w, q);
        }
        __syncthreads();                                               // cur is read
#pragma unroll 1
        for (int s = 0; s <= pnp::STEPS; ++s) {
            if (tid == 0) {
                if (s > 0) {
                    float S[pnp::SUMS], delta[6];
#pragma unroll
                    for (int c = 0; c < pnp::SUMS; ++c) S[c] = red[c * BLOCK];
                    if (pnp::gn_solve(S, delta)) pnp::pose_update(q, t, delta);
                }
                float model[12];
                pnp::model_of_pose(q, t, model);
#pragma unroll
                for (int k = 0; k < 12; ++k) cur[k] = model[k];
            }
            __syncthreads();
            if (s == pnp::STEPS) break;
            float w[12], part[pnp::SUMS];
#pragma unroll
            for (int k = 0; k < 12; ++k) w[k] = cur[k];
#pragma unroll
            for (int c = 0; c < pnp::SUMS; ++c) part[c] = 0.0f;
            for (int i = tid; i < n; i += BLOCK) {
                const int idx = prev[i];
                float terms[pnp::SUMS];
                pnp::gn_terms(w, cam, X[idx], X[stride + idx], X[2 * stride + idx], X[3 * stride + idx], X[4 * stride + idx], terms);
#pragma unroll
                for (int c = 0; c < pnp::SUMS; ++c) part[c] = part[c] + terms[c];
            }
            tree<pnp::SUMS>(part);
        }
    }
    __device__ __forceinline__ int select(float thr) {
        float w[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) w[k] = cur[k];
        return Group::select(err, [&](int i, float& e) __attribute__((always_inline)) { return inlier(w, i, thr, e); });
    }
    __device__ __forceinline__ float threshold(float thr0) {
        if (tid == 0) *bcast = (double)pnp::refined_threshold(err, n_last, thr0);
        __syncthreads();
        const float v = (float)*bcast;
        __syncthreads();
        return v;
    }
    __device__ __forceinline__ void covariance(int kind, const float pose[12], int ratio, double& lin, double& cosine) {
        const int n = n_prev;
        lin = 1.0; cosine = 1.0;
        float w[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) w[k] = cur[k];
        if (kind == 1) {
            float cam_pose[12];
            m3d::invert(w, cam_pose);
            uint32_t* kd = reinterpret_cast<uint32_t*>(err);
            uint32_t* kc = reinterpret_cast<uint32_t*>(next);
            for (int i = tid; i < n; i += BLOCK) {
                const int j = prev[i];
                float d2, c;
                pnp::cov_terms(pose, w, cam_pose, cam, X[j], X[stride + j], X[2 * stride + j], X[3 * stride + j], X[4 * stride + j], has_to,
                               has_to ? X[5 * stride + j] : 0.0f, has_to ? X[6 * stride + j] : 0.0f, has_to ? X[7 * stride + j] : 0.0f, d2, c);
                kd[i] = pnp::order_key(d2);
                kc[i] = pnp::order_key(c);
            }
            __syncthreads();
            const int k = n / ratio;
            lin = pnp::VARIANCE_FACTOR * (double)pnp::key_value(ranked(kd, n, k));
            cosine = (double)pnp::key_value(ranked(kc, n, n - 1 - k));
        } else {
            if (tid == 0) {
                float e = 0.0f;                                        // the reference's serial sum, in the inliers' order
                for (int i = 0; i < n; ++i) {
                    const int j = prev[i];
                    bool front;
                    const float ee = pnp::reproj_sq(w, cam, X[j], X[stride + j], X[2 * stride + j], X[3 * stride + j], X[4 * stride + j], front);
                    e = e + ee;
                }
                const float mean = e / (float)n;
                *bcast = (double)sqrtf(mean);
            }
            __syncthreads();
            lin = *bcast;
            __syncthreads();
        }
    }
};

__global__ __launch_bounds__(BLOCK) void motion_pnp_kernel(PnpArgs a) {
    __shared__ int wsum[WAVES];
    __shared__ int valid[BLOCK];
    __shared__ int hist[256];
    __shared__ unsigned long long best;
    __shared__ double bcast;
    __shared__ float cur[12];
    __shared__ float model0[12];
    __shared__ float local[12];
    const PnpJob& J = a.jobs[blockIdx.x];
    const int nf = J.n_from, nt = J.n_to, tid = threadIdx.x;
    const int64_t first_from = J.first_from, first_to = J.first_to;
    if (tid < 12) { model0[tid] = J.model0[tid]; local[tid] = J.local[tid]; cur[tid] = 0.0f; }
    uint32_t* scratch = a.scratch + (size_t)SCRATCH_WORDS * first_to;
    float* gx = reinterpret_cast<float*>(scratch);                     // [planes][nt]
    int32_t* out_matches = a.out_matches + first_to;
    const bool has_to = a.planes == MAX_PLANES;

    // ---- (a) join: walk the to-frame's ids (util3d_motion_estimation.cpp:89-106)
    const int m = join_compact<MAX_PLANES>(pnp_smem, a.p_max, a.from_ids + first_from, nf, a.to_ids + first_to, nt, a.planes, out_matches, gx, wsum,
                                           [&](uint32_t row_t, uint32_t row_f, float* c) __attribute__((always_inline)) {
        const float* pf = a.from_xyz + (first_from + (int64_t)row_f) * 3;
        c[0] = pf[0]; c[1] = pf[1]; c[2] = pf[2];
        const bool keep = m3d::finite(c[0]) && m3d::finite(c[1]) && m3d::finite(c[2]);
        if (keep) {
            const float* pp = a.to_points + (first_to + (int64_t)row_t) * 2;
            c[3] = pp[0]; c[4] = pp[1];
            if (has_to) {
                const float* pt = a.to_xyz + (first_to + (int64_t)row_t) * 3;
                c[5] = pt[0]; c[6] = pt[1]; c[7] = pt[2];
            }
        }
        return keep;
    });

    GroupBackend b;
    b.seed = a.seed; b.iterations = a.iterations; b.has_to = has_to;
    b.cam = pnp::Camera{J.fx, J.fy, J.cx, J.cy, J.width, J.height};
    b.model0 = model0; b.bcast = &bcast;
    b.err = gx + (size_t)MAX_PLANES * nt;
    b.init(m, pnp_smem, pnp::SUMS, wsum, valid, hist, &best, cur, reinterpret_cast<int32_t*>(scratch) + (size_t)(MAX_PLANES + 1) * nt, gx, a.planes, nt,
           a.stage_cap);

    // ---- (b), (c), (d): the rule's own control flow
    pnp::Result r;
    pnp::solve(b, m, a.min_inliers, a.refine_iterations, a.reproj_error, a.ratio, a.max_variance, J.kind, J.has_local != 0, local, r);

    // ---- (e) outputs
    b.write_inliers(a.out_inliers + first_to, out_matches, nt, r.n_inliers);
    if (tid == 0) {
        float* t = a.out_transform + (size_t)blockIdx.x * 12;
#pragma unroll
        for (int k = 0; k < 12; ++k) t[k] = r.transform[k];
        a.out_status[blockIdx.x] = r.status;
        a.out_n_matches[blockIdx.x] = m;
        a.out_n_inliers[blockIdx.x] = r.n_inliers;
        a.out_variance_lin[blockIdx.x] = r.variance_lin;
        a.out_angle_cos[blockIdx.x] = r.angle_cos;
        a.out_variance_kind[blockIdx.x] = r.kind;
    }
}

const float IDENTITY[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};

}  // namespace
}  // namespace lcd

using namespace lcd;

namespace {

int estimate_motion_pnp(lcd_engine* h, const lcd_motion_pnp_args* a, bool on_device) {
    const char* who = on_device ? "lcd_estimate_motion_pnp_dev" : "lcd_estimate_motion_pnp";
    auto bad = [&](int code, const char* what) { return h->fail(code, std::string(who) + ": " + what); };
    // ---- everything that can be refused is refused before anything is enqueued or written
    if (!a || a->struct_size != (int32_t)sizeof(lcd_motion_pnp_args)) return bad(LCD_ERR_INVALID, "null arguments or wrong struct_size");
    if (a->iterations < 1) return bad(LCD_ERR_INVALID, "iterations is >= 1");
    if (a->iterations > 65535) return bad(LCD_ERR_UNSUPPORTED, "more than 65535 iterations");
    const float thr0 = (float)a->reproj_error;
    if (!std::isfinite(a->reproj_error) || !(a->reproj_error > 0.0) || !(thr0 > 0.0f) || !std::isfinite((float)((double)thr0 * (double)thr0)))
        return bad(LCD_ERR_INVALID, "reproj_error is finite and > 0, as a float and squared too");
    if (a->refine_iterations < 0 || a->min_inliers < 1) return bad(LCD_ERR_INVALID, "refine_iterations is >= 0 and min_inliers >= 1");
    if (a->variance_median_ratio <= 1) return bad(LCD_ERR_INVALID, "variance_median_ratio is > 1");
    if (!(a->max_variance >= 0.0f) || !std::isfinite(a->max_variance)) return bad(LCD_ERR_INVALID, "max_variance is finite and >= 0");
    if (const int rc = refuse_pairs(h, a->n_pairs, bad)) return rc;
    if (a->n_pairs == 0) return LCD_OK;
    const int np = a->n_pairs;
    const int64_t* fo = a->from_offsets;
    const int64_t* to = a->to_offsets;
    int n_max, m_max;
    if (const int rc = refuse_offsets(np, fo, to, bad, n_max, m_max)) return rc;
    if (!a->cameras) return bad(LCD_ERR_INVALID, "null cameras");
    for (int i = 0; i < np; ++i) {
        const lcd_camera& c = a->cameras[i];
        if (!std::isfinite(c.fx) || !std::isfinite(c.fy) || c.fx == 0.0f || c.fy == 0.0f) return bad(LCD_ERR_INVALID, "a camera whose fx or fy is 0 or not finite");
    }
    const int64_t Nf = fo[np], Nt = to[np];
    if (!a->out_transform || !a->out_status || !a->out_n_matches || !a->out_n_inliers || !a->out_variance_lin || !a->out_angle_cos || !a->out_variance_kind)
        return bad(LCD_ERR_INVALID, "a null per-pair output");
    if (Nf > 0 && (!a->from_word_ids || !a->from_xyz)) return bad(LCD_ERR_INVALID, "null from-arrays");
    if (Nt > 0 && (!a->to_word_ids || !a->to_points || !a->out_matches || !a->out_inliers)) return bad(LCD_ERR_INVALID, "null to-arrays or id outputs");

    StatelessScratch& S = h->pairs;
    hipStream_t st = h->stream;
    const bool has_to = a->to_xyz != nullptr;
    std::vector<PnpJob> jobs((size_t)np);
    for (int i = 0; i < np; ++i) {
        const lcd_camera& c = a->cameras[i];
        PnpJob& j = jobs[(size_t)i];
        j.first_from = fo[i]; j.first_to = to[i]; j.n_from = (int32_t)(fo[i + 1] - fo[i]); j.n_to = (int32_t)(to[i + 1] - to[i]);
        j.fx = c.fx; j.fy = c.fy; j.cx = c.cx; j.cy = c.cy; j.width = c.image_width; j.height = c.image_height;
        j.has_local = c.has_local_transform != 0;
        j.kind = has_to || c.image_width != 0 || c.image_height != 0 ? 1 : 2;
        pnp::model_of_guess(a->guesses ? a->guesses + (size_t)12 * i : IDENTITY, j.has_local != 0, c.local_transform, j.model0);
        for (int k = 0; k < 12; ++k) j.local[k] = j.has_local ? c.local_transform[k] : IDENTITY[k];
    }

    PnpArgs g;
    g.min_inliers = a->min_inliers; g.iterations = a->iterations; g.refine_iterations = a->refine_iterations; g.ratio = a->variance_median_ratio;
    g.seed = a->seed; g.max_variance = a->max_variance; g.reproj_error = a->reproj_error;
    g.planes = has_to ? MAX_PLANES : 5;
    const GroupPlan plan = group_plan(n_max, m_max, FIXED_BYTES, (size_t)g.planes * 4);
    g.p_max = plan.p_max; g.stage_cap = plan.stage_cap;
    g.from_ids = a->from_word_ids; g.from_xyz = a->from_xyz; g.to_ids = a->to_word_ids; g.to_points = a->to_points; g.to_xyz = a->to_xyz;
    g.out_transform = a->out_transform; g.out_status = a->out_status; g.out_n_matches = a->out_n_matches; g.out_n_inliers = a->out_n_inliers;
    g.out_variance_lin = a->out_variance_lin; g.out_angle_cos = a->out_angle_cos; g.out_variance_kind = a->out_variance_kind;
    g.out_matches = a->out_matches; g.out_inliers = a->out_inliers;

    // ---- host entry: everything to the device, results back at the end (one synchronisation)
    HostStage stage(S, host_row_bytes(h), (size_t)h->row_bytes, on_device);
    stage.in(g.from_ids, (size_t)Nf * 4); stage.in(g.from_xyz, (size_t)Nf * 12);
    stage.in(g.to_ids, (size_t)Nt * 4); stage.in(g.to_points, (size_t)Nt * 8);
    stage.in(g.to_xyz, (size_t)Nt * 12);                               // optional: null stays null
    stage.out(g.out_transform, (size_t)np * 48); stage.out(g.out_status, (size_t)np * 4);
    stage.out(g.out_n_matches, (size_t)np * 4); stage.out(g.out_n_inliers, (size_t)np * 4);
    stage.out(g.out_variance_lin, (size_t)np * 8); stage.out(g.out_angle_cos, (size_t)np * 8);
    stage.out(g.out_variance_kind, (size_t)np * 4);
    stage.out(g.out_matches, (size_t)Nt * 4); stage.out(g.out_inliers, (size_t)Nt * 4);
    LCD_HIP(h, stage.commit(st, &h->bytes_device));
    LCD_HIP(h, dreserve(h, S.d_small, (size_t)std::max<int64_t>(Nt, 1) * SCRATCH_WORDS * 4));
    g.scratch = S.d_small.as<uint32_t>();
    LCD_HIP(h, S.upload_table(&g.jobs, st, &h->bytes_device, jobs.data(), jobs.size() * sizeof(PnpJob)));
    allow_large_lds<&motion_pnp_kernel>();
    motion_pnp_kernel<<<dim3((unsigned)np), dim3(BLOCK), plan.lds, st>>>(g);
    LCD_HIP(h, hipGetLastError());
    LCD_HIP(h, stage.finish(st));
    return LCD_OK;
}

}  // namespace

extern "C" {

int lcd_estimate_motion_pnp(lcd_engine* h, const lcd_motion_pnp_args* a) { return stateless_entry(h, "lcd_estimate_motion_pnp", estimate_motion_pnp, a, false); }
int lcd_estimate_motion_pnp_dev(lcd_engine* h, const lcd_motion_pnp_args* a) { return stateless_entry(h, "lcd_estimate_motion_pnp", estimate_motion_pnp, a, true); }

}  // extern "C"
