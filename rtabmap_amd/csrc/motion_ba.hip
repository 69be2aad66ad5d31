// motion_ba.hip -- lcd_refine_motion_ba and its _dev form: the two-pose bundle adjustment behind the visual registration's motion estimate
// (reference RegistrationVis.cpp:1873-2188 with Vis/BundleAdjustment = 1, OptimizerG2O::optimizeBA, OptimizerG2O.cpp:1429-2117) for a caller who
// holds both frames and the PnP's outputs in device memory.  The rule is include/lcd.h's; its arithmetic and its control flow (stages, schedule,
// gates) are motion_ba_rule.h's, compiled here for the device and in host/MotionBA.cpp for the mirror.
//   motion_ba_kernel: one launch per call, one workgroup of 256 threads per pair, in phases behind barriers:
//     (a) lookup: both frames' sorted keys in LDS (motion_join.cuh); every inlier id is found in both, its point's state (the initial and the
//         current estimate, the saved copy of a rejected trial, the two observations, the flags with the edge levels, the to-depth) goes to the
//         call's scratch and, when it fits behind the 27 rows of lane partials, into LDS; one pointer serves both.
//     (b) the rule's stages: thread tid owns the points tid, tid + 256, ..: their blocks, their 27 Schur terms (Group::tree), their
//         back-substitution, their part of the fp64 cost and gain sums; the 6 x 6 system, the camera edge and the pose are thread 0's.
//     (c) the survivors' ids compacted in input order, the gates, the outputs.
// Nothing of the engine is read or written: the job table is StatelessScratch's, the per-row scratch its d_small.
#include "motion_group.cuh"
#include "motion_ba_rule.h"

#include <cmath>
#include <vector>

static_assert(sizeof(lcd_motion_ba_args) == 248, "lcd_motion_ba_args: the layout include/lcd.h documents (LP64)");
static_assert(LCD_BA_OK == lcd::ba::ST_OK && LCD_BA_NO_INPUT == lcd::ba::ST_NO_INPUT && LCD_BA_BAD_INLIER == lcd::ba::ST_BAD_INLIER &&
              LCD_BA_DIVERGED == lcd::ba::ST_DIVERGED && LCD_BA_BELOW_MIN_INLIERS == lcd::ba::ST_BELOW_MIN_INLIERS &&
              LCD_BA_MEAN_DISTANCE_REJECTED == lcd::ba::ST_MEAN_DISTANCE_REJECTED && LCD_BA_DISTRIBUTION_REJECTED == lcd::ba::ST_DISTRIBUTION_REJECTED,
              "lcd_motion_ba_status");

namespace lcd {
namespace {

constexpr size_t FIXED_BYTES = (size_t)BLOCK * ba::SUMS * 4;            // the rows of lane partials; the fp64 sums use their front
constexpr size_t POINT_BYTES = (size_t)ba::PLANES * 4;
// a point's planes
constexpr int PL_P0 = 0, PL_P = 3, PL_SAVED = 6, PL_FROM = 9, PL_TO = 12, PL_FLAGS = 15, PL_DEPTH = 16;

struct BaJob {
    int64_t first_from, first_to;            // the pair's first row in the from- / to-arrays
    int32_t n_from, n_to;
    ba::Frame f;                             // read where it is used: a copy in registers would live across the whole adjustment
    int32_t width, height;                   // of the to-camera
    int32_t has_local_to, distribution_valid;
    double base_from, base_to;
    float inv_local_to[12], local_to[12];
};
static_assert(sizeof(BaJob) == 264, "the job table");

struct BaArgs {
    const BaJob* jobs;
    int min_inliers, iterations;
    float max_mean_distance, min_distribution;
    int p_max;                               // keys per side the LDS carve holds (a power of two >= every frame)
    int stage_cap;                           // points whose state fits the carve behind the fixed part
    const int32_t* from_ids; const float* from_xyz; const float* from_points; const int32_t* to_ids; const float* to_points; const float* to_xyz;
    const int32_t* inliers; const int32_t* n_inliers; const float* transforms;
    uint32_t* scratch;                       // [PLANES x Nt] words; a pair's part starts at PLANES x first_to
    float* out_transform; int32_t* out_status; int32_t* out_inliers; int32_t* out_n_inliers; int32_t* out_n_outliers; double* out_chi2_before;
    double* out_chi2_after; int32_t* out_lm_accepted; float* out_mean_distance; float* out_distribution;
};

extern __shared__ __attribute__((aligned(16))) unsigned char ba_smem[];

// the backend of ba::solve as a workgroup: every method is called by all 256 threads and returns the same value to each
struct GroupBackend {
    Group g;                                 // the halving tree and what it needs: tid, red
    const ba::Frame& f;
    __device__ __forceinline__ explicit GroupBackend(const ba::Frame& frame) : f(frame) {}
    int n, tid;
    float* S;                                // word w of point i: S[w * stride + i]; LDS or the scratch
    int stride;
    int* wsum;
    float* cur; float* moved; float* C0;     // the moving camera's model, the trial's, its initial pose
    float* pose; float* pose_saved;          // thread 0's (q, t)
    float* dcs;                              // the camera's step
    double* bcast;
    int* ok;
    const int32_t* ids_in; int32_t* ids_out;
    int rows;
    float cx, cy;
    int32_t width, height;

    __device__ __forceinline__ void load(int i, ba::Point& pt) const {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            pt.p0[a] = S[(PL_P0 + a) * stride + i]; pt.p[a] = S[(PL_P + a) * stride + i];
            pt.of[a] = S[(PL_FROM + a) * stride + i]; pt.ot[a] = S[(PL_TO + a) * stride + i];
        }
        pt.flags = m3d::bits_of(S[PL_FLAGS * stride + i]);
    }
    __device__ __forceinline__ void model_of(const float* src, float m[12]) const {
#pragma unroll
        for (int k = 0; k < 12; ++k) m[k] = src[k];
    }
    // the fp64 halving tree of C sums in the front of red; the sums are red64[c * BLOCK], read into out; ends behind a barrier
    template <int C>
    __device__ __forceinline__ void tree64(const double part[C], double out[C]) {
        double* red64 = reinterpret_cast<double*>(g.red);
#pragma unroll
        for (int c = 0; c < C; ++c) red64[c * BLOCK + tid] = part[c];
        __syncthreads();
        for (int s = BLOCK / 2; s >= 1; s >>= 1) {
            if (tid < s) {
#pragma unroll
                for (int c = 0; c < C; ++c) red64[c * BLOCK + tid] = red64[c * BLOCK + tid] + red64[c * BLOCK + tid + s];
            }
            __syncthreads();
        }
#pragma unroll
        for (int c = 0; c < C; ++c) out[c] = red64[c * BLOCK];
        __syncthreads();
    }
    __device__ __forceinline__ double prior_cost_under(const float m[12]) const {
        float c0[12], e[6], q[4], rt[3];
        model_of(C0, c0);
        ba::prior_error(m, c0, e, q, rt);
        return ba::prior_cost(f, e);
    }
    __device__ __forceinline__ double cost() {
        float m[12];
        model_of(cur, m);
        double part[1] = {0.0}, sum[1];
        for (int i = tid; i < n; i += BLOCK) {
            ba::Point pt;
            load(i, pt);
            float cf, ct;
            const double c = ba::point_cost(f, m, pt, cf, ct);
            part[0] = part[0] + c;
        }
        tree64<1>(part, sum);
        return sum[0] + prior_cost_under(m);
    }
    __device__ __forceinline__ float max_diagonal() {
        float m[12], c0[12];
        model_of(cur, m);
        model_of(C0, c0);
        float top = 0.0f, part[6];
#pragma unroll
        for (int d = 0; d < 6; ++d) part[d] = 0.0f;
        for (int i = tid; i < n; i += BLOCK) {
            ba::Point pt;
            load(i, pt);
            ba::Blocks B;
            if (ba::point_blocks(f, m, pt, B)) {
                top = B.Hpp[0] > top ? B.Hpp[0] : top; top = B.Hpp[3] > top ? B.Hpp[3] : top; top = B.Hpp[5] > top ? B.Hpp[5] : top;
            }
            part[0] = part[0] + B.Hcc[0]; part[1] = part[1] + B.Hcc[6]; part[2] = part[2] + B.Hcc[11];
            part[3] = part[3] + B.Hcc[15]; part[4] = part[4] + B.Hcc[18]; part[5] = part[5] + B.Hcc[20];
        }
        g.tree<6>(part);
        g.red[6 * BLOCK + tid] = top;
        __syncthreads();
        for (int l = 0; l < BLOCK; ++l) { const float v = g.red[6 * BLOCK + l]; top = v > top ? v : top; }
        ba::Prior pr;
        ba::prior_system(f, m, c0, pr);
#pragma unroll
        for (int d = 0; d < 6; ++d) {
            const float v = g.red[d * BLOCK] + pr.P[ba::diag6(d)];
            top = v > top ? v : top;
        }
        __syncthreads();                                               // red is read
        return top;
    }
    __device__ __forceinline__ bool trial(float lambda, double& F, double& scale) {
        float m[12];
        model_of(cur, m);
        {
            float part[ba::SUMS];
#pragma unroll
            for (int c = 0; c < ba::SUMS; ++c) part[c] = 0.0f;
            for (int i = tid; i < n; i += BLOCK) {
                ba::Point pt;
                load(i, pt);
                ba::Blocks B;
                float terms[ba::SUMS];
                if (ba::point_blocks(f, m, pt, B)) {
                    ba::point_terms(B, lambda, terms);
                } else {
#pragma unroll
                    for (int c = 0; c < ba::SUMS; ++c) terms[c] = 0.0f;
                }
#pragma unroll
                for (int c = 0; c < ba::SUMS; ++c) part[c] = part[c] + terms[c];
            }
            g.tree<ba::SUMS>(part);
        }
        if (tid == 0) {
            float sums[ba::SUMS], c0[12], q[4], t[3], dc[6];
#pragma unroll
            for (int c = 0; c < ba::SUMS; ++c) sums[c] = g.red[c * BLOCK];
            model_of(C0, c0);
            ba::Prior pr;
            ba::prior_system(f, m, c0, pr);
#pragma unroll
            for (int k = 0; k < 7; ++k) pose_saved[k] = pose[k];
            q[0] = pose[0]; q[1] = pose[1]; q[2] = pose[2]; q[3] = pose[3]; t[0] = pose[4]; t[1] = pose[5]; t[2] = pose[6];
            double scale0 = 0.0;
            const bool solved = ba::camera_step(f, sums, pr, lambda, q, t, dc, scale0);
            if (solved) {
                float mm[12];
                pnp::model_of_pose(q, t, mm);
#pragma unroll
                for (int k = 0; k < 12; ++k) moved[k] = mm[k];
                pose[0] = q[0]; pose[1] = q[1]; pose[2] = q[2]; pose[3] = q[3]; pose[4] = t[0]; pose[5] = t[1]; pose[6] = t[2];
#pragma unroll
                for (int k = 0; k < 6; ++k) dcs[k] = dc[k];
                bcast[0] = scale0;
            }
            *ok = solved ? 1 : 0;
        }
        __syncthreads();
        if (!*ok) return false;
        float mm[12], dc[6];
        model_of(moved, mm);
#pragma unroll
        for (int k = 0; k < 6; ++k) dc[k] = dcs[k];
        const double scale0 = bcast[0];
        double part[2] = {0.0, 0.0}, sum[2];
        for (int i = tid; i < n; i += BLOCK) {
            ba::Point pt;
            load(i, pt);
#pragma unroll
            for (int a = 0; a < 3; ++a) S[(PL_SAVED + a) * stride + i] = pt.p[a];
            ba::Blocks B;
            double sc = 0.0;
            if (ba::point_blocks(f, m, pt, B)) {
                float dp[3];
                ba::point_step(B, lambda, dc, dp, sc);
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    pt.p[a] = pt.p[a] + dp[a];
                    S[(PL_P + a) * stride + i] = pt.p[a];
                }
            }
            part[0] = part[0] + sc;
            float cf, ct;
            const double c = ba::point_cost(f, mm, pt, cf, ct);
            part[1] = part[1] + c;
        }
        tree64<2>(part, sum);
        scale = sum[0] + scale0;
        F = sum[1] + prior_cost_under(mm);
        return true;
    }
    __device__ __forceinline__ void restore() {
        for (int i = tid; i < n; i += BLOCK) {
#pragma unroll
            for (int a = 0; a < 3; ++a) S[(PL_P + a) * stride + i] = S[(PL_SAVED + a) * stride + i];
        }
        if (tid == 0) {
#pragma unroll
            for (int k = 0; k < 7; ++k) pose[k] = pose_saved[k];
        }
        __syncthreads();
    }
    __device__ __forceinline__ void accept() {
        if (tid < 12) cur[tid] = moved[tid];
        __syncthreads();
    }
    __device__ __forceinline__ void flag_outliers() {
        float m[12];
        model_of(cur, m);
        for (int i = tid; i < n; i += BLOCK) {
            ba::Point pt;
            load(i, pt);
            float cf, ct;
            (void)ba::point_cost(f, m, pt, cf, ct);
            uint32_t add = 0;
            if (ba::from_active(pt.flags) && cf > f.delta) add |= ba::F_FROM_OUT;
            if (ba::to_active(pt.flags) && ct > f.delta) add |= ba::F_TO_OUT;
            if (add) {
                S[PL_FLAGS * stride + i] = m3d::float_of(pt.flags | add | ba::F_OUTLIER);
#pragma unroll
                for (int a = 0; a < 3; ++a) S[(PL_P + a) * stride + i] = pt.p0[a];
            }
        }
        __syncthreads();
    }
    // the ids of the points that are no outliers to ids_out in input order, zeros behind them; their indices into the saved plane's first word
    __device__ __forceinline__ int survivors() {
        int count = 0;
        for (int base = 0; base < n; base += BLOCK) {
            const int i = base + tid;
            const bool keep = i < n && (m3d::bits_of(S[PL_FLAGS * stride + i]) & ba::F_OUTLIER) == 0u;
            const int32_t id = i < n ? ids_in[i] : 0;
            int total;
            const int pos = count + block_rank(keep, wsum, total);
            if (keep) { ids_out[pos] = id; S[PL_SAVED * stride + pos] = m3d::float_of((uint32_t)i); }
            count += total;
        }
        for (int j = count + tid; j < rows; j += BLOCK) ids_out[j] = 0;
        __syncthreads();
        return count;
    }
    __device__ __forceinline__ float mean_distance(int count, bool& any) {
        if (tid == 0) {
            float sum = 0.0f;                                          // uMean: the reference's serial sum, in the inliers' order
            int used = 0;
            for (int j = 0; j < count; ++j) {
                const int i = (int)m3d::bits_of(S[PL_SAVED * stride + j]);
                if ((m3d::bits_of(S[PL_FLAGS * stride + i]) & ba::F_TO_FINITE) == 0u) continue;
                sum = sum + S[PL_DEPTH * stride + i];
                ++used;
            }
            const float mean = used > 0 ? sum / (float)used : 0.0f;
            bcast[0] = (double)mean;
            *ok = used;
        }
        __syncthreads();
        any = *ok > 0;
        const float v = (float)bcast[0];
        __syncthreads();
        return v;
    }
    __device__ __forceinline__ float distribution(int count) {
        const float nn = (float)count;
        float part[2] = {0.0f, 0.0f};
        for (int j = tid; j < count; j += BLOCK) {
            const int i = (int)m3d::bits_of(S[PL_SAVED * stride + j]);
            const float x = ba::normalised(S[PL_TO * stride + i], cx, width), y = ba::normalised(S[(PL_TO + 1) * stride + i], cy, height);
            part[0] = part[0] + x; part[1] = part[1] + y;
        }
        g.tree<2>(part);
        const float sx = g.red[0], sy = g.red[BLOCK];
        __syncthreads();
        const float mx = sx / nn, my = sy / nn;
        float sq[3] = {0.0f, 0.0f, 0.0f};
        for (int j = tid; j < count; j += BLOCK) {
            const int i = (int)m3d::bits_of(S[PL_SAVED * stride + j]);
            const float x = ba::normalised(S[PL_TO * stride + i], cx, width), y = ba::normalised(S[(PL_TO + 1) * stride + i], cy, height);
            const float d = x - mx, e = y - my;
            const float dd = d * d, de = d * e, ee = e * e;
            sq[0] = sq[0] + dd; sq[1] = sq[1] + de; sq[2] = sq[2] + ee;
        }
        g.tree<3>(sq);
        const float sxx = g.red[0], sxy = g.red[BLOCK], syy = g.red[2 * BLOCK];
        __syncthreads();
        const float a = sxx / nn, b = sxy / nn, c = syy / nn;
        return ba::small_eigenvalue(a, b, c);
    }
    __device__ __forceinline__ const float* model() const { return cur; }
};

__global__ __launch_bounds__(BLOCK) void motion_ba_kernel(BaArgs a) {
    __shared__ int wsum[WAVES];
    __shared__ double bcast[2];
    __shared__ float cur[12];
    __shared__ float moved[12];
    __shared__ float C0[12];
    __shared__ float pose[8];
    __shared__ float pose_saved[8];
    __shared__ float dcs[8];
    __shared__ int ok;
    const BaJob& J = a.jobs[blockIdx.x];
    const int nf = J.n_from, nt = J.n_to, tid = threadIdx.x;
    const int64_t first_from = J.first_from, first_to = J.first_to;
    const int32_t* ids_in = a.inliers + first_to;
    int32_t* ids_out = a.out_inliers + first_to;
    const float* T = a.transforms + (size_t)blockIdx.x * 12;
    const int n_raw = a.n_inliers[blockIdx.x];
    const int n = n_raw < 0 ? 0 : n_raw > nt ? nt : n_raw;

    bool zero = true;
#pragma unroll
    for (int k = 0; k < 12; ++k) zero = zero && T[k] == 0.0f;
    int status = zero || n_raw == 0 ? ba::ST_NO_INPUT : n_raw < 0 || n_raw > nt ? ba::ST_BAD_INLIER : ba::ST_OK;

    // ---- (a) lookup: every inlier id in both frames (RegistrationVis.cpp:1964-2027)
    float* gx = reinterpret_cast<float*>(a.scratch + (size_t)ba::PLANES * first_to);   // [PLANES][nt]
    if (status == ba::ST_OK) {
        uint64_t* keys_f = reinterpret_cast<uint64_t*>(ba_smem);
        uint64_t* keys_t = keys_f + padded(a.p_max);
        join_sort_keys(keys_f, a.from_ids + first_from, nf);
        join_sort_keys(keys_t, a.to_ids + first_to, nt);
        int bad = 0;
        for (int i = tid; i < n; i += BLOCK) {
            const uint32_t idk = m3d::id_key(ids_in[i]);
            uint32_t row_f, row_t;
            const bool found = join_find_unique(keys_f, nf, idk, row_f) && join_find_unique(keys_t, nt, idk, row_t);
            if (!found) { bad = 1; continue; }
            const float* pf = a.from_xyz + (first_from + (int64_t)row_f) * 3;
            const float px = pf[0], py = pf[1], pz = pf[2];
            if (!(m3d::finite(px) && m3d::finite(py) && m3d::finite(pz))) { bad = 1; continue; }
            uint32_t flags = 0;
            float of[3] = {0.0f, 0.0f, 0.0f}, ot[3], depth;
            if (a.from_points) {
                const float* kf = a.from_points + (first_from + (int64_t)row_f) * 2;
                flags |= ba::F_FROM;
                if (ba::observe(J.f.M1, true, px, py, pz, J.base_from, J.f.v1.fx, kf[0], kf[1], of, depth)) flags |= ba::F_FROM_STEREO;
            }
            const float* kt = a.to_points + (first_to + (int64_t)row_t) * 2;
            float tx = 0.0f, ty = 0.0f, tz = 0.0f;
            if (a.to_xyz) {
                const float* pt = a.to_xyz + (first_to + (int64_t)row_t) * 3;
                tx = pt[0]; ty = pt[1]; tz = pt[2];
                if (m3d::finite(tx) && m3d::finite(ty) && m3d::finite(tz)) flags |= ba::F_TO_FINITE;
            }
            if (ba::observe(J.inv_local_to, a.to_xyz != nullptr, tx, ty, tz, J.base_to, J.f.v2.fx, kt[0], kt[1], ot, depth)) flags |= ba::F_TO_STEREO;
            gx[(size_t)(PL_P0 + 0) * nt + i] = px; gx[(size_t)(PL_P0 + 1) * nt + i] = py; gx[(size_t)(PL_P0 + 2) * nt + i] = pz;
            gx[(size_t)(PL_P + 0) * nt + i] = px; gx[(size_t)(PL_P + 1) * nt + i] = py; gx[(size_t)(PL_P + 2) * nt + i] = pz;
            gx[(size_t)(PL_SAVED + 0) * nt + i] = px; gx[(size_t)(PL_SAVED + 1) * nt + i] = py; gx[(size_t)(PL_SAVED + 2) * nt + i] = pz;
#pragma unroll
            for (int c = 0; c < 3; ++c) { gx[(size_t)(PL_FROM + c) * nt + i] = of[c]; gx[(size_t)(PL_TO + c) * nt + i] = ot[c]; }
            gx[(size_t)PL_FLAGS * nt + i] = m3d::float_of(flags);
            gx[(size_t)PL_DEPTH * nt + i] = depth;
        }
        if (__syncthreads_or(bad)) status = ba::ST_BAD_INLIER;         // behind the barrier the keys are dead, the state written
    }

    ba::Result r;
    if (status != ba::ST_OK) {
#pragma unroll
        for (int k = 0; k < 12; ++k) r.transform[k] = 0.0f;
        r.status = status; r.n_inliers = n; r.n_outliers = 0; r.lm_accepted = 0; r.chi2_before = 0.0; r.chi2_after = 0.0;
        r.mean_distance = 0.0f; r.distribution = 0.0f;
        for (int j = tid; j < nt; j += BLOCK) ids_out[j] = j < n ? ids_in[j] : 0;
    } else {
        GroupBackend b(J.f);
        b.n = n; b.tid = tid; b.g.tid = tid; b.g.red = reinterpret_cast<float*>(ba_smem);
        b.wsum = wsum; b.cur = cur; b.moved = moved; b.C0 = C0; b.pose = pose; b.pose_saved = pose_saved; b.dcs = dcs; b.bcast = bcast; b.ok = &ok;
        b.ids_in = ids_in; b.ids_out = ids_out; b.rows = nt;
        b.cx = J.f.v2.cx; b.cy = J.f.v2.cy; b.width = J.width; b.height = J.height;
        if (n <= a.stage_cap) {
            float* lx = b.g.red + BLOCK * ba::SUMS;
            for (int e = tid; e < ba::PLANES * n; e += BLOCK) { const int k = e / n, i = e - k * n; lx[e] = gx[(size_t)k * nt + i]; }
            b.S = lx; b.stride = n;
        } else {
            b.S = gx; b.stride = nt;
        }
        if (tid == 0) {
            float t0[12], c0[12], m0[12], q[4], t[3], m[12];
#pragma unroll
            for (int k = 0; k < 12; ++k) t0[k] = T[k];
            if (J.has_local_to) m3d::compose(t0, J.local_to, c0);
            else {
#pragma unroll
                for (int k = 0; k < 12; ++k) c0[k] = t0[k];
            }
            m3d::invert(c0, m0);
            pnp::quat_of_model(m0, q);
            t[0] = m0[3]; t[1] = m0[7]; t[2] = m0[11];
            pnp::model_of_pose(q, t, m);
#pragma unroll
            for (int k = 0; k < 12; ++k) { C0[k] = c0[k]; cur[k] = m[k]; moved[k] = m[k]; }
            pose[0] = q[0]; pose[1] = q[1]; pose[2] = q[2]; pose[3] = q[3]; pose[4] = t[0]; pose[5] = t[1]; pose[6] = t[2];
        }
        __syncthreads();

        // ---- (b), (c): the rule's own control flow
        ba::Params p;
        p.min_inliers = a.min_inliers; p.iterations = a.iterations; p.max_mean_distance = a.max_mean_distance; p.min_distribution = a.min_distribution;
        p.distribution_valid = J.distribution_valid != 0; p.has_to_xyz = a.to_xyz != nullptr; p.has_local = J.has_local_to != 0;
        ba::solve(b, n, J.f, p, T, J.local_to, r);
        if (r.status == ba::ST_DIVERGED)
            for (int j = tid; j < nt; j += BLOCK) ids_out[j] = j < n ? ids_in[j] : 0;
    }
    if (tid == 0) {
        float* t = a.out_transform + (size_t)blockIdx.x * 12;
#pragma unroll
        for (int k = 0; k < 12; ++k) t[k] = r.transform[k];
        a.out_status[blockIdx.x] = r.status;
        a.out_n_inliers[blockIdx.x] = r.n_inliers;
        a.out_n_outliers[blockIdx.x] = r.n_outliers;
        a.out_chi2_before[blockIdx.x] = r.chi2_before;
        a.out_chi2_after[blockIdx.x] = r.chi2_after;
        a.out_lm_accepted[blockIdx.x] = r.lm_accepted;
        a.out_mean_distance[blockIdx.x] = r.mean_distance;
        a.out_distribution[blockIdx.x] = r.distribution;
    }
}

const float IDENTITY[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};

}  // namespace
}  // namespace lcd

using namespace lcd;

namespace {

int refine_motion_ba(lcd_engine* h, const lcd_motion_ba_args* a, bool on_device) {
    const char* who = on_device ? "lcd_refine_motion_ba_dev" : "lcd_refine_motion_ba";
    auto bad = [&](int code, const char* what) { return h->fail(code, std::string(who) + ": " + what); };
    // ---- everything that can be refused is refused before anything is enqueued or written
    if (!a || a->struct_size != (int32_t)sizeof(lcd_motion_ba_args)) return bad(LCD_ERR_INVALID, "null arguments or wrong struct_size");
    if (a->iterations < 0 || a->min_inliers < 0) return bad(LCD_ERR_INVALID, "iterations and min_inliers are >= 0");
    if (a->iterations > 65535) return bad(LCD_ERR_UNSUPPORTED, "more than 65535 iterations");
    const float info = (float)(1.0 / a->pixel_variance), delta = (float)a->robust_delta;
    if (!std::isfinite(a->pixel_variance) || !(a->pixel_variance > 0.0) || !std::isfinite(info) || !(info > 0.0f))
        return bad(LCD_ERR_INVALID, "pixel_variance is finite and > 0, its inverse as a float too");
    if (!std::isfinite(a->robust_delta) || a->robust_delta < 0.0 || !std::isfinite(delta * delta)) return bad(LCD_ERR_INVALID, "robust_delta is finite and >= 0, as a float and squared too");
    if (!std::isfinite(a->max_inliers_mean_distance) || a->max_inliers_mean_distance < 0.0f || !std::isfinite(a->min_inliers_distribution) || a->min_inliers_distribution < 0.0f)
        return bad(LCD_ERR_INVALID, "the gates are finite and >= 0");
    if (!std::isfinite(a->default_baseline)) return bad(LCD_ERR_INVALID, "default_baseline is finite");
    if (const int rc = refuse_pairs(h, a->n_pairs, bad)) return rc;
    if (a->n_pairs == 0) return LCD_OK;
    const int np = a->n_pairs;
    const int64_t* fo = a->from_offsets;
    const int64_t* to = a->to_offsets;
    int n_max, m_max;
    if (const int rc = refuse_offsets(np, fo, to, bad, n_max, m_max)) return rc;
    if (!a->cameras_from || !a->cameras_to) return bad(LCD_ERR_INVALID, "null cameras");
    for (int i = 0; i < np; ++i)
        for (const lcd_camera* c : {a->cameras_from + i, a->cameras_to + i})
            if (!std::isfinite(c->fx) || !std::isfinite(c->fy) || c->fx == 0.0f || c->fy == 0.0f) return bad(LCD_ERR_INVALID, "a camera whose fx or fy is 0 or not finite");
    for (int i = 0; i < 2 * np; ++i) {
        if (a->prior_variance && (!std::isfinite(a->prior_variance[i]) || a->prior_variance[i] < 0.0)) return bad(LCD_ERR_INVALID, "a prior variance that is negative or not finite");
        if (a->baselines && !std::isfinite(a->baselines[i])) return bad(LCD_ERR_INVALID, "a baseline that is not finite");
    }
    const int64_t Nf = fo[np], Nt = to[np];
    if (!a->out_transform || !a->out_status || !a->out_n_inliers || !a->out_n_outliers || !a->out_chi2_before || !a->out_chi2_after || !a->out_lm_accepted ||
        !a->out_inliers_mean_distance || !a->out_inliers_distribution || !a->n_inliers || !a->transforms)
        return bad(LCD_ERR_INVALID, "a null per-pair input or output");
    if (Nf > 0 && (!a->from_word_ids || !a->from_xyz)) return bad(LCD_ERR_INVALID, "null from-arrays");
    if (Nt > 0 && (!a->to_word_ids || !a->to_points || !a->inliers || !a->out_inliers)) return bad(LCD_ERR_INVALID, "null to-arrays, inliers or id outputs");

    StatelessScratch& S = h->pairs;
    hipStream_t st = h->stream;
    std::vector<BaJob> jobs((size_t)np);
    for (int i = 0; i < np; ++i) {
        const lcd_camera& cf = a->cameras_from[i];
        const lcd_camera& ct = a->cameras_to[i];
        BaJob& j = jobs[(size_t)i];
        j.first_from = fo[i]; j.first_to = to[i]; j.n_from = (int32_t)(fo[i + 1] - fo[i]); j.n_to = (int32_t)(to[i + 1] - to[i]);
        j.f.info = info; j.f.delta = delta; j.f.delta2 = delta * delta; j.f.two_delta = 2.0f * delta;
        j.f.inf_lin = a->prior_variance ? ba::prior_information(a->prior_variance[2 * i], ba::LINEAR_EPSILON) : 1.0f;
        j.f.inf_ang = a->prior_variance ? ba::prior_information(a->prior_variance[2 * i + 1], ba::ANGULAR_EPSILON) : 1.0f;
        j.base_from = a->baselines ? a->baselines[2 * i] : a->default_baseline;
        j.base_to = a->baselines ? a->baselines[2 * i + 1] : a->default_baseline;
        j.f.v1 = ba::View{cf.fx, cf.fy, cf.cx, cf.cy, (float)j.base_from};
        j.f.v2 = ba::View{ct.fx, ct.fy, ct.cx, ct.cy, (float)j.base_to};
        j.width = ct.image_width; j.height = ct.image_height;
        j.has_local_to = ct.has_local_transform != 0;
        j.distribution_valid = ct.fx > 0.0f && ct.fy > 0.0f && ct.cx > 0.0f && ct.cy > 0.0f && ct.image_width > 0 && ct.image_height > 0;
        for (int k = 0; k < 12; ++k) j.local_to[k] = j.has_local_to ? ct.local_transform[k] : IDENTITY[k];
        m3d::invert(cf.has_local_transform ? cf.local_transform : IDENTITY, j.f.M1);
        m3d::invert(j.local_to, j.inv_local_to);
    }

    BaArgs g;
    g.min_inliers = a->min_inliers; g.iterations = a->iterations; g.max_mean_distance = a->max_inliers_mean_distance; g.min_distribution = a->min_inliers_distribution;
    const GroupPlan plan = group_plan(n_max, m_max, FIXED_BYTES, POINT_BYTES);
    g.p_max = plan.p_max; g.stage_cap = plan.stage_cap;
    g.from_ids = a->from_word_ids; g.from_xyz = a->from_xyz; g.from_points = a->from_points; g.to_ids = a->to_word_ids; g.to_points = a->to_points; g.to_xyz = a->to_xyz;
    g.inliers = a->inliers; g.n_inliers = a->n_inliers; g.transforms = a->transforms;
    g.out_transform = a->out_transform; g.out_status = a->out_status; g.out_inliers = a->out_inliers; g.out_n_inliers = a->out_n_inliers;
    g.out_n_outliers = a->out_n_outliers; g.out_chi2_before = a->out_chi2_before; g.out_chi2_after = a->out_chi2_after; g.out_lm_accepted = a->out_lm_accepted;
    g.out_mean_distance = a->out_inliers_mean_distance; g.out_distribution = a->out_inliers_distribution;

    // ---- host entry: everything to the device, results back at the end (one synchronisation)
    HostStage stage(S, host_row_bytes(h), (size_t)h->row_bytes, on_device);
    stage.in(g.from_ids, (size_t)Nf * 4); stage.in(g.from_xyz, (size_t)Nf * 12);
    stage.in(g.from_points, (size_t)Nf * 8);                           // optional: null stays null
    stage.in(g.to_ids, (size_t)Nt * 4); stage.in(g.to_points, (size_t)Nt * 8);
    stage.in(g.to_xyz, (size_t)Nt * 12);                               // optional
    stage.in(g.inliers, (size_t)Nt * 4); stage.in(g.n_inliers, (size_t)np * 4); stage.in(g.transforms, (size_t)np * 48);
    stage.out(g.out_transform, (size_t)np * 48); stage.out(g.out_status, (size_t)np * 4);
    stage.out(g.out_inliers, (size_t)Nt * 4); stage.out(g.out_n_inliers, (size_t)np * 4); stage.out(g.out_n_outliers, (size_t)np * 4);
    stage.out(g.out_chi2_before, (size_t)np * 8); stage.out(g.out_chi2_after, (size_t)np * 8); stage.out(g.out_lm_accepted, (size_t)np * 4);
    stage.out(g.out_mean_distance, (size_t)np * 4); stage.out(g.out_distribution, (size_t)np * 4);
    LCD_HIP(h, stage.commit(st, &h->bytes_device));
    LCD_HIP(h, dreserve(h, S.d_small, (size_t)std::max<int64_t>(Nt, 1) * ba::PLANES * 4));
    g.scratch = S.d_small.as<uint32_t>();
    LCD_HIP(h, S.upload_table(&g.jobs, st, &h->bytes_device, jobs.data(), jobs.size() * sizeof(BaJob)));
    allow_large_lds<&motion_ba_kernel>();
    motion_ba_kernel<<<dim3((unsigned)np), dim3(BLOCK), plan.lds, st>>>(g);
    LCD_HIP(h, hipGetLastError());
    LCD_HIP(h, stage.finish(st));
    return LCD_OK;
}

}  // namespace

extern "C" {

int lcd_refine_motion_ba(lcd_engine* h, const lcd_motion_ba_args* a) { return stateless_entry(h, "lcd_refine_motion_ba", refine_motion_ba, a, false); }
int lcd_refine_motion_ba_dev(lcd_engine* h, const lcd_motion_ba_args* a) { return stateless_entry(h, "lcd_refine_motion_ba", refine_motion_ba, a, true); }

}  // extern "C"
