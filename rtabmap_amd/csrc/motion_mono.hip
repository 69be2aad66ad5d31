// motion_mono.hip -- lcd_estimate_motion_mono and its _dev form: util3d::generateWords3DMono (reference util3d_features.cpp:209-413) behind
// RegistrationVis.cpp:1584-1675 with Vis/EstimationType = 2, for a caller who holds both monocular signatures' word ids and keypoints in device
// memory.  The rule is include/lcd.h's; its arithmetic is motion_mono_rule.h's, compiled here for the device and in host/MotionMono.cpp for the
// mirror.
//   motion_mono_kernel: one launch per call, one workgroup of 256 threads per pair, in phases behind barriers.  The join, the staging, the
//   selection and the radix select are motion_group.cuh's; the candidate loop is this file's own, because one five-point solve yields up to
//   ten candidates and Group::ransac makes one model per thread:
//     (a) join (join_compact): the to-frame's ids are walked, a negative id is refused, the normalised coordinates (from x, y, to x', y') and,
//         with from_points3, the from-frame's 3-D point go to the call's scratch and, when they fit, into LDS (Group::init).
//     (b) hypotheses in chunks of HYP = 32.  SOLVE: the solver's workspace is 256 doubles per hypothesis (the 10 x 20 constraint matrix alone
//         is 1 600 bytes: neither 256 of them fit the LDS nor one a lane's registers), so a chunk has 32 hypotheses, 64 KiB of LDS, element e
//         of hypothesis s at double e * 32 + s: the lanes of a wave read consecutive doubles whatever pivot rows they chose, without bank
//         conflicts.  Eight lanes of each of the four waves solve, so the four SIMDs run beside each other; each writes its up to ten matrices,
//         rounded to fp32, behind the workspace.  SCORE: as Group::ransac, each wave takes candidates in turn with a ballot count.
//     (c) the winner is solved again by thread 0 in fp64 and decomposed; every thread triangulates its correspondences under the four
//         configurations; the >= cascade chooses; Group::select compacts the inliers; their points go to the scratch.
//     (d) the scale and the variance: the usable 3-D correspondences compacted, the error list's element by Group::ranked, once with a guess,
//         once per correspondence without.
//     (e) outputs.
// Nothing of the engine is read or written: the job table is StatelessScratch's, the per-row scratch its d_small.
#include "motion_group.cuh"
#include "motion_mono_rule.h"

#include <cmath>
#include <vector>

static_assert(sizeof(lcd_motion_mono_args) == 184, "lcd_motion_mono_args: the layout include/lcd.h documents (LP64)");
static_assert(LCD_MONO_OK == lcd::mono::ST_OK && LCD_MONO_FEW_FEATURES == lcd::mono::ST_FEW_FEATURES && LCD_MONO_FEW_PAIRS == lcd::mono::ST_FEW_PAIRS &&
              LCD_MONO_NO_MODEL == lcd::mono::ST_NO_MODEL && LCD_MONO_FEW_INLIERS == lcd::mono::ST_FEW_INLIERS &&
              LCD_MONO_HIGH_VARIANCE == lcd::mono::ST_HIGH_VARIANCE, "lcd_motion_mono_status");
static_assert(LCD_MONO_BISECT == lcd::mono::BISECT, "the count include/lcd.h documents");

namespace lcd {
namespace {

constexpr int HYP = 32;                                                  // hypotheses per chunk
constexpr int SOLVERS_PER_WAVE = HYP / WAVES;
constexpr int CAND = HYP * mono::ROOTS;                                  // candidates per chunk
constexpr size_t WS_BYTES = (size_t)HYP * mono::WS * 8;                  // 64 KiB
static_assert(CAND * 9 <= MODEL_FLOATS, "the chunk's matrices fit Group's model area");
constexpr size_t FIXED_BYTES = WS_BYTES + group_fixed_bytes(1);
constexpr int MAX_PLANES = 7;
constexpr int SCRATCH_WORDS = MAX_PLANES + 9;                            // per to-row: the planes, the selection's values, two index sets, the ids when out_matches is NULL, the points, the usable list, the keys

struct MonoJob {
    int64_t first_from, first_to;            // the pair's first row in the from- / to-arrays
    int32_t n_from, n_to;
    float fx, fy, cx, cy;
    float thr2;                              // mono::threshold2
    int32_t has_guess;
    float guess_t[3];
    float local[12];
    int32_t pad;
};
static_assert(sizeof(MonoJob) == 112, "the job table");

struct MonoArgs {
    const MonoJob* jobs;
    int min_inliers, iterations, ratio;
    uint32_t seed;
    float max_variance;
    double distance;
    int p_max;                               // keys per side the LDS carve holds (a power of two >= every frame)
    int stage_cap;                           // correspondences whose coordinates fit the carve behind the fixed part
    int planes;                              // 7 with from_points3, 4 without
    const int32_t* from_ids; const float* from_points; const float* from_points3; const int32_t* to_ids; const float* to_points;
    uint32_t* scratch;                       // [SCRATCH_WORDS x Nt] words; a pair's part starts at SCRATCH_WORDS x first_to
    float* out_transform; int32_t* out_status; int32_t* out_n_matches; int32_t* out_n_inliers; double* out_variance;
    int32_t* out_matches; int32_t* out_inliers; float* out_points3;
};

// element e of one hypothesis' workspace
struct LdsWs {
    double* p;
    __device__ __forceinline__ double& operator()(int e) const { return p[e * HYP]; }
};

extern __shared__ __attribute__((aligned(16))) unsigned char mono_smem[];

// hypothesis h solved in workspace w: its number of real roots, 0 when it is invalid
template <class At>
__device__ __forceinline__ int solve_hypothesis(LdsWs w, uint32_t seed, uint32_t h, int m, At at) {
    int idx[5];
    if (!mono::draw5(seed, h, (uint32_t)m, idx)) return 0;
    float x1[5], y1[5], x2[5], y2[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) { x1[j] = at(0, idx[j]); y1[j] = at(1, idx[j]); x2[j] = at(2, idx[j]); y2[j] = at(3, idx[j]); }
    return mono::solve(w, x1, y1, x2, y2);
}

__global__ __launch_bounds__(BLOCK) void motion_mono_kernel(MonoArgs a) {
    __shared__ int wsum[WAVES];
    __shared__ int hist[256];
    __shared__ int cvalid[CAND];
    __shared__ int cnt[4];
    __shared__ int pose_ok;
    __shared__ unsigned long long best;
    __shared__ double pose[21];
    __shared__ float cur[12];
    const MonoJob& J = a.jobs[blockIdx.x];
    const int nf = J.n_from, nt = J.n_to, tid = threadIdx.x;
    const int64_t first_from = J.first_from, first_to = J.first_to;
    if (tid < 12) cur[tid] = 0.0f;
    if (tid < 4) cnt[tid] = 0;
    if (tid == 0) { pose_ok = 0; best = 0ull; }
    uint32_t* scratch = a.scratch + (size_t)SCRATCH_WORDS * first_to;
    float* gx = reinterpret_cast<float*>(scratch);                     // [planes][nt]
    float* values = gx + (size_t)MAX_PLANES * nt;
    int32_t* sets = reinterpret_cast<int32_t*>(scratch) + (size_t)(MAX_PLANES + 1) * nt;
    int32_t* out_matches = a.out_matches ? a.out_matches + first_to : reinterpret_cast<int32_t*>(scratch) + (size_t)(MAX_PLANES + 3) * nt;
    float* pts = gx + (size_t)(MAX_PLANES + 4) * nt;                   // [3][nt]
    int32_t* usable = reinterpret_cast<int32_t*>(scratch) + (size_t)(MAX_PLANES + 7) * nt;
    uint32_t* keys = scratch + (size_t)(MAX_PLANES + 8) * nt;
    const bool has3 = a.planes == MAX_PLANES;
    const float fx = J.fx, fy = J.fy, cx = J.cx, cy = J.cy;

    int status = mono::ST_FEW_FEATURES, m = 0, n_inliers = 0;
    float scale = 1.0f, variance = 1.0f;
    float T[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) T[k] = 0.0f;
    Group b;
    b.tid = tid; b.prev = sets; b.next = sets + nt; b.n_prev = b.n_next = b.n_last = 0;

    if (nf >= a.min_inliers && nt >= a.min_inliers) {                  // RegistrationVis.cpp:1594
        // ---- (a) pairs: uMultimapToMapUnique on both sides, then EpipolarGeometry::findPairs
        m = join_compact<MAX_PLANES>(mono_smem, a.p_max, a.from_ids + first_from, nf, a.to_ids + first_to, nt, a.planes, out_matches, gx, wsum,
                                     [&](uint32_t row_t, uint32_t row_f, float* c) __attribute__((always_inline)) {
            if (a.to_ids[first_to + (int64_t)row_t] < 0) return false;
            const float* pf = a.from_points + (first_from + (int64_t)row_f) * 2;
            const float* pt = a.to_points + (first_to + (int64_t)row_t) * 2;
            c[0] = mono::normalised(pf[0], cx, fx); c[1] = mono::normalised(pf[1], cy, fy);
            c[2] = mono::normalised(pt[0], cx, fx); c[3] = mono::normalised(pt[1], cy, fy);
            if (has3) {
                const float* p3 = a.from_points3 + (first_from + (int64_t)row_f) * 3;
                c[4] = p3[0]; c[5] = p3[1]; c[6] = p3[2];
            }
            return true;
        });
        b.init(m, mono_smem + WS_BYTES, 1, wsum, nullptr, hist, &best, cur, sets, gx, a.planes, nt, a.stage_cap);
        const float* X = b.X;
        const int stride = b.stride;
        float* models = b.models;
        auto at = [&](int plane, int i) __attribute__((always_inline)) { return X[plane * stride + i]; };

        status = mono::ST_FEW_PAIRS;
        if (m >= mono::MIN_PAIRS) {
            // ---- (b) the candidates
            const int lane = tid & 63, wave = tid >> 6;
            const int slot = lane < SOLVERS_PER_WAVE ? wave * SOLVERS_PER_WAVE + lane : -1;
            LdsWs w;
            w.p = reinterpret_cast<double*>(mono_smem) + (slot < 0 ? 0 : slot);
            const float thr2 = J.thr2;
            const uint32_t seed = a.seed;
            for (int h0 = 0; h0 < a.iterations; h0 += HYP) {
                if (slot >= 0) {
                    const int h = h0 + slot;
                    const int n = h < a.iterations ? solve_hypothesis(w, seed, (uint32_t)h, m, at) : 0;
#pragma unroll 1
                    for (int r = 0; r < mono::ROOTS; ++r) {
                        double E[9];
                        const bool ok = r < n && mono::model(w, r, E);
                        cvalid[slot * mono::ROOTS + r] = ok ? 1 : 0;
                        if (ok) {
#pragma unroll
                            for (int k = 0; k < 9; ++k) models[(slot * mono::ROOTS + r) * 9 + k] = (float)E[k];
                        }
                    }
                }
                __syncthreads();
                const int nc = min(HYP, a.iterations - h0) * mono::ROOTS;
                for (int j = wave; j < nc; j += WAVES) {
                    if (!cvalid[j]) continue;
                    float e[9];
#pragma unroll
                    for (int k = 0; k < 9; ++k) e[k] = models[j * 9 + k];
                    uint32_t count = 0;
                    for (int i0 = 0; i0 < m; i0 += 64) {
                        const int i = i0 + lane;
                        const bool in = i < m && mono::is_inlier(e, X[i], X[stride + i], X[2 * stride + i], X[3 * stride + i], thr2);
                        count += (uint32_t)__popcll(__ballot(in));
                    }
                    if (lane == 0 && count > 0) atomicMax(&best, ((unsigned long long)count << 32) | (uint32_t)~(uint32_t)(h0 * mono::ROOTS + j));
                }
                __syncthreads();
            }
            const unsigned long long key = best;
            status = mono::ST_NO_MODEL;
            if (key != 0) {
                // ---- (c) the winner again, in fp64, and its decomposition
                if (tid == 0) {
                    const uint32_t c = ~(uint32_t)key;
                    const uint32_t h = c / (uint32_t)mono::ROOTS;
                    const int r = (int)(c - h * (uint32_t)mono::ROOTS);
                    double E[9], P[21];
                    (void)solve_hypothesis(w, seed, h, m, at);
                    (void)mono::model(w, r, E);
#pragma unroll
                    for (int k = 0; k < 9; ++k) cur[k] = (float)E[k];
                    pose_ok = mono::decompose(E, P) ? 1 : 0;
#pragma unroll
                    for (int k = 0; k < 21; ++k) pose[k] = P[k];
                }
                __syncthreads();
                if (pose_ok) {
                    float e[9];
                    double P[21];
#pragma unroll
                    for (int k = 0; k < 9; ++k) e[k] = cur[k];
#pragma unroll
                    for (int k = 0; k < 21; ++k) P[k] = pose[k];
                    const double dist = a.distance;
                    for (int i = tid; i < m; i += BLOCK) {
                        if (!mono::is_inlier(e, X[i], X[stride + i], X[2 * stride + i], X[3 * stride + i], thr2)) continue;
#pragma unroll 1
                        for (int k = 0; k < 4; ++k) {
                            double d1;
                            if (mono::config_test(P, k, X[i], X[stride + i], X[2 * stride + i], X[3 * stride + i], dist, d1)) atomicAdd(&cnt[k], 1);
                        }
                    }
                    __syncthreads();
                    const int cfg = mono::choose_config(cnt[0], cnt[1], cnt[2], cnt[3]);
                    n_inliers = b.select(values, [&](int i, float& v) __attribute__((always_inline)) {
                        v = 0.0f;
                        double d1;
                        return mono::is_inlier(e, X[i], X[stride + i], X[2 * stride + i], X[3 * stride + i], thr2) &&
                               mono::config_test(P, cfg, X[i], X[stride + i], X[2 * stride + i], X[3 * stride + i], dist, d1);
                    });
                    b.swap_sets();
                    for (int j = tid; j < n_inliers; j += BLOCK) {
                        const int i = b.prev[j];
                        double d1;
                        (void)mono::config_test(P, cfg, X[i], X[stride + i], X[2 * stride + i], X[3 * stride + i], dist, d1);
                        float p[3];
                        mono::point_of(d1, X[i], X[stride + i], J.local, p);
                        pts[j] = p[0]; pts[nt + j] = p[1]; pts[2 * nt + j] = p[2];
                    }
                    mono::camera_transform(P, cfg, J.local, T);
                    __syncthreads();                                   // the points are read by other threads

                    // ---- (d) the scale and the variance (util3d_features.cpp:304-408)
                    const bool has_guess = J.has_guess != 0;
                    if (has_guess) scale = mono::norm3(J.guess_t[0], J.guess_t[1], J.guess_t[2]) / mono::norm3(T[3], T[7], T[11]);
                    if (has3) {
                        int n_use = 0;
                        for (int base = 0; base < n_inliers; base += BLOCK) {
                            const int j = base + tid;
                            bool in = false;
                            if (j < n_inliers) {
                                const int i = b.prev[j];
                                const float p[3] = {pts[j], pts[nt + j], pts[2 * nt + j]};
                                const float g[3] = {X[4 * stride + i], X[5 * stride + i], X[6 * stride + i]};
                                in = mono::usable(p, g);
                            }
                            int total;
                            const int pos = n_use + block_rank(in, wsum, total);
                            if (in) usable[pos] = j;
                            n_use += total;
                        }
                        __syncthreads();
                        if (n_use > 0) {
                            const int rank = mono::median_rank(n_use, a.ratio);
                            const int rounds = has_guess ? 1 : n_use;
#pragma unroll 1
                            for (int c = 0; c < rounds; ++c) {
                                float s = scale;
                                if (!has_guess) {
                                    const int jc = usable[c];
                                    s = X[4 * stride + b.prev[jc]] / pts[jc];  // "using x as depth" (:337)
                                }
                                for (int q = tid; q < n_use; q += BLOCK) {
                                    const int j = usable[q], i = b.prev[j];
                                    const float p[3] = {pts[j], pts[nt + j], pts[2 * nt + j]};
                                    const float g[3] = {X[4 * stride + i], X[5 * stride + i], X[6 * stride + i]};
                                    keys[q] = mono::order_key(mono::scaled_error(p, g, s));
                                }
                                const float var = mono::variance_of(mono::key_value(b.ranked(keys, n_use, rank)));
                                if (has_guess || c == 0 || var < variance) { variance = var; scale = s; }
                            }
                        }
                    }
                    if (scale != 1.0f) {                               // :384-402
                        T[3] = T[3] * scale; T[7] = T[7] * scale; T[11] = T[11] * scale;
                        for (int j = tid; j < n_inliers; j += BLOCK) {
                            const float x = pts[j], y = pts[nt + j], z = pts[2 * nt + j];
                            if (m3d::finite(x) && m3d::finite(y) && m3d::finite(z)) { pts[j] = x * scale; pts[nt + j] = y * scale; pts[2 * nt + j] = z * scale; }
                        }
                    }
                    // the two gates of RegistrationVis.cpp:1636-1667
                    status = n_inliers < a.min_inliers ? mono::ST_FEW_INLIERS : ((double)variance <= (double)a.max_variance ? mono::ST_OK : mono::ST_HIGH_VARIANCE);
                }
            }
        }
    } else {
        for (int i = tid; i < nt; i += BLOCK) out_matches[i] = 0;
    }
    __syncthreads();

    // ---- (e) outputs
    if (a.out_inliers) b.write_inliers(a.out_inliers + first_to, out_matches, nt, n_inliers);
    if (a.out_points3) {
        float* o = a.out_points3 + (size_t)first_to * 3;
        for (int j = tid; j < nt; j += BLOCK) {
            const bool in = j < n_inliers;
            o[3 * j] = in ? pts[j] : 0.0f; o[3 * j + 1] = in ? pts[nt + j] : 0.0f; o[3 * j + 2] = in ? pts[2 * nt + j] : 0.0f;
        }
    }
    if (tid == 0) {
        float* t = a.out_transform + (size_t)blockIdx.x * 12;
#pragma unroll
        for (int k = 0; k < 12; ++k) t[k] = status == mono::ST_OK ? T[k] : 0.0f;
        a.out_status[blockIdx.x] = status;
        a.out_n_matches[blockIdx.x] = m;
        a.out_n_inliers[blockIdx.x] = n_inliers;
        a.out_variance[blockIdx.x] = (double)variance;
    }
}

const float IDENTITY[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};

}  // namespace
}  // namespace lcd

using namespace lcd;

namespace {

int estimate_motion_mono(lcd_engine* h, const lcd_motion_mono_args* a, bool on_device) {
    const char* who = on_device ? "lcd_estimate_motion_mono_dev" : "lcd_estimate_motion_mono";
    auto bad = [&](int code, const char* what) { return h->fail(code, std::string(who) + ": " + what); };
    // ---- everything that can be refused is refused before anything is enqueued or written
    if (!a || a->struct_size != (int32_t)sizeof(lcd_motion_mono_args)) return bad(LCD_ERR_INVALID, "null arguments or wrong struct_size");
    if (a->iterations < 1) return bad(LCD_ERR_INVALID, "iterations is >= 1");
    if (a->iterations > 65535) return bad(LCD_ERR_UNSUPPORTED, "more than 65535 iterations");
    if (!std::isfinite(a->reproj_threshold) || !(a->reproj_threshold > 0.0)) return bad(LCD_ERR_INVALID, "reproj_threshold is finite and > 0");
    if (!std::isfinite(a->distance_threshold) || !(a->distance_threshold > 0.0)) return bad(LCD_ERR_INVALID, "distance_threshold is finite and > 0");
    if (a->min_inliers < 1) return bad(LCD_ERR_INVALID, "min_inliers is >= 1");
    if (a->variance_median_ratio < 0 || a->variance_median_ratio > 31) return bad(LCD_ERR_INVALID, "variance_median_ratio is a shift of 0 .. 31");
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
        if (!std::isfinite(c.fx) || !std::isfinite(c.fy) || c.fx == 0.0f || c.fy == 0.0f || !std::isfinite(c.cx) || !std::isfinite(c.cy))
            return bad(LCD_ERR_INVALID, "a camera whose fx or fy is 0 or whose fx, fy, cx or cy is not finite");
        const float t2 = mono::threshold2(a->reproj_threshold, c.fx, c.fy);
        if (!(t2 > 0.0f) || !std::isfinite(t2)) return bad(LCD_ERR_INVALID, "a camera under which the squared normalised threshold is not finite and > 0 as a float");
    }
    const int64_t Nf = fo[np], Nt = to[np];
    if (!a->out_transform || !a->out_status || !a->out_n_matches || !a->out_n_inliers || !a->out_variance) return bad(LCD_ERR_INVALID, "a null per-pair output");
    if (Nf > 0 && (!a->from_word_ids || !a->from_points)) return bad(LCD_ERR_INVALID, "null from-arrays");
    if (Nt > 0 && (!a->to_word_ids || !a->to_points)) return bad(LCD_ERR_INVALID, "null to-arrays");

    StatelessScratch& S = h->pairs;
    hipStream_t st = h->stream;
    const bool has3 = a->from_points3 != nullptr;
    std::vector<MonoJob> jobs((size_t)np);
    for (int i = 0; i < np; ++i) {
        const lcd_camera& c = a->cameras[i];
        MonoJob& j = jobs[(size_t)i];
        j.first_from = fo[i]; j.first_to = to[i]; j.n_from = (int32_t)(fo[i + 1] - fo[i]); j.n_to = (int32_t)(to[i + 1] - to[i]);
        j.fx = c.fx; j.fy = c.fy; j.cx = c.cx; j.cy = c.cy;
        j.thr2 = mono::threshold2(a->reproj_threshold, c.fx, c.fy);
        const float* g = a->guesses ? a->guesses + (size_t)12 * i : nullptr;
        j.has_guess = g && !mono::guess_is_null(g) ? 1 : 0;
        j.guess_t[0] = j.has_guess ? g[3] : 0.0f; j.guess_t[1] = j.has_guess ? g[7] : 0.0f; j.guess_t[2] = j.has_guess ? g[11] : 0.0f;
        for (int k = 0; k < 12; ++k) j.local[k] = c.has_local_transform ? c.local_transform[k] : IDENTITY[k];
        j.pad = 0;
    }

    MonoArgs g;
    g.min_inliers = a->min_inliers; g.iterations = a->iterations; g.ratio = a->variance_median_ratio; g.seed = a->seed;
    g.max_variance = a->max_variance; g.distance = a->distance_threshold;
    g.planes = has3 ? MAX_PLANES : 4;
    const GroupPlan plan = group_plan(n_max, m_max, FIXED_BYTES, (size_t)g.planes * 4);
    g.p_max = plan.p_max; g.stage_cap = plan.stage_cap;
    g.from_ids = a->from_word_ids; g.from_points = a->from_points; g.from_points3 = a->from_points3; g.to_ids = a->to_word_ids; g.to_points = a->to_points;
    g.out_transform = a->out_transform; g.out_status = a->out_status; g.out_n_matches = a->out_n_matches; g.out_n_inliers = a->out_n_inliers;
    g.out_variance = a->out_variance; g.out_matches = a->out_matches; g.out_inliers = a->out_inliers; g.out_points3 = a->out_points3;

    // ---- host entry: everything to the device, results back at the end (one synchronisation)
    HostStage stage(S, host_row_bytes(h), (size_t)h->row_bytes, on_device);
    stage.in(g.from_ids, (size_t)Nf * 4); stage.in(g.from_points, (size_t)Nf * 8);
    stage.in(g.from_points3, (size_t)Nf * 12);                         // optional: null stays null
    stage.in(g.to_ids, (size_t)Nt * 4); stage.in(g.to_points, (size_t)Nt * 8);
    stage.out(g.out_transform, (size_t)np * 48); stage.out(g.out_status, (size_t)np * 4);
    stage.out(g.out_n_matches, (size_t)np * 4); stage.out(g.out_n_inliers, (size_t)np * 4);
    stage.out(g.out_variance, (size_t)np * 8);
    stage.out(g.out_matches, (size_t)Nt * 4); stage.out(g.out_inliers, (size_t)Nt * 4); stage.out(g.out_points3, (size_t)Nt * 12);
    LCD_HIP(h, stage.commit(st, &h->bytes_device));
    LCD_HIP(h, dreserve(h, S.d_small, (size_t)std::max<int64_t>(Nt, 1) * SCRATCH_WORDS * 4));
    g.scratch = S.d_small.as<uint32_t>();
    LCD_HIP(h, S.upload_table(&g.jobs, st, &h->bytes_device, jobs.data(), jobs.size() * sizeof(MonoJob)));
    allow_large_lds<&motion_mono_kernel>();
    motion_mono_kernel<<<dim3((unsigned)np), dim3(BLOCK), plan.lds, st>>>(g);
    LCD_HIP(h, hipGetLastError());
    LCD_HIP(h, stage.finish(st));
    return LCD_OK;
}

}  // namespace

extern "C" {

int lcd_estimate_motion_mono(lcd_engine* h, const lcd_motion_mono_args* a) { return stateless_entry(h, "lcd_estimate_motion_mono", estimate_motion_mono, a, false); }
int lcd_estimate_motion_mono_dev(lcd_engine* h, const lcd_motion_mono_args* a) { return stateless_entry(h, "lcd_estimate_motion_mono", estimate_motion_mono, a, true); }

}  // extern "C"
