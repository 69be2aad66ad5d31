// epipolar.hip -- lcd_verify_epipolar and its _dev form: EpipolarGeometry::check (reference EpipolarGeometry.cpp:65-102, :298-379, EpipolarGeometry.h:158-186)
// for a caller who holds both signatures' word ids and keypoints in device memory.  The rule is include/lcd.h's; its arithmetic is
// epipolar_rule.h's, compiled here for the device and in host/EpipolarGeometryHip.cpp for the mirror.
//   epipolar_kernel: one launch per call, one workgroup of 256 threads per pair, in phases behind barriers.  The phases' machinery is
//   motion_group.cuh's, shared with motion_3d.hip and motion_pnp.hip; what is written here is what the epipolar rule puts into it:
//     (a) join (join_compact): the to-frame's ids are walked, a negative id is refused, the four coordinate planes (from u, v, to u', v') go to
//         the call's scratch and, when they fit beside the candidates, into LDS (Group::init).
//     (b) the two normalisations: the centroids' four sums, then the two sums of the distances, 256 lane partials and the halving tree (Group::tree).
//     (c) candidates in chunks of 256 (Group::ransac): candidate 3 h + r is hypothesis h's r-th root, the seven-point solver per lane with the
//         7 x 9 matrix in registers (epipolar_rule.h: no private segment, profiles/epipolar.txt); an inlier is epi::is_inlier.
//     (d) the winner's inliers compacted in correspondence order (Group::select), then the outputs.
// Nothing of the engine is read or written: the job table is StatelessScratch's, the per-row scratch its d_small.
#include "motion_group.cuh"
#include "epipolar_rule.h"

#include <cmath>
#include <vector>

static_assert(sizeof(lcd_epipolar_args) == 128, "lcd_epipolar_args: the layout include/lcd.h documents (LP64)");
static_assert(LCD_EPI_OK == lcd::epi::ST_OK && LCD_EPI_FEW_PAIRS == lcd::epi::ST_FEW_PAIRS && LCD_EPI_NO_MODEL == lcd::epi::ST_NO_MODEL &&
              LCD_EPI_FEW_INLIERS == lcd::epi::ST_FEW_INLIERS, "lcd_epipolar_status");
static_assert(LCD_EPI_BISECT == lcd::epi::BISECT, "the count include/lcd.h documents");

namespace lcd {
namespace {

constexpr size_t FIXED_BYTES = group_fixed_bytes(epi::SUMS);
constexpr int PLANES = 4;
constexpr int SCRATCH_WORDS = PLANES + 4;                                // per to-row: the coordinate planes, the selection's values, two index sets, the ids when out_matches is NULL

struct EpiJob {
    int64_t first_from, first_to;            // the pair's first row in the from- / to-arrays
    int32_t n_from, n_to;
};
static_assert(sizeof(EpiJob) == 24, "the job table");

struct EpiArgs {
    const EpiJob* jobs;
    int match_count_min, iterations;
    uint32_t seed;
    float thr2;                              // float(thr) x float(thr)
    int p_max;                               // keys per side the LDS carve holds (a power of two >= every frame)
    int stage_cap;                           // correspondences whose coordinates fit the carve behind the fixed part
    const int32_t* from_ids; const float* from_points; const int32_t* to_ids; const float* to_points;
    uint32_t* scratch;                       // [SCRATCH_WORDS x Nt] words; a pair's part starts at SCRATCH_WORDS x first_to
    float* out_fundamental; int32_t* out_status; int32_t* out_n_pairs; int32_t* out_n_inliers; int32_t* out_matches; int32_t* out_inliers;
};

extern __shared__ __attribute__((aligned(16))) unsigned char epi_smem[];

__global__ __launch_bounds__(BLOCK) void epipolar_kernel(EpiArgs a) {
    __shared__ int wsum[WAVES];
    __shared__ int valid[BLOCK];
    __shared__ unsigned long long best;
    __shared__ float cur[12];
    const EpiJob& J = a.jobs[blockIdx.x];
    const int nf = J.n_from, nt = J.n_to, tid = threadIdx.x;
    const int64_t first_from = J.first_from, first_to = J.first_to;
    if (tid < 12) cur[tid] = 0.0f;
    uint32_t* scratch = a.scratch + (size_t)SCRATCH_WORDS * first_to;
    float* gx = reinterpret_cast<float*>(scratch);                     // [PLANES][nt]
    float* values = gx + (size_t)PLANES * nt;
    int32_t* sets = reinterpret_cast<int32_t*>(scratch) + (size_t)(PLANES + 1) * nt;
    int32_t* out_matches = a.out_matches ? a.out_matches + first_to : reinterpret_cast<int32_t*>(scratch) + (size_t)(PLANES + 3) * nt;

    // ---- (a) pairs: findPairsUnique with ignoreNegativeIds (EpipolarGeometry.h:158-186)
    const int m = join_compact<PLANES>(epi_smem, a.p_max, a.from_ids + first_from, nf, a.to_ids + first_to, nt, PLANES, out_matches, gx, wsum,
                                       [&](uint32_t row_t, uint32_t row_f, float* c) __attribute__((always_inline)) {
        if (a.to_ids[first_to + (int64_t)row_t] < 0) return false;
        const float* pf = a.from_points + (first_from + (int64_t)row_f) * 2;
        const float* pt = a.to_points + (first_to + (int64_t)row_t) * 2;
        c[0] = pf[0]; c[1] = pf[1]; c[2] = pt[0]; c[3] = pt[1];
        return true;
    });

    Group b;
    b.init(m, epi_smem, epi::SUMS, wsum, valid, nullptr, &best, cur, sets, gx, PLANES, nt, a.stage_cap);
    const float* X = b.X;
    const int stride = b.stride;

    int status = epi::ST_FEW_PAIRS, n_inliers = 0;
    if (m >= a.match_count_min && m >= epi::MIN_PAIRS) {
        // ---- (b) the normalisations
        float part[epi::SUMS];
#pragma unroll
        for (int c = 0; c < epi::SUMS; ++c) part[c] = 0.0f;
        for (int i = tid; i < m; i += BLOCK) {
#pragma unroll
            for (int c = 0; c < PLANES; ++c) part[c] = part[c] + X[c * stride + i];
        }
        b.tree<epi::SUMS>(part);
        float cfx, cfy, ctx, cty;
        epi::centroid(b.red[0], b.red[BLOCK], m, cfx, cfy);
        epi::centroid(b.red[2 * BLOCK], b.red[3 * BLOCK], m, ctx, cty);
        __syncthreads();                                               // red is read
        float dist[2] = {0.0f, 0.0f};
        for (int i = tid; i < m; i += BLOCK) {
            const float df = epi::distance(X[i], X[stride + i], cfx, cfy), dt = epi::distance(X[2 * stride + i], X[3 * stride + i], ctx, cty);
            dist[0] = dist[0] + df;
            dist[1] = dist[1] + dt;
        }
        b.tree<2>(dist);
        epi::Norm norm_f, norm_t;
        const bool ok_f = epi::normalisation(cfx, cfy, b.red[0], m, norm_f), ok_t = epi::normalisation(ctx, cty, b.red[BLOCK], m, norm_t);
        __syncthreads();                                               // red is read
        status = epi::ST_NO_MODEL;
        if (ok_f && ok_t) {
            // ---- (c) the candidates
            const uint32_t seed = a.seed;
            const float thr2 = a.thr2;
            const unsigned long long key = b.ransac(3 * a.iterations,
                [&](uint32_t c, float* model) __attribute__((always_inline)) {
                    return epi::candidate(seed, c, m, norm_f, norm_t, [&](int plane, int i) __attribute__((always_inline)) { return X[plane * stride + i]; }, model);
                },
                [&](const float* w, int i) __attribute__((always_inline)) { return epi::is_inlier(w, X[i], X[stride + i], X[2 * stride + i], X[3 * stride + i], thr2); });
            if (key != 0) {
                // ---- (d) the winner's inliers, in correspondence order
                float w[12];
#pragma unroll
                for (int k = 0; k < 12; ++k) w[k] = cur[k];
                n_inliers = b.select(values, [&](int i, float& e) __attribute__((always_inline)) {
                    e = 0.0f;
                    return epi::is_inlier(w, X[i], X[stride + i], X[2 * stride + i], X[3 * stride + i], thr2);
                });
                b.swap_sets();
                status = n_inliers >= a.match_count_min ? epi::ST_OK : epi::ST_FEW_INLIERS;
            }
        }
    }

    // ---- outputs
    if (a.out_inliers) b.write_inliers(a.out_inliers + first_to, out_matches, nt, n_inliers);
    if (tid == 0) {
        if (a.out_fundamental) {
            float* f = a.out_fundamental + (size_t)blockIdx.x * 9;
            float unit[9];
            if (n_inliers > 0) {
                float w[12];
#pragma unroll
                for (int k = 0; k < 12; ++k) w[k] = cur[k];
                epi::unit_matrix(w, unit);
            } else {
#pragma unroll
                for (int k = 0; k < 9; ++k) unit[k] = 0.0f;
            }
#pragma unroll
            for (int k = 0; k < 9; ++k) f[k] = unit[k];
        }
        a.out_status[blockIdx.x] = status;
        a.out_n_pairs[blockIdx.x] = m;
        a.out_n_inliers[blockIdx.x] = n_inliers;
    }
}

}  // namespace
}  // namespace lcd

using namespace lcd;

namespace {

int verify_epipolar(lcd_engine* h, const lcd_epipolar_args* a, bool on_device) {
    const char* who = on_device ? "lcd_verify_epipolar_dev" : "lcd_verify_epipolar";
    auto bad = [&](int code, const char* what) { return h->fail(code, std::string(who) + ": " + what); };
    // ---- everything that can be refused is refused before anything is enqueued or written
    if (!a || a->struct_size != (int32_t)sizeof(lcd_epipolar_args)) return bad(LCD_ERR_INVALID, "null arguments or wrong struct_size");
    if (a->iterations < 1) return bad(LCD_ERR_INVALID, "iterations is >= 1");
    if (a->iterations > 65535) return bad(LCD_ERR_UNSUPPORTED, "more than 65535 iterations");
    const float thr = (float)a->ransac_threshold;
    const float thr2 = thr * thr;
    if (!std::isfinite(a->ransac_threshold) || !(thr > 0.0f) || !std::isfinite(thr) || !(thr2 > 0.0f) || !std::isfinite(thr2))
        return bad(LCD_ERR_INVALID, "ransac_threshold is finite and > 0, as a float and squared too");
    if (a->match_count_min < 1) return bad(LCD_ERR_INVALID, "match_count_min is >= 1");
    if (const int rc = refuse_pairs(h, a->n_pairs, bad)) return rc;
    if (a->n_pairs == 0) return LCD_OK;
    const int np = a->n_pairs;
    const int64_t* fo = a->from_offsets;
    const int64_t* to = a->to_offsets;
    int n_max, m_max;
    if (const int rc = refuse_offsets(np, fo, to, bad, n_max, m_max)) return rc;
    const int64_t Nf = fo[np], Nt = to[np];
    if (!a->out_status || !a->out_n_pairs || !a->out_n_inliers) return bad(LCD_ERR_INVALID, "a null per-pair output");
    if (Nf > 0 && (!a->from_word_ids || !a->from_points)) return bad(LCD_ERR_INVALID, "null from-arrays");
    if (Nt > 0 && (!a->to_word_ids || !a->to_points)) return bad(LCD_ERR_INVALID, "null to-arrays");

    StatelessScratch& S = h->pairs;
    hipStream_t st = h->stream;
    std::vector<EpiJob> jobs((size_t)np);
    for (int i = 0; i < np; ++i) {
        EpiJob& j = jobs[(size_t)i];
        j.first_from = fo[i]; j.first_to = to[i]; j.n_from = (int32_t)(fo[i + 1] - fo[i]); j.n_to = (int32_t)(to[i + 1] - to[i]);
    }

    EpiArgs g;
    g.match_count_min = a->match_count_min; g.iterations = a->iterations; g.seed = a->seed; g.thr2 = thr2;
    const GroupPlan plan = group_plan(n_max, m_max, FIXED_BYTES, (size_t)PLANES * 4);
    g.p_max = plan.p_max; g.stage_cap = plan.stage_cap;
    g.from_ids = a->from_word_ids; g.from_points = a->from_points; g.to_ids = a->to_word_ids; g.to_points = a->to_points;
    g.out_fundamental = a->out_fundamental; g.out_status = a->out_status; g.out_n_pairs = a->out_n_pairs; g.out_n_inliers = a->out_n_inliers;
    g.out_matches = a->out_matches; g.out_inliers = a->out_inliers;

    // ---- host entry: everything to the device, results back at the end (one synchronisation)
    HostStage stage(S, host_row_bytes(h), (size_t)h->row_bytes, on_device);
    stage.in(g.from_ids, (size_t)Nf * 4); stage.in(g.from_points, (size_t)Nf * 8);
    stage.in(g.to_ids, (size_t)Nt * 4); stage.in(g.to_points, (size_t)Nt * 8);
    stage.out(g.out_fundamental, (size_t)np * 36);                     // optional: null stays null
    stage.out(g.out_status, (size_t)np * 4); stage.out(g.out_n_pairs, (size_t)np * 4); stage.out(g.out_n_inliers, (size_t)np * 4);
    stage.out(g.out_matches, (size_t)Nt * 4); stage.out(g.out_inliers, (size_t)Nt * 4);
    LCD_HIP(h, stage.commit(st, &h->bytes_device));
    LCD_HIP(h, dreserve(h, S.d_small, (size_t)std::max<int64_t>(Nt, 1) * SCRATCH_WORDS * 4));
    g.scratch = S.d_small.as<uint32_t>();
    LCD_HIP(h, S.upload_table(&g.jobs, st, &h->bytes_device, jobs.data(), jobs.size() * sizeof(EpiJob)));
    allow_large_lds<&epipolar_kernel>();
    epipolar_kernel<<<dim3((unsigned)np), dim3(BLOCK), plan.lds, st>>>(g);
    LCD_HIP(h, hipGetLastError());
    LCD_HIP(h, stage.finish(st));
    return LCD_OK;
}

}  // namespace

extern "C" {

int lcd_verify_epipolar(lcd_engine* h, const lcd_epipolar_args* a) { return stateless_entry(h, "lcd_verify_epipolar", verify_epipolar, a, false); }
int lcd_verify_epipolar_dev(lcd_engine* h, const lcd_epipolar_args* a) { return stateless_entry(h, "lcd_verify_epipolar", verify_epipolar, a, true); }

}  // extern "C"
