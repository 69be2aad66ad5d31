// register_icp_plane.hip -- lcd_register_icp_plane and its _dev form: what RegistrationIcp::computeTransformationImpl does with Icp/PointToPlane
// = true, Icp/Strategy = 0 and 3-D scans that carry normals (reference RegistrationIcp.cpp:506-661 and :785-853; computeNormalsComplexity at
// util3d_surface.cpp:3164-3241, icpPointToPlane at util3d_registration.cpp:451-492, the normal-aware computeVarianceAndCorrespondences at
// :240-301).  The rule is include/lcd.h's; its arithmetic and control flow are icp_plane_rule.h's, compiled here for the device and in
// host/RegistrationIcp.cpp for the mirror.
//   register_icp_plane_kernel: one launch per call, one workgroup of 256 threads per pair, in phases behind barriers.  The staging of a
//   search's target, both search forms, the point-to-point sums, the reciprocal test and the median are register_icp_group.cuh's, shared with
//   register_icp.hip; this file adds
//     (a) the normals: the from-side's as given and the to-side's under the guess's rotation go to the call's scratch by row, three planes a
//         side; one bit a row says whether the given normal is finite.  The target's normals do not fit LDS beside its planes: the thread that
//         found a correspondence reads the one normal it needs from the scratch.
//     (b) the complexity: two 256-lane sums a side (three normal sums, six centred products), the 3 x 3 Jacobi on every thread alike.
//     (c) the decision, then the participation masks of the branch taken (branch 0: coordinates and normal finite) and Q staged.
//     (d) branch 0's fit: the 27 products of a correspondence into 27 rows of lane partials (lane = row mod 256 = the thread that searched
//         it), Group::tree<27>, thread 0 solves the 6 x 6 by LDL^T and hands T over.
//     (e) branch 0's step 5: the rank of a reciprocal correspondence in source-row order by compact_body.cuh's block_rank, the gate per
//         correspondence, and the median over the first `count` of them (the others' keys as all ones).
// LDS at 8 192 rows: 27 KiB of lane partials, 1 KiB of histogram, four masks of 1 KiB, 80 bytes, 96 KiB of planes (or 72 KiB of keys) = about
// 128 KiB of the 144 KiB motion_group.cuh allows.  Nothing of the engine is read or written.
#include "icp_plane_rule.h"
#include "register_icp_group.cuh"

#include <cmath>
#include <vector>

static_assert(sizeof(lcd_icp_plane_args) == 240, "lcd_icp_plane_args: the layout include/lcd.h documents (LP64)");
static_assert(LCD_ICP_PLANE_SWEEPS == lcd::icpp::SWEEPS, "the sweep count include/lcd.h names");
static_assert(LCD_ICP_LOW_COMPLEXITY == lcd::icpp::ST_LOW_COMPLEXITY && LCD_ICP_STOP_SINGULAR == lcd::icpp::STOP_SINGULAR, "lcd_icp_status, lcd_icp_stop");

namespace lcd {
namespace {

constexpr int PLANE_SCRATCH_WORDS = SCRATCH_WORDS + 3;                   // per row of either side: register_icp_group.cuh's five and the normal
// the carve, every part a multiple of 16 bytes: red, hist, the two participation masks, the two normal masks, cur, wsum, planes
constexpr size_t OFF_HIST = (size_t)icpp::SUMS * BLOCK * 4, OFF_MASK_F = OFF_HIST + 256 * 4, OFF_MASK_T = OFF_MASK_F + MASK_WORDS * 4;
constexpr size_t OFF_NMASK_F = OFF_MASK_T + MASK_WORDS * 4, OFF_NMASK_T = OFF_NMASK_F + MASK_WORDS * 4;
constexpr size_t OFF_CUR = OFF_NMASK_T + MASK_WORDS * 4, OFF_WSUM = OFF_CUR + 16 * 4, OFF_PLANES = OFF_WSUM + 4 * 4;
static_assert(OFF_PLANES % 16 == 0 && WAVES == 4, "the planes start on a 16-byte boundary");
inline size_t lds_bytes(int n_max) { return OFF_PLANES + std::max((size_t)3 * plane_stride(n_max) * 4, (size_t)key_slots(n_max) * 8); }
static_assert(OFF_PLANES + (size_t)3 * MAX_ROWS * 4 <= LDS_LIMIT, "8192 rows of a target fit the carve");

struct PlaneArgs {
    const IcpJob* jobs;
    icpp::Params p;
    int search;
    float cell;
    double thr2;
    int stride;
    int64_t n_from_all, n_to_all;
    const float* from_xyz; const float* to_xyz; const float* from_normals; const float* to_normals;
    uint32_t* scratch;                       // [SCRATCH_WORDS x (Nf + Nt)] words, then the normals [3 x (Nf + Nt)]
    IcpOutputs out;
    int32_t* out_branch; float* out_complexity; float* out_complexity_values; float* out_complexity_vectors; float* out_second_eigenvalue;
};

extern __shared__ __attribute__((aligned(16))) unsigned char icpp_smem[];

struct PlaneBackend : GroupBackend {
    uint32_t* pmask_f; uint32_t* pmask_t;    // LDS: from.mask and to.mask, writable
    const uint32_t* nmask_f; const uint32_t* nmask_t;   // LDS: the rows whose given normal is finite
    float* nrm_from; float* nrm_to;          // the scratch: a side's normals as three planes of its rows
    const float* raw_nrm_from;               // the pair's from-normals as given
    int oi_f, oi_t, rows_f, rows_t;

    __device__ __forceinline__ int rows_from() const { return rows_f; }
    __device__ __forceinline__ int rows_to() const { return rows_t; }

    __device__ __forceinline__ int normal_sums(bool to_side, float sum[3]) {
        const int n = to_side ? to.n : from.n;
        const float* nrm = to_side ? nrm_to : nrm_from;
        const uint32_t* nm = to_side ? nmask_t : nmask_f;
        float part[3] = {0.0f, 0.0f, 0.0f};
        for (int i = tid; i < n; i += BLOCK) {
            if (!bit_of(nm, i)) continue;
#pragma unroll
            for (int a = 0; a < 3; ++a) part[a] = part[a] + nrm[(size_t)a * n + i];
        }
        tree<3>(part);
#pragma unroll
        for (int a = 0; a < 3; ++a) sum[a] = red[a * BLOCK];
        __syncthreads();
        return to_side ? oi_t : oi_f;
    }
    __device__ __forceinline__ void normal_cov(bool to_side, const float mean[3], float C[6]) {
        const int n = to_side ? to.n : from.n;
        const float* nrm = to_side ? nrm_to : nrm_from;
        const uint32_t* nm = to_side ? nmask_t : nmask_f;
        float part[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) part[k] = 0.0f;
        for (int i = tid; i < n; i += BLOCK) {
            if (!bit_of(nm, i)) continue;
            const float v[3] = {nrm[i], nrm[(size_t)n + i], nrm[(size_t)2 * n + i]};
            float e[6];
            icpp::cov_terms(v, mean, e);
#pragma unroll
            for (int k = 0; k < 6; ++k) part[k] = part[k] + e[k];
        }
        tree<6>(part);
#pragma unroll
        for (int k = 0; k < 6; ++k) C[k] = red[k * BLOCK];
        __syncthreads();
    }
    __device__ __forceinline__ void participate(bool with_normals) {
        rows_f = rows_t = 0;
        for (int w = 0; w < MASK_WORDS; ++w) { rows_f += __popc(pmask_f[w]); rows_t += __popc(pmask_t[w]); }
        __syncthreads();
        if (with_normals) { pmask_f[tid] &= nmask_f[tid]; pmask_t[tid] &= nmask_t[tid]; }
        __syncthreads();
        np_from = np_to = 0;
        for (int w = 0; w < MASK_WORDS; ++w) { np_from += __popc(pmask_f[w]); np_to += __popc(pmask_t[w]); }
        stage(false);
    }
    __device__ __forceinline__ bool fit_plane(float T[12]) {
        float part[icpp::SUMS];
#pragma unroll
        for (int k = 0; k < icpp::SUMS; ++k) part[k] = 0.0f;
        for (int i = tid; i < from.n; i += BLOCK) {
            const int row = from.nn[i];
            if (!bit_of(from.mask, i) || !icp::corresponds(row, from.d2[i], thr2)) continue;
            float s[3], d[3], nv[3], e[icpp::SUMS];
#pragma unroll
            for (int a = 0; a < 3; ++a) { s[a] = from.xyz[(size_t)a * from.n + i]; d[a] = target(a, row); nv[a] = nrm_to[(size_t)a * to.n + row]; }
            icpp::plane_terms(s, d, nv, e);
#pragma unroll
            for (int k = 0; k < icpp::SUMS; ++k) part[k] = part[k] + e[k];
        }
        tree<icpp::SUMS>(part);
        if (tid == 0) {
            float S[icpp::SUMS], model[12];
#pragma unroll
            for (int k = 0; k < icpp::SUMS; ++k) S[k] = red[k * BLOCK];
#pragma unroll
            for (int k = 0; k < 12; ++k) model[k] = 0.0f;
            const bool ok = icpp::plane_fit(S, model);
#pragma unroll
            for (int k = 0; k < 12; ++k) cur[k] = model[k];
            cur[12] = ok ? 1.0f : 0.0f;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 12; ++k) T[k] = cur[k];
        return cur[12] != 0.0f;
    }
    __device__ __forceinline__ void register_normals(const float F[12]) {
        for (int i = tid; i < from.n; i += BLOCK) {
            float x, y, z;
            icpp::rotate(F, raw_nrm_from[(size_t)3 * i], raw_nrm_from[(size_t)3 * i + 1], raw_nrm_from[(size_t)3 * i + 2], x, y, z);
            nrm_from[i] = x; nrm_from[(size_t)from.n + i] = y; nrm_from[(size_t)2 * from.n + i] = z;
        }
    }
    __device__ __forceinline__ int reciprocal_gated(bool from_is_target, bool gate, double min_cos) {
        auto nothing = [](int, bool, int, float, float, float, float) __attribute__((always_inline)) {};
        search(from, to.n, nothing);                                   // Q is still staged
        stage(true);                                                   // (its first barrier also publishes the registered cloud and its normals)
        search(to, from.n, nothing);
        __syncthreads();
        const Side& src = from_is_target ? to : from;
        const Side& tgt = from_is_target ? from : to;
        const float* nsrc = from_is_target ? nrm_to : nrm_from;
        const float* ntgt = from_is_target ? nrm_from : nrm_to;
        int kept = 0, count = 0;
        for (int base = 0; base < src.n; base += BLOCK) {
            const int i = base + tid;
            bool keep = false, pass = false;
            if (i < src.n) {
                const int row = src.nn[i];
                keep = icp::corresponds(row, src.d2[i], thr2) && tgt.nn[row] == i;
                if (keep) {
                    pass = true;
                    if (gate) {
                        const float v1[3] = {ntgt[row], ntgt[(size_t)tgt.n + row], ntgt[(size_t)2 * tgt.n + row]};
                        const float v2[3] = {nsrc[i], nsrc[(size_t)src.n + i], nsrc[(size_t)2 * src.n + i]};
                        pass = icpp::gate_passes(v1, v2, min_cos);
                    }
                }
                if (from_is_target) { if (pass) out_match[row] = i; }
                else out_match[i] = pass ? row : -1;
            }
            int total;
            const int rank = kept + block_rank(keep, wsum, total);
            if (i < src.n) src.nn[i] = keep ? rank : -1;              // the thread's own row; the test above reads the other side's
            kept += total;
            count += __syncthreads_count(pass);
        }
        uint32_t* k32 = reinterpret_cast<uint32_t*>(src.d2);
        for (int i = tid; i < src.n; i += BLOCK) {
            const int rank = src.nn[i];
            if (rank < 0 || rank >= count) k32[i] = 0xffffffffu;
        }
        keys = k32; n_keys = src.n;
        return count;
    }
    __device__ __forceinline__ float median_first(int n) { return m3d::float_of(ranked(keys, n_keys, n >> 1)); }
};

__global__ __launch_bounds__(BLOCK) void register_icp_plane_kernel(PlaneArgs a) {
    const int tid = threadIdx.x;
    const IcpJob J = a.jobs[blockIdx.x];
    const int nf = J.n_from, nt = J.n_to;
    uint32_t* mask_f = reinterpret_cast<uint32_t*>(icpp_smem + OFF_MASK_F);
    uint32_t* mask_t = reinterpret_cast<uint32_t*>(icpp_smem + OFF_MASK_T);
    uint32_t* nmask_f = reinterpret_cast<uint32_t*>(icpp_smem + OFF_NMASK_F);
    uint32_t* nmask_t = reinterpret_cast<uint32_t*>(icpp_smem + OFF_NMASK_T);
    const float* raw_from = a.from_xyz + J.first_from * 3;
    const float* raw_to = a.to_xyz + J.first_to * 3;
    const float* raw_nf = a.from_normals + J.first_from * 3;
    const float* raw_nt = a.to_normals + J.first_to * 3;
    float* normals = reinterpret_cast<float*>(a.scratch + (size_t)SCRATCH_WORDS * (a.n_from_all + a.n_to_all));

    PlaneBackend b;
    b.tid = tid;
    b.red = reinterpret_cast<float*>(icpp_smem);
    b.hist = reinterpret_cast<int*>(icpp_smem + OFF_HIST);
    b.cur = reinterpret_cast<float*>(icpp_smem + OFF_CUR);
    b.wsum = reinterpret_cast<int*>(icpp_smem + OFF_WSUM);
    b.planes = reinterpret_cast<float*>(icpp_smem + OFF_PLANES); b.stride = a.stride;
    b.keys64 = reinterpret_cast<uint64_t*>(icpp_smem + OFF_PLANES); b.search_mode = a.search; b.cell = a.cell;
    b.thr2 = a.thr2; b.raw_from = raw_from; b.out_match = a.out.out_match + J.first_from;
    b.from.carve(a.scratch + (size_t)SCRATCH_WORDS * J.first_from, nf, mask_f);
    b.to.carve(a.scratch + (size_t)SCRATCH_WORDS * (a.n_from_all + J.first_to), nt, mask_t);
    b.pmask_f = mask_f; b.pmask_t = mask_t; b.nmask_f = nmask_f; b.nmask_t = nmask_t;
    b.nrm_from = normals + (size_t)3 * J.first_from;
    b.nrm_to = normals + (size_t)3 * (a.n_from_all + J.first_to);
    b.raw_nrm_from = raw_nf;

    // ---- (a) the rows with finite coordinates, Q and P_0, the normals
    mask_f[tid] = 0u; mask_t[tid] = 0u; nmask_f[tid] = 0u; nmask_t[tid] = 0u;
    __syncthreads();
    b.load_rows(raw_to, J.guess, mask_f, mask_t,
        [&](int i) __attribute__((always_inline)) {
            const float nx = raw_nf[(size_t)3 * i], ny = raw_nf[(size_t)3 * i + 1], nz = raw_nf[(size_t)3 * i + 2];
            b.nrm_from[i] = nx; b.nrm_from[(size_t)nf + i] = ny; b.nrm_from[(size_t)2 * nf + i] = nz;
            if (icpp::finite3(nx, ny, nz)) atomicOr(&nmask_f[i >> 5], 1u << (i & 31));
        },
        [&](int j) __attribute__((always_inline)) {
            const float nx = raw_nt[(size_t)3 * j], ny = raw_nt[(size_t)3 * j + 1], nz = raw_nt[(size_t)3 * j + 2];
            float rx, ry, rz;
            icpp::rotate(J.guess, nx, ny, nz, rx, ry, rz);
            b.nrm_to[j] = rx; b.nrm_to[(size_t)nt + j] = ry; b.nrm_to[(size_t)2 * nt + j] = rz;
            if (icpp::finite3(nx, ny, nz)) atomicOr(&nmask_t[j >> 5], 1u << (j & 31));
        });
    b.oi_f = b.oi_t = 0;
    for (int w = 0; w < MASK_WORDS; ++w) { b.oi_f += __popc(nmask_f[w]); b.oi_t += __popc(nmask_t[w]); }
    b.np_from = b.np_to = b.rows_f = b.rows_t = 0;

    // ---- (b) .. (e): the rule's own control flow
    icpp::Result r;
    icpp::solve(b, a.p, J.guess, r);

    if (tid == 0) {
        const size_t p = blockIdx.x;
        write_result(a.out, p, r);
        a.out_branch[p] = r.branch;
        a.out_complexity[p] = r.complexity;
#pragma unroll
        for (int k = 0; k < 3; ++k) a.out_complexity_values[p * 3 + k] = r.values[k];
#pragma unroll
        for (int k = 0; k < 9; ++k) a.out_complexity_vectors[p * 9 + k] = r.vectors[k];
        a.out_second_eigenvalue[p] = r.second;
    }
}

}  // namespace
}  // namespace lcd

using namespace lcd;

namespace {

int register_icp_plane(lcd_engine* h, const lcd_icp_plane_args* a, bool on_device) {
    const char* who = on_device ? "lcd_register_icp_plane_dev" : "lcd_register_icp_plane";
    auto bad = [&](int code, const char* what) { return h->fail(code, std::string(who) + ": " + what); };
    // ---- everything that can be refused is refused before anything is enqueued or written
    if (!a || a->struct_size != (int32_t)sizeof(lcd_icp_plane_args)) return bad(LCD_ERR_INVALID, "null arguments or wrong struct_size");
    double thr2;
    if (const int rc = refuse_icp_params(a, bad, &thr2)) return rc;
    if (!(a->min_complexity >= 0.0f) || !(a->min_complexity <= 1.0f)) return bad(LCD_ERR_INVALID, "min_complexity is in [0, 1]");
    if (a->low_complexity_strategy < 0 || a->low_complexity_strategy > 2) return bad(LCD_ERR_INVALID, "low_complexity_strategy is 0, 1 or 2");
    if (a->normal_gate != 0 && !std::isfinite(a->min_normal_cos)) return bad(LCD_ERR_INVALID, "min_normal_cos is finite while the gate is on");
    const IcpOwnArrays own{!a->out_branch || !a->out_complexity || !a->out_complexity_values || !a->out_complexity_vectors || !a->out_second_eigenvalue,
                           !a->from_normals, !a->to_normals, "null from-rows, from-normals or out_match", "null to-rows or to-normals"};
    IcpPairs c;
    if (const int rc = refuse_icp_pairs(h, a, on_device, bad, own, c)) return rc;
    if (c.np == 0) return LCD_OK;
    const size_t np = (size_t)c.np;

    StatelessScratch& S = h->pairs;
    hipStream_t st = h->stream;
    PlaneArgs g;
    g.p.max_iterations = a->max_iterations; g.p.force_3dof = a->force_3dof != 0; g.p.max_laser_scans = a->max_laser_scans;
    g.p.strategy = a->low_complexity_strategy; g.p.gate = a->normal_gate != 0; g.p.min_normal_cos = a->min_normal_cos;
    g.p.epsilon = a->epsilon; g.p.correspondence_ratio = a->correspondence_ratio; g.p.min_complexity = a->min_complexity;
    g.search = a->search; g.cell = icp::cell_size(a->max_correspondence_distance); g.thr2 = thr2;
    g.stride = plane_stride(c.n_max); g.n_from_all = c.Nf; g.n_to_all = c.Nt;
    g.from_xyz = a->from_xyz; g.to_xyz = a->to_xyz; g.from_normals = a->from_normals; g.to_normals = a->to_normals;
    g.out = icp_outputs(a);
    g.out_branch = a->out_branch; g.out_complexity = a->out_complexity; g.out_complexity_values = a->out_complexity_values;
    g.out_complexity_vectors = a->out_complexity_vectors; g.out_second_eigenvalue = a->out_second_eigenvalue;

    // ---- host entry: everything to the device, results back at the end (one synchronisation)
    HostStage stage(S, host_row_bytes(h), (size_t)h->row_bytes, on_device);
    stage_icp(stage, c, g.from_xyz, g.to_xyz, g.out);
    stage.in(g.from_normals, (size_t)c.Nf * 12); stage.in(g.to_normals, (size_t)c.Nt * 12);
    stage.out(g.out_branch, np * 4); stage.out(g.out_complexity, np * 4); stage.out(g.out_complexity_values, np * 12);
    stage.out(g.out_complexity_vectors, np * 36); stage.out(g.out_second_eigenvalue, np * 4);
    LCD_HIP(h, stage.commit(st, &h->bytes_device));
    LCD_HIP(h, dreserve(h, S.d_small, (size_t)std::max<int64_t>(c.Nf + c.Nt, 1) * PLANE_SCRATCH_WORDS * 4));
    g.scratch = S.d_small.as<uint32_t>();
    LCD_HIP(h, S.upload_table(&g.jobs, st, &h->bytes_device, c.jobs.data(), c.jobs.size() * sizeof(IcpJob)));
    allow_large_lds<&register_icp_plane_kernel>();
    register_icp_plane_kernel<<<dim3((unsigned)c.np), dim3(BLOCK), lds_bytes(c.n_max), st>>>(g);
    LCD_HIP(h, hipGetLastError());
    LCD_HIP(h, stage.finish(st));
    return LCD_OK;
}

}  // namespace

extern "C" {

int lcd_register_icp_plane(lcd_engine* h, const lcd_icp_plane_args* a) { return stateless_entry(h, "lcd_register_icp_plane", register_icp_plane, a, false); }
int lcd_register_icp_plane_dev(lcd_engine* h, const lcd_icp_plane_args* a) { return stateless_entry(h, "lcd_register_icp_plane", register_icp_plane, a, true); }

}  // extern "C"
