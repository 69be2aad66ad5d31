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
// Nothing of the engine is read or written: the job table is StatelessScratch's, the per-row scratch its d_small.  The workgroup's backend
// -- (b), the sums of (c) and (d) -- is register_icp_group.cuh's, shared with register_icp_plane.hip.
#include "register_icp_group.cuh"

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
// the carve, every part a multiple of 16 bytes (the target's planes are read 16 bytes at a time): red, hist, the two masks, cur, planes
constexpr size_t OFF_HIST = (size_t)SUMS * BLOCK * 4, OFF_MASK_F = OFF_HIST + 256 * 4, OFF_MASK_T = OFF_MASK_F + MASK_WORDS * 4;
constexpr size_t OFF_CUR = OFF_MASK_T + MASK_WORDS * 4, OFF_PLANES = OFF_CUR + 16 * 4;
static_assert(OFF_PLANES % 16 == 0, "the planes start on a 16-byte boundary");
inline size_t lds_bytes(int n_max) { return OFF_PLANES + std::max((size_t)3 * plane_stride(n_max) * 4, (size_t)key_slots(n_max) * 8); }
static_assert(OFF_PLANES + (size_t)3 * MAX_ROWS * 4 <= LDS_LIMIT && (size_t)(MAX_ROWS + MAX_ROWS / 8) * 8 <= (size_t)3 * MAX_ROWS * 4, "8192 rows of a target fit the carve, as planes and as keys");

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
