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
    IcpOutputs out;
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
    b.thr2 = a.thr2; b.raw_from = raw_from; b.out_match = a.out.out_match + J.first_from;
    b.from.carve(a.scratch + (size_t)SCRATCH_WORDS * J.first_from, nf, mask_f);
    b.to.carve(a.scratch + (size_t)SCRATCH_WORDS * (a.n_from_all + J.first_to), nt, mask_t);

    // ---- (a) the rows that take part, Q and P_0
    mask_f[tid] = 0u; mask_t[tid] = 0u;
    __syncthreads();
    auto nothing = [](int) __attribute__((always_inline)) {};
    b.load_rows(raw_to, J.guess, mask_f, mask_t, nothing, nothing);
    b.np_from = b.np_to = 0;
    for (int w = 0; w < MASK_WORDS; ++w) { b.np_from += __popc(mask_f[w]); b.np_to += __popc(mask_t[w]); }

    // ---- (b) .. (d): the rule's own control flow, Q staged for the loop
    b.stage(false);
    icp::Result r;
    icp::solve(b, a.max_iterations, a.force_3dof != 0, a.max_laser_scans, a.epsilon, a.correspondence_ratio, J.guess, r);

    // ---- (e) outputs
    if (tid == 0) write_result(a.out, blockIdx.x, r);
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
    double thr2;
    if (const int rc = refuse_icp_params(a, bad, &thr2)) return rc;
    IcpPairs c;
    if (const int rc = refuse_icp_pairs(h, a, on_device, bad, IcpOwnArrays{false, false, false, "null from-rows or out_match", "null to-rows"}, c)) return rc;
    if (c.np == 0) return LCD_OK;

    StatelessScratch& S = h->pairs;
    hipStream_t st = h->stream;
    IcpArgs g;
    g.max_iterations = a->max_iterations; g.force_3dof = a->force_3dof; g.max_laser_scans = a->max_laser_scans;
    g.search = a->search; g.cell = icp::cell_size(a->max_correspondence_distance);
    g.epsilon = a->epsilon; g.correspondence_ratio = a->correspondence_ratio; g.thr2 = thr2;
    g.stride = plane_stride(c.n_max); g.n_from_all = c.Nf;
    g.from_xyz = a->from_xyz; g.to_xyz = a->to_xyz; g.out = icp_outputs(a);

    // ---- host entry: everything to the device, results back at the end (one synchronisation)
    HostStage stage(S, host_row_bytes(h), (size_t)h->row_bytes, on_device);
    stage_icp(stage, c, g.from_xyz, g.to_xyz, g.out);
    LCD_HIP(h, stage.commit(st, &h->bytes_device));
    LCD_HIP(h, dreserve(h, S.d_small, (size_t)std::max<int64_t>(c.Nf + c.Nt, 1) * SCRATCH_WORDS * 4));
    g.scratch = S.d_small.as<uint32_t>();
    LCD_HIP(h, S.upload_table(&g.jobs, st, &h->bytes_device, c.jobs.data(), c.jobs.size() * sizeof(IcpJob)));
    allow_large_lds<&register_icp_kernel>();
    register_icp_kernel<<<dim3((unsigned)c.np), dim3(BLOCK), lds_bytes(c.n_max), st>>>(g);
    LCD_HIP(h, hipGetLastError());
    LCD_HIP(h, stage.finish(st));
    return LCD_OK;
}

}  // namespace

extern "C" {

int lcd_register_icp(lcd_engine* h, const lcd_icp_args* a) { return stateless_entry(h, "lcd_register_icp", register_icp, a, false); }
int lcd_register_icp_dev(lcd_engine* h, const lcd_icp_args* a) { return stateless_entry(h, "lcd_register_icp", register_icp, a, true); }

}  // extern "C"
