// scan_filter.hip -- lcd_filter_scans and its _dev form: what util3d::commonFiltering does to a scan in front of the ICP (reference
// RegistrationIcp.cpp:362-447, util3d_filtering.cpp:74-332): downsampling, the range, the voxel grid, the normals and the ground rule.  The rule
// is include/lcd.h's; its arithmetic is scan_filter_rule.h's, compiled here for the device and in host/ScanFilter.cpp for the mirror.
//   scan_voxel_kernel: one workgroup of 256 threads per scan.  Step 1 is a ballot-scan compaction in chunks of 256 rows (block_rank) into the
//   scratch, three planes.  Step 2 reduces the cell bounds, puts the keys voxel index << 32 | row into LDS and sorts them (bitonic_sort: at
//   16 384 keys the 144 KiB feature_select.hip uses); run heads get their rank by block_rank and the head's thread walks its run, which is in
//   ascending row order.  Without normals it also writes the outputs (emit) and the call is this one launch.
//   scan_normals_kernel<KMAX>: one workgroup per (scan, tile of 256 rows of the cloud).  The tile table is sized from the host's upper bound
//   min(n / step, 8192); a tile beyond the device's count returns at once.  A workgroup stages its scan's whole cloud as three planes in
//   LDS (at most 96 KiB, padded with +inf as GroupBackend::stage does) and each thread finds its row's neighbours by brute force over float4s
//   that the whole wave reads alike.  K mode keeps the KMAX smallest keys ascending in registers, fully unrolled (KMAX = 8, 16, 32; the first
//   min(K, |C|) are the neighbours -- a padding row's key is above every real row's); radius mode (KMAX = 0) accumulates as it walks.
//   The Jacobi and the flip run per thread.
//   scan_emit_kernel: one workgroup per scan, steps 4-6: the compaction by block_rank, the ground rule, the NaN padding of the region, the
//   counts and the status.
// The intermediate clouds live in StatelessScratch::d_small (stateless_scratch.h).  Nothing of the engine is read or written.
#include "scan_filter_rule.h"
#include "compact_body.cuh"
#include "motion_group.cuh"

#include <climits>
#include <cmath>
#include <vector>

static_assert(sizeof(lcd_scan_filter_args) == 120, "lcd_scan_filter_args: the layout include/lcd.h documents (LP64)");
static_assert(LCD_SCAN_MAX_K == lcd::scf::MAX_K && LCD_SCAN_NO_ROOM == lcd::scf::ST_NO_ROOM && LCD_SCAN_TOO_MANY_ROWS == lcd::scf::ST_TOO_MANY_ROWS, "lcd_scan_status");

namespace lcd {
namespace {

constexpr int SCAN_PLANES = 9;               // per sampled row in the scratch: step 1's cloud, step 2's cloud, the normals; three planes each
constexpr int HDR_WORDS = 4;                 // per scan: |C|, the status so far, the rows after step 1, the rows after step 2

struct ScanJob {
    int64_t first_in, first_out;             // the scan's first row in xyz / in the output arrays
    int64_t scratch;                         // the sampled rows of the scans before it
    int32_t m, step, cap, pad;               // sampled rows, the effective step, the output region's rows
};
static_assert(sizeof(ScanJob) == 40, "the job table");
struct ScanTile { int32_t scan, tile; };

struct ScanArgs {
    const ScanJob* jobs; const ScanTile* tiles;
    scf::Params p;
    const float* xyz;
    float* out_xyz; float* out_normals; int32_t* out_count; int32_t* out_stage_counts; int32_t* out_status;
    int32_t* hdr;                            // scratch: [n_scans x HDR_WORDS]
    float* rows;                             // scratch: [SCAN_PLANES x the sampled rows of all scans]
    int stride;                              // scan_normals_kernel's LDS plane
};

extern __shared__ __attribute__((aligned(16))) unsigned char scf_smem[];

// Steps 4-6 of scan `scan` over its cloud C (c rows, planes of m) and, with normals, N: every thread of the workgroup calls it alike.
// Nothing is written beyond the region's J.cap rows: a row is written only when all of them fit.
__device__ __forceinline__ void emit(const ScanArgs& a, const ScanJob& J, int scan, const float* C, const float* N, int c, int status, int c1, int c2, int* wsum) {
    const int tid = threadIdx.x, m = J.m;
    const bool with_n = a.p.normals != 0;
    float* ox = a.out_xyz + J.first_out * 3;
    float* on = with_n ? a.out_normals + J.first_out * 3 : nullptr;
    auto keeps = [&](int i) __attribute__((always_inline)) { return i < c && (!with_n || scf::finite3(N[i], N[(size_t)m + i], N[(size_t)2 * m + i])); };
    int final_rows = 0;
    if (status == scf::ST_OK) {
        for (int base = 0; base < c; base += BLOCK) final_rows += __syncthreads_count(keeps(base + tid));
        if (final_rows == 0) status = scf::ST_EMPTY;
        else if (final_rows > J.cap) status = scf::ST_NO_ROOM;
    }
    int written = 0;
    if (status == scf::ST_OK) {
        for (int base = 0; base < c; base += BLOCK) {
            const int i = base + tid;
            const bool keep = keeps(i);
            int total;
            const int pos = written + block_rank(keep, wsum, total);
            if (keep) {
                const float x = C[i], y = C[(size_t)m + i], z = C[(size_t)2 * m + i];
                ox[(size_t)3 * pos] = x; ox[(size_t)3 * pos + 1] = y; ox[(size_t)3 * pos + 2] = z;
                if (with_n) {
                    float n[3] = {N[i], N[(size_t)m + i], N[(size_t)2 * m + i]};
                    if (a.p.ground_up > 0.0f) scf::ground_up(a.p.ground_up, x, y, z, n);
                    on[(size_t)3 * pos] = n[0]; on[(size_t)3 * pos + 1] = n[1]; on[(size_t)3 * pos + 2] = n[2];
                }
            }
            written += total;
        }
    }
    const float nan = m3d::float_of(scf::QUIET_NAN);
    for (int i = written + tid; i < J.cap; i += BLOCK) {
        ox[(size_t)3 * i] = nan; ox[(size_t)3 * i + 1] = nan; ox[(size_t)3 * i + 2] = nan;
        if (with_n) { on[(size_t)3 * i] = nan; on[(size_t)3 * i + 1] = nan; on[(size_t)3 * i + 2] = nan; }
    }
    if (tid == 0) {
        a.out_count[scan] = written;
        a.out_status[scan] = status;
        a.out_stage_counts[(size_t)3 * scan] = c1;
        a.out_stage_counts[(size_t)3 * scan + 1] = c2;
        a.out_stage_counts[(size_t)3 * scan + 2] = (status == scf::ST_OK || status == scf::ST_NO_ROOM) ? final_rows : 0;
    }
}

__global__ __launch_bounds__(BLOCK) void scan_voxel_kernel(ScanArgs a) {
    __shared__ int wsum[WAVES];
    __shared__ int lo[3], hi[3];
    const int tid = threadIdx.x, scan = blockIdx.x;
    const ScanJob J = a.jobs[scan];
    const int m = J.m;
    const float* in = a.xyz + J.first_in * 3;
    float* A = a.rows + (size_t)SCAN_PLANES * J.scratch;
    float* B = A + (size_t)3 * m;

    // ---- step 1: the sampled rows that stay, in order
    int c1 = 0;
    for (int base = 0; base < m; base += BLOCK) {
        const int i = base + tid;
        bool keep = false;
        float x = 0.0f, y = 0.0f, z = 0.0f;
        if (i < m) {
            const int64_t row = (int64_t)i * J.step;
            x = in[row * 3]; y = in[row * 3 + 1]; z = in[row * 3 + 2];
            keep = scf::stays(a.p, x, y, z);
        }
        int total;
        const int pos = c1 + block_rank(keep, wsum, total);
        if (keep) { A[pos] = x; A[(size_t)m + pos] = y; A[(size_t)2 * m + pos] = z; }
        c1 += total;
    }
    __syncthreads();

    // ---- step 2: one row per occupied voxel in ascending index
    int status = scf::ST_OK, c2 = 0;
    const float* C = A;
    if (c1 == 0) status = scf::ST_EMPTY;
    else if (a.p.voxel > 0.0f) {
        const float inv = scf::inverse_leaf(a.p.voxel);
        if (tid < 3) { lo[tid] = INT_MAX; hi[tid] = INT_MIN; }
        __syncthreads();
        int bad = 0;
        int l[3] = {INT_MAX, INT_MAX, INT_MAX}, u[3] = {INT_MIN, INT_MIN, INT_MIN};
        for (int i = tid; i < c1; i += BLOCK) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                int32_t cell;
                if (!scf::cell_of(A[(size_t)k * m + i], inv, cell)) { bad = 1; continue; }
                l[k] = min(l[k], cell); u[k] = max(u[k], cell);
            }
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) { atomicMin(&lo[k], l[k]); atomicMax(&hi[k], u[k]); }
        bad = __syncthreads_or(bad);
        const int32_t lo3[3] = {lo[0], lo[1], lo[2]}, hi3[3] = {hi[0], hi[1], hi[2]};
        int64_t d[3];
        if (bad || !scf::grid_dims(lo3, hi3, d)) status = scf::ST_GRID_TOO_LARGE;
        else {
            uint64_t* keys = reinterpret_cast<uint64_t*>(scf_smem);
            int p2 = 2;
            while (p2 < c1) p2 <<= 1;
            for (int j = tid; j < p2; j += BLOCK) {
                uint64_t key = ~0ull;
                if (j < c1) {
                    int32_t cell[3];
#pragma unroll
                    for (int k = 0; k < 3; ++k) scf::cell_of(A[(size_t)k * m + j], inv, cell[k]);
                    key = ((uint64_t)scf::voxel_index(cell, lo3, d) << 32) | (uint32_t)j;
                }
                keys[padded(j)] = key;
            }
            __syncthreads();
            bitonic_sort(keys, p2);
            for (int base = 0; base < c1; base += BLOCK) {
                const int j = base + tid;
                bool head = false;
                uint64_t key = 0;
                if (j < c1) {
                    key = keys[padded(j)];
                    head = j == 0 || (keys[padded(j - 1)] >> 32) != (key >> 32);
                }
                int total;
                const int v = c2 + block_rank(head, wsum, total);
                if (head) {
                    float sx = 0.0f, sy = 0.0f, sz = 0.0f;
                    int count = 0;
                    for (int k = j; k < c1; ++k) {
                        const uint64_t kk = keys[padded(k)];
                        if ((kk >> 32) != (key >> 32)) break;
                        const int row = (int)(uint32_t)kk;
                        sx = sx + A[row]; sy = sy + A[(size_t)m + row]; sz = sz + A[(size_t)2 * m + row];
                        ++count;
                    }
                    const float fc = (float)count;
                    B[v] = sx / fc; B[(size_t)m + v] = sy / fc; B[(size_t)2 * m + v] = sz / fc;
                }
                c2 += total;
            }
            __syncthreads();
            C = B;
        }
    } else c2 = c1;

    int c = status == scf::ST_OK ? c2 : 0;
    if (a.p.normals) {
        if (status == scf::ST_OK && c > scf::MAX_NORMAL_ROWS) { status = scf::ST_TOO_MANY_ROWS; c = 0; }
        if (tid == 0) {
            int32_t* hdr = a.hdr + (size_t)HDR_WORDS * scan;
            hdr[0] = c; hdr[1] = status; hdr[2] = c1; hdr[3] = c2;
        }
        return;
    }
    emit(a, J, scan, C, nullptr, c, status, c1, c2, wsum);
}

template <int KMAX>
__global__ __launch_bounds__(BLOCK) void scan_normals_kernel(ScanArgs a) {
    const int tid = threadIdx.x;
    const ScanTile T = a.tiles[blockIdx.x];
    const ScanJob J = a.jobs[T.scan];
    const int32_t* hdr = a.hdr + (size_t)HDR_WORDS * T.scan;
    const int c = hdr[0];
    if (hdr[1] != scf::ST_OK || T.tile * BLOCK >= c) return;           // the same for every thread; c <= MAX_NORMAL_ROWS <= the planes
    const int m = J.m, stride = a.stride;
    float* base = a.rows + (size_t)SCAN_PLANES * J.scratch;
    const float* C = a.p.voxel > 0.0f ? base + (size_t)3 * m : base;
    float* N = base + (size_t)6 * m;
    float* planes = reinterpret_cast<float*>(scf_smem);
    const float inf = m3d::float_of(0x7f800000u);
    const int n4 = (c + 3) & ~3;
    for (int j = tid; j < n4; j += BLOCK) {
        const bool in = j < c;
        planes[j] = in ? C[j] : inf;
        planes[stride + j] = in ? C[(size_t)m + j] : inf;
        planes[2 * stride + j] = in ? C[(size_t)2 * m + j] : inf;
    }
    __syncthreads();
    const int i = T.tile * BLOCK + tid;
    const bool live = i < c;
    const float px = live ? planes[i] : 0.0f, py = live ? planes[stride + i] : 0.0f, pz = live ? planes[2 * stride + i] : 0.0f;
    const float4* X = reinterpret_cast<const float4*>(planes);
    const float4* Y = reinterpret_cast<const float4*>(planes + stride);
    const float4* Z = reinterpret_cast<const float4*>(planes + 2 * stride);
    scf::Acc acc;
    scf::acc_clear(acc);
    int n = 0;
    if constexpr (KMAX > 0) {
        uint64_t key[KMAX];
#pragma unroll
        for (int s = 0; s < KMAX; ++s) key[s] = ~0ull;
        auto offer = [&](float d, int row) __attribute__((always_inline)) {
            uint64_t k = scf::neighbour_key(d, row);
            if (k < key[KMAX - 1]) {
#pragma unroll
                for (int s = 0; s < KMAX; ++s) {
                    const uint64_t t = key[s];
                    const bool lt = k < t;
                    key[s] = lt ? k : t;
                    k = lt ? t : k;
                }
            }
        };
        for (int j = 0; j < n4; j += 4) {
            const float4 x = X[j >> 2], y = Y[j >> 2], z = Z[j >> 2];
            offer(scf::dist2(px, py, pz, x.x, y.x, z.x), j);
            offer(scf::dist2(px, py, pz, x.y, y.y, z.y), j + 1);
            offer(scf::dist2(px, py, pz, x.z, y.z, z.z), j + 2);
            offer(scf::dist2(px, py, pz, x.w, y.w, z.w), j + 3);
        }
        n = min(a.p.k, c);
#pragma unroll
        for (int s = 0; s < KMAX; ++s) {
            if (s < n) {
                const int row = (int)(uint32_t)key[s];                 // a real row: the padding's keys lie above every real row's
                scf::acc_add(acc, px, py, pz, planes[row], planes[stride + row], planes[2 * stride + row]);
            }
        }
    } else {
        const float r2 = scf::radius2(a.p.radius);
        auto offer = [&](float d, int row, float qx, float qy, float qz) __attribute__((always_inline)) {
            if (row < c && d <= r2) { scf::acc_add(acc, px, py, pz, qx, qy, qz); ++n; }
        };
        for (int j = 0; j < n4; j += 4) {
            const float4 x = X[j >> 2], y = Y[j >> 2], z = Z[j >> 2];
            offer(scf::dist2(px, py, pz, x.x, y.x, z.x), j, x.x, y.x, z.x);
            offer(scf::dist2(px, py, pz, x.y, y.y, z.y), j + 1, x.y, y.y, z.y);
            offer(scf::dist2(px, py, pz, x.z, y.z, z.z), j + 2, x.z, y.z, z.z);
            offer(scf::dist2(px, py, pz, x.w, y.w, z.w), j + 3, x.w, y.w, z.w);
        }
    }
    float nrm[3];
    scf::normal_of(acc, n, px, py, pz, a.p.vp, nrm);
    if (live) { N[i] = nrm[0]; N[(size_t)m + i] = nrm[1]; N[(size_t)2 * m + i] = nrm[2]; }
}

__global__ __launch_bounds__(BLOCK) void scan_emit_kernel(ScanArgs a) {
    __shared__ int wsum[WAVES];
    const int scan = blockIdx.x;
    const ScanJob J = a.jobs[scan];
    const int32_t* hdr = a.hdr + (size_t)HDR_WORDS * scan;
    const float* base = a.rows + (size_t)SCAN_PLANES * J.scratch;
    const float* C = a.p.voxel > 0.0f ? base + (size_t)3 * J.m : base;
    emit(a, J, scan, C, base + (size_t)6 * J.m, hdr[0], hdr[1], hdr[2], hdr[3], wsum);
}

template <int KMAX>
void launch_normals(const ScanArgs& g, unsigned tiles, size_t lds, hipStream_t st) {
    allow_large_lds<&scan_normals_kernel<KMAX>>();
    scan_normals_kernel<KMAX><<<dim3(tiles), dim3(BLOCK), lds, st>>>(g);
}

}  // namespace
}  // namespace lcd

using namespace lcd;

namespace {

int filter_scans(lcd_engine* h, const lcd_scan_filter_args* a, bool on_device) {
    const char* who = on_device ? "lcd_filter_scans_dev" : "lcd_filter_scans";
    auto bad = [&](int code, const char* what) { return h->fail(code, std::string(who) + ": " + what); };
    // ---- everything that can be refused is refused before anything is enqueued or written
    if (!a || a->struct_size != (int32_t)sizeof(lcd_scan_filter_args)) return bad(LCD_ERR_INVALID, "null arguments or wrong struct_size");
    const float fl[] = {a->range_min, a->range_max, a->voxel_size, a->normal_radius, a->ground_normals_up, a->viewpoint[0], a->viewpoint[1], a->viewpoint[2]};
    for (float v : fl) if (!std::isfinite(v)) return bad(LCD_ERR_INVALID, "a float parameter that is not finite");
    if (a->voxel_size < 0.0f || a->normal_radius < 0.0f || a->ground_normals_up < 0.0f) return bad(LCD_ERR_INVALID, "voxel_size, normal_radius and ground_normals_up are >= 0");
    if (a->normal_k < 0 || a->normal_k > LCD_SCAN_MAX_K) return bad(LCD_ERR_INVALID, "normal_k is in 0 .. LCD_SCAN_MAX_K");
    if (a->normal_k > 0 && a->normal_radius > 0.0f) return bad(LCD_ERR_INVALID, "normal_k and normal_radius are both set");
    const bool normals = a->normal_k > 0 || a->normal_radius > 0.0f;
    if (const int rc = refuse_pairs(h, a->n_scans, bad)) return rc;
    if (normals && a->is_2d) return bad(LCD_ERR_UNSUPPORTED, "normals of 2-D scans are not offered");
    if (a->n_scans == 0) return LCD_OK;
    const int ns = a->n_scans;
    const int64_t* off = a->offsets;
    const int64_t* oo = a->out_offsets;
    if (!off || !oo || off[0] != 0 || oo[0] != 0) return bad(LCD_ERR_INVALID, "offsets missing or not starting at 0");
    for (int f = 0; f < ns; ++f) if (off[f + 1] < off[f] || oo[f + 1] < oo[f]) return bad(LCD_ERR_INVALID, "decreasing offsets");
    std::vector<ScanJob> jobs((size_t)ns);
    std::vector<ScanTile> tiles;
    int64_t sampled = 0;
    int m_max = 0;
    for (int f = 0; f < ns; ++f) {
        const int64_t n = off[f + 1] - off[f], cap = oo[f + 1] - oo[f];
        const int step = scf::step_of(a->downsampling_step, n);
        const int64_t m = n / step;
        if (m > scf::MAX_SAMPLED) return bad(LCD_ERR_UNSUPPORTED, "more than 16384 sampled rows in a scan");
        if (cap > INT_MAX) return bad(LCD_ERR_UNSUPPORTED, "an output region of more than INT_MAX rows");
        ScanJob& j = jobs[(size_t)f];
        j.first_in = off[f]; j.first_out = oo[f]; j.scratch = sampled; j.m = (int32_t)m; j.step = step; j.cap = (int32_t)cap; j.pad = 0;
        sampled += m;
        m_max = std::max(m_max, (int)m);
        if (normals)
            for (int t = 0; t * BLOCK < std::min<int64_t>(m, scf::MAX_NORMAL_ROWS); ++t) tiles.push_back(ScanTile{f, t});
    }
    const int64_t N = off[ns], M = oo[ns];
    if (!a->out_count || !a->out_stage_counts || !a->out_status) return bad(LCD_ERR_INVALID, "a null per-scan output");
    if ((N > 0 && !a->xyz) || (M > 0 && !a->out_xyz)) return bad(LCD_ERR_INVALID, "null rows or null out_xyz");
    if (normals && M > 0 && !a->out_normals) return bad(LCD_ERR_INVALID, "null out_normals while normals are asked for");
    if (!on_device)
        for (int64_t k = 0; k < N * 3; ++k) if (!std::isfinite(a->xyz[k])) return bad(LCD_ERR_INVALID, "a row that is not finite");

    StatelessScratch& S = h->pairs;
    hipStream_t st = h->stream;
    ScanArgs g;
    g.p.step = a->downsampling_step; g.p.is_2d = a->is_2d != 0; g.p.k = a->normal_k; g.p.normals = normals ? 1 : 0;
    g.p.range_min = a->range_min; g.p.range_max = a->range_max; g.p.voxel = a->voxel_size; g.p.radius = a->normal_radius; g.p.ground_up = a->ground_normals_up;
    for (int k = 0; k < 3; ++k) g.p.vp[k] = a->viewpoint[k];
    g.xyz = a->xyz; g.out_xyz = a->out_xyz; g.out_normals = normals ? a->out_normals : nullptr;
    g.out_count = a->out_count; g.out_stage_counts = a->out_stage_counts; g.out_status = a->out_status;
    g.stride = std::max((std::min(m_max, scf::MAX_NORMAL_ROWS) + 3) & ~3, 4);

    // ---- host entry: everything to the device, results back at the end (one synchronisation)
    HostStage stage(S, host_row_bytes(h), (size_t)h->row_bytes, on_device);
    stage.in(g.xyz, (size_t)N * 12);
    stage.out(g.out_xyz, (size_t)M * 12); stage.out(g.out_normals, (size_t)M * 12);
    stage.out(g.out_count, (size_t)ns * 4); stage.out(g.out_stage_counts, (size_t)ns * 12); stage.out(g.out_status, (size_t)ns * 4);
    LCD_HIP(h, stage.commit(st, &h->bytes_device));
    const size_t hdr_bytes = ((size_t)ns * HDR_WORDS * 4 + 15) & ~(size_t)15;
    LCD_HIP(h, dreserve(h, S.d_small, hdr_bytes + (size_t)std::max<int64_t>(sampled, 1) * SCAN_PLANES * 4));
    g.hdr = S.d_small.as<int32_t>();
    g.rows = reinterpret_cast<float*>(S.d_small.as<char>() + hdr_bytes);
    const size_t job_bytes = jobs.size() * sizeof(ScanJob);
    LCD_HIP(h, S.upload_table(&g.jobs, st, &h->bytes_device, jobs.data(), job_bytes, tiles.data(), tiles.size() * sizeof(ScanTile)));
    g.tiles = reinterpret_cast<const ScanTile*>(reinterpret_cast<const char*>(g.jobs) + job_bytes);

    int p2 = 2;
    while (p2 < m_max) p2 <<= 1;
    const size_t key_lds = a->voxel_size > 0.0f ? (size_t)padded(p2) * 8 : 16;
    allow_large_lds<&scan_voxel_kernel>();
    scan_voxel_kernel<<<dim3((unsigned)ns), dim3(BLOCK), key_lds, st>>>(g);
    LCD_HIP(h, hipGetLastError());
    if (normals) {
        if (!tiles.empty()) {
            const size_t lds = (size_t)3 * g.stride * 4;
            const unsigned nt = (unsigned)tiles.size();
            if (a->normal_k == 0) launch_normals<0>(g, nt, lds, st);
            else if (a->normal_k <= 8) launch_normals<8>(g, nt, lds, st);
            else if (a->normal_k <= 16) launch_normals<16>(g, nt, lds, st);
            else launch_normals<32>(g, nt, lds, st);
            LCD_HIP(h, hipGetLastError());
        }
        scan_emit_kernel<<<dim3((unsigned)ns), dim3(BLOCK), 0, st>>>(g);
        LCD_HIP(h, hipGetLastError());
    }
    LCD_HIP(h, stage.finish(st));
    return LCD_OK;
}

}  // namespace

extern "C" {

int lcd_filter_scans(lcd_engine* h, const lcd_scan_filter_args* a) { return stateless_entry(h, "lcd_filter_scans", filter_scans, a, false); }
int lcd_filter_scans_dev(lcd_engine* h, const lcd_scan_filter_args* a) { return stateless_entry(h, "lcd_filter_scans", filter_scans, a, true); }

}  // extern "C"
