// flow_track.hip -- lcd_track_flow and its _dev form: the optical-flow correspondences of RegistrationVis (Vis/CorType = 1, reference
// RegistrationVis.cpp:510-780): every corner of the from image is tracked into the to image by pyramidal Lucas-Kanade on both axes, and the
// tracked ones that land inside the image are kept and compacted with their payload.  The rule is include/lcd.h's; its arithmetic is
// flow_track_rule.h's (over stereo_flow_rule.h), compiled here for the device and in rtabmap_amd/host/FlowTrack.cpp for the host mirror.
//   stereo_pyramid_kernel (pyramid_kernel.cuh, shared with keypoints_3d_stereo.hip): one launch per level for the whole batch, over every
//     DISTINCT image (pointer, pitch and size), built to the highest level any of its pairs needs.
//   flow_track_kernel: one wave per corner, four waves per workgroup, the levels top down inside the kernel.  The wave stages the from
//     (w + 3) x (h + 3) patch and computes I, dx and dy of the window into LDS as shorts.  Lane l owns the window pixels l, l + 64, ..: it
//     adds their terms in ascending order from +0, and the 64 partials are added by a butterfly of five ds_swizzle steps and one exchange
//     of the wave's halves -- lane l adds what lane l ^ s holds, s = 32, 16, .. 1, which is the rule's halving tree (fp32 addition commutes)
//     and leaves the sum in every lane.  Every branch on bounds, eigenvalue, convergence and status is the wave's: it has one corner.  No
//     workgroup barrier, no private segment.
//   flow_keep_kernel: one workgroup of 256 threads per pair: the keep test, the compaction (compact_body.cuh), the optional per-input outputs.
// Nothing of the engine is read or written: the pyramids' upper levels and the tracker's results live in StatelessScratch::d_small, the job
// table (pairs, then distinct images) and the host entry's staging are StatelessScratch's (stateless_scratch.h).
#include "engine_impl.h"
#include "compact_body.cuh"
#include "pyramid_kernel.cuh"
#include "flow_track_rule.h"

#include <map>
#include <tuple>
#include <vector>

static_assert(sizeof(lcd_flow_pair) == 48, "lcd_flow_pair: the layout include/lcd.h documents (LP64)");
static_assert(sizeof(lcd_flow_params) == 40, "lcd_flow_params: the layout include/lcd.h documents");
static_assert(sizeof(lcd_track_flow_args) == 128, "lcd_track_flow_args: the layout include/lcd.h documents (LP64)");

namespace lcd {
namespace {

namespace rule = lcd::stereo;

using pyramid::BLOCK;
using pyramid::PatchPx;
using pyramid::stereo_pyramid_kernel;
constexpr int TRACK_WAVES = 4;

struct FlowJob {
    int64_t first;                           // the pair's first feature in every array
    int32_t n, from, to;                     // from, to: the pair's images in the image table
    int32_t n_levels, use_initial;
    int32_t width, height, pad;
};
static_assert(sizeof(FlowJob) % 8 == 0, "the job table: pairs, then images, back to back");
static_assert(sizeof(rule::Track) == 16, "16 bytes per corner in d_small");

struct TrackArgs {
    const FlowJob* jobs;
    const pyramid::Image* images;
    rule::Params P;
    const float2* points;
    const float2* initial;
    rule::Track* track;
    int wave_bytes;                          // LDS per wave: the window's I, dx, dy as shorts, then the from patch
};

// what a wave wrote to LDS is what its other lanes read behind this
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// what lane ^ S holds, S < 32: ds_swizzle in bit-mask mode (and 0x1f, or 0, xor S) moves registers and touches no LDS memory
template <int S>
__device__ __forceinline__ float swizzle_xor(float v) { return __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(v), (S << 10) | 0x1f)); }
// the halving tree of the rule over the 64 lanes' partials; every lane ends with the sum
__device__ __forceinline__ float lane_tree(float v) {
    v = v + __shfl_xor(v, 32);
    v = v + swizzle_xor<16>(v);
    v = v + swizzle_xor<8>(v);
    v = v + swizzle_xor<4>(v);
    v = v + swizzle_xor<2>(v);
    v = v + swizzle_xor<1>(v);
    return v;
}

__global__ __launch_bounds__(TRACK_WAVES * 64) void flow_track_kernel(TrackArgs a) {
    extern __shared__ unsigned char lds[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const FlowJob& Jb = a.jobs[blockIdx.y];
    const int i = (int)blockIdx.x * TRACK_WAVES + wave;
    if (i >= Jb.n) return;
    const pyramid::Image& From = a.images[Jb.from];
    const pyramid::Image& To = a.images[Jb.to];
    const rule::Params& P = a.P;
    const int ww = P.win_w, wh = P.win_h, n = ww * wh, pw = ww + 3, ph = wh + 3;
    short* Ib = reinterpret_cast<short*>(lds + (size_t)wave * a.wave_bytes);
    short* dxb = Ib + n;
    short* dyb = Ib + 2 * n;
    unsigned char* patch = reinterpret_cast<unsigned char*>(Ib + 3 * n);
    rule::Track* out = a.track + Jb.first + i;
    const float2 pt = a.points[Jb.first + i];
    const int use_initial = Jb.use_initial;
    float2 start = make_float2(0.0f, 0.0f);
    if (use_initial) start = a.initial[Jb.first + i];
    if (!flow::trackable(pt.x, pt.y, use_initial, start.x, start.y)) {
        if (lane == 0) { out->rx = out->ry = kp3d::quiet_nan(); out->status = 0; out->err = 0.0f; }
        return;
    }
    const float hx = (float)(ww - 1) * 0.5f, hy = (float)(wh - 1) * 0.5f;
    const int levels = Jb.n_levels;
    int status = 1;
    float err = 0.0f, nx = 0.0f, ny = 0.0f;
    // the body below is flow::track_point_2d's, statement for statement; only the window loops and the sums are the wave's
    for (int level = levels - 1; level >= 0; --level) {
        const rule::GlobalPx pi{From.level[level]}, pj{To.level[level]};
        const int cols = pi.L.w, rows = pi.L.h;
        const float scale = 1.0f / (float)(1 << level);
        float px = pt.x * scale, py = pt.y * scale;
        float qx, qy;
        if (level == levels - 1) {
            if (use_initial) { qx = start.x * scale; qy = start.y * scale; }
            else { qx = px; qy = py; }
        } else { qx = nx * 2.0f; qy = ny * 2.0f; }
        nx = qx; ny = qy;
        px = px - hx; py = py - hy;
        const int ipx = rule::floor_int(px), ipy = rule::floor_int(py);
        if (rule::outside(ipx, ipy, ww, wh, cols, rows)) {
            if (level == 0) status = 0;
            continue;
        }
        int iw[4];
        rule::weights(px - (float)ipx, py - (float)ipy, iw);
        wave_sync();                                                   // the window of the level above is no longer read
        for (int e = lane; e < pw * ph; e += 64) {
            const int r = e / pw, c = e - r * pw;
            patch[e] = (unsigned char)pi(ipx - 1 + c, ipy - 1 + r);
        }
        wave_sync();
        const PatchPx pp{patch, ipx - 1, ipy - 1, pw};
        float s11 = 0.0f, s12 = 0.0f, s22 = 0.0f;                      // this lane's part: its pixels in ascending order
        for (int p = lane; p < n; p += 64) {
            const int y = p / ww, x = p - y * ww;
            const int iv = rule::sample(pp, ipx, ipy, x, y, iw);
            int ix, iy;
            rule::sample_deriv(pp, ipx, ipy, x, y, cols, rows, iw, ix, iy);
            Ib[p] = (short)iv; dxb[p] = (short)ix; dyb[p] = (short)iy;
            s11 = s11 + (float)(ix * ix);
            s12 = s12 + (float)(ix * iy);
            s22 = s22 + (float)(iy * iy);
        }
        // (a lane reads back only the Ib, dxb, dyb it wrote itself: pixel p belongs to lane p % 64 in every loop)
        s11 = lane_tree(s11); s12 = lane_tree(s12); s22 = lane_tree(s22);
        const float A11 = s11 * rule::FLT_SCALE, A12 = s12 * rule::FLT_SCALE, A22 = s22 * rule::FLT_SCALE;
        const float eig = flow::min_eig(A11, A12, A22, ww, wh);
        if (P.use_min_eigenvals) err = eig;
        float inv_d;
        if (!flow::solve(A11, A12, A22, eig, P.min_eig_threshold, &inv_d)) {
            if (level == 0) status = 0;
            continue;
        }
        qx = qx - hx; qy = qy - hy;
        float prev_dx = 0.0f, prev_dy = 0.0f;
        for (int j = 0; j < P.iterations; ++j) {
            const int inx = rule::floor_int(qx), iny = rule::floor_int(qy);
            if (rule::outside(inx, iny, ww, wh, cols, rows)) {
                if (level == 0) status = 0;
                break;
            }
            rule::weights(qx - (float)inx, qy - (float)iny, iw);
            float sb1 = 0.0f, sb2 = 0.0f;
            for (int p = lane; p < n; p += 64) {
                const int y = p / ww, x = p - y * ww;
                const int diff = rule::sample(pj, inx, iny, x, y, iw) - (int)Ib[p];
                sb1 = sb1 + (float)(diff * (int)dxb[p]);
                sb2 = sb2 + (float)(diff * (int)dyb[p]);
            }
            sb1 = lane_tree(sb1); sb2 = lane_tree(sb2);
            const float b1 = sb1 * rule::FLT_SCALE, b2 = sb2 * rule::FLT_SCALE;
            float dx, dy;
            flow::step(A11, A12, A22, b1, b2, inv_d, &dx, &dy);
            qx = qx + dx; qy = qy + dy;
            nx = qx + hx; ny = qy + hy;
            if (flow::converged(dx, dy, P.eps2)) break;
            if (j > 0 && flow::oscillates(dx, dy, prev_dx, prev_dy)) {
                const float half_x = dx * 0.5f, half_y = dy * 0.5f;
                nx = nx - half_x; ny = ny - half_y;
                break;
            }
            prev_dx = dx; prev_dy = dy;
        }
        if (status && level == 0 && !P.use_min_eigenvals) {
            const float ex = nx - hx, ey = ny - hy;
            const int iex = rule::floor_int(ex), iey = rule::floor_int(ey);
            if (rule::outside(iex, iey, ww, wh, cols, rows)) { status = 0; continue; }
            rule::weights(ex - (float)iex, ey - (float)iey, iw);
            float errval = 0.0f;
            for (int p = lane; p < n; p += 64) {
                const int y = p / ww, x = p - y * ww;
                int diff = rule::sample(pj, iex, iey, x, y, iw) - (int)Ib[p];
                if (diff < 0) diff = -diff;
                errval = errval + (float)diff;
            }
            errval = lane_tree(errval);
            err = errval / (float)(32 * ww * wh);
        }
    }
    if (lane == 0) { out->rx = nx; out->ry = ny; out->status = status; out->err = err; }
}

struct KeepArgs {
    const FlowJob* jobs;
    const rule::Track* track;
    int use_min_eigenvals;
    float error_threshold;
    int aux_bytes, aux_vec;                  // aux_vec: 16 or 4, the widest copy the addresses and sizes allow
    const float2* points; const void* aux;
    int32_t* out_count; int32_t* out_index; float2* out_from; float2* out_to; void* out_aux;
    float2* out_track; uint8_t* out_status; float* out_err;
};

__global__ __launch_bounds__(BLOCK) void flow_keep_kernel(KeepArgs a) {
    __shared__ int wsum[BLOCK / 64];
    const FlowJob& J = a.jobs[blockIdx.x];
    const int n = J.n, tid = threadIdx.x;
    const int64_t first = J.first;
    int32_t* out_index = a.out_index + first;
    int count = 0;
    for (int base = 0; base < n; base += BLOCK) {
        const int i = base + tid;
        bool keep = false;
        float2 pt = make_float2(0.0f, 0.0f), to = make_float2(0.0f, 0.0f);
        if (i < n) {
            pt = a.points[first + i];
            const rule::Track T = a.track[first + i];
            to = make_float2(T.rx, T.ry);
            if (a.out_track) a.out_track[first + i] = to;
            if (a.out_status) a.out_status[first + i] = (uint8_t)T.status;
            if (a.out_err) a.out_err[first + i] = T.err;
            keep = flow::keep(T, J.width, J.height, a.use_min_eigenvals, a.error_threshold);
        }
        int total;
        const int pos = count + block_rank(keep, wsum, total);
        if (keep) {
            out_index[pos] = i;
            a.out_from[first + pos] = pt;
            a.out_to[first + pos] = to;
        }
        count += total;
    }
    for (int i = count + tid; i < n; i += BLOCK) out_index[i] = -1;
    if (tid == 0) a.out_count[blockIdx.x] = count;
    if (!a.aux) return;
    __syncthreads();                                                   // the index list is read back by the threads that gather
    gather_kept_rows(a.aux, a.out_aux, out_index, first, count, a.aux_bytes, a.aux_vec);
}

}  // namespace
}  // namespace lcd

using namespace lcd;

namespace {

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline bool is_nan(double v) { return v != v; }

struct ImageKey { const void* data; int64_t pitch; int32_t width, height; size_t at; };

int track_flow(lcd_engine* h, const lcd_track_flow_args* a, bool on_device) {
    const char* who = on_device ? "lcd_track_flow_dev" : "lcd_track_flow";
    auto bad = [&](int code, const char* what) { return h->fail(code, std::string(who) + ": " + what); };
    // ---- everything that can be refused is refused before anything is enqueued or written
    if (!a || a->struct_size != (int32_t)sizeof(lcd_track_flow_args)) return bad(LCD_ERR_INVALID, "null arguments or wrong struct_size");
    if (a->aux_bytes < 0 || a->aux_bytes > 64 || a->aux_bytes % 4) return bad(LCD_ERR_INVALID, "aux_bytes is a multiple of 4, 0..64");
    if (!a->params) return bad(LCD_ERR_INVALID, "null params");
    const lcd_flow_params& fp = *a->params;
    if (fp.win_width < rule::MIN_WIN || fp.win_width > rule::MAX_WIN || fp.win_height < rule::MIN_WIN || fp.win_height > rule::MAX_WIN) return bad(LCD_ERR_INVALID, "win_width and win_height are 3..31");
    if (is_nan(fp.eps) || is_nan(fp.min_eig_threshold) || is_nan(fp.error_threshold)) return bad(LCD_ERR_INVALID, "a NaN parameter");
    if (a->n_pairs < 0) return bad(LCD_ERR_INVALID, "negative n_pairs");
    if (a->n_pairs > 65535) return bad(LCD_ERR_UNSUPPORTED, "more than 65535 pairs per call");
    if (h->shard_append || h->shard_first || h->shard_block) return bad(LCD_ERR_UNSUPPORTED, "not offered on the handles of a sharded vocabulary");
    if (a->n_pairs == 0) return LCD_OK;
    const int np = a->n_pairs;
    const int64_t* off = a->offsets;
    if (!off || off[0] != 0) return bad(LCD_ERR_INVALID, "offsets missing or not starting at 0");
    for (int p = 0; p < np; ++p) {
        if (off[p + 1] < off[p]) return bad(LCD_ERR_INVALID, "decreasing offsets");
        if (off[p + 1] - off[p] > 0x7fffffff) return bad(LCD_ERR_UNSUPPORTED, "more than 2^31 - 1 features in a pair");
    }
    const int64_t N = off[np];
    const bool with_aux = a->aux != nullptr && a->aux_bytes > 0;
    if (!a->out_count || !a->pairs) return bad(LCD_ERR_INVALID, "null out_count or pairs");
    if (N > 0 && (!a->points || !a->out_index || !a->out_from || !a->out_to)) return bad(LCD_ERR_INVALID, "null points, out_index, out_from or out_to");
    if (N > 0 && with_aux && !a->out_aux) return bad(LCD_ERR_INVALID, "aux without an output");

    const rule::Params P = rule::clamp_params(fp.win_width, fp.win_height, 0, fp.iterations, fp.eps, fp.use_min_eigenvals, fp.min_eig_threshold,
                                              (double)fp.error_threshold, 0.0f, 0.0f);
    std::vector<FlowJob> jobs((size_t)np);
    std::vector<pyramid::Image> images;
    std::vector<ImageKey> keys;
    std::map<std::tuple<const void*, int64_t, int, int>, int> index_of;
    auto image_of = [&](const void* data, int64_t pitch, int w, int ht, int levels) {
        const auto found = index_of.emplace(std::make_tuple(data, pitch, w, ht), (int)keys.size());      // a map: 65 535 pairs may bring 131 070 images
        const int e = found.first->second;
        if (found.second) {
            pyramid::Image Q;
            std::memset(&Q, 0, sizeof Q);
            Q.level[0] = rule::Level{(const unsigned char*)data, (int32_t)pitch, w, ht, 0};
            images.push_back(Q);
            keys.push_back(ImageKey{data, pitch, w, ht, 0});
        }
        images[(size_t)e].n_levels = std::max(images[(size_t)e].n_levels, (int32_t)levels);   // to the highest level any of its pairs needs
        return e;
    };
    int max_n = 0;
    bool any_initial = false;
    for (int p = 0; p < np; ++p) {
        const lcd_flow_pair& S = a->pairs[p];
        if (!S.from || !S.to) return bad(LCD_ERR_INVALID, "a pair without image data");
        if (S.max_level < 0 || S.max_level >= rule::MAX_LEVELS) return bad(LCD_ERR_INVALID, "max_level is 0..8");
        if (S.width <= fp.win_width || S.height <= fp.win_height) return bad(LCD_ERR_INVALID, "an image that is not larger than the window");
        if (S.from_pitch_bytes < S.width || S.to_pitch_bytes < S.width) return bad(LCD_ERR_INVALID, "a pitch below the row");
        if (S.from_pitch_bytes > 0x7fffffff || S.to_pitch_bytes > 0x7fffffff) return bad(LCD_ERR_INVALID, "a pitch beyond 2^31 - 1");
        if (S.use_initial && !a->initial) return bad(LCD_ERR_INVALID, "use_initial without initial");
        any_initial = any_initial || S.use_initial != 0;
        FlowJob& J = jobs[(size_t)p];
        J.first = off[p]; J.n = (int32_t)(off[p + 1] - off[p]);
        max_n = std::max(max_n, (int)J.n);
        J.n_levels = rule::n_levels(S.width, S.height, P.win_w, P.win_h, S.max_level);
        J.use_initial = S.use_initial ? 1 : 0;
        J.width = S.width; J.height = S.height; J.pad = 0;
        J.from = image_of(S.from, S.from_pitch_bytes, S.width, S.height, J.n_levels);
        J.to = image_of(S.to, S.to_pitch_bytes, S.width, S.height, J.n_levels);
    }
    if (!on_device)                                                    // where the reference asserts or is undefined
        for (int p = 0; p < np; ++p)
            for (int64_t i = off[p]; i < off[p + 1]; ++i) {
                const bool ui = jobs[(size_t)p].use_initial != 0;
                if (!flow::trackable(a->points[2 * i], a->points[2 * i + 1], ui, ui ? a->initial[2 * i] : 0.0f, ui ? a->initial[2 * i + 1] : 0.0f))
                    return bad(LCD_ERR_INVALID, "a corner or a start position that is not finite or beyond the range of int");
            }
    StatelessScratch& S = h->pairs;
    hipStream_t st = h->stream;

    KeepArgs g;
    g.use_min_eigenvals = P.use_min_eigenvals; g.error_threshold = fp.error_threshold;
    g.aux_bytes = a->aux_bytes;
    g.points = (const float2*)a->points; g.aux = with_aux ? a->aux : nullptr;
    g.out_count = a->out_count; g.out_index = a->out_index; g.out_from = (float2*)a->out_from; g.out_to = (float2*)a->out_to;
    g.out_aux = with_aux ? a->out_aux : nullptr;
    g.out_track = (float2*)a->out_track; g.out_status = a->out_status; g.out_err = a->out_err;
    const float2* initial = any_initial ? (const float2*)a->initial : nullptr;

    // ---- host entry: everything to the device (every distinct image once, its rows packed), results back at the end (one synchronisation)
    HostStage stage(S, host_row_bytes(h), (size_t)h->row_bytes, on_device);
    std::vector<unsigned char> packed;
    if (!on_device)
        for (size_t e = 0; e < images.size(); ++e) {
            const rule::Level& L = images[e].level[0];
            const size_t at = packed.size();
            packed.resize(at + (((size_t)L.w * (size_t)L.h + 15) & ~(size_t)15));
            for (int r = 0; r < L.h; ++r) std::memcpy(packed.data() + at + (size_t)r * (size_t)L.w, (const char*)L.data + (int64_t)r * L.pitch, (size_t)L.w);
            keys[e].at = at;
        }
    const size_t aux_bytes = g.aux ? (size_t)N * a->aux_bytes : 0;
    const unsigned char* pixels = packed.data();
    stage.in(g.points, (size_t)N * 8); stage.in(initial, (size_t)N * 8); stage.in(g.aux, aux_bytes);
    stage.in(pixels, packed.size());                                   // a plain region: behind commit(), `pixels` is where it lies on the device
    stage.out(g.out_count, (size_t)np * 4); stage.out(g.out_index, (size_t)N * 4);
    stage.out(g.out_track, (size_t)N * 8); stage.out(g.out_status, (size_t)N); stage.out(g.out_err, (size_t)N * 4);
    // handed out below: only what each pair kept
    const int o_from = stage.out_kept(g.out_from, (size_t)N * 8), o_to = stage.out_kept(g.out_to, (size_t)N * 8);
    const int o_aux = stage.out_kept(g.out_aux, aux_bytes);
    LCD_HIP(h, stage.commit(st, &h->bytes_device));
    if (!on_device)
        for (size_t e = 0; e < images.size(); ++e) { images[e].level[0].data = pixels + keys[e].at; images[e].level[0].pitch = images[e].level[0].w; }
    g.aux_vec = g.aux && g.aux_bytes % 16 == 0 && aligned16(g.aux) && aligned16(g.out_aux) ? 16 : 4;

    // ---- d_small: the tracker's results, then every distinct image's levels 1..
    size_t small = ((size_t)N * sizeof(rule::Track) + 255) & ~(size_t)255;
    int top = 1;                                                       // the most levels an image has
    unsigned max_tiles = 1;
    for (pyramid::Image& Q : images) {
        top = std::max(top, (int)Q.n_levels);
        pyramid::place_levels(Q, &small, &max_tiles);                  // offsets until d_small is known
    }
    LCD_HIP(h, S.d_small.reserve(small, 0, st, &h->bytes_device));
    for (pyramid::Image& Q : images) pyramid::rebase(Q, S.d_small.as<unsigned char>());

    const size_t job_bytes = jobs.size() * sizeof(FlowJob);
    LCD_HIP(h, S.upload_table(&g.jobs, st, &h->bytes_device, jobs.data(), job_bytes, images.data(), images.size() * sizeof(pyramid::Image)));
    const pyramid::Image* d_images = reinterpret_cast<const pyramid::Image*>(reinterpret_cast<const char*>(g.jobs) + job_bytes);
    g.track = S.d_small.as<rule::Track>();
    if (max_n > 0) {
        const uint64_t blocks = (uint64_t)max_tiles * images.size();
        if (blocks > 0x7fffffffu) return bad(LCD_ERR_UNSUPPORTED, "more than 2^31 - 1 pyramid tiles in a call");
        for (int l = 1; l < top; ++l) {
            stereo_pyramid_kernel<<<dim3((unsigned)(blocks)), dim3(BLOCK), 0, st>>>(d_images, l, max_tiles);
            LCD_HIP(h, hipGetLastError());
        }
        TrackArgs t;
        t.jobs = g.jobs; t.images = d_images; t.P = P; t.points = g.points; t.initial = initial; t.track = S.d_small.as<rule::Track>();
        const int n = P.win_w * P.win_h;
        t.wave_bytes = (n * 6 + (P.win_w + 3) * (P.win_h + 3) + 15) & ~15;
        flow_track_kernel<<<dim3((unsigned)((max_n + TRACK_WAVES - 1) / TRACK_WAVES), (unsigned)np), dim3(TRACK_WAVES * 64), (size_t)t.wave_bytes * TRACK_WAVES, st>>>(t);
        LCD_HIP(h, hipGetLastError());
    }
    flow_keep_kernel<<<dim3((unsigned)np), dim3(BLOCK), 0, st>>>(g);
    LCD_HIP(h, hipGetLastError());
    LCD_HIP(h, stage.finish(st));
    // only what the pair wrote: the rest of its region stays as it was
    stage.hand_out(o_from, a->out_count, off, np, 8); stage.hand_out(o_to, a->out_count, off, np, 8);
    stage.hand_out(o_aux, a->out_count, off, np, (size_t)a->aux_bytes);
    return LCD_OK;
}

}  // namespace

extern "C" {

int lcd_track_flow(lcd_engine* h, const lcd_track_flow_args* a) { return stateless_entry(h, "lcd_track_flow", track_flow, a, false); }
int lcd_track_flow_dev(lcd_engine* h, const lcd_track_flow_args* a) { return stateless_entry(h, "lcd_track_flow", track_flow, a, true); }

}  // extern "C"
