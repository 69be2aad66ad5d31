// keypoints_3d_stereo.hip -- lcd_keypoints_3d_stereo and its _dev form: lcd_keypoints_3d for a frame with a right image instead of a depth
// image (reference Features2d.cpp:960-1016 with Stereo/OpticalFlow = true).  The rule is include/lcd.h's; its arithmetic is
// stereo_flow_rule.h's, compiled here for the device and in rtabmap_amd/host/Stereo.cpp for the host mirror.
//   stereo_pyramid_kernel (pyramid_kernel.cuh, shared with flow_track.hip): one launch per level for the whole batch.  A workgroup takes a
//     32 x 8 tile of the new level of one image: the source rows with their two-pixel halo go to LDS, the horizontal pass goes once into LDS,
//     then the vertical pass.  No derivative image is written: the tracker takes the derivatives from the patch it stages anyway.
//   stereo_track_kernel: one wave per keypoint, four waves per workgroup, the levels top down inside the kernel.  The wave stages the left
//     (w + 3) x (h + 3) patch and computes I, dx and dy of the window into LDS as shorts; in each iteration the lanes compute the window's int
//     terms in parallel (64 window pixels at a time) and the fp32 sums run in the rule's order over those terms by lane broadcast -- ordered
//     adds, not a tree.  Every branch on convergence, bounds and status is the wave's: it has one keypoint.  No workgroup barrier.
//   stereo_emit_kernel: one workgroup of 256 threads per frame, as keypoints_3d_kernel: updateStatus, the projection in double, the filter
//     and the compaction (compact_body.cuh).
// Nothing of the engine is read or written: the pyramids' upper levels and the tracker's results live in StatelessScratch::d_small, the job
// table (frames with their cameras, then image pairs) and the host entry's staging are StatelessScratch's (stateless_scratch.h).
#include "engine_impl.h"
#include "compact_body.cuh"
#include "pyramid_kernel.cuh"

#include <vector>

static_assert(sizeof(lcd_stereo_camera) == 104, "lcd_stereo_camera: the layout include/lcd.h documents");
static_assert(sizeof(lcd_stereo_image) == 48, "lcd_stereo_image: the layout include/lcd.h documents (LP64)");
static_assert(sizeof(lcd_stereo_params) == 56, "lcd_stereo_params: the layout include/lcd.h documents");
static_assert(sizeof(lcd_keypoints_3d_stereo_args) == 152, "lcd_keypoints_3d_stereo_args: the layout include/lcd.h documents (LP64)");

namespace lcd {
namespace {

namespace rule = lcd::stereo;

using pyramid::BLOCK;
using pyramid::PatchPx;
using pyramid::stereo_pyramid_kernel;
constexpr int TRACK_WAVES = 4;

struct StereoPair {                          // two images of pyramid_kernel.cuh's table, with the same number of levels
    pyramid::Image left, right;
};
struct StereoJob {
    int64_t first;                           // the frame's first feature in every array
    int32_t n, pair;
    rule::Camera cam;
};
static_assert(sizeof(StereoJob) % 8 == 0 && sizeof(StereoPair) == 2 * sizeof(pyramid::Image), "the job table: frames, then pairs (two images each), back to back");
static_assert(sizeof(rule::Track) == 16, "16 bytes per keypoint in d_small");

struct TrackArgs {
    const StereoJob* jobs;
    const StereoPair* pairs;
    rule::Params P;
    const float2* points;
    rule::Track* track;
    int wave_bytes;                          // LDS per wave: the window's I, dx, dy as shorts, then the left patch
};

// what a wave wrote to LDS is what its other lanes read behind this
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ float lane_value(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }

__global__ __launch_bounds__(TRACK_WAVES * 64) void stereo_track_kernel(TrackArgs a) {
    extern __shared__ unsigned char lds[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const StereoJob& Jb = a.jobs[blockIdx.y];
    const int i = (int)blockIdx.x * TRACK_WAVES + wave;
    if (i >= Jb.n) return;
    const StereoPair& Pr = a.pairs[Jb.pair];
    const rule::Params& P = a.P;
    const int ww = P.win_w, wh = P.win_h, n = ww * wh, pw = ww + 3, ph = wh + 3;
    short* Ib = reinterpret_cast<short*>(lds + (size_t)wave * a.wave_bytes);
    short* dxb = Ib + n;
    short* dyb = Ib + 2 * n;
    unsigned char* patch = reinterpret_cast<unsigned char*>(Ib + 3 * n);
    rule::Track* out = a.track + Jb.first + i;
    const float2 pt = a.points[Jb.first + i];
    if (!kp3d::convertible(pt.x) || !kp3d::convertible(pt.y)) {
        if (lane == 0) { out->rx = out->ry = kp3d::quiet_nan(); out->status = 0; out->err = 0.0f; }
        return;
    }
    const float hx = (float)(ww - 1) * 0.5f, hy = (float)(wh - 1) * 0.5f;
    const int levels = Pr.left.n_levels;
    int status = 1;
    float err = 0.0f, nx = 0.0f, ny = 0.0f;
    // the body below is stereo::track_point's, statement for statement; only the window loops are the wave's
    for (int level = levels - 1; level >= 0; --level) {
        const rule::GlobalPx pi{Pr.left.level[level]}, pj{Pr.right.level[level]};
        const int cols = pi.L.w, rows = pi.L.h;
        const float scale = 1.0f / (float)(1 << level);
        float px = pt.x * scale, py = pt.y * scale;
        float qx, qy;
        if (level == levels - 1) { qx = px; qy = py; }
        else { qx = nx * 2.0f; qy = ny * 2.0f; }
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
        float s11 = 0.0f, s12 = 0.0f, s22 = 0.0f;
        for (int base = 0; base < n; base += 64) {
            const int p = base + lane;
            float t11 = 0.0f, t12 = 0.0f, t22 = 0.0f;
            if (p < n) {
                const int y = p / ww, x = p - y * ww;
                const int iv = rule::sample(pp, ipx, ipy, x, y, iw);
                int ix, iy;
                rule::sample_deriv(pp, ipx, ipy, x, y, cols, rows, iw, ix, iy);
                Ib[p] = (short)iv; dxb[p] = (short)ix; dyb[p] = (short)iy;
                t11 = (float)(ix * ix); t12 = (float)(ix * iy); t22 = (float)(iy * iy);
            }
            const int cnt = min(64, n - base);
            for (int l = 0; l < cnt; ++l) {                            // the rule's order: row-major over the window
                s11 = s11 + lane_value(t11, l);
                s12 = s12 + lane_value(t12, l);
                s22 = s22 + lane_value(t22, l);
            }
        }
        wave_sync();
        const float A11 = s11 * rule::FLT_SCALE, A12 = s12 * rule::FLT_SCALE, A22 = s22 * rule::FLT_SCALE;
        float inv_d;
        if (!rule::solve(A11, A12, A22, ww, wh, P.min_eig_threshold, &inv_d)) {
            if (level == 0) status = 0;
            continue;
        }
        qx = qx - hx; qy = qy - hy;
        float prev_dx = 0.0f;
        for (int j = 0; j < P.iterations; ++j) {
            const int inx = rule::floor_int(qx), iny = rule::floor_int(qy);
            if (rule::outside(inx, iny, ww, wh, cols, rows)) {
                if (level == 0) status = 0;
                break;
            }
            rule::weights(qx - (float)inx, qy - (float)iny, iw);
            float sb1 = 0.0f, sb2 = 0.0f;
            for (int base = 0; base < n; base += 64) {
                const int p = base + lane;
                float t1 = 0.0f, t2 = 0.0f;
                if (p < n) {
                    const int y = p / ww, x = p - y * ww;
                    const int diff = rule::sample(pj, inx, iny, x, y, iw) - (int)Ib[p];
                    t1 = (float)(diff * (int)dxb[p]); t2 = (float)(diff * (int)dyb[p]);
                }
                const int cnt = min(64, n - base);
                for (int l = 0; l < cnt; ++l) {
                    sb1 = sb1 + lane_value(t1, l);
                    sb2 = sb2 + lane_value(t2, l);
                }
            }
            const float b1 = sb1 * rule::FLT_SCALE, b2 = sb2 * rule::FLT_SCALE;
            const float dx = rule::delta_x(A12, A22, b1, b2, inv_d);
            qx = qx + dx;
            nx = qx + hx; ny = qy + hy;
            if (rule::converged(dx, P.eps2)) break;
            if (j > 0 && rule::oscillates(dx, prev_dx)) {
                const float half = dx * 0.5f;
                nx = nx - half;
                break;
            }
            prev_dx = dx;
        }
        if (status && level == 0 && !P.use_min_eigenvals) {
            const float ex = nx - hx, ey = ny - hy;
            const int iex = rule::floor_int(ex), iey = rule::floor_int(ey);
            if (rule::outside(iex, iey, ww, wh, cols, rows)) { status = 0; continue; }
            rule::weights(ex - (float)iex, ey - (float)iey, iw);
            float errval = 0.0f;
            for (int base = 0; base < n; base += 64) {
                const int p = base + lane;
                float t = 0.0f;
                if (p < n) {
                    const int y = p / ww, x = p - y * ww;
                    int diff = rule::sample(pj, iex, iey, x, y, iw) - (int)Ib[p];
                    if (diff < 0) diff = -diff;
                    t = (float)diff;
                }
                const int cnt = min(64, n - base);
                for (int l = 0; l < cnt; ++l) errval = errval + lane_value(t, l);
            }
            err = errval / (float)(32 * ww * wh);
        }
    }
    if (lane == 0) { out->rx = nx; out->ry = ny; out->status = status; out->err = err; }
}

struct EmitArgs {
    const StereoJob* jobs;
    const rule::Track* track;
    rule::Params P;
    int filter;
    float min_depth, max_depth;
    int row_bytes, row_vec, aux_bytes, aux_vec;   // *_vec: 16 or 4, the widest copy the addresses and sizes allow
    const float2* points; const float* response; const void* rows; const void* aux;
    int32_t* out_count; int32_t* out_index; float* out_xyz; float2* out_points; float* out_response; void* out_rows; void* out_aux;
    float2* out_right; uint8_t* out_status;
};

__global__ __launch_bounds__(BLOCK) void stereo_emit_kernel(EmitArgs a) {
    __shared__ int wsum[BLOCK / 64];
    const StereoJob& J = a.jobs[blockIdx.x];
    const int n = J.n, tid = threadIdx.x;
    const int64_t first = J.first;
    int32_t* out_index = a.out_index + first;
    int count = 0;
    for (int base = 0; base < n; base += BLOCK) {
        const int i = base + tid;
        bool keep = false;
        float p[3] = {0.0f, 0.0f, 0.0f};
        float2 pt = make_float2(0.0f, 0.0f);
        if (i < n) {
            pt = a.points[first + i];
            const rule::Track T = a.track[first + i];
            const int status = rule::update_status(T, pt.x, a.P);
            if (a.out_right) a.out_right[first + i] = make_float2(T.rx, T.ry);
            if (a.out_status) a.out_status[first + i] = (uint8_t)status;
            rule::point_of(J.cam, status, pt.x, pt.y, T.rx, a.min_depth, a.max_depth, p);
            keep = a.filter == kp3d::KEEP_ALL || kp3d::keep_3d(p, a.min_depth, a.max_depth);
        }
        int total;
        const int pos = count + block_rank(keep, wsum, total);
        if (keep) {
            out_index[pos] = i;
            float* o = a.out_xyz + (first + pos) * 3;
            o[0] = p[0]; o[1] = p[1]; o[2] = p[2];
            if (a.out_points) a.out_points[first + pos] = pt;
            if (a.out_response) a.out_response[first + pos] = a.response[first + i];
        }
        count += total;
    }
    for (int i = count + tid; i < n; i += BLOCK) out_index[i] = -1;
    if (tid == 0) a.out_count[blockIdx.x] = count;
    if (!a.rows && !a.aux) return;
    __syncthreads();                                                   // the index list is read back by the threads that gather
    if (a.rows) gather_kept_rows(a.rows, a.out_rows, out_index, first, count, a.row_bytes, a.row_vec);
    if (a.aux) gather_kept_rows(a.aux, a.out_aux, out_index, first, count, a.aux_bytes, a.aux_vec);
}

}  // namespace
}  // namespace lcd

using namespace lcd;

namespace {

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline bool is_nan(double v) { return v != v; }

struct HostImage { const void* data; int64_t pitch; int32_t width, height; size_t at; };

int keypoints_3d_stereo(lcd_engine* h, const lcd_keypoints_3d_stereo_args* a, bool on_device) {
    const char* who = on_device ? "lcd_keypoints_3d_stereo_dev" : "lcd_keypoints_3d_stereo";
    auto bad = [&](int code, const char* what) { return h->fail(code, std::string(who) + ": " + what); };
    // ---- everything that can be refused is refused before anything is enqueued or written
    if (!a || a->struct_size != (int32_t)sizeof(lcd_keypoints_3d_stereo_args)) return bad(LCD_ERR_INVALID, "null arguments or wrong struct_size");
    if (a->filter == LCD_KP3D_FILTER_PIXEL) return bad(LCD_ERR_INVALID, "LCD_KP3D_FILTER_PIXEL has no meaning without a depth image");
    if (a->filter != LCD_KP3D_KEEP_ALL && a->filter != LCD_KP3D_FILTER_3D) return bad(LCD_ERR_INVALID, "unknown filter");
    if (a->aux_bytes < 0 || a->aux_bytes > 64 || a->aux_bytes % 4) return bad(LCD_ERR_INVALID, "aux_bytes is a multiple of 4, 0..64");
    if (a->min_depth != a->min_depth || a->max_depth != a->max_depth) return bad(LCD_ERR_INVALID, "a NaN depth bound");
    if (a->filter != LCD_KP3D_KEEP_ALL && a->min_depth < 0.0f) return bad(LCD_ERR_INVALID, "a filter needs min_depth >= 0");
    if (a->max_depth > 0.0f && a->max_depth <= a->min_depth) return bad(LCD_ERR_INVALID, "max_depth is <= 0 or above min_depth");
    if (!a->params) return bad(LCD_ERR_INVALID, "null params");
    const lcd_stereo_params& sp = *a->params;
    if (sp.win_width < rule::MIN_WIN || sp.win_width > rule::MAX_WIN || sp.win_height < rule::MIN_WIN || sp.win_height > rule::MAX_WIN) return bad(LCD_ERR_INVALID, "win_width and win_height are 3..31");
    if (sp.max_level < 0 || sp.max_level >= rule::MAX_LEVELS) return bad(LCD_ERR_INVALID, "max_level is 0..8");
    if (is_nan(sp.eps) || is_nan(sp.min_eig_threshold) || is_nan(sp.error_threshold) || is_nan(sp.min_disparity) || is_nan(sp.max_disparity)) return bad(LCD_ERR_INVALID, "a NaN parameter");
    if (sp.min_disparity < 0.0f || sp.min_disparity > sp.max_disparity) return bad(LCD_ERR_INVALID, "min_disparity is >= 0 and <= max_disparity");
    if (a->n_frames < 0) return bad(LCD_ERR_INVALID, "negative n_frames");
    if (a->n_frames > 65535) return bad(LCD_ERR_UNSUPPORTED, "more than 65535 frames per call");
    if (h->shard_append || h->shard_first || h->shard_block) return bad(LCD_ERR_UNSUPPORTED, "not offered on the handles of a sharded vocabulary");
    const bool with_rows = a->rows != nullptr, with_aux = a->aux != nullptr && a->aux_bytes > 0, with_resp = a->response != nullptr;
    if (on_device && with_rows && rows_padded(h)) return bad(LCD_ERR_UNSUPPORTED, "the handle's rows are padded: a [n x dim] device buffer is not what the kernel walks");
    if (a->n_frames == 0) return LCD_OK;
    const int nf = a->n_frames;
    const int64_t* off = a->offsets;
    if (!off || off[0] != 0) return bad(LCD_ERR_INVALID, "offsets missing or not starting at 0");
    for (int f = 0; f < nf; ++f) {
        if (off[f + 1] < off[f]) return bad(LCD_ERR_INVALID, "decreasing offsets");
        if (off[f + 1] - off[f] > 0x7fffffff) return bad(LCD_ERR_UNSUPPORTED, "more than 2^31 - 1 features in a frame");
    }
    const int64_t N = off[nf];
    const bool filtered = a->filter != LCD_KP3D_KEEP_ALL;
    if (!a->out_count || !a->images) return bad(LCD_ERR_INVALID, "null out_count or images");
    if (N > 0 && (!a->points || !a->out_index || !a->out_xyz)) return bad(LCD_ERR_INVALID, "null points, out_index or out_xyz");
    if (N > 0 && filtered && (!a->out_points || (with_resp && !a->out_response))) return bad(LCD_ERR_INVALID, "points or response without an output");
    if (N > 0 && filtered && ((with_rows && !a->out_rows) || (with_aux && !a->out_aux))) return bad(LCD_ERR_INVALID, "rows or aux without an output");

    const rule::Params P = rule::clamp_params(sp.win_width, sp.win_height, sp.max_level, sp.iterations, sp.eps, sp.use_min_eigenvals, sp.min_eig_threshold,
                                              sp.error_threshold, sp.min_disparity, sp.max_disparity);
    std::vector<StereoJob> jobs((size_t)nf);
    std::vector<StereoPair> pairs;
    std::vector<int> pair_frame;                                       // the first frame of each pair
    int max_n = 0;
    for (int f = 0; f < nf; ++f) {
        const lcd_stereo_image& S = a->images[f];
        if (!S.left || !S.right || !S.camera) return bad(LCD_ERR_INVALID, "an image pair without data or camera");
        if (S.width <= sp.win_width || S.height <= sp.win_height) return bad(LCD_ERR_INVALID, "an image that is not larger than the window");
        if (S.left_pitch_bytes < S.width || S.right_pitch_bytes < S.width) return bad(LCD_ERR_INVALID, "a pitch below the row");
        if (S.left_pitch_bytes > 0x7fffffff || S.right_pitch_bytes > 0x7fffffff) return bad(LCD_ERR_INVALID, "a pitch beyond 2^31 - 1");
        const lcd_stereo_camera& L = *S.camera;
        if (is_nan(L.fx) || is_nan(L.fy) || is_nan(L.cx) || is_nan(L.cy) || is_nan(L.right_cx) || is_nan(L.baseline)) return bad(LCD_ERR_INVALID, "a NaN in the camera");
        if (!(L.baseline > 0.0) || !(L.fx > 0.0)) return bad(LCD_ERR_INVALID, "baseline and fx are > 0");
        StereoJob& J = jobs[(size_t)f];
        J.first = off[f]; J.n = (int32_t)(off[f + 1] - off[f]);
        max_n = std::max(max_n, (int)J.n);
        J.cam.fx = L.fx; J.cam.fy = L.fy; J.cam.cx = L.cx; J.cam.cy = L.cy; J.cam.right_cx = L.right_cx; J.cam.baseline = L.baseline;
        std::memcpy(J.cam.t, L.local_transform, sizeof J.cam.t);
        J.cam.has_t = L.has_local_transform ? 1 : 0; J.cam.pad = 0;
        int same = -1;
        for (size_t e = 0; e < pairs.size() && same < 0; ++e) {
            const lcd_stereo_image& E = a->images[pair_frame[e]];
            if (E.left == S.left && E.right == S.right && E.left_pitch_bytes == S.left_pitch_bytes && E.right_pitch_bytes == S.right_pitch_bytes &&
                E.width == S.width && E.height == S.height) same = (int)e;
        }
        if (same < 0) {
            same = (int)pairs.size();
            StereoPair Q;
            std::memset(&Q, 0, sizeof Q);
            Q.left.n_levels = Q.right.n_levels = rule::n_levels(S.width, S.height, P.win_w, P.win_h, P.max_level);
            Q.left.level[0] = rule::Level{(const unsigned char*)S.left, (int32_t)S.left_pitch_bytes, S.width, S.height, 0};
            Q.right.level[0] = rule::Level{(const unsigned char*)S.right, (int32_t)S.right_pitch_bytes, S.width, S.height, 0};
            pairs.push_back(Q);
            pair_frame.push_back(f);
        }
        J.pair = same;
    }
    if (!on_device)                                                    // where the reference asserts or is undefined
        for (int64_t i = 0; i < N; ++i)
            if (!kp3d::convertible(a->points[2 * i]) || !kp3d::convertible(a->points[2 * i + 1])) return bad(LCD_ERR_INVALID, "a keypoint that is not finite or beyond the range of int");
    StatelessScratch& S = h->pairs;
    hipStream_t st = h->stream;

    EmitArgs g;
    g.P = P; g.filter = a->filter; g.min_depth = a->min_depth; g.max_depth = a->max_depth;
    g.row_bytes = h->row_bytes; g.aux_bytes = a->aux_bytes;
    g.points = (const float2*)a->points; g.response = filtered ? a->response : nullptr;
    g.rows = filtered && with_rows ? a->rows : nullptr; g.aux = filtered && with_aux ? a->aux : nullptr;
    g.out_count = a->out_count; g.out_index = a->out_index; g.out_xyz = a->out_xyz;
    g.out_points = filtered ? (float2*)a->out_points : nullptr; g.out_response = g.response ? a->out_response : nullptr;
    g.out_rows = a->out_rows; g.out_aux = a->out_aux;
    g.out_right = (float2*)a->out_right; g.out_status = a->out_status;

    // ---- host entry: everything to the device (every distinct image once, its rows packed), results back at the end (one synchronisation)
    HostStage stage(S, host_row_bytes(h), (size_t)h->row_bytes, on_device);
    std::vector<unsigned char> packed;
    std::vector<HostImage> staged;
    auto stage_image = [&](const void* data, int64_t pitch, int w, int ht) {
        for (const HostImage& E : staged) if (E.data == data && E.pitch == pitch && E.width == w && E.height == ht) return E.at;
        const size_t at = packed.size();
        packed.resize(at + (((size_t)w * (size_t)ht + 15) & ~(size_t)15));
        for (int r = 0; r < ht; ++r) std::memcpy(packed.data() + at + (size_t)r * (size_t)w, (const char*)data + (int64_t)r * pitch, (size_t)w);
        staged.push_back(HostImage{data, pitch, w, ht, at});
        return at;
    };
    std::vector<size_t> at_left, at_right;
    if (!on_device)
        for (StereoPair& Q : pairs) {
            at_left.push_back(stage_image(Q.left.level[0].data, Q.left.level[0].pitch, Q.left.level[0].w, Q.left.level[0].h));
            at_right.push_back(stage_image(Q.right.level[0].data, Q.right.level[0].pitch, Q.right.level[0].w, Q.right.level[0].h));
            Q.left.level[0].pitch = Q.right.level[0].pitch = Q.left.level[0].w;
        }
    const size_t aux_bytes = g.aux ? (size_t)N * a->aux_bytes : 0;
    const unsigned char* images = packed.data();
    stage.in(g.points, (size_t)N * 8); stage.in(g.response, (size_t)N * 4);
    stage.in_rows(g.rows, N); stage.in(g.aux, aux_bytes);
    stage.in(images, packed.size());                                   // a plain region: behind commit(), `images` is where it lies on the device
    stage.out(g.out_count, (size_t)nf * 4); stage.out(g.out_index, (size_t)N * 4);
    stage.out(g.out_right, (size_t)N * 8); stage.out(g.out_status, (size_t)N);
    // handed out below: only what each frame kept
    const int o_xyz = stage.out_kept(g.out_xyz, (size_t)N * 12), o_pts = stage.out_kept(g.out_points, (size_t)N * 8);
    const int o_resp = stage.out_kept(g.out_response, (size_t)N * 4);
    const int o_rows = stage.out_kept(g.out_rows, g.rows ? (size_t)N * h->row_bytes : 0), o_aux = stage.out_kept(g.out_aux, aux_bytes);
    LCD_HIP(h, stage.commit(st, &h->bytes_device));
    for (size_t e = 0; e < at_left.size(); ++e) { pairs[e].left.level[0].data = images + at_left[e]; pairs[e].right.level[0].data = images + at_right[e]; }
    g.row_vec = g.rows && g.row_bytes % 16 == 0 && aligned16(g.rows) && aligned16(g.out_rows) ? 16 : 4;
    g.aux_vec = g.aux && g.aux_bytes % 16 == 0 && aligned16(g.aux) && aligned16(g.out_aux) ? 16 : 4;

    // ---- d_small: the tracker's results, then every pair's levels 1.. of the left and of the right image
    size_t small = ((size_t)N * sizeof(rule::Track) + 255) & ~(size_t)255;
    int top = 1;                                                       // the most levels a pair has
    unsigned max_tiles = 1;
    for (StereoPair& Q : pairs) {
        top = std::max(top, (int)Q.left.n_levels);
        pyramid::place_levels(Q.left, &small, &max_tiles);             // offsets until d_small is known
        pyramid::place_levels(Q.right, &small, &max_tiles);
    }
    LCD_HIP(h, S.d_small.reserve(small, 0, st, &h->bytes_device));
    for (StereoPair& Q : pairs) { pyramid::rebase(Q.left, S.d_small.as<unsigned char>()); pyramid::rebase(Q.right, S.d_small.as<unsigned char>()); }

    const size_t job_bytes = jobs.size() * sizeof(StereoJob);
    LCD_HIP(h, S.upload_table(&g.jobs, st, &h->bytes_device, jobs.data(), job_bytes, pairs.data(), pairs.size() * sizeof(StereoPair)));
    const StereoPair* d_pairs = reinterpret_cast<const StereoPair*>(reinterpret_cast<const char*>(g.jobs) + job_bytes);
    g.track = S.d_small.as<rule::Track>();
    if (max_n > 0) {
        const uint64_t blocks = (uint64_t)max_tiles * 2u * pairs.size();
        if (blocks > 0x7fffffffu) return bad(LCD_ERR_UNSUPPORTED, "more than 2^31 - 1 pyramid tiles in a call");
        for (int l = 1; l < top; ++l) {
            stereo_pyramid_kernel<<<dim3((unsigned)(blocks)), dim3(BLOCK), 0, st>>>(reinterpret_cast<const pyramid::Image*>(d_pairs), l, max_tiles);
            LCD_HIP(h, hipGetLastError());
        }
        TrackArgs t;
        t.jobs = g.jobs; t.pairs = d_pairs; t.P = P; t.points = g.points; t.track = S.d_small.as<rule::Track>();
        const int n = P.win_w * P.win_h;
        t.wave_bytes = (n * 6 + (P.win_w + 3) * (P.win_h + 3) + 15) & ~15;
        stereo_track_kernel<<<dim3((unsigned)((max_n + TRACK_WAVES - 1) / TRACK_WAVES), (unsigned)nf), dim3(TRACK_WAVES * 64), (size_t)t.wave_bytes * TRACK_WAVES, st>>>(t);
        LCD_HIP(h, hipGetLastError());
    }
    stereo_emit_kernel<<<dim3((unsigned)nf), dim3(BLOCK), 0, st>>>(g);
    LCD_HIP(h, hipGetLastError());
    LCD_HIP(h, stage.finish(st));
    // only what the frame wrote: the rest of its region stays as it was
    stage.hand_out(o_xyz, a->out_count, off, nf, 12); stage.hand_out(o_pts, a->out_count, off, nf, 8); stage.hand_out(o_resp, a->out_count, off, nf, 4);
    stage.hand_out_rows(o_rows, a->out_count, off, nf); stage.hand_out(o_aux, a->out_count, off, nf, (size_t)a->aux_bytes);
    return LCD_OK;
}

}  // namespace

extern "C" {

int lcd_keypoints_3d_stereo(lcd_engine* h, const lcd_keypoints_3d_stereo_args* a) { return stateless_entry(h, "lcd_keypoints_3d_stereo", keypoints_3d_stereo, a, false); }
int lcd_keypoints_3d_stereo_dev(lcd_engine* h, const lcd_keypoints_3d_stereo_args* a) { return stateless_entry(h, "lcd_keypoints_3d_stereo", keypoints_3d_stereo, a, true); }

}  // extern "C"
