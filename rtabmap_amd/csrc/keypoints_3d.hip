// keypoints_3d.hip -- lcd_keypoints_3d and its _dev form: the depth stage in front of the selection (reference Memory.cpp:5683-5694,
// :5911-5915, RegistrationVis.cpp:926-969) for a caller whose extractor leaves keypoints and whose camera leaves the depth image in device
// memory.  Every keypoint is looked up in the depth image and projected (util3d::generateKeypoints3DDepth), then the keypoints without a point
// in range are dropped (Feature2D::filterKeypointsByDepth) and keypoints, responses, descriptors, payload and points are compacted.  The rule
// is include/lcd.h's; its arithmetic is keypoints_3d_rule.h's, compiled here for the device and for the host entry's checks.
//   keypoints_3d_kernel: one launch per call, one workgroup of 256 threads per frame.  A thread takes a keypoint, gathers its 3 x 3 window
//     (nine loads at most) and computes the point; the kept flags are compacted in feature order with the ballot scan feature_select.hip uses
//     (compact_body.cuh), the thread writes its point, position and response at its rank; rows and payload follow behind the index list.
// Nothing of the engine is read or written: the job table (per frame the image, per camera the scaled intrinsics and the transform) and the
// host entry's staging are StatelessScratch's (stateless_scratch.h).
#include "engine_impl.h"
#include "compact_body.cuh"
#include "keypoints_3d_rule.h"

#include <vector>

static_assert(sizeof(lcd_camera) == 80, "lcd_camera: the layout include/lcd.h documents");
static_assert(sizeof(lcd_depth_image) == 40, "lcd_depth_image: the layout include/lcd.h documents (LP64)");
static_assert(sizeof(lcd_keypoints_3d_args) == 128, "lcd_keypoints_3d_args: the layout include/lcd.h documents (LP64)");
static_assert(LCD_DEPTH_U16_MM == lcd::kp3d::DEPTH_U16_MM && LCD_DEPTH_F32_M == lcd::kp3d::DEPTH_F32_M, "lcd_depth_type");
static_assert(LCD_KP3D_KEEP_ALL == lcd::kp3d::KEEP_ALL && LCD_KP3D_FILTER_3D == lcd::kp3d::FILTER_3D && LCD_KP3D_FILTER_PIXEL == lcd::kp3d::FILTER_PIXEL, "lcd_kp3d_filter");

namespace lcd {
namespace {

constexpr int BLOCK = 256;

struct Kp3dJob {
    kp3d::Image image;
    int64_t first;                           // the frame's first feature in every array
    int32_t n;
    int32_t cam_first;                       // the frame's first camera in the camera table
};
static_assert(sizeof(Kp3dJob) % 8 == 0 && sizeof(kp3d::Camera) == 80, "the job table: frames, then cameras, back to back");

struct Kp3dArgs {
    const Kp3dJob* jobs;
    const kp3d::Camera* cameras;
    int filter;
    float min_depth, max_depth;
    int row_bytes, row_vec, aux_bytes, aux_vec;   // *_vec: 16 or 4, the widest copy the addresses and sizes allow
    const float2* points; const float* response; const void* rows; const void* aux;
    int32_t* out_count; int32_t* out_index; float* out_xyz; float2* out_points; float* out_response; void* out_rows; void* out_aux;
};

__global__ __launch_bounds__(BLOCK) void keypoints_3d_kernel(Kp3dArgs a) {
    __shared__ int wsum[BLOCK / 64];
    const Kp3dJob& J = a.jobs[blockIdx.x];
    const kp3d::Image im = J.image;
    const kp3d::Camera* cams = a.cameras + J.cam_first;
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
            bool defined = true;
            if (a.out_xyz || a.filter != kp3d::FILTER_PIXEL) defined = kp3d::point_of(im, cams, pt.x, pt.y, a.min_depth, a.max_depth, p);
            if (a.filter == kp3d::KEEP_ALL) keep = true;
            else if (a.filter == kp3d::FILTER_3D) keep = defined && kp3d::keep_3d(p, a.min_depth, a.max_depth);
            else {
                bool px_defined;
                keep = kp3d::keep_pixel(im, pt.x, pt.y, a.min_depth, a.max_depth, &px_defined) && defined;
            }
        }
        int total;
        const int pos = count + block_rank(keep, wsum, total);
        if (keep) {
            out_index[pos] = i;
            if (a.out_xyz) {
                float* o = a.out_xyz + (first + pos) * 3;
                o[0] = p[0]; o[1] = p[1]; o[2] = p[2];
            }
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

int keypoints_3d(lcd_engine* h, const lcd_keypoints_3d_args* a, bool on_device) {
    const char* who = on_device ? "lcd_keypoints_3d_dev" : "lcd_keypoints_3d";
    auto bad = [&](int code, const char* what) { return h->fail(code, std::string(who) + ": " + what); };
    // ---- everything that can be refused is refused before anything is enqueued or written
    if (!a || a->struct_size != (int32_t)sizeof(lcd_keypoints_3d_args)) return bad(LCD_ERR_INVALID, "null arguments or wrong struct_size");
    if (a->filter != LCD_KP3D_KEEP_ALL && a->filter != LCD_KP3D_FILTER_3D && a->filter != LCD_KP3D_FILTER_PIXEL) return bad(LCD_ERR_INVALID, "unknown filter");
    if (a->aux_bytes < 0 || a->aux_bytes > 64 || a->aux_bytes % 4) return bad(LCD_ERR_INVALID, "aux_bytes is a multiple of 4, 0..64");
    if (a->min_depth != a->min_depth || a->max_depth != a->max_depth) return bad(LCD_ERR_INVALID, "a NaN depth bound");
    if (a->filter != LCD_KP3D_KEEP_ALL && a->min_depth < 0.0f) return bad(LCD_ERR_INVALID, "a filter needs min_depth >= 0");
    if (a->max_depth > 0.0f && a->max_depth <= a->min_depth) return bad(LCD_ERR_INVALID, "max_depth is <= 0 or above min_depth");
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
    const bool with_xyz = a->out_xyz != nullptr;
    if (!a->out_count || !a->images) return bad(LCD_ERR_INVALID, "null out_count or images");
    if (N > 0 && (!a->points || !a->out_index)) return bad(LCD_ERR_INVALID, "null points or out_index");
    if (N > 0 && !with_xyz && a->filter != LCD_KP3D_FILTER_PIXEL) return bad(LCD_ERR_INVALID, "null out_xyz");
    if (N > 0 && filtered && (!a->out_points || (with_resp && !a->out_response))) return bad(LCD_ERR_INVALID, "points or response without an output");
    if (N > 0 && filtered && ((with_rows && !a->out_rows) || (with_aux && !a->out_aux))) return bad(LCD_ERR_INVALID, "rows or aux without an output");

    std::vector<Kp3dJob> jobs((size_t)nf);
    std::vector<kp3d::Camera> cams;
    for (int f = 0; f < nf; ++f) {
        const lcd_depth_image& D = a->images[f];
        if (D.type != LCD_DEPTH_U16_MM && D.type != LCD_DEPTH_F32_M) return bad(LCD_ERR_INVALID, "unknown depth type");
        const int64_t px = D.type == LCD_DEPTH_U16_MM ? 2 : 4;
        if (!D.data || !D.cameras || D.width < 1 || D.height < 1 || D.n_cameras < 1) return bad(LCD_ERR_INVALID, "an empty depth image or no camera");
        if (D.width % D.n_cameras) return bad(LCD_ERR_INVALID, "the image width is no multiple of the number of cameras");
        if (D.pitch_bytes < (int64_t)D.width * px) return bad(LCD_ERR_INVALID, "a pitch below the row");
        if (D.pitch_bytes % px || (uintptr_t)D.data % (uintptr_t)px) return bad(LCD_ERR_INVALID, "an image that is not aligned to its pixels");
        Kp3dJob& J = jobs[(size_t)f];
        J.image.data = (const unsigned char*)D.data; J.image.pitch = D.pitch_bytes;
        J.image.width = D.width; J.image.height = D.height; J.image.type = D.type; J.image.n_cameras = D.n_cameras;
        kp3d::set_factors(J.image, D.cameras[0].image_width, D.cameras[0].image_height);
        J.first = off[f]; J.n = (int32_t)(off[f + 1] - off[f]); J.cam_first = (int32_t)cams.size();
        for (int c = 0; c < D.n_cameras; ++c) {
            const lcd_camera& L = D.cameras[c];
            kp3d::Camera C;
            C.cx = L.cx * J.image.factor_x; C.cy = L.cy * J.image.factor_y; C.fx = L.fx * J.image.factor_x; C.fy = L.fy * J.image.factor_y;
            std::memcpy(C.t, L.local_transform, sizeof C.t);
            C.has_t = L.has_local_transform ? 1 : 0; C.pad[0] = C.pad[1] = C.pad[2] = 0;
            cams.push_back(C);
        }
    }
    if (!on_device)                                                    // where the reference asserts or is undefined
        for (int f = 0; f < nf; ++f) {
            const Kp3dJob& J = jobs[(size_t)f];
            kp3d::Image probe = J.image;
            probe.width = probe.height = probe.sub_cols = 0;           // a probe reads no pixel: every lookup is outside
            for (int64_t i = off[f]; i < off[f + 1]; ++i) {
                float p[3];
                bool defined = true, px_defined = true;
                if (with_xyz || a->filter != LCD_KP3D_FILTER_PIXEL) defined = kp3d::point_of(probe, cams.data() + J.cam_first, a->points[2 * i], a->points[2 * i + 1], a->min_depth, a->max_depth, p);
                if (a->filter == LCD_KP3D_FILTER_PIXEL) (void)kp3d::keep_pixel(probe, a->points[2 * i], a->points[2 * i + 1], a->min_depth, a->max_depth, &px_defined);
                if (!defined || !px_defined) return bad(LCD_ERR_INVALID, "a keypoint that is not finite, beyond the range of int or in no camera's sub-image");
            }
        }
    StatelessScratch& S = h->pairs;
    hipStream_t st = h->stream;

    Kp3dArgs g;
    g.filter = a->filter; g.min_depth = a->min_depth; g.max_depth = a->max_depth;
    g.row_bytes = h->row_bytes; g.aux_bytes = a->aux_bytes;
    g.points = (const float2*)a->points; g.response = filtered ? a->response : nullptr;
    g.rows = filtered && with_rows ? a->rows : nullptr; g.aux = filtered && with_aux ? a->aux : nullptr;
    g.out_count = a->out_count; g.out_index = a->out_index; g.out_xyz = a->out_xyz;
    g.out_points = filtered ? (float2*)a->out_points : nullptr; g.out_response = g.response ? a->out_response : nullptr;
    g.out_rows = a->out_rows; g.out_aux = a->out_aux;

    // ---- host entry: everything to the device (every distinct image once, its rows packed), results back at the end (one synchronisation)
    HostStage stage(S, host_row_bytes(h), (size_t)h->row_bytes, on_device);
    std::vector<unsigned char> packed;
    std::vector<size_t> at;                                            // where each frame's image lies in `packed`
    if (!on_device) {
        at.resize((size_t)nf);
        for (int f = 0; f < nf; ++f) {
            const lcd_depth_image& D = a->images[f];
            int same = -1;
            for (int e = 0; e < f && same < 0; ++e) {
                const lcd_depth_image& E = a->images[e];
                if (E.data == D.data && E.pitch_bytes == D.pitch_bytes && E.width == D.width && E.height == D.height && E.type == D.type) same = e;
            }
            const size_t row = (size_t)D.width * (D.type == LCD_DEPTH_U16_MM ? 2 : 4);
            if (same >= 0) at[(size_t)f] = at[(size_t)same];
            else {
                at[(size_t)f] = packed.size();
                packed.resize(packed.size() + ((row * (size_t)D.height + 15) & ~(size_t)15));
                for (int r = 0; r < D.height; ++r) std::memcpy(packed.data() + at[(size_t)f] + (size_t)r * row, (const char*)D.data + (int64_t)r * D.pitch_bytes, row);
            }
            jobs[(size_t)f].image.pitch = (int64_t)row;
        }
    }
    const size_t aux_bytes = g.aux ? (size_t)N * a->aux_bytes : 0;
    const unsigned char* images = packed.data();
    stage.in(g.points, (size_t)N * 8); stage.in(g.response, (size_t)N * 4);
    stage.in_rows(g.rows, N); stage.in(g.aux, aux_bytes);
    stage.in(images, packed.size());                                   // a plain region: behind commit(), `images` is where it lies on the device
    stage.out(g.out_count, (size_t)nf * 4); stage.out(g.out_index, (size_t)N * 4);
    // handed out below: only what each frame kept
    const int o_xyz = stage.out_kept(g.out_xyz, (size_t)N * 12), o_pts = stage.out_kept(g.out_points, (size_t)N * 8);
    const int o_resp = stage.out_kept(g.out_response, (size_t)N * 4);
    const int o_rows = stage.out_kept(g.out_rows, g.rows ? (size_t)N * h->row_bytes : 0), o_aux = stage.out_kept(g.out_aux, aux_bytes);
    LCD_HIP(h, stage.commit(st, &h->bytes_device));
    for (size_t f = 0; f < at.size(); ++f) jobs[f].image.data = images + at[f];
    g.row_vec = g.rows && g.row_bytes % 16 == 0 && aligned16(g.rows) && aligned16(g.out_rows) ? 16 : 4;
    g.aux_vec = g.aux && g.aux_bytes % 16 == 0 && aligned16(g.aux) && aligned16(g.out_aux) ? 16 : 4;

    const size_t job_bytes = jobs.size() * sizeof(Kp3dJob);
    LCD_HIP(h, S.upload_table(&g.jobs, st, &h->bytes_device, jobs.data(), job_bytes, cams.data(), cams.size() * sizeof(kp3d::Camera)));
    g.cameras = reinterpret_cast<const kp3d::Camera*>(reinterpret_cast<const char*>(g.jobs) + job_bytes);
    keypoints_3d_kernel<<<dim3((unsigned)nf), dim3(BLOCK), 0, st>>>(g);
    LCD_HIP(h, hipGetLastError());
    LCD_HIP(h, stage.finish(st));
    // only what the frame wrote: the rest of its region stays as it was
    stage.hand_out(o_xyz, a->out_count, off, nf, 12); stage.hand_out(o_pts, a->out_count, off, nf, 8); stage.hand_out(o_resp, a->out_count, off, nf, 4);
    stage.hand_out_rows(o_rows, a->out_count, off, nf); stage.hand_out(o_aux, a->out_count, off, nf, (size_t)a->aux_bytes);
    return LCD_OK;
}

}  // namespace

extern "C" {

int lcd_keypoints_3d(lcd_engine* h, const lcd_keypoints_3d_args* a) { return stateless_entry(h, "lcd_keypoints_3d", keypoints_3d, a, false); }
int lcd_keypoints_3d_dev(lcd_engine* h, const lcd_keypoints_3d_args* a) { return stateless_entry(h, "lcd_keypoints_3d", keypoints_3d, a, true); }

}  // extern "C"
