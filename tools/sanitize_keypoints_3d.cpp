// sanitize_keypoints_3d.cpp -- Keypoints3D's three functions (plain host code: the rule of lcd_keypoints_3d) driven from a stand-alone
// program, for a host-only AddressSanitizer / UndefinedBehaviorSanitizer run.  No engine is created and nothing touches a GPU.
//
//   g++ -std=c++17 -g -O1 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -Irtabmap_amd/host \
//       tools/sanitize_keypoints_3d.cpp rtabmap_amd/host/Keypoints3D.cpp -o keypoints_3d_asan
//   ./keypoints_3d_asan
//
// Random images whose buffers end with their last pixel (a read past the sub-image, the row or the image is a heap overflow), u16 and f32,
// 1, 2 and 4 cameras, a pitch larger than the row, holes of every kind, keypoints on and beyond every border, NaN, infinite and huge
// coordinates, against a second, naive restatement of the rule that copies each camera's sub-image into an image of its own and walks it
// as the reference's text does; exit status 0 and "ok" when all agree bit for bit.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "Keypoints3D.h"

using rtabmap_amd::DepthCamera;
using rtabmap_amd::DepthImage;
using rtabmap_amd::Keypoints3D;

namespace {

struct Sub {                                   // one camera's sub-image in metres, 0 where a u16 pixel is no measurement
    int cols, rows;
    std::vector<float> m;
    float at(int u, int v) const { return m[(size_t)v * cols + u]; }
};

bool intOk(float v) { return std::isfinite(v) && v > -2147483648.0f && v < 2147483648.0f; }

// util2d::getDepth with smoothing, as the reference writes it
float naiveDepth(const Sub& s, float x, float y) {
    int u = int(x + 0.5f), v = int(y + 0.5f);
    if (u == s.cols && x < float(s.cols)) u = s.cols - 1;
    if (v == s.rows && y < float(s.rows)) v = s.rows - 1;
    if (!(u >= 0 && u < s.cols && v >= 0 && v < s.rows)) return 0;
    const int u_start = std::max(u - 1, 0), v_start = std::max(v - 1, 0), u_end = std::min(u + 1, s.cols - 1), v_end = std::min(v + 1, s.rows - 1);
    volatile float depth = s.at(u, v);
    if (!(depth != 0.0f && std::isfinite(depth))) return 0;
    volatile float sumWeights = 0.0f, sumDepths = 0.0f;
    for (int uu = u_start; uu <= u_end; ++uu)
        for (int vv = v_start; vv <= v_end; ++vv)
            if (!(uu == u && vv == v)) {
                volatile float d = s.at(uu, vv);
                volatile float depthError = 0.02f * depth;
                if (d != 0.0f && std::isfinite(d) && std::fabs(d - depth) < depthError) {
                    if (uu == u || vv == v) { sumWeights = sumWeights + 2.0f; d = d * 2.0f; }
                    else sumWeights = sumWeights + 1.0f;
                    sumDepths = sumDepths + d;
                }
            }
    depth = depth * 4.0f;
    sumWeights = sumWeights + 4.0f;
    volatile float total = depth + sumDepths;
    return total / sumWeights;
}

// generateKeypoints3DDepth's loop body; false where the reference asserts or is undefined
bool naivePoint(const std::vector<Sub>& subs, const std::vector<DepthCamera>& cams, float px, float py, float minDepth, float maxDepth, float out[3]) {
    const float nan = std::numeric_limits<float>::quiet_NaN();
    out[0] = out[1] = out[2] = nan;
    const float subW = float(subs[0].cols);
    volatile float rx = cams[0].imageWidth > 0 ? float(cams[0].imageWidth) / subW : 1.0f;
    volatile float ry = cams[0].imageHeight > 0 ? float(cams[0].imageHeight) / float(subs[0].rows) : 1.0f;
    volatile float fX = 1.0f / rx, fY = 1.0f / ry;
    volatile float x = px * fX, y = py * fY;
    volatile float q = x / subW;
    volatile float xh = x + 0.5f, yh = y + 0.5f;
    if (!intOk(xh) || !intOk(yh) || !intOk(q)) return false;
    const int cam = int(q);
    if (cam < 0 || cam >= (int)cams.size()) return false;
    volatile float shift = subW * float(cam);
    volatile float xs = x - shift;
    const float depth = naiveDepth(subs[(size_t)cam], xs, y);
    if (!(depth > 0.0f)) return true;
    const DepthCamera& C = cams[(size_t)cam];
    volatile float cx = C.cx * fX, cy = C.cy * fY, fx = C.fx * fX, fy = C.fy * fY;
    if (!(cx > 0.0f)) cx = float(subs[0].cols / 2) - 0.5f;
    if (!(cy > 0.0f)) cy = float(subs[0].rows / 2) - 0.5f;
    volatile float dx = xs - cx, dy = y - cy;
    volatile float nx = dx * depth, ny = dy * depth;
    volatile float X = nx / fx, Y = ny / fy, Z = depth;
    if (!(std::isfinite(X) && std::isfinite(Y) && std::isfinite(Z) && (minDepth < 0.0f || Z > minDepth) && (maxDepth <= 0.0f || Z <= maxDepth))) return true;
    if (!C.hasLocalTransform) { out[0] = X; out[1] = Y; out[2] = Z; return true; }
    for (int r = 0; r < 3; ++r) {
        volatile float a = C.localTransform[4 * r] * X, b = C.localTransform[4 * r + 1] * Y, c = C.localTransform[4 * r + 2] * Z;
        volatile float s = a + b;
        s = s + c;
        out[r] = s + C.localTransform[4 * r + 3];
    }
    return true;
}

bool sameBits(const float* a, const float* b, size_t n) { return n == 0 || std::memcmp(a, b, n * sizeof(float)) == 0; }

}  // namespace

int main() {
    std::mt19937 rng(13);
    auto upto = [&](int n) { return n <= 0 ? 0 : (int)(rng() % (unsigned)n); };
    auto unit = [&]() { return (float)(rng() >> 8) / 16777216.0f; };
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    long checked = 0, refused = 0, kept3 = 0, keptPx = 0;
    for (int it = 0; it < 6000; ++it) {
        const int nCam = 1 << upto(3), subCols = 1 + upto(9), rows = 1 + upto(8), width = nCam * subCols, pad = upto(3);
        const int type = upto(2);
        const size_t px = type == 0 ? 2 : 4;
        const size_t pitch = (size_t)(width + pad) * px;
        // the buffer ends with the last pixel of the last row: nothing behind it may be read
        std::vector<unsigned char>* heap = new std::vector<unsigned char>(pitch * (size_t)(rows - 1) + (size_t)width * px);
        std::vector<Sub> subs((size_t)nCam);
        for (Sub& s : subs) { s.cols = subCols; s.rows = rows; s.m.assign((size_t)subCols * rows, 0.0f); }
        const float base = 1.0f + 3.0f * unit();
        for (int v = 0; v < rows; ++v)
            for (int u = 0; u < width + pad; ++u) {
                if (v == rows - 1 && u >= width) break;
                const int kind = upto(12);
                float metres = base * (1.0f + 0.03f * (unit() - 0.5f));
                unsigned char* at = heap->data() + (size_t)v * pitch + (size_t)u * px;
                if (type == 0) {
                    uint16_t p = kind == 0 ? 0 : kind == 1 ? 65535 : (uint16_t)(metres * 1000.0f);
                    std::memcpy(at, &p, 2);
                    metres = (p == 0 || p == 65535) ? 0.0f : float(p) * 0.001f;
                } else {
                    if (kind == 0) metres = 0.0f; else if (kind == 1) metres = nan; else if (kind == 2) metres = inf; else if (kind == 3) metres = -metres;
                    std::memcpy(at, &metres, 4);
                }
                if (u < width) subs[(size_t)(u / subCols)].m[(size_t)v * subCols + u % subCols] = metres;
            }
        std::vector<DepthCamera> cams((size_t)nCam);
        const int iw = upto(3) == 0 ? 0 : 1 + upto(3 * subCols), ih = upto(3) == 0 ? 0 : 1 + upto(3 * rows);
        for (DepthCamera& C : cams) {
            C.fx = 1.0f + 10.0f * unit(); C.fy = 1.0f + 10.0f * unit();
            C.cx = upto(5) == 0 ? 0.0f : subCols * unit(); C.cy = upto(5) == 0 ? -1.0f : rows * unit();
            C.imageWidth = iw; C.imageHeight = ih; C.hasLocalTransform = upto(2) == 1;
            for (float& t : C.localTransform) t = 2.0f * unit() - 1.0f;
        }
        DepthImage image;
        image.data = heap->data(); image.pitchBytes = (int64_t)pitch; image.width = width; image.height = rows; image.type = type;
        const float sx = iw > 0 ? (float)iw / subCols : 1.0f, sy = ih > 0 ? (float)ih / rows : 1.0f;
        const int n = upto(24);
        const bool wild = upto(6) == 0;
        std::vector<float> pts((size_t)n * 2);
        for (int i = 0; i < n; ++i) {
            const int k = upto(10);
            float x = (width + (wild ? 3.0f : 1.5f)) * unit() - 1.6f, y = (rows + 3.0f) * unit() - 1.6f;
            if (k < 3) { x = std::floor(x * 2.0f) / 2.0f; y = std::floor(y * 2.0f) / 2.0f; }
            if (k == 3) x = (float)(upto(nCam) * subCols) - 0.5f * upto(3) + (upto(2) ? (float)subCols - 0.5f : 0.0f);
            if (k == 4) y = (float)rows - 0.5f * upto(3);
            if (wild && k == 5) { const float w[] = {nan, inf, -inf, 1e20f, -1e20f, 3e9f}; (upto(2) ? x : y) = w[upto(6)]; }
            pts[(size_t)i * 2] = x * sx; pts[(size_t)i * 2 + 1] = y * sy;
        }
        const float minDepth = upto(4) == 0 ? -1.0f : base * 0.98f * (float)upto(2), maxDepth = upto(3) == 0 ? 0.0f : base * 1.01f;
        // ---- generateKeypoints3DDepth
        std::vector<float> got((size_t)n * 3, -7.0f), want((size_t)n * 3);
        bool defined = true;
        for (int i = 0; i < n && defined; ++i) defined = naivePoint(subs, cams, pts[(size_t)i * 2], pts[(size_t)i * 2 + 1], minDepth, maxDepth, &want[(size_t)i * 3]);
        const bool ok = Keypoints3D::generateKeypoints3DDepth(pts.data(), n, image, cams.data(), nCam, minDepth, maxDepth, got.data());
        if (ok != defined) { std::printf("case %d: refused %d, the restatement %d\n", it, !ok, !defined); return 1; }
        if (ok && !sameBits(got.data(), want.data(), got.size())) { std::printf("case %d: points differ\n", it); return 1; }
        if (!ok) { for (float g : got) if (g != -7.0f) { std::printf("case %d: written although refused\n", it); return 1; } ++refused; }
        // ---- the 3-D filter
        if (ok) {
            std::vector<int> kept, wantKept;
            const bool boundsOk = minDepth >= 0.0f && (maxDepth <= 0.0f || maxDepth > minDepth);
            if (Keypoints3D::filterKeypointsByDepth(got.data(), n, minDepth, maxDepth, kept) != boundsOk) { std::printf("case %d: bounds\n", it); return 1; }
            if (boundsOk) {
                volatile float mn = minDepth * minDepth, mx = maxDepth * maxDepth;
                for (int i = 0; i < n; ++i) {
                    const float* p = &want[(size_t)i * 3];
                    if (!(std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]))) continue;
                    volatile float xx = p[0] * p[0], yy = p[1] * p[1], zz = p[2] * p[2];
                    volatile float d2 = xx + yy;
                    d2 = d2 + zz;
                    if (d2 >= mn && (mx == 0.0f || d2 <= mx)) wantKept.push_back(i);
                }
                if (kept != wantKept) { std::printf("case %d: the 3-D filter differs\n", it); return 1; }
                kept3 += (long)kept.size();
            }
        }
        // ---- the pixel filter: the whole image, no factors, no clamp
        {
            std::vector<int> kept, wantKept;
            bool pxDefined = minDepth >= 0.0f && (maxDepth <= 0.0f || maxDepth > minDepth);
            for (int i = 0; i < n && pxDefined; ++i) {
                volatile float fu = pts[(size_t)i * 2] + 0.5f, fv = pts[(size_t)i * 2 + 1] + 0.5f;
                if (!intOk(fu) || !intOk(fv)) { pxDefined = false; break; }
                const int u = int(fu), v = int(fv);
                if (!(u >= 0 && u < width && v >= 0 && v < rows)) continue;
                float d;
                const unsigned char* at = heap->data() + (size_t)v * pitch + (size_t)u * px;
                if (type == 0) { uint16_t p; std::memcpy(&p, at, 2); volatile float m = float(p) * 0.001f; d = m; } else std::memcpy(&d, at, 4);
                if (std::isfinite(d) && d > minDepth && (maxDepth <= 0.0f || d < maxDepth)) wantKept.push_back(i);
            }
            if (Keypoints3D::filterKeypointsByDepth(pts.data(), n, image, minDepth, maxDepth, kept) != pxDefined) { std::printf("case %d: the pixel filter's refusal\n", it); return 1; }
            if (pxDefined && kept != wantKept) { std::printf("case %d: the pixel filter differs\n", it); return 1; }
            keptPx += (long)kept.size();
        }
        checked += n;
        delete heap;
    }
    // what makes no image is refused, not read
    {
        float p[2] = {0.0f, 0.0f}, out[3];
        uint16_t one = 1000;
        DepthCamera C = {1, 1, 0, 0, 0, 0, false, {0}};
        std::vector<int> kept;
        DepthImage bad[] = {{nullptr, 2, 1, 1, 0}, {&one, 1, 1, 1, 0}, {&one, 2, 0, 1, 0}, {&one, 2, 1, 0, 0}, {&one, 2, 1, 1, 2}, {&one, 2, 1, 1, 1}};
        for (const DepthImage& d : bad)
            if (Keypoints3D::generateKeypoints3DDepth(p, 1, d, &C, 1, 0, 0, out)) { std::printf("an impossible image was accepted\n"); return 1; }
        DepthImage good = {&one, 2, 1, 1, 0};
        if (Keypoints3D::generateKeypoints3DDepth(p, 1, good, &C, 2, 0, 0, out) || Keypoints3D::generateKeypoints3DDepth(p, 1, good, nullptr, 1, 0, 0, out) ||
            Keypoints3D::generateKeypoints3DDepth(p, -1, good, &C, 1, 0, 0, out)) { std::printf("impossible cameras were accepted\n"); return 1; }
        if (!Keypoints3D::generateKeypoints3DDepth(p, 1, good, &C, 1, 0, 0, out) || out[2] != 1000 * 0.001f) { std::printf("the 1 x 1 image\n"); return 1; }
    }
    if (refused < 100 || kept3 < 1000 || keptPx < 1000) { std::printf("the cases do not cover: %ld refused, %ld / %ld kept\n", refused, kept3, keptPx); return 1; }
    std::printf("ok: %ld keypoints, %ld calls refused, %ld and %ld kept\n", checked, refused, kept3, keptPx);
    return 0;
}
