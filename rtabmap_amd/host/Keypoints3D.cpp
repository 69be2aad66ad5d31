// Keypoints3D.cpp -- see Keypoints3D.h.
#include "Keypoints3D.h"

#include "../csrc/keypoints_3d_rule.h"

namespace rtabmap_amd {

namespace {

namespace rule = lcd::kp3d;

bool makeImage(const DepthImage& d, int nCameras, rule::Image& im) {
    if (!d.data || d.width < 1 || d.height < 1 || nCameras < 1 || d.width % nCameras) return false;
    if (d.type != rule::DEPTH_U16_MM && d.type != rule::DEPTH_F32_M) return false;
    const int64_t px = d.type == rule::DEPTH_U16_MM ? 2 : 4;
    if (d.pitchBytes < (int64_t)d.width * px || d.pitchBytes % px || (uintptr_t)d.data % (uintptr_t)px) return false;
    im.data = (const unsigned char*)d.data; im.pitch = d.pitchBytes;
    im.width = d.width; im.height = d.height; im.type = d.type; im.n_cameras = nCameras;
    return true;
}

bool boundsOk(float minDepth, float maxDepth) {
    return minDepth >= 0.0f && (maxDepth <= 0.0f || maxDepth > minDepth);      // NaN bounds fail the first comparison or pass neither
}

}  // namespace

bool Keypoints3D::generateKeypoints3DDepth(const float* points, int n, const DepthImage& depth, const DepthCamera* cameras, int nCameras,
                                           float minDepth, float maxDepth, float* xyz) {
    rule::Image im;
    if (n < 0 || !cameras || !makeImage(depth, nCameras, im) || minDepth != minDepth || maxDepth != maxDepth) return false;
    rule::set_factors(im, cameras[0].imageWidth, cameras[0].imageHeight);
    std::vector<rule::Camera> cams((size_t)nCameras);
    for (int c = 0; c < nCameras; ++c) {
        rule::Camera& C = cams[(size_t)c];
        C.cx = cameras[c].cx * im.factor_x; C.cy = cameras[c].cy * im.factor_y; C.fx = cameras[c].fx * im.factor_x; C.fy = cameras[c].fy * im.factor_y;
        for (int k = 0; k < 12; ++k) C.t[k] = cameras[c].localTransform[k];
        C.has_t = cameras[c].hasLocalTransform ? 1 : 0; C.pad[0] = C.pad[1] = C.pad[2] = 0;
    }
    std::vector<float> result((size_t)n * 3);
    for (int i = 0; i < n; ++i)
        if (!rule::point_of(im, cams.data(), points[2 * i], points[2 * i + 1], minDepth, maxDepth, &result[(size_t)i * 3])) return false;
    for (size_t k = 0; k < result.size(); ++k) xyz[k] = result[k];
    return true;
}

bool Keypoints3D::filterKeypointsByDepth(const float* xyz, int n, float minDepth, float maxDepth, std::vector<int>& kept) {
    if (n < 0 || !boundsOk(minDepth, maxDepth)) return false;
    std::vector<int> result;
    for (int i = 0; i < n; ++i) if (rule::keep_3d(xyz + (size_t)i * 3, minDepth, maxDepth)) result.push_back(i);
    kept.swap(result);
    return true;
}

bool Keypoints3D::filterKeypointsByDepth(const float* points, int n, const DepthImage& depth, float minDepth, float maxDepth, std::vector<int>& kept) {
    rule::Image im;
    if (n < 0 || !boundsOk(minDepth, maxDepth) || !makeImage(depth, 1, im)) return false;
    rule::set_factors(im, 0, 0);
    std::vector<int> result;
    for (int i = 0; i < n; ++i) {
        bool defined;
        const bool keep = rule::keep_pixel(im, points[2 * i], points[2 * i + 1], minDepth, maxDepth, &defined);
        if (!defined) return false;
        if (keep) result.push_back(i);
    }
    kept.swap(result);
    return true;
}

}  // namespace rtabmap_amd
