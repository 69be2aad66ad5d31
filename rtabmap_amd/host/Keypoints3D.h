// Keypoints3D.h -- the depth stage of Memory::createSignature in front of the selection as plain host code, for a process without a device:
// util3d::generateKeypoints3DDepth (util3d_features.cpp:67-120) and both Feature2D::filterKeypointsByDepth overloads (Features2d.cpp:105-212)
// by the rule include/lcd.h writes down for lcd_keypoints_3d.  The arithmetic is the engine's own (csrc/keypoints_3d_rule.h, compiled here for
// the host), so a frame gets the same bits with and without a device.  tools/sanitize_keypoints_3d.cpp drives it under the host sanitizers.
#pragma once
#include <stdint.h>
#include <vector>

namespace rtabmap_amd {

struct DepthCamera {                     // what the rule reads of a CameraModel
    float fx, fy, cx, cy;
    int imageWidth, imageHeight;         // may be 0
    bool hasLocalTransform;              // !localTransform().isNull() && !localTransform().isIdentity()
    float localTransform[12];            // row-major 3 x 4
};

struct DepthImage {
    const void* data;
    int64_t pitchBytes;
    int width, height;
    int type;                            // 0: CV_16UC1 millimetres, 1: CV_32FC1 metres
};

class Keypoints3D {
public:
    // points: x, y per keypoint; xyz: [n x 3], three quiet NaNs where a keypoint has no point in range.  false (nothing written): sizes that make
    // no image, a width that the cameras do not divide, or a keypoint the reference asserts on (not finite, beyond int, in no camera's sub-image)
    static bool generateKeypoints3DDepth(const float* points, int n, const DepthImage& depth, const DepthCamera* cameras, int nCameras,
                                         float minDepth, float maxDepth, float* xyz);
    // the 3-D overload: kept = the indices, ascending, of the points that are finite and in range.  false: minDepth < 0 or 0 < maxDepth <= minDepth
    static bool filterKeypointsByDepth(const float* xyz, int n, float minDepth, float maxDepth, std::vector<int>& kept);
    // the 2-D overload the extractors call: the nearest pixel of the whole image.  false: the bounds as above, or a coordinate that is not
    // finite or beyond int
    static bool filterKeypointsByDepth(const float* points, int n, const DepthImage& depth, float minDepth, float maxDepth, std::vector<int>& kept);
};

}  // namespace rtabmap_amd
