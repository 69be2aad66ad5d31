// Stereo.h -- the stereo stage of Feature2D::generateKeypoints3D (Features2d.cpp:960-1016 with Stereo/OpticalFlow = true) as plain host code,
// for a process without a device: StereoOpticalFlow::computeCorrespondences (util2d::calcOpticalFlowPyrLKStereo behind the engine's own
// pyramid and Scharr derivative), updateStatus and util3d::generateKeypoints3DStereo by the rule include/lcd.h writes down for
// lcd_keypoints_3d_stereo.  The arithmetic is the engine's own (csrc/stereo_flow_rule.h, compiled here for the host), so a frame gets the same
// bits with and without a device.  tools/sanitize_stereo.cpp drives it under the host sanitizers.
#pragma once
#include <stdint.h>
#include <vector>

namespace rtabmap_amd {

struct StereoCamera {                    // what the rule reads of a StereoCameraModel
    double fx, fy, cx, cy;               // the left model
    double rightCx;
    double baseline;
    bool hasLocalTransform;              // !localTransform().isNull() && !localTransform().isIdentity()
    float localTransform[12];            // row-major 3 x 4
};

struct GrayImage {                       // CV_8UC1
    const unsigned char* data;
    int64_t pitchBytes;
    int width, height;
};

struct StereoParams {                    // the reference's defaults
    int winWidth = 15, winHeight = 3;    // Stereo/WinWidth, Stereo/WinHeight
    int maxLevel = 5;                    // Stereo/MaxLevel
    int iterations = 30;                 // Stereo/Iterations
    double eps = 0.01;                   // Stereo/Eps
    bool useMinEigenVals = true;
    double minEigThreshold = 1e-4;
    double errorThreshold = 50.0;
    float minDisparity = 0.5f, maxDisparity = 128.0f;   // Stereo/MinDisparity, Stereo/MaxDisparity
};

class StereoOpticalFlowHip {
public:
    explicit StereoOpticalFlowHip(const StereoParams& params = StereoParams()) : _p(params) {}
    const StereoParams& params() const { return _p; }
    // true where the engine's lcd_keypoints_3d_stereo would accept the parameters
    bool valid() const;

    // leftCorners, rightCorners: x, y per keypoint; status: [n], behind updateStatus.  false (nothing written): parameters or images the
    // engine refuses, or a keypoint that is not finite or beyond int
    bool computeCorrespondences(const GrayImage& left, const GrayImage& right, const float* leftCorners, int n, float* rightCorners,
                                unsigned char* status) const;
    // the disparity gate alone; err: NULL, or [n] the L1 errors (useMinEigenVals == false)
    void updateStatus(const float* leftCorners, const float* rightCorners, int n, unsigned char* status, const float* err) const;
    // xyz: [n x 3], three quiet NaNs where a keypoint has no point in range; status may be NULL (every keypoint counts).  false: baseline or
    // fx not > 0, a NaN among the camera's values or the bounds
    static bool generateKeypoints3DStereo(const float* leftCorners, const float* rightCorners, int n, const StereoCamera& camera,
                                          const unsigned char* status, float minDepth, float maxDepth, float* xyz);

    // the pyramid of one image by the engine's rule: levels[l] is widths[l] x heights[l], rows packed.  false: an image that is not larger than the window
    static bool buildPyramid(const GrayImage& image, int winWidth, int winHeight, int maxLevel, std::vector<std::vector<unsigned char> >& levels,
                             std::vector<int>& widths, std::vector<int>& heights);
    // the Scharr derivative of one image at every pixel: dxdy [height x width x 2] shorts
    static void derivative(const GrayImage& image, short* dxdy);

private:
    StereoParams _p;
};

}  // namespace rtabmap_amd
