// MotionMono.h -- util3d::generateWords3DMono behind RegistrationVis' Vis/EstimationType = 2 (reference util3d_features.cpp:209-413,
// RegistrationVis.cpp:1584-1675) over the project's minimal types: the class that hands the estimate to the engine (lcd_estimate_motion_mono),
// and motion_mono_cpu, the whole rule of include/lcd.h as plain host code for a process without a device.  The arithmetic is the engine's own
// (csrc/motion_mono_rule.h, compiled here for the host), so a pair gets the same bits with and without a device.
// tools/sanitize_motion_mono.cpp drives motion_mono_cpu under the host sanitizers.
#pragma once
#include <stdint.h>
#include <vector>

#include "../../include/lcd.h"
#include "VWDictionaryHip.h"

namespace rtabmap_amd {

struct MotionMonoParams {
    int minInliers = 20;                 // Vis/MinInliers (Parameters.h)
    int iterations = 1000;               // every candidate is scored: the confidence 0.99 has no effect on the engine's rule
    uint32_t seed = 0;
    double reprojThreshold = 2.0;        // Vis/PnPReprojError, pixels
    int varianceMedianRatio = 4;         // Vis/PnPVarianceMedianRatio, used as a shift
    float maxVariance = 0.1f;            // Vis/EpipolarGeometryVar
    double distanceThreshold = 50.0;     // recoverPose's distanceThresh (util3d_features.cpp:268)
    float fx = 0.0f, fy = 0.0f, cx = 0.0f, cy = 0.0f;
    bool hasLocalTransform = false;
    float localTransform[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    bool hasGuess = false;               // cameraTransform on entry; a NaN or twelve zeros count as null
    float guess[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
};

struct MotionMonoResult {
    float transform[12];                 // twelve zeros: none
    int status;                          // lcd_motion_mono_status
    double variance;
    std::vector<int> matches;            // the pairs' ids, ascending
    std::vector<int> inliers;            // the inliers' ids, in correspondence order
    std::vector<float> points3;          // [inliers x 3] their triangulated points, base frame, scaled
};

// The rule on the CPU: one pair of signatures as parallel arrays (ids, [n x 2] keypoints, optional [nFrom x 3] words3).  false (out untouched):
// what lcd_estimate_motion_mono refuses.
bool motion_mono_cpu(const int32_t* fromIds, const float* fromPoints, const float* fromPoints3, int nFrom, const int32_t* toIds, const float* toPoints,
                     int nTo, const MotionMonoParams& params, MotionMonoResult& out);

class MotionMonoHip {
public:
    explicit MotionMonoHip(const ParametersMap& parameters = ParametersMap());
    void parseParameters(const ParametersMap& parameters);   // Vis/MinInliers, Vis/PnPReprojError, Vis/PnPVarianceMedianRatio, Vis/EpipolarGeometryVar

    // generateWords3DMono and the gates of RegistrationVis.cpp:1636-1667 over the engine; false when the engine refuses the call.  camera: fx,
    // fy, cx, cy and the local transform; points3A may be empty; guess: NULL or 12 floats.
    bool estimate(lcd_engine* engine, const std::vector<int>& wordIdsA, const std::vector<float>& pointsA, const std::vector<float>& points3A,
                  const std::vector<int>& wordIdsB, const std::vector<float>& pointsB, const lcd_camera& camera, const float* guess,
                  MotionMonoResult& out, uint32_t seed = 0) const;

    int getMinInliers() const { return _minInliers; }
    double getReprojThreshold() const { return _reprojThreshold; }
    int getVarianceMedianRatio() const { return _varianceMedianRatio; }
    float getMaxVariance() const { return _maxVariance; }
    void setMinInliers(int v) { _minInliers = v; }
    void setReprojThreshold(double v) { _reprojThreshold = v; }
    void setVarianceMedianRatio(int v) { _varianceMedianRatio = v; }
    void setMaxVariance(float v) { _maxVariance = v; }

private:
    int _minInliers;
    double _reprojThreshold;
    int _varianceMedianRatio;
    float _maxVariance;
};

}  // namespace rtabmap_amd
