// MotionBA.h -- the two-view bundle adjustment behind the visual registration's motion estimate (RegistrationVis.cpp:1873-2188 with
// Vis/BundleAdjustment = 1, the reference's default; OptimizerG2O::optimizeBA, OptimizerG2O.cpp:1429-2117) over the project's minimal types: the
// entry that hands the PnP's result to the engine (lcd_refine_motion_ba), and motion_ba_cpu, the whole rule of include/lcd.h as plain host code
// for a process without a device.  The arithmetic is the engine's own (csrc/motion_ba_rule.h, compiled here for the host), so a pair gets the
// same bits with and without a device.  tools/sanitize_motion_ba.cpp drives motion_ba_cpu under the host sanitizers.
#pragma once
#include <stdint.h>
#include <map>
#include <vector>

#include "../../include/lcd.h"
#include "Motion2D.h"

namespace rtabmap_amd {

struct MotionBAParams {
    double pixelVariance = 1.0, robustDelta = 8.0;      // g2o/PixelVariance, g2o/RobustKernelDelta
    int iterations = 20, minInliers = 20;               // Optimizer/Iterations, Vis/MinInliers
    float maxInliersMeanDistance = 0.0f, minInliersDistribution = 0.0f;   // Vis/MeanInliersDistance, Vis/MinInliersDistribution
    double baselineFrom = 0.075, baselineTo = 0.075;    // the stereo models' baselines, or g2o/Baseline; <= 0: mono edges only
};

struct MotionBAResult {
    float transform[12];                 // twelve zeros: no transform
    int status;                          // lcd_motion_ba_status
    int nOutliers, lmAccepted;
    double chi2Before, chi2After;
    float inliersMeanDistance, inliersDistribution;
    std::vector<int> inliers;            // the surviving ids, in input order
};

// The rule on the CPU: one pair of frames as parallel arrays (from: ids, [n x 3] points, [n x 2] keypoints or null; to: ids, [n x 2]
// keypoints, [n x 3] points or null), the PnP's inliers and transform, priorVariance: linear and angular, or null (identity information).
// false (out untouched): what lcd_refine_motion_ba refuses.
bool motion_ba_cpu(const int32_t* fromIds, const float* fromXyz, const float* fromPoints, int nFrom, const int32_t* toIds, const float* toPoints,
                   const float* toXyz, int nTo, const int32_t* inliers, int nInliers, const float* transform, const double* priorVariance,
                   const lcd_camera& cameraFrom, const lcd_camera& cameraTo, const MotionBAParams& params, MotionBAResult& out);

// what the reference's RegistrationInfo carries out of the step
struct MotionBAInfo {
    int status = 0;
    float inliersMeanDistance = 0.0f, inliersDistribution = 0.0f;
};

class MotionBA {
public:
    // RegistrationVis.cpp:1873-2188 for one link: `transform`, `inliers` and the covariance's inputs as Motion2D::estimateMotion3DTo2D (or
    // lcd_estimate_motion_pnp) left them.  The angular prior variance is 2.1981 x acos(angleCos), as motion_pnp_covariance has it; varianceKind
    // 0 means identity information.  kptsA may be empty (the reference's empty getWordsKpts()), words3B may be empty.  Returns the refined
    // transform (null when rejected, or when the engine refuses the call) and replaces `inliers` by the survivors.
    static Transform3D refine(lcd_engine* engine, const std::multimap<int, Point3f>& words3A, const std::multimap<int, Point2f>& kptsA,
                              const std::multimap<int, Point2f>& kptsB, const std::multimap<int, Point3f>& words3B, const lcd_camera& cameraFrom,
                              const lcd_camera& cameraTo, const Transform3D& transform, std::vector<int>& inliers, int varianceKind, double varianceLin,
                              double angleCos, const MotionBAParams& params, MotionBAInfo* info = nullptr);
};

}  // namespace rtabmap_amd
