// Motion2D.h -- util3d::estimateMotion3DTo2D (util3d_motion_estimation.cpp:59-289, RegistrationVis.cpp:1676-1819 with Vis/EstimationType = 1,
// the reference's default) over the project's minimal types: the entry that hands the work to the engine (lcd_estimate_motion_pnp), and
// motion_pnp_cpu, the whole rule of include/lcd.h as plain host code for a process without a device.  The arithmetic is the engine's own
// (csrc/motion_pnp_rule.h, compiled here for the host), so a pair gets the same bits with and without a device.
// tools/sanitize_motion_pnp.cpp drives motion_pnp_cpu under the host sanitizers.
#pragma once
#include <stdint.h>
#include <map>
#include <vector>

#include "../../include/lcd.h"
#include "Motion3D.h"

namespace rtabmap_amd {

struct Point2f { float x, y; };

struct MotionPnpParams {
    int minInliers = 20, iterations = 100, refineIterations = 1, varianceMedianRatio = 4;
    double reprojError = 2.0;
    float maxVariance = 0.0f;
    uint32_t seed = 0;
    int steps = 0;                       // 0 = the rule's Gauss-Newton step count; another value is for measuring how it was chosen and is not the rule
};

struct MotionPnpResult {
    float transform[12];                 // twelve zeros: no transform
    int status;                          // lcd_motion_pnp_status
    int varianceKind;                    // 0 none, 1 linear + cosine, 2 RMS reprojection in varianceLin
    double varianceLin, angleCos;
    std::vector<int> matches;            // the correspondences' ids, ascending
    std::vector<int> inliers;            // the inliers' ids, in correspondence order
};

// The rule on the CPU: one pair of frames as parallel arrays (from: ids, [n x 3] points; to: ids, [n x 2] pixels, [n x 3] points or null).
// guess: 12 floats or null (identity).  false (out untouched): what lcd_estimate_motion_pnp refuses.
bool motion_pnp_cpu(const int32_t* fromIds, const float* fromXyz, int nFrom, const int32_t* toIds, const float* toPoints, const float* toXyz, int nTo,
                    const lcd_camera& camera, const float* guess, const MotionPnpParams& params, MotionPnpResult& out);

// the 6 x 6 covariance (36 doubles, row-major) of util3d_motion_estimation.cpp:227-231 / :270 from what the rule returns
void motion_pnp_covariance(int varianceKind, double varianceLin, double angleCos, double* covariance);

class Motion2D {
public:
    // The reference's signature; the word maps are multimaps as RegistrationVis holds them (uMultimapToMapUnique is part of the call,
    // RegistrationVis.cpp:1704-1720).  words3B may be empty.  covariance: 36 doubles or null, like matchesOut and inliersOut.  A null
    // transform also when the engine refuses the call (lcd_last_error tells why).
    static Transform3D estimateMotion3DTo2D(lcd_engine* engine, const std::multimap<int, Point3f>& words3A, const std::multimap<int, Point2f>& words2B,
                                            const lcd_camera& camera, int minInliers, int iterations, double reprojError, int refineIterations,
                                            int varianceMedianRatio, float maxVariance, const Transform3D& guess,
                                            const std::multimap<int, Point3f>& words3B, double* covariance, std::vector<int>* matchesOut,
                                            std::vector<int>* inliersOut, uint32_t seed = 0);
};

}  // namespace rtabmap_amd
