// Motion3D.h -- util3d::estimateMotion3DTo3D (util3d_motion_estimation.cpp:730-807, RegistrationVis.cpp:1823-1871 with Vis/EstimationType = 0)
// over the project's minimal types: the entry that hands the work to the engine (lcd_estimate_motion_3d), and motion3d_cpu, the whole rule of
// include/lcd.h as plain host code for a process without a device.  The arithmetic is the engine's own (csrc/motion_3d_rule.h, compiled here
// for the host), so a pair gets the same bits with and without a device.  tools/sanitize_motion_3d.cpp drives motion3d_cpu under the host
// sanitizers.
#pragma once
#include <stdint.h>
#include <map>
#include <vector>

struct lcd_engine;

namespace rtabmap_amd {

struct Point3f { float x, y, z; };

struct Transform3D {                     // row-major 3 x 4; all zero = Transform::isNull()
    float data[12];
    Transform3D() { for (int k = 0; k < 12; ++k) data[k] = 0.0f; }
    bool isNull() const { for (int k = 0; k < 12; ++k) if (data[k] != 0.0f) return false; return true; }
};

struct Motion3DResult {
    float transform[12];                 // twelve zeros: no transform
    int status;                          // lcd_motion_3d_status
    double variance;
    std::vector<int> matches;            // the correspondences' ids, ascending
    std::vector<int> inliers;            // the inliers' ids, in correspondence order
};

// The rule on the CPU: one pair of frames as parallel arrays (ids, [n x 3] points).  false (out untouched): what lcd_estimate_motion_3d
// refuses.  sweeps: 0 = the rule's Jacobi sweep count; another value is for measuring how the count was chosen and is not the rule.
bool motion3d_cpu(const int32_t* fromIds, const float* fromXyz, int nFrom, const int32_t* toIds, const float* toXyz, int nTo, int minInliers,
                  double inlierDistance, int iterations, int refineIterations, uint32_t seed, Motion3DResult& out, int sweeps = 0);

class Motion3D {
public:
    // The reference's signature; words3A / words3B are multimaps as RegistrationVis holds them (uMultimapToMapUnique is part of the call:
    // an id that occurs twice in a frame takes no part).  covariance: 36 doubles, row-major 6 x 6, = eye x variance; may be null, like
    // matchesOut and inliersOut.  A null transform also when the engine refuses the call (lcd_last_error tells why).
    static Transform3D estimateMotion3DTo3D(lcd_engine* engine, const std::multimap<int, Point3f>& words3A, const std::multimap<int, Point3f>& words3B,
                                            int minInliers, double inliersDistance, int iterations, int refineIterations, double* covariance,
                                            std::vector<int>* matchesOut, std::vector<int>* inliersOut, uint32_t seed = 0);
};

}  // namespace rtabmap_amd
