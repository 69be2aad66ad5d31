// RegistrationIcp.h -- RegistrationIcp::computeTransformationImpl with Icp/Strategy = 0: the point-to-point branch (RegistrationIcp.cpp:662-971) and
// the point-to-plane branch with its complexity test and low-complexity fallback (:506-661, :785-853),
// over the project's minimal types: the entry that hands the work to the engine (lcd_register_icp) and applies what the rule leaves to the
// host (the Icp/MaxTranslation / Icp/MaxRotation gate over Euler angles, variance /= 10, the covariance), and register_icp_cpu, the whole rule
// of include/lcd.h as plain host code for a process without a device.  The arithmetic is the engine's own (csrc/icp_rule.h, compiled here for
// the host), so a pair gets the same bits with and without a device.  tools/sanitize_register_icp.cpp drives register_icp_cpu under the host
// sanitizers.
#pragma once
#include <stdint.h>
#include <string>
#include <vector>

#include "Motion3D.h"

struct lcd_engine;

namespace rtabmap_amd {

struct IcpResult {
    float transform[12];                 // twelve zeros: no transform
    float icpTransform[12];              // F: source onto target
    float correction[12];                // guess^-1 x F^-1 x guess
    int status, stop, iterations;        // lcd_icp_status, lcd_icp_stop
    int correspondences;
    float ratio;
    double variance;                     // undivided
    std::vector<int> match;              // per from-row: the to-row it is kept with, or -1
};

// The rule on the CPU: one pair of scans as [n x 3] rows.  false (out untouched): what the entry refuses -- deviceEntry chooses whose
// refusals: lcd_register_icp's (a row that is not finite is refused) or lcd_register_icp_dev's (such a row takes no part).
bool register_icp_cpu(const float* fromXyz, int nFrom, const float* toXyz, int nTo, const float guess[12], int maxIterations, bool force3DoF,
                      int maxLaserScans, double maxCorrespondenceDistance, float epsilon, float correspondenceRatio, int search, bool deviceEntry,
                      IcpResult& out);

struct IcpPlaneResult : IcpResult {        // lcd_register_icp_plane's further outputs
    int branch = 0;                      // 0 = point to plane, 1 = point-to-point fallback
    float complexity = 0.0f, complexityValues[3] = {0, 0, 0}, complexityVectors[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, secondEigenvalue = 1.0f;
};

// The rule of lcd_register_icp_plane on the CPU (csrc/icp_plane_rule.h compiled for the host): one pair of 3-D scans with normals as [n x 3]
// rows.  false (out untouched): what the entry refuses; deviceEntry as above.  A normal that is not finite is legal on both entries.
// tools/sanitize_register_icp_plane.cpp drives it under the host sanitizers.
bool register_icp_plane_cpu(const float* fromXyz, const float* fromNormals, int nFrom, const float* toXyz, const float* toNormals, int nTo,
                            const float guess[12], int maxIterations, bool force3DoF, int maxLaserScans, double maxCorrespondenceDistance, float epsilon,
                            float correspondenceRatio, float minComplexity, int lowComplexityStrategy, bool normalGate, double minNormalCos, int search,
                            bool deviceEntry, IcpPlaneResult& out);

// The grid form's cell of each of n coordinates under a correspondence distance, INT_MIN where a coordinate does not fit the key's cell range;
// returns the cell size.  What the tests prove the one-cell margin of the grid with.
float icp_cells(const float* x, int n, double maxCorrespondenceDistance, int* outCells);

struct RegistrationInfoIcp {             // the fields of RegistrationInfo that the ICP step fills
    float icpTranslation = 0.0f, icpRotation = 0.0f, icpInliersRatio = 0.0f, icpStructuralComplexity = 0.0f;
    int icpCorrespondences = 0;
    double covariance[36];               // row-major 6 x 6; the identity until a variance is known
    std::string rejectedMsg;
    RegistrationInfoIcp() { for (int k = 0; k < 36; ++k) covariance[k] = k % 7 == 0 ? 1.0 : 0.0; }
};

struct FilteredScans {                   // what the filters in front handed to the ICP
    std::vector<Point3f> fromScan, fromNormals, toScan, toNormals;
    int maxLaserScans = 0;
};

class RegistrationIcpHip {
public:
    int maxIterations = 30;                      // Icp/Iterations
    float maxTranslation = 0.2f;                 // Icp/MaxTranslation, 0 = off
    float maxRotation = 0.78f;                   // Icp/MaxRotation, 0 = off
    double maxCorrespondenceDistance = 0.1;      // Icp/MaxCorrespondenceDistance
    float epsilon = 0.0f;                        // Icp/Epsilon
    float correspondenceRatio = 0.1f;            // Icp/CorrespondenceRatio
    bool force3DoF = false;                      // Reg/Force3DoF
    bool pointToPlane = true;                    // Icp/PointToPlane
    float pointToPlaneMinComplexity = 0.02f;     // Icp/PointToPlaneMinComplexity
    int pointToPlaneLowComplexityStrategy = 1;   // Icp/PointToPlaneLowComplexityStrategy
    int filtersEnabled = 3;                      // Icp/FiltersEnabled: 1 = the from-scan, 2 = the to-scan
    int downsamplingStep = 1;                    // Icp/DownsamplingStep
    float rangeMin = 0.0f, rangeMax = 0.0f;      // Icp/RangeMin, Icp/RangeMax
    float voxelSize = 0.05f;                     // Icp/VoxelSize
    int pointToPlaneK = 5;                       // Icp/PointToPlaneK
    float pointToPlaneRadius = 0.0f;             // Icp/PointToPlaneRadius
    float pointToPlaneGroundNormalsUp = 0.0f;    // Icp/PointToPlaneGroundNormalsUp

    // The reference's shape: both scans as point rows in their base frames, the guess, the scan's maximum number of points (0: the ratio is
    // relative).  A null transform when the registration is rejected (info.rejectedMsg says why) or the engine refuses the call.
    Transform3D computeTransformation(lcd_engine* engine, const std::vector<Point3f>& fromScan, const std::vector<Point3f>& toScan, const Transform3D& guess,
                                      int maxLaserScans, RegistrationInfoIcp& info) const;
    // The same with the scans' normals (empty: the scan has none) and whether a scan is 2-D: with Icp/PointToPlane, two 3-D scans and normals on
    // both sides the work goes to lcd_register_icp_plane (the complexity test, point to plane or the low-complexity fallback; the gate's
    // cosine is cos(Icp/MaxRotation)) and info.icpStructuralComplexity is filled; every other pair goes to the call above, as RegistrationIcp.cpp:510-524 does.
    Transform3D computeTransformation(lcd_engine* engine, const std::vector<Point3f>& fromScan, const std::vector<Point3f>& fromNormals, bool fromIs2d,
                                      const std::vector<Point3f>& toScan, const std::vector<Point3f>& toNormals, bool toIs2d, const Transform3D& guess,
                                      int maxLaserScans, RegistrationInfoIcp& info) const;
    // The same over RAW scans (RegistrationIcp.cpp:362-447): the sides filtersEnabled names go through lcd_filter_scans in one call (two when
    // one scan is 2-D and the other is not) with K, radius and ground-up passed as 0 without pointToPlane (:374-376) or for a 2-D scan (2-D
    // normals are out of scope); a scan the filter leaves with a status other than LCD_SCAN_OK is empty.  maxLaserScansFrom / To are the
    // reference's: maxPoints when > 0 else the raw size, times float(filtered size) / float(raw size) for a filtered side; the ratio is
    // relative to the to-side's when it is not 0, else the from-side's (:879).  Then the overload above.  `filtered`, when given, receives what
    // the ICP was handed.
    Transform3D computeTransformation(lcd_engine* engine, const std::vector<Point3f>& fromScan, bool fromIs2d, int fromMaxPoints, const std::vector<Point3f>& toScan,
                                      bool toIs2d, int toMaxPoints, const Transform3D& guess, RegistrationInfoIcp& info, struct FilteredScans* filtered = nullptr) const;
    // RegistrationIcp.cpp:856-961 behind the rule: what computeTransformation does with the engine's (or register_icp_cpu's) result
    Transform3D finish(const IcpResult& r, RegistrationInfoIcp& info) const;
};

}  // namespace rtabmap_amd
