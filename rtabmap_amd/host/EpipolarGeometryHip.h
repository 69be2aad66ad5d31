// EpipolarGeometryHip.h -- rtabmap::EpipolarGeometry (reference EpipolarGeometry.cpp:65-102, :298-379, EpipolarGeometry.h:158-186) over the project's
// minimal types: the class that hands the check to the engine (lcd_verify_epipolar), and epipolar_cpu, the whole rule of include/lcd.h as
// plain host code for a process without a device.  The arithmetic is the engine's own (csrc/epipolar_rule.h, compiled here for the host), so
// a pair gets the same bits with and without a device.  tools/sanitize_epipolar.cpp drives epipolar_cpu under the host sanitizers.
#pragma once
#include <stdint.h>
#include <vector>

#include "../../include/lcd.h"
#include "VWDictionaryHip.h"

namespace rtabmap_amd {

struct EpipolarParams {
    int matchCountMin = 8;               // VhEp/MatchCountMin (Parameters.h)
    double ransacParam1 = 3.0;           // VhEp/RansacParam1: the distance to the epipolar line, pixels
    double ransacParam2 = 0.99;          // VhEp/RansacParam2: the confidence; no effect on the engine's rule (every candidate is scored)
    int iterations = 1000;               // OpenCV's cap for FM_RANSAC
    uint32_t seed = 0;
};

struct EpipolarResult {
    float fundamental[9];                // nine zeros: no model
    int status;                          // lcd_epipolar_status
    std::vector<int> matches;            // the pairs' ids, ascending
    std::vector<int> inliers;            // the inliers' ids, in correspondence order
};

// The rule on the CPU: one pair of signatures as parallel arrays (ids, [n x 2] keypoints).  false (out untouched): what lcd_verify_epipolar refuses.
bool epipolar_cpu(const int32_t* fromIds, const float* fromPoints, int nFrom, const int32_t* toIds, const float* toPoints, int nTo,
                  const EpipolarParams& params, EpipolarResult& out);

class EpipolarGeometryHip {
public:
    explicit EpipolarGeometryHip(const ParametersMap& parameters = ParametersMap());
    void parseParameters(const ParametersMap& parameters);   // VhEp/MatchCountMin, VhEp/RansacParam1, VhEp/RansacParam2

    // EpipolarGeometry::check (:65-102) over the engine: the accept decision; false also when the engine refuses the call
    bool check(lcd_engine* engine, const std::vector<int>& wordIdsA, const std::vector<float>& pointsA, const std::vector<int>& wordIdsB,
               const std::vector<float>& pointsB, uint32_t seed = 0) const;
    // EpipolarGeometry::findFFromWords (:298-379): the matrix (nine zeros: none) and one status byte per pair in ascending id (1 inlier, 0 outlier);
    // pairsOut: the pairs' ids
    bool findFFromWords(lcd_engine* engine, const std::vector<int>& wordIdsA, const std::vector<float>& pointsA, const std::vector<int>& wordIdsB,
                        const std::vector<float>& pointsB, float fundamental[9], std::vector<unsigned char>& status, std::vector<int>* pairsOut = nullptr,
                        int* engineStatus = nullptr, uint32_t seed = 0) const;

    int getMatchCountMinAccepted() const { return _matchCountMin; }
    double getRansacParam1() const { return _ransacParam1; }
    double getRansacParam2() const { return _ransacParam2; }
    void setMatchCountMinAccepted(int v) { _matchCountMin = v; }
    void setRansacParam1(double v) { _ransacParam1 = v; }
    void setRansacParam2(double v) { _ransacParam2 = v; }

private:
    int _matchCountMin;
    double _ransacParam1, _ransacParam2;
};

}  // namespace rtabmap_amd
