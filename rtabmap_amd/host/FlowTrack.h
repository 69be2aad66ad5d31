// FlowTrack.h -- the optical-flow correspondences of RegistrationVis (Vis/CorType = 1, RegistrationVis.cpp:510-780) as plain host code, for a
// process without a device: the 2-D pyramidal Lucas-Kanade tracker and the keep step by the rule include/lcd.h writes down for
// lcd_track_flow.  The arithmetic is the engine's own (csrc/flow_track_rule.h, compiled here for the host), so a pair gets the same bits with
// and without a device.  tools/sanitize_flow.cpp drives it under the host sanitizers.
#pragma once
#include <stdint.h>
#include <vector>

#include "Stereo.h"

namespace rtabmap_amd {

struct FlowParams {                      // the reference's defaults
    int winWidth = 16, winHeight = 16;   // Vis/CorFlowWinSize
    int iterations = 30;                 // Vis/CorFlowIterations
    double eps = 0.01;                   // Vis/CorFlowEps
    bool useMinEigenVals = true;         // Vis/CorFlowUseMinEigenVals
    double minEigThreshold = 1e-4;       // Vis/CorFlowMinEigThreshold
    float errorThreshold = 20.0f;        // Vis/CorFlowErrorThreshold
};

// One pair: the n corners (x, y) of `from` tracked into `to`.  maxLevel: guessSet ? 0 : Vis/CorFlowMaxLevel.  initial: NULL, or [n x 2] the
// start positions (OPTFLOW_USE_INITIAL_FLOW).  outTrack [n x 2], outStatus [n], outErr [n]: calcOpticalFlowPyrLK's outputs by input index
// (each may be NULL); kept: the indices RegistrationVis keeps, ascending.  asDevice: a corner or start position that is not finite or beyond
// int gets status 0 and the track (NaN, NaN), as lcd_track_flow_dev gives it, instead of a refusal.  false (nothing written): parameters or
// images the engine refuses, or (without asDevice) such a corner.
bool flow_track_cpu(const GrayImage& from, const GrayImage& to, int maxLevel, const float* corners, const float* initial, int n, const FlowParams& params,
                    bool asDevice, float* outTrack, unsigned char* outStatus, float* outErr, std::vector<int>& kept);

}  // namespace rtabmap_amd
