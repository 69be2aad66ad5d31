// LaneSum.h -- the summation order the motion rules share (include/lcd.h, lcd_estimate_motion_3d step 4), for the host mirrors.
#pragma once

namespace rtabmap_amd {

// the sum of e(0) .. e(n - 1): lane l of LANES adds the elements l, l + LANES, ... in ascending order from +0, then a halving tree
template <int LANES, class F>
float laneTreeSum(int n, F e) {
    float part[LANES];
    for (int l = 0; l < LANES; ++l) part[l] = 0.0f;
    for (int i = 0; i < n; ++i) part[i % LANES] = part[i % LANES] + e(i);
    for (int s = LANES / 2; s >= 1; s >>= 1)
        for (int l = 0; l < s; ++l) part[l] = part[l] + part[l + s];
    return part[0];
}

}  // namespace rtabmap_amd
