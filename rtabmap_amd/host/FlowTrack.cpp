// FlowTrack.cpp -- see FlowTrack.h.
#include "FlowTrack.h"

#include "../csrc/flow_track_rule.h"

namespace rtabmap_amd {

namespace {

namespace rule = lcd::stereo;
namespace flow = lcd::flow;

bool imageOk(const GrayImage& im) { return im.data && im.width >= 2 && im.height >= 2 && im.pitchBytes >= im.width && im.pitchBytes <= 0x7fffffff; }
rule::Level levelOf(const unsigned char* data, int64_t pitch, int w, int h) { return rule::Level{data, (int32_t)pitch, w, h, 0}; }
bool isNan(double v) { return v != v; }

}  // namespace

bool flow_track_cpu(const GrayImage& from, const GrayImage& to, int maxLevel, const float* corners, const float* initial, int n, const FlowParams& p,
                    bool asDevice, float* outTrack, unsigned char* outStatus, float* outErr, std::vector<int>& kept) {
    if (n < 0 || !imageOk(from) || !imageOk(to) || from.width != to.width || from.height != to.height) return false;
    if (p.winWidth < rule::MIN_WIN || p.winWidth > rule::MAX_WIN || p.winHeight < rule::MIN_WIN || p.winHeight > rule::MAX_WIN) return false;
    if (maxLevel < 0 || maxLevel >= rule::MAX_LEVELS) return false;
    if (isNan(p.eps) || isNan(p.minEigThreshold) || isNan((double)p.errorThreshold)) return false;
    const int useInitial = initial ? 1 : 0;
    if (!asDevice)
        for (int i = 0; i < n; ++i)
            if (!flow::trackable(corners[2 * i], corners[2 * i + 1], useInitial, initial ? initial[2 * i] : 0.0f, initial ? initial[2 * i + 1] : 0.0f)) return false;
    std::vector<std::vector<unsigned char> > fp, tp;
    std::vector<int> w, h;
    if (!StereoOpticalFlowHip::buildPyramid(from, p.winWidth, p.winHeight, maxLevel, fp, w, h) ||
        !StereoOpticalFlowHip::buildPyramid(to, p.winWidth, p.winHeight, maxLevel, tp, w, h)) return false;
    const int levels = (int)fp.size();
    rule::Level I[rule::MAX_LEVELS], J[rule::MAX_LEVELS];
    I[0] = levelOf(from.data, from.pitchBytes, from.width, from.height);          // level 0 is the image itself, read at its own pitch
    J[0] = levelOf(to.data, to.pitchBytes, to.width, to.height);
    for (int l = 1; l < levels; ++l) { I[l] = levelOf(fp[l].data(), w[l], w[l], h[l]); J[l] = levelOf(tp[l].data(), w[l], w[l], h[l]); }
    const rule::Params P = rule::clamp_params(p.winWidth, p.winHeight, maxLevel, p.iterations, p.eps, p.useMinEigenVals ? 1 : 0, p.minEigThreshold,
                                              (double)p.errorThreshold, 0.0f, 0.0f);
    std::vector<short> buf((size_t)p.winWidth * p.winHeight * 4);
    kept.clear();
    for (int i = 0; i < n; ++i) {
        const rule::Track T = flow::track_point_2d(I, J, levels, P, corners[2 * i], corners[2 * i + 1], useInitial, initial ? initial[2 * i] : 0.0f,
                                                   initial ? initial[2 * i + 1] : 0.0f, buf.data());
        if (outTrack) { outTrack[2 * i] = T.rx; outTrack[2 * i + 1] = T.ry; }
        if (outStatus) outStatus[i] = (unsigned char)T.status;
        if (outErr) outErr[i] = T.err;
        if (flow::keep(T, to.width, to.height, P.use_min_eigenvals, p.errorThreshold)) kept.push_back(i);
    }
    return true;
}

}  // namespace rtabmap_amd
