// c_shim.cpp -- flat C entry points over VWDictionaryHip / MemoryHip so that the Python parity tests can drive the C++
// host mirror exactly as they drive the oracle (same call sequence, same argument meaning).  Not part of lcd.h.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>

#include "BayesFilterHip.h"
#include "DbLoaderHip.h"
#include "FeatureSelect.h"
#include "Keypoints3D.h"
#include "MemoryHip.h"
#include "Motion2D.h"
#include "Motion3D.h"
#include "MotionBA.h"
#include "MotionMono.h"
#include "RegistrationIcp.h"
#include "ScanFilter.h"
#include "Stereo.h"
#include "FlowTrack.h"
#include "RtabmapHip.h"

using namespace rtabmap_amd;

static ParametersMap make_params(int strategy, int incremental, float nndr, int together, const char* dictPath) {
    ParametersMap p;
    p["Kp/NNStrategy"] = std::to_string(strategy);
    p["Kp/IncrementalDictionary"] = incremental ? "true" : "false";
    p["Kp/NndrRatio"] = std::to_string(nndr);
    p["Kp/NewWordsComparedTogether"] = together ? "true" : "false";
    if (dictPath && dictPath[0]) p["Kp/DictionaryPath"] = dictPath;
    return p;
}
static Mat make_mat(const void* data, int rows, int cols, int type) { return Mat(rows, cols, type == 0 ? MAT_32F : MAT_8U, data); }

extern "C" {

void* hvwd_create(int strategy, int incremental, float nndr, int together, const char* dictPath, int device) {
    return new VWDictionaryHip(make_params(strategy, incremental, nndr, together, dictPath), device);
}
void hvwd_destroy(void* h) { delete (VWDictionaryHip*)h; }
int hvwd_available(void* h) { return ((VWDictionaryHip*)h)->isAvailable() ? 1 : 0; }
const char* hvwd_last_error(void* h) { return ((VWDictionaryHip*)h)->lastError().c_str(); }
int hvwd_add_new_words(void* h, const void* desc, int rows, int cols, int type, int sigId, int* out, int cap) {
    std::list<int> ids = ((VWDictionaryHip*)h)->addNewWords(make_mat(desc, rows, cols, type), sigId);
    int n = 0;
    for (std::list<int>::iterator i = ids.begin(); i != ids.end() && n < cap; ++i) out[n++] = *i;
    return (int)ids.size();
}
int hvwd_find_nn(void* h, const void* desc, int rows, int cols, int type, int* out) {
    std::vector<int> r = ((VWDictionaryHip*)h)->findNN(make_mat(desc, rows, cols, type));
    for (int i = 0; i < rows; ++i) out[i] = r[i];
    return rows;
}
void hvwd_update(void* h) { ((VWDictionaryHip*)h)->update(); }
// VWDictionaryHip::matchFrames: outFrom[rowsFrom], outTo[rowsTo]; origIds NULL or one per from-row; 1 = done, 0 = failed (hvwd_last_error)
int hvwd_match_frames(void* h, const void* from, int rowsFrom, const void* to, int rowsTo, int cols, int type, int nnType, float nndr,
                      const int* origIds, int* outFrom, int* outTo) {
    std::list<int> f, t;
    const std::vector<int> orig = origIds ? std::vector<int>(origIds, origIds + rowsFrom) : std::vector<int>();
    if (!((VWDictionaryHip*)h)->matchFrames(make_mat(from, rowsFrom, cols, type), make_mat(to, rowsTo, cols, type), nnType, nndr, orig, f, t)) return 0;
    if ((int)f.size() != rowsFrom || (int)t.size() != rowsTo) return 0;
    std::copy(f.begin(), f.end(), outFrom);
    std::copy(t.begin(), t.end(), outTo);
    return 1;
}
void hvwd_add_word(void* h, int id, const void* desc, int cols, int type) {
    ((VWDictionaryHip*)h)->addWord(new VisualWord(id, make_mat(desc, 1, cols, type)));
}
int hvwd_add_word_ref(void* h, int wordId, int sigId) { return ((VWDictionaryHip*)h)->addWordRef(wordId, sigId) ? 1 : 0; }
void hvwd_remove_all_word_ref(void* h, int wordId, int sigId) { ((VWDictionaryHip*)h)->removeAllWordRef(wordId, sigId); }
int hvwd_get_unused_word_ids(void* h, int* out, int cap) {
    std::vector<int> v = ((VWDictionaryHip*)h)->getUnusedWordIds();
    for (size_t i = 0; i < v.size() && (int)i < cap; ++i) out[i] = v[i];
    return (int)v.size();
}
void hvwd_delete_unused_words(void* h) { ((VWDictionaryHip*)h)->deleteUnusedWords(); }
void hvwd_clear(void* h) { ((VWDictionaryHip*)h)->clear(false); }
int hvwd_rebuild_engine(void* h) { return ((VWDictionaryHip*)h)->rebuildEngine() ? 1 : 0; }
// which: 0 visualWords, 1 notIndexed, 2 indexed, 3 totalActiveReferences, 4 lastIndexedWordId, 5 unused
long hvwd_stat(void* h, int which) {
    VWDictionaryHip* d = (VWDictionaryHip*)h;
    switch (which) {
        case 0: return (long)d->getVisualWords().size();
        case 1: return (long)d->getNotIndexedWordsCount();
        case 2: return (long)d->getIndexedWordsCount();
        case 3: return d->getTotalActiveReferences();
        case 4: return d->getLastIndexedWordId();
        case 5: return (long)d->getUnusedWordsSize();
    }
    return -1;
}
int hvwd_get_word_refs(void* h, int wordId, int* sigs, int* counts, int cap) {
    const VisualWord* vw = ((VWDictionaryHip*)h)->getWord(wordId);
    if (!vw) return -1;
    int n = 0;
    for (std::map<int, int>::const_iterator j = vw->getReferences().begin(); j != vw->getReferences().end(); ++j, ++n)
        if (n < cap) { sigs[n] = j->first; counts[n] = j->second; }
    return n;
}
int hvwd_index_ids(void* h, int* out, int cap) {
    std::vector<int> v = ((VWDictionaryHip*)h)->getIndexedWordIds();
    for (size_t i = 0; i < v.size() && (int)i < cap; ++i) out[i] = v[i];
    return (int)v.size();
}
int hvwd_export_text(void* h, const char* refs, const char* desc) { ((VWDictionaryHip*)h)->exportDictionary(refs, desc); return 0; }

// the id bookkeeping of Vis/CorNNType 5 alone (no engine involved): match[rowsTo] as lcd_match_args.out_to_match
void hvwd_cross_check_word_ids(int rowsFrom, const int* origIds, const int* match, int rowsTo, int* outFrom, int* outTo) {
    std::list<int> f, t;
    VWDictionaryHip::crossCheckWordIds(rowsFrom, origIds ? std::vector<int>(origIds, origIds + rowsFrom) : std::vector<int>(), match, rowsTo, f, t);
    std::copy(f.begin(), f.end(), outFrom);
    std::copy(t.begin(), t.end(), outTo);
}

// VWDictionaryHip::matchFramesGuided: corners[2 nCorners], cornerRows[nCorners], pointsTo[2 rowsTo]; outFrom[rowsFrom], outTo[rowsTo],
// outProjected[nCorners] (may be NULL) with *nProjected entries written; 1 = done, 0 = failed (hvwd_last_error)
int hvwd_match_frames_guided(void* h, const void* from, int rowsFrom, const void* to, int rowsTo, int cols, int type, const float* corners,
                             const int* cornerRows, int nCorners, const float* pointsTo, int winSize, int nnType, float nndr, int matchToProjection,
                             const int* origIds, int* outFrom, int* outTo, int* outProjected, int* nProjected) {
    std::list<int> f, t, p;
    const std::vector<int> orig = origIds ? std::vector<int>(origIds, origIds + rowsFrom) : std::vector<int>();
    if (!((VWDictionaryHip*)h)->matchFramesGuided(make_mat(from, rowsFrom, cols, type), make_mat(to, rowsTo, cols, type),
                                                  std::vector<float>(corners, corners + 2 * (size_t)nCorners), std::vector<int>(cornerRows, cornerRows + nCorners),
                                                  std::vector<float>(pointsTo, pointsTo + 2 * (size_t)rowsTo), winSize, nnType, nndr, matchToProjection != 0,
                                                  orig, f, t, &p)) return 0;
    if ((int)f.size() != rowsFrom || (int)t.size() != rowsTo || (int)p.size() > nCorners) return 0;
    std::copy(f.begin(), f.end(), outFrom);
    std::copy(t.begin(), t.end(), outTo);
    if (outProjected) std::copy(p.begin(), p.end(), outProjected);
    if (nProjected) *nProjected = (int)p.size();
    return 1;
}
// the id bookkeeping of the guided match alone (no engine involved): toCorner[rowsTo] = lcd_guided_args.out_to_owner / out_match,
// cornerCount NULL or [nCorners]; returns the number of projected ids written
int hvwd_guided_word_ids(int rowsFrom, const int* origIds, const int* cornerRows, int nCorners, const int* toCorner, int rowsTo, const int* cornerCount,
                         int* outFrom, int* outTo, int* outProjected) {
    std::list<int> f, t, p;
    VWDictionaryHip::guidedWordIds(rowsFrom, origIds ? std::vector<int>(origIds, origIds + rowsFrom) : std::vector<int>(),
                                   std::vector<int>(cornerRows, cornerRows + nCorners), toCorner, rowsTo, cornerCount, f, t, &p);
    std::copy(f.begin(), f.end(), outFrom);
    std::copy(t.begin(), t.end(), outTo);
    if (outProjected) std::copy(p.begin(), p.end(), outProjected);
    return (int)p.size();
}

void* hmem_create(int strategy, int incremental, float nndr, int together, const char* dictPath, int device) {
    return new MemoryHip(make_params(strategy, incremental, nndr, together, dictPath), device);
}
void* hmem_create_stm(int strategy, int incremental, float nndr, int together, const char* dictPath, int device, int stmSize) {
    ParametersMap p = make_params(strategy, incremental, nndr, together, dictPath);
    p["Mem/STMSize"] = std::to_string(stmSize);
    return new MemoryHip(p, device);
}
// a memory that selects its own features: Kp/MaxFeatures, Kp/GridRows, Kp/GridCols (MemoryHip::update with responses and points)
void* hmem_create_select(int strategy, int incremental, float nndr, int together, int device, int stmSize, int maxFeatures, int gridRows, int gridCols) {
    ParametersMap p = make_params(strategy, incremental, nndr, together, "");
    p["Mem/STMSize"] = std::to_string(stmSize);
    p["Kp/MaxFeatures"] = std::to_string(maxFeatures);
    p["Kp/GridRows"] = std::to_string(gridRows);
    p["Kp/GridCols"] = std::to_string(gridCols);
    return new MemoryHip(p, device);
}
// ... and Kp/SSC
void* hmem_create_select_ssc(int strategy, int incremental, float nndr, int together, int device, int stmSize, int maxFeatures, int gridRows, int gridCols, int ssc) {
    ParametersMap p = make_params(strategy, incremental, nndr, together, "");
    p["Mem/STMSize"] = std::to_string(stmSize);
    p["Kp/MaxFeatures"] = std::to_string(maxFeatures);
    p["Kp/GridRows"] = std::to_string(gridRows);
    p["Kp/GridCols"] = std::to_string(gridCols);
    p["Kp/SSC"] = ssc ? "true" : "false";
    return new MemoryHip(p, device);
}
// responses[rows], points[2 rows] (may be NULL with a 1 x 1 grid); returns the signature id, 0 = refused (hmem_select_error)
int hmem_update_select(void* h, const void* desc, int rows, int cols, int type, const float* responses, const float* points, int imageWidth,
                       int imageHeight, int* outIds) {
    std::vector<int> ids;
    const int id = ((MemoryHip*)h)->update(make_mat(desc, rows, cols, type), std::vector<float>(responses, responses + rows),
                                           points ? std::vector<float>(points, points + 2 * (size_t)rows) : std::vector<float>(), imageWidth, imageHeight, ids);
    for (size_t i = 0; i < ids.size(); ++i) outIds[i] = ids[i];
    return id;
}
// cameras as the Python glue passes them: nCameras x 20 floats -- fx, fy, cx, cy, imageWidth, imageHeight, hasLocalTransform, 0, then the 3 x 4 transform
static std::vector<DepthCamera> make_cameras(const float* cameras, int nCameras) {
    std::vector<DepthCamera> cams((size_t)(nCameras > 0 ? nCameras : 0));
    for (size_t c = 0; c < cams.size(); ++c) {
        const float* m = cameras + 20 * c;
        DepthCamera& D = cams[c];
        D.fx = m[0]; D.fy = m[1]; D.cx = m[2]; D.cy = m[3]; D.imageWidth = (int)m[4]; D.imageHeight = (int)m[5]; D.hasLocalTransform = m[6] != 0.0f;
        std::copy(m + 8, m + 20, D.localTransform);
    }
    return cams;
}
static DepthImage make_depth(const void* data, long long pitchBytes, int width, int height, int type) {
    DepthImage image;
    image.data = data; image.pitchBytes = pitchBytes; image.width = width; image.height = height; image.type = type;
    return image;
}
// the same for an RGB-D frame (MemoryHip::update with a depth image and cameras).  depthType: 0 u16 millimetres, 1 f32 metres.  outIds[rows],
// outXyz[3 rows] and outKept[rows] receive one entry per feature the depth filter kept; *outKeptCount their number
int hmem_update_depth(void* h, const void* desc, int rows, int cols, int type, const float* responses, const float* points, int imageWidth,
                      int imageHeight, const void* depth, long long pitchBytes, int depthWidth, int depthHeight, int depthType,
                      const float* cameras, int nCameras, int* outIds, float* outXyz, int* outKept, int* outKeptCount) {
    const std::vector<DepthCamera> cams = make_cameras(cameras, nCameras);
    const DepthImage image = make_depth(depth, pitchBytes, depthWidth, depthHeight, depthType);
    std::vector<int> ids, kept;
    std::vector<float> xyz;
    const int id = ((MemoryHip*)h)->update(make_mat(desc, rows, cols, type), std::vector<float>(responses, responses + rows),
                                           std::vector<float>(points, points + 2 * (size_t)rows), imageWidth, imageHeight, image, cams, ids, xyz, kept);
    *outKeptCount = id ? (int)kept.size() : 0;
    if (!id) return 0;
    std::copy(ids.begin(), ids.end(), outIds);
    std::copy(xyz.begin(), xyz.end(), outXyz);
    std::copy(kept.begin(), kept.end(), outKept);
    return id;
}
void* hmem_create_depth(int strategy, int incremental, float nndr, int together, int device, int stmSize, int maxFeatures, int gridRows, int gridCols,
                        float minDepth, float maxDepth) {
    ParametersMap p = make_params(strategy, incremental, nndr, together, "");
    p["Mem/STMSize"] = std::to_string(stmSize);
    p["Kp/MaxFeatures"] = std::to_string(maxFeatures);
    p["Kp/GridRows"] = std::to_string(gridRows);
    p["Kp/GridCols"] = std::to_string(gridCols);
    char text[2][32];                                                  // nine digits: the float comes back as it was given
    snprintf(text[0], sizeof text[0], "%.9g", (double)minDepth);
    snprintf(text[1], sizeof text[1], "%.9g", (double)maxDepth);
    p["Kp/MinDepth"] = text[0];
    p["Kp/MaxDepth"] = text[1];
    return new MemoryHip(p, device);
}
// Keypoints3D's three functions (no engine involved).  1 = done (the filters: the number kept), 0 / -1 = refused
int hk3_generate(const float* points, int n, const void* depth, long long pitchBytes, int width, int height, int type, const float* cameras,
                 int nCameras, float minDepth, float maxDepth, float* outXyz) {
    const std::vector<DepthCamera> cams = make_cameras(cameras, nCameras);
    const DepthImage image = make_depth(depth, pitchBytes, width, height, type);
    return Keypoints3D::generateKeypoints3DDepth(points, n, image, cams.data(), nCameras, minDepth, maxDepth, outXyz) ? 1 : 0;
}
int hk3_filter_3d(const float* xyz, int n, float minDepth, float maxDepth, int* outKept) {
    std::vector<int> kept;
    if (!Keypoints3D::filterKeypointsByDepth(xyz, n, minDepth, maxDepth, kept)) return -1;
    std::copy(kept.begin(), kept.end(), outKept);
    return (int)kept.size();
}
int hk3_filter_pixel(const float* points, int n, const void* depth, long long pitchBytes, int width, int height, int type, float minDepth,
                     float maxDepth, int* outKept) {
    const DepthImage image = make_depth(depth, pitchBytes, width, height, type);
    std::vector<int> kept;
    if (!Keypoints3D::filterKeypointsByDepth(points, n, image, minDepth, maxDepth, kept)) return -1;
    std::copy(kept.begin(), kept.end(), outKept);
    return (int)kept.size();
}
// ---- the stereo stage.  params as the Python glue passes them: 10 doubles -- winWidth, winHeight, maxLevel, iterations, eps, useMinEigenVals,
// minEigThreshold, errorThreshold, minDisparity, maxDisparity (the last two are floats widened); camera: 7 doubles -- fx, fy, cx, cy, rightCx,
// baseline, hasLocalTransform --, then the 3 x 4 transform as 12 floats
static StereoParams make_stereo_params(const double* p) {
    StereoParams s;
    s.winWidth = (int)p[0]; s.winHeight = (int)p[1]; s.maxLevel = (int)p[2]; s.iterations = (int)p[3]; s.eps = p[4]; s.useMinEigenVals = p[5] != 0.0;
    s.minEigThreshold = p[6]; s.errorThreshold = p[7]; s.minDisparity = (float)p[8]; s.maxDisparity = (float)p[9];
    return s;
}
static StereoCamera make_stereo_camera(const double* c, const float* transform) {
    StereoCamera s;
    s.fx = c[0]; s.fy = c[1]; s.cx = c[2]; s.cy = c[3]; s.rightCx = c[4]; s.baseline = c[5]; s.hasLocalTransform = c[6] != 0.0;
    std::copy(transform, transform + 12, s.localTransform);
    return s;
}
static GrayImage make_gray(const void* data, long long pitchBytes, int width, int height) {
    GrayImage g;
    g.data = (const unsigned char*)data; g.pitchBytes = pitchBytes; g.width = width; g.height = height;
    return g;
}
// StereoOpticalFlowHip (no engine involved).  1 = done, 0 = refused
int hst_correspondences(const double* params, const void* left, long long leftPitch, const void* right, long long rightPitch, int width, int height,
                        const float* points, int n, float* outRight, unsigned char* outStatus) {
    const StereoOpticalFlowHip flow(make_stereo_params(params));
    return flow.computeCorrespondences(make_gray(left, leftPitch, width, height), make_gray(right, rightPitch, width, height), points, n, outRight, outStatus) ? 1 : 0;
}
int hst_generate(const float* points, const float* right, int n, const double* camera, const float* transform, const unsigned char* status,
                 float minDepth, float maxDepth, float* outXyz) {
    return StereoOpticalFlowHip::generateKeypoints3DStereo(points, right, n, make_stereo_camera(camera, transform), status, minDepth, maxDepth, outXyz) ? 1 : 0;
}
// the pyramid of one image: outLevels receives the levels' packed rows back to back (at most 2 * width * height bytes), outSizes w, h per
// level; returns the number of levels, 0 = refused
int hst_pyramid(const void* image, long long pitchBytes, int width, int height, int winWidth, int winHeight, int maxLevel, unsigned char* outLevels, int* outSizes) {
    std::vector<std::vector<unsigned char> > levels;
    std::vector<int> w, h;
    if (!StereoOpticalFlowHip::buildPyramid(make_gray(image, pitchBytes, width, height), winWidth, winHeight, maxLevel, levels, w, h)) return 0;
    for (size_t l = 0; l < levels.size(); ++l) {
        outLevels = std::copy(levels[l].begin(), levels[l].end(), outLevels);
        outSizes[2 * l] = w[l]; outSizes[2 * l + 1] = h[l];
    }
    return (int)levels.size();
}
void hst_derivative(const void* image, long long pitchBytes, int width, int height, short* outDxDy) {
    StereoOpticalFlowHip::derivative(make_gray(image, pitchBytes, width, height), outDxDy);
}
// ---- the optical-flow correspondences (FlowTrack.h; no engine involved).  params: 7 doubles -- winWidth, winHeight, iterations, eps,
// useMinEigenVals, minEigThreshold, errorThreshold (a float widened).  initial may be NULL.  outKept [n].  Returns the number kept, -1 = refused
int hflow_track(const double* params, const void* from, long long fromPitch, const void* to, long long toPitch, int width, int height, int maxLevel,
                const float* points, const float* initial, int n, int asDevice, float* outTrack, unsigned char* outStatus, float* outErr, int* outKept) {
    FlowParams p;
    p.winWidth = (int)params[0]; p.winHeight = (int)params[1]; p.iterations = (int)params[2]; p.eps = params[3]; p.useMinEigenVals = params[4] != 0.0;
    p.minEigThreshold = params[5]; p.errorThreshold = (float)params[6];
    std::vector<int> kept;
    if (!flow_track_cpu(make_gray(from, fromPitch, width, height), make_gray(to, toPitch, width, height), maxLevel, points, initial, n, p, asDevice != 0,
                        outTrack, outStatus, outErr, kept)) return -1;
    std::copy(kept.begin(), kept.end(), outKept);
    return (int)kept.size();
}
void hmem_set_stereo_params(void* h, const double* params) { ((MemoryHip*)h)->setStereoParams(make_stereo_params(params)); }
// a stereo frame through MemoryHip::update; the outputs as hmem_update_depth's
int hmem_update_stereo(void* h, const void* desc, int rows, int cols, int type, const float* responses, const float* points, int imageWidth,
                       int imageHeight, const void* left, long long leftPitch, const void* right, long long rightPitch, int width, int height,
                       const double* camera, const float* transform, int* outIds, float* outXyz, int* outKept, int* outKeptCount) {
    std::vector<int> ids, kept;
    std::vector<float> xyz;
    const int id = ((MemoryHip*)h)->update(make_mat(desc, rows, cols, type), std::vector<float>(responses, responses + rows),
                                           std::vector<float>(points, points + 2 * (size_t)rows), imageWidth, imageHeight, make_gray(left, leftPitch, width, height),
                                           make_gray(right, rightPitch, width, height), make_stereo_camera(camera, transform), ids, xyz, kept);
    *outKeptCount = id ? (int)kept.size() : 0;
    if (!id) return 0;
    std::copy(ids.begin(), ids.end(), outIds);
    std::copy(xyz.begin(), xyz.end(), outXyz);
    std::copy(kept.begin(), kept.end(), outKept);
    return id;
}
// motion3d_cpu (no engine involved).  outTransform[12], outScalars[3] = status, matches, inliers; outMatches / outInliers hold nFrom ids.  1 = done, 0 = refused
int hm3_cpu(const int* fromIds, const float* fromXyz, int nFrom, const int* toIds, const float* toXyz, int nTo, int minInliers, double inlierDistance,
            int iterations, int refineIterations, unsigned seed, int sweeps, float* outTransform, int* outScalars, double* outVariance, int* outMatches,
            int* outInliers) {
    Motion3DResult r;
    if (!motion3d_cpu(fromIds, fromXyz, nFrom, toIds, toXyz, nTo, minInliers, inlierDistance, iterations, refineIterations, seed, r, sweeps)) return 0;
    std::copy(r.transform, r.transform + 12, outTransform);
    outScalars[0] = r.status; outScalars[1] = (int)r.matches.size(); outScalars[2] = (int)r.inliers.size();
    *outVariance = r.variance;
    std::copy(r.matches.begin(), r.matches.end(), outMatches);
    std::copy(r.inliers.begin(), r.inliers.end(), outInliers);
    return 1;
}
// Motion3D::estimateMotion3DTo3D through the dictionary's engine, the frames as parallel arrays.  outCovariance[36]; returns 1 with a transform, 0 without
int hm3_estimate(void* h, const int* idsA, const float* xyzA, int nA, const int* idsB, const float* xyzB, int nB, int minInliers, double inliersDistance,
                 int iterations, int refineIterations, unsigned seed, float* outTransform, double* outCovariance, int* outCounts, int* outMatches,
                 int* outInliers) {
    std::multimap<int, Point3f> a, b;
    for (int i = 0; i < nA; ++i) a.insert(std::make_pair(idsA[i], Point3f{xyzA[3 * i], xyzA[3 * i + 1], xyzA[3 * i + 2]}));
    for (int i = 0; i < nB; ++i) b.insert(std::make_pair(idsB[i], Point3f{xyzB[3 * i], xyzB[3 * i + 1], xyzB[3 * i + 2]}));
    std::vector<int> matches, inliers;
    const Transform3D t = Motion3D::estimateMotion3DTo3D(((VWDictionaryHip*)h)->engine(), a, b, minInliers, inliersDistance, iterations, refineIterations,
                                                         outCovariance, &matches, &inliers, seed);
    std::copy(t.data, t.data + 12, outTransform);
    outCounts[0] = (int)matches.size(); outCounts[1] = (int)inliers.size();
    std::copy(matches.begin(), matches.end(), outMatches);
    std::copy(inliers.begin(), inliers.end(), outInliers);
    return t.isNull() ? 0 : 1;
}
// register_icp_cpu (no engine involved).  guess[12]; outTransforms[36] = transform, icp transform, correction; outScalars[4] = status, stop, iterations,
// correspondences; outMatch holds nFrom rows.  1 = done, 0 = refused
int hicp_cpu(const float* fromXyz, int nFrom, const float* toXyz, int nTo, const float* guess, int maxIterations, int force3DoF, int maxLaserScans,
             double maxCorrespondenceDistance, float epsilon, float correspondenceRatio, int search, int deviceEntry, float* outTransforms, int* outScalars,
             float* outRatio, double* outVariance, int* outMatch) {
    IcpResult r;
    if (!register_icp_cpu(fromXyz, nFrom, toXyz, nTo, guess, maxIterations, force3DoF != 0, maxLaserScans, maxCorrespondenceDistance, epsilon,
                          correspondenceRatio, search, deviceEntry != 0, r)) return 0;
    std::copy(r.transform, r.transform + 12, outTransforms);
    std::copy(r.icpTransform, r.icpTransform + 12, outTransforms + 12);
    std::copy(r.correction, r.correction + 12, outTransforms + 24);
    outScalars[0] = r.status; outScalars[1] = r.stop; outScalars[2] = r.iterations; outScalars[3] = r.correspondences;
    *outRatio = r.ratio; *outVariance = r.variance;
    std::copy(r.match.begin(), r.match.end(), outMatch);
    return 1;
}
// the grid form's cell of every coordinate (csrc/icp_rule.h: cell_size, cell_of); INT_MIN where it does not fit the key's range.  Returns the cell size
float hicp_cells(const float* x, int n, double maxCorrespondenceDistance, int* outCells) {
    return icp_cells(x, n, maxCorrespondenceDistance, outCells);
}
static int icp_info_out(const Transform3D& t, const RegistrationInfoIcp& info, float* outTransform, float* outInfo, int* outCorrespondences, double* outCovariance) {
    std::copy(t.data, t.data + 12, outTransform);
    outInfo[0] = info.icpTranslation; outInfo[1] = info.icpRotation; outInfo[2] = info.icpInliersRatio;
    *outCorrespondences = info.icpCorrespondences;
    std::copy(info.covariance, info.covariance + 36, outCovariance);
    return t.isNull() ? 0 : 1;
}
// RegistrationIcpHip::finish over a rule's result (no engine involved): transforms[36] and scalars[4] as hicp_cpu writes them.  outInfo[3] =
// icpTranslation, icpRotation, icpInliersRatio; outCovariance[36]; returns 1 with a transform, 0 without
int hicp_finish(const float* transforms, const int* scalars, float ratio, double variance, float maxTranslation, float maxRotation, float correspondenceRatio,
                float* outTransform, float* outInfo, int* outCorrespondences, double* outCovariance) {
    IcpResult r;
    std::copy(transforms, transforms + 12, r.transform);
    std::copy(transforms + 12, transforms + 24, r.icpTransform);
    std::copy(transforms + 24, transforms + 36, r.correction);
    r.status = scalars[0]; r.stop = scalars[1]; r.iterations = scalars[2]; r.correspondences = scalars[3]; r.ratio = ratio; r.variance = variance;
    RegistrationIcpHip reg;
    reg.maxTranslation = maxTranslation; reg.maxRotation = maxRotation; reg.correspondenceRatio = correspondenceRatio;
    RegistrationInfoIcp info;
    return icp_info_out(reg.finish(r, info), info, outTransform, outInfo, outCorrespondences, outCovariance);
}
// RegistrationIcpHip::computeTransformation through the dictionary's engine, the scans as [n x 3] rows; outputs as hicp_finish
int hicp_compute(void* h, const float* fromXyz, int nFrom, const float* toXyz, int nTo, const float* guess, int maxIterations, int force3DoF,
                 int maxLaserScans, double maxCorrespondenceDistance, float epsilon, float correspondenceRatio, float maxTranslation, float maxRotation,
                 float* outTransform, float* outInfo, int* outCorrespondences, double* outCovariance) {
    std::vector<Point3f> from((size_t)nFrom), to((size_t)nTo);
    for (int i = 0; i < nFrom; ++i) from[(size_t)i] = Point3f{fromXyz[3 * i], fromXyz[3 * i + 1], fromXyz[3 * i + 2]};
    for (int i = 0; i < nTo; ++i) to[(size_t)i] = Point3f{toXyz[3 * i], toXyz[3 * i + 1], toXyz[3 * i + 2]};
    Transform3D g;
    std::copy(guess, guess + 12, g.data);
    RegistrationIcpHip reg;
    reg.maxIterations = maxIterations; reg.force3DoF = force3DoF != 0; reg.maxCorrespondenceDistance = maxCorrespondenceDistance; reg.epsilon = epsilon;
    reg.correspondenceRatio = correspondenceRatio; reg.maxTranslation = maxTranslation; reg.maxRotation = maxRotation;
    RegistrationInfoIcp info;
    return icp_info_out(reg.computeTransformation(((VWDictionaryHip*)h)->engine(), from, to, g, maxLaserScans, info), info, outTransform, outInfo,
                        outCorrespondences, outCovariance);
}
// register_icp_plane_cpu (no engine involved).  outTransforms[36] and outScalars as hicp_cpu, outScalars[4] = branch; outComplexity[14] = complexity,
// values[3], vectors[9], second eigenvalue.  1 = done, 0 = refused
int hicpp_cpu(const float* fromXyz, const float* fromNormals, int nFrom, const float* toXyz, const float* toNormals, int nTo, const float* guess,
              int maxIterations, int force3DoF, int maxLaserScans, double maxCorrespondenceDistance, float epsilon, float correspondenceRatio,
              float minComplexity, int lowComplexityStrategy, int normalGate, double minNormalCos, int search, int deviceEntry, float* outTransforms,
              int* outScalars, float* outRatio, double* outVariance, int* outMatch, float* outComplexity) {
    IcpPlaneResult r;
    if (!register_icp_plane_cpu(fromXyz, fromNormals, nFrom, toXyz, toNormals, nTo, guess, maxIterations, force3DoF != 0, maxLaserScans,
                                maxCorrespondenceDistance, epsilon, correspondenceRatio, minComplexity, lowComplexityStrategy, normalGate != 0, minNormalCos,
                                search, deviceEntry != 0, r)) return 0;
    std::copy(r.transform, r.transform + 12, outTransforms);
    std::copy(r.icpTransform, r.icpTransform + 12, outTransforms + 12);
    std::copy(r.correction, r.correction + 12, outTransforms + 24);
    outScalars[0] = r.status; outScalars[1] = r.stop; outScalars[2] = r.iterations; outScalars[3] = r.correspondences; outScalars[4] = r.branch;
    *outRatio = r.ratio; *outVariance = r.variance;
    std::copy(r.match.begin(), r.match.end(), outMatch);
    outComplexity[0] = r.complexity;
    std::copy(r.complexityValues, r.complexityValues + 3, outComplexity + 1);
    std::copy(r.complexityVectors, r.complexityVectors + 9, outComplexity + 4);
    outComplexity[13] = r.secondEigenvalue;
    return 1;
}
// RegistrationIcpHip::computeTransformation with normals through the dictionary's engine; outputs as hicp_finish, outInfo[3] = icpStructuralComplexity
int hicpp_compute(void* h, const float* fromXyz, const float* fromNormals, int nFrom, int fromIs2d, const float* toXyz, const float* toNormals, int nTo,
                  int toIs2d, const float* guess, int maxIterations, int force3DoF, int maxLaserScans, double maxCorrespondenceDistance, float epsilon,
                  float correspondenceRatio, float maxTranslation, float maxRotation, int pointToPlane, float minComplexity, int lowComplexityStrategy,
                  float* outTransform, float* outInfo, int* outCorrespondences, double* outCovariance) {
    auto rows = [](const float* x, int n) {
        std::vector<Point3f> v((size_t)(x ? n : 0));
        for (size_t i = 0; i < v.size(); ++i) v[i] = Point3f{x[3 * i], x[3 * i + 1], x[3 * i + 2]};
        return v;
    };
    Transform3D g;
    std::copy(guess, guess + 12, g.data);
    RegistrationIcpHip reg;
    reg.maxIterations = maxIterations; reg.force3DoF = force3DoF != 0; reg.maxCorrespondenceDistance = maxCorrespondenceDistance; reg.epsilon = epsilon;
    reg.correspondenceRatio = correspondenceRatio; reg.maxTranslation = maxTranslation; reg.maxRotation = maxRotation;
    reg.pointToPlane = pointToPlane != 0; reg.pointToPlaneMinComplexity = minComplexity; reg.pointToPlaneLowComplexityStrategy = lowComplexityStrategy;
    RegistrationInfoIcp info;
    const Transform3D t = reg.computeTransformation(((VWDictionaryHip*)h)->engine(), rows(fromXyz, nFrom), rows(fromNormals, nFrom), fromIs2d != 0,
                                                    rows(toXyz, nTo), rows(toNormals, nTo), toIs2d != 0, g, maxLaserScans, info);
    outInfo[3] = info.icpStructuralComplexity;
    return icp_info_out(t, info, outTransform, outInfo, outCorrespondences, outCovariance);
}
// filter_scans_cpu (no engine involved): one scan into a region of `capacity` rows.  viewpoint[3]; outXyz / outNormals [capacity x 3] (outNormals
// is written only when normals are asked for); outInts[5] = status, count, the three stage counts.  Returns LCD_OK or the refusal's code
int hsf_cpu(const float* xyz, long long n, int downsamplingStep, int is2d, float rangeMin, float rangeMax, float voxelSize, int normalK, float normalRadius,
            float groundNormalsUp, const float* viewpoint, long long capacity, int deviceEntry, float* outXyz, float* outNormals, int* outInts) {
    ScanFilterParams p;
    p.downsamplingStep = downsamplingStep; p.is2d = is2d != 0; p.rangeMin = rangeMin; p.rangeMax = rangeMax; p.voxelSize = voxelSize;
    p.normalK = normalK; p.normalRadius = normalRadius; p.groundNormalsUp = groundNormalsUp;
    std::copy(viewpoint, viewpoint + 3, p.viewpoint);
    ScanFilterResult r;
    const int rc = filter_scans_cpu(xyz, n, p, capacity, deviceEntry != 0, r);
    if (rc != 0) return rc;
    std::copy(r.xyz.begin(), r.xyz.end(), outXyz);
    std::copy(r.normals.begin(), r.normals.end(), outNormals);
    outInts[0] = r.status; outInts[1] = r.count;
    std::copy(r.stageCounts, r.stageCounts + 3, outInts + 2);
    return 0;
}
// RegistrationIcpHip::computeTransformation over raw scans through the dictionary's engine: the filters of `filtersEnabled` in front (lcd_filter_scans),
// then hicpp_compute's work.  filter[8] = downsamplingStep, rangeMin, rangeMax, voxelSize, pointToPlaneK, pointToPlaneRadius,
// pointToPlaneGroundNormalsUp, filtersEnabled; outputs as hicpp_compute, outSizes[3] = the from-scan's and the to-scan's rows behind the filters, maxLaserScans
int hicpf_compute(void* h, const float* fromXyz, int nFrom, int fromIs2d, int fromMaxPoints, const float* toXyz, int nTo, int toIs2d, int toMaxPoints,
                  const float* guess, const float* filter, int maxIterations, int force3DoF, double maxCorrespondenceDistance, float epsilon,
                  float correspondenceRatio, float maxTranslation, float maxRotation, int pointToPlane, float minComplexity, int lowComplexityStrategy,
                  float* outTransform, float* outInfo, int* outCorrespondences, double* outCovariance, int* outSizes) {
    auto rows = [](const float* x, int n) {
        std::vector<Point3f> v((size_t)(x ? n : 0));
        for (size_t i = 0; i < v.size(); ++i) v[i] = Point3f{x[3 * i], x[3 * i + 1], x[3 * i + 2]};
        return v;
    };
    Transform3D g;
    std::copy(guess, guess + 12, g.data);
    RegistrationIcpHip reg;
    reg.maxIterations = maxIterations; reg.force3DoF = force3DoF != 0; reg.maxCorrespondenceDistance = maxCorrespondenceDistance; reg.epsilon = epsilon;
    reg.correspondenceRatio = correspondenceRatio; reg.maxTranslation = maxTranslation; reg.maxRotation = maxRotation;
    reg.pointToPlane = pointToPlane != 0; reg.pointToPlaneMinComplexity = minComplexity; reg.pointToPlaneLowComplexityStrategy = lowComplexityStrategy;
    reg.downsamplingStep = (int)filter[0]; reg.rangeMin = filter[1]; reg.rangeMax = filter[2]; reg.voxelSize = filter[3]; reg.pointToPlaneK = (int)filter[4];
    reg.pointToPlaneRadius = filter[5]; reg.pointToPlaneGroundNormalsUp = filter[6]; reg.filtersEnabled = (int)filter[7];
    RegistrationInfoIcp info;
    FilteredScans fs;
    const Transform3D t = reg.computeTransformation(((VWDictionaryHip*)h)->engine(), rows(fromXyz, nFrom), fromIs2d != 0, fromMaxPoints, rows(toXyz, nTo),
                                                    toIs2d != 0, toMaxPoints, g, info, &fs);
    outSizes[0] = (int)fs.fromScan.size(); outSizes[1] = (int)fs.toScan.size(); outSizes[2] = fs.maxLaserScans;
    outInfo[3] = info.icpStructuralComplexity;
    return icp_info_out(t, info, outTransform, outInfo, outCorrespondences, outCovariance);
}
// motion_pnp_cpu (no engine involved).  camera[4] = fx, fy, cx, cy; image[2]; local: 12 floats or null; guess: 12 floats or null; toXyz may be null.
// outTransform[12], outScalars[4] = status, matches, inliers, variance kind; outVariance[2] = linear, cosine; outMatches / outInliers hold nTo ids.
// 1 = done, 0 = refused
int hmp_cpu(const int* fromIds, const float* fromXyz, int nFrom, const int* toIds, const float* toPoints, const float* toXyz, int nTo, const float* camera,
            const int* image, const float* local, const float* guess, int minInliers, int iterations, double reprojError, int refineIterations,
            int varianceMedianRatio, float maxVariance, unsigned seed, int steps, float* outTransform, int* outScalars, double* outVariance, int* outMatches,
            int* outInliers) {
    lcd_camera cam = {};
    cam.fx = camera[0]; cam.fy = camera[1]; cam.cx = camera[2]; cam.cy = camera[3]; cam.image_width = image[0]; cam.image_height = image[1];
    cam.has_local_transform = local ? 1 : 0;
    if (local) std::copy(local, local + 12, cam.local_transform);
    MotionPnpParams p;
    p.minInliers = minInliers; p.iterations = iterations; p.reprojError = reprojError; p.refineIterations = refineIterations;
    p.varianceMedianRatio = varianceMedianRatio; p.maxVariance = maxVariance; p.seed = seed; p.steps = steps;
    MotionPnpResult r;
    if (!motion_pnp_cpu(fromIds, fromXyz, nFrom, toIds, toPoints, toXyz, nTo, cam, guess, p, r)) return 0;
    std::copy(r.transform, r.transform + 12, outTransform);
    outScalars[0] = r.status; outScalars[1] = (int)r.matches.size(); outScalars[2] = (int)r.inliers.size(); outScalars[3] = r.varianceKind;
    outVariance[0] = r.varianceLin; outVariance[1] = r.angleCos;
    std::copy(r.matches.begin(), r.matches.end(), outMatches);
    std::copy(r.inliers.begin(), r.inliers.end(), outInliers);
    return 1;
}
// Motion2D::estimateMotion3DTo2D through the dictionary's engine, the frames as parallel arrays.  outCovariance[36]; returns 1 with a transform, 0 without
int hmp_estimate(void* h, const int* idsA, const float* xyzA, int nA, const int* idsB, const float* pointsB, const float* xyzB, int nB, const float* camera,
                 const int* image, const float* local, const float* guess, int minInliers, int iterations, double reprojError, int refineIterations,
                 int varianceMedianRatio, float maxVariance, unsigned seed, float* outTransform, double* outCovariance, int* outCounts, int* outMatches,
                 int* outInliers) {
    lcd_camera cam = {};
    cam.fx = camera[0]; cam.fy = camera[1]; cam.cx = camera[2]; cam.cy = camera[3]; cam.image_width = image[0]; cam.image_height = image[1];
    cam.has_local_transform = local ? 1 : 0;
    if (local) std::copy(local, local + 12, cam.local_transform);
    std::multimap<int, Point3f> a, b3;
    std::multimap<int, Point2f> b;
    for (int i = 0; i < nA; ++i) a.insert(std::make_pair(idsA[i], Point3f{xyzA[3 * i], xyzA[3 * i + 1], xyzA[3 * i + 2]}));
    for (int i = 0; i < nB; ++i) b.insert(std::make_pair(idsB[i], Point2f{pointsB[2 * i], pointsB[2 * i + 1]}));
    if (xyzB)
        for (int i = 0; i < nB; ++i) b3.insert(std::make_pair(idsB[i], Point3f{xyzB[3 * i], xyzB[3 * i + 1], xyzB[3 * i + 2]}));
    Transform3D g;
    if (guess) std::copy(guess, guess + 12, g.data);
    std::vector<int> matches, inliers;
    const Transform3D t = Motion2D::estimateMotion3DTo2D(((VWDictionaryHip*)h)->engine(), a, b, cam, minInliers, iterations, reprojError, refineIterations,
                                                         varianceMedianRatio, maxVariance, g, b3, outCovariance, &matches, &inliers, seed);
    std::copy(t.data, t.data + 12, outTransform);
    outCounts[0] = (int)matches.size(); outCounts[1] = (int)inliers.size();
    std::copy(matches.begin(), matches.end(), outMatches);
    std::copy(inliers.begin(), inliers.end(), outInliers);
    return t.isNull() ? 0 : 1;
}
static lcd_camera shim_camera(const float* camera, const int* image, const float* local) {
    lcd_camera cam = {};
    cam.fx = camera[0]; cam.fy = camera[1]; cam.cx = camera[2]; cam.cy = camera[3]; cam.image_width = image[0]; cam.image_height = image[1];
    cam.has_local_transform = local ? 1 : 0;
    if (local) std::copy(local, local + 12, cam.local_transform);
    return cam;
}
static MotionBAParams shim_ba_params(const double* params, int iterations, int minInliers) {
    MotionBAParams p;
    p.pixelVariance = params[0]; p.robustDelta = params[1]; p.baselineFrom = params[2]; p.baselineTo = params[3];
    p.maxInliersMeanDistance = (float)params[4]; p.minInliersDistribution = (float)params[5];
    p.iterations = iterations; p.minInliers = minInliers;
    return p;
}
// motion_ba_cpu (no engine involved).  cameras as hmp_cpu's, one per side; fromPoints, toXyz, priorVariance[2], the locals may be null;
// params[6] = pixelVariance, robustDelta, baselineFrom, baselineTo, maxInliersMeanDistance, minInliersDistribution.  outTransform[12],
// outInts[4] = status, inliers, outliers, accepted steps; outChi2[2]; outGates[2] = mean distance, distribution; outInliers holds nTo ids.
// 1 = done, 0 = refused
int hmba_cpu(const int* fromIds, const float* fromXyz, const float* fromPoints, int nFrom, const int* toIds, const float* toPoints, const float* toXyz, int nTo,
             const int* inliers, int nInliers, const float* transform, const double* priorVariance, const float* cameraFrom, const int* imageFrom,
             const float* localFrom, const float* cameraTo, const int* imageTo, const float* localTo, const double* params, int iterations, int minInliers,
             float* outTransform, int* outInts, double* outChi2, float* outGates, int* outInliers) {
    MotionBAResult r;
    if (!motion_ba_cpu(fromIds, fromXyz, fromPoints, nFrom, toIds, toPoints, toXyz, nTo, inliers, nInliers, transform, priorVariance,
                       shim_camera(cameraFrom, imageFrom, localFrom), shim_camera(cameraTo, imageTo, localTo), shim_ba_params(params, iterations, minInliers), r))
        return 0;
    std::copy(r.transform, r.transform + 12, outTransform);
    outInts[0] = r.status; outInts[1] = (int)r.inliers.size(); outInts[2] = r.nOutliers; outInts[3] = r.lmAccepted;
    outChi2[0] = r.chi2Before; outChi2[1] = r.chi2After;
    outGates[0] = r.inliersMeanDistance; outGates[1] = r.inliersDistribution;
    std::copy(r.inliers.begin(), r.inliers.end(), outInliers);
    return 1;
}
// MotionBA::refine through the dictionary's engine, the frames as parallel arrays (pointsA and xyzB may be null); variance[2] = linear, the
// cosine, as the PnP left them.  inliers: nInliers ids in, the survivors out; outInts[2] = status, survivors.  Returns 1 with a transform
int hmba_refine(void* h, const int* idsA, const float* xyzA, const float* pointsA, int nA, const int* idsB, const float* pointsB, const float* xyzB, int nB,
                int* inliers, int nInliers, const float* transform, int varianceKind, const double* variance, const float* cameraFrom, const int* imageFrom,
                const float* localFrom, const float* cameraTo, const int* imageTo, const float* localTo, const double* params, int iterations, int minInliers,
                float* outTransform, int* outInts, float* outGates) {
    std::multimap<int, Point3f> a3, b3;
    std::multimap<int, Point2f> a2, b2;
    for (int i = 0; i < nA; ++i) {
        a3.insert(std::make_pair(idsA[i], Point3f{xyzA[3 * i], xyzA[3 * i + 1], xyzA[3 * i + 2]}));
        if (pointsA) a2.insert(std::make_pair(idsA[i], Point2f{pointsA[2 * i], pointsA[2 * i + 1]}));
    }
    for (int i = 0; i < nB; ++i) {
        b2.insert(std::make_pair(idsB[i], Point2f{pointsB[2 * i], pointsB[2 * i + 1]}));
        if (xyzB) b3.insert(std::make_pair(idsB[i], Point3f{xyzB[3 * i], xyzB[3 * i + 1], xyzB[3 * i + 2]}));
    }
    Transform3D t0;
    std::copy(transform, transform + 12, t0.data);
    std::vector<int> in(inliers, inliers + nInliers);
    MotionBAInfo info;
    const Transform3D t = MotionBA::refine(((VWDictionaryHip*)h)->engine(), a3, a2, b2, b3, shim_camera(cameraFrom, imageFrom, localFrom),
                                           shim_camera(cameraTo, imageTo, localTo), t0, in, varianceKind, variance[0], variance[1],
                                           shim_ba_params(params, iterations, minInliers), &info);
    std::copy(t.data, t.data + 12, outTransform);
    std::copy(in.begin(), in.end(), inliers);
    outInts[0] = info.status; outInts[1] = (int)in.size();
    outGates[0] = info.inliersMeanDistance; outGates[1] = info.inliersDistribution;
    return t.isNull() ? 0 : 1;
}
const char* hmem_select_error(void* h) { return ((MemoryHip*)h)->lastSelectError().c_str(); }
// FeatureSelect's three functions (no engine involved).  1 = done, 0 = refused
int hfs_limit_keypoints(const float* response, const float* points, int n, int maxKeypoints, int imageWidth, int imageHeight, int gridRows, int gridCols,
                        unsigned char* outInliers) {
    std::vector<bool> inliers;
    if (!FeatureSelect::limitKeypoints(response, points, n, maxKeypoints, imageWidth, imageHeight, gridRows, gridCols, inliers)) return 0;
    for (size_t i = 0; i < inliers.size(); ++i) outInliers[i] = inliers[i] ? 1 : 0;
    return 1;
}
// returns the number of indices written to outKept[n], -1 = refused
int hfs_limit_keypoints_compact(const float* response, int n, int maxKeypoints, int* outKept) {
    std::vector<int> kept;
    if (!FeatureSelect::limitKeypoints(response, n, maxKeypoints, kept)) return -1;
    std::copy(kept.begin(), kept.end(), outKept);
    return (int)kept.size();
}
// the Kp/SSC forms: points[2 n] and the image size are needed when the frame is cut
int hfs_limit_keypoints_ssc(const float* response, const float* points, int n, int maxKeypoints, int imageWidth, int imageHeight, unsigned char* outInliers) {
    std::vector<bool> inliers;
    if (!FeatureSelect::limitKeypointsSSC(response, points, n, maxKeypoints, imageWidth, imageHeight, inliers)) return 0;
    for (size_t i = 0; i < inliers.size(); ++i) outInliers[i] = inliers[i] ? 1 : 0;
    return 1;
}
int hfs_limit_keypoints_ssc_compact(const float* response, const float* points, int n, int maxKeypoints, int imageWidth, int imageHeight, int* outKept) {
    std::vector<int> kept;
    if (!FeatureSelect::limitKeypointsSSC(response, points, n, maxKeypoints, imageWidth, imageHeight, kept)) return -1;
    std::copy(kept.begin(), kept.end(), outKept);
    return (int)kept.size();
}
int hfs_expand_word_ids(int n, const int* index, const int* wordIds, int count, int firstNewWordId, int* out) {
    std::vector<int> all;
    if (!FeatureSelect::expandWordIds(n, index, wordIds, count, firstNewWordId, all)) return 0;
    std::copy(all.begin(), all.end(), out);
    return 1;
}
void hmem_destroy(void* h) { delete (MemoryHip*)h; }
void* hmem_vwd(void* h) { return ((MemoryHip*)h)->getVWDictionary(); }
int hmem_update(void* h, const void* desc, int rows, int cols, int type, int nq, int* outIds) {
    std::vector<int> ids;
    const int id = ((MemoryHip*)h)->update(make_mat(desc, rows, cols, type), nq, ids);
    for (size_t i = 0; i < ids.size(); ++i) outIds[i] = ids[i];
    return id;
}
int hmem_add_signature(void* h, int id, const int* wordIds, int n) {
    return ((MemoryHip*)h)->addSignature(std::vector<int>(wordIds, wordIds + n), id);
}
void hmem_forget(void* h, int sigId) { ((MemoryHip*)h)->forget(sigId); }
// the statistics under the reference's names (MemoryHip::getStatistics): value of `name`, -1 if there is no such key; name == NULL: the
// number of keys; refresh != 0: the engine figures are read first (synchronises)
float hmem_statistic(void* h, const char* name, int refresh) {
    MemoryHip* m = (MemoryHip*)h;
    if (refresh) m->refreshEngineStatistics();
    if (!name) return (float)m->getStatistics().size();
    std::map<std::string, float>::const_iterator it = m->getStatistics().find(name);
    return it == m->getStatistics().end() ? -1.0f : it->second;
}
int hmem_set_engine_option(void* h, const char* key, long value) {
    VWDictionaryHip* d = ((MemoryHip*)h)->getVWDictionary();
    return d->engine() ? lcd_set_option(d->engine(), key, (int64_t)value) : -1;
}
int hmem_get_ni(void* h, int sigId) { return ((MemoryHip*)h)->getNi(sigId); }
long hmem_num_signatures(void* h) { return (long)((MemoryHip*)h)->signaturesSize(); }
int hmem_compute_likelihood(void* h, const int* words, int nwords, const int* ids, int nids, int* outIds, float* out) {
    std::map<int, float> L = ((MemoryHip*)h)->computeLikelihood(std::list<int>(words, words + nwords), std::list<int>(ids, ids + nids));
    int n = 0;
    for (std::map<int, float>::iterator i = L.begin(); i != L.end(); ++i, ++n) { outIds[n] = i->first; out[n] = i->second; }
    return n;
}

// The per-frame loop a caller of the reference's interface runs, timed inside C++ (bench.py's `cpp_interface_ms_per_step`): Memory::update
// (-> VWDictionary::addNewWords) of frame i, Memory::computeLikelihood of the new signature against every signature in memory
// (Rtabmap.cpp:2046-2117 builds that list), the oldest signature forgotten (WM -> LTM).  Returns the mean milliseconds per frame.
double hmem_time_loop(void* h, const void* descs, int n_frames, int rows, int cols, int type, int steps) {
    MemoryHip* m = (MemoryHip*)h;
    const size_t frame_bytes = (size_t)rows * cols * (type == 0 ? 4 : 1);
    std::vector<int> ids;
    double total = 0.0;
    for (int i = 0; i < steps + 2; ++i) {
        const auto t0 = std::chrono::steady_clock::now();
        const Mat d = make_mat((const char*)descs + (size_t)(i % n_frames) * frame_bytes, rows, cols, type);
        const int id = m->update(d, -1, ids);
        const std::vector<int> all = m->signatureIds();
        std::list<int> lst(all.begin(), all.end());
        const std::map<int, float> L = m->computeLikelihood(id, lst);
        if (!all.empty()) m->forget(all.front());
        if (L.empty()) return -1.0;
        if (i >= 2) total += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    return total / steps;
}

void hmem_set_device_frames(void* h, int on) { ((MemoryHip*)h)->setDeviceFrames(on != 0); }
// Kp/TfIdfLikelihoodUsed: 0 = every computeLikelihood answers with Signature::compareTo's words branch (Memory.cpp:2179-2214)
void hmem_set_tfidf_likelihood_used(void* h, int on) { ((MemoryHip*)h)->setTfIdfLikelihoodUsed(on != 0); }
// sigA->compareTo(*sigB) for two signatures in memory (the comparison of Memory::rehearsal, Memory.cpp:4245)
float hmem_compare_to(void* h, int a, int b) { return ((MemoryHip*)h)->compareTo(a, b); }
// SensorData::setGlobalDescriptors of a signature in memory: n descriptors, types[i] / dims[i], their floats one behind the other in `data`
// (1: stored, 0: refused -- MemoryHip::setGlobalDescriptors); n == 0 is clearGlobalDescriptors
int hmem_set_global_descriptors(void* h, int sigId, int n, const int* types, const int* dims, const float* data) {
    if (n <= 0) { ((MemoryHip*)h)->clearGlobalDescriptors(sigId); return 1; }
    std::vector<MemoryHip::GlobalDescriptor> g((size_t)n);
    for (int i = 0; i < n; ++i) {
        g[(size_t)i].type = types[i];
        if (dims[i] > 0) g[(size_t)i].data.assign(data, data + dims[i]);
        data += dims[i] > 0 ? dims[i] : 0;
    }
    return ((MemoryHip*)h)->setGlobalDescriptors(sigId, g) ? 1 : 0;
}
// globalDescriptors().size() of a signature in memory (0: none, or no such signature)
int hmem_num_global_descriptors(void* h, int sigId) { return (int)((MemoryHip*)h)->globalDescriptors(sigId).size(); }
// mean milliseconds a device-resident update() spent inside lcd_frame_host so far (-1: none ran)
double hmem_fast_frame_device_ms(void* h) {
    long long ns = 0, calls = 0;
    ((MemoryHip*)h)->getVWDictionary()->fastFrameStats(&ns, &calls);
    return calls ? 1e-6 * (double)ns / (double)calls : -1.0;
}
// n signatures of q words each (ids first_id, first_id + 1, ...) through addSignature, then ONE bulk registration on the device
int hmem_add_signatures_bulk(void* h, const int* words, int n, int q, int first_id) {
    MemoryHip* m = (MemoryHip*)h;
    for (int s = 0; s < n; ++s)
        if (m->addSignature(std::vector<int>(words + (size_t)s * q, words + (size_t)(s + 1) * q), first_id + s) != first_id + s) return -1;
    return m->flushReferencesBulk() ? n : -1;
}
// computeLikelihoodFlat of the signature update() has just created: returns the number of entries (-1: no result at hand)
int hmem_compute_likelihood_flat(void* h, int sigId, int* outIds, float* out, int cap) {
    std::vector<int> ids; std::vector<float> v;
    if (!((MemoryHip*)h)->computeLikelihoodFlat(sigId, ids, v)) return -1;
    for (size_t i = 0; i < ids.size() && (int)i < cap; ++i) { outIds[i] = ids[i]; out[i] = v[i]; }
    return (int)ids.size();
}
// Memory::computeLikelihood(signature id, ids) -- the overload Rtabmap::process calls (Rtabmap.cpp:2117): after update() it is answered
// from the frame's own device call
int hmem_compute_likelihood_of(void* h, int sigId, const int* ids, int nids, int* outIds, float* out) {
    std::map<int, float> L = ((MemoryHip*)h)->computeLikelihood(sigId, std::list<int>(ids, ids + nids));
    int n = 0;
    for (std::map<int, float>::iterator i = L.begin(); i != L.end(); ++i, ++n) { outIds[n] = i->first; out[n] = i->second; }
    return n;
}

// hmem_time_loop with the three ways a caller can take the likelihood (bench.py's cpp_interface_* keys), the caller's own list of ids
// kept from frame to frame (one push, one pop) instead of rebuilt: mode 0 = std::map by value (the reference's signature), 1 = into a
// caller-owned std::map updated in place, 2 = flat vectors.  out4 = mean ms per frame of {whole step, update, computeLikelihood, forget}.
int hmem_time_loop_modes(void* h, const void* descs, int n_frames, int rows, int cols, int type, int steps, int mode, double* out4) {
    MemoryHip* m = (MemoryHip*)h;
    const size_t frame_bytes = (size_t)rows * cols * (type == 0 ? 4 : 1);
    std::vector<int> ids;
    const std::vector<int> all0 = m->signatureIds();
    std::list<int> lst(all0.begin(), all0.end());
    std::map<int, float> keep;
    std::vector<int> fi; std::vector<float> fv;
    double t[4] = {0, 0, 0, 0};
    for (int i = 0; i < steps + 2; ++i) {
        const auto t0 = std::chrono::steady_clock::now();
        const Mat d = make_mat((const char*)descs + (size_t)(i % n_frames) * frame_bytes, rows, cols, type);
        const int id = m->update(d, -1, ids);
        lst.push_back(id);
        const auto t1 = std::chrono::steady_clock::now();
        size_t n_out = 0;
        if (mode == 0) { const std::map<int, float> L = m->computeLikelihood(id, lst); n_out = L.size(); }
        else if (mode == 1) { m->computeLikelihood(id, lst, keep); n_out = keep.size(); }
        else { if (!m->computeLikelihoodFlat(id, fi, fv)) return -1; n_out = fi.size(); }
        const auto t2 = std::chrono::steady_clock::now();
        if (!lst.empty()) { m->forget(lst.front()); lst.pop_front(); }
        const auto t3 = std::chrono::steady_clock::now();
        if (n_out == 0) return -1;
        if (i >= 2) {
            t[0] += std::chrono::duration<double, std::milli>(t3 - t0).count();
            t[1] += std::chrono::duration<double, std::milli>(t1 - t0).count();
            t[2] += std::chrono::duration<double, std::milli>(t2 - t1).count();
            t[3] += std::chrono::duration<double, std::milli>(t3 - t2).count();
        }
    }
    for (int k = 0; k < 4; ++k) out4[k] = t[k] / steps;
    return 0;
}

// the values the mirror's classes take when no parameter is given (tests/test_parameter_defaults.py compares them with the defaults of
// the reference's Parameters.h): out[0..7] = Kp/NndrRatio, Kp/IncrementalDictionary, Kp/NewWordsComparedTogether, Mem/STMSize,
// Rtabmap/LoopThr, Rtabmap/LoopRatio, Bayes/VirtualPlacePriorThr, Bayes/FullPredictionUpdate; then the Bayes/PredictionLC values.
// Returns the number of PredictionLC values.  No device call is made (the engine is created on first use).
int hparams_defaults(double* out, int cap) {
    RtabmapHip r((ParametersMap()));
    const VWDictionaryHip* d = r.getMemory()->getVWDictionary();
    out[0] = d->getNndrRatio(); out[1] = d->isIncremental() ? 1 : 0; out[2] = d->isNewWordsComparedTogether() ? 1 : 0;
    out[3] = r.getMemory()->getMaxStMemSize(); out[4] = r.getLoopThr(); out[5] = r.getLoopRatio();
    out[6] = r.getBayesFilter()->getVirtualPlacePrior(); out[7] = r.getBayesFilter()->isFullPredictionUpdate() ? 1 : 0;
    const std::vector<double>& lc = r.getBayesFilter()->getPredictionLC();
    for (size_t i = 0; i < lc.size() && 8 + (int)i < cap; ++i) out[8 + i] = lc[i];
    return (int)lc.size();
}

// uStr2Float as the mirror's parameter parsing uses it (VWDictionaryHip.h; the reference's: utilite UConversion.cpp)
float hutil_str2float(const char* s) { return uStr2Float(std::string(s ? s : "")); }

// ---- the database reader (DbLoaderHip.h): no device call is made by the hdb_* entries
struct HDb { DbLoaderHip db; DbDictionary dict; DbSignatures sigs; };
void* hdb_open(const char* path) {
    HDb* h = new HDb();
    if (!h->db.open(path ? path : "")) { delete h; return nullptr; }
    return h;
}
void hdb_close(void* h) { delete (HDb*)h; }
const char* hdb_version(void* h) { return ((HDb*)h)->db.version().c_str(); }
const char* hdb_last_error(void* h) { return ((HDb*)h)->db.lastError().c_str(); }
// out4: type (0 = CV_8U, 5 = CV_32F, -1 none), descriptor size, last word id, bytes of the rows; returns the number of words, -1 on error
int hdb_load_dictionary(void* h, int lastStateOnly, int* out4) {
    HDb* d = (HDb*)h;
    if (!d->db.loadDictionary(d->dict, lastStateOnly != 0)) return -1;
    out4[0] = d->dict.type; out4[1] = d->dict.cols; out4[2] = d->dict.lastWordId; out4[3] = (int)d->dict.rows.size();
    return (int)d->dict.wordIds.size();
}
void hdb_dictionary_copy(void* h, int* wordIds, unsigned char* rows) {
    HDb* d = (HDb*)h;
    if (!d->dict.wordIds.empty()) std::memcpy(wordIds, d->dict.wordIds.data(), d->dict.wordIds.size() * sizeof(int));
    if (!d->dict.rows.empty()) std::memcpy(rows, d->dict.rows.data(), d->dict.rows.size());
}
// returns the number of signatures (-1 on error); *nWords = total word entries
int hdb_load_signatures(void* h, int lastStateOnly, long long* nWords) {
    HDb* d = (HDb*)h;
    if (!d->db.loadSignatureWords(d->sigs, lastStateOnly != 0)) return -1;
    *nWords = (long long)d->sigs.wordIds.size();
    return (int)d->sigs.sigIds.size();
}
void hdb_signatures_copy(void* h, int* sigIds, long long* offsets, int* wordIds, int* ni) {
    HDb* d = (HDb*)h;
    const size_t n = d->sigs.sigIds.size();
    if (n) { std::memcpy(sigIds, d->sigs.sigIds.data(), n * sizeof(int)); std::memcpy(ni, d->sigs.ni.data(), n * sizeof(int)); }
    for (size_t i = 0; i < d->sigs.offsets.size(); ++i) offsets[i] = (long long)d->sigs.offsets[i];
    if (!d->sigs.wordIds.empty()) std::memcpy(wordIds, d->sigs.wordIds.data(), d->sigs.wordIds.size() * sizeof(int));
}
int hdb_get_ni(void* h, int nodeId) { return ((HDb*)h)->db.getNi(nodeId); }
int hdb_version_cmp(const char* a, const char* b) { return DbLoaderHip::versionCmp(a, b); }
// Memory::loadDataFromDb through the mirror (device: the dictionary's update() and ONE bulk registration)
int hmem_load_data_from_db(void* h, const char* path, int lastStateOnly) { return ((MemoryHip*)h)->loadDataFromDb(path ? path : "", lastStateOnly != 0); }
const char* hmem_load_error(void* h) { return ((MemoryHip*)h)->loadError().c_str(); }

// type 1: Memory::addLink of a global loop closure; type 0: a neighbour link as the database hands it to a replayed signature
int hmem_add_link(void* h, int from, int to, int type) {
    return ((MemoryHip*)h)->addLink(from, to, type == 0 ? MemoryHip::kNeighbor : MemoryHip::kGlobalClosure) ? 1 : 0;
}
int hmem_get_neighbors_id(void* h, int sigId, int maxGraphDepth, int* outIds, int* outMargins, int cap) {
    std::map<int, int> n = ((MemoryHip*)h)->getNeighborsId(sigId, maxGraphDepth);
    int k = 0;
    for (std::map<int, int>::iterator i = n.begin(); i != n.end(); ++i, ++k) if (k < cap) { outIds[k] = i->first; outMargins[k] = i->second; }
    return (int)n.size();
}
// which: 0 short-term memory, 1 working memory (the virtual place -1 included)
int hmem_ids(void* h, int which, int* out, int cap) {
    const std::set<int>& s = which == 0 ? ((MemoryHip*)h)->getStMem() : ((MemoryHip*)h)->getWorkingMem();
    int k = 0;
    for (std::set<int>::const_iterator i = s.begin(); i != s.end(); ++i, ++k) if (k < cap) out[k] = *i;
    return (int)s.size();
}

void* hbayes_create(const char* predictionLC, float virtualPlacePrior, int fullPredictionUpdate) {
    ParametersMap p;
    if (predictionLC && predictionLC[0]) p["Bayes/PredictionLC"] = predictionLC;
    p["Bayes/VirtualPlacePriorThr"] = std::to_string(virtualPlacePrior);
    p["Bayes/FullPredictionUpdate"] = fullPredictionUpdate ? "true" : "false";
    return new BayesFilterHip(p);
}
void hbayes_destroy(void* b) { delete (BayesFilterHip*)b; }
void hbayes_reset(void* b) { ((BayesFilterHip*)b)->reset(); }
void hbayes_set_prediction_lc(void* b, const char* s) { ((BayesFilterHip*)b)->setPredictionLC(s); }
int hbayes_get_prediction_lc(void* b, double* out, int cap) {
    const std::vector<double>& v = ((BayesFilterHip*)b)->getPredictionLC();
    for (size_t i = 0; i < v.size() && (int)i < cap; ++i) out[i] = v[i];
    return (int)v.size();
}
// BayesFilter::computePosterior(memory, likelihood); returns the size of the posterior map, written to outIds / out; hyp = the
// highest hypothesis (id, value) as Rtabmap.cpp:2147-2158 reads it off
int hbayes_compute_posterior(void* b, void* mem, const int* ids, const float* values, int n, int* outIds, float* out, int cap, int* hypId,
                             float* hypValue) {
    std::map<int, float> L;
    for (int i = 0; i < n; ++i) L[ids[i]] = values[i];
    const std::map<int, float>& P = ((BayesFilterHip*)b)->computePosterior((MemoryHip*)mem, L);
    int k = 0;
    for (std::map<int, float>::const_iterator i = P.begin(); i != P.end(); ++i, ++k) if (k < cap) { outIds[k] = i->first; out[k] = i->second; }
    if (hypId) *hypId = ((BayesFilterHip*)b)->getHighestHypothesis().first;
    if (hypValue) *hypValue = ((BayesFilterHip*)b)->getHighestHypothesis().second;
    return (int)P.size();
}
const char* hbayes_last_error(void* b) { return ((BayesFilterHip*)b)->lastError().c_str(); }

void* hrtab_create(float loopThr, float loopRatio, int virtualPlaceLikelihoodRatio, int stmSize, const char* predictionLC, float virtualPlacePrior,
                   int device) {
    ParametersMap p = make_params(5, 1, 0.8f, 1, "");
    p["Rtabmap/LoopThr"] = std::to_string(loopThr);
    p["Rtabmap/LoopRatio"] = std::to_string(loopRatio);
    p["Rtabmap/VirtualPlaceLikelihoodRatio"] = std::to_string(virtualPlaceLikelihoodRatio);
    p["Mem/STMSize"] = std::to_string(stmSize);
    if (predictionLC && predictionLC[0]) p["Bayes/PredictionLC"] = predictionLC;
    p["Bayes/VirtualPlacePriorThr"] = std::to_string(virtualPlacePrior);
    return new RtabmapHip(p, device);
}
void hrtab_destroy(void* r) { delete (RtabmapHip*)r; }
void* hrtab_memory(void* r) { return ((RtabmapHip*)r)->getMemory(); }
// Rtabmap::process for one frame of descriptors; out4 = {last location id, highest hypothesis id, loop closure id, processed}
int hrtab_process(void* r, const void* desc, int rows, int cols, int type, int* out4, float* outValues2) {
    RtabmapHip* R = (RtabmapHip*)r;
    const bool ok = R->process(make_mat(desc, rows, cols, type));
    out4[0] = R->getLastLocationId(); out4[1] = R->getHighestHypothesisId(); out4[2] = R->getLoopClosureId(); out4[3] = ok ? 1 : 0;
    outValues2[0] = R->getHighestHypothesisValue(); outValues2[1] = R->getLoopClosureValue();
    return ok ? 1 : 0;
}
// which: 0 raw likelihood, 1 adjusted likelihood, 2 posterior of the last frame
int hrtab_vector(void* r, int which, int* outIds, float* out, int cap) {
    RtabmapHip* R = (RtabmapHip*)r;
    const std::map<int, float>& m = which == 0 ? R->getRawLikelihood() : which == 1 ? R->getLikelihood() : R->getPosterior();
    int k = 0;
    for (std::map<int, float>::const_iterator i = m.begin(); i != m.end(); ++i, ++k) if (k < cap) { outIds[k] = i->first; out[k] = i->second; }
    return (int)m.size();
}
// hrtab_create with the epipolar check's parameters: VhEp/Enabled, VhEp/MatchCountMin, VhEp/RansacParam1
void* hrtab_create_epipolar(float loopThr, float loopRatio, int virtualPlaceLikelihoodRatio, int stmSize, const char* predictionLC, float virtualPlacePrior,
                            int device, int epipolarEnabled, int matchCountMin, float ransacParam1) {
    ParametersMap p = make_params(5, 1, 0.8f, 1, "");
    p["Rtabmap/LoopThr"] = std::to_string(loopThr);
    p["Rtabmap/LoopRatio"] = std::to_string(loopRatio);
    p["Rtabmap/VirtualPlaceLikelihoodRatio"] = std::to_string(virtualPlaceLikelihoodRatio);
    p["Mem/STMSize"] = std::to_string(stmSize);
    if (predictionLC && predictionLC[0]) p["Bayes/PredictionLC"] = predictionLC;
    p["Bayes/VirtualPlacePriorThr"] = std::to_string(virtualPlacePrior);
    p["VhEp/Enabled"] = epipolarEnabled ? "true" : "false";
    p["VhEp/MatchCountMin"] = std::to_string(matchCountMin);
    p["VhEp/RansacParam1"] = std::to_string(ransacParam1);
    return new RtabmapHip(p, device);
}
// hrtab_process with the frame's keypoints, [rows x 2]
int hrtab_process_keypoints(void* r, const void* desc, int rows, int cols, int type, const float* keypoints, int* out4, float* outValues2) {
    RtabmapHip* R = (RtabmapHip*)r;
    const std::vector<float> kp(keypoints, keypoints + (size_t)rows * 2);
    const bool ok = R->process(make_mat(desc, rows, cols, type), kp);
    out4[0] = R->getLastLocationId(); out4[1] = R->getHighestHypothesisId(); out4[2] = R->getLoopClosureId(); out4[3] = ok ? 1 : 0;
    outValues2[0] = R->getHighestHypothesisValue(); outValues2[1] = R->getLoopClosureValue();
    return ok ? 1 : 0;
}
// epipolar_cpu (no engine involved).  outFundamental[9], outScalars[3] = status, pairs, inliers; outMatches / outInliers hold nTo ids.  1 = done, 0 = refused
int hepi_cpu(const int* fromIds, const float* fromPoints, int nFrom, const int* toIds, const float* toPoints, int nTo, int matchCountMin, int iterations,
             double ransacParam1, unsigned seed, float* outFundamental, int* outScalars, int* outMatches, int* outInliers) {
    EpipolarParams p;
    p.matchCountMin = matchCountMin; p.iterations = iterations; p.ransacParam1 = ransacParam1; p.seed = seed;
    EpipolarResult r;
    if (!epipolar_cpu(fromIds, fromPoints, nFrom, toIds, toPoints, nTo, p, r)) return 0;
    std::copy(r.fundamental, r.fundamental + 9, outFundamental);
    outScalars[0] = r.status; outScalars[1] = (int)r.matches.size(); outScalars[2] = (int)r.inliers.size();
    std::copy(r.matches.begin(), r.matches.end(), outMatches);
    std::copy(r.inliers.begin(), r.inliers.end(), outInliers);
    return 1;
}
// EpipolarGeometryHip::check and findFFromWords through the dictionary's engine.  outStatus: one byte per pair (cap nB); outScalars[3] = the
// engine's status, pairs, accepted; returns 1 when the engine took the call
int hepi_check(void* h, const int* idsA, const float* pointsA, int nA, const int* idsB, const float* pointsB, int nB, int matchCountMin, double ransacParam1,
               double ransacParam2, unsigned seed, float* outFundamental, unsigned char* outStatus, int* outPairs, int* outScalars) {
    ParametersMap p;
    p["VhEp/MatchCountMin"] = std::to_string(matchCountMin);
    p["VhEp/RansacParam1"] = std::to_string(ransacParam1);
    p["VhEp/RansacParam2"] = std::to_string(ransacParam2);
    const EpipolarGeometryHip epi(p);
    const std::vector<int> a(idsA, idsA + nA), b(idsB, idsB + nB);
    const std::vector<float> pa(pointsA, pointsA + (size_t)nA * 2), pb(pointsB, pointsB + (size_t)nB * 2);
    lcd_engine* engine = ((VWDictionaryHip*)h)->engine();
    std::vector<unsigned char> status;
    std::vector<int> pairs;
    int st = 0;
    if (!epi.findFFromWords(engine, a, pa, b, pb, outFundamental, status, &pairs, &st, seed)) return 0;
    std::copy(status.begin(), status.end(), outStatus);
    std::copy(pairs.begin(), pairs.end(), outPairs);
    outScalars[0] = st; outScalars[1] = (int)pairs.size();
    return 1;
}
// EpipolarGeometryHip::check alone: 1 accepted, 0 rejected or refused
int hepi_accept(void* h, const int* idsA, const float* pointsA, int nA, const int* idsB, const float* pointsB, int nB, int matchCountMin, double ransacParam1,
                double ransacParam2, unsigned seed) {
    ParametersMap p;
    p["VhEp/MatchCountMin"] = std::to_string(matchCountMin);
    p["VhEp/RansacParam1"] = std::to_string(ransacParam1);
    p["VhEp/RansacParam2"] = std::to_string(ransacParam2);
    const EpipolarGeometryHip epi(p);
    const std::vector<int> a(idsA, idsA + nA), b(idsB, idsB + nB);
    const std::vector<float> pa(pointsA, pointsA + (size_t)nA * 2), pb(pointsB, pointsB + (size_t)nB * 2);
    return epi.check(((VWDictionaryHip*)h)->engine(), a, pa, b, pb, seed) ? 1 : 0;
}
// motion_mono_cpu (no engine involved).  camera[4] = fx, fy, cx, cy; local, guess: NULL or 12 floats; fromPoints3 may be NULL.  outScalars[3] =
// status, matches, inliers; outMatches / outInliers hold nTo ids, outPoints3 nTo x 3 floats.  1 = done, 0 = refused
int hmono_cpu(const int* fromIds, const float* fromPoints, const float* fromPoints3, int nFrom, const int* toIds, const float* toPoints, int nTo,
              int minInliers, int iterations, unsigned seed, double reprojThreshold, int varianceMedianRatio, float maxVariance, double distanceThreshold,
              const float* camera, const float* local, const float* guess, float* outTransform, double* outVariance, int* outScalars, int* outMatches,
              int* outInliers, float* outPoints3) {
    MotionMonoParams p;
    p.minInliers = minInliers; p.iterations = iterations; p.seed = seed; p.reprojThreshold = reprojThreshold; p.varianceMedianRatio = varianceMedianRatio;
    p.maxVariance = maxVariance; p.distanceThreshold = distanceThreshold;
    p.fx = camera[0]; p.fy = camera[1]; p.cx = camera[2]; p.cy = camera[3];
    p.hasLocalTransform = local != nullptr;
    if (local) std::copy(local, local + 12, p.localTransform);
    p.hasGuess = guess != nullptr;
    if (guess) std::copy(guess, guess + 12, p.guess);
    MotionMonoResult r;
    if (!motion_mono_cpu(fromIds, fromPoints, fromPoints3, nFrom, toIds, toPoints, nTo, p, r)) return 0;
    std::copy(r.transform, r.transform + 12, outTransform);
    *outVariance = r.variance;
    outScalars[0] = r.status; outScalars[1] = (int)r.matches.size(); outScalars[2] = (int)r.inliers.size();
    std::copy(r.matches.begin(), r.matches.end(), outMatches);
    std::copy(r.inliers.begin(), r.inliers.end(), outInliers);
    std::copy(r.points3.begin(), r.points3.end(), outPoints3);
    return 1;
}
// MotionMonoHip::estimate through the dictionary's engine; arguments and outputs as hmono_cpu's; returns 1 when the engine took the call
int hmono_estimate(void* h, const int* idsA, const float* pointsA, const float* points3A, int nA, const int* idsB, const float* pointsB, int nB,
                   int minInliers, double reprojThreshold, int varianceMedianRatio, float maxVariance, unsigned seed, const float* camera,
                   const float* local, const float* guess, float* outTransform, double* outVariance, int* outScalars, int* outMatches, int* outInliers,
                   float* outPoints3) {
    MotionMonoHip mono;                                                 // the values as they are: a decimal string would round them
    mono.setMinInliers(minInliers); mono.setReprojThreshold(reprojThreshold); mono.setVarianceMedianRatio(varianceMedianRatio);
    mono.setMaxVariance(maxVariance);
    const std::vector<int> a(idsA, idsA + nA), b(idsB, idsB + nB);
    const std::vector<float> pa(pointsA, pointsA + (size_t)nA * 2), pb(pointsB, pointsB + (size_t)nB * 2);
    const std::vector<float> p3 = points3A ? std::vector<float>(points3A, points3A + (size_t)nA * 3) : std::vector<float>();
    lcd_camera cam;
    cam.fx = camera[0]; cam.fy = camera[1]; cam.cx = camera[2]; cam.cy = camera[3];
    cam.image_width = 0; cam.image_height = 0; cam.has_local_transform = local ? 1 : 0; cam.reserved = 0;
    for (int k = 0; k < 12; ++k) cam.local_transform[k] = local ? local[k] : 0.0f;
    MotionMonoResult r;
    if (!mono.estimate(((VWDictionaryHip*)h)->engine(), a, pa, p3, b, pb, cam, guess, r, seed)) return 0;
    std::copy(r.transform, r.transform + 12, outTransform);
    *outVariance = r.variance;
    outScalars[0] = r.status; outScalars[1] = (int)r.matches.size(); outScalars[2] = (int)r.inliers.size();
    std::copy(r.matches.begin(), r.matches.end(), outMatches);
    std::copy(r.inliers.begin(), r.inliers.end(), outInliers);
    std::copy(r.points3.begin(), r.points3.end(), outPoints3);
    return 1;
}
// the number of signatures whose words and keypoints a RtabmapHip keeps for the epipolar check
int hrtab_epipolar_kept(void* r) { return ((RtabmapHip*)r)->getEpipolarKept(); }
int hrtab_last_word_ids(void* r, int* out, int cap) {
    const std::vector<int>& v = ((RtabmapHip*)r)->getLastWordIds();
    for (size_t i = 0; i < v.size() && (int)i < cap; ++i) out[i] = v[i];
    return (int)v.size();
}

}  // extern "C"
