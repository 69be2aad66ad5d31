// MemoryHip.cpp -- see MemoryHip.h.
#include "MemoryHip.h"

#include "DbLoaderHip.h"
#include "FeatureSelect.h"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <set>

namespace rtabmap_amd {

const int MemoryHip::kIdVirtual = -1;

namespace {
// a roctx range on the engine's track (lcd_set_option "roctx"; a no-op otherwise) + the elapsed milliseconds, like the UTimer the
// reference wraps around the same stages
struct Stage {
    lcd_engine* eng; std::chrono::steady_clock::time_point t0;
    Stage(VWDictionaryHip* vwd, const char* name) : eng(vwd->engine()), t0(std::chrono::steady_clock::now()) { if (eng) lcd_trace_push(eng, name); }
    ~Stage() { if (eng) lcd_trace_pop(eng); }
    float ms() const { return std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
};
}  // namespace

MemoryHip::MemoryHip(const ParametersMap& parameters, int device)
    : _vwd(new VWDictionaryHip(parameters, device)), _idCount(0), _maxStMemSize(10), _maxFeatures(500), _gridRows(1), _gridCols(1), _ssc(false), _minDepth(0.0f), _maxDepth(0.0f), _deviceFrames(true), _tfIdfLikelihoodUsed(true), _likeSig(0), _likeSortedValid(false) {
    ParametersMap::const_iterator it = parameters.find("Mem/STMSize");
    if (it != parameters.end()) _maxStMemSize = atoi(it->second.c_str());
    it = parameters.find("Kp/TfIdfLikelihoodUsed");
    if (it != parameters.end()) _tfIdfLikelihoodUsed = !(it->second == "false" || it->second == "0" || it->second == "False" || it->second == "FALSE");
    if (_maxStMemSize < 0) _maxStMemSize = 0;
    if ((it = parameters.find("Kp/MaxFeatures")) != parameters.end()) _maxFeatures = atoi(it->second.c_str());
    if ((it = parameters.find("Kp/GridRows")) != parameters.end()) _gridRows = atoi(it->second.c_str());
    if ((it = parameters.find("Kp/MinDepth")) != parameters.end()) _minDepth = (float)atof(it->second.c_str());
    if ((it = parameters.find("Kp/MaxDepth")) != parameters.end()) _maxDepth = (float)atof(it->second.c_str());
    if ((it = parameters.find("Kp/GridCols")) != parameters.end()) _gridCols = atoi(it->second.c_str());
    if ((it = parameters.find("Stereo/WinWidth")) != parameters.end()) _stereo.winWidth = atoi(it->second.c_str());
    if ((it = parameters.find("Stereo/WinHeight")) != parameters.end()) _stereo.winHeight = atoi(it->second.c_str());
    if ((it = parameters.find("Stereo/MaxLevel")) != parameters.end()) _stereo.maxLevel = atoi(it->second.c_str());
    if ((it = parameters.find("Stereo/Iterations")) != parameters.end()) _stereo.iterations = atoi(it->second.c_str());
    if ((it = parameters.find("Stereo/Eps")) != parameters.end()) _stereo.eps = atof(it->second.c_str());
    if ((it = parameters.find("Stereo/MinDisparity")) != parameters.end()) _stereo.minDisparity = (float)atof(it->second.c_str());
    if ((it = parameters.find("Stereo/MaxDisparity")) != parameters.end()) _stereo.maxDisparity = (float)atof(it->second.c_str());
    if ((it = parameters.find("Kp/SSC")) != parameters.end()) _ssc = it->second == "true" || it->second == "1" || it->second == "True" || it->second == "TRUE";
    _workingMem.insert(kIdVirtual);             // Memory.cpp:592
    static const char* names[] = {"TimingMem/Pre_update/ms", "TimingMem/Joining_dictionary_update/ms", "TimingMem/Add_new_words/ms",
                                  "Timing/Likelihood_computation/ms", "Timing/Forgetting/ms", "Keypoint/Dictionary_size/words",
                                  "Keypoint/Current_frame/words", "Keypoint/Indexed_words/words", "Keypoint/Index_memory_usage/KB"};
    for (size_t i = 0; i < sizeof(names) / sizeof(names[0]); ++i) _stats[names[i]] = 0.0f;   // (Statistics::_defaultData: every key exists from the start)
}

void MemoryHip::refreshEngineStatistics() {
    _stats["Keypoint/Dictionary_size/words"] = (float)_vwd->getVisualWords().size();
    _stats["Keypoint/Indexed_words/words"] = (float)_vwd->getIndexedWordsCount();
    lcd_stats st;
    if (_vwd->engine() && lcd_get_stats(_vwd->engine(), &st) == LCD_OK) _stats["Keypoint/Index_memory_usage/KB"] = (float)(st.bytes_device / 1024);
}
MemoryHip::~MemoryHip() { delete _vwd; }

void MemoryHip::cleanUnusedWords() {   // Memory.cpp:6899-6920 (no database: the words are deleted)
    std::vector<VisualWord*> removedWords = _vwd->getUnusedWords();
    if (removedWords.size()) {
        _vwd->removeWords(removedWords);
        for (unsigned int i = 0; i < removedWords.size(); ++i) delete removedWords[i];
    }
}

void MemoryHip::preUpdate() {   // Memory.cpp:1004-1016; with Kp/Parallelized the update() runs on PreUpdateThread, joined before addNewWords
    if (_vwd->isIncremental()) this->cleanUnusedWords();
    _vwd->update();
}

int MemoryHip::update(const Mat& descriptors, int nQuantized, std::vector<int>& outIds) {
    Stage whole(_vwd, "Memory::update");
    {
        Stage st(_vwd, "Memory::preUpdate");
        this->preUpdate();
        _stats["TimingMem/Pre_update/ms"] = st.ms();
    }
    Stage quant(_vwd, "VWDictionary::addNewWords");
    const int id = ++_idCount;
    std::list<int> wordIds;
    const int rows = descriptors.rows;
    int nq = nQuantized < 0 || nQuantized > rows ? rows : nQuantized;
    _likeSig = 0;
    bool fast = false;
    if (rows && nq == rows && _deviceFrames && _vwd->isIncremental()) {
        // quantisation + the signature's references + update()'s append + the likelihood of Rtabmap.cpp:2117, one device call
        fast = _vwd->addNewWordsAndScore(descriptors, id, (float)(_signatures.size() + 1), [this](int s) { return this->getNi(s); }, wordIds, _likeSlots);
        if (fast && !_likeSlots.empty() && _tfIdfLikelihoodUsed) { _likeSig = id; _likeSortedValid = false; }   // (the frame's values are TF-IDF)
    }
    if (rows && !fast) {
        if (nq > 0) {
            Mat forQuantization = nq == rows ? descriptors : Mat(nq, descriptors.cols, descriptors.type(), descriptors.data.data());
            wordIds = _vwd->addNewWords(forQuantization, id);
            if ((int)wordIds.size() < rows) {   // Memory.cpp:6029-6046: ids -1,-2,.. for features without a word
                std::vector<int> all(rows, -1);
                int i = 0;
                for (std::list<int>::iterator it = wordIds.begin(); it != wordIds.end(); ++it) all[i++] = *it;
                int neg = -1;
                for (i = 0; i < rows; ++i) if (all[i] < 0) all[i] = neg--;
                wordIds.assign(all.begin(), all.end());
            }
        } else {
            int neg = -1;
            for (int i = 0; i < rows; ++i) wordIds.push_back(neg--);
        }
    }
    _stats["TimingMem/Add_new_words/ms"] = quant.ms();          // (on the device-frame path this also holds the frame's likelihood: one call)
    _stats["Keypoint/Current_frame/words"] = (float)wordIds.size();
    _stats["Keypoint/Dictionary_size/words"] = (float)_vwd->getVisualWords().size();
    _stats["Keypoint/Indexed_words/words"] = (float)_vwd->getIndexedWordsCount();
    _signatures[id] = std::vector<int>(wordIds.begin(), wordIds.end());
    outIds.assign(wordIds.begin(), wordIds.end());
    this->addSignatureToStm(id);
    return id;
}

// Memory.cpp:6026-6049 for a signature whose quantised descriptors are a selection: addNewWords, then the ids back onto all features
bool MemoryHip::quantizeSelected(const Mat& forQuantization, const std::vector<int>* rawIndex, int rows, int id, std::list<int>& wordIds) {
    std::list<int> quantized;
    if (forQuantization.rows) quantized = _vwd->addNewWords(forQuantization, id);
    const std::vector<int32_t> ids(quantized.begin(), quantized.end());
    const int32_t count = (int32_t)ids.size();
    std::vector<int32_t> index((size_t)count);
    for (int32_t j = 0; j < count; ++j) index[(size_t)j] = rawIndex ? (*rawIndex)[(size_t)j] : j;
    std::vector<int> all;
    lcd_engine* eng = _vwd->engine();
    if (eng && rows > 0) {
        // the arrays of a frame share its offsets: count entries of index / ids are valid, rows are written
        std::vector<int32_t> idx((size_t)rows, -1), wid((size_t)rows, 0), out((size_t)rows, 0);
        std::copy(index.begin(), index.end(), idx.begin());
        std::copy(ids.begin(), ids.end(), wid.begin());
        const int64_t offsets[2] = {0, rows};
        lcd_expand_args e;
        e.struct_size = (int32_t)sizeof(e); e.n_frames = 1; e.offsets = offsets; e.count = &count; e.index = idx.data(); e.word_ids = wid.data();
        e.first_new_word_id = 0; e.out_word_ids = out.data(); e.n_features = 0;
        if (lcd_expand_word_ids(eng, &e) != LCD_OK) { _selectError = lcd_last_error(eng); return false; }
        all.assign(out.begin(), out.end());
    } else if (!FeatureSelect::expandWordIds(rows, index.data(), ids.data(), count, 0, all)) {
        _selectError = "expandWordIds: an index outside the frame";
        return false;
    }
    wordIds.assign(all.begin(), all.end());
    return true;
}

int MemoryHip::update(const Mat& descriptors, const std::vector<float>& responses, const std::vector<float>& points, int imageWidth, int imageHeight,
                      const DepthImage& depth, const std::vector<DepthCamera>& cameras, std::vector<int>& outIds, std::vector<float>& keypoints3D,
                      std::vector<int>& keptIndex) {
    const int rows = descriptors.rows;
    _selectError.clear();
    if ((int)responses.size() != rows || (int)points.size() != 2 * rows || cameras.empty()) { _selectError = "one response and one point per descriptor, one camera at least"; return 0; }
    // ---- the depth stage (:5683-5694, :5911-5915)
    std::vector<float> xyz((size_t)rows * 3), keptResponses, keptPoints;
    std::vector<unsigned char> keptRows;
    std::vector<int> kept;
    lcd_engine* eng = _vwd->engine();
    if (eng && rows > 0) {
        std::vector<lcd_camera> cams(cameras.size());
        for (size_t c = 0; c < cameras.size(); ++c) {
            lcd_camera& L = cams[c];
            L.fx = cameras[c].fx; L.fy = cameras[c].fy; L.cx = cameras[c].cx; L.cy = cameras[c].cy;
            L.image_width = cameras[c].imageWidth; L.image_height = cameras[c].imageHeight;
            L.has_local_transform = cameras[c].hasLocalTransform ? 1 : 0; L.reserved = 0;
            std::copy(cameras[c].localTransform, cameras[c].localTransform + 12, L.local_transform);
        }
        lcd_depth_image image;
        image.data = depth.data; image.pitch_bytes = depth.pitchBytes; image.width = depth.width; image.height = depth.height;
        image.type = depth.type; image.n_cameras = (int32_t)cams.size(); image.cameras = cams.data();
        const int64_t offsets[2] = {0, rows};
        int32_t count = 0;
        std::vector<int32_t> index((size_t)rows);
        keptResponses.resize((size_t)rows); keptPoints.resize((size_t)rows * 2); keptRows.resize(descriptors.data.size());
        lcd_keypoints_3d_args k;
        k.struct_size = (int32_t)sizeof(k); k.n_frames = 1; k.filter = LCD_KP3D_FILTER_3D; k.aux_bytes = 0; k.min_depth = _minDepth; k.max_depth = _maxDepth;
        k.offsets = offsets; k.images = &image; k.points = points.data(); k.response = responses.data(); k.rows = descriptors.data.data(); k.aux = 0;
        k.out_count = &count; k.out_index = index.data(); k.out_xyz = xyz.data(); k.out_points = keptPoints.data(); k.out_response = keptResponses.data();
        k.out_rows = keptRows.data(); k.out_aux = 0;
        if (lcd_keypoints_3d(eng, &k) != LCD_OK) { _selectError = lcd_last_error(eng); return 0; }
        kept.assign(index.begin(), index.begin() + count);
        xyz.resize((size_t)count * 3); keptResponses.resize((size_t)count); keptPoints.resize((size_t)count * 2);
        keptRows.resize((size_t)count * descriptors.rowBytes());
    } else {
        if (!Keypoints3D::generateKeypoints3DDepth(points.data(), rows, depth, cameras.data(), (int)cameras.size(), _minDepth, _maxDepth, xyz.data())) {
            _selectError = "generateKeypoints3DDepth: an image the cameras do not divide, or a keypoint that is not finite or in no camera's sub-image";
            return 0;
        }
        if (!Keypoints3D::filterKeypointsByDepth(xyz.data(), rows, _minDepth, _maxDepth, kept)) { _selectError = "filterKeypointsByDepth: Kp/MinDepth < 0 or 0 < Kp/MaxDepth <= Kp/MinDepth"; return 0; }
        std::vector<float> all;
        all.swap(xyz);
        for (size_t j = 0; j < kept.size(); ++j) {
            const size_t i = (size_t)kept[j];
            xyz.insert(xyz.end(), all.begin() + 3 * i, all.begin() + 3 * i + 3);
            keptResponses.push_back(responses[i]);
            keptPoints.push_back(points[2 * i]); keptPoints.push_back(points[2 * i + 1]);
            keptRows.insert(keptRows.end(), descriptors.ptr((int)i), descriptors.ptr((int)i) + descriptors.rowBytes());
        }
    }
    std::vector<int> ids;
    const int id = this->update(Mat((int)kept.size(), descriptors.cols, descriptors.type(), keptRows.data()), keptResponses, keptPoints, imageWidth, imageHeight, ids);
    if (!id) return 0;
    outIds.swap(ids); keypoints3D.swap(xyz); keptIndex.swap(kept);
    return id;
}

int MemoryHip::update(const Mat& descriptors, const std::vector<float>& responses, const std::vector<float>& points, int imageWidth, int imageHeight,
                      const GrayImage& left, const GrayImage& right, const StereoCamera& camera, std::vector<int>& outIds, std::vector<float>& keypoints3D,
                      std::vector<int>& keptIndex) {
    const int rows = descriptors.rows;
    _selectError.clear();
    if ((int)responses.size() != rows || (int)points.size() != 2 * rows) { _selectError = "one response and one point per descriptor"; return 0; }
    if (left.width != right.width || left.height != right.height) { _selectError = "the left and the right image differ in size"; return 0; }
    // ---- the stereo stage (Features2d.cpp:960-1016)
    std::vector<float> xyz((size_t)rows * 3), keptResponses, keptPoints;
    std::vector<unsigned char> keptRows;
    std::vector<int> kept;
    lcd_engine* eng = _vwd->engine();
    if (eng && rows > 0) {
        lcd_stereo_camera cam;
        cam.fx = camera.fx; cam.fy = camera.fy; cam.cx = camera.cx; cam.cy = camera.cy; cam.right_cx = camera.rightCx; cam.baseline = camera.baseline;
        cam.has_local_transform = camera.hasLocalTransform ? 1 : 0; cam.reserved = 0;
        std::copy(camera.localTransform, camera.localTransform + 12, cam.local_transform);
        lcd_stereo_image image;
        image.left = left.data; image.right = right.data; image.left_pitch_bytes = left.pitchBytes; image.right_pitch_bytes = right.pitchBytes;
        image.width = left.width; image.height = left.height; image.camera = &cam;
        lcd_stereo_params sp;
        sp.win_width = _stereo.winWidth; sp.win_height = _stereo.winHeight; sp.max_level = _stereo.maxLevel; sp.iterations = _stereo.iterations;
        sp.eps = _stereo.eps; sp.use_min_eigenvals = _stereo.useMinEigenVals ? 1 : 0; sp.reserved = 0; sp.min_eig_threshold = _stereo.minEigThreshold;
        sp.error_threshold = _stereo.errorThreshold; sp.min_disparity = _stereo.minDisparity; sp.max_disparity = _stereo.maxDisparity;
        const int64_t offsets[2] = {0, rows};
        int32_t count = 0;
        std::vector<int32_t> index((size_t)rows);
        keptResponses.resize((size_t)rows); keptPoints.resize((size_t)rows * 2); keptRows.resize(descriptors.data.size());
        lcd_keypoints_3d_stereo_args k;
        k.struct_size = (int32_t)sizeof(k); k.n_frames = 1; k.filter = LCD_KP3D_FILTER_3D; k.aux_bytes = 0; k.min_depth = _minDepth; k.max_depth = _maxDepth;
        k.offsets = offsets; k.images = &image; k.params = &sp; k.points = points.data(); k.response = responses.data(); k.rows = descriptors.data.data(); k.aux = 0;
        k.out_count = &count; k.out_index = index.data(); k.out_xyz = xyz.data(); k.out_points = keptPoints.data(); k.out_response = keptResponses.data();
        k.out_rows = keptRows.data(); k.out_aux = 0; k.out_right = 0; k.out_status = 0;
        if (lcd_keypoints_3d_stereo(eng, &k) != LCD_OK) { _selectError = lcd_last_error(eng); return 0; }
        kept.assign(index.begin(), index.begin() + count);
        xyz.resize((size_t)count * 3); keptResponses.resize((size_t)count); keptPoints.resize((size_t)count * 2);
        keptRows.resize((size_t)count * descriptors.rowBytes());
    } else {
        const StereoOpticalFlowHip flow(_stereo);
        std::vector<float> rightCorners((size_t)rows * 2);
        std::vector<unsigned char> status((size_t)rows);
        if (!flow.computeCorrespondences(left, right, points.data(), rows, rightCorners.data(), status.data())) {
            _selectError = "computeCorrespondences: Stereo/* parameters or images the rule refuses, or a keypoint that is not finite";
            return 0;
        }
        if (!StereoOpticalFlowHip::generateKeypoints3DStereo(points.data(), rightCorners.data(), rows, camera, status.data(), _minDepth, _maxDepth, xyz.data())) {
            _selectError = "generateKeypoints3DStereo: baseline or fx not above 0";
            return 0;
        }
        if (!Keypoints3D::filterKeypointsByDepth(xyz.data(), rows, _minDepth, _maxDepth, kept)) { _selectError = "filterKeypointsByDepth: Kp/MinDepth < 0 or 0 < Kp/MaxDepth <= Kp/MinDepth"; return 0; }
        std::vector<float> all;
        all.swap(xyz);
        for (size_t j = 0; j < kept.size(); ++j) {
            const size_t i = (size_t)kept[j];
            xyz.insert(xyz.end(), all.begin() + 3 * i, all.begin() + 3 * i + 3);
            keptResponses.push_back(responses[i]);
            keptPoints.push_back(points[2 * i]); keptPoints.push_back(points[2 * i + 1]);
            keptRows.insert(keptRows.end(), descriptors.ptr((int)i), descriptors.ptr((int)i) + descriptors.rowBytes());
        }
    }
    std::vector<int> ids;
    const int id = this->update(Mat((int)kept.size(), descriptors.cols, descriptors.type(), keptRows.data()), keptResponses, keptPoints, imageWidth, imageHeight, ids);
    if (!id) return 0;
    outIds.swap(ids); keypoints3D.swap(xyz); keptIndex.swap(kept);
    return id;
}

int MemoryHip::update(const Mat& descriptors, const std::vector<float>& responses, const std::vector<float>& points, int imageWidth, int imageHeight,
                      std::vector<int>& outIds) {
    const int rows = descriptors.rows;
    const bool grid = _gridRows > 1 || _gridCols > 1;
    _selectError.clear();
    if (!(_maxFeatures > 0 && rows > _maxFeatures)) return this->update(descriptors, -1, outIds);     // :5954: nothing to select
    if ((int)responses.size() != rows || ((grid || _ssc) && (int)points.size() != 2 * rows)) { _selectError = "one response (and one point) per descriptor"; return 0; }
    if (_ssc && grid) { _selectError = "Kp/SSC with a grid above 1 x 1: the reference indexes its covering mask outside its bounds"; return 0; }
    // ---- the selection (:5951-6023)
    std::vector<int> rawIndex;
    Mat forQuantization;
    lcd_engine* eng = _vwd->engine();
    if (eng) {
        const int64_t offsets[2] = {0, rows};
        const int32_t size[2] = {imageWidth, imageHeight};
        int32_t count = 0;
        std::vector<int32_t> index((size_t)rows);
        std::vector<unsigned char> selected(descriptors.data.size());
        lcd_select_args s;
        s.struct_size = (int32_t)sizeof(s); s.n_frames = 1; s.order = LCD_SELECT_KEEP_ORDER; s.max_features = _maxFeatures;
        s.grid_rows = _gridRows < 1 ? 1 : _gridRows; s.grid_cols = _gridCols < 1 ? 1 : _gridCols; s.aux_bytes = 0; s.flags = _ssc ? LCD_SELECT_SSC : 0;
        s.offsets = offsets; s.image_size = size; s.response = responses.data(); s.points = grid || _ssc ? points.data() : 0;
        s.rows = descriptors.data.data(); s.aux = 0; s.out_count = &count; s.out_index = index.data(); s.out_rows = selected.data(); s.out_aux = 0; s.n_in = 0;
        if (lcd_select_features(eng, &s) != LCD_OK) { _selectError = lcd_last_error(eng); return 0; }
        rawIndex.assign(index.begin(), index.begin() + count);
        forQuantization = Mat(count, descriptors.cols, descriptors.type(), selected.data());
    } else {
        std::vector<bool> inliers;
        if (_ssc) {
            if (!FeatureSelect::limitKeypointsSSC(responses.data(), points.data(), rows, _maxFeatures, imageWidth, imageHeight, inliers)) {
                _selectError = "limitKeypoints (Kp/SSC): a NaN response, Kp/MaxFeatures == 1, a keypoint outside the image or an image side outside 1 .. 16384";
                return 0;
            }
        } else if (!FeatureSelect::limitKeypoints(responses.data(), grid ? points.data() : 0, rows, _maxFeatures, imageWidth, imageHeight,
                                                  _gridRows < 1 ? 1 : _gridRows, _gridCols < 1 ? 1 : _gridCols, inliers)) {
            _selectError = "limitKeypoints: a NaN response, a keypoint outside the grid or an image not larger than the grid";
            return 0;
        }
        for (int k = 0; k < rows; ++k) if (inliers[(size_t)k]) rawIndex.push_back(k);
        forQuantization = Mat((int)rawIndex.size(), descriptors.cols, descriptors.type());
        for (size_t j = 0; j < rawIndex.size(); ++j)
            std::copy(descriptors.ptr(rawIndex[j]), descriptors.ptr(rawIndex[j]) + descriptors.rowBytes(), forQuantization.data.begin() + j * descriptors.rowBytes());
    }
    // ---- the frame, as update(descriptors, nQuantized, ..) runs one whose descriptors are not all quantised
    Stage whole(_vwd, "Memory::update");
    {
        Stage st(_vwd, "Memory::preUpdate");
        this->preUpdate();
        _stats["TimingMem/Pre_update/ms"] = st.ms();
    }
    Stage quant(_vwd, "VWDictionary::addNewWords");
    const int id = ++_idCount;
    _likeSig = 0;
    std::list<int> wordIds;
    if (!this->quantizeSelected(forQuantization, &rawIndex, rows, id, wordIds)) return 0;
    _stats["TimingMem/Add_new_words/ms"] = quant.ms();
    _stats["Keypoint/Current_frame/words"] = (float)wordIds.size();
    _stats["Keypoint/Dictionary_size/words"] = (float)_vwd->getVisualWords().size();
    _stats["Keypoint/Indexed_words/words"] = (float)_vwd->getIndexedWordsCount();
    _signatures[id] = std::vector<int>(wordIds.begin(), wordIds.end());
    outIds.assign(wordIds.begin(), wordIds.end());
    this->addSignatureToStm(id);
    return id;
}

// Memory::addSignatureToStm :1146-1230 (the neighbour link to the newest signature of the short-term memory; poses and covariances
// are out of scope) followed by the transfer loop of Memory::update :1112-1135 (no intermediate nodes here: every signature counts)
void MemoryHip::addSignatureToStm(int id) {
    if (_stMem.size()) {
        const int last = *_stMem.rbegin();
        _links[id][last] = kNeighbor;
        _links[last][id] = kNeighbor;
    }
    _stMem.insert(id);
    while (_stMem.size() && _maxStMemSize > 0 && (int)_stMem.size() > _maxStMemSize) {
        const int oldest = *_stMem.begin();     // moveSignatureToWMFromSTM :1442-1500 without graph reduction
        _workingMem.insert(oldest);
        _stMem.erase(oldest);
    }
}

// Memory::addLink :3877-3935 for a loop closure between two signatures in memory: nothing to do (true) when they are linked
// already, false + error when one of them is not in the working / short-term memory (weights are out of scope)
bool MemoryHip::addLink(int from, int to, LinkType type) {
    if (!_signatures.count(from) || !_signatures.count(to)) {
        if (!_signatures.count(from)) fprintf(stderr, "[ERROR] from=%d, to=%d, Signature %d not found in working/st memories\n", from, to, from);
        if (!_signatures.count(to)) fprintf(stderr, "[ERROR] from=%d, to=%d, Signature %d not found in working/st memories\n", from, to, to);
        return false;
    }
    if (from == to) return false;
    std::map<int, std::map<int, LinkType> >::const_iterator l = _links.find(to);
    if (l != _links.end() && l->second.count(from)) return true;
    _links[from][to] = type;
    _links[to][from] = type;
    return true;
}

// Memory::getNeighborsId(id, maxGraphDepth, 0, false, false, true, true) :1703-1893.  Level by level over the neighbour links; a
// loop-closure link puts its far end on the SAME level as the node it leaves from (incrementMarginOnLoop = false) and a node is
// taken that way only once per call; nodes that are not in memory are neither reported nor expanded (maxCheckedInDatabase = 0).
// Intermediate nodes, landmarks and local-space closures do not exist in this subset.  maxGraphDepth = 0: no limit.
std::map<int, int> MemoryHip::getNeighborsId(int signatureId, int maxGraphDepth) const {
    std::map<int, int> found;
    if (signatureId <= 0 || maxGraphDepth < 0) return found;
    std::set<int> nextLevel, viaClosure;
    nextLevel.insert(signatureId);
    for (int margin = 0; (maxGraphDepth == 0 || margin < maxGraphDepth) && !nextLevel.empty(); ++margin) {
        std::list<int> level(nextLevel.rbegin(), nextLevel.rend());       // most recent first, as the reference walks a level
        nextLevel.clear();
        for (std::list<int>::iterator n = level.begin(); n != level.end(); ++n) {
            if (found.count(*n) || !_signatures.count(*n)) continue;
            found[*n] = margin;
            std::map<int, std::map<int, LinkType> >::const_iterator links = _links.find(*n);
            if (links == _links.end()) continue;
            for (std::map<int, LinkType>::const_iterator l = links->second.begin(); l != links->second.end(); ++l) {
                if (found.count(l->first)) continue;
                if (l->second == kNeighbor) nextLevel.insert(l->first);
                else if (viaClosure.insert(l->first).second) level.push_back(l->first);
            }
        }
    }
    return found;
}

int MemoryHip::addSignature(const std::vector<int>& wordIds, int id) {
    _likeSig = 0;
    if (id == 0) id = ++_idCount;
    if (_signatures.count(id)) return 0;
    for (size_t k = 0; k < wordIds.size(); ++k) if (wordIds[k] > 0) _vwd->addWordRef(wordIds[k], id);
    _signatures[id] = wordIds;
    if (id > _idCount) _idCount = id;
    _workingMem.insert(id);                     // Memory::loadDataFromDb: loaded signatures enter the working memory (:447-480)
    return id;
}

int MemoryHip::loadDataFromDb(const std::string& path, bool lastStateOnly) {
    DbLoaderHip db;
    DbDictionary dict;
    DbSignatures sigs;
    _loadError.clear();
    if (!db.open(path) || !db.loadSignatureWords(sigs, lastStateOnly) || !db.loadDictionary(dict, sigs.sigIds.empty() && _vwd->isIncremental())) {
        _loadError = db.lastError();
        return -1;
    }
    // which words to keep: an incremental dictionary only what the loaded signatures reference (Memory.cpp:394-424)
    std::set<int> referenced;
    if (_vwd->isIncremental() && !sigs.sigIds.empty())
        for (size_t k = 0; k < sigs.wordIds.size(); ++k) if (sigs.wordIds[k] > 0) referenced.insert(sigs.wordIds[k]);
    const bool filter = _vwd->isIncremental() && !sigs.sigIds.empty();
    const size_t rowBytes = (size_t)dict.cols * (dict.type == MAT_32F ? 4 : 1);
    // every check that can fail comes BEFORE the first change of state: a refused load leaves the memory as it was
    {
        std::set<int> have(dict.wordIds.begin(), dict.wordIds.end()), nodes;
        const std::map<int, VisualWord*>& old = _vwd->getVisualWords();
        for (size_t s = 0; s < sigs.sigIds.size(); ++s) {
            if (_signatures.count(sigs.sigIds[s]) || !nodes.insert(sigs.sigIds[s]).second) {
                _loadError = "node " + std::to_string(sigs.sigIds[s]) + " is in memory already";
                return -1;
            }
            for (int64_t k = sigs.offsets[s]; k < sigs.offsets[s + 1]; ++k) {
                const int w = sigs.wordIds[(size_t)k];
                if (w > 0 && !have.count(w) && !old.count(w)) {
                    _loadError = "The dictionary is empty or missing some words from nodes in WM (word " + std::to_string(w) + " of node " +
                                 std::to_string(sigs.sigIds[s]) + ")";
                    fprintf(stderr, "[ERROR] %s\n", _loadError.c_str());
                    return -1;
                }
            }
        }
    }
    for (size_t k = 0; k < dict.wordIds.size(); ++k) {
        if (filter && !referenced.count(dict.wordIds[k])) continue;
        VisualWord* vw = new VisualWord(dict.wordIds[k], Mat(1, dict.cols, dict.type, dict.rows.data() + k * rowBytes));
        vw->setSaved(true);
        _vwd->addWord(vw);
    }
    if (!dict.wordIds.empty() || dict.lastWordId > 0) _vwd->setLastWordId(dict.lastWordId);   // DBDriverSqlite3::loadQuery :3617-3619: fixed dictionaries too
    _vwd->update();
    if (_vwd->getVisualWords().size() && !_vwd->isAvailable()) { _loadError = _vwd->lastError(); return -1; }
    int loaded = 0;
    for (size_t s = 0; s < sigs.sigIds.size(); ++s) {
        const std::vector<int> words(sigs.wordIds.begin() + sigs.offsets[s], sigs.wordIds.begin() + sigs.offsets[s + 1]);
        for (size_t k = 0; k < words.size(); ++k)
            if (words[k] > 0 && !_vwd->getWord(words[k])) {
                _loadError = "The dictionary is empty or missing some words from nodes in WM (word " + std::to_string(words[k]) + " of node " +
                             std::to_string(sigs.sigIds[s]) + ")";
                fprintf(stderr, "[ERROR] %s\n", _loadError.c_str());
                return -1;
            }
        if (this->addSignature(words, sigs.sigIds[s]) != sigs.sigIds[s]) { _loadError = "node " + std::to_string(sigs.sigIds[s]) + " is in memory already"; return -1; }
        loaded += 1;
    }
    if (!_vwd->flushReferencesBulk([this](int id) { return this->getNi(id); })) { _loadError = _vwd->lastError(); return -1; }
    return loaded;
}

int MemoryHip::getNi(int signatureId) const {   // Memory.cpp:4955-4968
    std::map<int, std::vector<int> >::const_iterator it = _signatures.find(signatureId);
    if (it != _signatures.end()) return (int)it->second.size();
    std::map<int, int>::const_iterator d = _dbNi.find(signatureId);
    return d == _dbNi.end() ? 0 : d->second;
}

void MemoryHip::forget(int signatureId) {
    std::map<int, std::vector<int> >::iterator it = _signatures.find(signatureId);
    if (it == _signatures.end()) return;
    Stage st(_vwd, "Memory::forget");
    struct Put { std::map<std::string, float>& m; Stage& s; ~Put() { m["Timing/Forgetting/ms"] = s.ms(); } } put{_stats, st};
    _likeSig = 0;                               // N and the references change: the frame's likelihood is no longer Memory::computeLikelihood's
    std::set<int> keys(it->second.begin(), it->second.end());   // uUniqueKeys (Memory.cpp:6885)
    _vwd->removeAllWordRefs(keys, signatureId);
    _dbNi[signatureId] = (int)it->second.size();
    _signatures.erase(it);
    _globals.erase(signatureId);                // (its device rows stay behind in a retired slot, which scores 0)
    _globalsDirty.erase(signatureId);
    _stMem.erase(signatureId);                  // the links stay (they are in the database): getNeighborsId stops at the missing node
    _workingMem.erase(signatureId);
}

std::vector<int> MemoryHip::signatureIds() const {
    std::vector<int> v;
    for (std::map<int, std::vector<int> >::const_iterator i = _signatures.begin(); i != _signatures.end(); ++i) v.push_back(i->first);
    return v;
}

std::map<int, float> MemoryHip::computeLikelihood(const std::list<int>& wordIds, const std::list<int>& ids) {
    Stage st(_vwd, "Memory::computeLikelihood");
    if (!_tfIdfLikelihoodUsed) {                 // Memory.cpp:2179-2214 (no signature, no global descriptors: the words branch)
        std::map<int, float> S = this->similarityOf(0, wordIds, ids);
        _stats["Timing/Likelihood_computation/ms"] = st.ms();
        return S;
    }
    const float N = (float)_signatures.size();   // Memory.cpp:2248: every signature in memory, not only `ids`
    std::map<int, float> L = _vwd->computeLikelihood(wordIds, ids, N, [this](int s) { return this->getNi(s); });
    _stats["Timing/Likelihood_computation/ms"] = st.ms();
    return L;
}

float MemoryHip::compareTo(int sigA, int sigB) {
    std::map<int, std::vector<int> >::const_iterator it = _signatures.find(sigA);
    if (it == _signatures.end() || sigB <= 0 || !_signatures.count(sigB)) return 0.0f;
    Stage st(_vwd, "Signature::compareTo");
    const std::map<int, float> S = this->similarityOf(sigA, std::list<int>(it->second.begin(), it->second.end()), std::list<int>(1, sigB));
    return S.empty() ? 0.0f : S.begin()->second;
}

// ---- global descriptors
bool MemoryHip::setGlobalDescriptors(int signatureId, const std::vector<GlobalDescriptor>& descriptors) {
    if (!_signatures.count(signatureId) || descriptors.size() > (size_t)LCD_GLOBAL_MAX_CHANNELS) return false;
    for (size_t c = 0; c < descriptors.size(); ++c) if (descriptors[c].data.size() > (size_t)LCD_GLOBAL_MAX_DIM) return false;
    _globals[signatureId] = descriptors;
    _globalsDirty.insert(signatureId);
    return true;
}

void MemoryHip::clearGlobalDescriptors(int signatureId) {
    if (_globals.erase(signatureId)) _globalsDirty.insert(signatureId);
}

const std::vector<MemoryHip::GlobalDescriptor>& MemoryHip::globalDescriptors(int signatureId) const {
    static const std::vector<GlobalDescriptor> none;
    std::map<int, std::vector<GlobalDescriptor> >::const_iterator it = _globals.find(signatureId);
    return it == _globals.end() ? none : it->second;
}

static std::vector<lcd_global_desc> asLcd(const std::vector<MemoryHip::GlobalDescriptor>& g) {
    std::vector<lcd_global_desc> d(g.size());
    for (size_t c = 0; c < g.size(); ++c) {
        d[c].type = g[c].data.empty() ? 0 : g[c].type;          // (an empty cv::Mat cannot be compared: absent)
        d[c].dim = (int32_t)g[c].data.size();
        d[c].data = g[c].data.empty() ? 0 : g[c].data.data();
    }
    return d;
}

bool MemoryHip::flushGlobals() {
    if (_globals.empty() && _globalsDirty.empty()) return this->flushReferences();
    // a signature whose references changed gets a new slot from flushReferences: its rows follow it there
    const std::set<int>& moved = _vwd->dirtySignatures();
    for (std::set<int>::const_iterator s = moved.begin(); s != moved.end(); ++s) if (_globals.count(*s)) _globalsDirty.insert(*s);
    if (!this->flushReferences()) return false;
    for (std::set<int>::iterator s = _globalsDirty.begin(); s != _globalsDirty.end();) {
        if (!_vwd->isOnDevice(*s)) { if (_globals.count(*s)) ++s; else s = _globalsDirty.erase(s); continue; }   // no slot yet: later
        std::map<int, std::vector<GlobalDescriptor> >::const_iterator g = _globals.find(*s);
        const std::vector<lcd_global_desc> d = g == _globals.end() ? std::vector<lcd_global_desc>() : asLcd(g->second);
        const int rc = d.empty() ? lcd_sig_clear_globals(_vwd->engine(), *s) : lcd_sig_set_globals(_vwd->engine(), *s, d.data(), (int)d.size());
        if (rc != LCD_OK) { fprintf(stderr, "[ERROR] global descriptors of signature %d: %s\n", *s, lcd_last_error(_vwd->engine())); return false; }
        s = _globalsDirty.erase(s);
    }
    return true;
}

// this->compareTo(s) of the query (signature querySig's descriptors, if it is in memory and has any) against every id of `ids`
std::map<int, float> MemoryHip::similarityOf(int querySig, const std::list<int>& wordIds, const std::list<int>& ids) {
    std::vector<lcd_global_desc> d;
    std::map<int, std::vector<GlobalDescriptor> >::const_iterator g = _globals.find(querySig);
    if (g != _globals.end()) d = asLcd(g->second);
    if (_vwd->engine() && !ids.empty() && !this->flushGlobals()) {
        std::map<int, float> zeros;
        for (std::list<int>::const_iterator i = ids.begin(); i != ids.end(); ++i) zeros[*i] = 0.0f;
        return zeros;
    }
    return _vwd->computeSimilarity(wordIds, ids, [this](int s) { return this->getNi(s); }, d.empty() ? 0 : d.data(), (int)d.size());
}

// (signature id, likelihood) of every signature registered on the device, ascending id, from the frame's slot-indexed result
const std::vector<std::pair<int, float> >& MemoryHip::sortedLikelihood() {
    if (_likeSortedValid) return _likeSorted;
    const std::vector<int>& slotSig = _vwd->slotSignatures();
    _likeSorted.clear();
    const size_t n = std::min(slotSig.size(), _likeSlots.size());
    _likeSorted.reserve(n);
    bool ascending = true;
    for (size_t s = 0; s < n; ++s) {
        if (slotSig[s] == 0) continue;
        if (!_likeSorted.empty() && slotSig[s] < _likeSorted.back().first) ascending = false;
        _likeSorted.push_back(std::pair<int, float>(slotSig[s], _likeSlots[s]));
    }
    if (!ascending) std::sort(_likeSorted.begin(), _likeSorted.end());   // (re-registered signatures sit in later slots)
    _likeSortedValid = true;
    return _likeSorted;
}

static float lookupSorted(const std::vector<std::pair<int, float> >& v, size_t& cursor, int id) {
    // ids usually arrive ascending (Rtabmap builds the list from a std::map): a cursor that only moves forward; else a binary search
    if (cursor < v.size() && v[cursor].first <= id) {
        while (cursor < v.size() && v[cursor].first < id) ++cursor;
        return cursor < v.size() && v[cursor].first == id ? v[cursor].second : 0.0f;
    }
    std::vector<std::pair<int, float> >::const_iterator it = std::lower_bound(v.begin(), v.end(), std::pair<int, float>(id, -1e30f));
    cursor = (size_t)(it - v.begin());
    return it != v.end() && it->first == id ? it->second : 0.0f;
}

std::map<int, float> MemoryHip::computeLikelihood(int signatureId, const std::list<int>& ids) {
    std::map<int, std::vector<int> >::const_iterator it = _signatures.find(signatureId);
    if (it == _signatures.end()) return std::map<int, float>();   // "The signature is null" (Memory.cpp:2222)
    if (_likeSig != 0 && _likeSig == signatureId) {
        Stage st(_vwd, "Memory::computeLikelihood");
        struct Put { std::map<std::string, float>& m; Stage& s; ~Put() { m["Timing/Likelihood_computation/ms"] = s.ms(); } } put{_stats, st};
        std::map<int, float> likelihood;
        if (ids.empty()) { fprintf(stderr, "[WARN] ids list is empty\n"); return likelihood; }   // :2227-2231
        const std::vector<std::pair<int, float> >& v = sortedLikelihood();
        size_t cursor = 0;
        bool sorted = true; int last = 0; bool first = true;
        for (std::list<int>::const_iterator i = ids.begin(); i != ids.end(); ++i) { if (!first && *i <= last) { sorted = false; break; } last = *i; first = false; }
        if (sorted) for (std::list<int>::const_iterator i = ids.begin(); i != ids.end(); ++i) likelihood.insert(likelihood.end(), std::pair<int, float>(*i, lookupSorted(v, cursor, *i)));
        else for (std::list<int>::const_iterator i = ids.begin(); i != ids.end(); ++i) likelihood[*i] = lookupSorted(v, cursor, *i);
        return likelihood;
    }
    if (!_tfIdfLikelihoodUsed) {                 // Memory.cpp:2179-2214: sim = signature->compareTo(*sB)
        Stage st(_vwd, "Memory::computeLikelihood");
        std::map<int, float> S = this->similarityOf(signatureId, std::list<int>(it->second.begin(), it->second.end()), ids);
        _stats["Timing/Likelihood_computation/ms"] = st.ms();
        return S;
    }
    return computeLikelihood(std::list<int>(it->second.begin(), it->second.end()), ids);
}

void MemoryHip::computeLikelihood(int signatureId, const std::list<int>& ids, std::map<int, float>& likelihood) {
    if (_likeSig == 0 || _likeSig != signatureId || !_signatures.count(signatureId) || ids.empty()) { likelihood = this->computeLikelihood(signatureId, ids); return; }
    Stage st(_vwd, "Memory::computeLikelihood");
    struct Put { std::map<std::string, float>& m; Stage& s; ~Put() { m["Timing/Likelihood_computation/ms"] = s.ms(); } } put{_stats, st};
    const std::vector<std::pair<int, float> >& v = sortedLikelihood();
    size_t cursor = 0;
    std::map<int, float>::iterator m = likelihood.begin();
    int last = 0; bool first = true;
    for (std::list<int>::const_iterator i = ids.begin(); i != ids.end(); ++i) {
        if (!first && *i <= last) { likelihood = this->computeLikelihood(signatureId, ids); return; }   // unsorted ids: the plain way
        last = *i; first = false;
        while (m != likelihood.end() && m->first < *i) m = likelihood.erase(m);
        const float val = lookupSorted(v, cursor, *i);
        if (m != likelihood.end() && m->first == *i) { m->second = val; ++m; }
        else m = ++likelihood.insert(m, std::pair<int, float>(*i, val));
    }
    likelihood.erase(m, likelihood.end());
}

bool MemoryHip::computeLikelihoodFlat(int signatureId, std::vector<int>& sigIds, std::vector<float>& values) {
    if (_likeSig == 0 || _likeSig != signatureId) return false;
    if (!_likeSortedValid) {
        // the usual case -- signatures registered in ascending id, so the device's slot order IS ascending id -- in ONE pass over the slots, without
        // the (id, value) pairs the map overloads look things up in: 100 000 slots are 1.2 MB read and 0.8 MB written
        Stage st(_vwd, "Memory::computeLikelihood");
        const std::vector<int>& slotSig = _vwd->slotSignatures();
        const size_t n = std::min(slotSig.size(), _likeSlots.size());
        sigIds.resize(n);
        values.resize(n);
        size_t m = 0;
        int last = 0;
        bool ascending = true;
        for (size_t k = 0; k < n; ++k) {
            const int id = slotSig[k];
            if (id == 0) continue;
            if (id < last) { ascending = false; break; }
            last = id;
            sigIds[m] = id; values[m] = _likeSlots[k];
            ++m;
        }
        if (ascending) {
            sigIds.resize(m);
            values.resize(m);
            _stats["Timing/Likelihood_computation/ms"] = st.ms();
            return true;
        }
    }
    const std::vector<std::pair<int, float> >& v = sortedLikelihood();
    sigIds.resize(v.size());
    values.resize(v.size());
    for (size_t k = 0; k < v.size(); ++k) { sigIds[k] = v[k].first; values[k] = v[k].second; }
    return true;
}

}  // namespace rtabmap_amd
