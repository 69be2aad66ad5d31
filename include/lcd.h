/* lcd.h -- C-ABI of the MI355X-native loop-closure detection engine (liblcd_hip.so).
 *
 * This is the drop-in boundary for ONE hot path of introlab/rtabmap (reference v0.23.8, paths below are relative to
 * /root/reference): descriptor -> visual-word quantisation (VWDictionary) + TF-IDF likelihood
 * (Memory::computeLikelihood).  Every entry point is `extern "C"`, takes plain pointers and sizes, returns an int
 * status (LCD_OK == 0) and never throws or aborts across the boundary (the reference's own convention is
 * "UERROR + return empty", VWDictionary.cpp:920-930, 948-957).  Pointers are caller-owned; host buffers are copied
 * before the call returns.  A handle is single-owner and not re-entrant (VWDictionary has no locks either; its
 * calls come from the Rtabmap thread and, for update(), from PreUpdateThread joined before use, Memory.cpp:5284,5926);
 * calls may come from different threads at different times -- every entry selects the engine's device itself.
 *
 * Numeric contract (identical to the reference): distances are SQUARED L2 for float descriptors (rtflann L2 functor,
 * dist.h:150-177, and cv::NORM_L2SQR) accumulated in the reference's own order -> bit-exact; Hamming distances as
 * float (VWDictionary.cpp:1078-1083) over EVERY byte of the descriptor (cv::NORM_HAMMING, the metric of the brute-force
 * strategies this engine stands in for; rtflann::Hamming, used by the FLANN strategies, ignores the size % 8 trailing
 * bytes, dist.h:555-579 -- the two only differ for sizes that are not a multiple of 8); on equal distance the lower vocabulary row wins (result_set.h:151-171); word
 * ids >= 1, 0 == none (ID_INVALID, VWDictionary.cpp:59-60); signature ids are any non-zero int (virtual place -1).
 *
 * There is NO CPU fallback inside this library: without a gfx950 device lcd_create() fails with LCD_ERR_HIP.
 */
#ifndef LCD_H_
#define LCD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LCD_ABI_VERSION 7

typedef struct lcd_engine lcd_engine;

enum lcd_status {
    LCD_OK = 0,
    LCD_ERR_INVALID = 1,      /* bad argument (size/type mismatch: the reference logs UERROR and returns empty) */
    LCD_ERR_HIP = 2,          /* HIP runtime / launch failure, or no gfx950 device */
    LCD_ERR_NOMEM = 3,
    LCD_ERR_STATE = 4,        /* call not valid in the current state (e.g. unknown word / signature) */
    LCD_ERR_UNSUPPORTED = 5
};

enum lcd_dtype {
    LCD_F32 = 0,              /* CV_32F rows, squared-L2 metric (SURF/SIFT...) */
    LCD_U8 = 1                /* CV_8U rows, Hamming metric (ORB/BRIEF...)      */
};

/* flags of lcd_quantize / lcd_find_nn (VWDictionary parameters, Parameters.h:243-266) */
enum lcd_quantize_flags {
    LCD_Q_INCREMENTAL = 1,              /* Kp/IncrementalDictionary: NNDR decides between "existing word" and "new word" */
    LCD_Q_NEW_WORDS_COMPARED = 2        /* Kp/NewWordsComparedTogether: also match words created earlier in the same call */
};

/* how the 2-NN is computed.  Every mode returns the SAME bits (the reference's distances and tie-break).
 * Squared L2 of 64-float descriptors: the matrix-core modes only rank candidates, an exact re-rank in the reference's arithmetic plus a
 * completeness certificate (exact redo when it fails) produces the result.
 * Squared L2 of 128- and 256-float descriptors (SIFT, extended SURF, SuperPoint): a handle whose config WRITES LCD_KNN_BF16X3 or LCD_KNN_F16
 * searches its main vocabulary (256 rows or more) with a stateless matrix-core filter of that arithmetic (knn_wide_filter_kernel: it reads the
 * fp32 rows and converts them on the way, the handle keeps no operand or norm table for them), the same exact re-rank with the certificate and
 * the same exact redo.  LCD_KNN_DEFAULT -- and LCD_KNN_EXACT_VALU, LCD_KNN_F32_MFMA, LCD_KNN_HAMMING_MFMA -- stay the exact scan on such a
 * handle: the two arms have NOT yet been measured against the scan at vocabulary sizes (49 000 rows and more) -- profiles/wide_mfma_scan.txt holds
 * the commands, the compiler's resource lines and what little was timed, DESIGN.md 4e the design -- so no speed-up is claimed, and a later change
 * decides whether the default moves.  A search whose launch plan cannot be made (candidate records beyond 2^31 - 1 bytes: about 200 000 shares
 * of 1 024 rows x 512 queries; more than 65 535 query blocks) silently uses the exact scan, same bits; lcd_profile_read names the kernel that ran.
 * Float rows of any other length use the exact scan.
 * Hamming (LCD_U8 handles): the exact vector-ALU scan unless the handle asks for LCD_KNN_HAMMING_MFMA, which computes the same integer
 * distances on the i8 matrix cores (an integer dot product: no filter, no re-rank); the float modes mean LCD_KNN_DEFAULT there. */
enum lcd_knn_mode {
    LCD_KNN_DEFAULT = 0,       /* = LCD_KNN_BF16X3 where it applies */
    LCD_KNN_EXACT_VALU = 1,    /* exact vector-ALU scan only */
    LCD_KNN_F32_MFMA = 2,      /* fp32 matrix-core filter (v_mfma_f32_32x32x2_f32) + exact re-rank */
    LCD_KNN_BF16X3 = 3,        /* bf16 matrix-core filter, three bf16 products per fp32 product + exact re-rank */
    LCD_KNN_F16 = 4,           /* fp16 matrix-core filter, ONE product per fp32 product (operands rounded to IEEE half: a third of the
                                  matrix work, an error bound of ~2^-10 (|q|^2 + |v|^2) instead of ~2^-14) + exact re-rank.  Made for
                                  unit-scale descriptors (SURF/SIFT are L2-normalised); queries whose certificate the wider bound
                                  cannot give -- and descriptors beyond half's range -- go to the exact scan, so the results stay the
                                  same bits; a vocabulary of near-duplicate words makes that the common case and this mode the slower one */
    LCD_KNN_HAMMING_MFMA = 5   /* LCD_U8 handles, any row length: the Hamming 2-NN of the main vocabulary (256 rows or more) on the matrix cores
                                  (v_mfma_i32_32x32x32_i8 over bits written as +-127 bytes), exact by construction.  Opt-in: LCD_KNN_DEFAULT on
                                  a u8 handle stays the vector-ALU scan.  On an LCD_F32 handle it means LCD_KNN_DEFAULT */
};

typedef struct lcd_config {
    int32_t struct_size;       /* sizeof(lcd_config), for ABI evolution */
    int32_t device;            /* HIP device ordinal */
    int32_t dtype;             /* lcd_dtype */
    int32_t dim;               /* columns: floats (LCD_F32) or bytes (LCD_U8) per descriptor.  LCD_U8 rows whose dim is no multiple of 4
                                  (AKAZE: 61) are stored zero-padded on the device: every entry point that takes HOST rows serves such a
                                  handle, the ones that take a DEVICE descriptor pointer (lcd_frame_dev, lcd_knn2_dev, lcd_shard_knn2_dev,
                                  lcd_shard_frame_dev) and lcd_frame_host return LCD_ERR_UNSUPPORTED -- a [q x dim] buffer is not what the
                                  kernels walk; use lcd_quantize / lcd_knn2 */
    int64_t vocab_capacity;    /* initial row capacity (grows on demand) */
    int64_t sig_capacity;      /* initial signature-slot capacity (grows on demand) */
    int32_t max_queries;       /* initial per-call query capacity (Kp/MaxFeatures; grows on demand) */
    int32_t knn_mode;          /* lcd_knn_mode, per handle */
    void*   stream;            /* optional hipStream_t to enqueue on; NULL = engine-owned stream */
    int32_t pipeline;          /* 1: consecutive lcd_frame_dev calls are software-pipelined (matrix-core 2-NN handles), lcd_pipeline_depth() = 3
                                  frames deep: the call for frame t only converts its descriptors into matrix-core operands; its launches
                                  carry the distance filter + re-rank of frame t - 1, the decision loop of frame t - 2 and the registration +
                                  scoring of frame t - 3, whose single-workgroup latency chains hide behind the filter.  Consequence for the
                                  caller: the outputs of a frame (d_word_ids, d_likelihood, d_bayes, ...) are written -- and its
                                  descriptors read -- by work that the NEXT THREE lcd_frame_dev calls enqueue (or any other call on the
                                  handle, which completes the owed stages first; lcd_synchronize to wait for them): keep
                                  lcd_pipeline_depth() + 1 sets of buffers and rotate.  lcd_sig_remove, lcd_record_event and
                                  lcd_bayes_set_neighbors are queued behind the owed stages of the frame they follow, so they keep their
                                  place in the call order.  Results are identical with and without.  The one exception to "any other
                                  call completes the owed stages": lcd_match_pairs / lcd_match_pairs_dev, lcd_match_guided / lcd_match_guided_dev and
                                  lcd_select_features / lcd_expand_word_ids / lcd_keypoints_3d / lcd_keypoints_3d_stereo / lcd_track_flow / lcd_estimate_motion_3d / lcd_estimate_motion_pnp / lcd_estimate_motion_mono / lcd_refine_motion_ba / lcd_register_icp / lcd_register_icp_plane / lcd_filter_scans with their _dev forms
                                  touch no engine state and complete nothing -- they are enqueued on the engine stream where the call lands, with scratch of their own. */
    int32_t reserved1;
} lcd_config;

/* ---------------------------------------------------------------------------------------------------------------
 * life cycle.  Replaces `new VWDictionary(parameters)` (Memory.cpp:144) for the device-side state. */
int  lcd_abi_version(void);
int  lcd_create(const lcd_config* cfg, lcd_engine** out);
void lcd_destroy(lcd_engine* h);
/* text of the last error on this handle ("" if none); valid until the next call on the handle */
const char* lcd_last_error(const lcd_engine* h);
/* block until all work enqueued by this handle has finished */
int  lcd_synchronize(lcd_engine* h);
/* 0 for a plain handle; for a pipelined one (lcd_config.pipeline) the number of later lcd_frame_dev calls that still enqueue work of a
 * frame: its outputs are complete (enqueued) once that many further frames have been submitted, or after any other call */
int  lcd_pipeline_depth(const lcd_engine* h);

/* ---------------------------------------------------------------------------------------------------------------
 * vocabulary == VWDictionary::_dataTree + _mapIndexId (VWDictionary.h:146-149), maintained by update() :475-701.
 * Rows live in HBM; the row ORDER is part of the contract because it is the distance tie-break. */

/* VWDictionary::clear() :843-873 / the reset at the top of the rebuild branch :612-615 */
int lcd_vocab_clear(lcd_engine* h);
/* brute-force append branch :571-609: rows appended in the given order; word_ids[i] > 0, not already present */
int lcd_vocab_append(lcd_engine* h, const void* rows, int n, const int32_t* word_ids);
/* VWDictionary::removeWords (:1595-1607, _removedIndexedWords): rows are tombstoned at once (never returned by a search) and
 * the words cease to exist.  As in the reference, only words without references are removed (its callers pass getUnusedWords(),
 * Memory.cpp:2867,6906); the postings key of a removed word is recycled once the device has confirmed that. */
int lcd_vocab_remove(lcd_engine* h, const int32_t* word_ids, int n);
/* Memory::cleanUnusedWords (Memory.cpp:6899-6920: removeWords(getUnusedWords()), run by preUpdate before every frame of an incremental
 * dictionary) from the DEVICE's reference counts: every vocabulary row whose word no signature references is removed as by
 * lcd_vocab_remove.  For callers that keep no host copy of the references (device-resident frame streams).  out_word_ids (may be NULL
 * with capacity 0) receives up to `capacity` of the removed ids in ascending row order, *out_n their number.  Synchronises. */
int lcd_vocab_remove_unused(lcd_engine* h, int32_t* out_word_ids, int capacity, int32_t* out_n);
/* The same cleanUnusedWords WITHOUT completing or synchronising anything: one kernel, enqueued behind the work the handle has taken on so
 * far, tombstones every row whose word no signature references (row id 0, |row|^2 = +inf: no search finds it any more) and logs it on the
 * device; the host's mirror of the rows and the postings keys of the removed words catch up the next time the handle is drained (any call
 * that completes the owed stages: lcd_vocab_count, lcd_vocab_rebuild, lcd_synchronize ...).  On a pipelined handle with frames in flight
 * the clean takes its place behind the newest frame -- its registration and the lcd_sig_remove calls made since, like those calls
 * themselves -- so it is what Memory::preUpdate (Memory.cpp:1004-1010) runs in front of the NEXT frame's update(); the frames already in
 * flight behind it (up to lcd_pipeline_depth()) took their snapshot of the vocabulary earlier: a word they still matched keeps the
 * references of their signatures (its key is recycled once those are gone) but is never matched again.  A caller that needs the
 * reference's order exactly calls lcd_vocab_remove_unused (or drains) instead. */
int lcd_vocab_remove_unused_async(lcd_engine* h);
/* full-rebuild branch :610-690: drop tombstones and reorder the live rows by ascending word id, on the device */
int lcd_vocab_rebuild(lcd_engine* h);
/* rows = rows in the matrix incl. tombstones, live = searchable rows */
int lcd_vocab_count(const lcd_engine* h, int64_t* rows, int64_t* live);
/* read back rows [first, first+n) and their word ids (0 = tombstone); either output may be NULL */
int lcd_vocab_read(lcd_engine* h, int64_t first, int n, void* out_rows, int32_t* out_word_ids);

/* ---------------------------------------------------------------------------------------------------------------
 * exact 2-NN == FlannIndex::knnSearch(k=2) (FlannIndex.cpp:701, linear index) == cv::BFMatcher::knnMatch(k=2)
 * (VWDictionary.cpp:1027-1028) == the cv::cuda brute-force matcher (:1053-1066, which re-uploads the vocabulary per
 * call; here it stays resident).  out_word_ids/out_dist are [q*2]; a missing neighbour is (0, -1.0f). */
int lcd_knn2(lcd_engine* h, const void* queries, int q, int32_t* out_word_ids, float* out_dist);

/* q x q distance matrix of a descriptor block against itself (same metric/arithmetics as lcd_knn2).
 * The reference computes these distances one cv::BFMatcher call per descriptor (VWDictionary.cpp:1140-1160). */
int lcd_selfdist(lcd_engine* h, const void* queries, int q, float* out_qxq);

/* VWDictionary::addNewWords search + decision loop (:1015-1219) without the bookkeeping:
 *   for each descriptor i (in order): candidates = indexed 2-NN (only if the vocabulary has >= 2 live rows, :1015)
 *   + [LCD_Q_NEW_WORDS_COMPARED] exact 2-NN among the descriptors j < i that became new words in this call (:1140);
 *   [LCD_Q_INCREMENTAL] new word iff fewer than 2 candidates or d1 > nndr_ratio * d2 (:1162-1183), else word = nearest;
 *   fixed dictionary: nearest word, or "no entry" when there is no candidate (:1211-1218).
 * out_word_ids[i] > 0  : existing word id (caller does addWordRef)
 * out_word_ids[i] < 0  : the (-out-1)-th new word of this call (caller assigns ++_lastWordId in that order, :1185)
 * out_word_ids[i] == 0 : fixed dictionary and no candidate (the reference emits no list entry)
 * out_n_new (may be NULL) receives the number of new words. */
int lcd_quantize(lcd_engine* h, const void* descriptors, int q, int flags, float nndr_ratio,
                 int32_t* out_word_ids, int32_t* out_n_new);

/* VWDictionary::findNN(cv::Mat) (:1273-1552): indexed 2-NN + exact 2-NN (1-NN if one row) over the caller's
 * not-yet-indexed words (`extra_rows` x dim with ids `extra_word_ids`, ascending id like _notIndexedWords; may be
 * NULL/0) + NNDR (LCD_Q_INCREMENTAL) -> out_word_ids[i] = matched word id or 0.  Read-only. */
int lcd_find_nn(lcd_engine* h, const void* queries, int q, const void* extra_rows, const int32_t* extra_word_ids,
                int n_extra, int flags, float nndr_ratio, int32_t* out_word_ids);

/* ---------------------------------------------------------------------------------------------------------------
 * inverted index == VisualWord::_references of every word (VisualWord.h:62) + Memory::getNi (Memory.cpp:4955).
 * The engine is signature-granular: a signature's word list is registered once and retired once. */

/* one signature's references: word_ids[n] in keypoint order, duplicates = occurrences (== n x addWordRef :880 for
 * ids > 0; ids <= 0 are features without a word: they only count in ni).  ni = Signature::getWords().size()
 * (Memory.cpp:4961), normally n.  The signature must not be registered already.  At most 8192 entries (n > 8192:
 * LCD_ERR_UNSUPPORTED, nothing registered, the handle stays usable; the same limit per signature for lcd_sig_add_bulk). */
int lcd_sig_add(lcd_engine* h, int32_t sig_id, const int32_t* word_ids, int n, int32_t ni);
/* Memory::disableWordsRef (:6877-6897) == removeAllWordRef(word, sig) for every word of the signature */
int lcd_sig_remove(lcd_engine* h, int32_t sig_id);
/* bulk registration (Memory::loadDataFromDb replay, Memory.cpp:447-480): sig_offsets[n_sigs+1] index word_ids.  One
 * registration launch for the whole call and a fixed number of launches per 64 full buckets (16 384 signatures) sealed. */
int lcd_sig_add_bulk(lcd_engine* h, int n_sigs, const int32_t* sig_ids, const int64_t* sig_offsets,
                     const int32_t* word_ids, const int32_t* ni);
int lcd_sig_count(const lcd_engine* h, int64_t* live_signatures, int64_t* postings);
/* nw = VisualWord::getReferences().size() of a word (0 if unknown) */
int lcd_word_nrefs(lcd_engine* h, int32_t word_id, int32_t* out_nw);

/* Memory::computeLikelihood(signature, ids), TF-IDF branch (Memory.cpp:2215-2291):
 *   out[k] = sum over unique word ids w > 0 of the query of  (nwi(w, sig_ids[k]) * log10(N / nw(w))) / ni(sig_ids[k])
 * query_word_ids[nq]: the query signature's words (any order, duplicates allowed, ids <= 0 ignored);
 * sig_ids[n_ids]: the signatures to score (unknown / retired ids and the virtual place score 0);
 * N = (float)Memory::getSignatures().size() as the caller counts it (:2248).  out[n_ids] pairs with sig_ids.
 * At most 8192 query entries (nq > 8192: LCD_ERR_UNSUPPORTED, the handle stays usable). */
int lcd_likelihood(lcd_engine* h, const int32_t* query_word_ids, int nq, const int32_t* sig_ids, int n_ids,
                   float N, float* out);

/* Signature::compareTo, words branch (Signature.cpp:273-286), for Memory::computeLikelihood with Kp/TfIdfLikelihoodUsed=false
 * (Memory.cpp:2179-2214) and Memory::rehearsal (:4245):
 *   pairs  = sum over word ids w > 0 of min(occurrences of w in the query, occurrences of w in the signature)
 *            (EpipolarGeometry::findPairs on the two multimaps pairs the k-th occurrence with the k-th, EpipolarGeometry.h:123-151)
 *   out[k] = float(pairs) / float(max(vq, vs)),  vq / vs = entries with id > 0 of the query / of signature sig_ids[k]
 *            (words.size() - invalidWordsCount); 0 when either is 0 (isBadSignature, Signature.cpp:277).
 * Integers up to one IEEE float division: bit-exact against the reference, whatever the index layout.  vq counts every id > 0 of the
 * query, also ids the index has never seen (valid words that pair with nothing).  Nothing is weighted or masked by idf.
 * out[k] pairs with sig_ids[k]; unknown / retired ids and ids <= 0 give 0 (the reference's "*iter > 0" test).  out_pairs / out_valid
 * (may be NULL): the integers behind out[k], pairs and vs.  nq <= 8192 (more: LCD_ERR_UNSUPPORTED, the handle stays usable); n_ids == 0
 * returns LCD_OK, an empty index gives zeros.
 * One departure from the reference: ids <= 0 are "no word" on both sides (findPairs would admit a key 0, which RTAB-Map never
 * issues).  This entry compares signatures by their words alone; lcd_compare_to below adds compareTo's global-descriptor branch and is
 * the whole of Signature::compareTo.  Not available across sharded handles (the pairs would all-reduce, vs needs a second exchange) and
 * not fused into the pipelined launches: stand-alone launches on the engine stream. */
int lcd_similarity(lcd_engine* h, const int32_t* query_word_ids, int nq, const int32_t* sig_ids, int n_ids,
                   float* out, int32_t* out_pairs, int32_t* out_valid);
/* the same with the query's word ids in DEVICE memory and the dense result over signature slots (as d_likelihood of lcd_frame_dev;
 * retired slots 0); enqueued, not synchronised; completes what a pipelined handle owes first.  capacity = floats available at d_out
 * (smaller than the slots in use: LCD_ERR_INVALID). */
int lcd_similarity_dev(lcd_engine* h, const int32_t* d_query_word_ids, int nq, float* d_out, int64_t capacity);

/* ---- Signature::compareTo complete: the global-descriptor branch (Signature.cpp:257-272) in front of the words branch.
 * A signature may carry up to LCD_GLOBAL_MAX_CHANNELS global descriptors (SensorData::globalDescriptors(), what Mem/GlobalDescriptorStrategy
 * produces: GlobalDescriptor(type, 1 x dim CV_32F), e.g. a NetVLAD vector of 4096 floats).  A CHANNEL is the index in that vector.  For every
 * channel on which the query AND the signature hold a descriptor of type 1
 *     dotProd = (a . b + 1.0f) / 2.0f;  similarity += dotProd;  totalDescs += 1          (ascending channel index)
 * and, when totalDescs > 0, out = similarity / float(totalDescs); otherwise out is exactly what lcd_similarity returns.
 * Arithmetic -- defined by the ENGINE: cv::Mat::dot is OpenCV's and its float summation order is not part of the reference tree, so
 * there is nothing to be bit-exact against.  Products and sums are fp32 with fused multiply-add; the summation order of a . b is a
 * function of the channel's dim and of nothing else (not of the slot, the number of signatures, the launch or the entry point, and
 * a . b == b . a); the three statements above are the reference's, in its order.
 * Not reproduced: UASSERT(dotProd >= 0) -- rows that are not unit vectors are answered as computed, negative values included; the
 * UASSERT of equal globalDescriptors().size() -- a channel one side never set simply counts as "not type 1".
 * Storage: a channel's dim (1 .. LCD_GLOBAL_MAX_DIM) is fixed by the first type-1 row stored on it, for the life of the handle.  Nothing
 * is allocated before that row; then the channel holds one fp32 row per signature slot on the device (counted in
 * lcd_stats.bytes_device).  lcd_sig_remove leaves the row where it is: the retired signature scores 0 like every retired one.
 * Not available across sharded handles and not fused into the pipelined launches, as lcd_similarity. */
#define LCD_GLOBAL_MAX_CHANNELS 4
#define LCD_GLOBAL_MAX_DIM 16384
typedef struct lcd_global_desc {
    int32_t type;              /* GlobalDescriptor::type(); only 1 takes part, anything else is stored as "absent" (data may be NULL) */
    int32_t dim;               /* floats in data (1 x dim CV_32F) */
    const float* data;
} lcd_global_desc;
/* descs[i] is channel i of signature sig_id; the call REPLACES all of the signature's channels (channels >= n become absent).  data on
 * the HOST, copied before the call returns.  Errors, after each of which nothing was stored and the handle stays usable: unknown or retired
 * sig_id LCD_ERR_STATE; n > LCD_GLOBAL_MAX_CHANNELS or dim > LCD_GLOBAL_MAX_DIM LCD_ERR_UNSUPPORTED; on a type-1 entry dim <= 0, a dim
 * other than the channel's, or data == NULL LCD_ERR_INVALID.  Completes what a pipelined handle owes first, so the signature of a frame in
 * flight has its slot. */
int lcd_sig_set_globals(lcd_engine* h, int32_t sig_id, const lcd_global_desc* descs, int n);
/* the same with data in DEVICE memory (the extractor's output, left where it is); enqueued on the engine stream, not synchronised */
int lcd_sig_set_globals_dev(lcd_engine* h, int32_t sig_id, const lcd_global_desc* descs, int n);
/* one type-1 row for each of n_sigs signatures on ONE channel (a database replay); rows on the HOST, [n_sigs x dim]; the signatures' other
 * channels are left as they are.  A repeated sig id is LCD_ERR_INVALID; otherwise the errors of lcd_sig_set_globals. */
int lcd_sig_set_global_bulk(lcd_engine* h, int channel, int n_sigs, const int32_t* sig_ids, const float* rows, int dim);
/* SensorData::clearGlobalDescriptors() (Memory.cpp:3124): every channel of the signature becomes absent */
int lcd_sig_clear_globals(lcd_engine* h, int32_t sig_id);
/* this->compareTo(s) for the query (its word ids and its global descriptors, both on the HOST) against the signatures sig_ids[n_ids].
 * The query's descriptors obey the rules of lcd_sig_set_globals; a query channel on which the handle never stored a row matches nothing.
 * out[k] pairs with sig_ids[k]; ids <= 0, unknown and retired ids give 0.  out_n_global (may be NULL): totalDescs per id.  n_globals == 0
 * returns lcd_similarity's bits; n_ids == 0 returns LCD_OK. */
int lcd_compare_to(lcd_engine* h, const int32_t* query_word_ids, int nq, const lcd_global_desc* query_globals, int n_globals,
                   const int32_t* sig_ids, int n_ids, float* out, int32_t* out_n_global);
/* the same with the word ids and the descriptors' data in DEVICE memory and the dense result over the signature slots, as
 * lcd_similarity_dev: enqueued, not synchronised (query_globals itself, the array of structs, is host memory read during the call) */
int lcd_compare_to_dev(lcd_engine* h, const int32_t* d_query_word_ids, int nq, const lcd_global_desc* query_globals, int n_globals,
                       float* d_out, int64_t capacity);

/* ---- two-frame descriptor matching, stateless: the verification step behind the loop-closure hypothesis (RegistrationVis.cpp:1383-1504,
 * Rtabmap::process and every proximity candidate).  n_pairs frame pairs per call; the rows of all pairs are concatenated, pair p owns the
 * from-rows [from_offsets[p], from_offsets[p+1]) and the to-rows [to_offsets[p], to_offsets[p+1]).  The call needs no handle per pair and
 * reads and writes NOTHING of the handle's vocabulary, index, Bayes filter or word numbering ("next_word_id"); it only borrows the
 * handle's dtype, dim, device and stream.
 *
 * LCD_MATCH_DICTIONARY (Vis/CorNNType 0-4, :1482-1503: the temporary two-frame VWDictionary).  For each pair the outputs are exactly what
 *   1. lcd_quantize(from, flags, nndr_ratio) on an empty vocabulary, new words numbered 1, 2, ... in descriptor order (++_lastWordId from 0),
 *   2. lcd_vocab_append of those words in ascending id (update()),
 *   3. lcd_quantize(to, flags, nndr_ratio), its new words continuing the numbering,
 * return on a fresh handle of the same dtype and dim: the indexed search of step 3 takes part only if step 1 made at least 2 words
 * (VWDictionary.cpp:1015); with LCD_Q_NEW_WORDS_COMPARED from-rows match each other (out_from_word_ids repeats ids), without it every
 * from-row is a word; a pair without to-rows gives only the from ids, a pair without from-rows runs `to` against nothing.
 * from_word_ids != NULL (orignalWordsFromIds): step 1 is addWord(id, row) per from-row (:1488-1496, VWDictionary::addWord :1554) --
 * out_from_word_ids echoes the ids, the vocabulary rows are in ascending id (the distance tie-break), the to-frame's new words are numbered
 * from max(id) + 1.  The ids must be > 0 and distinct within a pair: lcd_match_pairs checks it (LCD_ERR_INVALID); lcd_match_pairs_dev cannot
 * see them and leaves it to the caller (other ids give ids that mean nothing, never an access out of bounds).
 * flags without LCD_Q_INCREMENTAL: LCD_ERR_INVALID (a fixed dictionary without indexed words returns an empty list, :926).
 *
 * LCD_MATCH_CROSS_CHECK (Vis/CorNNType 5, :1451-1453: cv::BFMatcher(NORM_HAMMING | NORM_L2SQR, crossCheck = true).match(to, from)).  OpenCV's
 * source is not part of the reference tree, so the rule is defined by the ENGINE.  With D[i][j] the exact distance of to-row i and from-row j
 * (the bits lcd_knn2 returns):
 *     nn(i)   = argmin over j of D[i][j], the lowest j on ties;
 *     back(j) = the i with the smallest D[i][j] among { i : nn(i) == j }, the lowest i on ties;
 *     out_to_match[i] = nn(i) if back(nn(i)) == i, else -1;      out_to_dist[i] = D[i][nn(i)] for EVERY to-row, -1.0f when `from` is empty.
 * A from-row is kept by the closest of the to-rows that chose it (cv::batchDistance's cross-check as best known); this is NOT the symmetric
 * mutual nearest neighbour: a from-row's own nearest to-row is never computed.
 * The reference's id bookkeeping behind the match (:1465-1477) is the host mirror's (VWDictionaryHip::matchFrames).
 *
 * Limits and errors -- after each of them nothing was written and the handle stays usable: more than 8192 rows on one side of a pair or
 * n_pairs > 65535 LCD_ERR_UNSUPPORTED; offsets that do not start at 0 or decrease, a NULL pointer where the mode needs an input or output (rows or an output of zero rows may be NULL),
 * an unknown mode or a wrong struct_size LCD_ERR_INVALID; lcd_match_pairs_dev on a handle whose rows are padded (lcd_config.dim)
 * LCD_ERR_UNSUPPORTED (lcd_match_pairs serves it).  Not offered across sharded handles.
 * Pipelined handles: see lcd_config.pipeline -- this is the one call that does NOT complete what the handle owes.  It runs on scratch of its
 * own (counted in lcd_stats.bytes_device), two launches per group of pairs; a batch whose distance blocks exceed the larger of 256 MiB and
 * the largest single pair runs in consecutive groups ("pair_match_budget" of lcd_set_option moves the 256 MiB, results never depend on it). */
enum lcd_match_mode { LCD_MATCH_DICTIONARY = 0, LCD_MATCH_CROSS_CHECK = 1 };
typedef struct lcd_match_args {
    int32_t struct_size;            /* sizeof(lcd_match_args) */
    int32_t mode;                   /* lcd_match_mode */
    int32_t n_pairs;                /* >= 0; 0 returns LCD_OK */
    int32_t flags;                  /* lcd_quantize_flags, dictionary mode only */
    float   nndr_ratio;             /* Vis/CorNNDR, dictionary mode only */
    int32_t reserved;
    const void* from; const void* to;                          /* rows of all pairs, concatenated, the handle's dtype and dim (device entry: 16-byte aligned) */
    const int64_t* from_offsets; const int64_t* to_offsets;    /* HOST, [n_pairs + 1] row offsets, non-decreasing, [0] == 0 */
    const int32_t* from_word_ids;   /* may be NULL; dictionary mode: orignalWordsFromIds, one per from-row */
    int32_t* out_from_word_ids;     /* dictionary mode, one per from-row */
    int32_t* out_to_word_ids;       /* dictionary mode, one per to-row */
    int32_t* out_to_match;          /* cross-check mode, one per to-row: from-row index WITHIN its pair, -1 = none */
    float*   out_to_dist;           /* cross-check mode, may be NULL: distance to nn(i), written whether or not the match is kept */
} lcd_match_args;
/* every pointer on the HOST; synchronises the engine stream */
int lcd_match_pairs(lcd_engine* h, const lcd_match_args* a);
/* from, to, from_word_ids and out_* in DEVICE memory, the offsets on the HOST (read during the call); enqueued on the engine stream, not synchronised */
int lcd_match_pairs_dev(lcd_engine* h, const lcd_match_args* a);

/* ---- guided two-frame matching, stateless: what the verification runs whenever the caller has a guess transform (RegistrationVis.cpp:1078-1365,
 * Vis/CorGuessWinSize > 0: proximity detection with an odometry guess, the local loop closures in time, odometry refining, the graph's
 * re-registration).  The from-frame's 3-D points have been projected into the to-image; a descriptor is compared only with the descriptors
 * whose keypoints lie within `radius` pixels of the projection.  Stateless exactly as lcd_match_pairs: any number of pairs per call, nothing
 * of the handle's vocabulary, index, Bayes filter or numbering is read or written, a pipelined handle is not drained.
 *
 * The projection stays with the CALLER (cv::Rodrigues, cv::projectPoints, the in-bounds / z > 0 / duplicate filter and the multi-camera x
 * offset, :1032-1070: OpenCV is not part of the reference tree).  Per pair the caller passes what that block produces: `corners`
 * (cornersProjected, [n_corners x 2] fp32, the to-image's stitched coordinates), `corner_from_row` (projectedIndexToDescIndex: the from-row
 * of each corner WITHIN the pair; it need not be monotone nor cover every from-row), `to_points` (cv::KeyPoint::convert(kptsTo), [nt x 2]
 * fp32), the descriptor rows laid out as for lcd_match_args, and radius = (float)Vis/CorGuessWinSize.  Pair p owns the corners
 * [corner_offsets[p], corner_offsets[p+1]).  The descriptor of corner c is from[corner_from_row[c]].
 *
 * The rule.  A QUERY is a corner (LCD_GUIDED_PROJECTED_TO_FRAME, Vis/CorGuessMatchToProjection = false, the default, :1222-1364) or a to-row
 * (LCD_GUIDED_FRAME_TO_PROJECTED, :1080-1221); the TARGETS are the other side.
 *   1. Window: W(q) = { t : d2(q, t) < radius * radius }, d2 = rtflann's L2_Simple (dist.h:74-91) in fp32 without fused multiply-add:
 *      fl(fl(dx * dx) + fl(dy * dy)), radius * radius one fp32 product; the comparison is strict (result_set.h:477); a NaN coordinate is in
 *      no window.  The reference searches a kd-tree with 32 checks (:1085-1094, :1228-1235), best-bin-first: it may return a subset, in
 *      traversal order.  The engine's window is the EXACT set -- the same decision as "Vis/CorNNType 0-4 all mean the exact search".
 *   2. Decision.  |W| = 0: no match.  |W| = 1: that target, WITHOUT a descriptor comparison (:1150-1153, :1303-1306).  |W| >= 2: d1 <= d2 are
 *      the two smallest exact descriptor distances over W (the bits lcd_knn2 returns: squared L2, or Hamming over every byte) and the
 *      LOWEST TARGET INDEX WINS TIES -- the reference's order among equal distances is the kd-tree's traversal order, so this is defined by
 *      the ENGINE.  LCD_GUIDED_RATIO (Vis/CorNNType 0-4): matched iff d1 < nndr_ratio * d2, the product rounded to fp32, the comparison
 *      strict (:1144, :1297 -- not VWDictionary's <=: d1 == d2 == 0 is no match).  LCD_GUIDED_NEAREST (type 5): the nearest target, always
 *      (a crossCheck matcher with one query row keeps its only chooser).
 *   3. Projected-to-frame only: out_to_owner[t] = the lowest corner index whose decision is to-row t, or -1 -- addedWordsTo's first-come
 *      rule (:1319-1331): a later corner loses even when it is closer.  The reference's isFinite(kptsFrom3D) test (:1260) is the caller's,
 *      who passes only such corners.
 * Outputs, one per query (corners, or to-rows): out_count = |W| (info.projectedIDs lists the corners with count > 0); out_match = the target
 * index WITHIN the pair (a to-row, or a corner) or -1, before the first-come rule; out_dist (may be NULL) = d1, d2, both -1.0f for |W| <= 1.
 * The id bookkeeping behind the match is the host mirror's (VWDictionaryHip::matchFramesGuided).
 *
 * Limits and errors -- after each of them nothing was written and the handle stays usable: more than 8192 rows or corners on one side of a
 * pair, n_pairs > 65535, a handle of a sharded vocabulary (lcd_set_option "shard_*"; not offered by lcd_shard.h either), or
 * lcd_match_guided_dev on a handle whose rows are padded: LCD_ERR_UNSUPPORTED; offsets that do not start at 0 or decrease, a radius that is
 * not finite or <= 0, a wrong struct_size / direction / nn_type, a NULL pointer where rows, corners or outputs exist: LCD_ERR_INVALID;
 * lcd_match_guided also refuses a corner_from_row outside [0, nf) with LCD_ERR_INVALID.  lcd_match_guided_dev cannot see them: there such a
 * corner is treated as NO CANDIDATE -- as a query it gets count 0 and match -1, as a target it is in no window -- and its from-row is never
 * dereferenced.  n_pairs == 0 returns LCD_OK.
 * One kernel launch and one fill per call whatever the batch; scratch is O(rows) (the job table and, for the host entry, the staged rows). */
enum lcd_guided_direction { LCD_GUIDED_PROJECTED_TO_FRAME = 0, LCD_GUIDED_FRAME_TO_PROJECTED = 1 };
enum lcd_guided_nn_type { LCD_GUIDED_RATIO = 0, LCD_GUIDED_NEAREST = 1 };
typedef struct lcd_guided_args {
    int32_t struct_size;            /* sizeof(lcd_guided_args) */
    int32_t direction;              /* lcd_guided_direction */
    int32_t nn_type;                /* lcd_guided_nn_type */
    int32_t n_pairs;                /* >= 0; 0 returns LCD_OK */
    float   radius;                 /* (float)Vis/CorGuessWinSize, pixels; finite and > 0 */
    float   nndr_ratio;             /* Vis/CorNNDR, LCD_GUIDED_RATIO only */
    const void* from; const void* to;                          /* rows of all pairs, concatenated, the handle's dtype and dim (device entry: 16-byte aligned) */
    const float* corners;           /* [n_corners x 2], all pairs concatenated */
    const int32_t* corner_from_row; /* one per corner: from-row within its pair */
    const float* to_points;         /* [n_to x 2], one per to-row */
    const int64_t* from_offsets; const int64_t* to_offsets; const int64_t* corner_offsets;   /* HOST, [n_pairs + 1], non-decreasing, [0] == 0 */
    int32_t* out_count;             /* one per query: |W| */
    int32_t* out_match;             /* one per query: target index within the pair, -1 = none */
    float*   out_dist;              /* may be NULL; [2] per query: d1, d2 */
    int32_t* out_to_owner;          /* projected-to-frame only, one per to-row: lowest corner index within the pair that chose it, -1 = none */
} lcd_guided_args;
/* every pointer on the HOST; synchronises the engine stream */
int lcd_match_guided(lcd_engine* h, const lcd_guided_args* a);
/* rows, corners, corner_from_row, to_points and out_* in DEVICE memory (points 8-byte aligned), the offsets on the HOST (read during the
 * call); enqueued on the engine stream, not synchronised */
int lcd_match_guided_dev(lcd_engine* h, const lcd_guided_args* a);

/* ---- keypoint limiting and the -1, -2, ... word ids, stateless: the quantisation glue of Memory::createSignature (Memory.cpp:5941-6059) for a
 * caller whose extractor leaves responses, positions and descriptors in device memory.  SELECTION (:5951-6023, Feature2D::limitKeypoints,
 * Features2d.cpp:293-516) picks the features that are quantised; EXPANSION (:6029-6059) puts the word ids back onto all features and numbers
 * the ones without a word -1, -2, ...  Stateless exactly as lcd_match_pairs: the calls borrow the handle's dtype, dim, device and stream,
 * read and write nothing of its vocabulary, index, Bayes filter or numbering, do not complete what a pipelined handle owes, and keep their
 * job table in the scratch lcd_match_pairs uses (counted in lcd_stats.bytes_device).  A call serves any number of frames: frame f owns the
 * features [offsets[f], offsets[f+1]) of every array; an index is a position WITHIN its frame.
 *
 * The selection rule.
 *   Key.  The key of feature i is (bits(response[i]) & 0x7FFFFFFF, i), compared lexicographically; "stronger" = the larger key.  This is the
 *      reverse iteration of the reference's std::multimap<float, int> over fabs(response) (:362-371, :453-463): equivalent keys are inserted at
 *      the upper bound, so among equal responses the HIGHER index comes first; -0.0 equals 0.0, denormals keep their order.  A NaN response
 *      breaks the reference's ordering: lcd_select_features refuses it (LCD_ERR_INVALID), lcd_select_features_dev orders it by the same masked
 *      bits, above +inf -- the ENGINE's definition.
 *   A frame of n features is CUT when max_features > 0 and n > max_features; a frame that is not cut selects everything, in its own order,
 *      whatever the order, the grid and the points (the whole-frame early exit, :297, :414, :481): out_index = 0, 1, ..., n - 1.
 *   LCD_SELECT_KEEP_ORDER (the inlier mask of :412-516 compacted as :5999-6019 compacts it): out_index is quantizedToRawIndices, the selected
 *      features in ASCENDING index.  1 x 1 grid: exactly the max_features strongest.  Larger grid (Kp/GridRows, Kp/GridCols; :479-516):
 *      rowSize = height / grid_rows, colSize = width / grid_cols, perCell = max_features / (grid_rows * grid_cols), all integer divisions;
 *      the cell of feature i is (int(y) / rowSize, int(x) / colSize), the conversion and the division both truncating toward zero (so a
 *      coordinate in (-rowSize, 0) still belongs to row 0); a cell keeps its perCell strongest features when it holds more than perCell AND
 *      perCell > 0, otherwise all of them -- with perCell == 0 the inner call's maxKeypoints > 0 test fails and the whole cell stays (the
 *      reference's behaviour, restated and not repaired).  The number selected can therefore exceed max_features, or stay below it.
 *      A keypoint whose cell lies outside the grid (the remainder strip when the image size does not divide; a coordinate at or below -rowSize /
 *      -colSize) fails an assertion in the reference: lcd_select_features returns LCD_ERR_INVALID; lcd_select_features_dev selects such a
 *      feature NEVER and counts it in no cell -- the ENGINE's definition; the conversion saturates (NaN -> 0) and nothing is indexed out of
 *      range.  A cut frame with height <= grid_rows or width <= grid_cols: LCD_ERR_INVALID from both entries (the reference's second assertion).
 *   LCD_SELECT_BY_RESPONSE (the compacting variant the extractors call, :356-400): a cut frame gives its max_features strongest in DESCENDING
 *      key order -- the order matters, addNewWords numbers new words in row order.  With a grid above 1 x 1: LCD_ERR_INVALID (no such variant).
 *
 * The selection rule with LCD_SELECT_SSC (Kp/SSC; Features2d.cpp:304-355 and :420-446 over util2d::SSC, util2d.cpp:2295-2366).  With the
 * bit clear every call is what it was.  With it a frame that is not cut still selects everything in its own order; a CUT frame (n after
 * n_in) of a width x height image is selected as follows.  The reference's integers, types and control flow are restated; the tie order,
 * NaN, points outside the mask and the refusals are the ENGINE's.
 *   Order.  b(i) = the bits of response[i], -0.0 taken as +0.0, mapped monotonically to unsigned (negative: ~bits; otherwise bits |
 *      0x80000000).  Feature i PRECEDES j when b(i) > b(j), or b(i) == b(j) and i < j: cv::sortIdx(.., SORT_DESCENDING) on the SIGNED
 *      response -- no fabs, unlike the key above -- with ties to the lower index, which is the engine's definition (the reference tree
 *      does not hold cv::sortIdx).  A NaN response: lcd_select_features refuses it, lcd_select_features_dev orders it by the same mapped bits.
 *   Scalars (:2299-2319, with their types).  tolerance is the float 0.1f and max_features * tolerance a float product; round() rounds
 *      halves away from zero.  m = max_features - round(max_features * 0.1f).  int exp1 = height + width + 2 m; long long exp2 = 4 width +
 *      4 m + 4 height m + height^2 + width^2 - 2 height width + 4 height width m; double exp3 = sqrt(exp2), exp4 = m - 1; sol1 =
 *      -round((exp1 + exp3) / exp4), sol2 = -round((exp1 - exp3) / exp4); high = int(the larger of the two); low = max(1, floor(sqrt(
 *      (double)n / m))); Kmin = round(m - m * 0.1f), Kmax = round(m + m * 0.1f), float arithmetic.
 *   Search (:2325-2364).  prevWidth = -1 and the result is empty.  Repeat: width = low + (high - low) / 2 (C truncation); when width ==
 *      prevWidth or low > high, leave with the result of the PREVIOUS iteration (empty before the first); otherwise c = width / 2.0, the
 *      mask has the cells [0, floor(height / c)] x [0, floor(width / c)], feature i lies in cell (floor((double)y / c), floor((double)x /
 *      c)), and the features are walked in the order above: a feature is selected iff no feature selected earlier in this iteration
 *      lies within 2 rows AND 2 columns of its cell (width / c == 2 exactly: a selected feature covers the 5 x 5 cells around its own,
 *      clamped to the mask -- the same set for cells inside the mask).  With Kmin <= size <= Kmax leave with this result; below Kmin high
 *      = width - 1, above Kmax low = width + 1; prevWidth = width.
 *      The number selected can therefore be 0 (a 16 x 16 image with n = 204 and max_features = 166 leaves before its first iteration), stay
 *      below Kmin, or EXCEED max_features (n = 124, max_features = 59 on a 33 x 17 image can give 76): the reference's behaviour, restated
 *      and not repaired.  out_count is the only place the count can be learnt.
 *   Order of the output.  LCD_SELECT_KEEP_ORDER: ascending index (the inlier mask, what Memory.cpp:5966 calls); LCD_SELECT_BY_RESPONSE: the
 *      order above (ResultVec, :336-354).
 *   Undefined in the reference, refused before anything is written: a grid above 1 x 1 with the bit (:507 passes absolute coordinates with
 *      a cell-sized image), max_features == 1 (exp4 == 0), and with a frame whose REGION is cut a NULL image_size or points or a width or
 *      height < 1: LCD_ERR_INVALID from both entries.  A keypoint whose cell lies outside the mask makes the reference read outside it;
 *      that needs a coordinate that is negative, above its image side or NaN (x == width and y == height are inside): lcd_select_features
 *      returns LCD_ERR_INVALID for every such coordinate in a cut frame; lcd_select_features_dev, iteration by iteration, never selects a
 *      feature whose cell lies outside that iteration's mask and lets it cover nothing -- the ENGINE's definition; the conversion
 *      saturates and nothing is indexed out of range.  Limits: an image side above 16384 in a frame whose region is cut (a cell
 *      coordinate fits 16 bits), or more than 8192 features in such a frame (sorted indices, cells and the table of selected cells share
 *      one workgroup's LDS; without the bit the limit stays 16384): LCD_ERR_UNSUPPORTED.
 * Outputs.  Frame f writes the first out_count[f] entries of ITS OWN region of each output (the inputs' offsets): out_index (the rest of the
 * region reads -1), out_rows and out_aux (the rest is unspecified).  Its selected rows start at out_rows + offsets[f] * row bytes, ready to be
 * lcd_frame_args.d_descriptors where that address is 16-byte aligned.  With a 1 x 1 grid the host knows the count without a read-back
 * (min(n, max_features), or n); a larger grid's count is data-dependent: out_count is where the caller gets q.  Outputs must not overlap inputs.
 *
 * Expansion, per frame of n features: (1) every feature starts without a word; (2) for j < count[f] (clamped to [0, n]):
 * all[index[j]] = resolve(word_ids[j]), where an id > 0 stands, a code -(k+1) becomes first_new_word_id[f] + k when that array is given
 * and its entry is > 0, and otherwise -- and for id 0, the fixed dictionary's "no entry", where the reference's shorter list would shift every
 * later position -- means "no word" (the ENGINE's definition); the index entries of a frame are distinct; (3) in feature order every feature
 * without a word receives -1, -2, ... (:6040-6047).  count[f] == 0 gives the all-negative list of the _badSignRatio branch (:6051-6059).
 * An index entry outside [0, n): lcd_expand_word_ids returns LCD_ERR_INVALID, lcd_expand_word_ids_dev skips it without dereferencing.
 * In the device entry count, index, word_ids and first_new_word_id are device memory: first_new_word_id can be filled by the frames'
 * d_first_new_word_id outputs (LCD_NEW_WORD_IDS_AUTO) and nothing is read back.  On a pipelined handle the call is enqueued where it lands:
 * frame t's d_word_ids are final behind the lcd_frame_dev call of frame t + lcd_pipeline_depth(), or behind lcd_synchronize -- expand then.
 *
 * Limits and errors -- after each of them nothing was written and the handle stays usable: more than 16384 features in a frame (its 64-bit
 * keys are sorted in one workgroup's LDS: 128 KiB), n_frames > 65535, grid_rows * grid_cols > 1024, a handle of a sharded vocabulary, or a
 * device entry with rows on a handle whose rows are padded (lcd_config.dim; the host entry serves it): LCD_ERR_UNSUPPORTED; offsets that do not
 * start at 0 or decrease, a NULL pointer where an input or output is needed, an unknown order, a wrong struct_size, a grid dimension < 1,
 * aux_bytes that is negative, above 64 or no multiple of 4: LCD_ERR_INVALID.  n_frames == 0 returns LCD_OK.
 * One kernel launch per call whatever the batch (one workgroup per frame), no private segment.
 *
 * Frame sizes only the device knows (n_in, n_features): behind lcd_keypoints_3d_dev's filter the host knows a frame's REGION, offsets[f] ..
 * offsets[f+1], and the device knows how many features of it are left.  With n_in the selection's frame f is the first n = clamp(n_in[f], 0,
 * region) features of its region: the cut decision n > max_features, the order and the counts go by n, the limits above (16384, the
 * workgroup size) by the region; out_index reads -1 from out_count[f] to the END OF THE REGION.  With n_features the expansion numbers the
 * first n features of the region and writes 0 behind them, to the end of the region; count[f] is clamped to n.  NULL: exactly the behaviour
 * without the field.  In the host entries both arrays are host memory.  struct_size is the one sizeof of this header. */
enum lcd_select_order { LCD_SELECT_KEEP_ORDER = 0, LCD_SELECT_BY_RESPONSE = 1 };
enum lcd_select_flags { LCD_SELECT_SSC = 1 };   /* Kp/SSC, Vis/SSC: cut frames are selected by the square covering */
typedef struct lcd_select_args {
    int32_t struct_size;            /* sizeof(lcd_select_args) */
    int32_t n_frames;               /* >= 0; 0 returns LCD_OK */
    int32_t order;                  /* lcd_select_order */
    int32_t max_features;           /* Kp/MaxFeatures; <= 0: nothing is cut */
    int32_t grid_rows, grid_cols;   /* Kp/GridRows, Kp/GridCols, >= 1 */
    int32_t aux_bytes;              /* bytes of the caller's per-feature payload (the cv::KeyPoint, the 3-D point): a multiple of 4, 0..64 */
    int32_t flags;                  /* lcd_select_flags; the bits it does not name are ignored (the field was `reserved`) */
    const int64_t* offsets;         /* HOST, [n_frames + 1], non-decreasing, [0] == 0 */
    const int32_t* image_size;      /* HOST, [n_frames x 2]: width, height; may be NULL with a 1 x 1 grid and no frame cut under LCD_SELECT_SSC */
    const float* response;          /* [N] cv::KeyPoint::response */
    const float* points;            /* [N x 2] cv::KeyPoint::pt (x, y); may be NULL with a 1 x 1 grid and no frame cut under LCD_SELECT_SSC */
    const void* rows;               /* may be NULL: [N x dim] of the handle's dtype */
    const void* aux;                /* may be NULL (aux_bytes == 0): [N x aux_bytes] */
    int32_t* out_count;             /* [n_frames] */
    int32_t* out_index;             /* [N] */
    void* out_rows;                 /* [N x dim], needed with rows */
    void* out_aux;                  /* [N x aux_bytes], needed with aux */
    const int32_t* n_in;            /* may be NULL; [n_frames], DEVICE memory for the _dev entry: frame f is the first
                                       clamp(n_in[f], 0, offsets[f+1] - offsets[f]) features of its region (lcd_keypoints_3d_args.out_count) */
} lcd_select_args;
/* every pointer on the HOST; synchronises the engine stream */
int lcd_select_features(lcd_engine* h, const lcd_select_args* a);
/* response, points, rows, aux and out_* in DEVICE memory (4-byte aligned; rows and aux are copied as 16-byte vectors where their addresses and
 * sizes allow), offsets and image_size on the HOST (read during the call); enqueued on the engine stream, not synchronised */
int lcd_select_features_dev(lcd_engine* h, const lcd_select_args* a);

typedef struct lcd_expand_args {
    int32_t struct_size;            /* sizeof(lcd_expand_args) */
    int32_t n_frames;               /* >= 0; 0 returns LCD_OK */
    const int64_t* offsets;         /* HOST, [n_frames + 1], non-decreasing, [0] == 0 */
    const int32_t* count;           /* [n_frames]: the selected features of each frame (lcd_select_args.out_count) */
    const int32_t* index;           /* [N]: frame f's selected features at offsets[f], count[f] of them valid (lcd_select_args.out_index) */
    const int32_t* word_ids;        /* [N]: frame f's ids at offsets[f], count[f] of them valid, as lcd_quantize / lcd_frame_dev write them */
    const int32_t* first_new_word_id;   /* may be NULL; [n_frames] */
    int32_t* out_word_ids;          /* [N]: one id per feature */
    const int32_t* n_features;      /* may be NULL; [n_frames], DEVICE memory for the _dev entry: frame f has clamp(n_features[f], 0, its region)
                                       features (lcd_keypoints_3d_args.out_count) */
} lcd_expand_args;
/* every pointer on the HOST; synchronises the engine stream */
int lcd_expand_word_ids(lcd_engine* h, const lcd_expand_args* a);
/* count, index, word_ids, first_new_word_id and out_word_ids in DEVICE memory, the offsets on the HOST; enqueued on the engine stream, not synchronised */
int lcd_expand_word_ids_dev(lcd_engine* h, const lcd_expand_args* a);

/* ---- depth to 3-D keypoints and the depth filter, stateless: the depth stage in front of the selection (Memory.cpp:5683-5694, :5911-5915,
 * RegistrationVis.cpp:926-969) for a caller whose keypoints and depth image are in device memory.  Feature2D::generateKeypoints3D ->
 * util3d::generateKeypoints3DDepth (util3d_features.cpp:67-120) looks every keypoint up in the depth image (util2d::getDepth,
 * util2d.cpp:947-1111) and projects it (util3d::projectDepthTo3D, util3d.cpp:215-244); Feature2D::filterKeypointsByDepth drops the
 * keypoints without a point in range and compacts keypoints, descriptors and points (3-D overload Features2d.cpp:167-212, 2-D overload
 * :105-165).  Stateless exactly as lcd_select_features: the calls borrow the handle's dtype, dim, device and stream, read and write nothing
 * of its state, do not complete what a pipelined handle owes, and keep their job table in the scratch lcd_match_pairs uses.  A call serves
 * any number of frames: frame f owns the features [offsets[f], offsets[f+1]) of every array and has its own depth image, images[f] (frames
 * may share one).
 *
 * The rule.  All arithmetic is fp32, every operation rounded on its own: no product is fused into a sum anywhere (the reference's x86-64
 * build has no fused multiply-add), division is IEEE division.  int(v) truncates toward zero.
 *   Per frame (util3d_features.cpp:79-83): subCols = width / n_cameras (integer), subW = float(subCols);
 *      factorX = 1.0f / (image_width > 0 ? float(image_width) / subW : 1.0f), factorY = 1.0f / (image_height > 0 ? float(image_height) /
 *      float(height) : 1.0f), image_width and image_height those of cameras[0].
 *   Per keypoint (:87-102): x = pt.x * factorX, y = pt.y * factorY, cam = int(x / subW).  The lookup runs in camera cam's SUB-IMAGE, the
 *      columns [cam * subCols, (cam + 1) * subCols) of the depth image, at the coordinates (x - subW * float(cam), y), with the intrinsics
 *      cx * factorX, cy * factorY, fx * factorX, fy * factorY of cameras[cam].  cols = subCols and rows = height below.
 *   getDepth with smoothing = true, depthErrorRatio = 0.02f, estWithNeighborsIfNull = false (util2d.cpp:957-1110):
 *      u = int(x + 0.5f), v = int(y + 0.5f) -- a coordinate in (-1.5, -0.5) therefore lands on pixel 0 (the reference's behaviour, restated);
 *      u == cols && x < float(cols) gives u = cols - 1, the same for v and rows; outside [0, cols) x [0, rows) the depth is 0.
 *      A u16 pixel p is a measurement when it is neither 0 nor 65535, its value float(p) * 0.001f, otherwise 0; an f32 pixel is taken as it is.
 *      A centre depth of 0 or not finite gives 0.  Otherwise the window [max(u-1, 0), min(u+1, cols-1)] x [max(v-1, 0), min(v+1, rows-1)] --
 *      clipped to the SUB-IMAGE, never reading across the seam to the next camera -- is visited with uu in the OUTER loop and vv in the inner
 *      one, the centre left out (this order fixes the float sums).  A neighbour d counts when d != 0, d is finite and
 *      fabs(d - depth) < 0.02f * depth, strictly; with uu == u or vv == v (an edge neighbour) sumWeights += 2.0f and sumDepths += d * 2.0f,
 *      otherwise (a corner) sumWeights += 1.0f and sumDepths += d.  depth = (depth * 4.0f + sumDepths) / (sumWeights + 4.0f).
 *   projectDepthTo3D (util3d.cpp:228-242): depth > 0 is required (a negative f32 depth is a bad point); a cx that is not > 0 is replaced by
 *      float(cols / 2) - 0.5f, a cy by float(rows / 2) - 0.5f; X = ((x - cx) * depth) / fx, Y = ((y - cy) * depth) / fy, Z = depth.
 *   Range test, before the local transform (util3d_features.cpp:104-115): the point stands iff X, Y and Z are finite and
 *      (min_depth < 0 || Z > min_depth) && (max_depth <= 0 || Z <= max_depth); otherwise it is three quiet NaNs (0x7FC00000).  A point that
 *      stands goes through transformPoint when has_local_transform (util3d_transforms.cpp:211-220, left to right):
 *      X' = ((t[0] * X + t[1] * Y) + t[2] * Z) + t[3], Y' and Z' with t[4..7] and t[8..11].
 *   LCD_KP3D_KEEP_ALL: every keypoint is kept: out_count[f] = n, out_index = 0 .. n - 1, out_xyz[i] is keypoint i's point; nothing else is written.
 *   LCD_KP3D_FILTER_3D (Features2d.cpp:183-191): keep iff the three coordinates are finite and d2 = (X * X + Y * Y) + Z * Z satisfies
 *      d2 >= min_depth * min_depth && (max_depth * max_depth == 0 || d2 <= max_depth * max_depth).
 *   LCD_KP3D_FILTER_PIXEL (the 2-D overload the extractors call in front of limitKeypoints, :120-132): u = int(pt.x + 0.5f),
 *      v = int(pt.y + 0.5f) in the WHOLE image, no factors and no clamp; outside [0, width) x [0, height) the keypoint goes; d = float(p) *
 *      0.001f for a u16 pixel WITHOUT the 0 / 65535 test, the f32 pixel as it is; keep iff d is finite, d > min_depth and
 *      (max_depth <= 0 || d < max_depth).  out_xyz may be NULL; where it is given, the kept keypoints' points are computed as above.
 *   The engine's definitions, where the reference asserts or is undefined: a keypoint for which x + 0.5f, y + 0.5f or x / subW (with
 *      LCD_KP3D_FILTER_PIXEL also pt.x + 0.5f, pt.y + 0.5f) is not finite or not inside (-2^31, 2^31), or whose cam is outside [0, n_cameras):
 *      lcd_keypoints_3d returns LCD_ERR_INVALID; lcd_keypoints_3d_dev gives it the bad point, keeps it under no filter and reads no pixel for
 *      it.  (Without out_xyz, LCD_KP3D_FILTER_PIXEL looks at pt alone.)  min_depth < 0 with a filter, 0 < max_depth <= min_depth, or a NaN
 *      bound: LCD_ERR_INVALID (the reference's assertions).
 * Outputs follow the selection's convention: frame f writes the first out_count[f] entries of ITS OWN region of out_index (kept features in
 * ascending index; the rest of the region reads -1), out_xyz, out_points, out_response, out_rows and out_aux (the rest is unspecified), so
 * out_count can be lcd_select_args.n_in and the out_* arrays the selection's inputs, nothing read back.  Outputs must not overlap inputs.
 *
 * Limits and errors -- after each of them nothing was written and the handle stays usable: n_frames > 65535, a handle of a sharded vocabulary,
 * or a device entry with rows on a handle whose rows are padded: LCD_ERR_UNSUPPORTED; offsets that do not start at 0 or decrease, a NULL
 * pointer where an input or output is needed (out_xyz except with LCD_KP3D_FILTER_PIXEL; with a filter out_points, and out_response, out_rows,
 * out_aux with their inputs), an image without data, cameras or pixels, width % n_cameras != 0, an unknown type or filter, a pitch below
 * the row or data / pitch not aligned to the pixel size, a wrong struct_size, aux_bytes that is negative, above 64 or no multiple of 4:
 * LCD_ERR_INVALID.  n_frames == 0 returns LCD_OK.  There is no limit on the features of a frame: nothing is sorted.
 * One kernel launch per call whatever the batch (one workgroup of 256 threads per frame), no private segment. */
enum lcd_depth_type  { LCD_DEPTH_U16_MM = 0, LCD_DEPTH_F32_M = 1 };      /* CV_16UC1 millimetres, CV_32FC1 metres */
enum lcd_kp3d_filter { LCD_KP3D_KEEP_ALL = 0, LCD_KP3D_FILTER_3D = 1, LCD_KP3D_FILTER_PIXEL = 2 };
typedef struct lcd_camera {         /* HOST */
    float fx, fy, cx, cy;           /* of the CameraModel, before the rgb-to-depth factors */
    int32_t image_width, image_height;   /* CameraModel::imageWidth() / imageHeight(), may be 0; cameras[0]'s decide the factors */
    int32_t has_local_transform;    /* the caller's !localTransform().isNull() && !localTransform().isIdentity() */
    int32_t reserved;
    float local_transform[12];      /* row-major 3 x 4 */
} lcd_camera;
typedef struct lcd_depth_image {    /* HOST array, one per frame */
    const void* data;               /* DEVICE memory for the _dev entry, HOST memory for the host entry; aligned to the pixel size */
    int64_t pitch_bytes;            /* bytes between rows, >= the row, a multiple of the pixel size */
    int32_t width, height;          /* pixels, >= 1 */
    int32_t type;                   /* lcd_depth_type */
    int32_t n_cameras;              /* >= 1, width % n_cameras == 0: the sub-images side by side */
    const lcd_camera* cameras;      /* HOST, [n_cameras] */
} lcd_depth_image;
typedef struct lcd_keypoints_3d_args {
    int32_t struct_size;            /* sizeof(lcd_keypoints_3d_args) */
    int32_t n_frames;               /* >= 0; 0 returns LCD_OK */
    int32_t filter;                 /* lcd_kp3d_filter */
    int32_t aux_bytes;              /* bytes of the caller's per-feature payload: a multiple of 4, 0..64 */
    float min_depth, max_depth;     /* Kp/MinDepth, Kp/MaxDepth (Vis/MinDepth, Vis/MaxDepth for the registration) */
    const int64_t* offsets;         /* HOST, [n_frames + 1], non-decreasing, [0] == 0 */
    const lcd_depth_image* images;  /* HOST, [n_frames] */
    const float* points;            /* [N x 2] cv::KeyPoint::pt (x, y) */
    const float* response;          /* may be NULL: [N] */
    const void* rows;               /* may be NULL: [N x dim] of the handle's dtype */
    const void* aux;                /* may be NULL (aux_bytes == 0): [N x aux_bytes] */
    int32_t* out_count;             /* [n_frames] */
    int32_t* out_index;             /* [N]: the kept features in ascending index, the rest of the region -1 */
    float* out_xyz;                 /* [N x 3]; may be NULL with LCD_KP3D_FILTER_PIXEL */
    float* out_points;              /* [N x 2], needed with a filter */
    float* out_response;            /* [N], needed with a filter and response */
    void* out_rows;                 /* [N x dim], needed with a filter and rows */
    void* out_aux;                  /* [N x aux_bytes], needed with a filter and aux */
} lcd_keypoints_3d_args;
/* every pointer on the HOST (the images' data too); synchronises the engine stream */
int lcd_keypoints_3d(lcd_engine* h, const lcd_keypoints_3d_args* a);
/* the images' data, points, response, rows, aux and out_* in DEVICE memory (points 8-byte aligned, the rest 4-byte; rows and aux are copied as
 * 16-byte vectors where their addresses and sizes allow); offsets, images and cameras on the HOST (read during the call); enqueued on the
 * engine stream, not synchronised */
int lcd_keypoints_3d_dev(lcd_engine* h, const lcd_keypoints_3d_args* a);

/* ---- stereo keypoints to 3-D, stateless: lcd_keypoints_3d for a frame that has a right image instead of a depth image (Features2d.cpp:960-1016
 * with Stereo/OpticalFlow = true).  Stereo::computeCorrespondences tracks every left corner into the right image
 * (util2d::calcOpticalFlowPyrLKStereo, util2d.cpp:371-736: pyramidal Lucas-Kanade whose correction is forced onto the x axis),
 * StereoOpticalFlow::updateStatus gates the disparity (Stereo.cpp:240-268), util3d::generateKeypoints3DStereo projects each corner through
 * the stereo model (util3d_features.cpp:158-203, util3d::projectDisparityTo3D util3d.cpp:2806-2825), and the filter and the compaction
 * are lcd_keypoints_3d's.  Stateless exactly as lcd_keypoints_3d; frame f owns the features [offsets[f], offsets[f+1]) of every array and
 * has its own image pair, images[f] (frames may share a pair: its pyramids are built once).
 *
 * The rule.  No product is fused into a sum anywhere; int is 32 bits, >> is arithmetic.
 *   Pyramid -- the ENGINE'S rule, after OpenCV's buildOpticalFlowPyramid with pyrBorder = BORDER_REFLECT_101 and derivBorder =
 *   BORDER_CONSTANT; nothing of it is in the reference tree:
 *      Level 0 is the image.  Level l+1 has size ((w+1)/2, (h+1)/2).  Its pixel is
 *      (SUM_{i,j} k[i]*k[j]*src(reflect101(2y+i-2), reflect101(2x+j-2)) + 128) >> 8, with k = {1,4,6,4,1}.
 *      Building stops before the first level whose width is <= win_width or whose height is <= win_height.  It stops after level max_level
 *      at the latest.  Both images get the same number of levels.
 *      A pixel read outside a level is reflect101 (p < 0 -> -p, p >= n -> 2n-2-p, repeated until inside).  It is read at most win_width
 *      columns or win_height rows outside.
 *      The derivative of the LEFT level at a pixel inside is Scharr's, with reflect101 on its own taps:
 *         dx(x,y) = t0(x+1,y) - t0(x-1,y), where t0(x,y) = (I(x,y-1) + I(x,y+1))*3 + I(x,y)*10.
 *         dy(x,y) = (t1(x-1,y) + t1(x+1,y))*3 + t1(x,y)*10, where t1(x,y) = I(x,y+1) - I(x,y-1).
 *      The derivative read outside the level is 0.  All of this is int.
 *   Tracker -- the reference's, util2d.cpp:504-735, term for term, for every keypoint on its own, level = top .. 0:
 *      prevPt = pt * float(1/2^level); nextPt = prevPt at the top level, otherwise the previous nextPts * 2.f; nextPts = nextPt (:531-542).
 *      halfWin = ((w-1)*0.5f, (h-1)*0.5f); prevPt -= halfWin; iprevPt = cvFloor(prevPt).  iprevPt.x < -w || >= cols || iprevPt.y < -h ||
 *      >= rows: at level 0 the status becomes 0; the level is skipped (nextPts keeps its scaled position) (:545-560).
 *      a = prevPt.x - iprevPt.x, b likewise; iw00 = cvRound((1.f-a)*(1.f-b)*16384), iw01 = cvRound(a*(1.f-b)*16384), iw10 =
 *      cvRound((1.f-a)*b*16384), iw11 = 16384 - iw00 - iw01 - iw10; cvRound rounds half to EVEN (:562-569).
 *      Window pixel (x, y), y outer, x inner (row-major -- that order is the rule for every float sum below): with the four neighbours
 *      p00 = (X, Y), p01 = (X+1, Y), p10 = (X, Y+1), p11 = (X+1, Y+1), X = iprevPt.x + x, Y = iprevPt.y + y:
 *      ival = (I00*iw00 + I01*iw01 + I10*iw10 + I11*iw11 + 256) >> 9, ixval and iyval the same of dx and dy with (.. + 8192) >> 14;
 *      iA11 += float(ixval*ixval), iA12 += float(ixval*iyval), iA22 += float(iyval*iyval), fp32 accumulators, each product an int (:579-606).
 *      A11 = iA11 * 2^-20, A12, A22 alike; D = A11*A22 - A12*A12; minEig = (A22 + A11 - sqrt((A11-A22)*(A11-A22) + 4.f*A12*A12)) /
 *      float(2*w*h), sqrt and division correctly rounded fp32.  double(minEig) < min_eig_threshold || D < FLT_EPSILON: at level 0 the
 *      status becomes 0; the level is skipped.  D = 1.f / D (:608-626).
 *      nextPt -= halfWin; for j < iterations: inextPt = cvFloor(nextPt); outside as above (with the RIGHT level's cols, rows): at level 0
 *      status 0; break.  The weights of nextPt; diff = ((J00*iw00 + J01*iw01 + J10*iw10 + J11*iw11 + 256) >> 9) - ival;
 *      ib1 += float(diff*ixval), ib2 += float(diff*iyval); b1 = ib1 * 2^-20, b2 alike; delta.x = ((A12*b2) - (A22*b1)) * D, delta.y = 0;
 *      nextPt += delta; nextPts = nextPt + halfWin (both coordinates); double(delta.x)*delta.x + 0.0 <= eps^2: break;
 *      j > 0 && double(fabsf(delta.x + prevDelta.x)) < 0.01: nextPts.x -= delta.x*0.5f, break; prevDelta = delta (:628-691).
 *      iterations is clamped to [0, 100], eps to [0, 10] and squared in double (:493-501).
 *      use_min_eigenvals == 0: at level 0, status still set, the window at nextPts - halfWin (outside: status 0) gives
 *      err = (SUM float(|diff|)) / float(32*w*h) (:693-731).
 *      cvFloor of a value that is not finite or not inside int gives INT_MIN (what the reference's x86-64 conversion gives): outside.
 *   updateStatus (Stereo.cpp:240-268): status set and (use_min_eigenvals != 0 or double(err) < error_threshold): d = left.x - right.x;
 *      d <= min_disparity || d > max_disparity: status 0.  A keypoint whose err is not below the threshold keeps its status and is gated by
 *      nothing (the reference only counts it).
 *   generateKeypoints3DStereo and projectDisparityTo3D: the point is bad (three quiet NaNs) unless status is set, d != 0 and d > 0.
 *      c = float(right_cx - cx) when both are > 0, otherwise 0.  W = float(baseline / double(d + c)).
 *      X = float((double(pt.x) - cx) * double(W)).  Y = float((double(pt.y) - cy) * fx / fy * double(W)), evaluated left to right.
 *      Z = float(fx * double(W)).  Then the range test and transformPoint exactly as lcd_keypoints_3d states them.
 *   filter: LCD_KP3D_KEEP_ALL or LCD_KP3D_FILTER_3D, the rule lcd_keypoints_3d has.  LCD_KP3D_FILTER_PIXEL has no meaning without a
 *      depth image: LCD_ERR_INVALID.
 *   out_right [N x 2] and out_status [N] (both optional): the right corner (nextPts) and the status of every INPUT keypoint by input index,
 *      behind updateStatus.  A caller who wants only Stereo::computeCorrespondences passes out_xyz and these.
 *   The engine's definitions, where the reference asserts or is undefined: win_width or win_height < 3 or > 31, max_level outside 0..8,
 *      width <= win_width or height <= win_height, baseline <= 0 or fx <= 0, a NaN among the parameters, the depth bounds or the camera's
 *      doubles, min_disparity < 0 or min_disparity > max_disparity: LCD_ERR_INVALID.  A keypoint whose coordinates are not finite or not
 *      inside (-2^31, 2^31): lcd_keypoints_3d_stereo returns LCD_ERR_INVALID; lcd_keypoints_3d_stereo_dev gives it status 0, the right
 *      corner (NaN, NaN) and the bad point.
 * Outputs, limits and errors follow lcd_keypoints_3d (a sharded handle, a _dev call with rows on a padded handle, n_frames > 65535:
 * LCD_ERR_UNSUPPORTED; NULL pointers, a pitch below the row, a wrong struct_size: LCD_ERR_INVALID; n_frames == 0: LCD_OK).  The depth bounds
 * are checked as lcd_keypoints_3d checks them.  There is no limit on the features of a frame.
 * Launches: one per pyramid level for the whole batch, one for the tracker (one wave per keypoint), one for the projection, the filter and
 * the compaction (one workgroup per frame); nothing is read back between them, no private segment. */
typedef struct lcd_stereo_camera {  /* HOST; the reference's accessors are double */
    double fx, fy, cx, cy;          /* the left model */
    double right_cx;                /* the right model's cx (0: no correction) */
    double baseline;                /* StereoCameraModel::baseline(), > 0 */
    int32_t has_local_transform;    /* the caller's !localTransform().isNull() && !localTransform().isIdentity() */
    int32_t reserved;
    float local_transform[12];      /* row-major 3 x 4 */
} lcd_stereo_camera;
typedef struct lcd_stereo_image {   /* HOST array, one per frame */
    const void* left;               /* 8-bit single-channel; DEVICE memory for the _dev entry, HOST memory for the host entry */
    const void* right;
    int64_t left_pitch_bytes, right_pitch_bytes;   /* bytes between rows, >= width */
    int32_t width, height;          /* of both images; > win_width, > win_height */
    const lcd_stereo_camera* camera;   /* HOST */
} lcd_stereo_image;
typedef struct lcd_stereo_params {  /* HOST */
    int32_t win_width, win_height;  /* Stereo/WinWidth 15, Stereo/WinHeight 3; 3..31 */
    int32_t max_level;              /* Stereo/MaxLevel 5; 0..8 */
    int32_t iterations;             /* Stereo/Iterations 30 */
    double eps;                     /* Stereo/Eps 0.01 */
    int32_t use_min_eigenvals;      /* 1: OPTFLOW_LK_GET_MIN_EIGENVALS; 0: the L1 error against error_threshold */
    int32_t reserved;
    double min_eig_threshold;       /* 1e-4 */
    double error_threshold;         /* 50 */
    float min_disparity, max_disparity;   /* Stereo/MinDisparity 0.5, Stereo/MaxDisparity 128 */
} lcd_stereo_params;
typedef struct lcd_keypoints_3d_stereo_args {
    int32_t struct_size;            /* sizeof(lcd_keypoints_3d_stereo_args) */
    int32_t n_frames;               /* >= 0; 0 returns LCD_OK */
    int32_t filter;                 /* LCD_KP3D_KEEP_ALL or LCD_KP3D_FILTER_3D */
    int32_t aux_bytes;              /* a multiple of 4, 0..64 */
    float min_depth, max_depth;
    const int64_t* offsets;         /* HOST, [n_frames + 1], non-decreasing, [0] == 0 */
    const lcd_stereo_image* images; /* HOST, [n_frames] */
    const lcd_stereo_params* params;   /* HOST */
    const float* points;            /* [N x 2] the left corners (x, y) */
    const float* response;          /* may be NULL: [N] */
    const void* rows;               /* may be NULL: [N x dim] of the handle's dtype */
    const void* aux;                /* may be NULL (aux_bytes == 0): [N x aux_bytes] */
    int32_t* out_count;             /* [n_frames] */
    int32_t* out_index;             /* [N]: the kept features in ascending index, the rest of the region -1 */
    float* out_xyz;                 /* [N x 3] */
    float* out_points;              /* [N x 2], needed with a filter */
    float* out_response;            /* [N], needed with a filter and response */
    void* out_rows;                 /* [N x dim], needed with a filter and rows */
    void* out_aux;                  /* [N x aux_bytes], needed with a filter and aux */
    float* out_right;               /* may be NULL: [N x 2] by INPUT index */
    uint8_t* out_status;            /* may be NULL: [N] by INPUT index */
} lcd_keypoints_3d_stereo_args;
/* every pointer on the HOST (the images too; every distinct image is staged once); synchronises the engine stream */
int lcd_keypoints_3d_stereo(lcd_engine* h, const lcd_keypoints_3d_stereo_args* a);
/* the images, points, response, rows, aux and out_* in DEVICE memory (points and out_right 8-byte aligned); offsets, images, cameras and
 * params on the HOST (read during the call); enqueued on the engine stream, not synchronised */
int lcd_keypoints_3d_stereo_dev(lcd_engine* h, const lcd_keypoints_3d_stereo_args* a);

/* ---- optical-flow correspondences, stateless: the other way RegistrationVis finds the correspondences of two frames, Vis/CorType = 1
 * (RegistrationVis.cpp:510-780).  Every corner of the FROM image is tracked into the TO image by pyramidal Lucas-Kanade on both axes
 * (cv::calcOpticalFlowPyrLK at :697), the tracked corners that land inside the image are kept (:709-724), and both corner lists with the
 * caller's payload (the word id, the from-side 3-D point) go on to the estimators.  Stateless exactly as lcd_keypoints_3d_stereo; pair p owns
 * the features [offsets[p], offsets[p+1]) of every array and has its own two images, pairs[p].  Pairs may share images: every DISTINCT image
 * (pointer, pitch and size) gets one pyramid, built to the highest level any of its pairs needs (A->B and B->C build B once).
 *
 * The rule.  OpenCV's text is not in the reference tree, so the tracker is the ENGINE'S rule: lcd_keypoints_3d_stereo's tracker with the y
 * correction restored and the sums in the engine's lane-tree order.  No product is fused into a sum anywhere.
 *   Unchanged from lcd_keypoints_3d_stereo's rule, by reference: the pyramid, the Scharr derivative, reflect101, the 14-bit weights with
 *      half to even, ival / ixval / iyval of a window pixel, the bounds test, cvFloor, A11 / A12 / A22 -> D and minEig with their two tests,
 *      the clamping of iterations and eps.  Both images of a pair get the same number of levels: the stereo rule's count for width, height,
 *      the window and pairs[p].max_level.
 *   Start: at the top level nextPt = prevPt; with pairs[p].use_initial nextPt = initial * float(1/2^level) on both coordinates.  Below the top
 *      level it is the previous nextPts * 2.f.
 *   Sums: A11, A12, A22, b1, b2 and the L1 error are added in the lane-tree order the motion rules use (lcd_estimate_motion_3d step 4) with
 *      64 parts: with p the row-major index of the window pixel, part p % 64 adds its terms in ascending p from +0, then the 64 parts are
 *      added by the halving tree (part l += part l + s for l < s; s = 32, 16, .. 1).  Each term is float(int product) as in the stereo
 *      rule.  The stereo rule's row-major chain is NOT used here.
 *   Step: delta.x = ((A12*b2) - (A22*b1)) * D, delta.y = ((A12*b1) - (A11*b2)) * D, one operation per statement; nextPt += delta;
 *      nextPts = nextPt + halfWin.
 *   Stop: double(delta.x)*double(delta.x) + double(delta.y)*double(delta.y) <= eps^2.
 *   Oscillation: j > 0 && double(fabsf(delta.x + prevDelta.x)) < 0.01 && double(fabsf(delta.y + prevDelta.y)) < 0.01:
 *      nextPts -= delta * 0.5f on both coordinates, break.
 *   Error: use_min_eigenvals == 0: the L1 error of the stereo rule at level 0.  use_min_eigenvals == 1: out_err is minEig of the last level
 *      (the lowest) whose window at prevPt was inside, 0 where none was.
 *   Status: 0 exactly where the stereo rule sets it -- the window outside at level 0, the eigen test at level 0, leaving during the
 *      iterations at level 0, the error window outside.
 *   Keep (RegistrationVis.cpp:709-724): the status is set; to.x is finite, !(to.x < 0.f) and !(to.x >= float(width)); the same for to.y with
 *      height; use_min_eigenvals != 0 or err < error_threshold, compared in float.  The kept inputs are compacted in input order: out_from
 *      gets the input corner, out_to the tracked one, out_aux the payload, out_index the input index.
 *   out_track [N x 2], out_status [N] and out_err [N] (all optional): calcOpticalFlowPyrLK's own three outputs for every INPUT corner by
 *      input index.
 *   The engine's definitions, where OpenCV asserts or is undefined: the limits and the LCD_ERR_INVALID / LCD_ERR_UNSUPPORTED table of
 *      lcd_keypoints_3d_stereo apply (win_width or win_height outside 3..31, max_level outside 0..8, width <= win_width or height <=
 *      win_height, a NaN among eps, min_eig_threshold and error_threshold, a pitch below the row, NULL pointers, a wrong struct_size,
 *      aux_bytes: LCD_ERR_INVALID; a sharded handle, n_pairs > 65535: LCD_ERR_UNSUPPORTED; n_pairs == 0: LCD_OK).  use_initial set with
 *      initial == NULL: LCD_ERR_INVALID.  A corner, or with use_initial a start position, whose coordinates are not finite or not inside
 *      (-2^31, 2^31): lcd_track_flow returns LCD_ERR_INVALID; lcd_track_flow_dev gives it status 0, the track (NaN, NaN), err 0 and does
 *      not keep it.
 * Out of scope: the projection of the guess (cv::projectPoints, :589-651 -- the caller supplies initial, as lcd_match_guided's caller
 * supplies the projections), colour conversion, Vis/CorFlowGpu, sharded handles.
 * Launches: one per pyramid level for the whole batch, one for the tracker (one wave per corner), one for the keep test and the compaction
 * (one workgroup per pair; out_count is written on the device, so it can be lcd_select_args.n_in of a selection behind this call); nothing is
 * read back between them, no private segment. */
typedef struct lcd_flow_pair {      /* HOST array, one per pair */
    const void* from;               /* 8-bit single-channel; DEVICE memory for the _dev entry, HOST memory for the host entry */
    const void* to;
    int64_t from_pitch_bytes, to_pitch_bytes;   /* bytes between rows, >= width */
    int32_t width, height;          /* of both images; > win_width, > win_height */
    int32_t max_level;              /* 0..8; the caller writes guessSet ? 0 : Vis/CorFlowMaxLevel (3), as :695 does */
    int32_t use_initial;            /* OPTFLOW_USE_INITIAL_FLOW: the pair's rows of `initial` are the start positions */
} lcd_flow_pair;
typedef struct lcd_flow_params {    /* HOST */
    int32_t win_width, win_height;  /* both Vis/CorFlowWinSize 16; 3..31 */
    int32_t iterations;             /* Vis/CorFlowIterations 30 */
    int32_t use_min_eigenvals;      /* 1 (RegistrationVis passes OPTFLOW_LK_GET_MIN_EIGENVALS); 0: the L1 error against error_threshold */
    double eps;                     /* Vis/CorFlowEps 0.01 */
    double min_eig_threshold;       /* 1e-4 */
    float error_threshold;          /* 20, compared in float as :714 does */
    int32_t reserved;
} lcd_flow_params;
typedef struct lcd_track_flow_args {
    int32_t struct_size;            /* sizeof(lcd_track_flow_args) */
    int32_t n_pairs;                /* >= 0; 0 returns LCD_OK */
    int32_t aux_bytes;              /* a multiple of 4, 0..64 */
    int32_t reserved;
    const int64_t* offsets;         /* HOST, [n_pairs + 1], non-decreasing, [0] == 0 */
    const lcd_flow_pair* pairs;     /* HOST, [n_pairs] */
    const lcd_flow_params* params;  /* HOST */
    const float* points;            /* [N x 2] the from corners (x, y) */
    const float* initial;           /* [N x 2] the start positions; may be NULL when no pair sets use_initial */
    const void* aux;                /* may be NULL (aux_bytes == 0): [N x aux_bytes], e.g. the word id and the from-side 3-D point */
    int32_t* out_count;             /* [n_pairs] */
    int32_t* out_index;             /* [N]: the kept inputs in ascending index, the rest of the region -1 */
    float* out_from;                /* [N x 2] */
    float* out_to;                  /* [N x 2] */
    void* out_aux;                  /* [N x aux_bytes], needed with aux */
    float* out_track;               /* may be NULL: [N x 2] by INPUT index */
    uint8_t* out_status;            /* may be NULL: [N] by INPUT index */
    float* out_err;                 /* may be NULL: [N] by INPUT index */
} lcd_track_flow_args;
/* every pointer on the HOST (the images too; every distinct image is staged once); synchronises the engine stream */
int lcd_track_flow(lcd_engine* h, const lcd_track_flow_args* a);
/* the images, points, initial, aux and out_* in DEVICE memory (points, initial, out_from, out_to and out_track 8-byte aligned); offsets,
 * pairs and params on the HOST (read during the call); enqueued on the engine stream, not synchronised */
int lcd_track_flow_dev(lcd_engine* h, const lcd_track_flow_args* a);

/* ---- 3-D to 3-D motion estimation, stateless: the verification behind a loop-closure hypothesis for a caller who holds both frames' word
 * ids and 3-D points in device memory (RegistrationVis.cpp:1823-1871 with Vis/EstimationType = 0).  util3d::estimateMotion3DTo3D
 * (util3d_motion_estimation.cpp:730-807), util3d::findCorrespondences (the map overload, util3d_correspondences.cpp:364-408) behind
 * uMultimapToMapUnique (UStl.h:503-516) and the body of util3d::transformFromXYZCorrespondences (util3d_registration.cpp:63-238) are
 * reproduced exactly, integers and control flow.  What that body calls in PCL (RandomSampleConsensus, SampleConsensusModelRegistration,
 * TransformationEstimationSVD) is not in the reference tree: the sampling, the rigid fit and every summation order are the ENGINE'S, written
 * out here, as the window of lcd_match_guided and the cross-check of lcd_match_pairs are.  No bit parity with a PCL build is claimed.
 * Stateless exactly as lcd_keypoints_3d: the calls borrow the handle's device and stream, read and write nothing of its state, do not complete
 * what a pipelined handle owes, and keep their job table and scratch where lcd_match_pairs keeps its own.  A call serves any number of pairs:
 * pair i owns the rows [from_offsets[i], from_offsets[i+1]) of from_word_ids / from_xyz and [to_offsets[i], to_offsets[i+1]) of the to-arrays.
 *
 * The rule, per pair.  Point arithmetic is fp32, every operation rounded on its own (nothing fused), IEEE division and square root, only
 * + - x / sqrt.  "fp64" marks the few places that are double.
 *   1. Unique ids (UStl.h:503-516).  A row of a frame takes part iff its word id occurs exactly once in that frame.  No sign test.
 *   2. Correspondences (util3d_correspondences.cpp:372-407, maxDepth = 0 at :751).  The participating from-ids that also participate in `to`,
 *      ascending by id as signed integers; an id is kept iff all six coordinates are finite and neither point is (0, 0, 0).  m = the number
 *      kept, `matches` = the kept ids, correspondence j = the j-th of them.  m < min_inliers (:762) or m < 3 (util3d_registration.cpp:82, a
 *      separate guard that also holds for min_inliers < 3): LCD_M3D_FEW_CORRESPONDENCES.
 *   3. Hypotheses.  h = 0 .. iterations - 1 draws three distinct correspondence indices: with uint32 arithmetic and
 *      mix(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16,
 *      draw k = mix(mix(seed + h) * 3 + k) % m for k = 0, 1, ..; a draw equal to an earlier kept one is skipped; a hypothesis without three
 *      distinct indices after 16 draws is invalid and never wins.  Neither the pair's position nor the batch enters.  All hypotheses are
 *      evaluated (no adaptive stop).
 *   4. The rigid fit of an ordered set of n correspondences (from-points p onto to-points q, R p + t ~ q).
 *      Sums: SUM(e_0 .. e_{n-1}) is defined for 256 lanes: lane l starts at +0.0f and adds e_l, e_{l+256}, .. in ascending order; then for
 *      s = 128, 64, .., 1 lane l < s adds lane l + s; the sum is lane 0.  (For n = 3 this is ((0 + e_0) + (0 + e_2)) + (0 + e_1).)
 *      cp_a = SUM(p_a) / float(n), cq_a = SUM(q_a) / float(n) for a = x, y, z; S_ab = SUM((p_a - cp_a) * (q_b - cq_b)) for the nine (a, b).
 *      Horn's matrix, symmetric: N00 = (Sxx + Syy) + Szz, N01 = Syz - Szy, N02 = Szx - Sxz, N03 = Sxy - Syx, N11 = (Sxx - Syy) - Szz,
 *      N12 = Sxy + Syx, N13 = Szx + Sxz, N22 = (Syy - Sxx) - Szz, N23 = Syz + Szy, N33 = (Szz - Sxx) - Syy.
 *      Cyclic Jacobi, V = identity, LCD_M3D_SWEEPS sweeps, each over (p, q) = (0,1) (0,2) (0,3) (1,2) (1,3) (2,3).  A pair with a_pq == 0 is
 *      skipped.  Otherwise theta = (a_qq - a_pp) / (2 * a_pq); t = sgn(theta) / (|theta| + sqrt(theta * theta + 1)) with sgn(theta) = -1 for
 *      theta < 0 and +1 otherwise; a theta (or theta * theta) that overflows to infinity therefore gives t = +-0 and a rotation by nothing.
 *      c = 1 / sqrt(t * t + 1), s = t * c; a_pp -= t * a_pq, a_qq += t * a_pq, a_pq = 0; for the other two r: a_rp' = c * a_rp - s * a_rq,
 *      a_rq' = s * a_rp + c * a_rq (both halves of the matrix kept); for every r: v_rp' = c * v_rp - s * v_rq, v_rq' = s * v_rp + c * v_rq.
 *      The column of V under the largest diagonal entry, the lowest index on ties, is the quaternion (w, x, y, z) after division by
 *      sqrt(((w*w + x*x) + y*y) + z*z).  R00 = 1 - 2 * (yy + zz), R01 = 2 * (xy - wz), R02 = 2 * (xz + wy), R10 = 2 * (xy + wz),
 *      R11 = 1 - 2 * (xx + zz), R12 = 2 * (yz - wx), R20 = 2 * (xz - wy), R21 = 2 * (yz + wx), R22 = 1 - 2 * (xx + yy);
 *      t_r = cq_r - ((R_r0 * cp_x + R_r1 * cp_y) + R_r2 * cp_z).  A hypothesis is the fit of its three correspondences in draw order.
 *   5. Score.  d2 = (dx*dx + dy*dy) + dz*dz with dx = (((R00 * p_x + R01 * p_y) + R02 * p_z) + t_x) - q_x, dy and dz alike.  A correspondence
 *      is an inlier of a model iff double(d2) < thr2, strictly, thr2 = threshold * threshold in fp64.  The best hypothesis has the most
 *      inliers under inlier_distance, the lowest h on ties; no valid hypothesis or a best count of 0: LCD_M3D_NO_MODEL (:228).
 *   6. Selection with the best model under inlier_distance: `inliers`, ascending correspondence index, and their d2 ("the last selection").
 *   7. Refinement, refine_iterations > 0: the loop of util3d_registration.cpp:115-196 as written -- error_threshold starts at inlier_distance;
 *      each pass fits prev_inliers (step 4, in their order; fewer than three leave the model as it is), records their number, selects under
 *      error_threshold; an empty selection counts an iteration and `continue`s into the loop's condition; otherwise variance, then
 *      error_threshold = min(inlier_distance, 3.0 * sqrt(variance)) in fp64, swap, the size test with the oscillation test on the last four
 *      recorded sizes, the element-wise comparison; `while (inlier_changed && ++refine_iterations < refineIterations)`; the final swap makes
 *      the set that was fitted LAST the inliers, and the model is the last fitted one.  computeVariance = 2.1981 * double(median), the median
 *      the element of rank (size >> 1) in ascending order among the d2 of the last selection.
 *   8. Result (:198-222, util3d_motion_estimation.cpp:787-806).  Fewer than 3 inliers: LCD_M3D_FEW_INLIERS.  Otherwise variance =
 *      computeVariance of the last selection, out_inliers = matches[inlier] and out_n_inliers are returned, and the pose is the inverse of
 *      the model: rows of R^T, and -(((R0r * t_x) + (R1r * t_y)) + (R2r * t_z)) behind row r; it is returned iff inliers >= min_inliers
 *      (LCD_M3D_OK), otherwise twelve zeros (LCD_M3D_BELOW_MIN_INLIERS).
 *   9. Twelve zero floats mean no transform (Transform::isNull); then out_status != LCD_M3D_OK.  With LCD_M3D_FEW_CORRESPONDENCES,
 *      LCD_M3D_NO_MODEL and LCD_M3D_FEW_INLIERS out_n_inliers = 0 and out_variance = 1.0; out_matches / out_n_matches are always returned.
 *   A NaN that coordinates near the limits of fp32 may produce inside a fit is no inlier of anything; its sign and payload are not pinned.
 * Outputs: per pair out_transform [12], out_status, out_n_matches, out_n_inliers, out_variance; in the pair's FROM-region of out_matches the
 * ids ascending, of out_inliers the ids in correspondence order, the rest of both regions 0.  Outputs must not overlap inputs.
 *
 * Limits and errors -- after each of them nothing was written and the handle stays usable: more than 8192 rows on a side of a pair,
 * n_pairs > 65535, iterations > 65535 or a handle of a sharded vocabulary: LCD_ERR_UNSUPPORTED; iterations < 1 (the reference's assertion),
 * an inlier_distance that is not finite or <= 0, refine_iterations < 0, min_inliers < 1, n_pairs < 0, offsets that are missing, do not start
 * at 0 or decrease, a NULL pointer where rows or outputs exist, or a wrong struct_size: LCD_ERR_INVALID.  n_pairs == 0 returns LCD_OK.
 * One kernel launch per call whatever the batch: one workgroup of 256 threads per pair. */
#define LCD_M3D_SWEEPS 5
enum lcd_motion_3d_status {
    LCD_M3D_OK = 0,
    LCD_M3D_FEW_CORRESPONDENCES = 1,  /* m < min_inliers, or m < 3 */
    LCD_M3D_NO_MODEL = 2,             /* no hypothesis with an inlier */
    LCD_M3D_FEW_INLIERS = 3,          /* fewer than 3 inliers behind the refinement */
    LCD_M3D_BELOW_MIN_INLIERS = 4     /* inliers and variance returned, no transform */
};
typedef struct lcd_motion_3d_args {
    int32_t struct_size;            /* sizeof(lcd_motion_3d_args) */
    int32_t n_pairs;                /* >= 0; 0 returns LCD_OK */
    int32_t min_inliers;            /* Vis/MinInliers, >= 1 */
    int32_t iterations;             /* Vis/Iterations, 1 .. 65535 */
    int32_t refine_iterations;      /* Vis/RefineIterations, >= 0 */
    uint32_t seed;
    double inlier_distance;         /* Vis/InlierDistance, finite, > 0 */
    const int32_t* from_word_ids;   /* [Nf] */
    const float* from_xyz;          /* [Nf x 3] */
    const int32_t* to_word_ids;     /* [Nt] */
    const float* to_xyz;            /* [Nt x 3] */
    const int64_t* from_offsets;    /* HOST, [n_pairs + 1], non-decreasing, [0] == 0 */
    const int64_t* to_offsets;      /* HOST, [n_pairs + 1] */
    float* out_transform;           /* [n_pairs x 12], row-major 3 x 4 */
    int32_t* out_status;            /* [n_pairs], lcd_motion_3d_status */
    int32_t* out_n_matches;         /* [n_pairs] */
    int32_t* out_n_inliers;         /* [n_pairs] */
    double* out_variance;           /* [n_pairs] */
    int32_t* out_matches;           /* [Nf] */
    int32_t* out_inliers;           /* [Nf] */
} lcd_motion_3d_args;
/* every pointer on the HOST; synchronises the engine stream */
int lcd_estimate_motion_3d(lcd_engine* h, const lcd_motion_3d_args* a);
/* ids, points and out_* in DEVICE memory (4-byte aligned, out_variance 8-byte), the offsets on the HOST (read during the call); enqueued on the
 * engine stream, not synchronised */
int lcd_estimate_motion_3d_dev(lcd_engine* h, const lcd_motion_3d_args* a);

/* ---- 3-D to 2-D motion estimation (PnP), stateless: the same verification under the reference's default, Vis/EstimationType = 1
 * (RegistrationVis.cpp:1676-1819): util3d::estimateMotion3DTo2D (util3d_motion_estimation.cpp:59-289) with util3d::solvePnPRansac (:843-986)
 * and the RANSAC frame of the vendored cv3::solvePnPRansac (corelib/src/opencv/solvepnp.cpp).  What is in the reference tree is reproduced
 * exactly, integers and control flow; what it calls in OpenCV (cv::solvePnP, cv::projectPoints, cv::Rodrigues, cv::RNG, the EPnP kernel) is
 * not in the tree and is the ENGINE'S rule, written out here.  No bit parity with an OpenCV build is claimed.  Stateless exactly as
 * lcd_estimate_motion_3d; pair i owns the rows [from_offsets[i], from_offsets[i+1]) of the from-arrays, [to_offsets[i], to_offsets[i+1]) of
 * the to-arrays, cameras[i] and guesses[12 i .. 12 i + 11].
 *
 * The rule, per pair.  fp32, every operation rounded on its own (nothing fused), IEEE division and square root, only + - x / sqrt; "fp64"
 * marks the few places that are double, and none of them is a division or a square root.  SUM, mix and the three-point rigid fit are those of
 * lcd_estimate_motion_3d (steps 3 and 4 there); T(p) = (((R_r0 p_x + R_r1 p_y) + R_r2 p_z) + t_r) for a row-major 3 x 4 T.
 *   1. Unique ids (RegistrationVis.cpp:1704-1720, uMultimapToMapUnique).  A row takes part iff its id occurs exactly once in its frame.
 *   2. Correspondences (util3d_motion_estimation.cpp:88-116).  The participating TO-ids that also participate in `from`, ascending as signed
 *      integers; kept iff the from-point's three coordinates are finite (no zero test; the to-keypoint is not tested).  m = the number kept.
 *      m < min_inliers (:116), or m < 4: LCD_PNP_FEW_CORRESPONDENCES.
 *   3. Frames (:121, :154).  With has_local_transform, model0 = inverse(guess x local), otherwise inverse(guess); a NULL guess is the identity.
 *      A x B has the entries ((A_r0 B_0c + A_r1 B_1c) + A_r2 B_2c), + A_r3 in the last column; inverse(T) = rows of R^T and
 *      -(((R_0r t_x) + (R_1r t_y)) + (R_2r t_z)).  A model maps from-points into the to-camera.
 *   4. Camera and error.  Pinhole, no distortion.  Under a model, (X, Y, Z) = T(p); u' = fx * (X / Z) + cx, v' = fy * (Y / Z) + cy;
 *      e2 = (u - u')^2 + (v - v')^2, e = sqrt(e2).  A correspondence is an inlier under thr iff Z > 0 and e <= thr (a NaN is no inlier).
 *   5. Thresholds.  thr0 = float(reproj_error) (:853).  RANSAC compares the UNSQUARED e against thrR = float(double(thr0) * double(thr0))
 *      (solvepnp.cpp:245-262); the refinement compares e against error_threshold (:832).
 *   6. Hypothesis h = 0 .. iterations - 1: four distinct indices, draw k = mix(mix(seed + h) * 4 + k) % m, k = 0, 1, .., a draw equal to an
 *      earlier kept one skipped, invalid after 16 draws.  The first three go through P3P, the fourth picks among its solutions.
 *      Bearings b_i = (x, y, 1) / sqrt((x x + y y) + 1) with x = (u - cx) / fx, y = (v - cy) / fy.  cg = b0.b1, cb = b0.b2, ca = b1.b2 (dot =
 *      (x x' + y y') + z z'); c2 = |P1 - P0|^2, b2 = |P2 - P0|^2, a2 = |P2 - P1|^2 ((dx dx + dy dy) + dz dz).  The triple is invalid unless
 *      |(P1 - P0) x (P2 - P0)|^2 > 0 (each component a b - c d, then (x x + y y) + z z).  K = (a2 - c2) / b2, L = c2 / b2.  With the depths
 *      s1, s2 = U s1, s3 = V s1:  U = N(V) / D(V), N = (K - 1) V^2 - 2 (K cb) V + (K + 1), D = -2 ca V + 2 cg, and V is a root of the quartic
 *      Q = (N N + D D) - (2 cg) (N D) - L (W D D), W = V^2 - 2 cb V + 1, the products formed coefficient by coefficient, left to right in
 *      ascending index (rtabmap_amd/csrc/motion_pnp_rule.h p3p() is the normative order).  Polynomials are evaluated by Horner from the
 *      leading coefficient, degree 4 always (absent terms are zero).  Roots are sought in (0, 1] for V, then for 1 / V with the reversed
 *      coefficients: the breakpoints 0 <= k1 <= k2 <= k3 <= 1 are the roots of Q' between the roots of Q'' (closed form, clamped to [0, 1],
 *      a NaN to 0), an absent root replaced by its bracket's right end; a bracket [lo, hi] holds a root iff (Q(lo) < 0) != (Q(hi) < 0), found
 *      by LCD_PNP_BISECT halvings (mid = 0.5 (a + b); the half whose left sign is kept) and then the middle of what is left.  Per root:
 *      U as above, s1 = sqrt(b2 / ((V - 2 cb) V + 1)), s2 = U s1, s3 = V s1; kept iff all three are finite and > 0.  The pose of a depth
 *      triple is the three-point rigid fit of P_i onto s_i b_i.  Among the solutions in the order found the one with the smallest e on the
 *      fourth correspondence wins (strictly smaller replaces), provided Z > 0 there and e is finite; none: the hypothesis is invalid.
 *   7. Candidates.  Candidate 0 is model0, candidate h + 1 is hypothesis h.  Most inliers under thrR wins, the lowest candidate on ties; a
 *      best count of 0: LCD_PNP_NO_MODEL.  All hypotheses are evaluated (no adaptive stop).  The model returned by the RANSAC is the winning
 *      candidate's and its inliers are those under thrR (solvepnp.cpp:164-198: the result of the solvePnP at :180 is overwritten at :196).
 *   8. The fit of an ordered index set from the current model, n >= 4 members (fewer: the model stays as it is, bit for bit).
 *      q = Shepperd's quaternion of R (pivots 1 + tr, 1 + ((R00 - R11) - R22), 1 + ((R11 - R00) - R22), 1 + ((R22 - R00) - R11); the
 *      largest, the lowest index on ties), t as it is.  LCD_PNP_STEPS times: R = rotation of q / |q| (step 4 of lcd_estimate_motion_3d);
 *      per member M = R p, (X, Y, Z) = M + t, iz = 1 / Z, x = X iz, y = Y iz, a = fx iz, c = fy iz, Ju = (-(a x) My, a Mz + (a x) Mx,
 *      -(a My), a, 0, -(a x)), Jv = (-(c Mz + (c y) My), (c y) Mx, c Mx, 0, c, -(c y)), r = (u - (fx x + cx), v - (fy y + cy)); the 21 sums
 *      SUM(Ju_i Ju_j + Jv_i Jv_j), i <= j, and the 6 sums SUM(Ju_i r_u + Jv_i r_v); a member with Z <= 0 adds +0 everywhere.  The 6 x 6 system by
 *      LDL^T without pivoting, columns in order, each inner product subtracted term by term in ascending index; a pivot that is not positive
 *      and finite, or a solution that is not finite, leaves the pose as it was for that step.  Otherwise q <- (1, w / 2) (x) q (Hamilton
 *      product, terms in the order x, y, z of w), t <- t + dt.  After the last step the model is [R(q / |q|) | t].
 *   9. Refinement (util3d_motion_estimation.cpp:880-984), entered iff inliers >= minInliersCount = max(4, min_inliers) (:859) and
 *      refine_iterations > 0: as written -- each pass fits prev_inliers (step 8), records their number, selects under error_threshold (:832);
 *      fewer than minInliersCount selected counts an iteration and `continue`s into the loop's condition; otherwise uMean and uVariance
 *      (UMath.h:399-411, 489-502: a float accumulator from the first error to the last, / float(size), / float(size - 1)) over the NEW inliers'
 *      errors, error_threshold = min(thr0, 3.0f * sqrt(variance)), swap, the size test with the oscillation test guarded by
 *      inliers_sizes.size() >= minInliersCount (:944), the element-wise comparison, `while (inlier_changed && ++refine_iterations <
 *      refineIterations)`; the final swap (:981), and the model is the last fitted one.
 *  10. Result.  inliers < min_inliers (:147): LCD_PNP_BELOW_MIN_INLIERS, the inliers returned, no transform.  Otherwise transform =
 *      inverse(local x model) (inverse(model) without a local transform) and the covariance inputs (:156-271):
 *      kind 1, when to_xyz is given or the camera has an image size: per inlier newPt = transform(to-point) when the to-row has three finite
 *      coordinates, otherwise inverse(model) applied to float(double(ray) * (double(Z) * 1.1)) with Z of model(p) and ray = ((u - cx') / fx,
 *      (v - cy') / fy, 1), cx' = cx > 0 ? cx : float(width / 2) - 0.5f, cy' alike (util3d.cpp:246-264).  (The reference's products transform x
 *      local and their inverses are taken as inverse(model) and model.)  d2 = |p - newPt|^2; cosine = (p . newPt) / (|p| |newPt|), clamped
 *      to [-1, 1], +1 where the product of the lengths is not > 0 or the quotient is a NaN.  With k = inliers / variance_median_ratio:
 *      out_variance_lin = 2.1981 * double(the d2 of rank k ascending); out_angle_cos = the cosine of rank inliers - 1 - k ascending, whose
 *      arc cosine is the angle of rank k (acos decreases); the angular variance is 2.1981 * acos(out_angle_cos), the caller's.  max_variance
 *      > 0 and out_variance_lin > max_variance: LCD_PNP_VARIANCE_REJECTED, no transform, the covariance reset (kind 0).
 *      kind 2, otherwise: out_variance_lin = sqrt(err / float(inliers)), err the float sum of e2 over the inliers in their order (:264-270).
 *  11. Twelve zero floats mean no transform; then out_status != LCD_PNP_OK, out_variance_lin = out_angle_cos = 1.0 and out_variance_kind = 0.
 * Outputs: in the pair's TO-region of out_matches the ids ascending, of out_inliers the ids in correspondence order, the rest of both 0.
 * Out of scope: lens distortion (the struct carries no D; the registration's images are rectified), the multi-camera overload (OpenGV),
 * splitLinearCovarianceComponents and to3DoF.  The bundle adjustment behind this step is lcd_refine_motion_ba, below.
 *
 * Limits and errors -- after each of them nothing was written and the handle stays usable: more than 8192 rows on a side of a pair,
 * n_pairs > 65535, iterations > 65535 or a handle of a sharded vocabulary: LCD_ERR_UNSUPPORTED; iterations < 1, a reproj_error that is not
 * finite or whose float (or its square) is not finite and > 0, refine_iterations < 0, min_inliers < 1, variance_median_ratio <= 1,
 * a max_variance that is negative or not finite, n_pairs < 0, offsets that are missing, do not start at 0 or decrease, NULL cameras, a camera
 * whose fx or fy is not finite or is 0, a NULL pointer where rows or outputs exist (to_xyz and guesses may be NULL), or a wrong struct_size:
 * LCD_ERR_INVALID.  n_pairs == 0 returns LCD_OK.  One kernel launch per call whatever the batch: one workgroup of 256 threads per pair. */
#define LCD_PNP_STEPS 8
#define LCD_PNP_BISECT 26
enum lcd_motion_pnp_status {
    LCD_PNP_OK = 0,
    LCD_PNP_FEW_CORRESPONDENCES = 1,  /* m < min_inliers, or m < 4 */
    LCD_PNP_NO_MODEL = 2,             /* no candidate with an inlier */
    LCD_PNP_BELOW_MIN_INLIERS = 3,    /* inliers returned, no transform */
    LCD_PNP_VARIANCE_REJECTED = 4     /* inliers returned, the linear variance above max_variance, no transform */
};
typedef struct lcd_motion_pnp_args {
    int32_t struct_size;            /* sizeof(lcd_motion_pnp_args) */
    int32_t n_pairs;                /* >= 0; 0 returns LCD_OK */
    int32_t min_inliers;            /* Vis/MinInliers, >= 1 */
    int32_t iterations;             /* Vis/Iterations, 1 .. 65535 */
    int32_t refine_iterations;      /* Vis/PnPRefineIterations, >= 0 */
    int32_t variance_median_ratio;  /* Vis/PnPVarianceMedianRatio, > 1 */
    uint32_t seed;
    float max_variance;             /* Vis/PnPMaxVariance, 0 = off */
    double reproj_error;            /* Vis/PnPReprojError, finite, > 0 */
    const int32_t* from_word_ids;   /* [Nf] */
    const float* from_xyz;          /* [Nf x 3] */
    const int32_t* to_word_ids;     /* [Nt] */
    const float* to_points;         /* [Nt x 2] cv::KeyPoint::pt, the layout lcd_keypoints_3d writes as out_points */
    const float* to_xyz;            /* [Nt x 3]; may be NULL */
    const int64_t* from_offsets;    /* HOST, [n_pairs + 1], non-decreasing, [0] == 0 */
    const int64_t* to_offsets;      /* HOST, [n_pairs + 1] */
    const lcd_camera* cameras;      /* HOST, [n_pairs]; image_width / image_height decide the covariance branch */
    const float* guesses;           /* HOST, [n_pairs x 12]; NULL = identity */
    float* out_transform;           /* [n_pairs x 12], row-major 3 x 4 */
    int32_t* out_status;            /* [n_pairs], lcd_motion_pnp_status */
    int32_t* out_n_matches;         /* [n_pairs] */
    int32_t* out_n_inliers;         /* [n_pairs] */
    double* out_variance_lin;       /* [n_pairs] */
    double* out_angle_cos;          /* [n_pairs] */
    int32_t* out_variance_kind;     /* [n_pairs]: 0 none, 1 linear + cosine, 2 RMS reprojection in out_variance_lin */
    int32_t* out_matches;           /* [Nt] */
    int32_t* out_inliers;           /* [Nt] */
} lcd_motion_pnp_args;
/* every pointer on the HOST; synchronises the engine stream */
int lcd_estimate_motion_pnp(lcd_engine* h, const lcd_motion_pnp_args* a);
/* ids, points and out_* in DEVICE memory (4-byte aligned, the doubles 8-byte), offsets, cameras and guesses on the HOST (read during the
 * call); enqueued on the engine stream, not synchronised */
int lcd_estimate_motion_pnp_dev(lcd_engine* h, const lcd_motion_pnp_args* a);

/* ---- Two-view bundle adjustment, stateless: the link of RegistrationVis::computeTransformationImpl between the PnP and the ICP
 * (RegistrationVis.cpp:1873-2188 with Vis/BundleAdjustment = 1, the reference's default): the transform of lcd_estimate_motion_pnp (or
 * lcd_estimate_motion_3d) is refined over its inliers by OptimizerG2O::optimizeBA (OptimizerG2O.cpp:1429-2117) with root 1 and one neighbour
 * link, the inliers the adjustment marks as outliers are dropped, Vis/MinInliers is tested again, and the gates Vis/MeanInliersDistance and
 * Vis/MinInliersDistribution decide.  What is in the reference tree is reproduced as written; what it calls in g2o (the projections, the
 * camera edge's error, the robust kernel, Levenberg-Marquardt and its linear solver) and in OpenCV (cv::PCA) is not in the tree and is the
 * ENGINE'S rule, written out here.  No parity with a g2o build is claimed.  Stateless exactly as lcd_estimate_motion_pnp; pair i owns the
 * rows [from_offsets[i], from_offsets[i+1]) of the from-arrays, [to_offsets[i], to_offsets[i+1]) of the to-arrays, of `inliers` and of
 * out_inliers, cameras_from[i], cameras_to[i], transforms[12 i ..], n_inliers[i], prior_variance[2 i ..] and baselines[2 i ..].
 *
 * The rule, per pair.  fp32, every operation rounded on its own, IEEE division and square root, only + - x / sqrt; "fp64" marks what is
 * double.  T(p), A x B, inverse(T), the quaternion of a rotation, the rotation of a quaternion, the pose update and the 6 x 6 LDL^T are those
 * of lcd_estimate_motion_pnp (its preamble and steps 3, 7, 8).  SUM is the sum of lcd_estimate_motion_3d (step 4 there: 256 lane partials in
 * ascending order from +0, then the halving tree); SUM64 the same in fp64.
 *   1. Input.  n = n_inliers[i].  Twelve zero floats in transforms[12 i ..] or n == 0: LCD_BA_NO_INPUT, out_inliers = the first max(n, 0)
 *      ids of `inliers` as they are (at most the pair's to-rows), out_n_inliers = their number, everything else 0.  n < 0, n above the pair's to-rows, an id among the first n that does
 *      not occur exactly once in the from-frame and exactly once in the to-frame, or a from-point with a coordinate that is not finite (the
 *      reference asserts): LCD_BA_BAD_INLIER, nothing is refined, outputs as for LCD_BA_NO_INPUT.  lcd_estimate_motion_pnp produces neither.
 *      Repeats WITHIN the list are not checked: an id given twice makes two points with the same observations (the reference's map would
 *      keep one); lcd_estimate_motion_pnp's list has none.
 *   2. Graph (:1885-2027).  Pose 1 is the identity and fixed, pose 2 the transform T; the cameras' poses are C1 = local_from, C2 = T x
 *      local_to (a camera without local transform: the identity).  The engine holds a camera as the model M = inverse(C) that maps points
 *      into it: M1 = inverse(local_from), M2 = inverse(T x local_to).  Point k is inlier k's from-point P0_k.  Its observations:
 *      from-side, only with from_points: depth = z of M1(P0_k), keypoint (u, v) of the from-row; to-side: depth = z of
 *      inverse(local_to)(to-point), 0 without to_xyz, keypoint of the to-row.  An edge is stereo iff its depth is finite and > 0 and the
 *      camera's baseline b (fp64) is > 0 (OptimizerG2O.cpp:1862); then obs = (u, v, u - float(b x double(fx) / double(depth))) (fp64,
 *      :1880); otherwise mono, obs = (u, v).  Information I / pixel_variance: info = float(1 / pixel_variance).  One camera-to-camera edge
 *      with measurement inverse(C1) x T x local_to, information diag(inf_lin x 3, inf_ang x 3) with inf = float(1 / max(variance, floor)),
 *      floors 1e-8 and 3e-8 (Registration.cpp:36-37); 1 and 1 without prior_variance (Optimizer/VarianceIgnored).
 *   3. Projection and chi2 (engine).  Under a model M: (Mx, My, Mz) = R p, (X, Y, Z) = that + t, iz = 1 / Z, x = X iz, y = Y iz,
 *      projection (fx x + cx, fy y + cy, fx ((X - float(b)) iz) + cx); r = obs - projection; chi2 = info x ((ru ru + rv rv) + rd rd), the
 *      last term only for a stereo edge.  Nothing is special about Z <= 0.
 *   4. Robust kernel (engine): Huber as IRLS.  delta = float(robust_delta), delta2 = delta x delta.  For chi2 <= delta2 (or delta == 0) the
 *      weight is 1 and the cost chi2; otherwise the weight is delta / sqrt(chi2) and the cost (2 delta) sqrt(chi2) - delta2.  No second-order
 *      term.
 *   5. Camera edge (engine).  E = M2 x C2_0, C2_0 = T x local_to as given.  Error e = (translation of E, 2 (x, y, z) of E's quaternion
 *      divided by its norm, negated when w < 0).  Cost inf_lin x ((e0 e0 + e1 e1) + e2 e2) + inf_ang x ((e3 e3 + e4 e4) + e5 e5).  Jacobian
 *      with respect to (w, dt) of step 8's update: rows 0-2 (-[R t0]x | I), rows 3-5 (w_E I - [v_E]x | 0), R t0 = R applied to C2_0's
 *      translation.  Its 21 + 6 entries: per entry the six rows in order, (J_ki J_kj) x inf_k, added from +0; the right-hand side subtracts
 *      (J_ki e_k) x inf_k.
 *   6. Cost.  F = SUM64 over the points of (double(cost of the from-edge) + double(cost of the to-edge)), active edges only, then
 *      + double(the camera edge's cost).
 *   7. Normal equations (engine), per point with an active edge, under the current M2 and point: per active edge W = info x weight; rows
 *      g = (a, 0, -(a x)), (0, c, -(c y)), (a, 0, -(a xb)) with a = fx iz, c = fy iz, xb = (X - b) iz; point Jacobian Jp_k = g_k R (each entry
 *      a product minus a product), camera Jacobian of the to-edge as lcd_estimate_motion_pnp's step 8 with the third row (-(a xb) My,
 *      a Mz + (a xb) Mx, -(a My), a, 0, -(a xb)).  Every entry of the 3 x 3 block Hpp, the gradient bp, the 6 x 3 coupling Hcp, the camera
 *      block Hcc and gradient bc is, per edge, ((J_0 J'_0 + J_1 J'_1) + J_2 J'_2) x W added to the entry, the from-edge first.
 *      Levenberg-Marquardt on the Schur complement: inverse of (Hpp + lambda I) by cofactors over the determinant, Y = Hcp inverse, the
 *      point's 27 terms Hcc_ij - ((Y_i0 Hcp_j0 + Y_i1 Hcp_j1) + Y_i2 Hcp_j2) and bc_i - (Y_i . bp); their SUM over the points; plus the
 *      camera edge's entries; lambda added to the six diagonal entries; the LDL^T.  Back-substitution per point: dp = inverse (bp - Hcp^T
 *      dc), the inner products in ascending index.  p <- p + dp; the pose update of lcd_estimate_motion_pnp's step 8 (q <- (1, w / 2) (x) q,
 *      t <- t + dt), M2 = [R(q / |q|) | t].
 *   8. Nielsen's schedule (engine).  At the start of a stage lambda = 1e-5f x the largest of: every point's three Hpp diagonal entries, and
 *      the six SUMs of the Hcc diagonal entries plus the camera edge's; nu = 2.  Per iteration up to 10 trials: solve with lambda (no
 *      solution counts as a rejected trial); F' = the cost of the moved state; scale = SUM64 over the points of (sum_a dp_a (lambda dp_a +
 *      bp_a) + sum_i dc_i bc_i) + sum_i dc_i (lambda dc_i + the camera edge's right-hand side i), fp64; rho = (F - F') / (scale + 1e-3),
 *      fp64.  Accepted iff rho > 0 and F' is finite: F = F', lambda = float(double(lambda) x max(1/3, 1 - (2 rho - 1)^3)), nu = 2.
 *      Otherwise the state is restored, lambda <- lambda nu, nu <- 2 nu.  Ten rejected trials end the stage.
 *   9. Stages and outliers (OptimizerG2O.cpp:1946-2027).  robust_delta > 0: two stages, 5 iterations, then `iterations`; otherwise one stage
 *      of `iterations`.  After each stage: F is NaN: LCD_BA_DIVERGED (:1954); after the second, F > 1e12 or not finite: LCD_BA_DIVERGED
 *      (:1962); otherwise, with a kernel, every active edge whose UN-ROBUSTIFIED chi2 is > delta -- delta, not delta2, as written at :1972 --
 *      leaves (level 1), its point goes back to P0_k and is an outlier (both edges are tested on the chi2 they had before either reset).  The
 *      second stage starts from the cost of what is left.  After the last stage F > 1e12: LCD_BA_DIVERGED (:2023).  out_chi2_before is the
 *      first F, out_chi2_after the last.  LCD_BA_DIVERGED: no transform, the inliers as they came.
 *  10. Result (RegistrationVis.cpp:2033-2063).  out_inliers = the ids whose point is no outlier, in input order; fewer than min_inliers:
 *      LCD_BA_BELOW_MIN_INLIERS, no transform.  Otherwise transform = inverse(local_to x M2) (:2049), inverse(M2) without local transform.
 *      iterations == 0: no adjustment; out_transform is the input, bit for bit, and the gates below decide.
 *  11. Gates (:2090-2188), with a transform and at least one inlier.  max_inliers_mean_distance > 0 and to_xyz given: the depths z of
 *      inverse(local_to)(to-point) of the surviving inliers whose to-point has three finite coordinates, in inlier order; uMean (UMath.h:
 *      a float accumulator from the first to the last, / float(count)); none: no test.  mean > max: LCD_BA_MEAN_DISTANCE_REJECTED.
 *      min_inliers_distribution > 0 and the to-camera has fx, fy, cx, cy > 0 and an image size (isValidForReprojection): x = float((double(u)
 *      - double(cx)) / double(width)), y alike with cy and height (:2154-2155, fp64); mean = SUM / float(n); covariance entries SUM of the
 *      products of the centred coordinates / float(n); out_inliers_distribution = the smaller eigenvalue (a + c) / 2 - sqrt(((a - c) / 2)^2 +
 *      b b); below the threshold: LCD_BA_DISTRIBUTION_REJECTED.  A rejected pair has no transform; its inliers and figures stay.
 * Precision: the 27 sums and the 6 x 6 solve are fp32, as lcd_estimate_motion_pnp's and lcd_register_icp_plane's.
 * Out of scope: multi-camera rigs (cameraIndex is 0), Reg/Force3DoF (the plane prior) and gravity links, cvsba and Ceres
 * (Vis/BundleAdjustment 2 and 3), full 6 x 6 priors, handing back the refined points (the reference discards them too), lens distortion,
 * the epipolar estimation type (Vis/EstimationType = 2 is lcd_estimate_motion_mono, below, which the reference does not adjust either).
 *
 * Limits and errors -- after each of them nothing was written and the handle stays usable: more than 8192 rows on a side of a pair,
 * n_pairs > 65535, iterations > 65535 or a handle of a sharded vocabulary: LCD_ERR_UNSUPPORTED; iterations < 0, min_inliers < 0, a pixel_variance that is not
 * finite and > 0 (itself and float(1 / it)), a robust_delta, gate or prior variance that is negative or not finite (float(robust_delta)
 * squared too), a baseline that is not finite, n_pairs < 0, offsets that are missing, do not start at 0 or decrease, NULL cameras, a camera
 * whose fx or fy is not finite or is 0, a NULL pointer where rows, pairs or outputs exist (from_points, to_xyz, prior_variance and baselines
 * may be NULL), or a wrong struct_size: LCD_ERR_INVALID.  n_pairs == 0 returns LCD_OK.  One kernel launch per call whatever the batch: one
 * workgroup of 256 threads per pair.  out_inliers must not overlap `inliers`. */
enum lcd_motion_ba_status {
    LCD_BA_OK = 0,
    LCD_BA_NO_INPUT = 1,              /* no transform came in, or no inliers: passed through */
    LCD_BA_BAD_INLIER = 2,            /* an inlier id that is not unique in both frames, or a count outside the region */
    LCD_BA_DIVERGED = 3,              /* the cost is NaN or above 1e12: no transform, the inliers as they came */
    LCD_BA_BELOW_MIN_INLIERS = 4,     /* survivors returned, no transform */
    LCD_BA_MEAN_DISTANCE_REJECTED = 5,
    LCD_BA_DISTRIBUTION_REJECTED = 6
};
typedef struct lcd_motion_ba_args {
    int32_t struct_size;            /* sizeof(lcd_motion_ba_args) */
    int32_t n_pairs;                /* >= 0; 0 returns LCD_OK */
    int32_t min_inliers;            /* Vis/MinInliers, >= 0 */
    int32_t iterations;             /* Optimizer/Iterations, 0 .. 65535; 0 = no adjustment, gates only */
    double pixel_variance;          /* g2o/PixelVariance, finite, > 0 */
    double robust_delta;            /* g2o/RobustKernelDelta, finite, >= 0; 0 = no kernel, one stage */
    double default_baseline;        /* g2o/Baseline, finite; used where baselines is NULL */
    float max_inliers_mean_distance;   /* Vis/MeanInliersDistance, 0 = off */
    float min_inliers_distribution;    /* Vis/MinInliersDistribution, 0 = off */
    const int32_t* from_word_ids;   /* [Nf] */
    const float* from_xyz;          /* [Nf x 3] */
    const float* from_points;       /* [Nf x 2] the from keypoints; NULL = none (the reference's empty getWordsKpts()) */
    const int32_t* to_word_ids;     /* [Nt] */
    const float* to_points;         /* [Nt x 2] */
    const float* to_xyz;            /* [Nt x 3]; may be NULL */
    const int32_t* inliers;         /* [Nt]: lcd_estimate_motion_pnp's out_inliers */
    const int32_t* n_inliers;       /* [n_pairs]: its out_n_inliers */
    const float* transforms;        /* [n_pairs x 12]: its out_transform */
    const double* prior_variance;   /* HOST, [n_pairs x 2] linear, angular; NULL = identity information */
    const int64_t* from_offsets;    /* HOST, [n_pairs + 1], non-decreasing, [0] == 0 */
    const int64_t* to_offsets;      /* HOST, [n_pairs + 1] */
    const lcd_camera* cameras_from; /* HOST, [n_pairs] */
    const lcd_camera* cameras_to;   /* HOST, [n_pairs] */
    const double* baselines;        /* HOST, [n_pairs x 2] from, to; NULL = default_baseline; <= 0: mono edges only */
    float* out_transform;           /* [n_pairs x 12]; twelve zeros = rejected */
    int32_t* out_status;            /* [n_pairs], lcd_motion_ba_status */
    int32_t* out_inliers;           /* [Nt]: the surviving ids in input order, zeros behind them */
    int32_t* out_n_inliers;         /* [n_pairs] */
    int32_t* out_n_outliers;        /* [n_pairs] */
    double* out_chi2_before;        /* [n_pairs] the robust cost before the first stage */
    double* out_chi2_after;         /* [n_pairs] and behind the last */
    int32_t* out_lm_accepted;       /* [n_pairs] accepted Levenberg-Marquardt steps */
    float* out_inliers_mean_distance;   /* [n_pairs]; 0 when the gate is off or has nothing to test */
    float* out_inliers_distribution;    /* [n_pairs]; 0 when the gate is off */
} lcd_motion_ba_args;
/* every pointer on the HOST; synchronises the engine stream */
int lcd_refine_motion_ba(lcd_engine* h, const lcd_motion_ba_args* a);
/* ids, points, inliers, n_inliers, transforms and out_* in DEVICE memory (4-byte aligned, the doubles 8-byte): the PnP's outputs go in with
 * nothing read back; offsets, cameras, prior_variance and baselines on the HOST (read during the call); enqueued on the engine stream, not
 * synchronised */
int lcd_refine_motion_ba_dev(lcd_engine* h, const lcd_motion_ba_args* a);

/* ---- Epipolar hypothesis check, stateless: the one geometric verification of the appearance-only mode, EpipolarGeometry::check
 * (EpipolarGeometry.cpp:65-102, :298-379) as Rtabmap::process calls it under VhEp/Enabled (Rtabmap.cpp:2193): the unique word pairs of two
 * signatures, a fundamental matrix by RANSAC over their keypoints, accepted with at least VhEp/MatchCountMin inliers.  What is in the
 * reference tree is reproduced exactly: the pairing, the thresholds, the accept rule, the parameter meanings, and "more than 7" of
 * util3d::extractXYZCorrespondencesRANSAC (util3d_correspondences.cpp:85).  cv::findFundamentalMat is not in the tree: the estimator is the
 * ENGINE'S rule, written out here.  No parity with an OpenCV build is claimed.  Stateless exactly as lcd_estimate_motion_pnp; pair i owns the
 * rows [from_offsets[i], from_offsets[i+1]) of the from-arrays and [to_offsets[i], to_offsets[i+1]) of the to-arrays.
 *
 * The rule, per pair.  fp32, every operation rounded on its own (nothing fused), IEEE division and square root, only + - x / sqrt.  SUM and
 * mix are those of lcd_estimate_motion_3d (steps 3 and 4 there).  rtabmap_amd/csrc/epipolar_rule.h is the normative order of operations.
 *   1. Pairs (EpipolarGeometry.h:158-186, findPairsUnique with ignoreNegativeIds).  A word id takes part iff it is >= 0 and occurs exactly
 *      once in `from` and exactly once in `to`; the correspondences in ascending id, m their number.  Keypoints are not tested for
 *      finiteness here; a NaN is never an inlier later.  m < match_count_min (:77), or m < 8: LCD_EPI_FEW_PAIRS, nothing is estimated.
 *      (OpenCV with exactly seven points runs its solver once; with the default VhEp/MatchCountMin = 8 the two never differ.)
 *   2. Normalisation, once per pair over all m correspondences, per image: centroid (cx, cy) = (SUM(u), SUM(v)) / float(m); d = SUM(sqrt((u -
 *      cx)^2 + (v - cy)^2)) / float(m); s = 1.41421356f / d; T = [s 0 -(s cx); 0 s -(s cy); 0 0 1]; a normalised coordinate is (s u) + T_02.
 *      A d that is 0 or not finite in either image: LCD_EPI_NO_MODEL.
 *   3. Hypothesis h = 0 .. iterations - 1: seven distinct indices, draw k = mix(mix(seed + h) * 8 + k) % m, k = 0, 1, .., a draw equal to an
 *      earlier kept one skipped, invalid after 32 draws.  The 7 x 9 matrix has the rows (x'x, x'y, x', y'x, y'y, y', x, y, 1) in normalised
 *      coordinates, x of `from`, x' of `to`.  Gauss-Jordan elimination with complete pivoting: in step k the pivot is the entry of largest
 *      magnitude in rows k .., columns k .. (the lowest row, then the lowest column on ties; a NaN is never chosen); row and column are
 *      exchanged with row and column k; a pivot that is 0 or not finite makes the sample invalid; the pivot row's entries behind the pivot
 *      are divided by it, and every other row r gets A_rc - (A_rk A_kc), element by element.  The two null vectors F1 and F2 have the free
 *      columns set to (1, 0) and (0, 1), the others the negated entries of the two remaining columns, put back into the columns' own order.
 *      det(x F1 + F2) = c3 x^3 + c2 x^2 + c1 x + c0 from four determinants: c0 = det F2, c3 = det F1, c2 = 0.5 (det(F1 + F2) + det(F2 -
 *      F1)) - c0, c1 = 0.5 (det(F1 + F2) - det(F2 - F1)) - c3; det M = ((M0 (M4 M8 - M5 M7)) - (M1 (M3 M8 - M5 M6))) + (M2 (M3 M7 - M4 M6)).
 *      c3 == 0 or a coefficient that is not finite: invalid.  Real roots as lcd_estimate_motion_pnp finds its quartic's: B = 1 + max |c_i /
 *      c3| (not finite: invalid); the breakpoints k1 <= k2 are the closed-form roots of the derivative when its discriminant (2 c2)^2 - 4 ((3
 *      c3) c1) is > 0, clamped to [-B, B] (a NaN to B), otherwise both are B; the brackets [-B, k1], [k1, k2], [k2, B]; a bracket holds a
 *      root iff (p(lo) < 0) != (p(hi) < 0) (Horner from c3), found by LCD_EPI_BISECT halvings and then the middle of what is left.
 *      Candidate c = 3 h + r is the r-th root found, in the brackets' order, with F^ = (x F1) + F2; an absent root: an invalid candidate.
 *      F = T'^T (F^ T): first G = F^ T with G_r2 = ((F^_r0 T_02) + (F^_r1 T_12)) + F^_r2, then T'^T G alike.
 *   4. Error and inlier.  l' = F (u, v, 1), l = F^T (u', v', 1), each component ((a u) + (b v)) + c; e = max((p'.l')^2 / (l'_x^2 + l'_y^2),
 *      (p.l)^2 / (l_x^2 + l_y^2)); an inlier iff both quotients are <= float(thr) * float(thr) (a NaN is no inlier).  thr is
 *      VhEp/RansacParam1, in pixels.
 *   5. Winner.  The candidate with most inliers wins, the lowest candidate on ties.  All candidates are scored: there is no adaptive stop,
 *      so VhEp/RansacParam2 (the confidence) has no effect on the device; the host mirror keeps the parameter and passes iterations = 1000,
 *      OpenCV's cap for this method.  A best count of 0: LCD_EPI_NO_MODEL.  As in current OpenCV the winning sample's matrix is the result;
 *      there is no refit over the inliers.
 *   6. Result.  inliers >= match_count_min: LCD_EPI_OK, otherwise LCD_EPI_FEW_INLIERS (:91-96).  In the pair's TO-region of out_matches the
 *      ids of all pairs ascending, of out_inliers the inliers' ids in correspondence order, the rest of both 0.  out_fundamental: the
 *      winner's F divided by its Frobenius norm (the squares added in index order), negated when its largest-magnitude entry (the lowest
 *      index on ties) is negative; nine zeros mean no model.
 * Out of scope: findEpipolesFromF, findPFromE and the triangulations, LMedS, lens distortion, sharded handles.  (Vis/EstimationType = 2,
 * util3d::generateWords3DMono, is lcd_estimate_motion_mono, below: its five-point solver is built from the constraints themselves, not from
 * the generated coefficient matrix of the reference tree.)
 *
 * Limits and errors -- after each of them nothing was written and the handle stays usable: more than 8192 rows on a side of a pair,
 * n_pairs > 65535, iterations > 65535 or a handle of a sharded vocabulary: LCD_ERR_UNSUPPORTED; iterations < 1, a ransac_threshold whose
 * float or its square is not finite and > 0, match_count_min < 1, n_pairs < 0, offsets that are missing, do not start at 0 or decrease, a
 * NULL pointer where rows or outputs exist (out_fundamental, out_matches and out_inliers may be NULL), or a wrong struct_size:
 * LCD_ERR_INVALID.  n_pairs == 0 returns LCD_OK.  One kernel launch per call whatever the batch: one workgroup of 256 threads per pair. */
#define LCD_EPI_BISECT 26
enum lcd_epipolar_status {
    LCD_EPI_OK = 0,
    LCD_EPI_FEW_PAIRS = 1,            /* m < match_count_min, or m < 8 */
    LCD_EPI_NO_MODEL = 2,             /* a degenerate normalisation, or no candidate with an inlier */
    LCD_EPI_FEW_INLIERS = 3           /* inliers and matrix returned, fewer than match_count_min */
};
typedef struct lcd_epipolar_args {
    int32_t struct_size;            /* sizeof(lcd_epipolar_args) */
    int32_t n_pairs;                /* >= 0; 0 returns LCD_OK */
    int32_t match_count_min;        /* VhEp/MatchCountMin, >= 1 */
    int32_t iterations;             /* 1 .. 65535 */
    uint32_t seed;
    double ransac_threshold;        /* VhEp/RansacParam1, pixels, finite, > 0 */
    const int32_t* from_word_ids;   /* [Nf] */
    const float* from_points;       /* [Nf x 2] cv::KeyPoint::pt, the layout lcd_keypoints_3d writes as out_points */
    const int32_t* to_word_ids;     /* [Nt] */
    const float* to_points;         /* [Nt x 2] */
    const int64_t* from_offsets;    /* HOST, [n_pairs + 1], non-decreasing, [0] == 0 */
    const int64_t* to_offsets;      /* HOST, [n_pairs + 1] */
    float* out_fundamental;         /* [n_pairs x 9], row-major; may be NULL */
    int32_t* out_status;            /* [n_pairs], lcd_epipolar_status */
    int32_t* out_n_pairs;           /* [n_pairs] */
    int32_t* out_n_inliers;         /* [n_pairs] */
    int32_t* out_matches;           /* [Nt]; may be NULL */
    int32_t* out_inliers;           /* [Nt]; may be NULL */
} lcd_epipolar_args;
/* every pointer on the HOST; synchronises the engine stream */
int lcd_verify_epipolar(lcd_engine* h, const lcd_epipolar_args* a);
/* ids, points and out_* in DEVICE memory (4-byte aligned), the offsets on the HOST (read during the call): the outputs of
 * lcd_select_features / lcd_keypoints_3d go in where they lie; enqueued on the engine stream, not synchronised */
int lcd_verify_epipolar_dev(lcd_engine* h, const lcd_epipolar_args* a);

/* ---- Monocular motion estimation, stateless: the last estimation type of RegistrationVis, Vis/EstimationType = 2
 * (RegistrationVis.cpp:1584-1675), util3d::generateWords3DMono (util3d_features.cpp:209-413): the unique word pairs of two monocular
 * signatures, an essential matrix by five-point RANSAC over their keypoints, recoverPose's choice among the four decompositions, one
 * triangulated point per inlier, and the scale and variance from the from-signature's words3 or from a guess.  What is in the reference
 * tree is reproduced exactly, integers and control flow: the pairing, the "> 8" gate, the normalisation and the threshold of
 * cv3::findEssentialMat (five-point.cpp:430-439), the error of computeError (:375-401), recoverPose's four configurations, its mask tests
 * and its >= cascade (:527-642), cameraTransform = local x inverse([R | t]) x inverse(local) (util3d_features.cpp:277-282), the scale and
 * variance block (:304-408) and the two gates of RegistrationVis.cpp:1636-1667.  The SVDs, solvePoly, cv::triangulatePoints and the RANSAC
 * driver are OpenCV's and not in the tree; the five-point solver of the tree (corelib/src/opencv/five-point.cpp) is a generated coefficient
 * table and is not taken over.  In their place stands the ENGINE'S rule, written out here; no parity with an OpenCV build is claimed.
 * Stateless exactly as lcd_estimate_motion_pnp; pair i owns the rows [from_offsets[i], from_offsets[i+1]) of the from-arrays and
 * [to_offsets[i], to_offsets[i+1]) of the to-arrays.
 *
 * The rule, per pair.  Every operation rounded on its own (nothing fused), IEEE division and square root, only + - x / sqrt.  fp64: the
 * solver (step 3), the decomposition (5) and the triangulation (6).  fp32: the normalised coordinates (2), the scoring (4) and everything
 * from the triangulated point on (7, 8).  mix is that of lcd_estimate_motion_3d (step 3 there); invert, A x B and T(p) are those of
 * lcd_estimate_motion_pnp.  rtabmap_amd/csrc/motion_mono_rule.h is the normative order of operations.
 *   1. Gates and pairs.  Either frame with fewer rows than min_inliers: LCD_MONO_FEW_FEATURES (:1594), nothing else is looked at.  A word id
 *      takes part iff it is >= 0 and occurs exactly once in `from` and exactly once in `to` (uMultimapToMapUnique, then
 *      EpipolarGeometry::findPairs); the correspondences in ascending id, m their number.  m < 9 ("pairsFound > 8"): LCD_MONO_FEW_PAIRS.
 *   2. Normalisation.  x = (u - cx) / fx, y = (v - cy) / fy as floats, once per pair.  thr2 = float(t t), t = reproj_threshold / ((double(fx)
 *      + double(fy)) / 2) in double.
 *   3. Hypothesis h = 0 .. iterations - 1: five distinct indices, draw k = mix(mix(seed + h) * 8 + k) % m, k = 0, 1, .., a draw equal to an
 *      earlier kept one skipped, invalid after 32 draws.  In double:
 *      a. The 5 x 9 matrix has the rows (x'x, x'y, x', y'x, y'y, y', x, y, 1), x of `from`, x' of `to`.  Gauss-Jordan elimination with
 *         complete pivoting as lcd_verify_epipolar's step 3 (a pivot that is 0 or not finite: invalid), four free columns: the null vectors
 *         X, Y, Z, W have the free columns (1,0,0,0) .. (0,0,0,1) and the negated entries of the four remaining columns, in the columns' own
 *         order.  E = x X + y Y + z Z + W, row-major.
 *      b. Ten cubic constraints by polynomial arithmetic.  A linear polynomial has the coefficients of (x, y, z, 1); a quadratic those of
 *         (x2 y2 z2 xy xz yz x y z 1); a cubic those of (x3 y3 x2y xy2 x2z x2 y2z y2 xyz xy | xz2 xz x yz2 yz y z3 z2 z 1).  A product adds a_i
 *         b_j to its monomial's coefficient in the order of the loops, i outer, j inner, onto zeros.  Row 0 = det E by the first row's
 *         cofactors: (E11 E22 - E12 E21) E00, minus (E10 E22 - E12 E20) E01, plus (E10 E21 - E11 E20) E02.  H = half the sum of the squares
 *         of E's nine entries.  Row 1 + 3 i + j = sum over k of ((sum over n of E_in E_kn) - [k = i] H) E_kj: the entry (i, j) of (E E^T -
 *         tr(E E^T) / 2) E.
 *      c. Gauss-Jordan elimination of the first ten columns of the 10 x 20 matrix: the pivot of column k is the largest magnitude in rows k
 *         .. 9 (the lowest row on ties; a NaN is never chosen), rows exchanged, the pivot row divided, every other row r gets A_rc - (A_rk
 *         A_kc).  A pivot that is 0 or not finite: invalid.
 *      d. B(z): row r = (row 4 + 2 r) - z (row 5 + 2 r) for r = 0, 1, 2 (x2z - z x2, y2z - z y2, xyz - z xy), whose leading monomials cancel:
 *         per row the coefficient of x (degree 3 in z), of y (degree 3) and the constant (degree 4).  p(z) = det B(z), degree 10, by the first
 *         row's cofactors, polynomial products as in b.  A leading coefficient of 0 or a coefficient that is not finite: invalid.
 *      e. Real roots.  B = 1 + max |c_i / c_10| (not finite: invalid).  Derivative k has the coefficients c_(i+1) (i + 1) of derivative k -
 *         1.  From the derivative of degree 1 upwards: the ascending roots of the derivative of degree d - 1, between -B and B, are the ends
 *         of the brackets of the one of degree d; a bracket holds a root iff (p(lo) < 0) != (p(hi) < 0) (Horner from the leading
 *         coefficient), found by LCD_MONO_BISECT halvings and then the middle of what is left.  The roots of p ascend.
 *      f. Candidate c = 10 h + r is root r.  The rows of B(z) at the root; of the cross products of rows (0, 1), (0, 2), (1, 2) the one of
 *         largest squared length (the first on ties) is (v0, v1, v2); x = v0 / v2, y = v1 / v2; E = ((x X + y Y) + z Z) + W.  An absent root,
 *         or an x, y or entry that is not finite: an invalid candidate.
 *   4. Score.  E rounded to fp32.  e = (x2^T E x1)^2 / (((a + b) + c) + d), a, b the squares of the first two components of E x1, c, d of E^T
 *      x2, each component ((p u) + (q v)) + r; an inlier iff e <= thr2 (a NaN is none).  The candidate with most inliers wins, the lowest
 *      candidate on ties.  All candidates are scored: there is no adaptive stop, so the confidence 0.99 has no effect; the host mirror passes
 *      iterations = 1000.  A best count of 0: LCD_MONO_NO_MODEL.  There is no refit over the inliers.
 *   5. Decomposition of the winner's fp64 E, without an SVD (Horn): M = tr(E E^T) / 2 I - E E^T; b = M's column of the largest diagonal entry
 *      (the lowest on ties) / sqrt(that entry); C's row i = the cross product of E's rows i + 1 and i + 2 (cyclic); R1 = (C - [b]x E) / (b.b),
 *      R2 = (C + [b]x E) / (b.b), t = b / sqrt(b.b).  An entry that is not finite: LCD_MONO_NO_MODEL.
 *   6. recoverPose.  For each of (R1, t), (R2, t), (R1, -t), (R2, -t) and each inlier of step 4: the depths d1, d2 that minimise |d2 x2 - (d1 R
 *      x1 + t)|^2: a = R x1, det = (a.a)(x2.x2) - (a.x2)^2, d1 = ((a.x2)(x2.t) - (a.t)(x2.x2)) / det, d2 = ((a.a)(x2.t) - (a.x2)(a.t)) / det; a
 *      det that is 0 or not finite gives no point.  The mask: d1 > 0 ("z w > 0"), d1 < distance_threshold, 0 < d2 < distance_threshold.  The
 *      four counts go through the >= cascade as written (:609-642).  The inliers are the masked correspondences of the chosen configuration,
 *      in correspondence order; the point of each is float(d1 x1, d1 y1, d1) moved by the local transform, T(p) in fp32.
 *   7. cameraTransform = local x inverse(float [R | +-t]) x inverse(local), fp32.
 *   8. Scale and variance (:304-408).  scale = 1, variance = 1.  A guess (not NULL, no NaN, not twelve zeros): scale = |guess t| / |cameraTransform
 *      t|, |.| = sqrt((x x + y y) + z z).  With from_points3: the usable correspondences are the inliers whose point and from_points3 row are
 *      finite and not (0, 0, 0) (util3d_correspondences.cpp:388-391), n their number.  The error of one under s: |s p - g|^2 with s p
 *      component by component.  With a guess and n > 0: variance = float(2.1981 double(e_k)), e_k the error of rank k ascending (NaNs last)
 *      under scale, k = min(n >> variance_median_ratio, n - 1) (a shift, as written; where the reference would read one past the end the
 *      last is taken).  Without a guess and n > 0: candidate i = 0 .. n - 1 has s_i = g_i.x / p_i.x and its variance alike; the first is
 *      taken, and a later one replaces it iff its variance is smaller (the multimap's begin()).  scale != 1.0f: cameraTransform's
 *      translation and every finite point are multiplied by it.
 *   9. Gates (:1636-1667): inliers < min_inliers: LCD_MONO_FEW_INLIERS; then double(variance) > double(max_variance): LCD_MONO_HIGH_VARIANCE;
 *      otherwise LCD_MONO_OK.
 * Outputs: out_transform is cameraTransform for LCD_MONO_OK and twelve zeros otherwise.  out_n_matches = m (0 for LCD_MONO_FEW_FEATURES);
 * in the pair's TO-region of out_matches the ids of all pairs ascending, of out_inliers the inliers' ids and of out_points3 their points in
 * correspondence order, the rest of all three 0.  out_variance is 1.0 where step 8 was not reached.
 * Classes the search for test scenes did not find are listed in tests/motion_mono_inputs.py.
 * Out of scope: LMedS, multi-camera rigs, lens distortion, to3DoF (Reg/Force3DoF), OdometryMono, wiring Mem/StereoFromMotion, a refit over
 * the inliers, sharded handles.
 *
 * Limits and errors -- after each of them nothing was written and the handle stays usable: more than 8192 rows on a side of a pair,
 * n_pairs > 65535, iterations > 65535 or a handle of a sharded vocabulary: LCD_ERR_UNSUPPORTED; iterations < 1, min_inliers < 1, a
 * reproj_threshold or distance_threshold that is not finite and > 0, a variance_median_ratio outside 0 .. 31, a max_variance that is negative
 * or not finite, n_pairs < 0, offsets that are missing, do not start at 0 or decrease, NULL cameras, a camera whose fx or fy is 0, whose fx,
 * fy, cx or cy is not finite or under which thr2 is not finite and > 0, a NULL pointer where rows or outputs exist (from_points3, guesses,
 * out_matches, out_inliers and out_points3 may be NULL), or a wrong struct_size: LCD_ERR_INVALID.  n_pairs == 0 returns LCD_OK.  One kernel
 * launch per call whatever the batch: one workgroup of 256 threads per pair. */
#define LCD_MONO_BISECT 56
enum lcd_motion_mono_status {
    LCD_MONO_OK = 0,
    LCD_MONO_FEW_FEATURES = 1,        /* a frame with fewer rows than min_inliers */
    LCD_MONO_FEW_PAIRS = 2,           /* m < 9 */
    LCD_MONO_NO_MODEL = 3,            /* no candidate with an inlier, or a decomposition that is not finite */
    LCD_MONO_FEW_INLIERS = 4,         /* inliers, points and variance returned, no transform */
    LCD_MONO_HIGH_VARIANCE = 5        /* inliers, points and variance returned, the variance above max_variance, no transform */
};
typedef struct lcd_motion_mono_args {
    int32_t struct_size;            /* sizeof(lcd_motion_mono_args) */
    int32_t n_pairs;                /* >= 0; 0 returns LCD_OK */
    int32_t min_inliers;            /* Vis/MinInliers, >= 1 */
    int32_t iterations;             /* 1 .. 65535 */
    uint32_t seed;
    int32_t variance_median_ratio;  /* Vis/PnPVarianceMedianRatio, used as a shift: 0 .. 31 */
    double reproj_threshold;        /* Vis/PnPReprojError, pixels, finite, > 0 */
    double distance_threshold;      /* recoverPose's distanceThresh (the reference passes 50), finite, > 0 */
    float max_variance;             /* Vis/EpipolarGeometryVar, finite, >= 0 */
    int32_t reserved;
    const int32_t* from_word_ids;   /* [Nf] */
    const float* from_points;       /* [Nf x 2] cv::KeyPoint::pt, the layout lcd_keypoints_3d writes as out_points */
    const float* from_points3;      /* [Nf x 3] words3 of the from-signature, for the scale; may be NULL */
    const int32_t* to_word_ids;     /* [Nt] */
    const float* to_points;         /* [Nt x 2] */
    const int64_t* from_offsets;    /* HOST, [n_pairs + 1], non-decreasing, [0] == 0 */
    const int64_t* to_offsets;      /* HOST, [n_pairs + 1] */
    const lcd_camera* cameras;      /* HOST, [n_pairs]: fx, fy, cx, cy and the local transform */
    const float* guesses;           /* HOST, [n_pairs x 12]: cameraTransform on entry; NULL, a NaN or twelve zeros = null */
    float* out_transform;           /* [n_pairs x 12], row-major 3 x 4; twelve zeros = none */
    int32_t* out_status;            /* [n_pairs], lcd_motion_mono_status */
    int32_t* out_n_matches;         /* [n_pairs] */
    int32_t* out_n_inliers;         /* [n_pairs] */
    double* out_variance;           /* [n_pairs] */
    int32_t* out_matches;           /* [Nt]; may be NULL */
    int32_t* out_inliers;           /* [Nt]; may be NULL */
    float* out_points3;             /* [Nt x 3]; may be NULL */
} lcd_motion_mono_args;
/* every pointer on the HOST; synchronises the engine stream */
int lcd_estimate_motion_mono(lcd_engine* h, const lcd_motion_mono_args* a);
/* ids, points, from_points3 and out_* in DEVICE memory (4-byte aligned, out_variance 8-byte): the outputs of lcd_keypoints_3d go in where
 * they lie; offsets, cameras and guesses on the HOST (read during the call); enqueued on the engine stream, not synchronised */
int lcd_estimate_motion_mono_dev(lcd_engine* h, const lcd_motion_mono_args* a);

/* ---- Scan registration (point-to-point ICP), stateless: the other half of the registration step, Reg/Strategy = 1 (ICP) and 2 (visual, then
 * ICP), for a caller who holds both laser scans in device memory.  RegistrationIcp::computeTransformationImpl, the point-to-point branch
 * with Icp/Strategy = 0 (RegistrationIcp.cpp:662-971): util3d::icp (util3d_registration.cpp:384-434), util3d::computeVarianceAndCorrespondences
 * (:327-360) and the gates and the result of RegistrationIcp.cpp:856-961.  What is in the reference tree is reproduced exactly, integers and
 * control flow: the roles (source = the from-scan, target = guess x the to-scan), Reg/Force3DoF choosing the 2-D estimator, the
 * transformation epsilon epsilon x epsilon, in computeVarianceAndCorrespondences the larger cloud as the target (cloud B, the to-scan, on equal
 * sizes), correspondences that are ALWAYS reciprocal (the `reciprocal` argument is ignored at :343, as written), the >= 3 guard, the rank
 * size >> 1, variance = 2.1981 x median in fp64, the ratio against max_laser_scans when it is set and against the larger scan otherwise, the
 * gate ratio <= Icp/CorrespondenceRatio, transform = icpT.inverse() x guess.  pcl::IterativeClosestPoint, its kd-tree, its convergence
 * criteria and its two estimators are not in the reference tree: the loop, the search's tie rule, the fits and every summation order are the
 * ENGINE'S, modelled on PCL's defaults and written out here.  No bit parity with a PCL build is claimed.  Stateless exactly as
 * lcd_estimate_motion_3d; pair i owns the rows [from_offsets[i], from_offsets[i+1]) of from_xyz and out_match, [to_offsets[i],
 * to_offsets[i+1]) of to_xyz, and guesses[12 i .. 12 i + 11].  For Reg/Strategy = 2 the guess is the out_transform of
 * lcd_estimate_motion_3d / lcd_estimate_motion_pnp, copied to the host by the caller.
 *
 * The rule, per pair.  fp32, every operation rounded on its own (nothing fused), IEEE division and square root, only + - x / sqrt; "fp64"
 * marks the few places that are double.  SUM's lanes and tree, the rigid fit and inverse(T) are those of lcd_estimate_motion_3d (steps 4 and
 * 8 there); T(p) and A x B those of lcd_estimate_motion_pnp (its preamble and step 3).
 *   1. Clouds.  A row takes part iff its three coordinates are finite (the host entry refuses any other row).  The source P_0 is the
 *      participating from-rows; the target Q is T_guess(to-row) of the participating to-rows (whatever T_guess gives, finite or not).  Row
 *      indices stay those of the pair's regions; n_f and n_t are the numbers of participating rows.  n_f == 0 or n_t == 0: LCD_ICP_EMPTY.
 *   2. The nearest neighbour of p in a cloud C.  d2(c) = (dx*dx + dy*dy) + dz*dz with dx = p_x - c_x, dy and dz alike; all three coordinates
 *      enter, also with force_3dof.  The participating row of C with the smallest d2 wins, the lowest row index on ties (the order of the
 *      keys bits(d2) << 32 | row); a d2 that is NaN or +inf never wins, so p may have no neighbour.  The neighbour is a CORRESPONDENCE iff
 *      double(d2) <= thr2, thr2 = max_correspondence_distance * max_correspondence_distance in fp64 (PCL drops distance > max_dist_sqr).
 *      How an implementation finds the row (brute force, a grid) is not part of the rule; it returns this row, bit for bit.
 *   3. Iteration k = 0, 1, ..  The correspondences of the current cloud P_k against Q, NOT reciprocal (util3d::icp never sets PCL's flag);
 *      c = their number.  c < 3: LCD_ICP_NOT_CONVERGED with stop LCD_ICP_STOP_FEW_CORRESPONDENCES, and out_iterations = k.
 *      mse_k = SUM(d2) / float(c).  SUM over source rows is the 256-lane sum taken over the ROW INDEX: lane l starts at +0.0f and walks
 *      the rows l, l + 256, .. of the pair's from-region in ascending order; a row without a correspondence (or that takes no part) adds
 *      nothing -- it is skipped, not added as zero; then the halving tree.  No compaction is part of the rule.
 *   4. The fit T_k of the correspondences (p_i, q_j(i)), q from Q.  cp_a = SUM(p_a) / float(c), cq_a = SUM(q_a) / float(c),
 *      S_ab = SUM((p_a - cp_a) * (q_b - cq_b)) with this SUM.
 *      3-D: Horn's quaternion by LCD_M3D_SWEEPS Jacobi sweeps and t_r, exactly step 4 of lcd_estimate_motion_3d from cp, cq and S on.
 *      2-D (force_3dof): A = Sxx + Syy, B = Sxy - Syx, n = sqrt(A*A + B*B); if n is 0 or not finite c = 1, s = 0, else c = A / n, s = B / n.
 *      T_k = [[c, -s, 0, cq_x - (c*cp_x - s*cp_y)], [s, c, 0, cq_y - (s*cp_x + c*cp_y)], [0, 0, 1, 0]] (PCL's 2-D estimator without the
 *      arc tangent; -s is the negation of s, no rounding).
 *   5. Update.  P_{k+1} = T_k(P_k), every participating row, incrementally as PCL does.  F <- T_k x F (A x B with A = T_k: each entry
 *      ((A_r0 B_0c + A_r1 B_1c) + A_r2 B_2c), + A_r3 in the last column), F starting as the identity.  iterations = k + 1.
 *   6. Stop, tested in this order, each of them meaning converged: iterations >= max_iterations: LCD_ICP_STOP_ITERATIONS;
 *      0.5f * (((R00 + R11) + R22) - 1.0f) >= 1.0f - eps2 and (t_x*t_x + t_y*t_y) + t_z*t_z <= eps2, R and t of T_k, eps2 = epsilon * epsilon
 *      in fp32: LCD_ICP_STOP_TRANSFORM; |mse_k - mse_{k-1}| < 1e-12f with mse_{-1} = FLT_MAX: LCD_ICP_STOP_MSE.  Otherwise k + 1 follows.
 *   7. The registered cloud A = F(P_0) -- not P_k: PCL transforms the input by the final transformation.
 *   8. Variance and correspondences (:327-360) over A and B = Q.  The target is the one with more participating rows, B on equal numbers;
 *      the other is the source.  For each source row i, its nearest target row j (step 2) that is a correspondence is kept iff the nearest
 *      row of target row j in the source (step 2, no threshold) is i.  out_n_correspondences = the number kept.  out_match is written on the
 *      FROM-rows whichever cloud played the source: the to-row kept with that from-row, or -1.  With >= 3 kept out_variance =
 *      2.1981 * double(the d2 of rank (number >> 1) ascending among the kept, d2 the source row's), fp64 and undivided; otherwise 1.0.
 *   9. Ratio and result.  out_ratio = float(number) / float(max_laser_scans) when max_laser_scans > 0, otherwise / float(max(n_f, n_t)).
 *      X = inverse(F) x guess; out_correction = inverse(guess) x X; out_icp_transform = F.  out_ratio <= correspondence_ratio:
 *      LCD_ICP_BELOW_RATIO and out_transform = twelve zeros; otherwise out_transform = X and LCD_ICP_OK.
 *  10. Twelve zero floats mean no transform; then out_status != LCD_ICP_OK.  With LCD_ICP_EMPTY and LCD_ICP_NOT_CONVERGED out_icp_transform
 *      and out_correction are twelve zeros too, out_n_correspondences = 0, out_ratio = 0, out_variance = 1.0, out_match = -1 everywhere;
 *      out_stop is LCD_ICP_STOP_NONE with LCD_ICP_EMPTY.  out_icp_transform, out_correction, the counts and the variance are returned whenever
 *      the loop converged.
 * The remaining steps of :856-928 take out_correction and out_variance and are the HOST mirror's (host/RegistrationIcp.cpp), as the arc cosine
 * of lcd_estimate_motion_pnp is: the Icp/MaxTranslation / Icp/MaxRotation gate (Euler angles: an arc tangent), variance /= 10, and the
 * covariance (eye x variance, the rotation block / 10).
 * Out of scope here: point-to-plane (Icp/PointToPlane, normals, the low-complexity fallback), which is lcd_register_icp_plane below;
 * libpointmatcher and CCCoreLib (Icp/Strategy 1, 2),
 * Icp/Force4DoF, the scan filters in front (Icp/VoxelSize, DownsamplingStep, RangeMin / RangeMax), which are lcd_filter_scans below,
 * intensity, scans above 8192 points, sharded
 * handles, and on the device the Euler-angle gate and the covariance.
 *
 * search: how step 2 is carried out, never what the call returns.  LCD_ICP_SEARCH_BRUTE walks the whole target for every row.
 * LCD_ICP_SEARCH_GRID sorts the target once by cell (and the registered source for step 8) and looks at the 27 cells around a row; the cell is
 * float(max_correspondence_distance) * 1.0625, a coordinate's cell floor(x / cell).  Every output is the same bit for bit: only
 * correspondences (d2 <= thr2) and the reciprocal test reach an output, and no pair within the threshold sits more than one cell apart
 * (rtabmap_amd/csrc/icp_rule.h has the argument).  A target with a coordinate beyond +-65 535 cells is searched in the brute form inside the
 * same call, and so is a single row beyond that range.  LCD_ICP_SEARCH_AUTO takes the grid form for a target of 1 024 participating rows
 * or more, the measured size at which it overtakes the brute form on a single pair.
 *
 * Limits and errors -- after each of them nothing was written and the handle stays usable: more than 8192 rows on a side of a pair,
 * n_pairs > 65535 or a handle of a sharded vocabulary: LCD_ERR_UNSUPPORTED; max_iterations < 1, max_laser_scans < 0, a
 * search that is no lcd_icp_search, a max_correspondence_distance that is not finite or <= 0 or whose square is not finite, an epsilon that
 * is negative or not finite, a correspondence_ratio outside [0, 1], n_pairs < 0, offsets that are missing, do not start at 0 or decrease,
 * NULL guesses or a guess entry that is not finite, a NULL pointer where rows or outputs exist, a wrong struct_size, and on the HOST entry a
 * row with a coordinate that is not finite (the reference demands finite clouds): LCD_ERR_INVALID.  On the device entry such a row takes part
 * in nothing and counts towards no size.  n_pairs == 0 returns LCD_OK.  One kernel launch per call whatever the batch: one workgroup of 256
 * threads per pair. */
enum lcd_icp_status {
    LCD_ICP_OK = 0,
    LCD_ICP_EMPTY = 1,                /* a side has no participating row */
    LCD_ICP_NOT_CONVERGED = 2,        /* fewer than 3 correspondences in an iteration */
    LCD_ICP_BELOW_RATIO = 3,          /* everything returned but the transform */
    LCD_ICP_LOW_COMPLEXITY = 4        /* lcd_register_icp_plane only: strategy 0 on a pair below min_complexity */
};
enum lcd_icp_stop {
    LCD_ICP_STOP_NONE = 0,
    LCD_ICP_STOP_ITERATIONS = 1,
    LCD_ICP_STOP_TRANSFORM = 2,
    LCD_ICP_STOP_MSE = 3,
    LCD_ICP_STOP_FEW_CORRESPONDENCES = 4,
    LCD_ICP_STOP_SINGULAR = 5         /* lcd_register_icp_plane only: the point-to-plane system has no positive pivot */
};
enum lcd_icp_search {
    LCD_ICP_SEARCH_AUTO = 0,
    LCD_ICP_SEARCH_BRUTE = 1,
    LCD_ICP_SEARCH_GRID = 2
};
typedef struct lcd_icp_args {
    int32_t struct_size;            /* sizeof(lcd_icp_args) */
    int32_t n_pairs;                /* >= 0; 0 returns LCD_OK */
    int32_t max_iterations;         /* Icp/Iterations, >= 1 */
    int32_t force_3dof;             /* Reg/Force3DoF: != 0 selects the 2-D estimator */
    int32_t max_laser_scans;        /* the scan's maximum number of points; 0 = the ratio is relative to the larger scan */
    int32_t search;                 /* lcd_icp_search */
    double max_correspondence_distance; /* Icp/MaxCorrespondenceDistance, finite, > 0 */
    float epsilon;                  /* Icp/Epsilon, >= 0 */
    float correspondence_ratio;     /* Icp/CorrespondenceRatio, 0 .. 1 */
    const float* from_xyz;          /* [Nf x 3], in the from-scan's base frame; a 2-D scan has z = 0 */
    const float* to_xyz;            /* [Nt x 3], in the to-scan's base frame */
    const int64_t* from_offsets;    /* HOST, [n_pairs + 1], non-decreasing, [0] == 0 */
    const int64_t* to_offsets;      /* HOST, [n_pairs + 1] */
    const float* guesses;           /* HOST, [n_pairs x 12], row-major 3 x 4, finite */
    float* out_transform;           /* [n_pairs x 12] */
    float* out_icp_transform;       /* [n_pairs x 12]: F, source onto target */
    float* out_correction;          /* [n_pairs x 12]: guess^-1 x F^-1 x guess */
    int32_t* out_status;            /* [n_pairs], lcd_icp_status */
    int32_t* out_stop;              /* [n_pairs], lcd_icp_stop */
    int32_t* out_iterations;        /* [n_pairs] */
    int32_t* out_n_correspondences; /* [n_pairs] */
    float* out_ratio;               /* [n_pairs] */
    double* out_variance;           /* [n_pairs], undivided */
    int32_t* out_match;             /* [Nf] */
} lcd_icp_args;
/* every pointer on the HOST; synchronises the engine stream */
int lcd_register_icp(lcd_engine* h, const lcd_icp_args* a);
/* points and out_* in DEVICE memory (4-byte aligned, out_variance 8-byte), offsets and guesses on the HOST (read during the call); enqueued on
 * the engine stream, not synchronised */
int lcd_register_icp_dev(lcd_engine* h, const lcd_icp_args* a);

/* ---- Scan registration (point to plane), stateless: what RegistrationIcp::computeTransformationImpl does with the reference's defaults
 * (Icp/PointToPlane = true, Icp/Strategy = 0) to a pair of 3-D scans that carry normals (RegistrationIcp.cpp:506-661, :785-853): the
 * structural-complexity test on the normals of both scans (util3d::computeNormalsComplexity, util3d_surface.cpp:3164-3241), then either
 * util3d::icpPointToPlane (util3d_registration.cpp:451-492) with the normal-aware computeVarianceAndCorrespondences (:240-301), or -- on a
 * corridor-like pair -- the point-to-point loop of lcd_register_icp with the translation limited to the well-constrained axes.  What is in
 * the reference tree is reproduced exactly, integers and control flow: the 2 oi rows handed to the PCA, the `<` of :530 and :539 (the
 * to-side on equal complexities), the three strategies, removeNaNNormalsFromPointCloud, to3DoF applied after the registered cloud is taken,
 * the gate's count, the resize before the sort, the missing >= 3 guard.  What is PCL's or OpenCV's is the ENGINE'S rule, modelled on them and
 * written out here: cv::PCA's eigen decomposition is a cyclic Jacobi, pcl::registration::TransformationEstimationPointToPlaneLLS is solved by
 * LDL^T with a product of axis quaternions in place of Rz Ry Rx, pcl::getAngle3D is a cosine compared against a cosine.  No bit parity
 * with a PCL or OpenCV build is claimed.  Stateless exactly as lcd_register_icp: one launch per call, one workgroup of 256 threads per pair,
 * nothing of a pipelined handle drained.  Arguments that lcd_icp_args has keep their names and meaning.  A caller routes 2-D scans to
 * lcd_register_icp, as the reference does at :510-518.
 *
 * The rule, per pair.  fp32, every operation rounded on its own, IEEE division and square root, only + - x / sqrt; "fp64" marks the few
 * places that are double.  SUM, T(p), A x B, inverse(T), the search, the threshold and the stops are those of lcd_register_icp ("4n" below
 * names its steps).
 *   1. Rotated normals.  n' = R n, each entry ((R_r0 n_x + R_r1 n_y) + R_r2 n_z).  The to-scan's normals are rotated by the guess's
 *      rotation, the registered cloud's by F's (F as the loop left it, before step 4's force_3dof).
 *   2. Complexity of a side (the to-side under the guess's rotation).  oi = the number of rows whose three GIVEN normal components are
 *      finite (whatever their coordinates are).  oi <= 1: complexity 0, no values, no vectors.  Otherwise the PCA over 2 oi rows of which oi
 *      are zero, as :3221 hands them over: mean_a = SUM(n'_a) / float(2 oi); cov_ab = (SUM((n'_a - mean_a) * (n'_b - mean_b)) + float(oi) *
 *      (mean_a * mean_b)) / float(2 oi), SUM the 256-lane sum over the row index, rows without a finite normal skipped.  Eigenvalues by
 *      LCD_ICP_PLANE_SWEEPS sweeps of cyclic Jacobi over the planes (0,1), (0,2), (1,2) -- the rotation of lcd_estimate_motion_3d's step 4 --,
 *      sorted descending (the lower index first among equals), the vectors as rows.  complexity = third value * 3.0f.  Eigenvector signs
 *      are not pinned; nothing downstream depends on them (n (v . n) is even in n).
 *   3. Decision (:522-583).  complexity = the from-side's iff it is < the to-side's, else the to-side's; out_complexity_values and
 *      out_complexity_vectors are that side's (zeros without a PCA).  complexity < min_complexity is the low-complexity path: second = the
 *      smaller of the two sides' second values when complexity > 0 (the from-side's iff it is <), else 1.0; strategy 0:
 *      LCD_ICP_LOW_COMPLEXITY, everything zero but out_complexity, its values and vectors and out_second_eigenvalue; otherwise branch 1
 *      with that side's vectors when complexity > 0 and none when it is 0.  Otherwise branch 0 and second = 1.0.
 *   4. Branch 0, the loop.  A row takes part iff its coordinates AND its given normal are finite (removeNaNNormalsFromPointCloud); n_f and
 *      n_t count those rows; either 0: LCD_ICP_EMPTY.  The search, the threshold, the order of the stops and mse are 4n's steps 2, 3, 5, 6.
 *      The fit (TransformationEstimationPointToPlaneLLS, uncentred as PCL's): per correspondence (s, d, n) -- source point, target point,
 *      the target's rotated normal -- a = (s x n, n) with s x n = (s_y n_z - s_z n_y, s_z n_x - s_x n_z, s_x n_y - s_y n_x), b = n.d - n.s,
 *      dots as ((x x + y y) + z z).  The 21 products a_i a_j (i <= j, row by row) and the 6 a_i b are SUMmed over the row index; x solves
 *      the 6 x 6 by the LDL^T of lcd_estimate_motion_pnp's step 7.  A pivot that is not positive and finite, or an x that is not finite:
 *      LCD_ICP_NOT_CONVERGED with LCD_ICP_STOP_SINGULAR, out_iterations = k.  Rotation: PCL builds Rz(x_2) Ry(x_1) Rx(x_0) with sines and
 *      cosines; the rule has none.  With a = x_0 / 2, b = x_1 / 2, c = x_2 / 2 (0.5f * x) it is the unit quaternion (1 + (a b) c, a - b c,
 *      b + a c, c - a b) / norm -- the product of the three axis quaternions (1, c k) (1, b j) (1, a i), through lcd_estimate_motion_3d's
 *      quaternion rotation.  It is an exact rotation by the angles 2 atan(x / 2) = x - x^3 / 12 about the same axes in the same order, so it
 *      agrees with PCL's matrix to second order; the loop iterates, so the fixed point is the same.  Translation: (x_3, x_4, x_5).
 *      force_3dof (Transform::to3DoF, :485-489) is applied to F AFTER the registered cloud F(P_0) and its normals are taken: n = sqrt(R00 *
 *      R00 + R10 * R10), c = R00 / n, s = R10 / n (the identity when n is 0 or not finite), F <- [[c, -s, 0, F_x], [s, c, 0, F_y], [0, 0, 1, 0]].
 *   5. Branch 0, variance and correspondences (:240-301).  The target is the side with more participating rows, B on equality.  The
 *      reciprocal correspondences are 4n's step 8.  The gate (normal_gate != 0): with u = v / sqrt(v . v) (v itself when v . v is 0),
 *      double(u_target . u_source) > min_normal_cos; with the gate off all pass.  out_n_correspondences = count = those passing; out_match
 *      lists those.  Variance AS WRITTEN: distances.resize(count) precedes the sort, so with count >= 1 out_variance = 2.1981 * double(the d2
 *      of rank count >> 1 among the FIRST count reciprocal correspondences in ascending source-row order, whichever of them passed).
 *   6. Branch 1.  4n's loop unchanged over all rows with finite coordinates, force_3dof choosing the 2-D estimator.  Strategy 1 (:789-832):
 *      C = guess^-1 x F^-1 x guess, v = C's translation, vp = n1 (v . n1), plus n2 (v . n2) iff second >= min_complexity (vp_k = n1_k a + n2_k
 *      b), vp = 0 without vectors; C's rotation is kept (the Euler round trip of :826-828 returns it); F <- guess x [R_C | vp]^-1 x guess^-1,
 *      and the registered cloud is this F(P_0).  Strategy 2: F as it is.  Then 4n's steps 8-9 (the >= 3 guard, no gate).
 *   7. Outputs.  out_ratio's denominator counts the rows with finite COORDINATES (:895); X, out_correction, the gate on
 *      correspondence_ratio and the zero conventions are 4n's steps 9-10.  out_branch and the complexity outputs are written whatever the
 *      status; out_branch is 0 with LCD_ICP_LOW_COMPLEXITY.
 * min_normal_cos is cos(Icp/MaxRotation), computed by the caller (the host mirror does); angle < max is cosine > cos(max).
 * Out of scope: normal estimation (commonFiltering's computeNormals, Icp/PointToPlaneK, Radius, GroundNormalsUp), which is
 * lcd_filter_scans below, 2-D scans with normals
 * (the reference ignores point to plane for them), and everything lcd_register_icp leaves out.
 *
 * Limits and errors: those of lcd_register_icp, and LCD_ERR_INVALID for a min_complexity outside [0, 1], a low_complexity_strategy outside
 * 0 .. 2, a min_normal_cos that is not finite while the gate is on, and NULL normals where rows exist.  After a refusal nothing was written.
 * A normal that is not finite is legal on BOTH entries (the reference produces such normals); a coordinate that is not finite is refused by
 * the host entry and takes no part on the device entry. */
#define LCD_ICP_PLANE_SWEEPS 5
typedef struct lcd_icp_plane_args {
    int32_t struct_size;            /* sizeof(lcd_icp_plane_args) */
    int32_t n_pairs;                /* >= 0; 0 returns LCD_OK */
    int32_t max_iterations;         /* Icp/Iterations, >= 1 */
    int32_t force_3dof;             /* Reg/Force3DoF */
    int32_t max_laser_scans;        /* 0 = the ratio is relative to the larger scan */
    int32_t search;                 /* lcd_icp_search */
    double max_correspondence_distance; /* Icp/MaxCorrespondenceDistance, finite, > 0 */
    float epsilon;                  /* Icp/Epsilon, >= 0 */
    float correspondence_ratio;     /* Icp/CorrespondenceRatio, 0 .. 1 */
    float min_complexity;           /* Icp/PointToPlaneMinComplexity, 0 .. 1 */
    int32_t low_complexity_strategy;/* Icp/PointToPlaneLowComplexityStrategy: 0 reject, 1 limit the translation, 2 accept */
    int32_t normal_gate;            /* != 0: correspondences are counted behind the angle test (Icp/MaxRotation > 0) */
    int32_t reserved;               /* 0 */
    double min_normal_cos;          /* cos(Icp/MaxRotation); finite while the gate is on */
    const float* from_xyz;          /* [Nf x 3] */
    const float* to_xyz;            /* [Nt x 3] */
    const float* from_normals;      /* [Nf x 3], in the from-scan's own frame; may hold NaN */
    const float* to_normals;        /* [Nt x 3], in the to-scan's own frame */
    const int64_t* from_offsets;    /* HOST, [n_pairs + 1], non-decreasing, [0] == 0 */
    const int64_t* to_offsets;      /* HOST, [n_pairs + 1] */
    const float* guesses;           /* HOST, [n_pairs x 12], row-major 3 x 4, finite */
    float* out_transform;           /* [n_pairs x 12] */
    float* out_icp_transform;       /* [n_pairs x 12] */
    float* out_correction;          /* [n_pairs x 12] */
    int32_t* out_status;            /* [n_pairs], lcd_icp_status or LCD_ICP_LOW_COMPLEXITY */
    int32_t* out_stop;              /* [n_pairs], lcd_icp_stop or LCD_ICP_STOP_SINGULAR */
    int32_t* out_iterations;        /* [n_pairs] */
    int32_t* out_n_correspondences; /* [n_pairs] */
    float* out_ratio;               /* [n_pairs] */
    double* out_variance;           /* [n_pairs], undivided */
    int32_t* out_match;             /* [Nf] */
    int32_t* out_branch;            /* [n_pairs]: 0 = point to plane, 1 = point-to-point fallback */
    float* out_complexity;          /* [n_pairs] */
    float* out_complexity_values;   /* [n_pairs x 3], of the less complex side, descending */
    float* out_complexity_vectors;  /* [n_pairs x 9], its eigenvectors as rows */
    float* out_second_eigenvalue;   /* [n_pairs] */
} lcd_icp_plane_args;
/* every pointer on the HOST; synchronises the engine stream */
int lcd_register_icp_plane(lcd_engine* h, const lcd_icp_plane_args* a);
/* rows, normals and out_* in DEVICE memory (4-byte aligned, out_variance 8-byte), offsets and guesses on the HOST (read during the call);
 * enqueued on the engine stream, not synchronised */
int lcd_register_icp_plane_dev(lcd_engine* h, const lcd_icp_plane_args* a);

/* ---- Scan filtering, stateless: what RegistrationIcp does to each scan in front of the ICP, util3d::commonFiltering
 * (RegistrationIcp.cpp:362-447, util3d_filtering.cpp:74-332): Icp/DownsamplingStep, Icp/RangeMin / RangeMax, Icp/VoxelSize, the normals of
 * Icp/PointToPlaneK or Icp/PointToPlaneRadius, and Icp/PointToPlaneGroundNormalsUp -- with the reference's defaults a voxel grid of 0.05 m and
 * normals from 5 neighbours.  It turns a raw scan into what lcd_register_icp_plane takes and brings it under that call's 8 192 rows.  What is
 * in the reference tree is reproduced exactly (steps 1, 4 and 5).  pcl::VoxelGrid, pcl::NormalEstimation and the kd-tree are not in the tree:
 * steps 2 and 3 are the ENGINE'S rule, modelled on PCL's defaults and written out here.  No bit parity with a PCL build is claimed.
 * Stateless exactly as lcd_register_icp: any number of scans per call, the handle's device and stream borrowed, nothing of its state touched,
 * nothing of a pipelined handle drained.
 *
 * Scan f reads the rows [offsets[f], offsets[f+1]) of xyz and owns the rows [out_offsets[f], out_offsets[f+1]) of out_xyz and out_normals,
 * its output region; the region's length is its capacity.  The first out_count[f] rows of the region are the result; EVERY remaining row of
 * the region is written as three quiet NaNs (0x7FC00000), in out_xyz and in out_normals.  The device entries of lcd_register_icp and
 * lcd_register_icp_plane skip a row with a coordinate that is not finite and count it towards no size, so a caller who gives each scan a
 * region of at most 8 192 rows passes out_offsets to them as the pair's offsets, with nothing read back.
 *
 * The rule, per scan of n rows.  fp32, every operation rounded on its own (nothing fused), IEEE division and square root, only + - x / sqrt
 * and floor.
 *   1. Downsampling and range (util3d_filtering.cpp:90-140).  step = downsampling_step; step <= 1 or n <= step gives step = 1.  The sampled
 *      rows are 0, step, 2 step, .. while i < n - step + 1: n / step of them.  With range_min > 0 || range_max > 0: r = (x*x + y*y) + z*z, with
 *      is_2d x*x + y*y; a row goes when r is not finite, when range_min > 0 && r < range_min * range_min, or when range_max > 0 && r >
 *      range_max * range_max (strict, as written).  Order is kept.  The engine's definition for a row with a coordinate that is not finite:
 *      the host entry refuses it; the device entry drops it here, whether or not a range is set, and it still occupies its sampling slot.
 *      No row left: LCD_SCAN_EMPTY.
 *   2. Voxel grid (voxel_size > 0; pcl::VoxelGrid as voxelizeImpl :740-751 configures it).  inv = 1.0f / voxel_size; a coordinate's cell is
 *      floor(x_a * inv) as an integer -- a floor, so negative coordinates round down.  A cell beyond int32: LCD_SCAN_GRID_TOO_LARGE.  d_a =
 *      max cell - min cell + 1 in int64; d_x d_y d_z > INT32_MAX: LCD_SCAN_GRID_TOO_LARGE (the reference then splits space into octants,
 *      :695-737, which is out of scope).  A voxel's index is (c_x - min_x) + (c_y - min_y) d_x + (c_z - min_z) d_x d_y.  The output has one
 *      row per occupied voxel in ascending index: the centroid, each coordinate summed from +0.0f over the voxel's rows in ascending row
 *      order, then divided by float(count).
 *   3. Normals (normal_k > 0 or normal_radius > 0; pcl::NormalEstimation as computeNormalsImpl :2819-2857 configures it).  The cloud C is
 *      what steps 1-2 left; more than 8 192 rows in C: LCD_SCAN_TOO_MANY_ROWS.  d2 is lcd_register_icp's step 2.  The neighbours of row p in
 *      K mode: the min(K, |C|) rows with the smallest keys bits(d2) << 32 | row, p itself among them, visited in ascending key; in radius
 *      mode every row with d2 <= normal_radius * normal_radius, visited in ascending row.  Fewer than 3 neighbours: the normal is three NaNs.
 *      The sums, each from +0.0f in the visiting order, over u = q - p: S_a = SUM u_a, S_ab = SUM u_a * u_b for the upper triangle; m_a =
 *      S_a / float(n); cov_ab = S_ab / float(n) - m_a * m_b.  LCD_ICP_PLANE_SWEEPS sweeps of the cyclic Jacobi of lcd_register_icp_plane's
 *      step 2; the normal is the vector of the smallest value as the Jacobi leaves it (not normalised again; the lower index among equal
 *      values).  Flip: with v = viewpoint - p the normal is negated iff ((v_x n_x + v_y n_y) + v_z n_z) < 0.
 *   4. Rows without a normal go (laserScanFromPointCloud(cloud, normals) filters NaNs, :187, :239, :299): a row whose normal is not finite
 *      is dropped, order kept.  No row left: LCD_SCAN_EMPTY.
 *   5. Ground normals up (adjustNormalsToViewPoint, util3d_surface.cpp:3573-3606, with the viewpoint (0, 0, 10) of :328; only with
 *      ground_normals_up > 0 and normals): v = (0, 0, 10) - p; the normal is negated iff ((v_x n_x + v_y n_y) + v_z n_z) < 0 or (n_z <
 *      -ground_normals_up && p_z < 10.0f).
 *   6. Outputs.  More rows than the region holds: LCD_SCAN_NO_ROOM.  Every status but LCD_SCAN_OK gives out_count = 0 and an all-NaN region.
 *      out_stage_counts = the rows after step 1, after step 2 (step 1's without a voxel grid) and the final count, each as far as the scan
 *      got and 0 behind that; with LCD_SCAN_NO_ROOM the third is the count that found no room.  They let a caller redo the reference's
 *      maxPoints bookkeeping (util3d_filtering.cpp:159, :180-181; RegistrationIcp.cpp:363-364, :404-405, :879), as the host mirror does.
 * Out of scope: 2-D normals (computeNormals2D, computeFastOrganizedNormals2D), intensity, RGB and input normals carried through the voxel
 * grid, the octant split of an over-large grid, libpointmatcher's data-point filters (:377-402), organised scans whose rows outnumber their
 * columns (:102), scans above 16 384 sampled rows or above 8 192 rows reaching step 3, sharded handles.
 *
 * Limits and errors -- after each of them nothing was written and the handle stays usable.  LCD_ERR_UNSUPPORTED: more than 16 384 sampled
 * rows (n / step) in a scan, n_scans > 65535, a handle of a sharded vocabulary, is_2d with normals asked for.  LCD_ERR_INVALID: normal_k > 0
 * together with normal_radius > 0 (PCL refuses both), normal_k outside 0 .. LCD_SCAN_MAX_K, a float parameter that is not finite, voxel_size,
 * normal_radius or ground_normals_up below 0, n_scans < 0, offsets that are missing, do not start at 0 or decrease, NULL where rows or outputs
 * exist, out_normals NULL while normals are asked for (it is not touched when none are), a wrong struct_size, and on the HOST entry a row with
 * a coordinate that is not finite.  A negative range bound disables that bound, as the reference does.  n_scans == 0 returns LCD_OK.  At most
 * three kernel launches per call whatever the batch (one without normals): one workgroup per scan for steps 1-2, one per 256 rows of C for
 * step 3, one per scan for steps 4-6. */
enum lcd_scan_status {
    LCD_SCAN_OK = 0,
    LCD_SCAN_EMPTY = 1,               /* no row left behind step 1 or behind step 4 */
    LCD_SCAN_GRID_TOO_LARGE = 2,
    LCD_SCAN_TOO_MANY_ROWS = 3,       /* more than 8 192 rows reach the normals */
    LCD_SCAN_NO_ROOM = 4              /* the result does not fit the scan's output region */
};
#define LCD_SCAN_MAX_K 32
typedef struct lcd_scan_filter_args {
    int32_t struct_size;            /* sizeof(lcd_scan_filter_args) */
    int32_t n_scans;                /* >= 0; 0 returns LCD_OK */
    int32_t downsampling_step;      /* Icp/DownsamplingStep; <= 1: none */
    int32_t is_2d;                  /* the range uses x and y only */
    int32_t normal_k;               /* Icp/PointToPlaneK, 0 .. LCD_SCAN_MAX_K */
    int32_t reserved;               /* 0 */
    float range_min, range_max;     /* Icp/RangeMin, RangeMax; <= 0: off */
    float voxel_size;               /* Icp/VoxelSize; 0: off */
    float normal_radius;            /* Icp/PointToPlaneRadius; 0: off */
    float ground_normals_up;        /* Icp/PointToPlaneGroundNormalsUp; 0: off */
    float viewpoint[3];             /* the reference passes (0, 0, 0) */
    const float* xyz;               /* [N x 3] */
    const int64_t* offsets;         /* HOST [n_scans + 1], non-decreasing, [0] == 0 */
    const int64_t* out_offsets;     /* HOST [n_scans + 1]: each scan's output region, its capacity */
    float* out_xyz;                 /* [M x 3] */
    float* out_normals;             /* [M x 3]; NULL iff no normals are asked for */
    int32_t* out_count;             /* [n_scans] */
    int32_t* out_stage_counts;      /* [n_scans x 3]: after step 1, after the voxel grid, final */
    int32_t* out_status;            /* [n_scans], lcd_scan_status */
} lcd_scan_filter_args;
/* every pointer on the HOST; synchronises the engine stream */
int lcd_filter_scans(lcd_engine* h, const lcd_scan_filter_args* a);
/* rows and out_* in DEVICE memory (4-byte aligned), both offset arrays on the HOST (read during the call); enqueued on the engine stream,
 * not synchronised */
int lcd_filter_scans_dev(lcd_engine* h, const lcd_scan_filter_args* a);

/* Rtabmap::adjustLikelihood (Rtabmap.cpp:5691-5760) on a likelihood vector whose entry 0 is the virtual place;
 * in/out on the host, reduction on the device.  ("next" row f1 of the scope table) */
int lcd_adjust_likelihood(lcd_engine* h, float* likelihood, int n, float virtual_place_ratio);
/* the same in place on a DEVICE vector, enqueued on the engine stream and not synchronised: with the likelihood of lcd_frame_dev
 * written at d_likelihood + 1 and the virtual place's value at d_likelihood[0], the adjusted vector never leaves the device */
int lcd_adjust_likelihood_dev(lcd_engine* h, float* d_likelihood, int n, float virtual_place_ratio);

/* ---------------------------------------------------------------------------------------------------------------
 * device-resident frame path (no host round trip; what bench.py times).  All pointers are DEVICE pointers valid on
 * the engine's device; work is enqueued and NOT synchronised (lcd_synchronize, or synchronise the engine stream).
 *
 * lcd_frame_dev == Memory::update's quantisation (addNewWords :913) -> the frame's references (addWordRef :880 for
 * existing words, the VisualWord constructor's addRef :1185 for new ones) -> Memory::computeLikelihood (Memory.cpp:2177)
 * against every live signature -> optionally Rtabmap::adjustLikelihood (Rtabmap.cpp:5691) and the best candidate.
 * New words are NOT added to the vocabulary here (that is VWDictionary::update() of the next frame: lcd_vocab_append). */
typedef struct lcd_hypothesis {
    int32_t sig_id;            /* signature with the highest likelihood among the considered ones (0: none is positive);
                                  of equal likelihoods the one in the higher slot */
    int32_t slot;              /* its slot (-1: none) */
    float likelihood;          /* its raw likelihood */
    float adjusted;            /* its value after adjustLikelihood (1.0 when it is not above mean + stddev) */
    float virtual_place;       /* adjustLikelihood's value for the virtual place (entry -1 of the reference's map) */
    float mean, stddev;        /* over the positive likelihoods considered (uMean / sqrt(uVariance), UMath.h:419,512) */
    int32_t n_positive;
} lcd_hypothesis;

#define LCD_NEW_WORD_IDS_AUTO (-1)     /* lcd_frame_args.first_new_word_id: the device numbers the frame's new words (see there) */
typedef struct lcd_frame_args {
    int32_t struct_size;               /* sizeof(lcd_frame_args) */
    int32_t q;                         /* descriptors in the frame (1..8192) */
    const void* d_descriptors;         /* [q x dim], 16-byte aligned (rows are read as 16-byte vectors).  A handle whose rows are padded
                                          (lcd_config.dim): LCD_ERR_UNSUPPORTED, nothing is enqueued */
    int32_t flags;                     /* lcd_quantize_flags */
    float nndr_ratio;
    int32_t sig_id;                    /* != 0: register the frame as this signature (it must not exist yet) */
    int32_t first_new_word_id;         /* the id the caller gives the frame's first new word (VWDictionary::_lastWordId + 1); the
                                          k-th new word (descriptor order, the -(k+1) codes of d_word_ids) is first_new_word_id + k,
                                          and consecutive frames must number their new words consecutively, as ++_lastWordId does
                                          (:1185).  The frame's signature then references its new words as well, so that a later
                                          frame matching one of them -- after lcd_vocab_append -- scores this signature.
                                          0: new words get no references (fixed dictionary / caller never indexes them).
                                          LCD_NEW_WORD_IDS_AUTO (needs append_new_words): the DEVICE numbers the words, exactly as ++_lastWordId does, for a
                                          caller that does not read back how many words a frame created before it submits the next one: the id of a new
                                          word is its vocabulary row + (next word id - rows) as they stood when the run of appending frames began -- every
                                          new word is one row and one id.  The run starts from lcd_set_option(h, "next_word_id", _lastWordId + 1), or from one
                                          past the highest id the handle has seen; the frame's first id is written to d_first_new_word_id.  (Not in the
                                          sharded entry points.  ABI v7.) */
    float N;                           /* Memory::getSignatures().size() as the caller counts it (Memory.cpp:2248) */
    int32_t exclude_recent;            /* hypothesis only: the newest `exclude_recent` slots (short-term memory + this frame,
                                          Rtabmap.cpp:2050-2117 compares against the working memory only) are not considered */
    int32_t* d_word_ids;               /* out [q], as lcd_quantize */
    float* d_likelihood;               /* out, may be NULL: dense likelihood over signature slots [n_slots] (lcd_slots_dev), the
                                          frame's own slot included */
    int64_t likelihood_capacity;       /* floats available at d_likelihood */
    lcd_hypothesis* d_hypothesis;      /* out, may be NULL (needs d_likelihood): 32 bytes instead of the whole vector to the host */
    float* d_adjusted;                 /* out, may be NULL: [n_slots + 1], entry 0 = virtual place, entry 1 + slot = adjusted value
                                          (0 for slots that are retired or not considered) */
    float virtual_place_ratio;         /* Rtabmap/VirtualPlaceLikelihoodRatio (0 = default branch) */
    int32_t append_new_words;          /* 1 (needs first_new_word_id > 0, LCD_Q_INCREMENTAL, 64-float rows): the words this frame creates become
                                          vocabulary rows ON THE DEVICE, in descriptor order behind the rows that exist, before the next frame is
                                          searched == VWDictionary::update()'s append branch (:571-609) run by Memory::preUpdate of the next
                                          frame (Memory.cpp:1004-1016) -- no lcd_vocab_append, no host round trip.  On a pipelined handle the next
                                          frame's filter has already taken its snapshot by then: its re-rank scans the appended rows exactly, so
                                          the result is the 2-NN over the updated vocabulary.  Removals (lcd_vocab_remove / lcd_vocab_rebuild,
                                          cleanUnusedWords) stay host calls that complete the owed stages first. */
    int32_t* d_first_new_word_id;      /* out, may be NULL (device memory; chained frames: append_new_words on a handle whose rows live on the device): the id of
                                          the frame's first new word -- first_new_word_id itself, or what LCD_NEW_WORD_IDS_AUTO resolved to (the -(k+1) codes of
                                          d_word_ids are this + k).  (ABI v7: the field was a reserved pointer, NULL.) */
    float* d_posterior;                /* out, may be NULL (needs d_likelihood and lcd_bayes_configure): the Bayes filter's posterior
                                          after this frame, [n_slots + 1], entry 0 = virtual place, 0 for slots that are retired or
                                          not considered (BayesFilter::computePosterior, BayesFilter.cpp:145-235) */
    struct lcd_bayes_result* d_bayes;  /* out, may be NULL: the highest loop-closure hypothesis (Rtabmap.cpp:2147-2158), 32 bytes */
} lcd_frame_args;
int lcd_frame_dev(lcd_engine* h, const lcd_frame_args* args);

/* The same frame for a caller whose descriptors live in HOST memory -- what corelib hands VWDictionary::addNewWords (a cv::Mat,
 * VWDictionary.cpp:913) and gets back from Memory::computeLikelihood (Memory.cpp:2177): ONE call, one synchronisation.  The descriptors
 * are copied to the device (engine-owned pinned staging), the frame runs as lcd_frame_dev describes (quantisation -> the signature's
 * references -> [append_new_words: the words it creates become vocabulary rows, VWDictionary::update()'s append branch] -> TF-IDF
 * likelihood against every registered signature), and the word ids and the dense likelihood over the signature slots come back.
 * Slots are handed out in registration order (lcd_sig_add, lcd_sig_add_bulk in array order, frames) and never reused; a retired
 * signature's slot scores 0.  What the frames in flight of a pipelined handle owe is completed first and this frame is completed
 * before the call returns (a host caller needs its answer: use a plain handle).  (ABI v5; the reference-side caller is
 * rtabmap_amd/host/VWDictionaryHip::addNewWordsAndScore.) */
typedef struct lcd_frame_host_args {
    int32_t struct_size;               /* sizeof(lcd_frame_host_args) */
    int32_t q;                         /* descriptors in the frame (1..8192) */
    const void* descriptors;           /* HOST [q x dim], row-major, as cv::Mat::data of a continuous matrix.  A handle whose rows are
                                          padded (lcd_config.dim): LCD_ERR_UNSUPPORTED (the mirror then takes the call-by-call path) */
    int32_t flags;                     /* lcd_quantize_flags */
    float nndr_ratio;
    int32_t sig_id;                    /* != 0: register the frame as this signature */
    int32_t first_new_word_id;         /* as lcd_frame_args */
    float N;                           /* as lcd_frame_args */
    int32_t append_new_words;          /* as lcd_frame_args */
    int32_t* word_ids;                 /* HOST out [q], as lcd_quantize */
    float* likelihood;                 /* HOST out, may be NULL: [likelihood_capacity], entry = signature slot */
    int64_t likelihood_capacity;       /* floats available at likelihood (>= slots after this frame, else LCD_ERR_INVALID) */
    int64_t* n_slots;                  /* HOST out, may be NULL: slots in use after this frame = entries written */
} lcd_frame_host_args;
int lcd_frame_host(lcd_engine* h, const lcd_frame_host_args* args);
/* slots in use (host bookkeeping, nothing is synchronised or completed): what lcd_frame_host's likelihood_capacity must cover is this + 1 */
int lcd_slot_count(const lcd_engine* h, int64_t* n_slots);

/* ---------------------------------------------------------------------------------------------------------------
 * Bayes filter over the signatures of the working memory ("next" row f2 of the scope table).
 * == BayesFilter (corelib/src/BayesFilter.cpp): the posterior lives on the device, one float per signature slot; the
 * reference's dense m x m prediction matrix (:313) is never formed -- each column's non-zeros are evaluated from the
 * signature's graph-neighbour list.  The considered signatures are the live slots below n_slots - exclude_recent, as for
 * the hypothesis of lcd_frame_dev (the reference passes the working memory's likelihood, Rtabmap.cpp:2050-2133). */
typedef struct lcd_bayes_result {
    int32_t sig_id;            /* _highestHypothesis.first: the considered signature with the highest posterior (0: none > 0) */
    int32_t slot;              /* its slot (-1: none) */
    float posterior;           /* its posterior */
    float value;               /* _highestHypothesis.second = 1 - posterior of the virtual place (Rtabmap.cpp:2157) */
    float virtual_place;       /* posterior of the virtual place */
    int32_t n_considered;      /* signatures that took part (the reference's likelihood.size() - 1) */
    float sum;                 /* normalisation constant of this update (BayesFilter.cpp:221) */
    int32_t reserved;
} lcd_bayes_result;
/* BayesFilter::setPredictionLC (:77-122) + Bayes/VirtualPlacePriorThr: prediction_lc = {virtual place, loop closure, neighbour
 * level 1, level 2, ...} as getPredictionLC() returns them (2..32 values in [0, 1]).  Needed before any update. */
int lcd_bayes_configure(lcd_engine* h, const double* prediction_lc, int n_values, float virtual_place_prior);
/* BayesFilter::reset (:138-143): forget the posterior and the neighbour lists */
int lcd_bayes_reset(lcd_engine* h);
/* The graph neighbourhood of n_sigs registered signatures: for signature sig_ids[i] the entries [offsets[i], offsets[i+1]) of
 * nbr_sig_ids / nbr_margins are what Memory::getNeighborsId(id, prediction_lc.size() - 1, 0, false, false, true, true) returned
 * (BayesFilter.cpp:328, :581) -- the signature itself with margin 0 included, margins in [0, n_values - 2].  The list REPLACES
 * what the engine held for that signature (the reference's _neighborsIndex entry of a new id is exactly this answer), and like the
 * reference's incremental update (:583-592) every entry is also entered into the neighbour's own list (an existing entry for the
 * same pair is replaced) -- so a signature's list is passed once, when it enters the working memory, and keeps growing through the
 * lists of the signatures that come after it; passing every list again (Bayes/FullPredictionUpdate = true, :328-352) rebuilds them
 * all.  Neighbours that are not registered are skipped (they are in the long-term memory and can not be in a likelihood).  Host
 * pointers. */
int lcd_bayes_set_neighbors(lcd_engine* h, int n_sigs, const int32_t* sig_ids, const int64_t* offsets, const int32_t* nbr_sig_ids,
                            const int32_t* nbr_margins);
/* One filter update from an adjusted likelihood that is already on the device: d_adjusted[n_slots + 1] laid out as lcd_frame_dev
 * writes it (entry 0 = virtual place, entry 1 + slot).  Enqueued, not synchronised.  d_posterior (may be NULL) like d_adjusted. */
int lcd_bayes_update_dev(lcd_engine* h, const float* d_adjusted, int exclude_recent, float* d_posterior, lcd_bayes_result* d_result);
/* BayesFilter::computePosterior(memory, likelihood) (:145-235) with the likelihood as the std::map hands it out: n parallel host
 * entries in ascending id order, the virtual place (id -1) first (Rtabmap.cpp:2111-2115 always compares against it; a likelihood
 * without it is LCD_ERR_UNSUPPORTED).  The other ids must be every registered signature up to the newest one named -- the working
 * memory without the short-term memory, the list Rtabmap.cpp:2046-2115 builds.  Synchronises; *result (may be NULL) receives the
 * highest hypothesis (Rtabmap.cpp:2147-2158); lcd_bayes_posterior reads the vector. */
int lcd_bayes_update(lcd_engine* h, const int32_t* sig_ids, const float* adjusted, int n, lcd_bayes_result* result);
/* the filter's current posterior for some signatures (host arrays; unknown / never considered signatures -> 0); sig id -1 = the
 * virtual place.  Synchronises. */
int lcd_bayes_posterior(lcd_engine* h, const int32_t* sig_ids, int n, float* out);
/* lcd_knn2 with device-resident queries [q x dim] and outputs (d_word_ids[q*2], d_dist[q*2]); enqueued, not synchronised.  A handle whose
 * rows are padded (lcd_config.dim): LCD_ERR_UNSUPPORTED, nothing is enqueued. */
int lcd_knn2_dev(lcd_engine* h, const void* d_queries, int q, int32_t* d_word_ids, float* d_dist);
/* ---- vocabulary sharded by word-ID range over several engines/GPUs (one handle per rank).
 * Every rank holds a consecutive id range of the vocabulary and the references of those words; every rank registers
 * every signature (same order => same slots).  Per frame: (1) lcd_shard_knn2_dev on each rank, (2) all-gather of the
 * 16-byte candidate records, (3) lcd_shard_frame_dev on each rank (merge + same-frame resolution, replicated; registers the
 * frame with the words THIS rank owns; integer partial likelihood into d_lfix), (4) all-reduce(sum, int64) of d_lfix --
 * order-free, so the result equals the single-GPU one bit for bit -- (5) lcd_finalize_dev.
 * (1) and (3) of a frame are one pair: the search also leaves the frame's same-frame distance matrix on the handle (it rides in the
 * filter's launch), and the frame call that follows it with the SAME d_descriptors pointer and q -- their content unchanged in between --
 * takes it from there; any other frame call computes the matrix itself.
 * d_descriptors is [q x dim] as for lcd_frame_dev; both calls return LCD_ERR_UNSUPPORTED on a handle whose rows are padded (lcd_config.dim),
 * before anything is enqueued. */
typedef struct lcd_shard_cand { uint64_t key; int32_t word; int32_t wslot; } lcd_shard_cand;
int lcd_shard_knn2_dev(lcd_engine* h, const void* d_descriptors, int q, lcd_shard_cand* d_cand /* [q*2] */);
int lcd_shard_frame_dev(lcd_engine* h, const void* d_descriptors, int q, int flags, float nndr_ratio, int32_t sig_id,
                        int32_t first_new_word_id /* as lcd_frame_args; new words belong to the LAST rank, or block-cyclically to all of
                                                     them: lcd_set_option "shard_growth_first" / "shard_growth_block" */, float N,
                        int rank, int world, const lcd_shard_cand* d_all_cand /* [world*q*2], rank-major */,
                        int64_t total_live_rows, int32_t* d_word_ids, int64_t* d_lfix, int64_t lfix_capacity);
int lcd_finalize_dev(lcd_engine* h, int64_t* d_lfix, int64_t n, float* d_likelihood);
/* slot table: d_slot_sig[slot] = signature id (0 = retired slot), n_slots = number of slots in use */
int lcd_slots_dev(lcd_engine* h, const int32_t** d_slot_sig, int64_t* n_slots);
/* record a caller-owned hipEvent_t on the engine stream BEHIND everything the calls made so far will enqueue there (a pipelined
 * handle enqueues the registration / scoring of its latest frame with the next call: recording on lcd_stream() directly would
 * land in front of it) */
int lcd_record_event(lcd_engine* h, void* event);
/* the engine's hipStream_t (so a caller can record events around enqueued work) */
void* lcd_stream(lcd_engine* h);

/* ---------------------------------------------------------------------------------------------------------------
 * kernel timing: while enabled, every launch of the dominant kernel of a frame (the 2-NN scan: MFMA filter, or the VALU
 * scan when the filter does not apply) is bracketed by a pair of HIP events on the engine stream.  lcd_profile_read
 * synchronises, returns the average duration in milliseconds and the number of samples, and disables profiling. */
int lcd_profile_begin(lcd_engine* h, int max_samples);
int lcd_profile_read(lcd_engine* h, float* avg_ms, int* n_samples, const char** kernel_name);
/* the same for the fused likelihood kernel of lcd_frame_dev (both series are recorded while profiling is enabled) */
int lcd_profile_read_likelihood(lcd_engine* h, float* avg_ms, int* n_samples, const char** kernel_name);

/* tuning knobs for experiments (results never depend on them; every one of them is per handle).  "filter_delay": the filter workgroups
 * of a pipelined frame's launch A wait value x 64 clocks in front of their first request (0 .. 127; timing experiments).  "roctx": 1 = roctx ranges (see lcd_trace_push below).  "shadow_rows": 1 (built-in: while the stream creates 16 words per frame or more; 2 = always) = a frame that appends its words on the device also leaves its descriptors as rows
 * of an operand table, and the matrix-core filter of the NEXT frame ranks them beside the vocabulary (its re-rank keeps the ones that became words)
 * instead of every re-rank workgroup staging the new rows and scanning them (0).  "mirror_from_b": 1 (built-in) = the pinned row-count mirror of an appending
 * frame is stored by a workgroup of launch B instead of at the end of the decision loop's chain in launch A.  "row_writer_wgs": the rows a
 * frame appends are written by that many extra workgroups of launch B's re-rank role (built-in 16; 0 = by the re-rank workgroups themselves; 0 .. 256).  "slots_from_rows": 1 (built-in: while the stream creates 16 words per frame or more; 2 = always) = the decision loop of a
 * pipelined frame hands the registration the vocabulary ROW of every matched word and the registration looks the postings key up (in the
 * round trip that fetches the retired signature's words); 0 = the decision loop gathers the keys itself.  "score_block": threads per workgroup of the scoring kernel
 * (256 / 512 / 1024).  "filter_units": compute units the bf16 filter plans its persistent workgroups for when the vocabulary has
 * more 256-word strips than that (-1 built-in, 0 never persistent).  A value > 0 is also the number of compute units the matrix-core Hamming scan of a u8 handle
 * (LCD_KNN_HAMMING_MFMA) plans its workgroups for (two on each; 0 and -1: the device's own count).  "decision_straight": 1 (built-in: while the stream creates 16 words per frame or more; 2 = always; 0 = never) = the decision loop of a pipelined frame requests
 * everything its first round trip reads unconditionally, in one straight line (faster while frames create words, slower once they only revisit: DESIGN.md 4d).  "next_word_id": one past the highest word id handed out so far (VWDictionary::_lastWordId + 1): where LCD_NEW_WORD_IDS_AUTO continues (never lowered: the handle
 * keeps the maximum of this and the ids of the rows it has seen).  "profile_skip": the number of launches of a pipelined handle that lcd_profile_begin lets pass before it brackets one (0; the first launches behind an idle
 * queue are not the steady state).  "profile_likelihood": 0 = lcd_profile_begin brackets only the
 * 2-NN launch of a pipelined frame (every timed launch costs stream time).  "strip_tiles": 32-word tiles per filter workgroup of a
 * pipelined frame (1 .. 8; 0 = the built-in plan).  "append_split_buckets": sealed buckets of 256 signatures from which
 * the rows a frame appends are written by a kernel of their own behind launch B instead of by workgroups inside it (-1 = built-in, 1 024).
 * "append_from_rerank": 1 (built-in) = those rows are written by the re-rank workgroups of launch B, 0 = by eight row-writer
 * workgroups.  "cross_frame_tiles": 1 = launch A also computes a frame's distances to the frame before it and the re-rank reads
 * the distances of the rows that frame appended from there instead of staging the rows (0 / -1 = built-in: staged).
 * "pair_match_budget": bytes of distance blocks lcd_match_pairs gives one group of pairs (0 = built-in, 256 MiB; a single pair always fits; tests).
 * Unknown keys / values -> LCD_ERR_INVALID.
 * The two keys that DO change what a call means (sharded handles only, identical on every rank): "shard_growth_first" = F and
 * "shard_growth_block" = B > 0 make lcd_shard_frame_dev give the words frames create (ids >= F) to rank ((id - F) / B) % world instead of
 * the last rank, and merge the gathered candidates with ties going to the lower WORD ID -- the single-GPU row order as long as every rank
 * appends its words in ascending id ("block-cyclic so growth stays balanced").  "shard_append" = 1 (what
 * lcd_shard_set_append of include/lcd_shard.h sets): lcd_shard_frame_dev also turns the new words this rank owns into rows of its shard,
 * on the device, from the replicated decision -- VWDictionary::update()'s append, per rank. */
int lcd_set_option(lcd_engine* h, const char* key, int64_t value);

/* ---------------------------------------------------------------------------------------------------------------
 * tracing (tracing row; ABI v6).  lcd_set_option("roctx", 1) loads libroctx64.so at run time (no link dependency;
 * LCD_ERR_UNSUPPORTED when it is not installed) and from then on the engine brackets what it enqueues with roctx ranges that
 * `rocprofv3 --marker-trace` shows beside the kernels: "lcd_frame_dev", "lcd:launch_A", "lcd:launch_B", "lcd:drain", "lcd_frame_host",
 * "lcd_likelihood", "lcd_quantize".  lcd_trace_push / lcd_trace_pop put a caller's own range on the same track (the host mirror brackets its
 * CPU-side stages with the reference's names: "Memory::update", "VWDictionary::addNewWords", "Memory::computeLikelihood", ...).  Both are
 * no-ops (LCD_OK) while the option is off.  The reference has ULOGGER_DEBUG timings at these places (Memory.cpp:5931,6062; Rtabmap.cpp:4357). */
int lcd_trace_push(lcd_engine* h, const char* name);
int lcd_trace_pop(lcd_engine* h);

/* the work of ONE scoring launch for the words of the last frame (diagnostic, synchronises): out8[0] bytes of dense count rows
 * read, [1] sparse postings read (4 B each), [2] directory lookups, [3] lookups that found the word, [4] entries of the open
 * bucket's log (8 B each), [5] postings of the frame's words over all live signatures (the P of SURVEY.md 8d), [6] unique
 * words of the frame, [7] of them with dense rows */
int lcd_profile_score_work(lcd_engine* h, int64_t* out8);

/* ---------------------------------------------------------------------------------------------------------------
 * statistics (names follow Statistics.h:178,202,209-212 where one exists) */
typedef struct lcd_stats {
    int64_t vocab_rows, vocab_live;        /* Keypoint/Dictionary_size */
    int64_t signatures, postings;
    int64_t knn_launches, likelihood_launches, rebuilds;
    int64_t buckets_sealed;                /* 256-signature blocks of the inverted index regrouped on the device */
    int64_t word_slots;                    /* postings keys in use (recycled when words are removed) */
    int64_t dense_words;                   /* words whose postings are kept as dense count rows (last value the device reported) */
    int64_t frame_calls, frame_host_ns;    /* lcd_frame_dev calls and the host time spent inside them (enqueue cost) */
    int64_t bytes_device;                  /* HBM held by the handle */
    int64_t knn_last_fallback_queries;     /* queries of the LAST 2-NN call that the MFMA certificate sent to the exact scan */
    double knn_max_err_ratio;              /* largest |filter score - exact distance| / eps seen by the re-rank so far (must stay < 1) */
    int64_t clean_divergent_refs;          /* (ABI v6) references registered to a word that an ENQUEUED cleanUnusedWords (lcd_vocab_remove_unused_async) had tombstoned
                                            * while the referencing frame was in flight: the one documented departure of the device-resident mode from the
                                            * reference, whose clean runs behind that frame's addNewWords and keeps the word (Memory.cpp:6899-6920).  0 on streams
                                            * that drain before they clean */
} lcd_stats;
/* synchronises the engine stream (the fallback counter lives on the device) */
int lcd_get_stats(lcd_engine* h, lcd_stats* out);

#ifdef __cplusplus
}
#endif
#endif /* LCD_H_ */
