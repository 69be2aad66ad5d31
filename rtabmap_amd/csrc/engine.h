// engine.h -- internal state of an lcd_engine handle (liblcd_hip.so).  Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include <chrono>
#include <cmath>
#include <deque>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../include/lcd.h"
#include "devbuf.h"
#include "lcd_kernels.h"
#include "bayes.h"
#include "tfidf.h"
#include "stateless_scratch.h"

// Host mirror of the vocabulary's row order (the tie-break contract): key = word id the row was appended with, live = not tombstoned.
// While the keys are ascending (the usual case: word ids only grow) a word's row is found by binary search; only a vocabulary with
// out-of-order appends (re-activated old words) needs the id -> row map, built lazily.
struct RowMirror {
    std::vector<int32_t> h_row_key;
    std::vector<char> h_row_live;
    bool rows_sorted = true;
    std::unordered_map<int32_t, int32_t> word_row;      // only valid when !rows_sorted && word_row_valid
    bool word_row_valid = false;
    // one past the highest word id this handle has seen (rows appended by any call; "next_word_id" sets it: VWDictionary::_lastWordId + 1)
    int32_t next_word_id = 1;
    int find(int32_t word_id);                          // row of a live word, -1 if absent
    void push(int32_t id, int64_t row);                 // a row enters the mirror (the caller adds to n_rows / n_live)
    void kill(int64_t row);                             // a row is tombstoned (the caller takes it out of n_live)
    void clear() { std::vector<int32_t> none; reset(none); }
    void reset(std::vector<int32_t>& keys);             // every row live, keys ascending (taken from `keys`)
    int32_t key(int64_t row) const { return h_row_key[(size_t)row]; }
    bool live(int64_t row) const { return h_row_live[(size_t)row] != 0; }
};

struct ShardOwnership { int32_t world = 0, rank = 0, first = 0, block = 0; };   // the new words a rank appends (world 0: not sharded, every word)

// The device's record of the rows frames appended (lcd_frame_args.append_new_words): the decision loop's workgroup turns the frame's new
// words into vocabulary rows, so the row count lives on the device (d_vcnt: two alternating counters + a log of rows appended per frame).
// The host plans launches for an upper bound (the pinned report the appender writes, + q per younger frame) and catches up with the exact
// rows (RowMirror) the next time the handle is drained (lcd_engine::reconcile()).
struct AppendLog {
    static constexpr int VLOG = 4096;
    lcd::DevBuf d_vcnt;                                 // int32: [0], [1] row counters, [16 .. 16 + VLOG) rows appended by frame seq % VLOG
    unsigned long long* h_vmirror = nullptr;            // pinned: (seq + 1) << 32 | rows after that frame's append
    struct DevAppend { uint64_t seq; int32_t first_id; int32_t q; bool enabled;
                       // sharded append (lcd_shard_frame_dev): the log holds the frame's TOTAL of new words, this rank owns the ids the rule gives it
                       ShardOwnership own; };
    // LCD_NEW_WORD_IDS_AUTO: the words frames create are numbered on the device, id = row + id_delta (AppendArgs::first_id <= 0; DevAppend::first_id = -id_delta).
    // id_delta is fixed while appends are unreconciled (every new word is one row and one id), auto_window says the unreconciled appenders are numbered that way
    int32_t id_delta = 1; bool auto_window = false;
    std::deque<DevAppend> unreconciled;                 // frames whose appends the host mirror has not caught up with
    uint64_t vseq = 0;                                  // sequence number of the next frame in the chain: it reads counter vseq & 1, writes the other
    bool vcnt_active = false;                           // the counters hold the row count (set when the first appending frame arrives)
    uint32_t est_tag = 0; int64_t est_cnt = 0; double est_new = 0.0;   // last report seen, decaying maximum of new rows per appending frame

    struct Report { uint32_t tag; int64_t rows; };      // what the newest finished appender wrote (tag 0: nothing yet)
    Report report() const;
    // rows the vocabulary can have by now: exact when nothing was appended on the device since the last reconciliation, else the count the
    // newest finished appender reported (read without synchronising) + q per younger appending frame
    int64_t rows_ub(int64_t n_rows) const;
    // The rows the FILTER of chain frame `fseq` will most likely see (the count its launch reads is the one written a launch earlier: the
    // words of the frames up to fseq - 2): what the newest finished appender reported + an estimate per appending frame between that one
    // and fseq - 2, from the growth the reports have shown.  Only the launch PLAN is made for it -- correctness does not rest on it: the
    // filter masks rows beyond the device's count, and the re-rank scans exactly everything from min(plan, device count) on.
    int64_t rows_plan(uint64_t fseq, int64_t n_rows);
    int32_t* count_before(uint64_t seq) const { return d_vcnt.as<int32_t>() + (seq & 1); }         // the counter frame `seq` reads
    int32_t* count_after(uint64_t seq) const { return d_vcnt.as<int32_t>() + ((seq + 1) & 1); }    // ... and writes
    int32_t* log_slot(uint64_t seq) const { return d_vcnt.as<int32_t>() + 16 + seq % VLOG; }
    // (no-op while active) the first appending frame since the host last changed the vocabulary: the device counters take over the row count
    hipError_t activate(int64_t n_rows, hipStream_t s, int64_t* bytes_device);
    void restart() { vcnt_active = false; }             // the host changed the vocabulary: the counters start over from its count
    int32_t first_id(int32_t first_new_word_id) const { return first_new_word_id == LCD_NEW_WORD_IDS_AUTO ? -id_delta : first_new_word_id; }
    uint64_t record(int32_t first_new_word_id, int32_t q, bool enabled, ShardOwnership own = ShardOwnership());   // returns the frame's sequence number
    // the launches are planned for an upper bound that grows by q per unreported frame: the caller stays within 8 frames of the device
    hipError_t throttle(hipStream_t s) const;
    // the log is a ring (half full: catch up); removals keep their postings keys out of circulation until the host has caught up (512 frames)
    bool must_reconcile(bool rm_pending, int frames) const { return unreconciled.size() >= (size_t)VLOG / 2 || (rm_pending && frames >= 512); }
    // the id of the k-th new word of `e`, which became row `row` (first_id <= 0: the id follows the row)
    static int32_t id_of(const DevAppend& e, int k, int64_t row) { return e.first_id > 0 ? e.first_id + k : (int32_t)row - e.first_id; }
    static bool owns(const DevAppend& e, int32_t id) {                              // the sharded ownership rule
        return e.own.world <= 0 || (e.own.block > 0 ? (id >= e.own.first && ((id - e.own.first) / e.own.block) % e.own.world == e.own.rank)
                                                    : e.own.rank == e.own.world - 1);
    }
    void release(int64_t* bytes_device) { d_vcnt.release(bytes_device); if (h_vmirror) (void)hipHostFree(h_vmirror); h_vmirror = nullptr; }
};

inline AppendLog::Report AppendLog::report() const {
    if (!h_vmirror) return Report{0, 0};
    const unsigned long long v = *(volatile const unsigned long long*)h_vmirror;
    return Report{(uint32_t)(v >> 32), (int64_t)(uint32_t)v};
}

inline int64_t AppendLog::rows_ub(int64_t n_rows) const {
    if (unreconciled.empty()) return n_rows;
    const Report r = report();
    int64_t extra = 0;
    for (auto it = unreconciled.rbegin(); it != unreconciled.rend(); ++it) {
        if (r.tag != 0 && (uint32_t)(it->seq + 1) == r.tag) return r.rows + extra;
        if (it->enabled) extra += it->q;
    }
    return n_rows + extra;
}

inline int64_t AppendLog::rows_plan(uint64_t fseq, int64_t n_rows) {
    if (unreconciled.empty()) return n_rows;
    const Report r = report();
    if (r.tag == 0) return rows_ub(n_rows);                          // nothing reported yet
    if (est_tag != 0 && r.tag != est_tag) {                          // the reports moved on: rows per frame since the last look
        const double per = (double)(r.rows - est_cnt) / (double)(uint32_t)(r.tag - est_tag);
        est_new = std::max(est_new * 0.9, per);
    }
    est_tag = r.tag; est_cnt = r.rows;
    const int64_t ub = rows_ub(n_rows);
    int64_t frames = 0; bool found = false;
    for (auto it = unreconciled.rbegin(); it != unreconciled.rend(); ++it) {
        if ((uint32_t)(it->seq + 1) == r.tag) { found = true; break; }
        if (it->enabled && it->seq + 2 <= fseq) frames += 1;          // an appender the filter's count includes, not reported yet
    }
    if (!found) return ub;
    const int64_t est = r.rows + (int64_t)std::ceil((double)frames * (est_new * 1.25 + 8.0));
    return std::min(std::max(est, r.rows), ub);
}

inline hipError_t AppendLog::activate(int64_t n_rows, hipStream_t s, int64_t* bytes_device) {
    if (vcnt_active) return hipSuccess;
    hipError_t e = d_vcnt.reserve((size_t)(16 + VLOG) * 4, 0, s, bytes_device);
    if (e == hipSuccess && !h_vmirror) {
        e = hipHostMalloc((void**)&h_vmirror, 64, hipHostMallocDefault);
        if (e == hipSuccess) *h_vmirror = 0ull;
    }
    if (e == hipSuccess) e = hipMemsetD32Async((hipDeviceptr_t)d_vcnt.p, (int)n_rows, 2, s);
    if (e == hipSuccess) vcnt_active = true;
    return e;
}

inline uint64_t AppendLog::record(int32_t first_new_word_id, int32_t q, bool enabled, ShardOwnership own) {
    unreconciled.push_back(DevAppend{vseq, first_id(first_new_word_id), q, enabled, own});
    return vseq++;
}

// (the wait spins for the few microseconds a frame takes, then yields; a stream that makes no progress for a long time -- a caller-provided
// one may legitimately sit behind an event -- is waited for with hipStreamSynchronize instead of failing)
inline hipError_t AppendLog::throttle(hipStream_t s) const {
    if (!h_vmirror || unreconciled.size() <= 8) return hipSuccess;
    const auto t0 = std::chrono::steady_clock::now();
    for (int spins = 0;; ++spins) {
        if ((uint32_t)vseq - report().tag <= 8u) return hipSuccess;
        if (spins > 4096) std::this_thread::yield();
        if ((spins & 1023) == 1023 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(200)) return hipStreamSynchronize(s);
    }
}

// The software pipeline of lcd_frame_dev (lcd_config.pipeline): four frames are in flight.  With frame t the newest, its call launches
//        A = query pre-split of frame t  +  filter of frame t - 1  +  decision loop of frame t - 2  +  retirement / registration of frame t - 3
//        B = re-rank of frame t - 1  +  scoring of frame t - 3            (then the decision stage of frame t - 3, if asked for)
// so every single-workgroup latency chain hides behind the matrix-core filter.  The scratch a frame's stages hand to each other
// lives in a ring indexed by the frame's sequence number; what a frame still owes (`stage`) and the calls made behind it
// (retirements, neighbour lists, event records, cleans) wait in `inflight` until a later lcd_frame_dev carries them or any other call
// on the handle completes them stand-alone (lcd_engine::drain()).  The rules are the methods below; the launches are frame_pipeline.hip's.
struct FramePipeline {
    static constexpr int PIPE_SETS = 4;                 // a frame's set is in use for four calls (pre-split .. registration)
    static constexpr int DEPTH = PIPE_SETS - 1;         // lcd_pipeline_depth(): the later calls that still enqueue work of a frame (callers rotate DEPTH + 1 buffer sets)
    struct FrameScratch {
        lcd::DevBuf d_knn_row, d_knn_word, d_knn_dist, d_selfdist, d_bits, d_partial2, d_partial3, d_fail_list, d_fail_count, d_out_wslot;
        lcd::DevBuf d_qsplit, d_qnorm;                  // the frame's queries pre-split into bf16 matrix-core operands, their norms
        lcd::DevBuf d_applist;                          // deferred append: which descriptors of the frame became words (AppendArgs::list_out)
        lcd::DevBuf d_cross;                            // the frame's distances to the descriptors of the frame before it (PipeKnn::cross)
        lcd::DevBuf d_shadow_bf, d_shadow_norm, d_newmask;   // shadow rows: the frame's descriptors as operand-table rows + augmentation entries (written by its
                                                        // query pre-split), its final new-word mask + prefix sums (written by its decision loop)
        bool fail_count_clean = false;
    };
    struct DeferredLink { std::vector<int32_t> triples, restart; };
    enum class Stage { Filter, Decision, Registration };   // what a frame owes next: filter + re-rank / the decision loop / registration + scoring
    struct InFlight {
        lcd_frame_args a; lcd::ResolveArgs r; int set = 0;
        uint64_t vseq = 0; bool chained = false;        // the frame takes part in the device row-count chain (applog.vcnt_active at its call)
        bool has_shadow = false;                        // its query pre-split also wrote its shadow rows (FrameScratch::d_shadow_bf)
        bool slots_are_rows = false;                    // its decision loop left vocabulary ROWS in r.out_wslot (PipeOpts::slots_from_rows): the registration looks the keys up
        lcd::WsRuns runs; bool reserved = false;        // postings keys of its new words (reserved when its decision loop is prepared)
        Stage stage = Stage::Filter;
        std::vector<int32_t> retire_after;              // lcd_sig_remove calls made while this was the newest frame
        std::vector<void*> events_after;                // lcd_record_event calls ...
        std::vector<DeferredLink> links_after;          // lcd_bayes_set_neighbors calls ...
        int cleans_after = 0;                           // lcd_vocab_remove_unused_async calls ...
    };
    FrameScratch ring[PIPE_SETS];
    std::deque<InFlight> inflight;                      // oldest first
    uint64_t frame_seq = 0;                             // frames submitted so far
    uint64_t advances = 0;                              // launch pairs that moved the frames in flight on (progress())
    bool clean_armed = false;                           // a clean waits for the next fused launch pair, whose registration applies the
                                                        // retirements asked for before it (they ride there: no launches of their own)

    // frames in flight hold pointers into their ring sets: the OTHER sets may only be resized while this holds
    bool empty() const { return inflight.empty(); }
    const InFlight& newest() const { return inflight.back(); }
    // the signatures the frames in flight register: each gets a slot when its registration runs
    int64_t owed_sigs() const { int64_t n = 0; for (const InFlight& f : inflight) if (f.a.sig_id != 0) n += 1; return n; }
    bool registers(int32_t id) const {
        for (const InFlight& f : inflight) if (f.a.sig_id != 0 && f.a.sig_id == id) return true;
        return false;
    }
    bool retirement_queued(int32_t id) const {
        for (const InFlight& f : inflight) if (std::find(f.retire_after.begin(), f.retire_after.end(), id) != f.retire_after.end()) return true;
        return false;
    }
    // the slot signature `id` has, or will get: an owed signature gets n_slots + its rank among the owed ones, in frame order.  -1: not held, or on its way out
    int64_t slot_of(int32_t id, const lcd::Tfidf& t) const {
        int64_t k = 0;
        for (const InFlight& f : inflight) {
            if (f.a.sig_id == 0) continue;
            if (f.a.sig_id == id) return retirement_queued(id) ? -1 : t.n_slots + k;
            k += 1;
        }
        auto it = t.sig_slot.find(id);
        return it == t.sig_slot.end() || retirement_queued(id) ? -1 : it->second;
    }
    // a call made with frames in flight takes its place behind the newest: it runs, in call order, once every stage of that frame is enqueued
    void queue_retire(int32_t sig_id) { inflight.back().retire_after.push_back(sig_id); }
    void queue_event(void* event) { inflight.back().events_after.push_back(event); }
    void queue_link(DeferredLink&& dl) { inflight.back().links_after.push_back(std::move(dl)); }
    void queue_clean() { inflight.back().cleans_after += 1; }

    // stages advance oldest first, one per launch pair: a pair carries the oldest frame owing each stage
    struct Owing { InFlight* reg = nullptr; InFlight* res = nullptr; InFlight* knn = nullptr; };
    Owing owing() {
        Owing o;
        for (InFlight& f : inflight) {
            if (f.stage == Stage::Registration && !o.reg) o.reg = &f;
            else if (f.stage == Stage::Decision && !o.res) o.res = &f;
            else if (f.stage == Stage::Filter && !o.knn) o.knn = &f;
        }
        return o;
    }
    // the pair that carried `o` is enqueued: each frame owes its next stage.  True: a registration ran, that frame is complete -- it is the
    // oldest entry (stages advance in order) and leaves with pop_oldest()
    bool advance(const Owing& o) {
        if (o.res) o.res->stage = Stage::Registration;
        if (o.knn) o.knn->stage = Stage::Decision;
        advances += 1;
        return o.reg != nullptr;
    }
    InFlight pop_oldest() { InFlight f = std::move(inflight.front()); inflight.pop_front(); return f; }
    uint64_t progress() const { return advances; }      // changes whenever advance() ran: a failed launch pair that left it alone moved nothing
    // a frame's ring set is seq % PIPE_SETS: its own for the PIPE_SETS calls from its pre-split to its registration
    int next_set() const { return (int)(frame_seq % PIPE_SETS); }
    FrameScratch& scratch(const InFlight& f) { return ring[f.set]; }
    void submit(InFlight&& f) { f.set = next_set(); f.stage = Stage::Filter; inflight.push_back(std::move(f)); frame_seq += 1; }
};

struct lcd_engine {
    int device = 0;
    int dtype = 0;
    int dim = 0;            // columns as given by the caller
    int row_bytes = 0;      // bytes per stored row (u8 rows are zero-padded to a multiple of 4)
    int kdim = 0;           // `dim` as the kernels see it (floats, or padded bytes)
    hipStream_t stream = nullptr;
    bool own_stream = false;
    std::string err;
    int64_t bytes_device = 0;

    // ---- vocabulary: rows [n_rows x row_bytes], row_id[r] = word id (0 = tombstone), row_wslot[r] = postings key
    lcd::DevBuf vocab, row_id, row_wslot;
    lcd::DevBuf vocab_alt, row_id_alt, row_wslot_alt;   // rebuild target (swapped in)
    int64_t n_rows = 0, n_live = 0;
    RowMirror mirror;
    lcd::DevBuf row_norm_alt;
    lcd::DevBuf vocab_bf;                               // hi/lo bf16 split of the rows (256 B per row) for the bf16x3 filter

    // ---- per-call scratch
    lcd::DevBuf d_queries, d_partial, d_knn_row, d_knn_word, d_knn_wslot, d_knn_dist, d_selfdist, d_out_word, d_out_wslot,
        d_n_new, d_tmp_i32, d_extra_rows, d_extra_id, d_extra_word, d_extra_dist, d_extra_row, d_like, d_slots, d_bits, row_norm, norm_max, d_partial2, d_partial3, d_fail_list, d_fail_count;
    // a sharded search (lcd_shard_knn2_dev) leaves the frame's same-frame distance matrix here when its filter launch can carry it; the frame call
    // behind the all-gather (lcd_shard_frame_dev, same descriptors) then only merges and derives the bit rows
    lcd::DevBuf d_shard_selfdist;
    const void* shard_sd_desc = nullptr; int shard_sd_q = 0;
    bool fail_count_clean = false;                      // d_fail_count[0..1] known to be zero (the fused frame tail resets them)
    bool bf_family() const { return knn_mode == 2 || knn_mode == 3; }   // the bf16x3 / fp16 filters share kernels, tables and the pipelined frame
    int f16() const { return knn_mode == 3 ? 1 : 0; }
    int knn_mode = 2;                                   // f32 dim 64: 2 = bf16x3 MFMA filter + exact re-rank (default), 3 = fp16 one-product filter, 1 = f32 MFMA filter
                                                        // + exact re-rank, 0 = exact VALU scan only (lcd_config.knn_mode)
    bool hamming_mfma = false;                          // u8 handles, LCD_KNN_HAMMING_MFMA: the main vocabulary's Hamming 2-NN runs on the i8 matrix cores (knn_hamming_mfma.hip)
    bool wide_mfma = false;                             // f32 x 128 / f32 x 256 handles whose caller wrote LCD_KNN_BF16X3 or LCD_KNN_F16: the main vocabulary's 2-NN runs the
                                                        // stateless matrix-core filter + re-rank + redo (wide_filter_body.cuh); f16() picks the operands
    lcd::DevBuf d_wide_norm;                            // its scratch word: the largest |row|^2 the filter multiplied (zeroed by every search)
    // ---- pipelined frames (lcd_config.pipeline): see FramePipeline
    int pipeline = 0;
    hipStream_t kst = nullptr;                          // the stream the 2-NN stage is enqueued on (== stream)
    FramePipeline pipe;
    const void* last_fail_count = nullptr;              // certificate counters of the latest pipelined frame (lcd_get_stats)
    // tests (lcd_debug_last_frame_knn): where the latest frame's 2-NN stage left its rows, words and distances ([q x 2] each)
    const void* dbg_knn_row = nullptr; const void* dbg_knn_word = nullptr; const void* dbg_knn_dist = nullptr; int dbg_knn_q = 0;
    // ---- VWDictionary::update()'s append branch on the device (lcd_frame_args.append_new_words): see AppendLog
    AppendLog applog;
    int64_t vocab_capacity_cfg = 0;                     // lcd_config.vocab_capacity: every per-row buffer is sized for it
    int64_t tail_filled_rows = 0;                       // rows [n_rows, tail_filled_rows) carry +inf norms and a zero bf16 split
    // ---- Memory::cleanUnusedWords on the device without completing the frames in flight (lcd_vocab_remove_unused_async): the rows a
    // clean_unused_kernel tombstoned are logged on the device; the host's row mirror and the postings keys of the removed words catch up
    // with the log the next time the handle is drained (reconcile()).
    lcd::DevBuf d_rmlog;                                // int32: [0] rows logged, [16 ..] the rows
    int64_t rm_seen = 0;                                // log entries the host mirror has caught up with
    bool rm_pending = false;                            // a clean was enqueued since the last reconciliation
    int frames_since_reconcile = 0;                     // pipelined frames submitted with rm_pending set
    int enqueue_clean(const int32_t* reg_cnt = nullptr);  // flush the pending retirements, launch the kernel (nothing is synchronised); reg_cnt:
                                                        // device row count as of the newest registered frame (rows behind it are not scanned)
    int reconcile();
    // sharded vocabulary, balanced growth (lcd_set_option "shard_growth_first" / "shard_growth_block"): the words frames create (ids >=
    // shard_first) belong to rank ((id - shard_first) / shard_block) % world; 0 = they belong to the last rank
    int32_t shard_first = 0, shard_block = 0;
    int shard_append = 0;                               // lcd_set_option("shard_append"): lcd_shard_frame_dev appends the new words this rank owns on the device
    int filter_units = -1;                              // lcd_set_option("filter_units")
    int strip_tiles = 0;                                // lcd_set_option("strip_tiles"): tiles per filter workgroup of a pipelined frame (0: planner)
    lcd::PipeOpts popt;                                 // options of the fused launches ("cross_frame_tiles", "append_from_rerank", "append_split_buckets", "filter_delay"); f16 follows knn_mode
    int sync_all();                                     // stream drained
    int drain(bool rows = true);                        // complete the owed index stage (stand-alone launches); rows: the host's row mirror
                                                        // catches up with the rows appended / removed on the device (reconcile(): synchronises, two small reads)
    const char* prof2_kernel = "score_kernel";
    lcd::PinBuf h_in, h_out, h_out2;
    lcd::PinBuf h_frame_in, h_frame_out;                // lcd_frame_host: descriptors in, word ids + likelihood out (one synchronisation per call)
    lcd::DevBuf d_frame_desc, d_frame_words, d_frame_like;
    lcd::Bayes bayes;                                   // Bayes filter over the signature slots (bayes.h)
    lcd::DevBuf d_adj_scratch;                          // adjusted likelihood when the caller wants the posterior but not that vector
    lcd::DevBuf d_hyp_scratch;                          // hypothesis record when the caller only wants the adjusted vector
    StatelessScratch pairs;                             // the scratch of every stateless call (stateless_scratch.h lists them)

    // ---- inverted index / TF-IDF
    lcd::Tfidf tfidf;

    // ---- event bracketing of the dominant kernel (lcd_profile_*)
    std::vector<hipEvent_t> prof_ev, prof2_ev;          // 2-NN scan kernel / fused likelihood kernel
    int prof_n = 0, prof_cap = 0, prof2_n = 0;
    int prof_skip = 0;                                  // "profile_skip": pipelined launches lcd_profile_begin lets pass before it samples
    bool prof_likelihood = true;                        // lcd_set_option("profile_likelihood"): also bracket launch B of a pipelined frame
    const char* prof_kernel = "";

    // ---- statistics
    int64_t knn_launches = 0, likelihood_launches = 0, rebuilds = 0, frame_calls = 0, frame_host_ns = 0;
    // where the host time of a pipelined lcd_frame_dev goes (lcd_debug_host_profile): ns accumulated per section
    //   0 checks + throttle + capacity   1 ring reservations   2 reserve_frame_words + decision-loop arguments   3 registration + scoring arguments
    //   4 filter plan (build_knn)   5 launch A   6 launch B   7 the rest of pipeline_launch (flush_held, finish_frame_ops)   8 calls
    int64_t host_prof[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};

    // ---- roctx ranges (lcd_set_option "roctx"): resolved from libroctx64.so at run time, NULL while off
    int (*roctx_push)(const char*) = nullptr;
    int (*roctx_pop)() = nullptr;
    struct Range {   // a range for the lifetime of a scope
        lcd_engine* h;
        Range(lcd_engine* e, const char* name) : h(e && e->roctx_push ? e : nullptr) { if (h) h->roctx_push(name); }
        ~Range() { if (h) h->roctx_pop(); }
    };

    int fail(int code, const std::string& msg) { err = msg; return code; }
    int hip_fail(hipError_t e, const char* what) {
        err = std::string(what) + ": " + hipGetErrorString(e);
        return LCD_ERR_HIP;
    }
};
