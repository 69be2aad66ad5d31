// frame_pipeline.hip -- the per-frame path of the C-ABI (lcd_frame_dev, lcd_frame_host): the software pipeline of a pipelined handle
// (FramePipeline, engine.h: what is in flight and the rules it follows; here: what each fused launch pair carries) and the
// stand-alone frame of a plain handle.  Host code only, like engine.hip: the launches are knn_mfma_kernels.hip's, tfidf.hip's and
// bayes.hip's.  The host time of a pipelined call is on the headline's critical path: what is called per frame is in this file or
// inline in engine.h / engine_impl.h.
#include "engine_impl.h"

#include <algorithm>
#include <chrono>
#include <cstring>

using namespace lcd;

namespace {
struct FrameHostTimer {   // host time spent inside lcd_frame_dev (lcd_stats.frame_host_ns)
    lcd_engine* h; std::chrono::steady_clock::time_point t0;
    explicit FrameHostTimer(lcd_engine* e) : h(e), t0(std::chrono::steady_clock::now()) {}
    ~FrameHostTimer() { h->frame_host_ns += std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count(); h->frame_calls += 1; }
};
struct HostLap {   // section timer of the pipelined frame's host path (host_prof)
    lcd_engine* h; std::chrono::steady_clock::time_point t;
    explicit HostLap(lcd_engine* e) : h(e), t(std::chrono::steady_clock::now()) {}
    void lap(int i) { const auto n = std::chrono::steady_clock::now(); h->host_prof[i] += std::chrono::duration_cast<std::chrono::nanoseconds>(n - t).count(); t = n; }
};
// what a frame's flags and size decide for every stage: `together` = its new words are compared with each other (a same-frame distance
// matrix of ld columns, candidate bit rows of bw words)
struct FrameShape { bool incremental, together; int ld, bw; };
inline FrameShape frame_shape(const lcd_frame_args& a) {
    const bool incremental = (a.flags & LCD_Q_INCREMENTAL) != 0;
    const int ld = (a.q + 63) / 64 * 64;
    return FrameShape{incremental, incremental && (a.flags & LCD_Q_NEW_WORDS_COMPARED) != 0, ld, ld / 32};
}
}  // namespace

// the index stage of a frame, launched on its own: registration (or query preparation), scoring, hypothesis
// Rtabmap::adjustLikelihood + the best candidate (Rtabmap.cpp:2121-2158), then the Bayes filter's update and its highest
// hypothesis (Rtabmap.cpp:2133-2158), without any vector leaving the device.  The frame's likelihood is already enqueued.
static int hypothesis_stage(lcd_engine* h, const lcd_frame_args& a) {
    Tfidf& t = h->tfidf;
    const bool bayes = a.d_posterior || a.d_bayes;
    if (!(a.d_hypothesis || a.d_adjusted || bayes)) return LCD_OK;
    const long long n_cons = (long long)t.n_slots - std::max(a.exclude_recent, 0);
    DecideArgs d;
    d.like = a.d_likelihood; d.ratio = a.virtual_place_ratio; d.adj_out = a.d_adjusted; d.hyp = (HypothesisOut*)a.d_hypothesis;
    d.bayes = bayes; d.d_posterior = a.d_posterior; d.d_bayes = (BayesOut*)a.d_bayes;
    LCD_HIP(h, h->bayes.decide(d, t.slot_sig.as<int32_t>(), t.n_slots, n_cons));
    return LCD_OK;
}

// likelihood + decision stage of a frame whose registration (or query preparation) has just been enqueued stand-alone
static int frame_score_s(lcd_engine* h, const lcd_frame_args& a) {
    Tfidf& t = h->tfidf;
    if (!a.d_likelihood) return LCD_OK;
    if (h->prof_cap > 0 && h->prof2_n < h->prof_cap) {
        t.prof_b = h->prof2_ev[2 * h->prof2_n]; t.prof_e = h->prof2_ev[2 * h->prof2_n + 1];
        h->prof2_n += 1;
        h->prof2_kernel = "score_kernel";
    }
    LCD_HIP(h, t.score(a.d_likelihood));
    if (t.prof_b) { t.prof_b = t.prof_e = nullptr; h->prof2_n -= 1; }     // the launch that would have been bracketed did not happen
    h->likelihood_launches += 1;
    return hypothesis_stage(h, a);
}

// (any descriptor type: rows that are not 64 floats are copied without the matrix-core filter's tables -- such handles are never pipelined;
// rows are stored as they arrive: a handle whose rows are padded does not get here, frame_dev_body refuses it)
static bool frame_appends(const lcd_engine* h, const lcd_frame_args& a) {
    (void)h;
    return a.append_new_words != 0 && (a.first_new_word_id > 0 || a.first_new_word_id == LCD_NEW_WORD_IDS_AUTO) && (a.flags & LCD_Q_INCREMENTAL) != 0;
}

// Who numbers the words this frame creates.  LCD_NEW_WORD_IDS_AUTO: the device, id = row + id_delta -- exact as long as every unreconciled appender is
// numbered that way (one new word = one row = one id), so a change of mode completes what is owed first; id_delta is set while the host's row
// mirror is current.
static int id_window(lcd_engine* h, const lcd_frame_args& a) {
    const bool is_auto = a.first_new_word_id == LCD_NEW_WORD_IDS_AUTO;
    if (a.first_new_word_id < 0 && !is_auto) return h->fail(LCD_ERR_INVALID, "lcd_frame_dev: first_new_word_id");
    if (is_auto && !frame_appends(h, a))
        return h->fail(LCD_ERR_INVALID, "lcd_frame_dev: LCD_NEW_WORD_IDS_AUTO needs append_new_words on an incremental dictionary of unpadded rows");
    if (!frame_appends(h, a)) return LCD_OK;
    if (!h->applog.unreconciled.empty() && h->applog.auto_window != is_auto) { int rc = h->drain(); if (rc) return rc; }
    if (h->applog.unreconciled.empty()) {
        h->applog.auto_window = is_auto;
        if (is_auto) {
            const int64_t d = (int64_t)h->mirror.next_word_id - h->n_rows;
            if (d < 1 || d >= (1ll << 28)) return h->fail(LCD_ERR_STATE, "lcd_frame_dev: next_word_id lies below the ids the vocabulary holds (lcd_set_option \"next_word_id\")");
            h->applog.id_delta = (int32_t)d;
        }
    }
    return LCD_OK;
}

static int reserve_frame_words(lcd_engine* h, const lcd_frame_args& a, WsRuns* runs, bool may_flush = true) {
    *runs = WsRuns();
    // postings keys for the words this frame may create (VisualWord(id, descriptor, signatureId) references the signature; a word that
    // becomes a vocabulary row on the device needs its key there as well)
    if ((a.sig_id != 0 || frame_appends(h, a)) && (a.first_new_word_id > 0 || (a.first_new_word_id == LCD_NEW_WORD_IDS_AUTO && frame_appends(h, a))) && (a.flags & LCD_Q_INCREMENTAL)) {
        hipError_t e = h->tfidf.keys.reserve_new_words(a.first_new_word_id, a.q, runs, may_flush);
        if (e == hipErrorInvalidValue) return h->fail(LCD_ERR_UNSUPPORTED, "lcd_frame_dev: word ids must be below 2^28");
        LCD_HIP(h, e);
    }
    return LCD_OK;
}

// the whole index stage of a frame, launched on its own: decision loop + registration (one workgroup), scoring, decision stage
// chained / vseq: the frame's place in the device row-count chain (a frame that takes part appends its new words, or hands the count on)
static int frame_stage_s(lcd_engine* h, const lcd_frame_args& a, ResolveArgs r, bool chained = false, uint64_t vseq = 0) {
    Tfidf& t = h->tfidf;
    const int q = a.q;
    if (a.sig_id != 0 && t.sig_slot.count(a.sig_id)) return h->fail(LCD_ERR_STATE, "lcd_frame_dev: signature already registered");
    const int64_t slots_after = t.n_slots + (a.sig_id != 0 ? 1 : 0);
    if (a.d_likelihood && a.likelihood_capacity < slots_after) return h->fail(LCD_ERR_INVALID, "lcd_frame_dev: likelihood buffer too small");
    { int rc = reserve_frame_words(h, a, &r.new_ws); if (rc) return rc; }
    if (chained) fill_append(h, a, vseq, frame_appends(h, a), &r); else r.ap = AppendArgs();
    if (a.sig_id != 0) LCD_HIP(h, t.register_dev(a.sig_id, r.out_wslot, q, q, a.N, &r));
    else LCD_HIP(h, t.query_dev(r.out_wslot, q, a.N, &r));
    return frame_score_s(h, a);
}

// the same for a frame whose decision loop has already run (it left the word slots in r.out_wslot, new words as codes)
static int frame_stage_reg_s(lcd_engine* h, const lcd_frame_args& a, const ResolveArgs& r) {
    Tfidf& t = h->tfidf;
    if (a.sig_id != 0 && t.sig_slot.count(a.sig_id)) return h->fail(LCD_ERR_STATE, "lcd_frame_dev: signature already registered");
    if (a.sig_id != 0) LCD_HIP(h, t.register_dev(a.sig_id, r.out_wslot, a.q, a.q, a.N));
    else LCD_HIP(h, t.query_dev(r.out_wslot, a.q, a.N));
    return frame_score_s(h, a);
}

// the calls made while `f` was the newest frame of a pipelined handle, in call order, once every stage of `f` is enqueued
static int finish_frame_ops(lcd_engine* h, FramePipeline::InFlight& f) {
    for (int32_t sig : f.retire_after) LCD_HIP(h, h->tfidf.retire(sig));
    f.retire_after.clear();
    for (const FramePipeline::DeferredLink& dl : f.links_after) {
        LCD_HIP(h, h->bayes.ensure(std::max<int64_t>(h->tfidf.n_slots, 1)));
        const hipError_t e = h->bayes.link(dl.triples, dl.restart);
        if (e == hipErrorInvalidValue) { f.links_after.clear(); return h->fail(LCD_ERR_UNSUPPORTED, "lcd_bayes_set_neighbors: a neighbour list longer than 8192 entries"); }
        LCD_HIP(h, e);
    }
    f.links_after.clear();
    if (f.cleans_after > 0) { f.cleans_after = 0; h->pipe.clean_armed = true; }   // runs behind the next launch pair (pipeline_launch) or the drain
    for (void* ev : f.events_after) LCD_HIP(h, hipEventRecord((hipEvent_t)ev, h->stream));
    f.events_after.clear();
    return LCD_OK;
}

// the vocabulary buffers may have been reallocated since a frame's arguments were stored (device-side appends grow them)
static void refresh_vocab_ptrs(lcd_engine* h, ResolveArgs* r) {
    r->row_wslot = h->row_wslot.as<int32_t>();
    if (r->rp.enabled) { r->rp.vocab = (const float*)h->vocab.p; r->rp.row_id = h->row_id.as<int32_t>(); }
}

// One scratch buffer of a pipelined frame: in the frame's own set of the ring -- and, while nothing is in flight, in every other set as
// well, so that a steady stream of frames does not meet a hipMalloc (hundreds of microseconds) each time a set sees its first frame.
// The other sets are NOT touched while frames are in flight: those frames' launch arguments hold pointers into them.
static inline hipError_t ring_reserve(lcd_engine* h, int own_set, DevBuf FramePipeline::FrameScratch::*member, size_t bytes) {
    hipError_t e = dreserve(h, h->pipe.ring[own_set].*member, bytes);
    if (e != hipSuccess || !h->pipe.empty()) return e;
    for (FramePipeline::FrameScratch& sc : h->pipe.ring) {
        e = dreserve(h, sc.*member, bytes);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// ... for a buffer whose size follows the vocabulary: `need` bytes now; when that takes a (re)allocation, `want` >= need bytes are asked for, so that the set does
// not outgrow the buffer again a few frames later (a reallocation with frames in flight waits for the stream, and every set of the ring pays its own)
static inline hipError_t ring_reserve_grow(lcd_engine* h, int own_set, DevBuf FramePipeline::FrameScratch::*member, size_t need, size_t want) {
    if ((h->pipe.ring[own_set].*member).cap >= need) return hipSuccess;
    return ring_reserve(h, own_set, member, std::max(need, want));
}

// The 2-NN stage of an in-flight frame, planned when its filter is about to be launched (the row count may have grown since the frame was
// submitted): scratch of the frame's ring set, launch plan, and the arguments its decision loop will need one launch later.
// f_sh: the frame whose decision loop rides in the same launch A and whose shadow rows this filter ranks (NULL: none)
static int build_knn(lcd_engine* h, FramePipeline::InFlight& f, PipeKnn* kp, const FramePipeline::InFlight* f_sh) {
    PipeKnn& k = *kp;
    const lcd_frame_args& a = f.a;
    const int q = a.q;
    FramePipeline::FrameScratch& sc = h->pipe.scratch(f);
    const auto [incremental, together, ld, bw] = frame_shape(a);
    const int64_t rows_bound = f.chained ? h->applog.rows_ub(h->n_rows) : h->n_rows;   // a true upper bound: the exact redo and the buffers are sized for it
    const int64_t plan_rows = f.chained ? h->applog.rows_plan(f.vseq, h->n_rows) : h->n_rows;
    if (plan_rows > 0x7FFFFFF0ll) return h->fail(LCD_ERR_UNSUPPORTED, "lcd_frame_dev: more than 2^31 rows");
    // The distance tiles get compute units of their own (a tile that shares one with a strip takes twice as long, and so does the
    // strip); the two tail workgroups do not: a filter workgroup holds 66 KB of LDS, so two of the launch's workgroups can share a
    // compute unit, and one strip less per workgroup is worth more than the two shared units (49 000 words x 500 descriptors:
    // 219 seven-tile strips + 36 tiles + 2 = 257 workgroups, frame 31.6 us; 192 eight-tile strips 32.1; 256 six-tile strips 34.5).
    k.plan = knn_bf16_plan_pipelined(q, (int)plan_rows, together ? knn_selfdist_wgs(q) : 0, h->filter_units);
    k.plan.f16 = h->f16();
    if (h->strip_tiles > 0 && plan_rows > 0) {                       // timing experiments: a fixed strip length, one workgroup per strip
        const int n_tiles = (int)((plan_rows + 31) / 32);
        k.plan.tiles_per_block = h->strip_tiles; k.plan.n_blocks = (n_tiles + h->strip_tiles - 1) / h->strip_tiles; k.plan.one_strip = 1;
        k.plan.f16 = h->f16();
    }
    if (f_sh && !knn_bf16_persistent(k.plan) && plan_rows < (int64_t)SHADOW_ROW_BASE) {
        const FramePipeline::FrameScratch& ss = h->pipe.scratch(*f_sh);
        k.plan.n_shadow = 1;
        k.sh_bf = ss.d_shadow_bf.p; k.sh_norm = ss.d_shadow_norm.as<float>(); k.sh_rows = (f_sh->a.q + 63) / 64 * 64;
        k.sh_mask = ss.d_newmask.as<uint32_t>(); k.sh_q = f_sh->a.q;
        k.sh_ld = k.sh_rows;
        LCD_HIP(h, ring_reserve(h, f.set, &FramePipeline::FrameScratch::d_cross, (size_t)q * k.sh_ld * 4));   // (the buffer the cross-frame tiles use: never both)
        k.sh_x = sc.d_cross.as<float>();
    }
    {   // the candidate records: sized for this plan AND for the one the upper bound would get (a growing vocabulary crosses the planner's
        // thresholds: a reallocation drains the stream)
        // ... and, when that takes an allocation, for a vocabulary half as large again: a set that outgrows its buffers while frames are in flight reallocates
        // behind a synchronisation of the stream, and so does each of the other sets when its turn comes -- four stalls of ~0.24 ms in a row where
        // 125 000 rows happen to fill their allocation (profiles/dead_ends_r06.txt 15)
        size_t bytes = knn_bf16_partial_bytes(k.plan), want = 0;
        if (f.chained) {
            bytes = std::max(bytes, knn_bf16_partial_bytes(knn_bf16_plan_pipelined(q, (int)(rows_bound + 8 * (int64_t)q), together ? knn_selfdist_wgs(q) : 0, h->filter_units)));
            want = knn_bf16_partial_bytes(knn_bf16_plan_pipelined(q, (int)std::min<int64_t>(rows_bound + rows_bound / 2 + 65536, 0x7FFFFF00ll), together ? knn_selfdist_wgs(q) : 0, h->filter_units));
        }
        LCD_HIP(h, ring_reserve_grow(h, f.set, &FramePipeline::FrameScratch::d_partial2, bytes, want));
    }
    {
        const int64_t rows3 = rows_bound + (f.chained ? 8 * (int64_t)q : 0);
        LCD_HIP(h, ring_reserve_grow(h, f.set, &FramePipeline::FrameScratch::d_partial3, knn_rowpar_partial_bytes((int)rows3, q),
                                     f.chained ? knn_rowpar_partial_bytes((int)std::min<int64_t>(rows3 + rows3 / 2 + 65536, 0x7FFFFF00ll), q) : 0));
    }
    k.vocab = h->vocab.p; k.vocab_bf = h->vocab_bf.p; k.row_norm = h->row_norm.as<float>(); k.norm_max_bits = h->norm_max.as<uint32_t>();
    k.row_id = h->row_id.as<int32_t>(); k.queries = a.d_descriptors; k.partial = sc.d_partial2.p;
    k.qsplit = sc.d_qsplit.p; k.qnorm = sc.d_qnorm.as<float>();
    k.out_row = sc.d_knn_row.as<int32_t>(); k.out_word = sc.d_knn_word.as<int32_t>(); k.out_dist = sc.d_knn_dist.as<float>();
    k.fail_list = sc.d_fail_list.as<int32_t>(); k.fail_count = sc.d_fail_count.as<int32_t>();
    k.n_lo = nullptr; k.n_hi = nullptr;
    if (f.chained) { k.n_lo = h->applog.count_after(f.vseq); k.n_hi = h->applog.count_before(f.vseq); }
    k.cb = CandBits();
    if (together) { k.cb.selfdist = sc.d_selfdist.as<float>(); k.cb.ld = ld; k.cb.nq = q; k.cb.have_index = 1; cand_bits_layout(k.cb, sc.d_bits.as<uint32_t>(), q, bw); }
    if (!sc.fail_count_clean) LCD_HIP(h, hipMemsetAsync(sc.d_fail_count.p, 0, 8, h->stream));
    sc.fail_count_clean = true;                                      // the frame's decision loop (a later launch A) resets the counters
    h->last_fail_count = sc.d_fail_count.p;
    h->dbg_knn_row = k.out_row; h->dbg_knn_word = k.out_word; h->dbg_knn_dist = k.out_dist; h->dbg_knn_q = q;
    // ---- the decision loop's arguments (launched one call later), the redo of rejected queries riding with it
    ResolveArgs& r = f.r;
    r = ResolveArgs();
    r.q = q; r.flags = (incremental ? LCD_Q_INCREMENTAL : 0) | (together ? LCD_Q_NEW_WORDS_COMPARED : 0); r.nndr = a.nndr_ratio; r.have_index = 1;
    r.knn_word = k.out_word; r.knn_dist = k.out_dist; r.selfdist = together ? sc.d_selfdist.as<float>() : nullptr; r.ld = ld;
    r.cand_bits = together ? sc.d_bits.as<uint32_t>() : nullptr; r.bw = bw; r.out_word = a.d_word_ids; r.out_n_new = h->d_n_new.as<int32_t>();
    r.cand_list = together ? k.cb.list : nullptr; r.cand_cnt = together ? k.cb.cnt : nullptr;
    r.knn_row = k.out_row; r.row_wslot = h->row_wslot.as<int32_t>(); r.out_wslot = sc.d_out_wslot.as<int32_t>(); r.new_ws = WsRuns();
    r.fail_count = sc.d_fail_count.as<int32_t>();
    RowparArgs& rp = r.rp;
    rp.enabled = 1; rp.vocab = (const float*)h->vocab.p; rp.row_id = h->row_id.as<int32_t>(); rp.n_rows = (int)rows_bound;
    rp.n_rows_dev = k.n_hi;                                          // the rows that exist when the redo runs: after the previous frame's append
    rp.queries = (const float*)a.d_descriptors; rp.fail_list = sc.d_fail_list.as<int32_t>(); rp.partial = (unsigned long long*)sc.d_partial3.p;
    rp.out_row = k.out_row; rp.out_word = k.out_word; rp.out_dist = k.out_dist;
    if (together) rp.cb = k.cb;
    return LCD_OK;
}

// What one pair of fused launches carries: the frames owing a stage (f_reg / f_res / f_knn below are o.reg / o.res / o.knn) and the launch
// arguments of each role, built in the order of pipeline_launch()
struct LaunchPair {
    FramePipeline::Owing o;
    TailLaunch tl_reg, tl_res;                          // the registration of f_reg, the decision loop of f_res
    ScoreArgs sa; int score_wgs = 0; bool reg_like = false;   // the scoring of f_reg (launch B), when it asked for a likelihood
    PipeKnn k;                                          // the filter (launch A) and re-rank (launch B) of f_knn
};

// the decision loop of f_res (+ its redo helpers, + the append of its new words)
static int decision_args(lcd_engine* h, LaunchPair& p) {
    FramePipeline::InFlight* f_res = p.o.res; TailLaunch& tl_res = p.tl_res;
    // FIRST, before any launch argument is built: the reservation may move the word-indexed tables (they double when the keys run
    // out -- every ~3 000 frames at 150 new words per frame), and the registration / scoring arguments below hold pointers into
    // them.  The postings keys of the words that frame may create are reserved now (the batched check of older reservations waits until
    // launch A is enqueued: the registration that rides in it may still use some of those keys)
    { int rc = reserve_frame_words(h, f_res->a, &f_res->runs, false); if (rc) return rc; }
    f_res->reserved = true;
    tl_res.r = f_res->r;
    tl_res.r.new_ws = f_res->runs;
    refresh_vocab_ptrs(h, &tl_res.r);
    // (rows instead of postings keys in out_wslot: NULL is the decision loop's "knn_row already holds the word slot"; the registration translates)
    // (built-in: only while the stream creates words, like the shadow scores -- the gather leaves the decision loop's chain for the registration's, and once frames
    // revisit, the decision loop is short and the registration is what ends launch A: 13.8 -> 14.5 us in the revisit phase with the rows always on, r06_ab_notes.txt 10)
    f_res->slots_are_rows = h->popt.slots_from_rows && (h->popt.slots_from_rows >= 2 || h->applog.est_new >= 16.0) && tl_res.r.row_wslot && tl_res.r.knn_row && tl_res.r.q <= 1024;
    if (f_res->slots_are_rows) { tl_res.r.row_wslot = nullptr; tl_res.r.slots_are_rows = 1; }
    tl_res.r.straight = (h->popt.decision_straight >= 2 || (h->popt.decision_straight == 1 && h->applog.est_new >= 16.0)) ? 1 : 0;
    if (f_res->chained) fill_append(h, f_res->a, f_res->vseq, frame_appends(h, f_res->a), &tl_res.r, h->pipe.scratch(*f_res).d_applist.as<uint32_t>());
    // the pinned row-count mirror is a store to HOST memory, waited for at the end of the decision loop's chain: with "mirror_from_b" a
    // workgroup of launch B of this pair (which writes the frame's rows anyway) stores it instead
    if (h->popt.mirror_from_b && tl_res.r.ap.enabled && tl_res.r.ap.defer_rows) tl_res.r.ap.mirror_later = 1;
    resolve_launch_info(tl_res.r, pipe_block_size(), &tl_res.n_redo, &tl_res.shmem_resolve);
    return LCD_OK;
}

// the retirement / registration of f_reg and its scoring
static int registration_args(lcd_engine* h, LaunchPair& p) {
    Tfidf& t = h->tfidf;
    const FramePipeline::InFlight* f_reg = p.o.reg;
    const lcd_frame_args& pa = f_reg->a;
    if (pa.sig_id != 0) LCD_HIP(h, t.register_dev(pa.sig_id, f_reg->r.out_wslot, pa.q, pa.q, pa.N, nullptr, false, &p.tl_reg));
    else LCD_HIP(h, t.query_dev(f_reg->r.out_wslot, pa.q, pa.N, nullptr, false, &p.tl_reg));
    if (f_reg->slots_are_rows) p.tl_reg.a.row_wslot = h->row_wslot.as<int32_t>();
    if (pa.d_likelihood) {
        LCD_HIP(h, t.score_args(pa.d_likelihood, nullptr, pipe_b_block_size(), &p.sa, &p.score_wgs));
        p.reg_like = true;
        h->likelihood_launches += 1;
    }
    return LCD_OK;
}

// the filter + re-rank of f_knn, and what it has to know about the words f_res creates in the same launch A
static int filter_plan(lcd_engine* h, LaunchPair& p) {
    FramePipeline::InFlight* f_knn = p.o.knn; FramePipeline::InFlight* f_res = p.o.res;
    TailLaunch& tl_res = p.tl_res; PipeKnn& k = p.k;
    // shadow rows: f_res's new words are not rows when f_knn's filter runs (its decision loop rides in the same launch) -- the filter ranks f_res's
    // descriptors from the operand rows its query pre-split left, the re-rank keeps the ones the mask f_res's decision loop publishes names
    const bool sh_ok = f_knn && f_res && f_res->has_shadow && f_res->chained && f_knn->chained && tl_res.r.ap.enabled && tl_res.r.ap.defer_rows && tl_res.r.ap.is_f32_64 &&
                       h->popt.shadow_rows && !h->popt.cross_frames && h->popt.append_from_rerank;
    if (f_knn) { int rc = build_knn(h, *f_knn, &k, sh_ok ? f_res : nullptr); if (rc) return rc; h->knn_launches += 1; }
    if (f_res && f_res->has_shadow && tl_res.r.ap.enabled && tl_res.r.ap.defer_rows) tl_res.r.ap.mask_out = h->pipe.scratch(*f_res).d_newmask.as<uint32_t>();
    if (f_knn && f_res && tl_res.r.ap.enabled && tl_res.r.ap.defer_rows && tl_res.r.ap.is_f32_64 && h->popt.cross_frames) {
        // The rows f_res appends (its decision loop rides in this launch A) are descriptors of f_res, and f_knn's re-rank (this launch B)
        // must scan them exactly: extra distance tiles of launch A compute f_knn x f_res in the reference's arithmetic, the re-rank reads
        // its pending rows' distances there instead of staging the rows (the buffer was sized when f_knn was submitted: no reallocation here)
        const int ncols = f_res->a.q, ldx = (ncols + 63) / 64 * 64;
        lcd::DevBuf& xb = h->pipe.scratch(*f_knn).d_cross;
        if (ncols > 0 && f_knn->a.q > 0 && xb.cap >= (size_t)f_knn->a.q * ldx * 4) {
            k.cross = xb.as<float>(); k.cross_ld = ldx; k.cross_cols = tl_res.r.ap.descriptors; k.cross_ncols = ncols;
        }
    }
    return LCD_OK;
}

static int launch_a(lcd_engine* h, LaunchPair& p, const QSplitArgs* qs) {
    const FramePipeline::Owing& o = p.o;
    bool prof = o.knn && h->prof_cap > 0 && h->prof_n < h->prof_cap;
    if (prof && h->prof_skip > 0) { h->prof_skip -= 1; prof = false; }     // ("profile_skip": not the first launches behind an idle queue)
    h->popt.f16 = h->f16();
    if (h->roctx_push) h->roctx_push("lcd:launch_A");
    const hipError_t ea__ = launch_frame_a(o.knn ? &p.k : nullptr, qs, o.res ? &p.tl_res : nullptr, o.reg ? &p.tl_reg : nullptr, h->stream,
                              prof ? h->prof_ev[2 * h->prof_n] : nullptr, prof ? h->prof_ev[2 * h->prof_n + 1] : nullptr, h->popt);
    if (h->roctx_pop) h->roctx_pop();
    LCD_HIP(h, ea__);
    if (prof) {
        h->prof_n += 1;
        if (h->f16())
            h->prof_kernel = knn_bf16_persistent(p.k.plan) ? "frame_a_kernel_p (persistent fp16 filter of frame t-1 + query pre-split of t + decision loop of t-2 + registration of t-3)"
                                                           : "frame_a_kernel (fp16 filter of frame t-1 + query pre-split of t + decision loop of t-2 + registration of t-3)";
        else
            h->prof_kernel = knn_bf16_persistent(p.k.plan) ? "frame_a_kernel_p (persistent bf16 filter of frame t-1 + query pre-split of t + decision loop of t-2 + registration of t-3)"
                                                           : "frame_a_kernel (bf16 filter of frame t-1 + query pre-split of t + decision loop of t-2 + registration of t-3)";
    }
    return LCD_OK;
}

// launch B and what follows it: the clean that was waiting for this pair, then the frames in flight move on and the complete one leaves
static int launch_b(lcd_engine* h, LaunchPair& p, HostLap& lap) {
    const FramePipeline::Owing& o = p.o; const TailLaunch& tl_res = p.tl_res;
    const bool prof2 = o.knn && p.reg_like && h->prof_likelihood && h->prof_cap > 0 && h->prof2_n < h->prof_cap;
    AppendRowsArgs app;
    if (o.res && tl_res.r.ap.enabled && tl_res.r.ap.defer_rows) { app.ap = tl_res.r.ap; app.new_ws = tl_res.r.new_ws; }
    if (h->roctx_push) h->roctx_push("lcd:launch_B");
    const hipError_t eb__ = launch_frame_b(o.knn ? &p.k : nullptr, p.reg_like ? &p.sa : nullptr, p.score_wgs, h->stream, prof2 ? h->prof2_ev[2 * h->prof2_n] : nullptr,
                                           prof2 ? h->prof2_ev[2 * h->prof2_n + 1] : nullptr, app.ap.enabled ? &app : nullptr, h->popt);
    if (h->roctx_pop) h->roctx_pop();
    LCD_HIP(h, eb__);
    lap.lap(6);
    LCD_HIP(h, h->tfidf.keys.flush_held_if_due());                        // (behind launch B: the rows it writes claim their postings keys there)
    if (prof2) { h->prof2_n += 1; h->prof2_kernel = "frame_b_kernel (re-rank of frame t-1 + scoring of frame t-3)"; }
    if (h->pipe.clean_armed && o.reg) {
        // cleanUnusedWords asked for behind an earlier frame: the retirements made in front of it rode with the registration of this
        // launch A, the reference counts are what Memory::preUpdate would see -- one kernel, between this launch B and the next launch A
        // f_res's decision loop ran in this launch A and its new words are rows since this launch B, but they get their first reference
        // with its registration, in the NEXT launch A: the clean stops at the count f_res started from (the counter it read, untouched
        // until the next decision loop writes it) -- addNewWords references a word as it creates it, cleanUnusedWords never sees one
        h->pipe.clean_armed = false;
        const int32_t* reg_cnt = o.res && o.res->chained ? h->applog.count_before(o.res->vseq) : nullptr;
        int rc = h->enqueue_clean(reg_cnt); if (rc) return rc;        // (flushes what more than four retirements per frame left over)
    }
    if (h->pipe.advance(o)) {                                        // a frame is complete: its decision stage and the calls queued behind it
        FramePipeline::InFlight done = h->pipe.pop_oldest();
        if (done.a.d_likelihood) { int rc = hypothesis_stage(h, done.a); if (rc) return rc; }
        int rc = finish_frame_ops(h, done);
        if (rc) return rc;
    }
    return LCD_OK;
}

// One pair of fused launches of a pipelined handle.  With frame t the newest:
//   A = queries of frame t pre-split into matrix-core operands  +  filter (+ same-frame distance tiles) of frame t-1
//       + decision loop of frame t-2 (+ its redo helpers, + the append of its new words)  +  retirement / registration of frame t-3
//   B = re-rank of frame t-1  +  scoring of frame t-3   (then the decision stage of frame t-3 and the calls queued behind it)
// qs == NULL: nothing new -- drain() advances what is in flight with the same fused launches.
// (the laps are lcd_engine::host_prof's sections)
static int pipeline_launch(lcd_engine* h, const QSplitArgs* qs) {
    LaunchPair p;
    p.o = h->pipe.owing();
    HostLap lap(h);
    if (p.o.res) { int rc = decision_args(h, p); if (rc) return rc; }
    lap.lap(2);
    if (p.o.reg) { int rc = registration_args(h, p); if (rc) return rc; }
    lap.lap(3);
    { int rc = filter_plan(h, p); if (rc) return rc; }
    lap.lap(4);
    { int rc = launch_a(h, p, qs); if (rc) return rc; }
    lap.lap(5);
    { int rc = launch_b(h, p, lap); if (rc) return rc; }             // (lap 6 ends behind the launch itself)
    lap.lap(7);
    return LCD_OK;
}

int lcd_engine::drain(bool rows) {
    int rc_all = LCD_OK;
    Range range__(pipe.empty() ? nullptr : this, "lcd:drain");
    while (!pipe.empty()) {                                          // three fused launch pairs complete what is owed, oldest first
        const uint64_t before = pipe.progress();
        const int rc = pipeline_launch(this, nullptr);
        if (rc && !rc_all) rc_all = rc;
        if (rc && pipe.progress() == before) {                       // no progress: drop the frame instead of spinning
            FramePipeline::InFlight f = pipe.pop_oldest();
            (void)finish_frame_ops(this, f);
        }
    }
    if (pipe.clean_armed) { pipe.clean_armed = false; const int rc = enqueue_clean(); if (rc && !rc_all) rc_all = rc; }
    const int rc3 = rows ? reconcile() : LCD_OK;                     // rows appended on the device: the host mirror catches up
    return rc_all ? rc_all : rc3;
}

// Pipelined handle, matrix-core 2-NN (knn_mfma_kernels.hip, frame_a_kernel / frame_b_kernel): four frames are in flight.  The call for
// frame t pre-splits its queries and carries one stage of each of the three frames before it (pipeline_launch); what the frames still
// owe afterwards waits in h->pipe.
static int frame_pipelined(lcd_engine* h, const lcd_frame_args* a) {
    Tfidf& t = h->tfidf;
    const int q = a->q;
    HostLap lap0(h);
    h->host_prof[8] += 1;
    // validate against the index as it will be once the owed stages have run
    if (a->sig_id != 0 && (h->pipe.registers(a->sig_id) || t.sig_slot.count(a->sig_id))) return h->fail(LCD_ERR_STATE, "lcd_frame_dev: signature already registered");
    const int64_t slots_after = t.n_slots + h->pipe.owed_sigs() + (a->sig_id != 0 ? 1 : 0);
    if (a->d_likelihood && a->likelihood_capacity < slots_after) return h->fail(LCD_ERR_INVALID, "lcd_frame_dev: likelihood buffer too small");
    // (a stream that never completes anything catches up every 512 frames with removals pending: three fused launch pairs, ~0.2 us per frame)
    if (h->rm_pending) h->frames_since_reconcile += 1;
    if (h->applog.must_reconcile(h->rm_pending, h->frames_since_reconcile)) { int rc = h->drain(); if (rc) return rc; }
    { int rc = id_window(h, *a); if (rc) return rc; }
    // rows appended on the device: the counters take over the row count, the buffers keep room for the words of the frames in flight
    const bool app = frame_appends(h, *a);
    if (app) LCD_HIP(h, h->applog.activate(h->n_rows, h->stream, &h->bytes_device));
    const bool chained = h->applog.vcnt_active;
    // The launches are planned for an upper bound of the row count: what the newest FINISHED appender reported + q per younger frame.  A
    // caller that enqueues frames much faster than the device runs them would inflate that bound without limit (the filter would scan
    // mostly empty rows): such a caller waits here until the device is at most 8 frames behind.
    if (chained) {
        LCD_HIP(h, h->applog.throttle(h->stream));
        int rc = ensure_append_capacity(h, h->applog.rows_ub(h->n_rows) + 3 * (int64_t)q); if (rc) return rc;
    }
    const int set = h->pipe.next_set();
    FramePipeline::FrameScratch& sc = h->pipe.ring[set];
    const auto [incremental, together, ld, bw] = frame_shape(*a);
    lap0.lap(0);
    // ---- the frame's scratch set (what does not depend on the launch plan; the partial keys are sized when the filter is planned)
    LCD_HIP(h, ring_reserve(h, set, &FramePipeline::FrameScratch::d_qsplit, knn_qsplit_bytes(q)));
    LCD_HIP(h, ring_reserve(h, set, &FramePipeline::FrameScratch::d_qnorm, (size_t)ld * 4));
    LCD_HIP(h, ring_reserve(h, set, &FramePipeline::FrameScratch::d_fail_list, (size_t)q * 4));
    LCD_HIP(h, ring_reserve(h, set, &FramePipeline::FrameScratch::d_knn_row, (size_t)q * 2 * 4));
    LCD_HIP(h, ring_reserve(h, set, &FramePipeline::FrameScratch::d_knn_word, (size_t)q * 2 * 4));
    LCD_HIP(h, ring_reserve(h, set, &FramePipeline::FrameScratch::d_knn_dist, (size_t)q * 2 * 4));
    LCD_HIP(h, ring_reserve(h, set, &FramePipeline::FrameScratch::d_out_wslot, (size_t)q * 4));
    LCD_HIP(h, ring_reserve(h, set, &FramePipeline::FrameScratch::d_applist, (size_t)std::max(q, 512) * 4));   // (the re-rank reads 512 entries unconditionally)
    if (together) {
        LCD_HIP(h, ring_reserve(h, set, &FramePipeline::FrameScratch::d_selfdist, (size_t)q * ld * 4));
        LCD_HIP(h, ring_reserve(h, set, &FramePipeline::FrameScratch::d_bits, cand_bits_bytes(q, bw)));
    }
    if (chained && !h->pipe.empty() && h->dtype == LCD_F32 && h->kdim == 64 && (h->popt.cross_frames || h->popt.shadow_rows))   // (pipeline_launch: this frame x the frame before it)
        LCD_HIP(h, ring_reserve(h, set, &FramePipeline::FrameScratch::d_cross, (size_t)q * ((h->pipe.newest().a.q + 63) / 64 * 64) * 4));
    // shadow rows: a frame that appends on the device leaves its descriptors as operand-table rows too, for the filter of the frame behind it
    // (built-in: only while the stream creates words -- the scores cost launch A ~1 us (16 more workgroups, the pre-split's extra stores) and buy launch B
    // ~3.5 us per frame whose predecessor appended ~150 rows, nothing when it appended none; est_new is the decaying maximum of rows per appending frame
    // that the launch plans already keep.  "shadow_rows" = 2: always)
    const bool with_shadow = chained && app && h->popt.shadow_rows && h->dtype == LCD_F32 && h->kdim == 64 && q <= 4096 &&
                             (h->popt.shadow_rows >= 2 || h->applog.est_new >= 16.0);
    if (with_shadow) {
        LCD_HIP(h, ring_reserve(h, set, &FramePipeline::FrameScratch::d_shadow_bf, (size_t)ld * 256));
        LCD_HIP(h, ring_reserve(h, set, &FramePipeline::FrameScratch::d_shadow_norm, (size_t)(ld + 1) * 8));
        LCD_HIP(h, ring_reserve(h, set, &FramePipeline::FrameScratch::d_newmask, (size_t)(2 * (ld / 32) + 4) * 4));
    }
    QSplitArgs qs;
    qs.queries = (const float*)a->d_descriptors; qs.nq = q; qs.qpad = ld; qs.qsplit = (uint4*)sc.d_qsplit.p; qs.qnorm = sc.d_qnorm.as<float>(); qs.n_wgs = 0; qs.f16 = h->f16();
    if (with_shadow) { qs.shadow_bf = sc.d_shadow_bf.as<uint32_t>(); qs.shadow_norm = sc.d_shadow_norm.as<float>(); qs.norm_max_bits = h->norm_max.as<uint32_t>(); }
    lap0.lap(1);
    // ---- what the frames in flight owe rides with this frame's launches
    { int rc = pipeline_launch(h, &qs); if (rc) return rc; }
    // ---- this frame's filter, re-rank, decision loop, registration and scoring are owed from here on
    FramePipeline::InFlight nf;
    nf.a = *a; nf.chained = chained; nf.has_shadow = with_shadow;
    if (chained) nf.vseq = h->applog.record(a->first_new_word_id, q, app);
    h->pipe.submit(std::move(nf));                                   // (into the set reserved above)
    return LCD_OK;
}

// this handle's frames go through the pipeline: it was asked for, the matrix-core filter serves the handle and has a vocabulary to work on
// (256 rows, an index of at least two words), and the frame fits the fused launches
static bool goes_through_pipeline(const lcd_engine* h, int q) {
    return h->pipeline && q <= 4096 && h->bf_family() && knn_mfma_supported(h->dtype, h->kdim) && h->n_live >= 2 && h->n_rows >= 256;
}

// A stream of appending frames on a plain handle with the exact scan (ORB: config 3) does not wait for the device between frames:
// the host's row mirror lags (as on a pipelined handle), the scan is planned for an upper bound of the row count.
static bool mirror_may_lag(const lcd_engine* h) {
    return h->pipe.empty() && h->applog.vcnt_active && h->n_live >= 2 && !(h->knn_mode != 0 && knn_mfma_supported(h->dtype, h->kdim)) &&
           !h->applog.must_reconcile(h->rm_pending, h->frames_since_reconcile);
}

static int frame_dev_body(lcd_engine* h, const lcd_frame_args* a) {
    if (!a || a->struct_size != (int32_t)sizeof(lcd_frame_args)) return h->fail(LCD_ERR_INVALID, "lcd_frame_dev: bad argument block");
    const int q = a->q;
    if (q <= 0 || q > 8192 || !a->d_descriptors || !a->d_word_ids) return h->fail(LCD_ERR_INVALID, "lcd_frame_dev: bad argument");
    if (((uintptr_t)a->d_descriptors & 15u) != 0) return h->fail(LCD_ERR_INVALID, "lcd_frame_dev: d_descriptors must be 16-byte aligned");
    if (rows_padded(h)) return h->fail(LCD_ERR_UNSUPPORTED, "lcd_frame_dev: rows of this size are padded on the device (use lcd_quantize)");
    if ((a->d_hypothesis || a->d_adjusted || a->d_posterior || a->d_bayes) && !a->d_likelihood)
        return h->fail(LCD_ERR_INVALID, "lcd_frame_dev: the hypothesis needs d_likelihood");
    if ((a->d_posterior || a->d_bayes) && !h->bayes.configured) return h->fail(LCD_ERR_STATE, "lcd_frame_dev: lcd_bayes_configure first");
    if (goes_through_pipeline(h, q)) return frame_pipelined(h, a);
    { int rc = id_window(h, *a); if (rc) return rc; }
    const bool app = frame_appends(h, *a);
    // anything but such a stream (mirror_may_lag) completes what is owed and brings the mirror up to date first
    const bool lazy = app && mirror_may_lag(h);
    if (!lazy) { int rc = h->drain(); if (rc) return rc; }         // (also brings the host's row mirror up to date)
    else {
        if (h->rm_pending) h->frames_since_reconcile += 1;
        LCD_HIP(h, h->applog.throttle(h->stream));
    }
    LCD_HIP(h, dreserve(h, h->d_out_wslot, (size_t)q * 4));
    if (app) {
        LCD_HIP(h, h->applog.activate(h->n_rows, h->stream, &h->bytes_device));
        { int rc = ensure_append_capacity(h, h->applog.rows_ub(h->n_rows) + 2 * (int64_t)q); if (rc) return rc; }
    }
    // 2-NN + same-frame distances, then ONE single-workgroup launch: decision loop -> pending retirements -> registration / idf
    ResolveArgs r;
    int rc = prepare_resolve(h, a->d_descriptors, q, a->flags, a->nndr_ratio, a->d_word_ids, h->d_out_wslot.as<int32_t>(), &r, true,
                             lazy ? h->applog.rows_ub(h->n_rows) : -1);
    if (rc) return rc;
    if (h->d_fail_count.p) { r.fail_count = h->d_fail_count.as<int32_t>(); h->fail_count_clean = true; }   // the tail resets the counters
    const uint64_t vseq = app ? h->applog.record(a->first_new_word_id, q, true) : 0;
    return frame_stage_s(h, *a, r, app, vseq);
}

extern "C" {

int lcd_frame_dev(lcd_engine* h, const lcd_frame_args* a) {
    LCD_TRY
    LCD_CHECK_HANDLE(h);
    FrameHostTimer timer__(h);
    lcd_engine::Range range__(h, "lcd_frame_dev");
    LCD_DEV_NODRAIN(h);
    return frame_dev_body(h, a);
    LCD_CATCH(h)
}

// where the host time of the pipelined lcd_frame_dev calls went so far (engine.h: host_prof): out9[0..7] ns per section, out9[8] calls.  Not part of lcd.h.
int lcd_debug_host_profile(const lcd_engine* h, int64_t* out9) {
    if (!h || !out9) return LCD_ERR_INVALID;
    for (int i = 0; i < 9; ++i) out9[i] = h->host_prof[i];
    return LCD_OK;
}

// The 2-NN stage of the LATEST frame as it stands on the device: rows, words and distances, [q x 2] each (capacity in queries; any of the three may be NULL),
// *out_q = its descriptor count.  Nothing is drained: behind lcd_synchronize these are the frame's final neighbours (exact redo included); on a pipelined
// handle right behind lcd_frame_dev they are the neighbours of the frame BEFORE the one just passed in (its launch B has run, its decision loop has not), and
// out_rejected = the queries its certificate sent to the exact redo (the decision loop resets that counter: 0 on a plain handle).  Tests; not part of lcd.h.
int lcd_debug_last_frame_knn(lcd_engine* h, int32_t* out_row, int32_t* out_word, float* out_dist, int capacity, int* out_q, int* out_rejected) {
    LCD_TRY
    LCD_CHECK_HANDLE(h);
    LCD_DEV_NODRAIN(h);
    if (!out_q) return LCD_ERR_INVALID;
    *out_q = h->dbg_knn_q;
    if (out_rejected) *out_rejected = 0;
    if (h->dbg_knn_q <= 0 || !h->dbg_knn_row) return LCD_OK;
    if (capacity < h->dbg_knn_q) return h->fail(LCD_ERR_INVALID, "lcd_debug_last_frame_knn: capacity below the frame's descriptor count");
    LCD_HIP(h, hipStreamSynchronize(h->stream));
    if (h->kst && h->kst != h->stream) LCD_HIP(h, hipStreamSynchronize(h->kst));
    const size_t bytes = (size_t)h->dbg_knn_q * 2 * 4;
    if (out_row) LCD_HIP(h, hipMemcpy(out_row, h->dbg_knn_row, bytes, hipMemcpyDeviceToHost));
    if (out_word) LCD_HIP(h, hipMemcpy(out_word, h->dbg_knn_word, bytes, hipMemcpyDeviceToHost));
    if (out_dist) LCD_HIP(h, hipMemcpy(out_dist, h->dbg_knn_dist, bytes, hipMemcpyDeviceToHost));
    if (out_rejected && h->last_fail_count) LCD_HIP(h, hipMemcpy(out_rejected, h->last_fail_count, 4, hipMemcpyDeviceToHost));
    return LCD_OK;
    LCD_CATCH(h)
}

int lcd_slot_count(const lcd_engine* h, int64_t* n_slots) {
    if (!h || !n_slots) return LCD_ERR_INVALID;
    *n_slots = h->tfidf.n_slots + h->pipe.owed_sigs();
    return LCD_OK;
}

int lcd_frame_host(lcd_engine* h, const lcd_frame_host_args* a) {
    LCD_TRY
    LCD_CHECK_HANDLE(h);
    lcd_engine::Range range__(h, "lcd_frame_host");
    LCD_DEV(h);                                                      // completes what a pipelined handle owes
    if (!a || a->struct_size != (int32_t)sizeof(lcd_frame_host_args)) return h->fail(LCD_ERR_INVALID, "lcd_frame_host: bad argument block");
    const int q = a->q;
    if (q <= 0 || q > 8192 || !a->descriptors || !a->word_ids) return h->fail(LCD_ERR_INVALID, "lcd_frame_host: bad argument");
    if (rows_padded(h)) return h->fail(LCD_ERR_UNSUPPORTED, "lcd_frame_host: rows of this size are padded on the device (use lcd_quantize)");
    const int64_t slots_after = h->tfidf.n_slots + (a->sig_id != 0 ? 1 : 0);
    if (a->likelihood && a->likelihood_capacity < slots_after) return h->fail(LCD_ERR_INVALID, "lcd_frame_host: likelihood buffer too small");
    // descriptors: host -> pinned staging -> device, on the engine's stream (the one synchronisation at the end frees the staging)
    const size_t dbytes = (size_t)q * h->row_bytes;
    LCD_HIP(h, h->h_frame_in.reserve(dbytes));
    std::memcpy(h->h_frame_in.p, a->descriptors, dbytes);
    LCD_HIP(h, dreserve(h, h->d_frame_desc, std::max<size_t>(dbytes, 16)));
    LCD_HIP(h, dreserve(h, h->d_frame_words, (size_t)q * 4));
    if (a->likelihood) LCD_HIP(h, dreserve(h, h->d_frame_like, (size_t)std::max<int64_t>(slots_after, 1) * 4));
    LCD_HIP(h, hipMemcpyAsync(h->d_frame_desc.p, h->h_frame_in.p, dbytes, hipMemcpyHostToDevice, h->stream));
    // from here on a copy out of / into the pinned staging may be in flight: a failure synchronises before it returns (the next call --
    // the mirror falls back to the call-by-call path on the same engine straight away -- reuses h_frame_in / h_frame_out)
    auto bail = [&](int rc) { (void)hipStreamSynchronize(h->stream); return rc; };
#define LCD_HIP_B(h, call) do { hipError_t e__ = (call); if (e__ != hipSuccess) return bail((h)->hip_fail(e__, #call)); } while (0)
    lcd_frame_args fa;
    std::memset(&fa, 0, sizeof(fa));
    fa.struct_size = (int32_t)sizeof(fa); fa.q = q; fa.d_descriptors = h->d_frame_desc.p; fa.flags = a->flags; fa.nndr_ratio = a->nndr_ratio;
    fa.sig_id = a->sig_id; fa.first_new_word_id = a->first_new_word_id; fa.N = a->N; fa.append_new_words = a->append_new_words;
    fa.d_word_ids = h->d_frame_words.as<int32_t>();
    if (a->likelihood) { fa.d_likelihood = h->d_frame_like.as<float>(); fa.likelihood_capacity = (int64_t)(h->d_frame_like.cap / 4); }
    { int rc = frame_dev_body(h, &fa); if (rc) return bail(rc); }
    { int rc = h->drain(false); if (rc) return bail(rc); }            // a pipelined handle: the frame's stages stand-alone (the row mirror is not needed here)
    const size_t wbytes = (size_t)q * 4, lbytes = a->likelihood ? (size_t)slots_after * 4 : 0;
    LCD_HIP_B(h, h->h_frame_out.reserve(wbytes + lbytes + 16));
    LCD_HIP_B(h, hipMemcpyAsync(h->h_frame_out.p, h->d_frame_words.p, wbytes, hipMemcpyDeviceToHost, h->stream));
    if (lbytes) LCD_HIP_B(h, hipMemcpyAsync((char*)h->h_frame_out.p + wbytes, h->d_frame_like.p, lbytes, hipMemcpyDeviceToHost, h->stream));
    LCD_HIP(h, hipStreamSynchronize(h->stream));
#undef LCD_HIP_B
    std::memcpy(a->word_ids, h->h_frame_out.p, wbytes);
    if (lbytes) std::memcpy(a->likelihood, (const char*)h->h_frame_out.p + wbytes, lbytes);
    if (a->n_slots) *a->n_slots = slots_after;
    // The word ids are here and the stream is idle: the rows this frame appended on the device are known without asking the device's log
    // (the k-th new word carries the code -(k + 1)), so the host's row mirror catches up now -- the next call finds nothing to reconcile
    // (a synchronisation and two small blocking copies less per frame).  Only when this frame is the one unreconciled appender, with ids the
    // caller gave: the postings keys of words numbered on the device are learnt from the rows (reconcile(), at the next drain).
    const AppendLog::DevAppend* e = h->applog.unreconciled.size() == 1 ? &h->applog.unreconciled.front() : nullptr;
    if (e && e->enabled && e->own.world == 0 && e->first_id > 0 && !h->rm_pending) {
        int n_new = 0;
        for (int i = 0; i < q; ++i) n_new = std::max(n_new, -a->word_ids[i]);
        const AppendLog::Report r = h->applog.report();
        if (r.tag == (uint32_t)(e->seq + 1) && r.rows == h->n_rows + n_new) {
            for (int k = 0; k < n_new; ++k) { h->mirror.push(AppendLog::id_of(*e, k, h->n_rows), h->n_rows); h->n_rows += 1; h->n_live += 1; }
            h->applog.unreconciled.clear();
            h->frames_since_reconcile = 0;                               // (what reconcile() leaves: nothing is owed to the mirror)
        }
    }
    return LCD_OK;
    LCD_CATCH(h)
}

}  // extern "C"
