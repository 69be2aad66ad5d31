// engine.hip -- implementation of the C-ABI declared in include/lcd.h (liblcd_hip.so).
//
// Host-side orchestration only: device memory, staging, stream ordering and the bookkeeping that keeps the
// vocabulary row order (the distance tie-break of the reference) and the signature/word slot maps.  All arithmetic
// of the hot path runs in the gfx950 kernels (knn2_kernels.hip, resolve_kernels.hip, tfidf.hip).  There is no CPU
// fallback: every entry point either runs on the device or returns an error status.
// Here: the handle's life cycle, vocabulary, signatures, stand-alone search / quantise, Bayes, the sharded stages, profiling, options,
// statistics.  The per-frame path (lcd_frame_dev, lcd_frame_host, lcd_engine::drain) is frame_pipeline.hip.
#include "engine_impl.h"
#include <dlfcn.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>
#include <numeric>
#include <unordered_map>

using namespace lcd;

static_assert(sizeof(lcd::HypothesisOut) == sizeof(lcd_hypothesis), "lcd_hypothesis is the kernel's output record");

// ---- the host's row mirror (engine.h)
int RowMirror::find(int32_t word_id) {
    if (rows_sorted) {
        auto it = std::lower_bound(h_row_key.begin(), h_row_key.end(), word_id);
        if (it == h_row_key.end() || *it != word_id) return -1;
        const int r = (int)(it - h_row_key.begin());
        return h_row_live[r] ? r : -1;
    }
    if (!word_row_valid) {
        word_row.clear();
        word_row.reserve(h_row_key.size() * 2);
        for (size_t r = 0; r < h_row_key.size(); ++r) if (h_row_live[r]) word_row[h_row_key[r]] = (int32_t)r;
        word_row_valid = true;
    }
    auto it = word_row.find(word_id);
    return it == word_row.end() ? -1 : it->second;
}

void RowMirror::push(int32_t id, int64_t row) {
    if (rows_sorted && !h_row_key.empty() && id <= h_row_key.back()) rows_sorted = false;   // out-of-order id
    if (word_row_valid) word_row[id] = (int32_t)row;
    h_row_key.push_back(id);
    if (id >= next_word_id) next_word_id = id + 1;
    h_row_live.push_back(1);
}

void RowMirror::kill(int64_t row) {
    h_row_live[(size_t)row] = 0;
    if (word_row_valid) word_row.erase(h_row_key[(size_t)row]);
}

void RowMirror::reset(std::vector<int32_t>& keys) {
    h_row_key.swap(keys);
    h_row_live.assign(h_row_key.size(), 1);
    rows_sorted = true;
    word_row.clear();
    word_row_valid = false;
}

// The sharded stages between a frame that appended on the device and the next one need no exact row mirror: the search plans for rows_ub() (the
// rows behind the device's count carry +inf norms, a zero operand split and row id 0: no scan ranks them), the index calls do not look at rows
// at all.  Round 6: they complete what is owed WITHOUT reconciling (drain(false)) -- the per-frame synchronisation of the sharded path -- as long
// as the append log has room and the caller is within 8 frames of the device (the bound grows by q per unreported frame).
static int drain_keep_rows_lazy(lcd_engine* h) {
    { int rc = h->drain(false); if (rc) return rc; }
    const bool lazy = h->applog.vcnt_active && h->shard_append && !h->rm_pending && !h->applog.must_reconcile(h->rm_pending, h->frames_since_reconcile);
    if (!lazy) return h->reconcile();
    LCD_HIP(h, h->applog.throttle(h->stream));
    return LCD_OK;
}

int lcd_engine::sync_all() {
    hipError_t e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return hip_fail(e, "hipStreamSynchronize(stream)");
    return LCD_OK;
}

namespace {

// copy `rows` host rows (h->dim columns) into a device buffer laid out with h->row_bytes per row (u8 rows zero-padded)
int upload_rows(lcd_engine* h, const void* rows, int n, DevBuf& dst) {
    const size_t bytes = (size_t)n * h->row_bytes;
    LCD_HIP(h, dreserve(h, dst, std::max<size_t>(bytes, 4)));
    if (n == 0) return LCD_OK;
    LCD_HIP(h, h->h_in.reserve(bytes));
    pack_rows(h->h_in.p, rows, n, host_row_bytes(h), (size_t)h->row_bytes);
    LCD_HIP(h, hipMemcpyAsync(dst.p, h->h_in.p, bytes, hipMemcpyHostToDevice, h->stream));
    // the staging buffer is reused by the next call: the copy must have left it
    LCD_HIP(h, hipStreamSynchronize(h->stream));
    return LCD_OK;
}

// the exact redo of rejected queries is left to the caller's next launch (the fused frame tail): describe it
static void fill_redo(lcd_engine* h, RowparArgs* a, const void* vocab, const int32_t* row_id, int n_rows, const void* d_queries, int32_t* o_row,
                      int32_t* o_word, float* o_dist, const CandBits* cb) {
    a->enabled = 1; a->vocab = (const float*)vocab; a->row_id = row_id; a->n_rows = n_rows; a->queries = (const float*)d_queries;
    a->fail_list = h->d_fail_list.as<int32_t>(); a->partial = (unsigned long long*)h->d_partial3.p;
    a->out_row = o_row; a->out_word = o_word; a->out_dist = o_dist;
    if (cb) a->cb = *cb;
}

// The partial keys [n_blocks][2][qpad] of an exact search, into d_partial; *pm is what the merge launches read.  The main vocabulary of a u8 handle in
// LCD_KNN_HAMMING_MFMA mode is searched on the matrix cores from 256 rows on (the threshold of the float matrix-core modes), everything else by the scan.
static int scan_partial(lcd_engine* h, const void* d_queries, int q, const void* vocab, const int32_t* row_id, int64_t n_rows, bool main_vocab, KnnPlan* pm) {
    const bool prof = main_vocab && h->prof_cap > 0 && h->prof_n < h->prof_cap;
    const bool hmfma = main_vocab && h->hamming_mfma && h->dtype == LCD_U8 && n_rows >= 256;
    const HammingMfmaPlan hp = hmfma ? knn_hamming_mfma_plan(q, (int)n_rows, h->row_bytes, h->filter_units > 0 ? h->filter_units : -1) : HammingMfmaPlan{};
    *pm = hmfma ? knn_hamming_mfma_merge_plan(hp) : knn_plan(q, (int)n_rows, h->row_bytes);
    LCD_HIP(h, dreserve(h, h->d_partial, hmfma ? knn_hamming_mfma_partial_bytes(hp) : knn_partial_bytes(*pm)));
    if (prof) LCD_HIP(h, hipEventRecord(h->prof_ev[2 * h->prof_n], h->kst));
    if (hmfma) LCD_HIP(h, launch_knn2_hamming_mfma(vocab, row_id, d_queries, hp, h->d_partial.as<uint64_t>(), h->kst));
    else LCD_HIP(h, launch_knn2_partial(h->dtype, h->kdim, vocab, row_id, d_queries, *pm, h->d_partial.as<uint64_t>(), h->kst));
    if (prof) {
        LCD_HIP(h, hipEventRecord(h->prof_ev[2 * h->prof_n + 1], h->kst));
        h->prof_n += 1;
        h->prof_kernel = hmfma ? "knn2_hamming_mfma_kernel" : h->dtype == LCD_F32 ? "knn2_l2_kernel" : "knn2_hamming_kernel";
    }
    return LCD_OK;
}

// 2-NN of q device-resident queries against a row matrix -> o_{row,word,dist}[q*2].  `main_vocab` selects the resident
// vocabulary (which has row norms and may use the MFMA filter); other matrices (findNN's not-indexed words) use the exact scan.
int run_knn2_raw(lcd_engine* h, const void* d_queries, int q, const void* vocab, const int32_t* row_id, int64_t n_rows, bool main_vocab,
                 int32_t* o_row, int32_t* o_word, float* o_dist, const CandBits* cb = nullptr, RowparArgs* defer_redo = nullptr,
                 const ShardPackArgs* pack = nullptr /* a sharded search: the candidate records ride in the redo's launch ... */,
                 bool* packed = nullptr /* ... when the search has one (matrix-core filter): told here */) {
    if (packed) *packed = false;
    if (q == 0) return LCD_OK;
    const bool mfma = main_vocab && h->knn_mode != 0 && knn_mfma_supported(h->dtype, h->kdim) && n_rows >= 256;
    // (a handle of 128- or 256-float rows whose caller wrote LCD_KNN_BF16X3 or LCD_KNN_F16; a search the plan cannot describe stays on the scan)
    WidePlan wp;
    const bool wide = !mfma && main_vocab && h->wide_mfma && n_rows >= 256 && n_rows <= 0x7fffffff &&
                      knn_wide_mfma_plan(q, (int)n_rows, h->kdim, h->filter_units > 0 ? h->filter_units : -1, &wp);
    if (mfma && h->bf_family()) {
        MfmaPlan mp = knn_bf16_plan(q, (int)n_rows, cb != nullptr ? knn_selfdist_wgs(q) : 0);
        mp.filter_units = h->filter_units;
        mp.f16 = h->f16();
        LCD_HIP(h, dreserve(h, h->d_partial2, knn_bf16_partial_bytes(mp)));
        LCD_HIP(h, dreserve(h, h->d_fail_list, (size_t)q * 4));
        const bool prof = h->prof_cap > 0 && h->prof_n < h->prof_cap;
        LCD_HIP(h, launch_knn_bf16(h->kdim, vocab, h->vocab_bf.p, h->row_norm.as<float>(), h->norm_max.as<uint32_t>(), row_id, d_queries, mp,
                                   h->d_partial2.p, o_row, o_word, o_dist, h->d_fail_list.as<int32_t>(), h->d_fail_count.as<int32_t>(),
                                   h->kst, prof ? h->prof_ev[2 * h->prof_n] : nullptr, prof ? h->prof_ev[2 * h->prof_n + 1] : nullptr,
                                   !h->fail_count_clean, cb, cb != nullptr));
        h->fail_count_clean = false;
        if (prof) { h->prof_n += 1; h->prof_kernel = h->f16() ? (knn_bf16_persistent(mp) ? "knn_bf16_filter_kernel_p (fp16 operands)" : "knn_bf16_filter_kernel (fp16 operands)")
                                                             : (knn_bf16_persistent(mp) ? "knn_bf16_filter_kernel_p" : "knn_bf16_filter_kernel"); }
        LCD_HIP(h, dreserve(h, h->d_partial3, knn_rowpar_partial_bytes((int)n_rows, q)));
        if (defer_redo) fill_redo(h, defer_redo, vocab, row_id, (int)n_rows, d_queries, o_row, o_word, o_dist, cb);
        else {
            LCD_HIP(h, launch_knn_rowpar(h->kdim, vocab, row_id, (int)n_rows, d_queries, h->d_fail_list.as<int32_t>(),
                                         h->d_fail_count.as<int32_t>(), h->d_partial3.p, o_row, o_word, o_dist, h->kst, cb, pack));
            if (pack && packed) *packed = true;
        }
    } else if (mfma) {
        const MfmaPlan mp = knn_mfma_plan(q, (int)n_rows);
        LCD_HIP(h, dreserve(h, h->d_partial2, knn_mfma_partial_bytes(mp)));
        LCD_HIP(h, dreserve(h, h->d_fail_list, (size_t)q * 4));
        const bool prof = h->prof_cap > 0 && h->prof_n < h->prof_cap;
        if (cb) LCD_HIP(h, launch_selfdist(h->dtype, h->kdim, d_queries, q, const_cast<float*>(cb->selfdist), cb->ld, h->kst));
        LCD_HIP(h, launch_knn_mfma(h->kdim, vocab, h->row_norm.as<float>(), h->norm_max.as<uint32_t>(), row_id, d_queries, mp, h->d_partial2.p,
                                   o_row, o_word, o_dist, h->d_fail_list.as<int32_t>(), h->d_fail_count.as<int32_t>(), h->kst,
                                   prof ? h->prof_ev[2 * h->prof_n] : nullptr, prof ? h->prof_ev[2 * h->prof_n + 1] : nullptr,
                                   !h->fail_count_clean, cb));
        h->fail_count_clean = false;
        if (prof) { h->prof_n += 1; h->prof_kernel = "knn_mfma_filter_kernel"; }
        // the queries the certificate rejected are redone exactly by the row-parallel kernel (usually none: it leaves at once)
        LCD_HIP(h, dreserve(h, h->d_partial3, knn_rowpar_partial_bytes((int)n_rows, q)));
        if (defer_redo) fill_redo(h, defer_redo, vocab, row_id, (int)n_rows, d_queries, o_row, o_word, o_dist, cb);
        else {
            LCD_HIP(h, launch_knn_rowpar(h->kdim, vocab, row_id, (int)n_rows, d_queries, h->d_fail_list.as<int32_t>(),
                                         h->d_fail_count.as<int32_t>(), h->d_partial3.p, o_row, o_word, o_dist, h->kst, cb, pack));
            if (pack && packed) *packed = true;
        }
    } else if (wide) {
        // rows of 128 / 256 floats, LCD_KNN_BF16X3 / LCD_KNN_F16 asked for: the stateless matrix-core filter, its re-rank and the exact redo.  cb,
        // defer_redo and pack are not looked at, exactly as in the scan branch below (the callers' own launches follow)
        LCD_HIP(h, dreserve(h, h->d_partial2, knn_wide_partial_bytes(wp)));
        LCD_HIP(h, dreserve(h, h->d_fail_list, (size_t)q * 4));
        LCD_HIP(h, dreserve(h, h->d_partial3, knn_rowpar_partial_bytes((int)n_rows, q)));
        LCD_HIP(h, dreserve(h, h->d_wide_norm, 64));
        const bool prof = h->prof_cap > 0 && h->prof_n < h->prof_cap;
        LCD_HIP(h, launch_knn_wide(wp, h->f16(), vocab, row_id, d_queries, h->d_partial2.p, h->d_partial3.p, h->d_wide_norm.as<uint32_t>(), o_row, o_word,
                                   o_dist, h->d_fail_list.as<int32_t>(), h->d_fail_count.as<int32_t>(), h->kst, prof ? h->prof_ev[2 * h->prof_n] : nullptr,
                                   prof ? h->prof_ev[2 * h->prof_n + 1] : nullptr, !h->fail_count_clean));
        h->fail_count_clean = false;
        if (prof) { h->prof_n += 1; h->prof_kernel = h->f16() ? "knn_wide_filter_kernel (fp16 operands)" : "knn_wide_filter_kernel"; }
    } else {
        KnnPlan pm;
        const int rc = scan_partial(h, d_queries, q, vocab, row_id, n_rows, main_vocab, &pm);
        if (rc) return rc;
        LCD_HIP(h, launch_knn2_merge(h->dtype, pm, h->d_partial.as<uint64_t>(), row_id, o_row, o_word, o_dist, h->kst));
    }
    h->knn_launches += 1;
    if (mfma || wide) h->last_fail_count = h->d_fail_count.p;
    return LCD_OK;
}

int run_knn2(lcd_engine* h, const void* d_queries, int q, const void* vocab, const int32_t* row_id, const int32_t* row_wslot,
             int64_t n_rows, DevBuf& o_row, DevBuf& o_word, DevBuf& o_dist) {
    (void)row_wslot;
    LCD_HIP(h, dreserve(h, o_row, (size_t)std::max(q, 1) * 2 * 4));
    LCD_HIP(h, dreserve(h, o_word, (size_t)std::max(q, 1) * 2 * 4));
    LCD_HIP(h, dreserve(h, o_dist, (size_t)std::max(q, 1) * 2 * 4));
    return run_knn2_raw(h, d_queries, q, vocab, row_id, n_rows, vocab == h->vocab.p, o_row.as<int32_t>(), o_word.as<int32_t>(),
                        o_dist.as<float>());
}

int download(lcd_engine* h, void* dst, const void* d_src, size_t bytes, PinBuf& pin) {
    if (!bytes) return LCD_OK;
    LCD_HIP(h, pin.reserve(bytes));
    LCD_HIP(h, hipMemcpyAsync(pin.p, d_src, bytes, hipMemcpyDeviceToHost, h->stream));
    LCD_HIP(h, hipStreamSynchronize(h->stream));
    std::memcpy(dst, pin.p, bytes);
    return LCD_OK;
}

}  // namespace

// the host's row mirror catches up with the device (synchronises)
int lcd_engine::reconcile() {
    if (applog.unreconciled.empty() && !rm_pending) return LCD_OK;
    { int rc = sync_all(); if (rc) return rc; }
    const int VLOG = AppendLog::VLOG;
    std::vector<int32_t> log((size_t)VLOG);
    if (!applog.unreconciled.empty()) {   // the log is a ring: the entries of the frames to catch up with form at most two stretches of it
        const size_t first = (size_t)(applog.unreconciled.front().seq % VLOG), n = applog.unreconciled.size();
        const size_t n1 = std::min(n, (size_t)VLOG - first);
        hipError_t e = hipMemcpy(log.data() + first, applog.log_slot(first), n1 * 4, hipMemcpyDeviceToHost);
        if (e == hipSuccess && n > n1) e = hipMemcpy(log.data(), applog.log_slot(0), std::min(n - n1, (size_t)VLOG) * 4, hipMemcpyDeviceToHost);
        if (e != hipSuccess) return hip_fail(e, "hipMemcpy(append log)");
    }
    std::vector<std::pair<int64_t, int> > auto_rows;
    for (const AppendLog::DevAppend& a : applog.unreconciled) {
        if (!a.enabled) continue;
        const int n = log[(size_t)(a.seq % VLOG)];
        applog.est_new = std::max(applog.est_new * 0.9, (double)n);             // (the estimate the launch plans and the shadow-score switch use: rows_plan() only sees it move while frames are in flight)
        const int64_t rows0 = n_rows;
        for (int k = 0; k < n; ++k) {
            const int32_t id = AppendLog::id_of(a, k, n_rows);
            if (!AppendLog::owns(a, id)) continue;                    // a sharded append: n is the frame's total, this rank wrote the ids it owns
            mirror.push(id, n_rows);
            n_rows += 1; n_live += 1;
        }
        if (a.first_id <= 0 && n_rows > rows0) auto_rows.push_back(std::pair<int64_t, int>(rows0, (int)(n_rows - rows0)));
    }
    if (!auto_rows.empty()) {
        // words numbered on the device: the host learns their postings keys from the rows themselves, in ONE copy (with ids the caller supplies
        // the reservation check pairs them; here nobody knew the ids when the keys were reserved)
        const int64_t r0 = auto_rows.front().first;
        std::vector<int32_t> keys((size_t)(n_rows - r0));
        hipError_t e = hipMemcpy(keys.data(), row_wslot.as<int32_t>() + r0, keys.size() * 4, hipMemcpyDeviceToHost);
        if (e != hipSuccess) return hip_fail(e, "hipMemcpy(row keys)");
        for (const std::pair<int64_t, int>& ar : auto_rows)
            for (int k = 0; k < ar.second; ++k) tfidf.keys.adopt_key(mirror.key(ar.first + k), keys[(size_t)(ar.first + k - r0)]);
    }
    applog.unreconciled.clear();
    applog.auto_window = false;
    if (rm_pending) {
        // rows tombstoned by the device-side cleanUnusedWords since the last reconciliation: the words are gone (removeWords,
        // VWDictionary.cpp:1595-1607), their postings keys go to the batched check that recycles them once nothing references them
        int32_t cnt = 0;
        hipError_t e = hipMemcpy(&cnt, d_rmlog.p, 4, hipMemcpyDeviceToHost);
        if (e != hipSuccess) return hip_fail(e, "hipMemcpy(removal log)");
        const int64_t cap = ((int64_t)(d_rmlog.cap / 4) - 16) / 2;
        const int64_t n = std::min<int64_t>(cnt, cap);
        if (n > rm_seen) {
            std::vector<int32_t> ent((size_t)(n - rm_seen) * 2);
            e = hipMemcpy(ent.data(), d_rmlog.as<int32_t>() + 16 + 2 * rm_seen, ent.size() * 4, hipMemcpyDeviceToHost);
            if (e != hipSuccess) return hip_fail(e, "hipMemcpy(removal log)");
            // every batched key check enqueued so far has finished (the stream is drained): with their verdicts in, a key is either the
            // word's permanent one -- released here -- or still on its way through the reservation checks, which will find it free
            tfidf.keys.harvest_released(true);
            e = tfidf.keys.rows_unlog_keys(d_rmlog.as<int32_t>() + 16 + 2 * rm_seen, (int)(n - rm_seen));   // nothing is in flight: the keys may circulate again
            if (e != hipSuccess) return hip_fail(e, "wrow_unlog_kernel");
            for (size_t i = 0; i < ent.size(); i += 2) {
                const int32_t r = ent[i];
                if (r < 0 || r >= n_rows || !mirror.live(r)) continue;
                const int32_t id = mirror.key(r);
                mirror.kill(r);
                n_live -= 1;
                tfidf.keys.forget_word(id, ent[i + 1]);
            }
            rm_seen = n;
        }
        rm_pending = false;
    }
    frames_since_reconcile = 0;
    return LCD_OK;
}

int lcd_engine::enqueue_clean(const int32_t* reg_cnt) {
    const int64_t rows = applog.rows_ub(n_rows);
    if (rows <= 0) return LCD_OK;
    hipError_t e = tfidf.flush_retire();                 // retirements ride with the next registration otherwise: the counts would be stale
    if (e != hipSuccess) return hip_fail(e, "flush_retire");
    const size_t need = ((size_t)std::max<int64_t>(rows, (int64_t)(vocab.cap / (size_t)row_bytes)) * 2 + 16) * 4;   // a row is logged at most once
    if (need > d_rmlog.cap) {
        const bool fresh = d_rmlog.p == nullptr;
        e = d_rmlog.reserve(need, d_rmlog.cap, stream, &bytes_device);
        if (e == hipSuccess && fresh) e = hipMemsetAsync(d_rmlog.p, 0, 64, stream);
        if (e != hipSuccess) return hip_fail(e, "removal log");
    }
    e = launch_clean_unused(row_id.as<int32_t>(), row_wslot.as<int32_t>(), tfidf.keys.nw.as<uint32_t>(), tfidf.keys.wrow.as<uint32_t>(),
                            dtype == LCD_F32 ? row_norm.as<float>() : nullptr, (int)rows, applog.vcnt_active ? applog.d_vcnt.as<int32_t>() : nullptr,
                            applog.vcnt_active ? reg_cnt : nullptr, d_rmlog.as<int32_t>(), (int)((d_rmlog.cap / 4 - 16) / 2), stream);
    if (e != hipSuccess) return hip_fail(e, "clean_unused_kernel");
    rm_pending = true;
    return LCD_OK;
}

// device part of addNewWords up to (not including) the decision loop: 2-NN, same-frame distances + candidate bits.
// Fills the decision loop's arguments.
int prepare_resolve(lcd_engine* h, const void* d_desc, int q, int flags, float nndr, int32_t* d_out_word, int32_t* d_out_wslot,
                    ResolveArgs* r, bool defer_redo, int64_t rows_now) {
    r->rp = RowparArgs{};
    if (rows_now < 0) rows_now = h->n_rows;
    const int have_index = h->n_live >= 2 ? 1 : 0;                  // VWDictionary.cpp:1015
    const bool incremental = (flags & LCD_Q_INCREMENTAL) != 0;
    const bool together = incremental && (flags & LCD_Q_NEW_WORDS_COMPARED);
    int ld = (q + 63) / 64 * 64;
    const int bw = ld / 32;
    if (together) {
        LCD_HIP(h, dreserve(h, h->d_selfdist, (size_t)q * ld * 4));
        LCD_HIP(h, dreserve(h, h->d_bits, cand_bits_bytes(q, bw)));
    }
    // With the MFMA filter the same-frame distance matrix does not wait for the 2-NN: extra workgroups of the filter launch
    // compute it, and the re-rank workgroup of a query -- the first to know the query's second neighbour -- derives the query's
    // candidate bits from its (symmetric) row: two launches fewer per frame.
    const int64_t knn_rows = have_index ? rows_now : 0;
    const bool side = together && h->knn_mode != 0 && knn_mfma_supported(h->dtype, h->kdim) && knn_rows >= 256 && q > 0;
    int rc;
    if (side) {
        CandBits cb;
        cb.selfdist = h->d_selfdist.as<float>(); cb.ld = ld; cb.nq = q; cb.have_index = have_index;
        cand_bits_layout(cb, h->d_bits.as<uint32_t>(), q, bw);
        LCD_HIP(h, dreserve(h, h->d_knn_row, (size_t)q * 2 * 4));
        LCD_HIP(h, dreserve(h, h->d_knn_word, (size_t)q * 2 * 4));
        LCD_HIP(h, dreserve(h, h->d_knn_dist, (size_t)q * 2 * 4));
        rc = run_knn2_raw(h, d_desc, q, h->vocab.p, h->row_id.as<int32_t>(), knn_rows, true, h->d_knn_row.as<int32_t>(),
                          h->d_knn_word.as<int32_t>(), h->d_knn_dist.as<float>(), &cb, defer_redo ? &r->rp : nullptr);
        if (rc) return rc;
    } else if (together && h->dtype == LCD_U8 && q > 0) {
        // Hamming frames (config 3): the scan, then ONE launch for the merge of its partial keys, the same-frame distance matrix and the candidate
        // bit rows (round 6: they were two dependent launches of ~5 us each behind the scan)
        LCD_HIP(h, dreserve(h, h->d_knn_row, (size_t)q * 2 * 4));
        LCD_HIP(h, dreserve(h, h->d_knn_word, (size_t)q * 2 * 4));
        LCD_HIP(h, dreserve(h, h->d_knn_dist, (size_t)q * 2 * 4));
        KnnPlan p;
        rc = scan_partial(h, d_desc, q, h->vocab.p, h->row_id.as<int32_t>(), knn_rows, true, &p);
        if (rc) return rc;
        LCD_HIP(h, launch_knn2_merge_selfdist_hamming(p, h->d_partial.as<uint64_t>(), h->row_id.as<int32_t>(), h->d_knn_row.as<int32_t>(),
                                                      h->d_knn_word.as<int32_t>(), h->d_knn_dist.as<float>(), d_desc, h->kdim, h->d_selfdist.as<float>(), ld,
                                                      have_index, h->d_bits.as<uint32_t>(), bw, h->kst));
        h->knn_launches += 1;
    } else {
        rc = run_knn2(h, d_desc, q, h->vocab.p, h->row_id.as<int32_t>(), h->row_wslot.as<int32_t>(), knn_rows, h->d_knn_row, h->d_knn_word,
                      h->d_knn_dist);
        if (rc) return rc;
        if (together)
            LCD_HIP(h, launch_selfdist(h->dtype, h->kdim, d_desc, q, h->d_selfdist.as<float>(), ld, h->kst, have_index,
                                       h->d_knn_word.as<int32_t>(), h->d_knn_dist.as<float>(), h->d_bits.as<uint32_t>(), bw));
    }
    r->q = q;
    r->flags = (incremental ? LCD_Q_INCREMENTAL : 0) | (together ? LCD_Q_NEW_WORDS_COMPARED : 0);
    r->nndr = nndr;
    r->have_index = have_index;
    r->knn_word = h->d_knn_word.as<int32_t>();
    r->knn_dist = h->d_knn_dist.as<float>();
    r->selfdist = together ? h->d_selfdist.as<float>() : nullptr;
    r->ld = ld;
    r->cand_bits = together ? h->d_bits.as<uint32_t>() : nullptr;
    r->bw = bw;
    r->out_word = d_out_word;
    r->out_n_new = h->d_n_new.as<int32_t>();
    r->knn_row = h->d_knn_row.as<int32_t>();
    h->dbg_knn_row = h->d_knn_row.p; h->dbg_knn_word = h->d_knn_word.p; h->dbg_knn_dist = h->d_knn_dist.p; h->dbg_knn_q = q;
    r->row_wslot = h->row_wslot.as<int32_t>();
    r->out_wslot = d_out_wslot;
    r->new_ws = WsRuns();
    r->cand_list = nullptr; r->cand_cnt = nullptr;
    if (side) {                                                      // the re-rank also left the compact candidate lists
        CandBits lay;
        cand_bits_layout(lay, h->d_bits.as<uint32_t>(), q, bw);
        r->cand_list = lay.list; r->cand_cnt = lay.cnt;
    }
    r->fail_count = nullptr;
    return LCD_OK;
}

extern "C" {

int lcd_abi_version(void) { return LCD_ABI_VERSION; }

int lcd_create(const lcd_config* cfg, lcd_engine** out) {
    LCD_TRY
    if (!cfg || !out) return LCD_ERR_INVALID;
    *out = nullptr;
    if (cfg->struct_size != (int32_t)sizeof(lcd_config)) return LCD_ERR_INVALID;
    if (cfg->dim <= 0 || cfg->dim > 4096 || (cfg->dtype != LCD_F32 && cfg->dtype != LCD_U8)) return LCD_ERR_INVALID;
    if (cfg->knn_mode < LCD_KNN_DEFAULT || cfg->knn_mode > LCD_KNN_HAMMING_MFMA) return LCD_ERR_INVALID;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || cfg->device < 0 || cfg->device >= ndev) return LCD_ERR_HIP;
    if (hipSetDevice(cfg->device) != hipSuccess) return LCD_ERR_HIP;
    {   // the filter's launch plans fill THIS device's compute units (256 on MI355X; fewer on a partitioned part)
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, cfg->device) == hipSuccess && cus > 0) { knn_set_compute_units(cus); knn_hamming_mfma_set_compute_units(cus); }
    }
    lcd_engine* h = new (std::nothrow) lcd_engine();
    if (!h) return LCD_ERR_NOMEM;
    h->device = cfg->device;
    h->dtype = cfg->dtype;
    h->dim = cfg->dim;
    if (cfg->dtype == LCD_F32) { h->row_bytes = cfg->dim * 4; h->kdim = cfg->dim; }
    else { h->row_bytes = (cfg->dim + 3) / 4 * 4; h->kdim = h->row_bytes; }
    if (cfg->stream) { h->stream = (hipStream_t)cfg->stream; h->own_stream = false; }
    else {
        if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) { delete h; return LCD_ERR_HIP; }
        h->own_stream = true;
    }
    const int64_t vcap = cfg->vocab_capacity > 0 ? cfg->vocab_capacity : 4096;
    h->vocab_capacity_cfg = vcap;
    hipError_t e = h->vocab.reserve((size_t)vcap * h->row_bytes, 0, h->stream, &h->bytes_device);
    if (e == hipSuccess) e = h->row_id.reserve((size_t)vcap * 4, 0, h->stream, &h->bytes_device);
    if (e == hipSuccess) e = h->row_wslot.reserve((size_t)vcap * 4, 0, h->stream, &h->bytes_device);
    if (e == hipSuccess) e = h->d_n_new.reserve(64, 0, h->stream, &h->bytes_device);
    if (e == hipSuccess) e = h->norm_max.reserve(64, 0, h->stream, &h->bytes_device);
    if (e == hipSuccess) e = hipMemsetAsync(h->norm_max.p, 0, 64, h->stream);
    if (e == hipSuccess) e = h->row_norm.reserve(((size_t)vcap + 1) * 8, 0, h->stream, &h->bytes_device);
    if (e == hipSuccess) e = h->d_fail_count.reserve(64, 0, h->stream, &h->bytes_device);   // [0] rejected, [1] arrivals, [2] max err / eps
    if (e == hipSuccess) e = h->d_hyp_scratch.reserve(64, 0, h->stream, &h->bytes_device);
    if (e == hipSuccess) e = hipMemsetAsync(h->d_fail_count.p, 0, 64, h->stream);
    h->knn_mode = cfg->knn_mode == LCD_KNN_EXACT_VALU ? 0 : cfg->knn_mode == LCD_KNN_F32_MFMA ? 1 : cfg->knn_mode == LCD_KNN_F16 ? 3 : 2;
    h->hamming_mfma = cfg->knn_mode == LCD_KNN_HAMMING_MFMA && cfg->dtype == LCD_U8;   // (on an f32 handle the value means the default, above)
    // rows of 128 / 256 floats take the matrix-core path only when the caller WROTE one of its two modes (DEFAULT folds into knn_mode 2 above)
    h->wide_mfma = (cfg->knn_mode == LCD_KNN_BF16X3 || cfg->knn_mode == LCD_KNN_F16) && knn_wide_mfma_supported(cfg->dtype, cfg->dim);
    h->kst = h->stream;
    if (cfg->pipeline < 0 || cfg->pipeline > 1) { delete h; return LCD_ERR_INVALID; }
    h->pipeline = cfg->pipeline;
    if (cfg->pipeline) {
        for (FramePipeline::FrameScratch& sc : h->pipe.ring) {
            if (e == hipSuccess) e = sc.d_fail_count.reserve(64, 0, h->stream, &h->bytes_device);
            if (e == hipSuccess) e = hipMemsetAsync(sc.d_fail_count.p, 0, 64, h->stream);
            sc.fail_count_clean = true;
        }
    }
    if (e == hipSuccess) e = h->tfidf.init(h->stream, &h->bytes_device, cfg->sig_capacity, cfg->vocab_capacity);
    h->bayes.init(h->stream, &h->bytes_device);
    if (e != hipSuccess) { lcd_destroy(h); return LCD_ERR_HIP; }
    *out = h;
    return LCD_OK;
    LCD_CATCH((const lcd_engine*)nullptr)
}

void lcd_destroy(lcd_engine* h) {
    try {
    if (!h) return;
    (void)hipSetDevice(h->device);
    (void)h->drain();
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    h->tfidf.destroy();
    h->bayes.destroy();
    for (FramePipeline::FrameScratch& sc : h->pipe.ring) {
        DevBuf* all[] = {&sc.d_knn_row, &sc.d_knn_word, &sc.d_knn_dist, &sc.d_selfdist, &sc.d_bits, &sc.d_partial2, &sc.d_partial3, &sc.d_fail_list,
                         &sc.d_fail_count, &sc.d_out_wslot, &sc.d_qsplit, &sc.d_qnorm, &sc.d_applist, &sc.d_cross};
        for (DevBuf* d : all) d->release(&h->bytes_device);
    }
    for (hipEvent_t e : h->prof_ev) (void)hipEventDestroy(e);
    for (hipEvent_t e : h->prof2_ev) (void)hipEventDestroy(e);
    DevBuf* all[] = {&h->vocab, &h->row_id, &h->row_wslot, &h->vocab_alt, &h->row_id_alt, &h->row_wslot_alt, &h->d_queries,
                     &h->d_partial, &h->d_knn_row, &h->d_knn_word, &h->d_knn_wslot, &h->d_knn_dist, &h->d_selfdist, &h->d_out_word,
                     &h->d_out_wslot, &h->d_n_new, &h->d_tmp_i32, &h->d_extra_rows, &h->d_extra_id, &h->d_extra_word,
                     &h->d_extra_dist, &h->d_extra_row, &h->d_like, &h->d_slots, &h->d_bits, &h->row_norm, &h->norm_max, &h->d_partial2,
                     &h->d_fail_list, &h->d_fail_count, &h->d_partial3, &h->row_norm_alt, &h->vocab_bf, &h->d_hyp_scratch, &h->d_adj_scratch,
                     &h->d_shard_selfdist, &h->d_wide_norm};
    for (DevBuf* d : all) d->release(&h->bytes_device);
    h->applog.release(&h->bytes_device);
    h->d_rmlog.release(&h->bytes_device);
    h->pairs.release(&h->bytes_device);
    h->h_in.release(); h->h_out.release(); h->h_out2.release();
    if (h->own_stream && h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
    } catch (...) { }
}

const char* lcd_last_error(const lcd_engine* h) { return h ? h->err.c_str() : "null handle"; }

int lcd_synchronize(lcd_engine* h) {
    LCD_TRY
    LCD_CHECK_HANDLE(h);
    LCD_DEV_NODRAIN(h);
    // what the frames in flight owe is completed and awaited; the host's row mirror is NOT brought up to date here (nothing a caller can
    // observe after this call needs it: every call that does completes the reconciliation itself) -- two device reads less per call
    { int rc = h->drain(false); if (rc) return rc; }
    return h->sync_all();
    LCD_CATCH(h)
}

void* lcd_stream(lcd_engine* h) { return h ? (void*)h->stream : nullptr; }

int lcd_pipeline_depth(const lcd_engine* h) { return (h && h->pipeline) ? FramePipeline::DEPTH : 0; }

int lcd_record_event(lcd_engine* h, void* event) {
    LCD_TRY
    LCD_CHECK_HANDLE(h);
    if (!event) return h->fail(LCD_ERR_INVALID, "lcd_record_event: null event");
    LCD_DEV_NODRAIN(h);
    if (!h->pipe.empty()) { h->pipe.queue_event(event); return LCD_OK; }   // recorded behind the stages still owed
    LCD_HIP(h, hipEventRecord((hipEvent_t)event, h->stream));
    return LCD_OK;
    LCD_CATCH(h)
}

// ------------------------------------------------------------------------------------------------ vocabulary
int lcd_vocab_clear(lcd_engine* h) {
    LCD_TRY
    LCD_CHECK_HANDLE(h);
    LCD_DEV(h);
    { int rc = h->sync_all(); if (rc) return rc; }
    h->n_rows = 0; h->n_live = 0;
    h->applog.restart(); h->tail_filled_rows = 0;
    LCD_HIP(h, h->tfidf.keys.rows_clear());
    if (h->d_rmlog.p) LCD_HIP(h, hipMemsetAsync(h->d_rmlog.p, 0, 4, h->stream));
    h->rm_seen = 0;
    h->mirror.clear();
    return LCD_OK;
    LCD_CATCH(h)
}

int lcd_vocab_append(lcd_engine* h, const void* rows, int n, const int32_t* word_ids) {
    LCD_TRY
    LCD_CHECK_HANDLE(h);
    LCD_DEV(h);
    if (n < 0 || (n > 0 && (!rows || !word_ids))) return h->fail(LCD_ERR_INVALID, "lcd_vocab_append: null input");
    if (n == 0) return LCD_OK;
    { int rc = h->sync_all(); if (rc) return rc; }                   // the 2-NN stage of a pipelined frame may still read the vocabulary
    for (int i = 0; i < n; ++i) {
        if (word_ids[i] <= 0) return h->fail(LCD_ERR_INVALID, "lcd_vocab_append: word ids must be > 0");
        if (h->mirror.find(word_ids[i]) >= 0) return h->fail(LCD_ERR_STATE, "lcd_vocab_append: word already in the vocabulary");
    }
    {   // the same id twice in one call would create two live rows for one word
        std::vector<int32_t> sorted(word_ids, word_ids + n);
        std::sort(sorted.begin(), sorted.end());
        if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end())
            return h->fail(LCD_ERR_INVALID, "lcd_vocab_append: duplicate word id in the call");
    }
    const int64_t total = h->n_rows + n;
    if (total > 0x7FFFFFF0ll) return h->fail(LCD_ERR_UNSUPPORTED, "lcd_vocab_append: more than 2^31 rows");
    LCD_HIP(h, dreserve(h, h->vocab, (size_t)total * h->row_bytes, (size_t)h->n_rows * h->row_bytes));
    LCD_HIP(h, dreserve(h, h->row_id, (size_t)total * 4, (size_t)h->n_rows * 4));
    LCD_HIP(h, dreserve(h, h->row_wslot, (size_t)total * 4, (size_t)h->n_rows * 4));
    // stage rows | ids | wslots in one pinned block
    const size_t rb = (size_t)n * h->row_bytes;
    LCD_HIP(h, h->h_in.reserve(rb + (size_t)n * 8));
    char* st = (char*)h->h_in.p;
    const size_t src_row = (size_t)h->dim * (h->dtype == LCD_F32 ? 4 : 1);
    if (src_row == (size_t)h->row_bytes) std::memcpy(st, rows, rb);
    else {
        std::memset(st, 0, rb);
        for (int i = 0; i < n; ++i) std::memcpy(st + (size_t)i * h->row_bytes, (const char*)rows + (size_t)i * src_row, src_row);
    }
    int32_t* ids = (int32_t*)(st + rb);
    int32_t* ws = ids + n;
    for (int i = 0; i < n; ++i) {
        ids[i] = word_ids[i];
        LCD_HIP(h, h->tfidf.keys.key_of(word_ids[i], true, &ws[i]));
    }
    LCD_HIP(h, hipMemcpyAsync((char*)h->vocab.p + (size_t)h->n_rows * h->row_bytes, st, rb, hipMemcpyHostToDevice, h->stream));
    LCD_HIP(h, hipMemcpyAsync(h->row_id.as<int32_t>() + h->n_rows, ids, (size_t)n * 4, hipMemcpyHostToDevice, h->stream));
    LCD_HIP(h, hipMemcpyAsync(h->row_wslot.as<int32_t>() + h->n_rows, ws, (size_t)n * 4, hipMemcpyHostToDevice, h->stream));
    LCD_HIP(h, h->tfidf.keys.rows_take_keys(h->row_wslot.as<int32_t>() + h->n_rows, n, h->n_rows));
    if (h->dtype == LCD_F32) {   // |row|^2 for the MFMA filter
        LCD_HIP(h, dreserve(h, h->row_norm, ((size_t)total + 1) * 8, (size_t)h->n_rows * 8));
        LCD_HIP(h, launch_row_norms(h->vocab.p, h->row_id.as<int32_t>(), (int)h->n_rows, n, h->kdim, h->row_norm.as<float>(),
                                    h->norm_max.as<uint32_t>(), h->stream));
        if (knn_mfma_supported(h->dtype, h->kdim)) {   // hi/lo bf16 split of the new rows
            // (for the capacity the caller configured, like the other row buffers: a stream of appending frames must not meet a reallocation -- 32 MB copied
            // behind a synchronisation -- where this table alone was sized for the rows it was given: 125 000 rows fill a 32 MiB allocation to 131 072)
            LCD_HIP(h, dreserve(h, h->vocab_bf, (size_t)std::max<int64_t>(total, h->vocab_capacity_cfg) * 256, (size_t)h->n_rows * 256));
            LCD_HIP(h, launch_vocab_bf16(h->vocab.p, (int)h->n_rows, n, h->kdim, h->vocab_bf.p, h->stream, h->f16()));
        }
    }
    LCD_HIP(h, hipStreamSynchronize(h->stream));
    for (int i = 0; i < n; ++i) h->mirror.push(word_ids[i], h->n_rows + i);
    h->n_rows = total;
    h->n_live += n;
    h->applog.restart(); h->tail_filled_rows = 0;                    // the device row counters (appends by frames) start over from this count
    return LCD_OK;
    LCD_CATCH(h)
}

static int vocab_remove_ids(lcd_engine* h, const int32_t* word_ids, int n);

int lcd_vocab_remove(lcd_engine* h, const int32_t* word_ids, int n) {
    LCD_TRY
    LCD_CHECK_HANDLE(h);
    LCD_DEV(h);
    if (n < 0 || (n > 0 && !word_ids)) return h->fail(LCD_ERR_INVALID, "lcd_vocab_remove: null input");
    if (n == 0) return LCD_OK;
    return vocab_remove_ids(h, word_ids, n);
    LCD_CATCH(h)
}

int lcd_vocab_remove_unused(lcd_engine* h, int32_t* out_word_ids, int capacity, int32_t* out_n) {
    LCD_TRY
    LCD_CHECK_HANDLE(h);
    LCD_DEV(h);
    if (capacity < 0 || (capacity > 0 && !out_word_ids)) return h->fail(LCD_ERR_INVALID, "lcd_vocab_remove_unused: bad output buffer");
    if (out_n) *out_n = 0;
    if (h->n_rows == 0) return LCD_OK;
    LCD_HIP(h, h->tfidf.flush_retire());                             // retirements ride with the next frame otherwise: nw would be stale
    LCD_HIP(h, dreserve(h, h->d_tmp_i32, ((size_t)h->n_rows + 16) * 4));
    int32_t* d_cnt = h->d_tmp_i32.as<int32_t>();
    LCD_HIP(h, hipMemsetAsync(d_cnt, 0, 4, h->stream));
    LCD_HIP(h, launch_unused_rows(h->row_id.as<int32_t>(), h->row_wslot.as<int32_t>(), h->tfidf.keys.nw.as<uint32_t>(), (int)h->n_rows, d_cnt + 16, d_cnt,
                                  (int)h->n_rows, h->stream));
    int32_t n = 0;
    { int rc = download(h, &n, d_cnt, 4, h->h_out2); if (rc) return rc; }
    if (n <= 0) return LCD_OK;
    std::vector<int32_t> rows((size_t)n);
    { int rc = download(h, rows.data(), d_cnt + 16, (size_t)n * 4, h->h_out); if (rc) return rc; }
    std::sort(rows.begin(), rows.end());
    std::vector<int32_t> ids((size_t)n);
    for (int i = 0; i < n; ++i) ids[(size_t)i] = h->mirror.key(rows[(size_t)i]);
    { int rc = vocab_remove_ids(h, ids.data(), n); if (rc) return rc; }
    if (out_n) *out_n = n;
    for (int i = 0; i < n && i < capacity; ++i) out_word_ids[i] = ids[(size_t)i];
    return LCD_OK;
    LCD_CATCH(h)
}

int lcd_vocab_remove_unused_async(lcd_engine* h) {
    LCD_TRY
    LCD_CHECK_HANDLE(h);
    LCD_DEV_NODRAIN(h);
    // a pipelined handle still owes stages of its latest frames: the clean takes its place behind the newest of them (its registration
    // and the retirements asked for since), like lcd_sig_remove -- nothing is completed, nothing is synchronised
    if (!h->pipe.empty()) { h->pipe.queue_clean(); return LCD_OK; }
    return h->enqueue_clean();
    LCD_CATCH(h)
}

static int vocab_remove_ids(lcd_engine* h, const int32_t* word_ids, int n) {
    { int rc = h->sync_all(); if (rc) return rc; }
    std::vector<int32_t> rows;
    rows.reserve(n);
    for (int i = 0; i < n; ++i) {
        const int r = h->mirror.find(word_ids[i]);
        if (r >= 0) { rows.push_back(r); continue; }
        // not a row: a word that was created by a frame (_notIndexedWords) and dies before update() indexed it only gives its
        // postings key back (removeWords erases it from _notIndexedWords, :1602); anything else is an error
        int32_t ws = -1;
        LCD_HIP(h, h->tfidf.keys.key_of(word_ids[i], false, &ws));
        if (ws < 0) return h->fail(LCD_ERR_STATE, "lcd_vocab_remove: unknown word");
    }
    {   // the same word twice would be counted out of n_live twice
        std::vector<int32_t> sorted(rows);
        std::sort(sorted.begin(), sorted.end());
        if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end())
            return h->fail(LCD_ERR_INVALID, "lcd_vocab_remove: duplicate word id in the call");
    }
    const int nr = (int)rows.size();
    if (nr) {
        LCD_HIP(h, dreserve(h, h->d_tmp_i32, (size_t)nr * 4));
        LCD_HIP(h, h->h_in.reserve((size_t)nr * 4));
        std::memcpy(h->h_in.p, rows.data(), (size_t)nr * 4);
        LCD_HIP(h, hipMemcpyAsync(h->d_tmp_i32.p, h->h_in.p, (size_t)nr * 4, hipMemcpyHostToDevice, h->stream));
        LCD_HIP(h, h->tfidf.keys.rows_drop_keys(h->row_wslot.as<int32_t>(), h->d_tmp_i32.as<int32_t>(), nr));
        LCD_HIP(h, launch_tombstone(h->row_id.as<int32_t>(), h->d_tmp_i32.as<int32_t>(), nr, h->stream));
        if (h->dtype == LCD_F32) LCD_HIP(h, launch_norm_tombstone(h->row_norm.as<float>(), h->d_tmp_i32.as<int32_t>(), nr, h->stream));
        LCD_HIP(h, hipStreamSynchronize(h->stream));
        for (int i = 0; i < nr; ++i) h->mirror.kill(rows[i]);
        h->applog.restart();                                         // the counters restart: the next frame's filter sees every row (tombstones carry
                                                                     // +inf norms), its re-rank has no pending rows -- one of them might be gone now
        h->n_live -= nr;
    }
    // removeWords: the words are gone; their postings keys come back once the device has found them unreferenced
    LCD_HIP(h, h->tfidf.release_words(word_ids, n));
    return LCD_OK;
}

int lcd_vocab_rebuild(lcd_engine* h) {
    LCD_TRY
    LCD_CHECK_HANDLE(h);
    LCD_DEV(h);
    { int rc = h->sync_all(); if (rc) return rc; }
    // permutation: live rows ordered by ascending word id (VWDictionary.cpp:636-660 walks std::map<int,VisualWord*>).
    // Word ids only grow in normal operation, so the live rows are already ascending and this is a stable compaction;
    // the sort is only needed after out-of-order appends (re-activated old words).
    std::vector<int32_t> perm;
    perm.reserve((size_t)h->n_live);
    for (int64_t r = 0; r < h->n_rows; ++r) if (h->mirror.live(r)) perm.push_back((int32_t)r);
    if (!h->mirror.rows_sorted)
        std::stable_sort(perm.begin(), perm.end(), [&](int32_t a, int32_t b) { return h->mirror.key(a) < h->mirror.key(b); });
    const int n = (int)perm.size();
    if (n == (int)h->n_rows && h->mirror.rows_sorted) return LCD_OK;       // nothing to drop, nothing to reorder
    LCD_HIP(h, dreserve(h, h->vocab_alt, std::max<size_t>(h->vocab.cap, 4)));
    LCD_HIP(h, dreserve(h, h->row_id_alt, std::max<size_t>(h->row_id.cap, 4)));
    LCD_HIP(h, dreserve(h, h->row_wslot_alt, std::max<size_t>(h->row_wslot.cap, 4)));
    if (h->dtype == LCD_F32) LCD_HIP(h, dreserve(h, h->row_norm_alt, std::max<size_t>(h->row_norm.cap, 16)));
    if (n) {
        LCD_HIP(h, dreserve(h, h->d_tmp_i32, (size_t)n * 4));
        LCD_HIP(h, h->h_in.reserve((size_t)n * 4 + 16));
        std::memcpy(h->h_in.p, perm.data(), (size_t)n * 4);
        LCD_HIP(h, hipMemcpyAsync(h->d_tmp_i32.p, h->h_in.p, (size_t)n * 4, hipMemcpyHostToDevice, h->stream));
        LCD_HIP(h, launch_gather_rows(h->vocab.p, h->row_id.as<int32_t>(), h->d_tmp_i32.as<int32_t>(), n, h->row_bytes,
                                      h->vocab_alt.p, h->row_id_alt.as<int32_t>(), h->stream));
        LCD_HIP(h, launch_gather_rows(h->row_wslot.p, h->row_id.as<int32_t>(), h->d_tmp_i32.as<int32_t>(), n, 4,
                                      h->row_wslot_alt.p, h->row_id_alt.as<int32_t>(), h->stream));
        if (h->dtype == LCD_F32) {
            // the augmentation table ({|row|^2, 1} per row) moves with the rows; the sentinel entry follows the last row
            LCD_HIP(h, launch_gather_rows(h->row_norm.p, h->row_id.as<int32_t>(), h->d_tmp_i32.as<int32_t>(), n, 8,
                                          h->row_norm_alt.p, h->row_id_alt.as<int32_t>(), h->stream));
            float* sentinel = (float*)((char*)h->h_in.p + (size_t)n * 4);
            const uint32_t inf_bits = 0x7f800000u;
            std::memcpy(&sentinel[0], &inf_bits, 4);
            sentinel[1] = 1.0f;
            LCD_HIP(h, hipMemcpyAsync(h->row_norm_alt.as<float>() + 2 * (size_t)n, sentinel, 8, hipMemcpyHostToDevice, h->stream));
        }
        LCD_HIP(h, hipStreamSynchronize(h->stream));                 // staging buffer reuse
    }
    std::swap(h->vocab, h->vocab_alt);
    std::swap(h->row_id, h->row_id_alt);
    std::swap(h->row_wslot, h->row_wslot_alt);
    if (h->dtype == LCD_F32) std::swap(h->row_norm, h->row_norm_alt);
    LCD_HIP(h, h->tfidf.keys.rows_take_keys(h->row_wslot.as<int32_t>(), n, 0));   // the rows moved (the keys of dropped rows were released with them)
    if (h->d_rmlog.p) LCD_HIP(h, hipMemsetAsync(h->d_rmlog.p, 0, 4, h->stream));   // (reconciled by the drain above: the log starts over)
    h->rm_seen = 0;
    if (n && knn_mfma_supported(h->dtype, h->kdim)) {   // the split is recomputed from the compacted rows
        LCD_HIP(h, dreserve(h, h->vocab_bf, (size_t)n * 256));
        LCD_HIP(h, launch_vocab_bf16(h->vocab.p, 0, n, h->kdim, h->vocab_bf.p, h->stream, h->f16()));
    }
    std::vector<int32_t> keys(n);
    for (int i = 0; i < n; ++i) keys[i] = h->mirror.key(perm[i]);
    h->mirror.reset(keys);
    h->n_rows = n;
    h->n_live = n;
    h->applog.restart(); h->tail_filled_rows = 0;
    h->rebuilds += 1;
    return LCD_OK;
    LCD_CATCH(h)
}

int lcd_vocab_count(const lcd_engine* h, int64_t* rows, int64_t* live) {
    LCD_TRY
    LCD_CHECK_HANDLE(h);
    if (hipSetDevice(h->device) != hipSuccess) return LCD_ERR_HIP;
    { int rc = const_cast<lcd_engine*>(h)->drain(); if (rc) return rc; }   // rows appended on the device: the owed stages run, the mirror catches up
    if (rows) *rows = h->n_rows;
    if (live) *live = h->n_live;
    return LCD_OK;
    LCD_CATCH(h)
}

int lcd_vocab_read(lcd_engine* h, int64_t first, int n, void* out_rows, int32_t* out_word_ids) {
    LCD_TRY
    LCD_CHECK_HANDLE(h);
    LCD_DEV(h);
    if (first < 0 || n < 0 || first + n > h->n_rows) return h->fail(LCD_ERR_INVALID, "lcd_vocab_read: range");
    if (n == 0) return LCD_OK;
    if (out_rows) {
        const size_t bytes = (size_t)n * h->row_bytes;
        LCD_HIP(h, h->h_out.reserve(bytes));
        LCD_HIP(h, hipMemcpyAsync(h->h_out.p, (const char*)h->vocab.p + (size_t)first * h->row_bytes, bytes, hipMemcpyDeviceToHost, h->stream));
        LCD_HIP(h, hipStreamSynchronize(h->stream));
        const size_t dst_row = (size_t)h->dim * (h->dtype == LCD_F32 ? 4 : 1);
        for (int i = 0; i < n; ++i) std::memcpy((char*)out_rows + (size_t)i * dst_row, (const char*)h->h_out.p + (size_t)i * h->row_bytes, dst_row);
    }
    if (out_word_ids) { int rc = download(h, out_word_ids, h->row_id.as<int32_t>() + first, (size_t)n * 4, h->h_out2); if (rc) return rc; }
    return LCD_OK;
    LCD_CATCH(h)
}

// ------------------------------------------------------------------------------------------------ 2-NN
int lcd_knn2(lcd_engine* h, const void* queries, int q, int32_t* out_word_ids, float* out_dist) {
    LCD_TRY
    LCD_CHECK_HANDLE(h);
    LCD_DEV(h);
    if (q < 0 || (q > 0 && (!queries || !out_word_ids || !out_dist))) return h->fail(LCD_ERR_INVALID, "lcd_knn2: null input");
    if (q == 0) return LCD_OK;
    int rc = upload_rows(h, queries, q, h->d_queries);
    if (rc) return rc;
    rc = run_knn2(h, h->d_queries.p, q, h->vocab.p, h->row_id.as<int32_t>(), h->row_wslot.as<int32_t>(), h->n_rows, h->d_knn_row,
                  h->d_knn_word, h->d_knn_dist);
    if (rc) return rc;
    rc = download(h, out_word_ids, h->d_knn_word.p, (size_t)q * 8, h->h_out);
    if (rc) return rc;
    return download(h, out_dist, h->d_knn_dist.p, (size_t)q * 8, h->h_out);
    LCD_CATCH(h)
}

int lcd_selfdist(lcd_engine* h, const void* queries, int q, float* out_qxq) {
    LCD_TRY
    LCD_CHECK_HANDLE(h);
    LCD_DEV(h);
    if (q < 0 || (q > 0 && (!queries || !out_qxq))) return h->fail(LCD_ERR_INVALID, "lcd_selfdist: null input");
    if (q == 0) return LCD_OK;
    int rc = upload_rows(h, queries, q, h->d_queries);
    if (rc) return rc;
    LCD_HIP(h, dreserve(h, h->d_selfdist, (size_t)q * q * 4));
    LCD_HIP(h, launch_selfdist(h->dtype, h->kdim, h->d_queries.p, q, h->d_selfdist.as<float>(), q, h->stream));
    return download(h, out_qxq, h->d_selfdist.p, (size_t)q * q * 4, h->h_out);
    LCD_CATCH(h)
}

// device part of addNewWords: d_queries already holds q descriptors.  Leaves d_out_word[q], d_n_new[1].
static int quantize_dev(lcd_engine* h, const void* d_desc, int q, int flags, float nndr, int32_t* d_out_word, int32_t* d_out_wslot = nullptr) {
    ResolveArgs r;
    int rc = prepare_resolve(h, d_desc, q, flags, nndr, d_out_word, d_out_wslot, &r);
    if (rc) return rc;
    LCD_HIP(h, launch_resolve(r.q, r.flags, r.nndr, r.have_index, r.knn_word, r.knn_dist, r.selfdist, r.ld, r.cand_bits, r.bw, r.out_word,
                              r.out_n_new, h->stream, r.knn_row, r.row_wslot, r.out_wslot, nullptr, r.cand_list, r.cand_cnt));
    return LCD_OK;
}

int lcd_quantize(lcd_engine* h, const void* descriptors, int q, int flags, float nndr_ratio, int32_t* out_word_ids, int32_t* out_n_new) {
    LCD_TRY
    LCD_CHECK_HANDLE(h);
    lcd_engine::Range range__(h, "lcd_quantize");
    LCD_DEV(h);
    if (q < 0 || (q > 0 && (!descriptors || !out_word_ids))) return h->fail(LCD_ERR_INVALID, "lcd_quantize: null input");
    if (out_n_new) *out_n_new = 0;
    if (q == 0) return LCD_OK;
    if (q > 8192) return h->fail(LCD_ERR_UNSUPPORTED, "lcd_quantize: more than 8192 descriptors per call");
    int rc = upload_rows(h, descriptors, q, h->d_queries);
    if (rc) return rc;
    LCD_HIP(h, dreserve(h, h->d_out_word, (size_t)q * 4));
    rc = quantize_dev(h, h->d_queries.p, q, flags, nndr_ratio, h->d_out_word.as<int32_t>());
    if (rc) return rc;
    rc = download(h, out_word_ids, h->d_out_word.p, (size_t)q * 4, h->h_out);
    if (rc) return rc;
    if (out_n_new) return download(h, out_n_new, h->d_n_new.p, 4, h->h_out2);
    return LCD_OK;
    LCD_CATCH(h)
}

int lcd_find_nn(lcd_engine* h, const void* queries, int q, const void* extra_rows, const int32_t* extra_word_ids, int n_extra, int flags,
                float nndr_ratio, int32_t* out_word_ids) {
    LCD_TRY
    LCD_CHECK_HANDLE(h);
    LCD_DEV(h);
    if (q < 0 || n_extra < 0 || (q > 0 && (!queries || !out_word_ids)) || (n_extra > 0 && (!extra_rows || !extra_word_ids)))
        return h->fail(LCD_ERR_INVALID, "lcd_find_nn: null input");
    if (q == 0) return LCD_OK;
    int rc = upload_rows(h, queries, q, h->d_queries);
    if (rc) return rc;
    const int have_index = h->n_live >= 2 ? 1 : 0;                  // VWDictionary.cpp:1347
    rc = run_knn2(h, h->d_queries.p, q, h->vocab.p, h->row_id.as<int32_t>(), h->row_wslot.as<int32_t>(), have_index ? h->n_rows : 0,
                  h->d_knn_row, h->d_knn_word, h->d_knn_dist);
    if (rc) return rc;
    if (n_extra > 0) {   // the not-yet-indexed words: a second, temporary vocabulary (VWDictionary.cpp:1416-1451)
        // upload_rows stages through h_in: upload extra rows after the queries are on the device
        rc = upload_rows(h, extra_rows, n_extra, h->d_extra_rows);
        if (rc) return rc;
        LCD_HIP(h, dreserve(h, h->d_extra_id, (size_t)n_extra * 4));
        LCD_HIP(h, h->h_in.reserve((size_t)n_extra * 4));
        std::memcpy(h->h_in.p, extra_word_ids, (size_t)n_extra * 4);
        LCD_HIP(h, hipMemcpyAsync(h->d_extra_id.p, h->h_in.p, (size_t)n_extra * 4, hipMemcpyHostToDevice, h->stream));
        LCD_HIP(h, hipStreamSynchronize(h->stream));
        // the merge kernel of the indexed search has consumed d_partial (stream order), so it can be reused
        rc = run_knn2(h, h->d_queries.p, q, h->d_extra_rows.p, h->d_extra_id.as<int32_t>(), nullptr, n_extra, h->d_extra_row,
                      h->d_extra_word, h->d_extra_dist);
        if (rc) return rc;
    }
    LCD_HIP(h, dreserve(h, h->d_out_word, (size_t)q * 4));
    LCD_HIP(h, launch_findnn_resolve(q, flags, nndr_ratio, have_index, h->d_knn_word.as<int32_t>(), h->d_knn_dist.as<float>(),
                                     n_extra > 0 ? 1 : 0, h->d_extra_word.as<int32_t>(), h->d_extra_dist.as<float>(),
                                     h->d_out_word.as<int32_t>(), h->stream));
    return download(h, out_word_ids, h->d_out_word.p, (size_t)q * 4, h->h_out);
    LCD_CATCH(h)
}

// ------------------------------------------------------------------------------------------------ inverted index
// word ids of a host-side call -> device (t.d_stage); the id -> postings-key translation happens in the kernels through the
// device copy of the table.  create: unknown ids get a postings key now (addWordRef on a word the index has not seen yet).
static int stage_word_ids(lcd_engine* h, const int32_t* word_ids, int64_t n, bool create) {
    Tfidf& t = h->tfidf;
    for (int64_t i = 0; i < n; ++i) {
        const int32_t id = word_ids[i];
        if (id <= 0) continue;
        if (t.keys.known(id)) continue;                                          // the common case: one vector read
        int32_t ws;
        hipError_t e = t.keys.key_of(id, create, &ws);
        if (e == hipErrorInvalidValue) return h->fail(LCD_ERR_UNSUPPORTED, "word ids must be below 2^28");
        if (e != hipSuccess) return h->hip_fail(e, "key_of");
    }
    LCD_HIP(h, dreserve(h, t.d_stage, (size_t)std::max<int64_t>(n, 1) * 4));
    if (n) LCD_HIP(h, hipMemcpyAsync(t.d_stage.p, word_ids, (size_t)n * 4, hipMemcpyHostToDevice, h->stream));   // caller-owned source:
    return LCD_OK;                                                                                               // every caller synchronises
}

int lcd_sig_add(lcd_engine* h, int32_t sig_id, const int32_t* word_ids, int n, int32_t ni) {
    LCD_TRY
    LCD_CHECK_HANDLE(h);
    LCD_DEV(h);
    if (sig_id == 0 || n < 0 || (n > 0 && !word_ids) || ni < 0) return h->fail(LCD_ERR_INVALID, "lcd_sig_add: bad argument");
    if (n > TF_MAX_WORDS) return h->fail(LCD_ERR_UNSUPPORTED, "lcd_sig_add: more than 8192 words in one signature");
    if (h->tfidf.sig_slot.count(sig_id)) return h->fail(LCD_ERR_STATE, "lcd_sig_add: signature already registered");
    int rc = stage_word_ids(h, word_ids, n, true);
    if (rc) return rc;
    LCD_HIP(h, h->tfidf.register_dev(sig_id, h->tfidf.d_stage.as<int32_t>(), n, ni, 0.0f, nullptr, true));
    LCD_HIP(h, hipStreamSynchronize(h->stream));   // the caller's buffer was the copy source
    return LCD_OK;
    LCD_CATCH(h)
}

int lcd_sig_add_bulk(lcd_engine* h, int n_sigs, const int32_t* sig_ids, const int64_t* sig_offsets, const int32_t* word_ids, const int32_t* ni) {
    LCD_TRY
    LCD_CHECK_HANDLE(h);
    LCD_DEV(h);
    if (n_sigs < 0 || (n_sigs > 0 && (!sig_ids || !sig_offsets || !word_ids))) return h->fail(LCD_ERR_INVALID, "lcd_sig_add_bulk: null input");
    if (n_sigs == 0) return LCD_OK;
    Tfidf& t = h->tfidf;
    const int64_t total = sig_offsets[n_sigs] - sig_offsets[0];
    int max_n = 0;
    {
        std::vector<int32_t> sorted(sig_ids, sig_ids + n_sigs);
        std::sort(sorted.begin(), sorted.end());
        if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return h->fail(LCD_ERR_STATE, "lcd_sig_add_bulk: duplicate signature id");
    }
    for (int s = 0; s < n_sigs; ++s) {
        if (sig_ids[s] == 0 || t.sig_slot.count(sig_ids[s])) return h->fail(LCD_ERR_STATE, "lcd_sig_add_bulk: bad or duplicate signature id");
        const int64_t a = sig_offsets[s], b = sig_offsets[s + 1];
        if (b < a || b - a > TF_MAX_WORDS) return h->fail(LCD_ERR_UNSUPPORTED, "lcd_sig_add_bulk: bad offsets / more than 8192 words");
        if (ni && ni[s] < 0) return h->fail(LCD_ERR_INVALID, "lcd_sig_add_bulk: negative ni");
        max_n = std::max(max_n, (int)(b - a));
    }
    // all word ids in one copy, one registration launch for every signature, a fixed number of launches per batch of sealed buckets
    int rc = stage_word_ids(h, word_ids + sig_offsets[0], total, true);
    if (rc) return rc;
    LCD_HIP(h, t.register_bulk(n_sigs, sig_ids, sig_offsets, ni, t.d_stage.as<int32_t>(), total, max_n));   // synchronises
    return LCD_OK;
    LCD_CATCH(h)
}

int lcd_sig_remove(lcd_engine* h, int32_t sig_id) {
    LCD_TRY
    LCD_CHECK_HANDLE(h);
    LCD_DEV_NODRAIN(h);
    if (!h->pipe.empty()) {
        // a pipelined handle still owes stages of its latest frames: the retirement takes its place behind the newest of them
        const bool known = h->tfidf.sig_slot.count(sig_id) != 0 || h->pipe.registers(sig_id);
        if (!known || h->pipe.retirement_queued(sig_id)) return h->fail(LCD_ERR_STATE, "lcd_sig_remove: unknown signature");
        h->pipe.queue_retire(sig_id);
        return LCD_OK;
    }
    if (!h->tfidf.sig_slot.count(sig_id)) return h->fail(LCD_ERR_STATE, "lcd_sig_remove: unknown signature");
    LCD_HIP(h, h->tfidf.retire(sig_id));
    return LCD_OK;
    LCD_CATCH(h)
}

int lcd_sig_count(const lcd_engine* h, int64_t* live_signatures, int64_t* postings) {
    LCD_TRY
    LCD_CHECK_HANDLE(h);
    { int rc = const_cast<lcd_engine*>(h)->drain(); if (rc) return rc; }
    if (live_signatures) *live_signatures = h->tfidf.live_sigs;
    if (postings) *postings = h->tfidf.postings_ub;
    return LCD_OK;
    LCD_CATCH(h)
}

int lcd_word_nrefs(lcd_engine* h, int32_t word_id, int32_t* out_nw) {
    LCD_TRY
    LCD_CHECK_HANDLE(h);
    LCD_DEV(h);
    if (!out_nw) return h->fail(LCD_ERR_INVALID, "lcd_word_nrefs: null output");
    int32_t ws = -1;
    LCD_HIP(h, h->tfidf.keys.key_of(word_id, false, &ws));
    if (ws < 0) { *out_nw = 0; return LCD_OK; }
    LCD_HIP(h, h->tfidf.flush_retire());             // retirements ride with the next frame otherwise: nw would be stale
    return download(h, out_nw, h->tfidf.keys.nw.as<uint32_t>() + ws, 4, h->h_out2);
    LCD_CATCH(h)
}

int lcd_likelihood(lcd_engine* h, const int32_t* query_word_ids, int nq, const int32_t* sig_ids, int n_ids, float N, float* out) {
    LCD_TRY
    LCD_CHECK_HANDLE(h);
    lcd_engine::Range range__(h, "lcd_likelihood");
    LCD_DEV(h);
    if (nq < 0 || n_ids < 0 || (nq > 0 && !query_word_ids) || (n_ids > 0 && (!sig_ids || !out)))
        return h->fail(LCD_ERR_INVALID, "lcd_likelihood: null input");
    if (n_ids == 0) return LCD_OK;                                   // reference: empty ids -> empty map (Memory.cpp:2227)
    if (nq > TF_MAX_WORDS) return h->fail(LCD_ERR_UNSUPPORTED, "lcd_likelihood: more than 8192 query words");
    Tfidf& t = h->tfidf;
    if (t.n_slots == 0 || !(N > 0.0f)) { std::memset(out, 0, (size_t)n_ids * 4); return LCD_OK; }
    int rc = stage_word_ids(h, query_word_ids, nq, false);
    if (rc) return rc;
    LCD_HIP(h, t.query_dev(t.d_stage.as<int32_t>(), nq, N, nullptr, true));
    LCD_HIP(h, dreserve(h, h->d_like, (size_t)(t.n_slots + n_ids) * 4));
    LCD_HIP(h, t.score(h->d_like.as<float>()));
    h->likelihood_launches += 1;
    // gather the requested signatures
    LCD_HIP(h, h->h_in.reserve((size_t)n_ids * 8));
    int64_t* slots = h->h_in.as<int64_t>();
    for (int i = 0; i < n_ids; ++i) { auto it = t.sig_slot.find(sig_ids[i]); slots[i] = it == t.sig_slot.end() ? -1 : it->second; }
    LCD_HIP(h, dreserve(h, h->d_slots, (size_t)n_ids * 8));
    LCD_HIP(h, hipMemcpyAsync(h->d_slots.p, slots, (size_t)n_ids * 8, hipMemcpyHostToDevice, h->stream));
    float* d_out = h->d_like.as<float>() + t.n_slots;
    LCD_HIP(h, launch_gather_f32(h->d_like.as<float>(), h->d_slots.as<int64_t>(), n_ids, d_out, h->stream));
    return download(h, out, d_out, (size_t)n_ids * 4, h->h_out);
    LCD_CATCH(h)
}

// Signature::compareTo's words branch of the query against the listed signatures (similarity.hip): built as lcd_likelihood is
int lcd_similarity(lcd_engine* h, const int32_t* query_word_ids, int nq, const int32_t* sig_ids, int n_ids, float* out, int32_t* out_pairs,
                   int32_t* out_valid) {
    LCD_TRY
    LCD_CHECK_HANDLE(h);
    lcd_engine::Range range__(h, "lcd_similarity");
    LCD_DEV(h);
    if (nq < 0 || n_ids < 0 || (nq > 0 && !query_word_ids) || (n_ids > 0 && (!sig_ids || !out)))
        return h->fail(LCD_ERR_INVALID, "lcd_similarity: null input");
    if (n_ids == 0) return LCD_OK;
    if (nq > TF_MAX_WORDS) return h->fail(LCD_ERR_UNSUPPORTED, "lcd_similarity: more than 8192 query words");
    Tfidf& t = h->tfidf;
    if (t.n_slots == 0) {
        std::memset(out, 0, (size_t)n_ids * 4);
        if (out_pairs) std::memset(out_pairs, 0, (size_t)n_ids * 4);
        if (out_valid) std::memset(out_valid, 0, (size_t)n_ids * 4);
        return LCD_OK;
    }
    int rc = stage_word_ids(h, query_word_ids, nq, false);
    if (rc) return rc;
    const size_t ns = (size_t)t.n_slots, ni = (size_t)n_ids;
    LCD_HIP(h, dreserve(h, h->d_like, (ns + ni) * 4));
    LCD_HIP(h, dreserve(h, t.sim.d_int, 2 * (ns + ni) * 4));
    float* d_sim = h->d_like.as<float>();
    int32_t* d_pairs = t.sim.d_int.as<int32_t>();
    int32_t* d_valid = d_pairs + ns;
    LCD_HIP(h, t.sim.run(t, t.d_stage.as<int32_t>(), nq, d_sim, d_pairs, d_valid));
    // gather the requested signatures
    LCD_HIP(h, h->h_in.reserve(ni * 8));
    int64_t* slots = h->h_in.as<int64_t>();
    for (int i = 0; i < n_ids; ++i) { auto it = t.sig_slot.find(sig_ids[i]); slots[i] = it == t.sig_slot.end() ? -1 : it->second; }
    LCD_HIP(h, dreserve(h, h->d_slots, ni * 8));
    LCD_HIP(h, hipMemcpyAsync(h->d_slots.p, slots, ni * 8, hipMemcpyHostToDevice, h->stream));
    int32_t* g_pairs = d_valid + ns;
    int32_t* g_valid = g_pairs + ni;
    LCD_HIP(h, launch_gather_f32(d_sim, h->d_slots.as<int64_t>(), n_ids, d_sim + ns, h->stream));
    LCD_HIP(h, launch_gather_i32(d_pairs, h->d_slots.as<int64_t>(), n_ids, g_pairs, h->stream));
    LCD_HIP(h, launch_gather_i32(d_valid, h->d_slots.as<int64_t>(), n_ids, g_valid, h->stream));
    // one synchronisation for the three results (g_pairs and g_valid are adjacent)
    LCD_HIP(h, h->h_out.reserve(3 * ni * 4));
    char* pin = h->h_out.as<char>();
    LCD_HIP(h, hipMemcpyAsync(pin, d_sim + ns, ni * 4, hipMemcpyDeviceToHost, h->stream));
    LCD_HIP(h, hipMemcpyAsync(pin + ni * 4, g_pairs, 2 * ni * 4, hipMemcpyDeviceToHost, h->stream));
    LCD_HIP(h, hipStreamSynchronize(h->stream));
    std::memcpy(out, pin, ni * 4);
    if (out_pairs) std::memcpy(out_pairs, pin + ni * 4, ni * 4);
    if (out_valid) std::memcpy(out_valid, pin + 2 * ni * 4, ni * 4);
    return LCD_OK;
    LCD_CATCH(h)
}

int lcd_similarity_dev(lcd_engine* h, const int32_t* d_query_word_ids, int nq, float* d_out, int64_t capacity) {
    LCD_TRY
    LCD_CHECK_HANDLE(h);
    lcd_engine::Range range__(h, "lcd_similarity_dev");
    LCD_DEV(h);                                                      // completes what a pipelined handle owes
    Tfidf& t = h->tfidf;
    if (nq < 0 || (nq > 0 && !d_query_word_ids) || capacity < 0 || (t.n_slots > 0 && !d_out))
        return h->fail(LCD_ERR_INVALID, "lcd_similarity_dev: bad argument");
    if (nq > TF_MAX_WORDS) return h->fail(LCD_ERR_UNSUPPORTED, "lcd_similarity_dev: more than 8192 query words");
    if (capacity < t.n_slots) return h->fail(LCD_ERR_INVALID, "lcd_similarity_dev: output buffer smaller than the slots in use");
    LCD_HIP(h, t.sim.run(t, d_query_word_ids, nq, d_out, nullptr, nullptr));
    return LCD_OK;
    LCD_CATCH(h)
}

// ---- global descriptors (global_similarity.hip): Signature::compareTo's other branch
// the rules every entry applies to an array of descriptors before anything is stored or launched; a query (sig == false) may name a channel
// the handle has never stored a row on (it matches nothing)
static int check_globals(lcd_engine* h, const char* who, const lcd_global_desc* d, int n) {
    if (n < 0 || (n > 0 && !d)) return h->fail(LCD_ERR_INVALID, std::string(who) + ": null input");
    if (n > GLOBAL_MAX_CHANNELS) return h->fail(LCD_ERR_UNSUPPORTED, std::string(who) + ": more than 4 global descriptors");
    for (int i = 0; i < n; ++i) {
        if (d[i].type != 1) continue;
        if (d[i].dim > GLOBAL_MAX_DIM) return h->fail(LCD_ERR_UNSUPPORTED, std::string(who) + ": a global descriptor of more than 16384 floats");
        if (d[i].dim <= 0 || !d[i].data) return h->fail(LCD_ERR_INVALID, std::string(who) + ": a type-1 global descriptor without data");
        const int have = h->tfidf.glob.ch[i].dim;
        if (have && have != d[i].dim) return h->fail(LCD_ERR_INVALID, std::string(who) + ": the channel holds rows of another length");
    }
    return LCD_OK;
}

static int set_globals(lcd_engine* h, const char* who, int32_t sig_id, const lcd_global_desc* descs, int n, bool on_device) {
    int rc = check_globals(h, who, descs, n);
    if (rc) return rc;
    Tfidf& t = h->tfidf;
    auto it = t.sig_slot.find(sig_id);
    if (it == t.sig_slot.end()) return h->fail(LCD_ERR_STATE, std::string(who) + ": unknown signature");
    const int64_t slot = it->second;
    const int64_t hint = (int64_t)(t.slot_sig.cap / 4);
    size_t off[GLOBAL_MAX_CHANNELS], total = 0;
    for (int c = 0; c < n; ++c) {
        if (descs[c].type != 1) continue;
        LCD_HIP(h, t.glob.ensure(t, c, descs[c].dim, slot + 1, hint));
        off[c] = total; total += (size_t)descs[c].dim * 4;
    }
    if (!on_device && total) {                                        // the rows in one pinned block, one copy
        LCD_HIP(h, h->h_in.reserve(total));
        for (int c = 0; c < n; ++c) if (descs[c].type == 1) std::memcpy(h->h_in.as<char>() + off[c], descs[c].data, (size_t)descs[c].dim * 4);
        LCD_HIP(h, dreserve(h, t.glob.stage, total));
        LCD_HIP(h, hipMemcpyAsync(t.glob.stage.p, h->h_in.p, total, hipMemcpyHostToDevice, h->stream));
    }
    for (int c = 0; c < GLOBAL_MAX_CHANNELS; ++c) {
        if (c < n && descs[c].type == 1)
            LCD_HIP(h, t.glob.store(t, c, on_device ? descs[c].data : (const float*)(t.glob.stage.as<char>() + off[c]), 1, nullptr, slot));
        else
            LCD_HIP(h, t.glob.clear(t, c, slot));
    }
    if (!on_device) LCD_HIP(h, hipStreamSynchronize(h->stream));      // h_in is reused by the next call
    return LCD_OK;
}

int lcd_sig_set_globals(lcd_engine* h, int32_t sig_id, const lcd_global_desc* descs, int n) {
    LCD_TRY
    LCD_CHECK_HANDLE(h);
    LCD_DEV(h);
    return set_globals(h, "lcd_sig_set_globals", sig_id, descs, n, false);
    LCD_CATCH(h)
}

int lcd_sig_set_globals_dev(lcd_engine* h, int32_t sig_id, const lcd_global_desc* descs, int n) {
    LCD_TRY
    LCD_CHECK_HANDLE(h);
    LCD_DEV(h);
    return set_globals(h, "lcd_sig_set_globals_dev", sig_id, descs, n, true);
    LCD_CATCH(h)
}

int lcd_sig_set_global_bulk(lcd_engine* h, int channel, int n_sigs, const int32_t* sig_ids, const float* rows, int dim) {
    LCD_TRY
    LCD_CHECK_HANDLE(h);
    LCD_DEV(h);
    if (channel < 0 || n_sigs < 0 || (n_sigs > 0 && (!sig_ids || !rows))) return h->fail(LCD_ERR_INVALID, "lcd_sig_set_global_bulk: bad argument");
    if (channel >= GLOBAL_MAX_CHANNELS) return h->fail(LCD_ERR_UNSUPPORTED, "lcd_sig_set_global_bulk: more than 4 global descriptors");
    if (dim > GLOBAL_MAX_DIM) return h->fail(LCD_ERR_UNSUPPORTED, "lcd_sig_set_global_bulk: a global descriptor of more than 16384 floats");
    if (dim <= 0) return h->fail(LCD_ERR_INVALID, "lcd_sig_set_global_bulk: dim <= 0");
    Tfidf& t = h->tfidf;
    if (t.glob.ch[channel].dim && t.glob.ch[channel].dim != dim) return h->fail(LCD_ERR_INVALID, "lcd_sig_set_global_bulk: the channel holds rows of another length");
    if (n_sigs == 0) return LCD_OK;
    {
        std::vector<int32_t> sorted(sig_ids, sig_ids + n_sigs);
        std::sort(sorted.begin(), sorted.end());
        if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return h->fail(LCD_ERR_INVALID, "lcd_sig_set_global_bulk: repeated signature id");
    }
    std::vector<int64_t> slots((size_t)n_sigs);
    int64_t top = 0;
    for (int i = 0; i < n_sigs; ++i) {
        auto it = t.sig_slot.find(sig_ids[i]);
        if (it == t.sig_slot.end()) return h->fail(LCD_ERR_STATE, "lcd_sig_set_global_bulk: unknown signature");
        slots[(size_t)i] = it->second;
        top = std::max(top, it->second + 1);
    }
    LCD_HIP(h, t.glob.ensure(t, channel, dim, top, (int64_t)(t.slot_sig.cap / 4)));
    const size_t bytes = (size_t)n_sigs * (size_t)dim * 4;
    LCD_HIP(h, h->h_in.reserve((size_t)n_sigs * 8));
    std::memcpy(h->h_in.p, slots.data(), (size_t)n_sigs * 8);
    LCD_HIP(h, dreserve(h, h->d_slots, (size_t)n_sigs * 8));
    LCD_HIP(h, hipMemcpyAsync(h->d_slots.p, h->h_in.p, (size_t)n_sigs * 8, hipMemcpyHostToDevice, h->stream));
    LCD_HIP(h, dreserve(h, t.glob.stage, bytes));
    LCD_HIP(h, hipMemcpyAsync(t.glob.stage.p, rows, bytes, hipMemcpyHostToDevice, h->stream));   // caller-owned source: synchronised below
    LCD_HIP(h, t.glob.store(t, channel, t.glob.stage.as<float>(), n_sigs, h->d_slots.as<int64_t>(), 0));
    LCD_HIP(h, hipStreamSynchronize(h->stream));
    return LCD_OK;
    LCD_CATCH(h)
}

int lcd_sig_clear_globals(lcd_engine* h, int32_t sig_id) {
    LCD_TRY
    LCD_CHECK_HANDLE(h);
    LCD_DEV(h);
    Tfidf& t = h->tfidf;
    auto it = t.sig_slot.find(sig_id);
    if (it == t.sig_slot.end()) return h->fail(LCD_ERR_STATE, "lcd_sig_clear_globals: unknown signature");
    for (int c = 0; c < GLOBAL_MAX_CHANNELS; ++c) LCD_HIP(h, t.glob.clear(t, c, it->second));
    return LCD_OK;
    LCD_CATCH(h)
}

static GlobalQuery global_query(const lcd_global_desc* d, int n, bool on_device) {
    GlobalQuery q;
    q.n = n; q.on_device = on_device;
    for (int c = 0; c < n; ++c) { q.type[c] = d[c].type; q.dim[c] = d[c].dim; q.data[c] = d[c].data; }
    return q;
}

// Signature::compareTo: the words branch over every slot (similarity.hip), then the global descriptors replace it where a channel matches
int lcd_compare_to(lcd_engine* h, const int32_t* query_word_ids, int nq, const lcd_global_desc* query_globals, int n_globals,
                   const int32_t* sig_ids, int n_ids, float* out, int32_t* out_n_global) {
    LCD_TRY
    LCD_CHECK_HANDLE(h);
    lcd_engine::Range range__(h, "lcd_compare_to");
    LCD_DEV(h);
    if (nq < 0 || n_ids < 0 || (nq > 0 && !query_word_ids) || (n_ids > 0 && (!sig_ids || !out)))
        return h->fail(LCD_ERR_INVALID, "lcd_compare_to: null input");
    int rc = check_globals(h, "lcd_compare_to", query_globals, n_globals);
    if (rc) return rc;
    if (nq > TF_MAX_WORDS) return h->fail(LCD_ERR_UNSUPPORTED, "lcd_compare_to: more than 8192 query words");
    if (n_ids == 0) return LCD_OK;
    Tfidf& t = h->tfidf;
    const size_t ns = (size_t)t.n_slots, ni = (size_t)n_ids;
    if (ns == 0) {
        std::memset(out, 0, ni * 4);
        if (out_n_global) std::memset(out_n_global, 0, ni * 4);
        return LCD_OK;
    }
    rc = stage_word_ids(h, query_word_ids, nq, false);
    if (rc) return rc;
    LCD_HIP(h, dreserve(h, h->d_like, (ns + ni) * 4));
    LCD_HIP(h, dreserve(h, t.sim.d_int, ni * 4));
    float* d_sim = h->d_like.as<float>();
    LCD_HIP(h, t.sim.run(t, t.d_stage.as<int32_t>(), nq, d_sim, nullptr, nullptr));
    LCD_HIP(h, t.glob.run(t, global_query(query_globals, n_globals, false), d_sim));
    LCD_HIP(h, h->h_in.reserve(ni * 8));
    int64_t* slots = h->h_in.as<int64_t>();
    for (int i = 0; i < n_ids; ++i) { auto it = t.sig_slot.find(sig_ids[i]); slots[i] = it == t.sig_slot.end() ? -1 : it->second; }
    LCD_HIP(h, dreserve(h, h->d_slots, ni * 8));
    LCD_HIP(h, hipMemcpyAsync(h->d_slots.p, slots, ni * 8, hipMemcpyHostToDevice, h->stream));
    LCD_HIP(h, launch_gather_f32(d_sim, h->d_slots.as<int64_t>(), n_ids, d_sim + ns, h->stream));
    const bool counted = t.glob.any();                               // (a handle that never stored a row: totalDescs is 0 everywhere)
    if (counted) LCD_HIP(h, launch_gather_i32(t.glob.acc_cnt.as<int32_t>(), h->d_slots.as<int64_t>(), n_ids, t.sim.d_int.as<int32_t>(), h->stream));
    LCD_HIP(h, h->h_out.reserve(2 * ni * 4));
    char* pin = h->h_out.as<char>();
    LCD_HIP(h, hipMemcpyAsync(pin, d_sim + ns, ni * 4, hipMemcpyDeviceToHost, h->stream));
    if (counted) LCD_HIP(h, hipMemcpyAsync(pin + ni * 4, t.sim.d_int.p, ni * 4, hipMemcpyDeviceToHost, h->stream));
    else std::memset(pin + ni * 4, 0, ni * 4);
    LCD_HIP(h, hipStreamSynchronize(h->stream));
    std::memcpy(out, pin, ni * 4);
    if (out_n_global) std::memcpy(out_n_global, pin + ni * 4, ni * 4);
    return LCD_OK;
    LCD_CATCH(h)
}

int lcd_compare_to_dev(lcd_engine* h, const int32_t* d_query_word_ids, int nq, const lcd_global_desc* query_globals, int n_globals,
                       float* d_out, int64_t capacity) {
    LCD_TRY
    LCD_CHECK_HANDLE(h);
    lcd_engine::Range range__(h, "lcd_compare_to_dev");
    LCD_DEV(h);                                                      // completes what a pipelined handle owes
    Tfidf& t = h->tfidf;
    if (nq < 0 || (nq > 0 && !d_query_word_ids) || capacity < 0 || (t.n_slots > 0 && !d_out))
        return h->fail(LCD_ERR_INVALID, "lcd_compare_to_dev: bad argument");
    int rc = check_globals(h, "lcd_compare_to_dev", query_globals, n_globals);
    if (rc) return rc;
    if (nq > TF_MAX_WORDS) return h->fail(LCD_ERR_UNSUPPORTED, "lcd_compare_to_dev: more than 8192 query words");
    if (capacity < t.n_slots) return h->fail(LCD_ERR_INVALID, "lcd_compare_to_dev: output buffer smaller than the slots in use");
    LCD_HIP(h, t.sim.run(t, d_query_word_ids, nq, d_out, nullptr, nullptr));
    LCD_HIP(h, t.glob.run(t, global_query(query_globals, n_globals, true), d_out));
    return LCD_OK;
    LCD_CATCH(h)
}

// Rtabmap::adjustLikelihood on a device vector whose entry 0 is the virtual place, in place: the decision stage's two passes
// (bayes.hip) with every entry taking part
static int adjust_vector(lcd_engine* h, float* d_L, int n, float ratio) {
    DecideArgs d;
    d.like = d_L + 1; d.ratio = ratio; d.adj_out = d_L;
    LCD_HIP(h, h->bayes.decide(d, nullptr, (int64_t)n - 1, (int64_t)n - 1));
    return LCD_OK;
}

int lcd_adjust_likelihood(lcd_engine* h, float* likelihood, int n, float virtual_place_ratio) {
    LCD_TRY
    LCD_CHECK_HANDLE(h);
    LCD_DEV(h);
    if (n < 0 || (n > 0 && !likelihood)) return h->fail(LCD_ERR_INVALID, "lcd_adjust_likelihood: null input");
    if (n == 0) return LCD_OK;
    LCD_HIP(h, dreserve(h, h->d_like, (size_t)n * 4));
    LCD_HIP(h, h->h_in.reserve((size_t)n * 4));
    std::memcpy(h->h_in.p, likelihood, (size_t)n * 4);
    LCD_HIP(h, hipMemcpyAsync(h->d_like.p, h->h_in.p, (size_t)n * 4, hipMemcpyHostToDevice, h->stream));
    { int rc = adjust_vector(h, h->d_like.as<float>(), n, virtual_place_ratio); if (rc) return rc; }
    return download(h, likelihood, h->d_like.p, (size_t)n * 4, h->h_out);
    LCD_CATCH(h)
}

int lcd_adjust_likelihood_dev(lcd_engine* h, float* d_likelihood, int n, float virtual_place_ratio) {
    LCD_TRY
    LCD_CHECK_HANDLE(h);
    LCD_DEV(h);
    if (n < 0 || (n > 0 && !d_likelihood)) return h->fail(LCD_ERR_INVALID, "lcd_adjust_likelihood_dev: null input");
    if (n == 0) return LCD_OK;
    return adjust_vector(h, d_likelihood, n, virtual_place_ratio);
    LCD_CATCH(h)
}

int lcd_knn2_dev(lcd_engine* h, const void* d_queries, int q, int32_t* d_word_ids, float* d_dist) {
    LCD_TRY
    LCD_CHECK_HANDLE(h);
    LCD_DEV_NODRAIN(h);
    if (rows_padded(h)) return h->fail(LCD_ERR_UNSUPPORTED, "lcd_knn2_dev: rows of this size are padded on the device (use lcd_knn2)");
    { int rc = h->drain(); if (rc) return rc; }
    if (q <= 0 || !d_queries || !d_word_ids || !d_dist) return h->fail(LCD_ERR_INVALID, "lcd_knn2_dev: bad argument");
    if (((uintptr_t)d_queries & 15u) != 0) return h->fail(LCD_ERR_INVALID, "lcd_knn2_dev: d_queries must be 16-byte aligned");
    LCD_HIP(h, dreserve(h, h->d_knn_row, (size_t)q * 2 * 4));
    return run_knn2_raw(h, d_queries, q, h->vocab.p, h->row_id.as<int32_t>(), h->n_rows, true, h->d_knn_row.as<int32_t>(), d_word_ids, d_dist);
    LCD_CATCH(h)
}

// ---------------------------------------------------------------------------------------------------------------- Bayes filter
int lcd_bayes_configure(lcd_engine* h, const double* prediction_lc, int n_values, float virtual_place_prior) {
    LCD_TRY
    LCD_CHECK_HANDLE(h);
    LCD_DEV(h);
    if (!prediction_lc) return h->fail(LCD_ERR_INVALID, "lcd_bayes_configure: bad argument");
    if (h->bayes.configure(prediction_lc, n_values, virtual_place_prior) != hipSuccess)
        return h->fail(LCD_ERR_INVALID, "lcd_bayes_configure: 2..32 values in [0, 1] and a prior in [0, 1] expected");   // the reference logs UERROR (:83, :103)
    return LCD_OK;
    LCD_CATCH(h)
}

int lcd_bayes_reset(lcd_engine* h) {
    LCD_TRY
    LCD_CHECK_HANDLE(h);
    LCD_DEV(h);
    LCD_HIP(h, h->bayes.reset());
    return LCD_OK;
    LCD_CATCH(h)
}

int lcd_bayes_set_neighbors(lcd_engine* h, int n_sigs, const int32_t* sig_ids, const int64_t* offsets, const int32_t* nbr_sig_ids,
                            const int32_t* nbr_margins) {
    LCD_TRY
    LCD_CHECK_HANDLE(h);
#ifdef LCD_DEBUG_TIMING
    static double dbg[4]; static int dbg_n;
    const auto d0 = std::chrono::steady_clock::now();
#endif
    LCD_DEV_NODRAIN(h);                                       // a pipelined handle queues the lists behind the index stage it still owes
#ifdef LCD_DEBUG_TIMING
    const auto d1 = std::chrono::steady_clock::now();
    struct Rep { std::chrono::steady_clock::time_point a, b; double* d; int* n; ~Rep() { auto c = std::chrono::steady_clock::now();
        d[0] += std::chrono::duration<double, std::micro>(b - a).count(); d[1] += std::chrono::duration<double, std::micro>(c - b).count();
        if (++*n % 100 == 0) { fprintf(stderr, "[set_neighbors] setdevice %.2f us, rest %.2f us (avg of 100)\n", d[0] / 100, d[1] / 100); d[0] = d[1] = 0; } } } rep__{d0, d1, dbg, &dbg_n};
#endif
    if (n_sigs < 0 || (n_sigs > 0 && (!sig_ids || !offsets))) return h->fail(LCD_ERR_INVALID, "lcd_bayes_set_neighbors: bad argument");
    if (!h->bayes.configured) return h->fail(LCD_ERR_STATE, "lcd_bayes_set_neighbors: lcd_bayes_configure first");
    if (n_sigs == 0) return LCD_OK;
    if (offsets[n_sigs] > offsets[0] && (!nbr_sig_ids || !nbr_margins)) return h->fail(LCD_ERR_INVALID, "lcd_bayes_set_neighbors: bad argument");
    Tfidf& t = h->tfidf;
    if (t.n_slots >= (1ll << BAYES_SLOT_BITS)) return h->fail(LCD_ERR_UNSUPPORTED, "lcd_bayes_set_neighbors: at most 2^27 signature slots");
    const int max_margin = h->bayes.prm.n_lc - 2;
    std::vector<int32_t> triples, restart;                    // restart: the slots of the listed signatures (their lists start over)
    std::unordered_map<uint64_t, int32_t> seen;
    seen.reserve((size_t)(offsets[n_sigs] - offsets[0]) * 2 + 16);
    // (the signatures of frames whose registration is still owed have no slots yet: FramePipeline::slot_of knows the ones they will get)
    for (int i = 0; i < n_sigs; ++i) {
        const int64_t a = h->pipe.slot_of(sig_ids[i], t);
        if (offsets[i + 1] < offsets[i]) return h->fail(LCD_ERR_INVALID, "lcd_bayes_set_neighbors: offsets must not decrease");
        // a signature the engine does not hold -- one without a single word never got references, hence no slot (a featureless
        // frame, Rtabmap.cpp:2234 "bad signature") -- has no likelihood and no posterior: its list is skipped, the reference's filter
        // carries such signatures along with probability 0 as well
        if (a < 0) continue;
        restart.push_back((int32_t)a);
        for (int64_t e = offsets[i]; e < offsets[i + 1]; ++e) {
            const int32_t m = nbr_margins[e];
            if (m < 0 || m > max_margin) return h->fail(LCD_ERR_INVALID, "lcd_bayes_set_neighbors: margin outside the prediction's levels");   // UASSERT :263
            if (nbr_sig_ids[e] < 0) continue;                 // "if(iter->first>=0)" (:254)
            const int64_t b = h->pipe.slot_of(nbr_sig_ids[e], t);
            if (b < 0) continue;                              // not in memory: it can not be in a likelihood
            const uint64_t key = ((uint64_t)std::min(a, b) << 32) | (uint64_t)std::max(a, b);
            auto st = seen.find(key);
            if (st != seen.end()) { triples[(size_t)st->second * 3 + 2] = m; continue; }   // listed from both ends: the later margin stays
            seen.emplace(key, (int32_t)(triples.size() / 3));
            triples.push_back((int32_t)std::min(a, b)); triples.push_back((int32_t)std::max(a, b)); triples.push_back(m);
        }
    }
    if (!h->pipe.empty()) { h->pipe.queue_link(FramePipeline::DeferredLink{std::move(triples), std::move(restart)}); return LCD_OK; }
    LCD_HIP(h, h->bayes.ensure(std::max<int64_t>(t.n_slots, 1)));
    const hipError_t le = h->bayes.link(triples, restart);
    if (le == hipErrorInvalidValue) return h->fail(LCD_ERR_UNSUPPORTED, "lcd_bayes_set_neighbors: a neighbour list longer than 8192 entries");
    LCD_HIP(h, le);
    return LCD_OK;
    LCD_CATCH(h)
}

int lcd_bayes_update_dev(lcd_engine* h, const float* d_adjusted, int exclude_recent, float* d_posterior, lcd_bayes_result* d_result) {
    LCD_TRY
    LCD_CHECK_HANDLE(h);
    LCD_DEV(h);
    if (!d_adjusted) return h->fail(LCD_ERR_INVALID, "lcd_bayes_update_dev: bad argument");
    if (!h->bayes.configured) return h->fail(LCD_ERR_STATE, "lcd_bayes_update_dev: lcd_bayes_configure first");
    Tfidf& t = h->tfidf;
    LCD_HIP(h, t.flush_retire());                             // slot_sig must show the retirements asked for so far
    const long long n_cons = (long long)t.n_slots - std::max(exclude_recent, 0);
    DecideArgs d;
    d.adj_in = d_adjusted; d.bayes = true; d.d_posterior = d_posterior; d.d_bayes = (BayesOut*)d_result;
    LCD_HIP(h, h->bayes.decide(d, t.slot_sig.as<int32_t>(), t.n_slots, n_cons));
    return LCD_OK;
    LCD_CATCH(h)
}

int lcd_bayes_update(lcd_engine* h, const int32_t* sig_ids, const float* adjusted, int n, lcd_bayes_result* result) {
    LCD_TRY
    LCD_CHECK_HANDLE(h);
    LCD_DEV(h);
    if (n < 1 || !sig_ids || !adjusted) return h->fail(LCD_ERR_INVALID, "lcd_bayes_update: bad argument");
    if (!h->bayes.configured) return h->fail(LCD_ERR_STATE, "lcd_bayes_update: lcd_bayes_configure first");
    if (sig_ids[0] != -1) return h->fail(LCD_ERR_UNSUPPORTED, "lcd_bayes_update: the likelihood must start with the virtual place (id -1)");
    Tfidf& t = h->tfidf;
    LCD_HIP(h, t.flush_retire());
    // scatter the map into slot order; its keys must be the registered signatures without the most recently registered ones
    const size_t bytes = ((size_t)t.n_slots + 1) * 4;
    LCD_HIP(h, h->h_in.reserve(bytes));
    float* adj = (float*)h->h_in.p;
    std::memset(adj, 0, bytes);
    adj[0] = adjusted[0];
    int64_t n_cons = 0, n_reg = 0;
    for (int i = 1; i < n; ++i) {
        if (sig_ids[i] <= sig_ids[i - 1]) return h->fail(LCD_ERR_INVALID, "lcd_bayes_update: ids must ascend (std::map order)");
        auto it = t.sig_slot.find(sig_ids[i]);
        if (it == t.sig_slot.end()) continue;                    // a signature without words holds no slot: no likelihood, posterior 0 (see set_neighbors)
        adj[(size_t)it->second + 1] = adjusted[i];
        n_cons = std::max<int64_t>(n_cons, it->second + 1);
        n_reg += 1;
    }
    int64_t live_below = 0;
    if (n_cons == t.n_slots) live_below = t.live_sigs;             // the usual case without a short-term memory: no walk over the table
    else for (const auto& kv : t.sig_slot) live_below += kv.second < n_cons ? 1 : 0;
    if (live_below != n_reg)
        return h->fail(LCD_ERR_UNSUPPORTED, "lcd_bayes_update: the likelihood must hold every registered signature up to its newest one "
                                            "(the working memory without the short-term memory)");
    LCD_HIP(h, dreserve(h, h->d_adj_scratch, bytes));
    LCD_HIP(h, hipMemcpyAsync(h->d_adj_scratch.p, adj, bytes, hipMemcpyHostToDevice, h->stream));
    DecideArgs d;
    d.adj_in = h->d_adj_scratch.as<float>(); d.bayes = true; d.d_bayes = (BayesOut*)h->d_hyp_scratch.p;
    LCD_HIP(h, h->bayes.decide(d, t.slot_sig.as<int32_t>(), t.n_slots, n_cons));
    lcd_bayes_result r;
    { int rc = download(h, &r, h->d_hyp_scratch.p, sizeof(r), h->h_out); if (rc) return rc; }   // (synchronises: h_in is free again)
    if (result) *result = r;
    return LCD_OK;
    LCD_CATCH(h)
}

int lcd_bayes_posterior(lcd_engine* h, const int32_t* sig_ids, int n, float* out) {
    LCD_TRY
    LCD_CHECK_HANDLE(h);
    LCD_DEV(h);
    if (n < 0 || (n > 0 && (!sig_ids || !out))) return h->fail(LCD_ERR_INVALID, "lcd_bayes_posterior: bad argument");
    if (n == 0) return LCD_OK;
    Tfidf& t = h->tfidf;
    std::vector<float> all;
    std::vector<uint8_t> in;
    const int64_t have = std::min<int64_t>(t.n_slots, h->bayes.cap);
    LCD_HIP(h, h->bayes.read_posterior(have, &all, &in));
    for (int i = 0; i < n; ++i) {
        float v = 0.0f;
        if (sig_ids[i] == -1) v = in[0] ? all[0] : 0.0f;
        else {
            auto it = t.sig_slot.find(sig_ids[i]);
            if (it != t.sig_slot.end() && it->second < have && in[(size_t)it->second + 1]) v = all[(size_t)it->second + 1];
        }
        out[i] = v;
    }
    return LCD_OK;
    LCD_CATCH(h)
}

int lcd_shard_knn2_dev(lcd_engine* h, const void* d_descriptors, int q, lcd_shard_cand* d_cand) {
    LCD_TRY
    LCD_CHECK_HANDLE(h);
    LCD_DEV_NODRAIN(h);
    if (rows_padded(h)) return h->fail(LCD_ERR_UNSUPPORTED, "lcd_shard_knn2_dev: rows of this size are padded on the device (use lcd_knn2)");
    { int rc = drain_keep_rows_lazy(h); if (rc) return rc; }
    if (q <= 0 || !d_descriptors || !d_cand) return h->fail(LCD_ERR_INVALID, "lcd_shard_knn2_dev: bad argument");
    if (((uintptr_t)d_descriptors & 15u) != 0) return h->fail(LCD_ERR_INVALID, "lcd_shard_knn2_dev: d_descriptors must be 16-byte aligned");
    const int64_t rows_scan = h->applog.rows_ub(h->n_rows);                           // == n_rows unless this rank appended on the device since the mirror last caught up
    if (rows_scan >= (1 << 26)) return h->fail(LCD_ERR_UNSUPPORTED, "lcd_shard_knn2_dev: a shard holds at most 2^26 - 1 rows (merge key: 26-bit row, 6-bit rank)");
    LCD_HIP(h, dreserve(h, h->d_knn_row, (size_t)q * 2 * 4));
    LCD_HIP(h, dreserve(h, h->d_knn_word, (size_t)q * 2 * 4));
    LCD_HIP(h, dreserve(h, h->d_knn_dist, (size_t)q * 2 * 4));
    // the candidate records are the work of the search's last launch: the exact redo's when the search has one (the matrix-core filter; one launch
    // less per frame and rank), a launch of their own behind the exact scan otherwise.  Either way the search's counters are left zeroed.
    ShardPackArgs pk;
    pk.knn_row = h->d_knn_row.as<int32_t>(); pk.knn_word = h->d_knn_word.as<int32_t>(); pk.knn_dist = h->d_knn_dist.as<float>();
    pk.row_wslot = h->row_wslot.as<int32_t>(); pk.q2 = 2 * q; pk.out = reinterpret_cast<ShardCand*>(d_cand);
    bool packed = false;
    // the same-frame distance matrix needs nothing but the descriptors: it rides in the filter's launch (extra workgroups, as in the single-GPU
    // frame) instead of waiting behind the all-gather.  No bit rows yet (bits == nullptr): their thresholds are the MERGED second neighbours'.
    CandBits sd;
    h->shard_sd_desc = nullptr;
    bool with_sd = h->knn_mode != 0 && h->bf_family() && knn_mfma_supported(h->dtype, h->kdim) && rows_scan >= 256;
    if (with_sd) {
        // ... unless the compute units its tiles take turn a one-strip-per-workgroup filter into the persistent one (between ~56 000 and ~65 000
        // rows at 500 descriptors: the filter then costs 4 us more, what the ride saves behind the all-gather; r06_call55)
        MfmaPlan p0 = knn_bf16_plan(q, (int)rows_scan, 0), p1 = knn_bf16_plan(q, (int)rows_scan, knn_selfdist_wgs(q));
        p0.filter_units = p1.filter_units = h->filter_units;
        with_sd = knn_bf16_persistent(p0) == knn_bf16_persistent(p1);
    }
    if (with_sd) {
        const int ld = (q + 63) / 64 * 64;
        LCD_HIP(h, dreserve(h, h->d_shard_selfdist, (size_t)q * ld * 4));
        sd.selfdist = h->d_shard_selfdist.as<float>(); sd.ld = ld; sd.nq = q;
    }
    int rc = run_knn2_raw(h, d_descriptors, q, h->vocab.p, h->row_id.as<int32_t>(), rows_scan, true, h->d_knn_row.as<int32_t>(),
                          h->d_knn_word.as<int32_t>(), h->d_knn_dist.as<float>(), with_sd ? &sd : nullptr, nullptr, &pk, &packed);
    if (rc) return rc;
    if (with_sd) { h->shard_sd_desc = d_descriptors; h->shard_sd_q = q; }
    if (!packed) LCD_HIP(h, launch_shard_pack(pk.knn_row, pk.knn_word, pk.knn_dist, pk.row_wslot, q, d_cand, h->stream, h->d_fail_count.as<int32_t>()));
    h->fail_count_clean = true;
    return LCD_OK;
    LCD_CATCH(h)
}

int lcd_shard_frame_dev(lcd_engine* h, const void* d_descriptors, int q, int flags, float nndr_ratio, int32_t sig_id,
                        int32_t first_new_word_id, float N, int rank, int world, const lcd_shard_cand* d_all_cand, int64_t total_live_rows,
                        int32_t* d_word_ids, int64_t* d_lfix, int64_t lfix_capacity) {
    LCD_TRY
    LCD_CHECK_HANDLE(h);
    LCD_DEV_NODRAIN(h);
    if (rows_padded(h)) return h->fail(LCD_ERR_UNSUPPORTED, "lcd_shard_frame_dev: rows of this size are padded on the device (use lcd_quantize)");
    { int rc = drain_keep_rows_lazy(h); if (rc) return rc; }
    const bool matrix_left = h->shard_sd_desc != nullptr && h->shard_sd_desc == d_descriptors && h->shard_sd_q == q;   // by this frame's search
    h->shard_sd_desc = nullptr;                                       // (one frame call per search: whatever happens below, it is used up)
    if (q <= 0 || q > 8192 || !d_descriptors || !d_all_cand || !d_word_ids || world < 1 || world > 64 || rank < 0 || rank >= world)
        return h->fail(LCD_ERR_INVALID, "lcd_shard_frame_dev: bad argument");
    Tfidf& t = h->tfidf;
    if (sig_id != 0 && t.sig_slot.count(sig_id)) return h->fail(LCD_ERR_STATE, "lcd_shard_frame_dev: signature already registered");
    const int64_t slots_after = t.n_slots + (sig_id != 0 ? 1 : 0);
    if (d_lfix && lfix_capacity < slots_after) return h->fail(LCD_ERR_INVALID, "lcd_shard_frame_dev: lfix buffer too small");
    LCD_HIP(h, dreserve(h, h->d_knn_row, (size_t)q * 2 * 4));
    LCD_HIP(h, dreserve(h, h->d_knn_word, (size_t)q * 2 * 4));
    LCD_HIP(h, dreserve(h, h->d_knn_dist, (size_t)q * 2 * 4));
    // global 2-NN from the gathered per-rank candidates; d_knn_row holds the postings keys of the neighbours this rank owns
    // ONE flag decides both the owner of a new word and the order of equal distances in the merge (block-cyclic owners need ties by word
    // id; ties by (rank, row) need every new word on the last rank): a block without a first id is no growth policy, and a frame whose
    // new ids would lie in front of the policy's origin has no owner rule at all -- refused rather than guessed
    const bool cyclic = h->shard_block > 0 && h->shard_first > 0;
    // the frame's new words become rows of this rank's shard on the device (shard_append): they need postings keys and an owner whether or
    // not the frame is registered as a signature (a query-only frame: the single-GPU path reserves keys whenever frame_appends() holds)
    const bool dev_append = h->shard_append && (flags & LCD_Q_INCREMENTAL) && first_new_word_id > 0;
    if (cyclic && (sig_id != 0 || dev_append) && first_new_word_id > 0 && (flags & LCD_Q_INCREMENTAL) && first_new_word_id < h->shard_first)
        return h->fail(LCD_ERR_INVALID, "lcd_shard_frame_dev: first_new_word_id lies in front of shard_growth_first");
    const int have_index = total_live_rows >= 2 ? 1 : 0;
    const bool incremental = (flags & LCD_Q_INCREMENTAL) != 0;
    const bool together = incremental && (flags & LCD_Q_NEW_WORDS_COMPARED);
    const int ld = (q + 63) / 64 * 64, bw = ld / 32;
    // the merge rides at the head of the same-frame distance launch when the frame has one that can carry it (one launch less per frame and rank)
    const bool have_matrix = together && matrix_left;
    const bool merge_in_selfdist = together && !have_matrix && selfdist_can_merge(h->dtype, h->kdim);
    if (have_matrix) {
        LCD_HIP(h, dreserve(h, h->d_bits, (size_t)q * bw * 4));
        ShardMergeJob mj;
        mj.cand = reinterpret_cast<const ShardCand*>(d_all_cand); mj.world = world; mj.rank = rank; mj.by_word = cyclic ? 1 : 0;
        mj.out_word = h->d_knn_word.as<int32_t>(); mj.out_dist = h->d_knn_dist.as<float>(); mj.out_wslot = h->d_knn_row.as<int32_t>();
        CandBits cb;
        cb.selfdist = h->d_shard_selfdist.as<float>(); cb.ld = ld; cb.nq = q; cb.bits = h->d_bits.as<uint32_t>(); cb.bw = bw; cb.have_index = have_index;
        LCD_HIP(h, launch_shard_merge_bits(mj, cb, h->stream));
    } else if (!merge_in_selfdist)
        LCD_HIP(h, launch_shard_merge(d_all_cand, world, rank, q, h->d_knn_word.as<int32_t>(), h->d_knn_dist.as<float>(),
                                      h->d_knn_row.as<int32_t>(), h->stream, cyclic));
    if (together && !have_matrix) {
        LCD_HIP(h, dreserve(h, h->d_selfdist, (size_t)q * ld * 4));
        LCD_HIP(h, dreserve(h, h->d_bits, (size_t)q * bw * 4));
        ShardMergeJob mj;
        mj.cand = reinterpret_cast<const ShardCand*>(d_all_cand); mj.world = world; mj.rank = rank; mj.by_word = cyclic ? 1 : 0;
        mj.out_word = h->d_knn_word.as<int32_t>(); mj.out_dist = h->d_knn_dist.as<float>(); mj.out_wslot = h->d_knn_row.as<int32_t>();
        LCD_HIP(h, launch_selfdist(h->dtype, h->kdim, d_descriptors, q, h->d_selfdist.as<float>(), ld, h->stream, have_index,
                                   h->d_knn_word.as<int32_t>(), h->d_knn_dist.as<float>(), h->d_bits.as<uint32_t>(), bw,
                                   merge_in_selfdist ? &mj : nullptr));
    }
    LCD_HIP(h, dreserve(h, h->d_out_wslot, (size_t)q * 4));
    // new words: every rank reserves the same keys (identical call sequence => identical numbering); only the LAST rank, which
    // will hold their rows, references them
    WsRuns new_ws;
    if ((sig_id != 0 || dev_append) && first_new_word_id > 0 && incremental) {
        hipError_t e = t.keys.reserve_new_words(first_new_word_id, q, &new_ws);
        if (e == hipErrorInvalidValue) return h->fail(LCD_ERR_UNSUPPORTED, "lcd_shard_frame_dev: word ids must be below 2^28");
        if (e != hipSuccess) return h->hip_fail(e, "reserve_new_words");
        if (cyclic) {                                      // block-cyclic ownership of the frame's new words (balanced growth)
            new_ws.own_id0 = first_new_word_id; new_ws.own_first = h->shard_first; new_ws.own_block = h->shard_block;
            new_ws.own_rank = rank; new_ws.own_world = world;
        } else if (rank != world - 1) new_ws.n = 0;
    }
    const int rflags = (incremental ? LCD_Q_INCREMENTAL : 0) | (together ? LCD_Q_NEW_WORDS_COMPARED : 0);
    LCD_HIP(h, launch_resolve(q, rflags, nndr_ratio, have_index, h->d_knn_word.as<int32_t>(), h->d_knn_dist.as<float>(),
                              together ? (have_matrix ? h->d_shard_selfdist.as<float>() : h->d_selfdist.as<float>()) : nullptr, ld,
                              together ? h->d_bits.as<uint32_t>() : nullptr, bw,
                              d_word_ids, h->d_n_new.as<int32_t>(), h->stream, h->d_knn_row.as<int32_t>(), nullptr,
                              h->d_out_wslot.as<int32_t>(), &new_ws));
    ShardAppendJob app;
    if (dev_append) {
        // VWDictionary::update()'s append branch, this rank's share, on the device: the words the frame created that this rank owns become
        // rows of its shard before the next frame is searched (lcd_shard_knn2_dev catches the host's row mirror up: one synchronisation,
        // no lcd_vocab_append, nothing read back by the caller)
        LCD_HIP(h, h->applog.activate(h->n_rows, h->stream, &h->bytes_device));
        { int rc = ensure_append_capacity(h, h->applog.rows_ub(h->n_rows) + (int64_t)q); if (rc) return rc; }
        lcd_frame_args fa;
        std::memset(&fa, 0, sizeof(fa));
        fa.d_descriptors = d_descriptors; fa.first_new_word_id = first_new_word_id; fa.q = q;
        ResolveArgs ra;
        fill_append(h, fa, h->applog.vseq, true, &ra);
        // ... as a second workgroup of the registration's launch (the two chains need nothing of each other: one launch less per frame and rank)
        app.ap = ra.ap; app.new_ws = new_ws;               // (n == 0 on a rank that owns nothing in last-rank mode: it appends nothing either)
        app.codes = d_word_ids; app.q = q; app.rank = rank; app.world = world;
        app.own_first = cyclic ? h->shard_first : 0; app.own_block = cyclic ? h->shard_block : 0;
    }
    if (sig_id != 0) LCD_HIP(h, t.register_dev(sig_id, h->d_out_wslot.as<int32_t>(), q, q, N, nullptr, false, nullptr, nullptr, dev_append ? &app : nullptr));
    else LCD_HIP(h, t.query_dev(h->d_out_wslot.as<int32_t>(), q, N, nullptr, false, nullptr, nullptr, dev_append ? &app : nullptr));
    if (dev_append) h->applog.record(first_new_word_id, q, true, ShardOwnership{world, rank, app.own_first, app.own_block});   // (enqueued: the host's record of it)
    if (d_lfix) {
        LCD_HIP(h, t.score_fix((long long*)d_lfix));       // every slot written: no zero-fill needed
        h->likelihood_launches += 1;
    }
    return LCD_OK;
    LCD_CATCH(h)
}

int lcd_finalize_dev(lcd_engine* h, int64_t* d_lfix, int64_t n, float* d_likelihood) {
    LCD_TRY
    LCD_CHECK_HANDLE(h);
    LCD_DEV_NODRAIN(h);
    { int rc = drain_keep_rows_lazy(h); if (rc) return rc; }
    if (n < 0 || (n > 0 && (!d_lfix || !d_likelihood))) return h->fail(LCD_ERR_INVALID, "lcd_finalize_dev: bad argument");
    if (n > h->tfidf.n_slots) return h->fail(LCD_ERR_INVALID, "lcd_finalize_dev: more entries than signature slots");
    LCD_HIP(h, h->tfidf.finalize((const long long*)d_lfix, (long long)n, d_likelihood));
    return LCD_OK;
    LCD_CATCH(h)
}

int lcd_slots_dev(lcd_engine* h, const int32_t** d_slot_sig, int64_t* n_slots) {
    LCD_TRY
    LCD_CHECK_HANDLE(h);
    { int rc = drain_keep_rows_lazy(h); if (rc) return rc; }           // (the slot table does not depend on the row mirror)
    if (d_slot_sig) *d_slot_sig = h->tfidf.slot_sig.as<int32_t>();
    if (n_slots) *n_slots = h->tfidf.n_slots;
    return LCD_OK;
    LCD_CATCH(h)
}

int lcd_profile_begin(lcd_engine* h, int max_samples) {
    LCD_TRY
    LCD_CHECK_HANDLE(h);
    LCD_DEV(h);
    if (max_samples <= 0 || max_samples > (1 << 20)) return h->fail(LCD_ERR_INVALID, "lcd_profile_begin: bad sample count");
    while ((int)h->prof_ev.size() < 2 * max_samples) {
        hipEvent_t e;
        LCD_HIP(h, hipEventCreate(&e));
        h->prof_ev.push_back(e);
        LCD_HIP(h, hipEventCreate(&e));
        h->prof_ev.push_back(e);
        LCD_HIP(h, hipEventCreate(&e));
        h->prof2_ev.push_back(e);
        LCD_HIP(h, hipEventCreate(&e));
        h->prof2_ev.push_back(e);
    }
    h->prof_n = 0;
    h->prof2_n = 0;
    h->prof_cap = max_samples;
    return LCD_OK;
    LCD_CATCH(h)
}

int lcd_profile_read(lcd_engine* h, float* avg_ms, int* n_samples, const char** kernel_name) {
    LCD_TRY
    LCD_CHECK_HANDLE(h);
    LCD_DEV(h);
    { int rc = h->sync_all(); if (rc) return rc; }
    double sum = 0.0;
    for (int i = 0; i < h->prof_n; ++i) {
        float ms = 0.0f;
        LCD_HIP(h, hipEventElapsedTime(&ms, h->prof_ev[2 * i], h->prof_ev[2 * i + 1]));
        sum += ms;
    }
    if (avg_ms) *avg_ms = h->prof_n ? (float)(sum / h->prof_n) : 0.0f;
    if (n_samples) *n_samples = h->prof_n;
    if (kernel_name) *kernel_name = h->prof_kernel;
    h->prof_cap = 0;
    return LCD_OK;
    LCD_CATCH(h)
}

int lcd_profile_read_likelihood(lcd_engine* h, float* avg_ms, int* n_samples, const char** kernel_name) {
    LCD_TRY
    LCD_CHECK_HANDLE(h);
    LCD_DEV(h);
    { int rc = h->sync_all(); if (rc) return rc; }
    double sum = 0.0;
    for (int i = 0; i < h->prof2_n; ++i) {
        float ms = 0.0f;
        LCD_HIP(h, hipEventElapsedTime(&ms, h->prof2_ev[2 * i], h->prof2_ev[2 * i + 1]));
        sum += ms;
    }
    if (avg_ms) *avg_ms = h->prof2_n ? (float)(sum / h->prof2_n) : 0.0f;
    if (n_samples) *n_samples = h->prof2_n;
    if (kernel_name) *kernel_name = h->prof2_kernel;
    h->prof_cap = 0;
    return LCD_OK;
    LCD_CATCH(h)
}

int lcd_set_option(lcd_engine* h, const char* key, int64_t value) {
    LCD_TRY
    LCD_CHECK_HANDLE(h);
    { int rc = h->drain(); if (rc) return rc; }
    if (!key) return h->fail(LCD_ERR_INVALID, "lcd_set_option: null key");
    if (!std::strcmp(key, "score_block") && (value == 256 || value == 512 || value == 1024)) { h->tfidf.score_block = (int)value; return LCD_OK; }
    // compute units the bf16 filter's persistent launch plans for (vocabularies of more 256-word strips than that): -1 built-in, 0 off
    if (!std::strcmp(key, "filter_units") && value >= -1 && value <= 4096) { h->filter_units = (int)value; return LCD_OK; }
    if (!std::strcmp(key, "strip_tiles") && value >= 0 && value <= 8) { h->strip_tiles = (int)value; return LCD_OK; }
    if (!std::strcmp(key, "shard_growth_first") && value >= 0 && value < (1ll << 28)) { h->shard_first = (int32_t)value; return LCD_OK; }
    if (!std::strcmp(key, "shard_growth_block") && value >= 0 && value <= (1 << 20)) { h->shard_block = (int32_t)value; return LCD_OK; }
    if (!std::strcmp(key, "shard_append") && (value == 0 || value == 1)) { h->shard_append = (int)value; return LCD_OK; }
    // 0: lcd_profile_begin brackets only the 2-NN launch of a pipelined frame (an event pair costs the stream ~10 us)
    if (!std::strcmp(key, "profile_likelihood") && (value == 0 || value == 1)) { h->prof_likelihood = value != 0; return LCD_OK; }
    // (per handle, like every option) sealed buckets from which the rows of a deferred append are written by a launch of their own; -1: built-in
    if (!std::strcmp(key, "append_split_buckets") && value >= -1 && value <= (1 << 24)) { h->popt.append_split_buckets = (int)value; return LCD_OK; }
    if (!std::strcmp(key, "cross_frame_tiles") && value >= -1 && value <= 1) { h->popt.cross_frames = value > 0 ? 1 : 0; return LCD_OK; }
    if (!std::strcmp(key, "append_from_rerank") && value >= -1 && value <= 1) { h->popt.append_from_rerank = value != 0 ? 1 : 0; return LCD_OK; }
    if (!std::strcmp(key, "roctx") && (value == 0 || value == 1)) {
        if (!value) { h->roctx_push = nullptr; h->roctx_pop = nullptr; return LCD_OK; }
        static void* lib = nullptr;                                  // (stays loaded: ranges of other handles may be open)
        if (!lib) lib = dlopen("libroctx64.so", RTLD_NOW | RTLD_GLOBAL);
        if (!lib) lib = dlopen("libroctx64.so.4", RTLD_NOW | RTLD_GLOBAL);
        if (!lib) lib = dlopen("/opt/rocm/lib/libroctx64.so", RTLD_NOW | RTLD_GLOBAL);
        if (!lib) return h->fail(LCD_ERR_UNSUPPORTED, "lcd_set_option(roctx): libroctx64.so not found");
        h->roctx_push = reinterpret_cast<int (*)(const char*)>(dlsym(lib, "roctxRangePushA"));
        h->roctx_pop = reinterpret_cast<int (*)()>(dlsym(lib, "roctxRangePop"));
        if (!h->roctx_push || !h->roctx_pop) { h->roctx_push = nullptr; h->roctx_pop = nullptr; return h->fail(LCD_ERR_UNSUPPORTED, "lcd_set_option(roctx): roctxRangePushA / roctxRangePop not exported"); }
        return LCD_OK;
    }
    // timing experiments: the filter workgroups of launch A wait value x 64 clocks in front of their first request (the single-workgroup
    // chains of the launch then get their first round trip ahead of the strips' opening burst)
    if (!std::strcmp(key, "filter_delay") && value >= 0 && value <= 127) { h->popt.filter_delay = (int)value; return LCD_OK; }
    if (!std::strcmp(key, "shadow_rows") && value >= -1 && value <= 2) { h->popt.shadow_rows = value < 0 ? 1 : (int)value; return LCD_OK; }   // (-1: built-in = 1)
    if (!std::strcmp(key, "mirror_from_b") && value >= -1 && value <= 1) { h->popt.mirror_from_b = value != 0 ? 1 : 0; return LCD_OK; }
    if (!std::strcmp(key, "next_word_id") && value >= 1 && value < (1ll << 28)) { h->mirror.next_word_id = std::max(h->mirror.next_word_id, (int32_t)value); return LCD_OK; }   // (the drain above has brought the row mirror up to date)
    if (!std::strcmp(key, "profile_skip") && value >= 0 && value <= (1 << 20)) { h->prof_skip = (int)value; return LCD_OK; }
    if (!std::strcmp(key, "decision_straight") && value >= -1 && value <= 2) { h->popt.decision_straight = value >= 0 ? (int)value : PipeOpts().decision_straight; return LCD_OK; }
    if (!std::strcmp(key, "slots_from_rows") && value >= -1 && value <= 2) { h->popt.slots_from_rows = value >= 0 ? (int)value : PipeOpts().slots_from_rows; return LCD_OK; }
    // tests: the distance-block bytes lcd_match_pairs gives one group of pairs (0: built-in); a single pair always fits
    if (!std::strcmp(key, "pair_match_budget") && value >= 0 && value <= (1ll << 40)) { h->pairs.budget_bytes = value; return LCD_OK; }
    if (!std::strcmp(key, "row_writer_wgs") && value >= -1 && value <= 256) { h->popt.row_writer_wgs = value >= 0 ? (int)value : PipeOpts().row_writer_wgs; return LCD_OK; }
    return h->fail(LCD_ERR_INVALID, "lcd_set_option: unknown key or value");
    LCD_CATCH(h)
}

int lcd_trace_push(lcd_engine* h, const char* name) {
    if (!h || !name) return LCD_ERR_INVALID;
    if (h->roctx_push) h->roctx_push(name);
    return LCD_OK;
}
int lcd_trace_pop(lcd_engine* h) {
    if (!h) return LCD_ERR_INVALID;
    if (h->roctx_pop) h->roctx_pop();
    return LCD_OK;
}

int lcd_profile_score_work(lcd_engine* h, int64_t* out8) {
    LCD_TRY
    LCD_CHECK_HANDLE(h);
    LCD_DEV(h);
    if (!out8) return h->fail(LCD_ERR_INVALID, "lcd_profile_score_work: null output");
    { int rc = h->sync_all(); if (rc) return rc; }
    LCD_HIP(h, h->tfidf.score_work(out8));
    return LCD_OK;
    LCD_CATCH(h)
}

int lcd_get_stats(lcd_engine* h, lcd_stats* out) {
    LCD_TRY
    LCD_CHECK_HANDLE(h);
    if (!out) return LCD_ERR_INVALID;
    LCD_DEV(h);
    { int rc = h->sync_all(); if (rc) return rc; }
    out->knn_last_fallback_queries = 0;
    out->knn_max_err_ratio = 0.0;
    const void* fc = h->last_fail_count ? h->last_fail_count : h->d_fail_count.p;
    if (fc) {
        int32_t n[3] = {0, 0, 0};
        int rc = download(h, n, fc, 12, h->h_out2);
        if (rc) return rc;
        out->knn_last_fallback_queries = n[0];
        float r;
        std::memcpy(&r, &n[2], 4);
        out->knn_max_err_ratio = r;
    }
    out->vocab_rows = h->n_rows; out->vocab_live = h->n_live;
    out->signatures = h->tfidf.live_sigs; out->postings = h->tfidf.postings_ub;
    out->knn_launches = h->knn_launches; out->likelihood_launches = h->likelihood_launches; out->rebuilds = h->rebuilds;
    h->tfidf.keys.harvest_released(false);
    out->frame_calls = h->frame_calls; out->frame_host_ns = h->frame_host_ns;
    out->buckets_sealed = h->tfidf.seals;
    out->word_slots = h->tfidf.keys.in_use();
    out->dense_words = h->tfidf.h_n_dense ? (int64_t)*(volatile uint32_t*)h->tfidf.h_n_dense : 0;
    out->bytes_device = h->bytes_device;
    out->clean_divergent_refs = 0;
    if (h->tfidf.q_meta.p) {
        uint32_t n = 0;
        int rc = download(h, &n, h->tfidf.q_meta.as<uint32_t>() + 8, 4, h->h_out2);
        if (rc) return rc;
        out->clean_divergent_refs = (int64_t)n;
    }
    return LCD_OK;
    LCD_CATCH(h)
}

}  // extern "C"
