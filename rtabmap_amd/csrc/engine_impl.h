// engine_impl.h -- what the translation units that implement the C-ABI (engine.hip, frame_pipeline.hip) share: the entry-point macros and
// the small helpers both call per frame (static inline: no per-frame call crosses a file, nothing is added to the exported symbols).  Not part of the ABI.
#pragma once
#include "engine.h"

#include <cstring>
#include <new>

#define LCD_CHECK_HANDLE(h) do { if (!(h)) return LCD_ERR_INVALID; } while (0)
#define LCD_HIP(h, x) do { hipError_t e__ = (x); if (e__ != hipSuccess) return (h)->hip_fail(e__, #x); } while (0)
// every entry selects the device; every entry except lcd_frame_dev / lcd_sig_remove / lcd_record_event first completes the index
// stage a pipelined handle still owes for its last frame
#define LCD_DEV_NODRAIN(h) LCD_HIP(h, hipSetDevice((h)->device))
#define LCD_DEV(h) do { LCD_DEV_NODRAIN(h); int rc__ = (h)->drain(); if (rc__) return rc__; } while (0)

// No exception crosses the C-ABI (lcd.h): the bookkeeping of every entry point uses std:: containers, whose allocations may throw
static inline int lcd_catch(const lcd_engine* h, int code, const char* what) noexcept {
    if (h) { try { const_cast<lcd_engine*>(h)->err = what; } catch (...) { } }
    return code;
}
#define LCD_TRY try {
#define LCD_CATCH(h) } catch (const std::bad_alloc&) { return lcd_catch(h, LCD_ERR_NOMEM, "out of host memory"); } \
    catch (const std::exception& e__) { return lcd_catch(h, LCD_ERR_STATE, e__.what()); } \
    catch (...) { return lcd_catch(h, LCD_ERR_STATE, "unexpected exception"); }

static inline hipError_t dreserve(lcd_engine* h, lcd::DevBuf& b, size_t bytes, size_t keep = 0) {
    return b.reserve(bytes, keep, h->stream, &h->bytes_device);
}

// u8 rows whose `dim` is no multiple of 4 are stored zero-padded (row_bytes > dim): a caller's [q x dim] DEVICE buffer does not have the layout
// the kernels walk (they stride by row_bytes), so every entry point that takes one refuses such a handle; host rows are padded as they are staged
static inline size_t host_row_bytes(const lcd_engine* h) { return (size_t)h->dim * (h->dtype == LCD_F32 ? 4 : 1); }
static inline bool rows_padded(const lcd_engine* h) { return (size_t)h->row_bytes != host_row_bytes(h); }

// The body of a stateless entry point and of its _dev form (stateless_scratch.h lists the calls): nothing is drained, the
// roctx range carries the base name for both
template <typename Args>
static inline int stateless_entry(lcd_engine* h, const char* name, int (*call)(lcd_engine*, const Args*, bool), const Args* a, bool on_device) {
    LCD_TRY
    LCD_CHECK_HANDLE(h);
    lcd_engine::Range range__(h, name);
    LCD_DEV_NODRAIN(h);
    return call(h, a, on_device);
    LCD_CATCH(h)
}

// ---- VWDictionary::update()'s append branch on the device (see engine.h)
static inline int64_t vocab_cap_rows(const lcd_engine* h) {
    int64_t c = (int64_t)(h->vocab.cap / (size_t)h->row_bytes);
    c = std::min<int64_t>(c, (int64_t)(h->row_id.cap / 4));
    c = std::min<int64_t>(c, (int64_t)(h->row_wslot.cap / 4));
    if (h->dtype == LCD_F32) c = std::min<int64_t>(c, (int64_t)(h->row_norm.cap / 8) - 1);
    if (lcd::knn_mfma_supported(h->dtype, h->kdim)) c = std::min<int64_t>(c, (int64_t)(h->vocab_bf.cap / 256));
    return std::max<int64_t>(c, 0);
}

// the row buffers hold `rows` rows; what lies behind the rows in use carries +inf norms and a zero bf16 split
static inline int ensure_append_capacity(lcd_engine* h, int64_t rows) {
    const int64_t keep = h->applog.rows_ub(h->n_rows);
    if (rows > vocab_cap_rows(h)) {
        LCD_HIP(h, dreserve(h, h->vocab, (size_t)rows * h->row_bytes, (size_t)keep * h->row_bytes));
        LCD_HIP(h, dreserve(h, h->row_id, (size_t)rows * 4, (size_t)keep * 4));
        LCD_HIP(h, dreserve(h, h->row_wslot, (size_t)rows * 4, (size_t)keep * 4));
        if (h->dtype == LCD_F32) LCD_HIP(h, dreserve(h, h->row_norm, ((size_t)rows + 1) * 8, ((size_t)keep + 1) * 8));
        if (lcd::knn_mfma_supported(h->dtype, h->kdim)) LCD_HIP(h, dreserve(h, h->vocab_bf, (size_t)rows * 256, (size_t)keep * 256));
        h->tail_filled_rows = std::min(h->tail_filled_rows, keep);
    }
    const int64_t cap = vocab_cap_rows(h);
    const int64_t first = std::max(h->tail_filled_rows, keep);
    if (first < cap) {
        if (lcd::knn_mfma_supported(h->dtype, h->kdim)) LCD_HIP(h, lcd::launch_vocab_tail(h->row_norm.as<float>(), h->vocab_bf.p, first, cap - first, h->stream));
        // row id 0 behind the rows: a scan planned for an upper bound of the row count skips what does not exist yet like a tombstone
        LCD_HIP(h, hipMemsetAsync(h->row_id.as<int32_t>() + first, 0, (size_t)(cap - first) * 4, h->stream));
        h->tail_filled_rows = cap;
    }
    return LCD_OK;
}

// the append (or, for a frame that appends nothing, the hand-over of the row count) that rides with the decision loop of chain frame `vseq`
static inline void fill_append(lcd_engine* h, const lcd_frame_args& a, uint64_t vseq, bool enabled, lcd::ResolveArgs* r, uint32_t* list_out = nullptr) {
    lcd::AppendArgs& ap = r->ap;
    ap = lcd::AppendArgs();
    ap.enabled = enabled ? 1 : 0;
    // pipelined frames of 64-float rows: the decision loop publishes the list, workgroups of launch B write the rows (append_rows_body)
    if (list_out && lcd::knn_mfma_supported(h->dtype, h->kdim)) { ap.defer_rows = 1; ap.list_out = list_out; }
    ap.descriptors = (const float*)a.d_descriptors; ap.row_dwords = h->row_bytes / 4; ap.is_f32_64 = lcd::knn_mfma_supported(h->dtype, h->kdim) ? 1 : 0;
    ap.vocab = h->vocab.as<uint32_t>(); ap.row_id = h->row_id.as<int32_t>(); ap.row_wslot = h->row_wslot.as<int32_t>();
    ap.row_norm = h->row_norm.as<float>(); ap.norm_max_bits = h->norm_max.as<uint32_t>(); ap.vocab_bf = h->vocab_bf.as<uint32_t>();
    ap.wrow = h->tfidf.keys.wrow.as<uint32_t>(); ap.f16 = h->f16();
    ap.cnt_in = h->applog.count_before(vseq); ap.cnt_out = h->applog.count_after(vseq); ap.log_slot = h->applog.log_slot(vseq);
    ap.first_id = h->applog.first_id(a.first_new_word_id); ap.capacity = vocab_cap_rows(h);
    ap.first_out = (int32_t*)a.d_first_new_word_id;
    ap.host_mirror = h->applog.h_vmirror; ap.tag = (uint32_t)(vseq + 1);
}

// device part of addNewWords up to (not including) the decision loop (engine.hip): 2-NN, same-frame distances + candidate bits
__attribute__((visibility("hidden")))
int prepare_resolve(lcd_engine* h, const void* d_desc, int q, int flags, float nndr, int32_t* d_out_word, int32_t* d_out_wslot,
                    lcd::ResolveArgs* r, bool defer_redo = false /* the caller's next launch is the fused frame tail */,
                    int64_t rows_now = -1 /* rows to scan when the host's count lags the device's (an upper bound: the rows behind the
                                             device's count carry row id 0 and are skipped like tombstones) */);
