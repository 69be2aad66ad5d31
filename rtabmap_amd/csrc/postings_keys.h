// postings_keys.h -- the lifecycle of postings keys (internal to liblcd_hip.so).
//
// A word of the inverted index (tfidf.h) is known to the kernels by its POSTINGS KEY ("wslot"), a dense index into the per-key tables.  A key is
// handed out when a word is first seen, or reserved for a word the coming frame may create, and handed out again only after the device has
// confirmed it free: no vocabulary row claims it (wrow == 0) and no live signature references it (nw == 0).  KeyPool owns it in between.
#pragma once
#include <map>
#include <vector>

#include "devbuf.h"
#include "lcd_kernels.h"

namespace lcd {

// The free keys as maximal intervals (start -> length) and their number.  Host only.
struct KeyIntervals {
    std::map<int32_t, int32_t> runs;
    int64_t count = 0;
    void free_key(int32_t w);                      // a key that is already free is ignored
    void free_run(int32_t start, int32_t len);     // consecutive keys, one operation (a run that overlaps the set: key by key)
    void free_verdicts(const int32_t* keys, const uint8_t* ok, size_t n);   // keys[k] with ok[k] == 1, consecutive keys coalesced into runs
    // up to `want` keys, the highest interval first, of each interval its top min(length, left) keys: start[r] / len[r] of at
    // most max_runs runs; returns the number of runs (it stops early only when the set is empty)
    int take_runs(int32_t want, int max_runs, int32_t* start, int32_t* len);
    int32_t take() { int32_t s, l; return take_runs(1, 1, &s, &l) ? s : -1; }   // the highest free key, or -1
};

struct KeyPool {
    static constexpr size_t CHECK_BATCH = 16384;   // held keys that make one check launch (~32 frames' worth, not one per frame)
    hipStream_t stream = nullptr; int64_t* bytes_device = nullptr;   // the owning Tfidf's (set by its init)
    // per key, on the device (one function grows them all: ensure_keys)
    DevBuf nw, did;                      // references, dense id (-1: none)
    DevBuf wrow;                         // vocabulary row that carries the key + 1 (0: none): a key held by a live row is never recycled, whatever
                                         // its reference count (rows appended on the device get their key there, the host learns of it later)
    DevBuf idf_tab;                      // {stamp, idf Q5.26} of the words of the current frame (valid iff stamp matches)
    KeyIntervals free;                   // recycled keys (confirmed unused by the device)
    void destroy();
    hipError_t ensure_keys(int32_t n);   // the per-key tables hold n keys
    int32_t n_keys() const { return n_wslots; }                    // keys ever handed out
    int64_t in_use() const { return (int64_t)n_wslots - free.count; }
    // key of a word id (assigned on first sight when `create`); -1 if unknown and !create
    hipError_t key_of(int32_t word_id, bool create, int32_t* out);
    bool known(int32_t word_id) const { return (size_t)word_id < id2ws.size() && id2ws[word_id] >= 0; }   // one vector read
    void bind(int32_t word_id, int32_t key) {
        if ((size_t)word_id >= id2ws.size()) id2ws.resize((size_t)word_id + 1 + id2ws.size() / 2, -1);
        id2ws[word_id] = key; id2ws_dirty.push_back(word_id);
    }
    void unbind(int32_t word_id) { id2ws[word_id] = -1; id2ws_dirty.push_back(word_id); }
    hipError_t sync_id2ws();             // bring the device copy of the id -> key table (xlate / xlate_n) up to date
    const int32_t* xlate() const { return d_id2ws.as<int32_t>(); }
    int64_t xlate_n() const { return d_id2ws_n; }
    // the words left the dictionary (VWDictionary::removeWords): their keys are recycled once the device confirms them free
    hipError_t release_words(const int32_t* word_ids, int n);
    // recheck: keys without a word id that turn out to be still referenced are checked again with a later batch
    hipError_t release_keys(const std::vector<int32_t>& ws, const std::vector<int32_t>* ids = nullptr, bool recheck = false);
    void harvest_released(bool wait);
    // reserve n keys for the new words first_id, first_id + 1, ... of the coming frame (recycled intervals first)
    // may_flush = false: the batched check of superseded reservations is not launched here (a pipelined handle launches it with
    // flush_held_if_due() once the registration that may still use those keys is enqueued)
    hipError_t reserve_new_words(int32_t first_id, int n, WsRuns* runs, bool may_flush = true);
    hipError_t flush_held();
    hipError_t flush_held_if_due() { return held_ws.size() >= CHECK_BATCH ? flush_held() : hipSuccess; }
    // a word the device numbered and keyed (LCD_NEW_WORD_IDS_AUTO): id and key read from its row at reconciliation
    void adopt_key(int32_t word_id, int32_t ws) { if (word_id > 0 && ws >= 0 && !known(word_id)) bind(word_id, ws); }
    // the device tombstoned the row of word `word_id` (key `ws`): if that is the word's permanent key it goes to the batched check
    void forget_word(int32_t word_id, int32_t ws);
    // the vocabulary rows' claim on their keys (wrow): rows [first_row, first_row + n) carry d_ws[0 .. n); rows d_rows[0 .. n) are gone;
    // the vocabulary was cleared
    hipError_t rows_take_keys(const int32_t* d_ws, int n, int64_t first_row);
    hipError_t rows_drop_keys(const int32_t* d_row_wslot, const int32_t* d_rows, int n);
    hipError_t rows_clear() { return (wrow.p && n_wslots > 0) ? hipMemsetAsync(wrow.p, 0, (size_t)n_wslots * 4, stream) : hipSuccess; }
    // the device-side cleanUnusedWords keeps the keys of the rows it tombstones out of circulation (wrow = 0xFFFFFFFF) until the host has
    // caught up with its log of {row, key} pairs -- with nothing in flight: then they are released like any removed word's key
    hipError_t rows_unlog_keys(const int32_t* d_pairs, int n);
private:
    int32_t n_wslots = 0;
    // word id -> key: host vector (ids are small consecutive integers in the reference, ++_lastWordId) mirrored on the device
    std::vector<int32_t> id2ws;          // -1 = none
    DevBuf d_id2ws;
    int64_t d_id2ws_n = 0;               // entries valid on the device
    std::vector<int32_t> id2ws_dirty;    // ids whose device entry is out of date
    DevBuf d_pairs;                      // (id, key) pairs on their way into d_id2ws
    PinBuf h_stage;
    // keys on their way back: a kernel checks each and reports through pinned memory.  ids[i] != 0: the key was reserved for new
    // word ids[i] of a frame; if it turns out to be in use, that word exists and keeps the key.
    struct PinBlock { void* p = nullptr; size_t cap = 0; hipEvent_t ev = nullptr; };   // pinned memory + event, recycled (one batch per frame)
    std::vector<PinBlock> pin_free;
    struct ReleaseBatch { std::vector<int32_t> ws, ids; PinBlock blk; const uint8_t* ok = nullptr; bool recheck = false; };
    std::vector<ReleaseBatch> releasing;
    std::vector<int32_t> held_ws, held_ids;   // keys of superseded reservations waiting for a batched check
    std::vector<int32_t> ghost_ws;            // keys of removed words that a batch found still referenced: asked about again every 8th batch
    uint32_t flushes = 0;
    struct Reservation { int32_t first_id = 0, n = 0; WsRuns runs; } resv;   // keys reserved for the new words of the last frame
};

}  // namespace lcd
