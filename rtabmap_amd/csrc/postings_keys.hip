// postings_keys.hip -- the free set of postings keys and their single owner (see postings_keys.h).
#include "postings_keys.h"

#include <algorithm>
#include <cstring>
#include <iterator>

namespace lcd {
namespace {

// the words left the dictionary: a wslot may be handed out again only if nothing references it (ok[i] tells the host)
// verdict: 1 = free (nothing references the key and no vocabulary row carries it), 2 = a live row's key (permanent, whatever its reference
// count: a word a frame appended on the device whose signature is gone, or that never had one), 0 = still referenced
__global__ void wslot_release_kernel(const int32_t* __restrict__ ws, int n, const uint32_t* __restrict__ nw, const uint32_t* __restrict__ wrow,
                                     int32_t* __restrict__ did, uint2* __restrict__ idf_tab, uint8_t* __restrict__ ok) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t w = ws[i];
    const bool is_row = wrow[w] != 0u;
    const bool free_now = !is_row && nw[w] == 0u;
    if (free_now) { did[w] = -1; idf_tab[w] = make_uint2(0u, 0u); }
    ok[i] = free_now ? 1 : (is_row ? 2 : 0);
}
// rows [first_row, first_row + n) carry the keys ws[0 .. n)
__global__ void wrow_set_kernel(const int32_t* __restrict__ ws, int n, long long first_row, uint32_t* __restrict__ wrow) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && ws[i] >= 0) wrow[ws[i]] = (uint32_t)(first_row + i) + 1u;
}
// the keys of logged removals ({row, key} pairs) leave their quarantine
__global__ void wrow_unlog_kernel(const int32_t* __restrict__ pairs, int n, uint32_t* __restrict__ wrow) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t w = pairs[2 * i + 1];
    if (w >= 0 && wrow[w] == 0xFFFFFFFFu) wrow[w] = 0u;
}
// the rows rows[0 .. n) are gone: their keys belong to no row any more
__global__ void wrow_clear_kernel(const int32_t* __restrict__ row_wslot, const int32_t* __restrict__ rows, int n, uint32_t* __restrict__ wrow) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t w = row_wslot[rows[i]];
    if (w >= 0) wrow[w] = 0u;
}
// table[pairs[2i]] = pairs[2i + 1]
__global__ void scatter_pairs_kernel(const int32_t* __restrict__ pairs, int n, int32_t* __restrict__ table) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) table[pairs[2 * i]] = pairs[2 * i + 1];
}

}  // namespace

// [start, start + len), which overlaps nothing in the set, becomes free: merged with the intervals that touch it (next = lower_bound(start))
static void insert_run(std::map<int32_t, int32_t>& runs, std::map<int32_t, int32_t>::iterator next, int32_t start, int32_t len) {
    if (next != runs.begin()) {
        auto prev = std::prev(next);
        if (prev->first + prev->second == start) { start = prev->first; len += prev->second; runs.erase(prev); }
    }
    if (next != runs.end() && next->first == start + len) { len += next->second; runs.erase(next); }
    runs[start] = len;
}
void KeyIntervals::free_key(int32_t w) {
    auto next = runs.lower_bound(w);
    if (next != runs.begin() && std::prev(next)->first + std::prev(next)->second > w) return;   // already free (cannot happen)
    insert_run(runs, next, w, 1); count += 1;
}
void KeyIntervals::free_run(int32_t start, int32_t len) {
    if (len <= 0) return;
    auto next = runs.lower_bound(start);
    const bool clash_next = next != runs.end() && next->first < start + len;
    const bool clash_prev = next != runs.begin() && std::prev(next)->first + std::prev(next)->second > start;
    if (len == 1 || clash_next || clash_prev) {                          // (an overlap cannot happen; key by key it is at least ignored safely)
        for (int32_t k = 0; k < len; ++k) free_key(start + k);
        return;
    }
    insert_run(runs, next, start, len); count += len;                     // one interval operation for the whole run
}

// the verdicts of a batch are mostly "free" for long runs of consecutive keys (what a frame reserved and did not use): a run
// goes back into the interval set with ONE operation -- key by key a batch of 16 384 keys kept the host busy for ~0.2 ms, a
// pause of the enqueueing thread every ~40 frames
void KeyIntervals::free_verdicts(const int32_t* keys, const uint8_t* ok, size_t n) {
    int32_t run_start = 0, run_len = 0;
    for (size_t k = 0; k < n; ++k) {
        if (ok[k] != 1) continue;
        if (run_len > 0 && keys[k] == run_start + run_len) { run_len += 1; continue; }
        free_run(run_start, run_len);
        run_start = keys[k]; run_len = 1;
    }
    free_run(run_start, run_len);
}

int KeyIntervals::take_runs(int32_t want, int max_runs, int32_t* start, int32_t* len) {
    int n = 0;
    for (int32_t left = want; left > 0 && n < max_runs && !runs.empty(); ++n) {
        auto it = std::prev(runs.end());
        const int32_t take = std::min(it->second, left);
        start[n] = it->first + it->second - take; len[n] = take;
        if ((it->second -= take) == 0) runs.erase(it);
        count -= take;
        left -= take;
    }
    return n;
}

void KeyPool::destroy() {
    harvest_released(true);
    for (PinBlock& b : pin_free) { (void)hipEventDestroy(b.ev); (void)hipHostFree(b.p); }
    pin_free.clear();
    for (DevBuf* d : {&nw, &did, &wrow, &idf_tab, &d_id2ws, &d_pairs}) d->release(bytes_device);
    h_stage.release();
}

hipError_t KeyPool::ensure_keys(int32_t n) {
    TF_TRY(grow_zeroed(nw, (size_t)n * 4, stream, bytes_device));
    TF_TRY(grow_filled(did, (size_t)n * 4, 0xFF, stream, bytes_device));
    TF_TRY(grow_zeroed(wrow, (size_t)n * 4, stream, bytes_device));
    TF_TRY(grow_zeroed(idf_tab, (size_t)n * 8, stream, bytes_device));
    return hipSuccess;
}

hipError_t KeyPool::key_of(int32_t word_id, bool create, int32_t* out) {
    *out = -1;
    if (word_id <= 0) return hipSuccess;
    if (known(word_id)) { *out = id2ws[word_id]; return hipSuccess; }
    int32_t w = -1;
    if (resv.n > 0 && resv.first_id > 0 && word_id >= resv.first_id && word_id < resv.first_id + resv.n) {
        // a new word of the last device-quantised frame: its key was reserved when the frame was enqueued
        w = ws_runs_at(resv.runs, word_id - resv.first_id);
    } else {
        // a new word of an earlier frame whose reservation is being checked by the device: the verdict decides whether it exists
        if (std::find(held_ids.begin(), held_ids.end(), word_id) != held_ids.end()) { TF_TRY(flush_held()); harvest_released(true); }
        for (size_t i = 0; i < releasing.size(); ++i) {
            const ReleaseBatch& r = releasing[i];
            if (std::find(r.ids.begin(), r.ids.end(), word_id) != r.ids.end()) { harvest_released(true); break; }
        }
        if (known(word_id)) { *out = id2ws[word_id]; return hipSuccess; }
        if (!create) return hipSuccess;
        if (word_id >= (1 << 28)) return hipErrorInvalidValue;        // the id -> key table is direct-indexed
        harvest_released(false);
        w = free.take();
        if (w < 0) { w = n_wslots++; TF_TRY(ensure_keys(n_wslots)); }
    }
    bind(word_id, w);
    *out = w;
    return hipSuccess;
}

// the entries changed since the last call travel as (id, key) pairs
hipError_t KeyPool::sync_id2ws() {
    TF_TRY(grow_filled(d_id2ws, std::max<size_t>(id2ws.size(), 1) * 4, 0xFF, stream, bytes_device));
    d_id2ws_n = (int64_t)(d_id2ws.cap / 4);
    if (id2ws_dirty.empty()) return hipSuccess;
    const size_t m = id2ws_dirty.size();
    TF_TRY(h_stage.reserve(m * 8));
    int32_t* st = h_stage.as<int32_t>();
    for (size_t i = 0; i < m; ++i) { st[2 * i] = id2ws_dirty[i]; st[2 * i + 1] = id2ws[id2ws_dirty[i]]; }
    TF_TRY(d_pairs.reserve(m * 8, 0, stream, bytes_device));
    TF_TRY(hipMemcpyAsync(d_pairs.p, st, m * 8, hipMemcpyHostToDevice, stream));
    scatter_pairs_kernel<<<(unsigned)((m + 255) / 256), 256, 0, stream>>>(d_pairs.as<int32_t>(), (int)m, d_id2ws.as<int32_t>());
    TF_TRY(hipGetLastError());
    TF_TRY(hipStreamSynchronize(stream));                             // staging buffers are reused
    id2ws_dirty.clear();
    return hipSuccess;
}

void KeyPool::harvest_released(bool wait) {
    for (size_t i = 0; i < releasing.size();) {
        ReleaseBatch& r = releasing[i];
        const hipError_t q = wait ? hipEventSynchronize(r.blk.ev) : hipEventQuery(r.blk.ev);
        if (q != hipSuccess) { ++i; continue; }
        free.free_verdicts(r.ws.data(), r.ok, r.ws.size());
        for (size_t k = 0; k < r.ws.size(); ++k) {
            if (r.ok[k] == 1) continue;
            // still referenced, or the key of a vocabulary row.  A key reserved for a frame's new word: the word exists (the frame
            // created it) and keeps it.
            const int32_t id = k < r.ids.size() ? r.ids[k] : 0;
            if (id > 0) {
                if (!known(id)) bind(id, r.ws[k]);
            } else if (r.ok[k] == 0 && r.recheck) {
                // a key without a word: the word was removed from the dictionary while a frame in flight still matched it (its row is
                // tombstoned, the references of that frame's signature remain).  It comes back when those references are gone.
                ghost_ws.push_back(r.ws[k]);
            }
        }
        pin_free.push_back(r.blk);
        releasing.erase(releasing.begin() + i);
    }
}

// hand keys back: a kernel checks each one and reports through pinned memory; the host collects the verdicts of finished batches
// later (harvest_released), so nothing is synchronised here and a key that is still in use is never handed out again
hipError_t KeyPool::release_keys(const std::vector<int32_t>& ws, const std::vector<int32_t>* ids, bool recheck) {
    if (ws.empty()) return hipSuccess;
    const size_t m = ws.size();
    ReleaseBatch r;
    r.ws = ws; r.recheck = recheck; if (ids) r.ids = *ids;
    const size_t need = m * 5 + 16;                                          // [m keys][m verdicts]
    for (size_t i = 0; i < pin_free.size(); ++i)
        if (pin_free[i].cap >= need) { r.blk = pin_free[i]; pin_free.erase(pin_free.begin() + i); break; }
    if (!r.blk.p) {
        r.blk.cap = 8192;
        while (r.blk.cap < need) r.blk.cap *= 2;
        TF_TRY(hipHostMalloc(&r.blk.p, r.blk.cap, hipHostMallocDefault));
        TF_TRY(hipEventCreateWithFlags(&r.blk.ev, hipEventDisableTiming));
    }
    int32_t* p_ws = (int32_t*)r.blk.p;
    uint8_t* p_ok = (uint8_t*)(p_ws + m);
    std::memcpy(p_ws, ws.data(), m * 4);
    std::memset(p_ok, 0, m);
    r.ok = p_ok;
    wslot_release_kernel<<<(unsigned)((m + 255) / 256), 256, 0, stream>>>(p_ws, (int)m, nw.as<uint32_t>(), wrow.as<uint32_t>(), did.as<int32_t>(),
                                                                           idf_tab.as<uint2>(), p_ok);
    TF_TRY(hipGetLastError());
    TF_TRY(hipEventRecord(r.blk.ev, stream));
    releasing.push_back(r);
    return hipSuccess;
}

hipError_t KeyPool::flush_held() {
    if (held_ws.empty()) return hipSuccess;
    std::vector<int32_t> ws, ids;
    ws.swap(held_ws); ids.swap(held_ids);
    if (!ghost_ws.empty() && (++flushes & 7u) == 0u) {                       // every 8th batch also asks about the keys that were still referenced
        ws.insert(ws.end(), ghost_ws.begin(), ghost_ws.end());
        ids.resize(ws.size(), 0);
        ghost_ws.clear();
    }
    return release_keys(ws, &ids, true);
}

hipError_t KeyPool::rows_take_keys(const int32_t* d_ws, int n, int64_t first_row) {
    if (n <= 0) return hipSuccess;
    wrow_set_kernel<<<(unsigned)((n + 255) / 256), 256, 0, stream>>>(d_ws, n, (long long)first_row, wrow.as<uint32_t>());
    return hipGetLastError();
}
hipError_t KeyPool::rows_drop_keys(const int32_t* d_row_wslot, const int32_t* d_rows, int n) {
    if (n <= 0) return hipSuccess;
    wrow_clear_kernel<<<(unsigned)((n + 255) / 256), 256, 0, stream>>>(d_row_wslot, d_rows, n, wrow.as<uint32_t>());
    return hipGetLastError();
}
hipError_t KeyPool::rows_unlog_keys(const int32_t* d_pairs, int n) {
    if (n <= 0) return hipSuccess;
    wrow_unlog_kernel<<<(unsigned)((n + 255) / 256), 256, 0, stream>>>(d_pairs, n, wrow.as<uint32_t>());
    return hipGetLastError();
}
void KeyPool::forget_word(int32_t word_id, int32_t ws) {
    if (word_id <= 0 || ws < 0 || !known(word_id) || id2ws[word_id] != ws) return;
    unbind(word_id);
    held_ws.push_back(ws); held_ids.push_back(0);
}

hipError_t KeyPool::release_words(const int32_t* word_ids, int n) {
    std::vector<int32_t> ws;
    for (int i = 0; i < n; ++i) {
        int32_t w = -1;
        TF_TRY(key_of(word_ids[i], false, &w));
        if (w >= 0) { unbind(word_ids[i]); ws.push_back(w); }
    }
    return release_keys(ws);
}

// Postings keys for the words the coming frame may create (at most n).  The previous frame's reservation is handed to the device
// for checking: keys it did not use (nw == 0) are recycled, used ones become the permanent keys of those words.
hipError_t KeyPool::reserve_new_words(int32_t first_id, int n, WsRuns* runs, bool may_flush) {
    runs->n = 0;
    // first_id == -1 (LCD_NEW_WORD_IDS_AUTO): the device numbers the words; the host learns id and key of each from its row when it catches up (adopt_key)
    if ((first_id <= 0 && first_id != -1) || n <= 0) return hipSuccess;
    if (first_id > 0 && (int64_t)first_id + n >= (1 << 28)) return hipErrorInvalidValue;
    if (resv.n > 0) {
        int32_t k = 0;
        for (int i = 0; i < resv.runs.n; ++i) {
            for (int32_t j = 0; j < resv.runs.len[i]; ++j, ++k) {
                const int32_t id = resv.first_id > 0 ? resv.first_id + k : 0;   // (0: numbered on the device -- the check only decides whether the key is in use)
                if (id > 0 && known(id)) continue;                               // already the word's permanent key
                held_ws.push_back(resv.runs.start[i] + j);
                held_ids.push_back((id > 0 && (first_id <= 0 || id < first_id)) ? id : 0);   // ids the caller is re-using now name other words
            }
        }
        resv.n = 0;
        if (may_flush) TF_TRY(flush_held_if_due());   // (the frame tail that may have used these keys is already enqueued)
    }
    harvest_released(false);
    runs->n = free.take_runs(n, 15, runs->start, runs->len);                  // recycled intervals first ...
    int left = n;
    for (int i = 0; i < runs->n; ++i) left -= runs->len[i];
    if (left > 0) {                                                           // ... the rest fresh
        runs->start[runs->n] = n_wslots; runs->len[runs->n] = left; runs->n += 1;
        n_wslots += left; TF_TRY(ensure_keys(n_wslots));
    }
    resv.first_id = first_id; resv.n = n; resv.runs = *runs;
    return hipSuccess;
}

}  // namespace lcd

// The interval set as the engine keeps it (host code, no device needed: tests).  keys[0 .. n) whose verdict ok[i] is 1 are freed -- by_runs:
// with KeyIntervals::free_verdicts, what harvest_released does, else key by key -- then `take` keys are taken back; out receives the intervals
// as (start, length) pairs in ascending order.  Returns the number of pairs (or -1 if out is too small); *count = free keys as the set counts them.
static int key_intervals_out(const lcd::KeyIntervals& s, int32_t* out, int cap, long long* count) {
    if ((int)s.runs.size() > cap) return -1;
    int k = 0;
    for (const auto& kv : s.runs) { out[2 * k] = kv.first; out[2 * k + 1] = kv.second; k += 1; }
    if (count) *count = (long long)s.count;
    return k;
}
extern "C" int lcd_debug_key_intervals(const int32_t* keys, const unsigned char* ok, int n, int by_runs, int take, int32_t* out, int cap, long long* count) {
    lcd::KeyIntervals s;
    if (by_runs) s.free_verdicts(keys, ok, (size_t)n);
    else for (int i = 0; i < n; ++i) if (ok[i] == 1) s.free_key(keys[i]);
    for (int i = 0; i < take; ++i) (void)s.take();
    return key_intervals_out(s, out, cap, count);
}
// the same set, freed by runs, after ONE take_runs(want, max_runs): out_runs receives the (start, length) pairs handed out in the order
// they were taken, out_left / count what is left.  Returns the number of runs handed out; *n_left = pairs in out_left (-1: too small).
extern "C" int lcd_debug_key_take_runs(const int32_t* keys, const unsigned char* ok, int n, int want, int max_runs, int32_t* out_runs,
                                       int32_t* out_left, int cap, int* n_left, long long* count) {
    lcd::KeyIntervals s;
    s.free_verdicts(keys, ok, (size_t)n);
    std::vector<int32_t> start((size_t)std::max(max_runs, 1)), len(start.size());
    const int r = s.take_runs(want, max_runs, start.data(), len.data());
    for (int i = 0; i < r; ++i) { out_runs[2 * i] = start[i]; out_runs[2 * i + 1] = len[i]; }
    *n_left = key_intervals_out(s, out_left, cap, count);
    return r;
}
