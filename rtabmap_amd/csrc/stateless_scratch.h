// stateless_scratch.h -- the scratch of the calls that neither read nor write engine state, and the rules for using it.  Internal.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cassert>
#include <cstring>

#include "devbuf.h"
#include "stage_rows.h"

// Scratch of the calls that do not complete what a pipelined handle owes, with their _dev forms:
//   lcd_match_pairs (pair_match.hip), lcd_match_guided (guided_match.hip),
//   lcd_select_features and lcd_expand_word_ids (feature_select.hip), lcd_keypoints_3d (keypoints_3d.hip),
//   lcd_estimate_motion_3d (motion_3d.hip), lcd_estimate_motion_pnp (motion_pnp.hip) and lcd_register_icp (register_icp.hip).
// Everything they write on the device lives here and nowhere else, so they can be enqueued between the stages of frames in flight.  The
// buffers only grow, and a growth frees the old allocation after the engine stream has drained (DevBuf::reserve): work of an earlier call
// that is still enqueued keeps what it reads.  The protocol is the methods' and HostStage's; the callers own only d_dist and d_small.
struct StatelessScratch {
    lcd::DevBuf d_dist;                                 // the distance blocks of one group of pairs (to x from; from x from and to x to when new words are compared)
    // d_small, by caller:
    //   the matching calls: per pair the to-rows' 2-NN among the from-words, word ranks, candidate bit rows / the cross-check keys
    //   lcd_estimate_motion_3d: 36 bytes per from-row (six coordinate planes, d2, two index sets)
    //   lcd_estimate_motion_pnp: 44 bytes per to-row (eight coordinate planes, errors, two index sets)
    //   lcd_register_icp: 20 bytes per row of either side (three coordinate planes, the nearest row, its d2)
    lcd::DevBuf d_small;
    int64_t budget_bytes = 0;                           // lcd_set_option("pair_match_budget"): distance-block bytes per group (0: built-in, 256 MiB)

    // A call's job table (one or two host arrays, back to back) reaches d_table through one of two pinned slots, taken in turn by every
    // call of every family.  The invariant: a slot is written again only after the copy that last read it has run (its event, recorded
    // behind that copy) -- whichever call enqueued it.  d_table itself is ordered by the stream.  *d_table_out: where the table is.
    template <typename Job>
    hipError_t upload_table(const Job** d_table_out, hipStream_t st, int64_t* bytes_device, const void* a, size_t a_bytes, const void* b = nullptr, size_t b_bytes = 0) {
        TF_TRY(d_table.reserve(a_bytes + b_bytes + 64, 0, st, bytes_device));
        const int slot = next_slot; next_slot ^= 1;
        if (!table_read[slot]) TF_TRY(hipEventCreateWithFlags(&table_read[slot], hipEventDisableTiming));
        else TF_TRY(hipEventSynchronize(table_read[slot]));
        TF_TRY(h_table[slot].reserve(a_bytes + b_bytes + 64));
        std::memcpy(h_table[slot].p, a, a_bytes);
        if (b_bytes) std::memcpy(h_table[slot].as<char>() + a_bytes, b, b_bytes);
        TF_TRY(hipMemcpyAsync(d_table.p, h_table[slot].p, a_bytes + b_bytes, hipMemcpyHostToDevice, st));
        TF_TRY(hipEventRecord(table_read[slot], st));
        *d_table_out = d_table.as<Job>();
        return hipSuccess;
    }

    // one all-ones candidate bit row of `bytes` bytes (a search without index: every earlier new word is a candidate), filled at its first use
    hipError_t ones_row(const uint32_t** row, size_t bytes, hipStream_t st, int64_t* bytes_device) {
        if (bytes > ones_bytes) {
            TF_TRY(d_ones.reserve(bytes, 0, st, bytes_device));
            TF_TRY(hipMemsetAsync(d_ones.p, 0xFF, bytes, st));
            ones_bytes = bytes;
        }
        *row = d_ones.as<uint32_t>();
        return hipSuccess;
    }

    void release(int64_t* bytes_device) {
        lcd::DevBuf* all[] = {&d_dist, &d_small, &d_table, &d_ones, &d_in, &d_out};
        for (lcd::DevBuf* d : all) d->release(bytes_device);
        h_in.release(); h_out.release();
        for (int i = 0; i < 2; ++i) { h_table[i].release(); if (table_read[i]) (void)hipEventDestroy(table_read[i]); table_read[i] = nullptr; }
        ones_bytes = 0;
    }

private:
    friend struct HostStage;
    lcd::DevBuf d_table;                                // the jobs of the launches enqueued last
    lcd::PinBuf h_table[2];
    hipEvent_t table_read[2] = {nullptr, nullptr};      // recorded behind the copy out of the slot
    int next_slot = 0;
    lcd::DevBuf d_ones;
    size_t ones_bytes = 0;
    lcd::DevBuf d_in, d_out;                            // host entries: the inputs as staged on the device / the results before they go back
    lcd::PinBuf h_in, h_out;
};

// What a host entry does around its launches, for the one call it lives in: the caller names its input and output regions in order,
// commit() lays them out (lcd::RegionLayout), stages the inputs in pinned memory and enqueues ONE copy to the device, the launches work on
// in<T>() / out<T>(), finish() enqueues ONE copy back, synchronises ONCE and hands the results out.  The host entries serialise on that
// synchronisation, which is what lets every one of them use the same four buffers.
struct HostStage {
    HostStage(StatelessScratch& scratch, size_t host_row_bytes, size_t row_bytes) : S(scratch), host_row(host_row_bytes), dev_row(row_bytes) {}
    int add_in(const void* src, size_t bytes) { const int r = li.add(bytes); assert(r >= 0); from[r] = src; rows[r] = -1; return r; }
    // `n` host rows of the handle (host_row_bytes each), staged at the stride the kernels walk
    int add_in_rows(const void* src, int64_t n) { const int r = add_in(src, (size_t)n * dev_row); rows[r] = n; return r; }
    // dst == nullptr: finish() leaves the region where host_out() finds it
    int add_out(void* dst, size_t bytes) { const int r = lo.add(bytes); assert(r >= 0); to[r] = dst; return r; }

    hipError_t commit(hipStream_t st, int64_t* bytes_device) {
        TF_TRY(S.h_in.reserve(li.bytes + 256));
        TF_TRY(S.h_out.reserve(lo.bytes + 256));
        TF_TRY(S.d_in.reserve(li.bytes + 256, 0, st, bytes_device));
        TF_TRY(S.d_out.reserve(lo.bytes + 256, 0, st, bytes_device));
        for (int r = 0; r < li.n; ++r) {
            if (!li.len[r]) continue;
            if (rows[r] >= 0) lcd::pack_rows(S.h_in.as<char>() + li.off[r], from[r], rows[r], host_row, dev_row);
            else std::memcpy(S.h_in.as<char>() + li.off[r], from[r], li.len[r]);
        }
        if (li.bytes) TF_TRY(hipMemcpyAsync(S.d_in.p, S.h_in.p, li.bytes, hipMemcpyHostToDevice, st));
        return hipSuccess;
    }
    template <typename T> const T* in(int r) const { return (const T*)(S.d_in.as<char>() + li.off[r]); }
    template <typename T> T* out(int r) const { return (T*)(S.d_out.as<char>() + lo.off[r]); }

    hipError_t finish(hipStream_t st) {
        TF_TRY(hipMemcpyAsync(S.h_out.p, S.d_out.p, lo.bytes, hipMemcpyDeviceToHost, st));
        TF_TRY(hipStreamSynchronize(st));
        for (int r = 0; r < lo.n; ++r) if (to[r] && lo.len[r]) std::memcpy(to[r], host_out(r), lo.len[r]);
        return hipSuccess;
    }
    const char* host_out(int r) const { return S.h_out.as<char>() + lo.off[r]; }

private:
    StatelessScratch& S;
    size_t host_row, dev_row;
    lcd::RegionLayout li, lo;
    const void* from[lcd::RegionLayout::MAX_REGIONS];
    int64_t rows[lcd::RegionLayout::MAX_REGIONS];       // >= 0: the region is that many handle rows, to be padded
    void* to[lcd::RegionLayout::MAX_REGIONS];
};
