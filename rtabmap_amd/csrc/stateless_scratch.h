// stateless_scratch.h -- the scratch of the calls that neither read nor write engine state, and the rules for using it.  Internal.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cassert>
#include <cstring>

#include "devbuf.h"
#include "stage_rows.h"

// Scratch of the stateless calls: those that do not complete what a pipelined handle owes, each with a host and a _dev form.  This is the
// one list of them; other files point here.
//   lcd_match_pairs (pair_match.hip), lcd_match_guided (guided_match.hip),
//   lcd_select_features and lcd_expand_word_ids (feature_select.hip), lcd_keypoints_3d (keypoints_3d.hip),
//   lcd_keypoints_3d_stereo (keypoints_3d_stereo.hip), lcd_track_flow (flow_track.hip),
//   lcd_estimate_motion_3d (motion_3d.hip), lcd_estimate_motion_pnp (motion_pnp.hip), lcd_refine_motion_ba (motion_ba.hip),
//   lcd_register_icp (register_icp.hip), lcd_register_icp_plane (register_icp_plane.hip) and lcd_filter_scans (scan_filter.hip).
// Everything they write on the device lives here and nowhere else, so they can be enqueued between the stages of frames in flight.  The
// buffers only grow, and a growth frees the old allocation after the engine stream has drained (DevBuf::reserve): work of an earlier call
// that is still enqueued keeps what it reads.  The protocol is the methods' and HostStage's; the callers own only d_dist and d_small.
struct StatelessScratch {
    lcd::DevBuf d_dist;                                 // the distance blocks of one group of pairs (to x from; from x from and to x to when new words are compared)
    // d_small, by caller:
    //   the matching calls: per pair the to-rows' 2-NN among the from-words, word ranks, candidate bit rows / the cross-check keys
    //   lcd_estimate_motion_3d: 36 bytes per from-row (six coordinate planes, d2, two index sets)
    //   lcd_estimate_motion_pnp: 44 bytes per to-row (eight coordinate planes, errors, two index sets)
    //   lcd_refine_motion_ba: 68 bytes per to-row (a point's state: initial, current and saved estimate, two observations, flags, to-depth)
    //   lcd_register_icp: 20 bytes per row of either side (three coordinate planes, the nearest row, its d2)
    //   lcd_register_icp_plane: 32 bytes per row of either side (lcd_register_icp's 20 and three normal planes)
    //   lcd_filter_scans: 16 bytes per scan (the counts and the status between its launches), then 36 bytes per sampled row (three
    //   coordinate planes behind step 1, three behind the voxel grid, three normal planes)
    //   lcd_keypoints_3d_stereo: 16 bytes per keypoint (the right corner, the status and the L1 error between the tracker and the
    //   projection), then the levels 1.. of every distinct image pair's two pyramids (rows at a pitch of 16 bytes)
    //   lcd_track_flow: 16 bytes per corner (the tracked corner, the status and the error between the tracker and the keep step), then
    //   the levels 1.. of every distinct image's pyramid (rows at a pitch of 16 bytes)
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

// What a host entry does around its launches, for the one call it lives in.  The entry fills its kernel arguments from the caller's pointers,
// as the _dev form needs them, and names each staged field ONCE: in() / in_rows() / out() / out_kept() bind the field to a region
// (lcd::BoundRegions).  commit() lays the regions out, stages the inputs in pinned memory, enqueues ONE copy to the device and points every
// bound field at its region of d_in / d_out; finish() enqueues ONE copy back, synchronises ONCE and copies every out() region to where its
// field pointed.  An out_kept() region stays in the pinned buffer for hand_out() / hand_out_rows().  A null field takes no region and stays
// null.  In the _dev form (on_device) every method does nothing and the fields keep the caller's pointers.  The host entries serialise on
// the one synchronisation, which is what lets every one of them use the same four buffers.
struct HostStage {
    HostStage(StatelessScratch& scratch, size_t host_row_bytes, size_t row_bytes, bool on_device) : S(scratch), host_row(host_row_bytes), dev_row(row_bytes), dev(on_device) {
        i.on_device = o.on_device = on_device;
    }
    // (a field need not be a kernel argument: a local pointer is bound the same way and holds its region's device address behind commit())
    template <typename T> void in(const T*& f, size_t bytes) { bound(i, f, bytes, rows, -1); }
    // `n` host rows of the handle (host_row_bytes each), staged at the stride the kernels walk
    template <typename T> void in_rows(const T*& f, int64_t n) { bound(i, f, (size_t)n * dev_row, rows, n); }
    template <typename T> void out(T*& f, size_t bytes) { bound(o, f, bytes, kept, 0); }
    // the region's index for hand_out() / hand_out_rows()
    template <typename T> int out_kept(T*& f, size_t bytes) { return bound(o, f, bytes, kept, 1); }

    hipError_t commit(hipStream_t st, int64_t* bytes_device) {
        if (dev) return hipSuccess;
        TF_TRY(S.h_in.reserve(i.lay.bytes + 256));
        TF_TRY(S.h_out.reserve(o.lay.bytes + 256));
        TF_TRY(S.d_in.reserve(i.lay.bytes + 256, 0, st, bytes_device));
        TF_TRY(S.d_out.reserve(o.lay.bytes + 256, 0, st, bytes_device));
        for (int r = 0; r < i.lay.n; ++r) {
            if (!i.lay.len[r]) continue;
            if (rows[r] >= 0) lcd::pack_rows(S.h_in.as<char>() + i.lay.off[r], i.host[r], rows[r], host_row, dev_row);
            else std::memcpy(S.h_in.as<char>() + i.lay.off[r], i.host[r], i.lay.len[r]);
        }
        if (i.lay.bytes) TF_TRY(hipMemcpyAsync(S.d_in.p, S.h_in.p, i.lay.bytes, hipMemcpyHostToDevice, st));
        i.patch(S.d_in.p); o.patch(S.d_out.p);
        return hipSuccess;
    }

    hipError_t finish(hipStream_t st) {
        if (dev) return hipSuccess;
        TF_TRY(hipMemcpyAsync(S.h_out.p, S.d_out.p, o.lay.bytes, hipMemcpyDeviceToHost, st));
        TF_TRY(hipStreamSynchronize(st));
        for (int r = 0; r < o.lay.n; ++r) if (!kept[r] && o.lay.len[r]) std::memcpy(o.host[r], S.h_out.as<char>() + o.lay.off[r], o.lay.len[r]);
        return hipSuccess;
    }
    // behind finish(), of the out_kept() region r: the first count[f] elements of `elem` bytes of every frame f, which begins at element
    // offsets[f], to where the field pointed (lcd::hand_out_frames).  r < 0 (a null field, the _dev form) or an empty region: nothing.
    void hand_out(int r, const int32_t* count, const int64_t* offsets, int n_frames, size_t elem) { hand_out(r, count, offsets, n_frames, elem, elem); }
    void hand_out_rows(int r, const int32_t* count, const int64_t* offsets, int n_frames) { hand_out(r, count, offsets, n_frames, host_row, dev_row); }   // handle rows, un-padded

private:
    template <typename P>
    int bound(lcd::BoundRegions& side, P*& f, size_t bytes, int64_t* tag, int64_t value) {
        const int r = side.bind(f, bytes);
        assert(r != lcd::BoundRegions::FULL);
        if (r >= 0) tag[r] = value;
        return r;
    }
    void hand_out(int r, const int32_t* count, const int64_t* offsets, int n_frames, size_t elem, size_t stride) {
        if (r >= 0 && o.lay.len[r]) lcd::hand_out_frames(o.host[r], S.h_out.as<char>() + o.lay.off[r], count, offsets, n_frames, elem, stride);
    }
    StatelessScratch& S;
    size_t host_row, dev_row;
    bool dev;
    lcd::BoundRegions i, o;
    int64_t rows[lcd::RegionLayout::MAX_REGIONS];       // inputs.  >= 0: the region is that many handle rows, to be padded
    int64_t kept[lcd::RegionLayout::MAX_REGIONS];       // outputs.  1: finish() leaves the region in the pinned buffer
};
