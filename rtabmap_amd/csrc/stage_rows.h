// stage_rows.h -- how host data is laid out on its way to the device and back (plain host code, no HIP: tools/sanitize_stage_rows.cpp
// drives it under the host sanitizers).  Internal.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <cstring>

namespace lcd {

inline size_t up256(size_t n) { return (n + 255) & ~(size_t)255; }

// `n` host rows of `src_row` bytes each -> rows at a stride of `row_bytes` (>= src_row), the bytes behind a row zeroed: u8 rows whose dim is
// no multiple of 4 are stored zero-padded
inline void pack_rows(void* dst, const void* src, int64_t n, size_t src_row, size_t row_bytes) {
    if (n <= 0) return;
    if (src_row == row_bytes) { std::memcpy(dst, src, (size_t)n * src_row); return; }
    std::memset(dst, 0, (size_t)n * row_bytes);
    for (int64_t i = 0; i < n; ++i) std::memcpy((char*)dst + (size_t)i * row_bytes, (const char*)src + (size_t)i * src_row, src_row);
}

// ... and back: rows at a stride of `row_bytes` -> `n` host rows of `dst_row` bytes
inline void unpack_rows(void* dst, const void* src, int64_t n, size_t dst_row, size_t row_bytes) {
    if (n <= 0) return;
    if (dst_row == row_bytes) { std::memcpy(dst, src, (size_t)n * dst_row); return; }
    for (int64_t i = 0; i < n; ++i) std::memcpy((char*)dst + (size_t)i * dst_row, (const char*)src + (size_t)i * row_bytes, dst_row);
}

// Regions of one staging buffer, in the order they are named: each starts at the 256-byte-aligned running sum of those before it (a region
// of zero bytes takes no room), `bytes` is what one copy of all of them moves.  A fixed array: no allocation per call.
struct RegionLayout {
    static constexpr int MAX_REGIONS = 16;              // the rule: at least the most inputs, and the most outputs, that one call names
    size_t off[MAX_REGIONS], len[MAX_REGIONS];
    int n = 0;
    size_t bytes = 0;
    int add(size_t region_bytes) {                      // returns the region's index, -1 when the array is full
        if (n == MAX_REGIONS) return -1;
        off[n] = bytes; len[n] = region_bytes;
        bytes += up256(region_bytes);
        return n++;
    }
};

// The staged arrays of one direction of a call, each bound to the pointer field of the kernel arguments that names it.  bind() takes the
// field holding the caller's pointer: that pointer is the copy's source or destination, the field's address is where patch() writes the
// region's address in the staging buffer.  The field may be of any object-pointer type; its bytes are copied, never read through another type.
struct BoundRegions {
    static constexpr int NONE = -1, FULL = -2;
    bool on_device = false;                             // the _dev form: the caller's pointers are the device's, nothing is bound or patched
    RegionLayout lay;
    void* field[RegionLayout::MAX_REGIONS];             // the bound field's address
    void* host[RegionLayout::MAX_REGIONS];              // what the field held when it was bound
    // the region's index; NONE for a null field, which takes no region and stays null; FULL when the array is full (nothing is recorded)
    template <typename P>
    int bind(P*& f, size_t region_bytes) {
        void* p;
        std::memcpy(&p, &f, sizeof p);
        if (!p || on_device) return NONE;
        const int r = lay.add(region_bytes);
        if (r < 0) return FULL;
        field[r] = &f; host[r] = p;
        return r;
    }
    void patch(void* base) const {                      // every bound field now points at its region of the buffer at `base`
        for (int r = 0; r < lay.n; ++r) {
            char* p = (char*)base + lay.off[r];
            std::memcpy(field[r], &p, sizeof p);
        }
    }
};

// Of a region of per-frame results (elements at a stride of `stride` bytes), the first count[f] elements of every frame f, which begins at
// element offsets[f], go to the same place in `dst` as elements of `elem` bytes (handle rows are un-padded: elem <= stride).  What lies
// behind a frame's count in `dst` stays as it was, and a count of zero copies nothing.
inline void hand_out_frames(void* dst, const void* src, const int32_t* count, const int64_t* offsets, int n_frames, size_t elem, size_t stride) {
    for (int f = 0; f < n_frames; ++f)
        unpack_rows((char*)dst + (size_t)offsets[f] * elem, (const char*)src + (size_t)offsets[f] * stride, count[f], elem, stride);
}

}  // namespace lcd
