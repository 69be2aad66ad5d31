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
    static constexpr int MAX_REGIONS = 16;              // lcd_estimate_motion_pnp names nine outputs, lcd_register_icp ten, lcd_register_icp_plane fifteen
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

}  // namespace lcd
