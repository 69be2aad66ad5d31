// sanitize_stage_rows.cpp -- rtabmap_amd/csrc/stage_rows.h (plain host code: how host rows are padded to the stride the kernels walk and
// un-padded again, and how the regions of a staging buffer are laid out) driven from a stand-alone program, for a host-only
// AddressSanitizer / UndefinedBehaviorSanitizer run.  No engine is created and nothing touches a GPU.
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Irtabmap_amd/csrc tools/sanitize_stage_rows.cpp -o stage_rows_asan
//   ./stage_rows_asan
//
// Every buffer is a heap allocation of exactly the size the functions may touch, so one byte too many is caught; a buffer of zero rows is
// a null pointer.  Exit status 0 and "ok" when every byte is where it belongs.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "stage_rows.h"

static unsigned char* exact(size_t bytes, int fill) {
    if (!bytes) return nullptr;
    unsigned char* p = (unsigned char*)std::malloc(bytes);
    if (!p) std::abort();
    std::memset(p, fill, bytes);
    return p;
}

// n rows of src_row bytes: packed to row_bytes, checked byte by byte, unpacked again
static bool round_trip(size_t src_row, size_t row_bytes, int n) {
    unsigned char* host = exact((size_t)n * src_row, 0);
    for (size_t i = 0; i < (size_t)n * src_row; ++i) host[i] = (unsigned char)(1 + i % 251);      // never 0: padding is told from data
    unsigned char* staged = exact((size_t)n * row_bytes, 0xAA);
    lcd::pack_rows(staged, host, n, src_row, row_bytes);
    bool ok = true;
    for (int r = 0; r < n; ++r)
        for (size_t c = 0; c < row_bytes; ++c)
            ok = ok && staged[(size_t)r * row_bytes + c] == (c < src_row ? host[(size_t)r * src_row + c] : 0);
    unsigned char* back = exact((size_t)n * src_row, 0x55);
    lcd::unpack_rows(back, staged, n, src_row, row_bytes);
    ok = ok && (n == 0 || std::memcmp(back, host, (size_t)n * src_row) == 0);
    std::free(host); std::free(staged); std::free(back);
    if (!ok) std::fprintf(stderr, "pack_rows / unpack_rows: mismatch at %zu -> %zu bytes, %d rows\n", src_row, row_bytes, n);
    return ok;
}

static bool layout() {
    const size_t sizes[] = {0, 1, 255, 256, 257, 0, 4096, 3};
    for (int first = 0; first < 3; ++first) {
        lcd::RegionLayout L;
        size_t end = 0;                                                     // one past the last byte of the regions so far
        for (int i = 0; i < lcd::RegionLayout::MAX_REGIONS; ++i) {
            const size_t b = sizes[first + i];
            const int r = L.add(b);
            if (r != i || L.n != i + 1 || L.len[r] != b) return false;
            if (L.off[r] % 256 || L.off[r] < end || (i > 0 && L.off[r] < L.off[r - 1])) return false;     // aligned, behind its predecessors, ascending
            if (L.off[r] != (i ? L.off[r - 1] + lcd::up256(L.len[r - 1]) : 0)) return false;                // the running sum, nothing else
            end = L.off[r] + b;
            if (L.bytes % 256 || L.bytes < end || L.bytes - end >= 256) return false;                       // one copy covers all of them
        }
        if (L.add(8) != -1 || L.n != lcd::RegionLayout::MAX_REGIONS) return false;                          // full: refused, nothing written
    }
    lcd::RegionLayout none;
    return none.n == 0 && none.bytes == 0 && lcd::up256(0) == 0 && lcd::up256(1) == 256 && lcd::up256(256) == 256 && lcd::up256(257) == 512;
}

int main() {
    const size_t u8[][2] = {{32, 32}, {61, 64}, {5, 8}, {1, 4}};            // (dim, row_bytes) of u8 handles
    const size_t f32[] = {64, 128};                                         // floats per row: stored as they come
    const int rows[] = {0, 1, 7};
    int cases = 0;
    for (int n : rows) {
        for (const auto& s : u8) { if (!round_trip(s[0], s[1], n)) return 1; ++cases; }
        for (size_t d : f32) { if (!round_trip(d * 4, d * 4, n)) return 1; ++cases; }
    }
    if (!layout()) { std::fprintf(stderr, "RegionLayout: mismatch\n"); return 1; }
    std::printf("ok: %d row cases, the region layout\n", cases);
    return 0;
}
