// sanitize_stage_rows.cpp -- rtabmap_amd/csrc/stage_rows.h (plain host code: how host rows are padded to the stride the kernels walk and
// un-padded again, how the regions of a staging buffer are laid out, how the pointer fields of a call's kernel arguments are bound to those
// regions and patched, and how per-frame results are handed out) driven from a stand-alone program, for a host-only
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

static const size_t sizes[] = {0, 1, 255, 256, 257, 0, 4096, 3};
static constexpr int N_SIZES = (int)(sizeof sizes / sizeof sizes[0]);

static bool layout() {
    for (int first = 0; first < 3; ++first) {
        lcd::RegionLayout L;
        size_t end = 0;                                                     // one past the last byte of the regions so far
        for (int i = 0; i < lcd::RegionLayout::MAX_REGIONS; ++i) {
            const size_t b = sizes[(first + i) % N_SIZES];
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

// kernel arguments as the entries have them: pointer fields of different types, some of them null
struct float2 { float x, y; };
struct Args {
    const float* xyz; const float2* points; const void* rows; const int32_t* ids; const float* no_response;
    int32_t* count; double* variance; float2* out_points; void* out_rows; float* no_dist;
};

// the fields bound with sizes[first..], patched against a buffer of exactly the layout's bytes: who lands where, who stays as it was
static bool bindings(int first, bool on_device) {
    unsigned char* host[8];
    for (unsigned char*& p : host) p = exact(1, 0);                         // eight distinct caller's pointers
    Args g = {(const float*)host[0], (const float2*)host[1], host[2], (const int32_t*)host[3], nullptr,
              (int32_t*)host[4], (double*)host[5], (float2*)host[6], host[7], nullptr};
    const Args before = g;
    lcd::BoundRegions B;
    B.on_device = on_device;
    int k = first, r[10];
    auto size = [&] { return sizes[k++ % N_SIZES]; };
    r[0] = B.bind(g.xyz, size()); r[1] = B.bind(g.points, size()); r[2] = B.bind(g.rows, size()); r[3] = B.bind(g.ids, size());
    r[4] = B.bind(g.no_response, size());
    r[5] = B.bind(g.count, size()); r[6] = B.bind(g.variance, size()); r[7] = B.bind(g.out_points, size()); r[8] = B.bind(g.out_rows, size());
    r[9] = B.bind(g.no_dist, size());
    bool ok = std::memcmp(&g, &before, sizeof g) == 0;                      // binding changes no field
    unsigned char* base = exact(B.lay.bytes, 0xAA);
    B.patch(base);
    const void* now[10] = {g.xyz, g.points, g.rows, g.ids, g.no_response, g.count, g.variance, g.out_points, g.out_rows, g.no_dist};
    if (on_device) ok = ok && B.lay.n == 0 && B.lay.bytes == 0 && std::memcmp(&g, &before, sizeof g) == 0;      // every field as it was
    else {
        ok = ok && B.lay.n == 8 && r[4] == lcd::BoundRegions::NONE && r[9] == lcd::BoundRegions::NONE && !g.no_response && !g.no_dist;
        int n = 0;
        for (int f = 0; f < 10 && ok; ++f) {
            if (f == 4 || f == 9) continue;
            const size_t off = B.lay.off[n], len = B.lay.len[n];
            ok = r[f] == n && now[f] == base + off && off % 256 == 0 && (n == 0 || off >= B.lay.off[n - 1] + B.lay.len[n - 1]) && off + len <= B.lay.bytes;
            ok = ok && B.host[n] == host[n] && len == sizes[(first + f) % N_SIZES];
            if (len) std::memset((void*)now[f], n, len);                    // the region is the buffer's: one byte too many is caught
            ++n;
        }
    }
    for (int f = 0; f < 10; ++f) ok = ok && (r[f] >= 0 || r[f] == lcd::BoundRegions::NONE);
    for (unsigned char* p : host) std::free(p);
    std::free(base);
    return ok;
}

// the seventeenth field is refused as RegionLayout refuses a seventeenth region: nothing recorded, the field untouched
static bool full() {
    unsigned char* host = exact(1, 0);
    const float* many[lcd::RegionLayout::MAX_REGIONS + 1];
    lcd::BoundRegions B;
    for (int i = 0; i < lcd::RegionLayout::MAX_REGIONS; ++i) {
        many[i] = (const float*)host;
        if (B.bind(many[i], 4) != i) return false;
    }
    const float* last = (const float*)host;
    const bool ok = B.bind(last, 4) == lcd::BoundRegions::FULL && B.lay.n == lcd::RegionLayout::MAX_REGIONS && last == (const float*)host;
    std::free(host);
    return ok;
}

// hand_out_frames over four frames of 3, 0, 4 and 1 elements: dst is all canary before, and behind a frame's count it still is
static bool frames(size_t elem, size_t stride, const int32_t count[4]) {
    const int64_t offsets[5] = {0, 3, 3, 7, 8};
    const size_t N = 8;
    unsigned char* src = exact(N * stride, 0);
    for (size_t i = 0; i < N * stride; ++i) src[i] = (unsigned char)(1 + i % 196);      // never the canary
    unsigned char* dst = exact(N * elem, 0xC5);
    lcd::hand_out_frames(dst, src, count, offsets, 4, elem, stride);
    bool ok = true;
    for (int f = 0; f < 4; ++f)
        for (int64_t e = offsets[f]; e < offsets[f + 1]; ++e)
            for (size_t c = 0; c < elem; ++c)
                ok = ok && dst[(size_t)e * elem + c] == (e - offsets[f] < count[f] ? src[(size_t)e * stride + c] : 0xC5);
    std::free(src); std::free(dst);
    if (!ok) std::fprintf(stderr, "hand_out_frames: mismatch at %zu bytes, stride %zu\n", elem, stride);
    return ok;
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
    int bound = 0;
    for (int first = 0; first < N_SIZES; ++first)
        for (int dev = 0; dev < 2; ++dev, ++bound)
            if (!bindings(first, dev != 0)) { std::fprintf(stderr, "BoundRegions: mismatch at sizes[%d..], on_device %d\n", first, dev); return 1; }
    if (!full()) { std::fprintf(stderr, "BoundRegions: a seventeenth field\n"); return 1; }
    // per frame: full / empty / full / full, then counts of 1 and 0 beside an empty frame, then nothing at all
    const int32_t counts[][4] = {{3, 0, 4, 1}, {1, 0, 1, 0}, {0, 0, 4, 1}, {0, 0, 0, 0}};
    const size_t elems[][2] = {{61, 64}, {32, 32}, {5, 8}, {4, 4}, {12, 12}};      // (bytes handed out, stride): padded rows, unpadded rows, plain elements
    int handed = 0;
    for (const auto& c : counts)
        for (const auto& e : elems) { if (!frames(e[0], e[1], c)) return 1; ++handed; }
    std::printf("ok: %d row cases, the region layout, %d field bindings and the seventeenth, %d per-frame hand-outs\n", cases, bound, handed);
    return 0;
}
