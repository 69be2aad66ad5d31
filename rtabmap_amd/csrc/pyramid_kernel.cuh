// pyramid_kernel.cuh -- the image pyramid of the optical-flow calls (keypoints_3d_stereo.hip, flow_track.hip): the table of images with their
// levels, the kernel that builds one level of every image of a batch, and the placement of the levels 1.. in a scratch buffer.  The
// arithmetic is stereo_flow_rule.h's (pyr_row, pyr_col).  Device code and the host code of the two entries.  Internal.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "stereo_flow_rule.h"

namespace lcd {
namespace pyramid {

constexpr int BLOCK = 256;
constexpr int TILE_W = 32, TILE_H = 8;       // a pyramid workgroup's tile of the new level
constexpr int SRC_W = 2 * TILE_W + 3, SRC_H = 2 * TILE_H + 3;

// one image of the batch: level 0 is the caller's, the levels 1 .. n_levels - 1 are built
struct Image {
    stereo::Level level[stereo::MAX_LEVELS];
    int32_t n_levels, pad;
};
static_assert(sizeof(stereo::Level) == 24 && sizeof(Image) % 8 == 0, "the image table lies behind the jobs, back to back");

// a staged piece of a level: pixel (x, y) of the level lies at p[(y - y0) * stride + (x - x0)], the border already reflected
struct PatchPx {
    const unsigned char* p;
    int x0, y0, stride;
    __device__ __forceinline__ int operator()(int x, int y) const { return p[(y - y0) * stride + (x - x0)]; }
};

// Level `level` of every image that has one.  blockIdx.x: image * max_tiles + tile.  A workgroup takes a 32 x 8 tile of the new level of one
// image: the source rows with their two-pixel halo go to LDS, the horizontal pass goes once into LDS, then the vertical pass.
static __global__ __launch_bounds__(BLOCK) void stereo_pyramid_kernel(const Image* images, int level, unsigned max_tiles) {
    __shared__ unsigned char src[SRC_H * SRC_W];
    __shared__ unsigned short hor[SRC_H * TILE_W];
    const unsigned image = blockIdx.x / max_tiles;
    const int tile = (int)(blockIdx.x - image * max_tiles);
    const Image& P = images[image];
    if (level >= P.n_levels) return;
    const stereo::Level S = P.level[level - 1];
    const stereo::Level D = P.level[level];
    const int tiles_x = (D.w + TILE_W - 1) / TILE_W, tiles_y = (D.h + TILE_H - 1) / TILE_H;
    if (tile >= tiles_x * tiles_y) return;
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int ox = tx * TILE_W, oy = ty * TILE_H, sx0 = 2 * ox - 2, sy0 = 2 * oy - 2;
    const int tid = threadIdx.x;
    const int cols = min(TILE_W, D.w - ox), rows = min(TILE_H, D.h - oy);      // what of the tile exists
    const int src_cols = 2 * cols + 3, src_rows = 2 * rows + 3;
    const stereo::GlobalPx px{S};
    for (int e = tid; e < src_rows * src_cols; e += BLOCK) {
        const int r = e / src_cols, c = e - r * src_cols;
        src[r * SRC_W + c] = (unsigned char)px(sx0 + c, sy0 + r);
    }
    __syncthreads();
    const PatchPx sp{src, sx0, sy0, SRC_W};
    for (int e = tid; e < src_rows * cols; e += BLOCK) {
        const int r = e / cols, c = e - r * cols;
        hor[r * TILE_W + c] = (unsigned short)stereo::pyr_row(sp, ox + c, sy0 + r);
    }
    __syncthreads();
    const int r = tid / TILE_W, c = tid - r * TILE_W;
    if (r < rows && c < cols) {
        const unsigned short* h0 = hor + (2 * r) * TILE_W + c;
        const int v = stereo::pyr_col(h0[0], h0[TILE_W], h0[2 * TILE_W], h0[3 * TILE_W], h0[4 * TILE_W]);
        const_cast<unsigned char*>(D.data)[(int64_t)(oy + r) * D.pitch + ox + c] = (unsigned char)v;
    }
}

// The levels 1 .. n_levels - 1 of an image whose level 0 and n_levels are set: their sizes, rows at a pitch of 16 bytes, and as `data` their
// OFFSET in a scratch buffer from *at on (*at moves behind them); *max_tiles grows to the most tiles a level has.  rebase() turns the
// offsets into addresses once the buffer is known.
inline void place_levels(Image& Q, size_t* at, unsigned* max_tiles) {
    for (int l = 1; l < Q.n_levels; ++l) {
        const int w = (Q.level[l - 1].w + 1) / 2, ht = (Q.level[l - 1].h + 1) / 2, pitch = (w + 15) & ~15;
        Q.level[l] = stereo::Level{reinterpret_cast<const unsigned char*>(*at), pitch, w, ht, 0};
        *at += (size_t)pitch * (size_t)ht;
        const unsigned tiles = (unsigned)(((w + TILE_W - 1) / TILE_W) * ((ht + TILE_H - 1) / TILE_H));
        if (tiles > *max_tiles) *max_tiles = tiles;
    }
}
inline void rebase(Image& Q, const unsigned char* base) {
    for (int l = 1; l < Q.n_levels; ++l) Q.level[l].data = base + reinterpret_cast<size_t>(Q.level[l].data);
}

}  // namespace pyramid
}  // namespace lcd
