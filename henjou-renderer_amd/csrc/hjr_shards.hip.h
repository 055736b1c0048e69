// Gathered shards of a multi-GPU frame -> row-major frames (hjr_assemble_shards_device, hjr_denoise_shards_device).
// Included by hjr_post.hip only (a non-template __global__ function: one translation unit).
#pragma once
#include <hip/hip_runtime.h>
#include "hjr_layout.h"

// ---- gathered shards -> frames (hjr_assemble_shards_device; DESIGN.md §7 "Denoise modes").  After the one gather of a multi-GPU frame rank 0
// holds `world` blocks, rank r's at byte offset r * rank_stride from each base pointer: up to three float4 AOVs and the one-float variance AOV,
// each [owned tile][64].  One launch scatters all of them: the inverse of hjr_slot_xy for every rank at once.  One lane per frame pixel, a wave
// per 8 x 8 tile (lane = slot within the tile), so a wave reads 1 KiB (256 B of variance) contiguous and writes 8 rows of 128 B (32 B).  The
// owner and the slot are arithmetic on the tile id (csrc/hjr_layout.h): tile t is rank t % world's (t / world)-th tile.  Lanes of an edge tile
// outside the image have no pixel and read nothing; padding behind a rank's last tile is never addressed (t < n_tiles).  Null = absent AOV.
struct ShardArgs {
    const char *color, *albedo, *normal, *variance; // rank 0's blocks
    float4 *out_color, *out_albedo, *out_normal;    // row-major frames
    float* out_variance;
    unsigned long long rank_stride;                 // bytes between the blocks of consecutive ranks
    uint32_t width, height, tiles_x, world;
};
__global__ void __launch_bounds__(256) hjr_assemble_shards_kernel(const ShardArgs a)
{
    const uint32_t lane = threadIdx.x & 63u, tx = blockIdx.x * 4u + (threadIdx.x >> 6), ty = blockIdx.y;
    const uint32_t x = tx * HJR_TILE + (lane & 7u), y = ty * HJR_TILE + (lane >> 3);
    if (x >= a.width || y >= a.height) return; // (also the tiles of the last workgroup of a row behind tiles_x)
    const uint32_t t = hjr_tile_id(tx, ty, a.tiles_x);
    const size_t off = (size_t)(t % a.world) * a.rank_stride, slot = (size_t)(t / a.world) * 64u + lane, pix = (size_t)y * a.width + x;
    if (a.color) a.out_color[pix] = reinterpret_cast<const float4*>(a.color + off)[slot];
    if (a.albedo) a.out_albedo[pix] = reinterpret_cast<const float4*>(a.albedo + off)[slot];
    if (a.normal) a.out_normal[pix] = reinterpret_cast<const float4*>(a.normal + off)[slot];
    if (a.variance) a.out_variance[pix] = reinterpret_cast<const float*>(a.variance + off)[slot];
}
