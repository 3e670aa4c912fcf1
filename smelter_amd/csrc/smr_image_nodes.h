// smr_image_nodes.h — k_image_nodes: up to 16 Image nodes drawn into their own resolution by ONE launch.  The image pass of the renderer
// (host/renderer.cpp, before an output's graph walk): every Image node whose size differs from its asset's — each frame for an animated
// asset, once for a static one — used to cost one k_rescale_bilinear launch; an overlay of a dozen stickers is a dozen small launches per
// frame, and host enqueue is half of the frame period (profiles/r06_host_rate.txt).  The argument that produced k_move_rects.
//
//   * Jobs by value in the kernel arguments, one 64 x 16 tile of one job's DESTINATION per workgroup, four texels of a row per lane, 16-byte
//     stores where the destination allows, nothing written outside [0, dw) x [0, dh): the geometry of smr_node_tiles.h.
//   * Each texel is sample_rgba_bilinear at ((x + .5) / dw, (y + .5) / dh), encoded as store_texel encodes (encode_rgba8, smr_shader_dev.h):
//     k_rescale_bilinear's operations in its order (rgba_rescale.wgsl:24-27), so the bytes are k_rescale_bilinear's in both rendering modes.
//   * No LDS, no barrier: threads do not talk to each other.
// The source compiles under SMR_EMU (tests/emu/emu_image_nodes.cpp): the CPU tests run it on guard-paged buffers.
#pragma once

#include "smr_node_tiles.h"

// (this kernel's former names for the shared geometry: emulator drivers written against them still compile; the values are smr_node_tiles.h's)
#define SMR_IMAGE_MAX_JOBS SMR_NODE_MAX_JOBS
#define SMR_IMAGE_BLOCK SMR_NODE_BLOCK
#define SMR_IMAGE_TILE_W SMR_NODE_TILE_W
#define SMR_IMAGE_TILE_H SMR_NODE_TILE_H

struct ImageJob {
    SurfView src, dst;  // premultiplied RGBA8, both
    int pxi;            // PXI_RGBA8_SRGB / PXI_RGBA8_UNORM: how texels are decoded and encoded
    u32 wide;           // nt_wide(dst) (in_plan)
};

struct ImageBatch {
    ImageJob j[SMR_NODE_MAX_JOBS];
    u32 first_tile[SMR_NODE_MAX_JOBS + 1];  // first_tile[i] .. first_tile[i + 1]: the workgroups of job i
    u32 n;
};

// Fills everything of B but j[].src / dst / pxi and n; returns the number of workgroups (0: nothing to draw).  Host code, shared with the
// emulator.  A job without a source or a destination texel has no tile.
static inline u32 in_plan(ImageBatch &B) {
    return nt_plan(B, [](const ImageJob &J) { return J.src.ptr && J.src.w > 0 && J.src.h > 0 ? &J.dst : nullptr; });
}

#ifdef __HIPCC__

// What thread `tid` of workgroup `block` does.  Every branch on B's fields is uniform per workgroup.
__device__ __forceinline__ void in_workgroup(const ImageBatch &B, u32 block, u32 tid, const float *__restrict__ tables) {
    if (block >= B.first_tile[SMR_NODE_MAX_JOBS]) return;
    const u32 i = nt_job_of(B.first_tile, block);
    const SurfView src = B.j[i].src, dst = B.j[i].dst;
    const int pxi = B.j[i].pxi;
    const u32 wide = B.j[i].wide;
    const NodeTile T = nt_tile_of(B.first_tile, i, block, dst.w);
    const int x0 = (int)nt_lane_x(T.x * SMR_NODE_TILE_W, tid);
    const int y = (int)nt_lane_y(T.y * SMR_NODE_TILE_H, tid);
    if (x0 >= dst.w || y >= dst.h) return;
    const float *dec = tables, *thr = tables + 256;
    const int n = dst.w - x0;  // the texels the row has from x0 on: the group is min(n, 4) of them
    const float v = ((float)y + 0.5f) / (float)dst.h;
    u32 px[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (k < n) px[k] = encode_rgba8(pxi, sample_rgba_bilinear(src, pxi, ((float)(x0 + k) + 0.5f) / (float)dst.w, v, dec), thr);
    }
    nt_store_group(dst.ptr + (size_t)y * dst.pitch + (size_t)x0 * 4, wide, n, px);
}

#ifndef SMR_EMU
__global__ void __launch_bounds__(SMR_NODE_BLOCK) k_image_nodes(const ImageBatch B, const float *__restrict__ tables) {
    in_workgroup(B, blockIdx.x, threadIdx.x, tables);
}
#endif

#endif  // __HIPCC__
