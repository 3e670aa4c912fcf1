// smr_image_nodes.h — k_image_nodes: up to 16 Image nodes drawn into their own resolution by ONE launch.  The image pass of the renderer
// (host/renderer.cpp, before an output's graph walk): every Image node whose size differs from its asset's — each frame for an animated
// asset, once for a static one — used to cost one k_rescale_bilinear launch; an overlay of a dozen stickers is a dozen small launches per
// frame, and host enqueue is half of the frame period (profiles/r06_host_rate.txt).  The argument that produced k_move_rects.
//
//   * The jobs travel BY VALUE in the kernel arguments (ImageBatch): no table upload, no host synchronisation, nothing to keep alive.
//   * A workgroup takes one tile of 64 x 16 destination texels of one job; ImageBatch::first_tile (a prefix sum over the jobs' tile counts,
//     made by in_plan on the host) maps blockIdx.x to (job, tile).  Every branch on a job's fields is uniform per workgroup.
//   * Lane l of wave w owns the four consecutive texels x = 4 * (l & 15) .. + 3 of row 4 * w + (l >> 4) of the tile.  Each texel is
//     sample_rgba_bilinear at ((x + .5) / dw, (y + .5) / dh), encoded as store_texel encodes: k_rescale_bilinear's operations in its order
//     (rgba_rescale.wgsl:24-27), so the bytes are k_rescale_bilinear's in both rendering modes.
//   * The four results leave as one 16-byte global store when the group is whole and the destination's base and pitch are multiples of 16
//     (every surface smr_surface_create makes); a row's last, partial group and any other destination go texel by texel.
//   * Nothing outside [0, dw) x [0, dh) of a destination is written: not its row padding, not a byte behind its last row.
//   * No LDS, no barrier: threads do not talk to each other.
// The source compiles under SMR_EMU (tests/emu/emu_image_nodes.cpp): the CPU tests run it on guard-paged buffers.
#pragma once

#include "smr_internal.h"

#define SMR_IMAGE_MAX_JOBS 16
#define SMR_IMAGE_BLOCK 256
#define SMR_IMAGE_TILE_W 64
#define SMR_IMAGE_TILE_H 16

struct ImageJob {
    SurfView src, dst;  // premultiplied RGBA8, both
    int pxi;            // PXI_RGBA8_SRGB / PXI_RGBA8_UNORM: how texels are decoded and encoded
    u32 wide;           // 1: the destination's base and pitch are multiples of 16 — whole groups leave as one 16-byte store (in_plan)
};

struct ImageBatch {
    ImageJob j[SMR_IMAGE_MAX_JOBS];
    u32 first_tile[SMR_IMAGE_MAX_JOBS + 1];  // first_tile[i] .. first_tile[i + 1]: the workgroups of job i
    u32 n;
};

// Fills everything of B but j[].src / dst / pxi and n; returns the number of workgroups (0: nothing to draw).  Host code, shared with the
// emulator.  A job without a source or a destination texel has no tile.
static inline u32 in_plan(ImageBatch &B) {
    u32 total = 0;
    for (u32 i = 0; i < SMR_IMAGE_MAX_JOBS; i++) {
        B.first_tile[i] = total;
        if (i >= B.n) continue;
        ImageJob &J = B.j[i];
        J.wide = 0;
        if (!J.src.ptr || !J.dst.ptr || J.src.w <= 0 || J.src.h <= 0 || J.dst.w <= 0 || J.dst.h <= 0) continue;
        J.wide = (((uintptr_t)J.dst.ptr | J.dst.pitch) & 15u) == 0 ? 1u : 0u;
        const u32 tx = ((u32)J.dst.w + SMR_IMAGE_TILE_W - 1) / SMR_IMAGE_TILE_W, ty = ((u32)J.dst.h + SMR_IMAGE_TILE_H - 1) / SMR_IMAGE_TILE_H;
        total += tx * ty;
    }
    B.first_tile[SMR_IMAGE_MAX_JOBS] = total;
    return total;
}

#ifdef __HIPCC__

// store_texel's RGBA8 word (smr_shader_dev.h), operation for operation, without the store
__device__ __forceinline__ u32 in_encode_rgba8(int pxi, float4 v, const float *__restrict__ thr) {
    u32 r, g, b;
    if (pxi == PXI_RGBA8_SRGB) {
        r = srgb_encode8(v.x, thr); g = srgb_encode8(v.y, thr); b = srgb_encode8(v.z, thr);
    } else {
        r = unorm8(v.x); g = unorm8(v.y); b = unorm8(v.z);
    }
    const u32 a = unorm8(v.w);
    return r | (g << 8) | (b << 16) | (a << 24);
}

// What thread `tid` of workgroup `block` does.  Every branch on B's fields is uniform per workgroup.
__device__ __forceinline__ void in_workgroup(const ImageBatch &B, u32 block, u32 tid, const float *__restrict__ tables) {
    if (block >= B.first_tile[SMR_IMAGE_MAX_JOBS]) return;
    u32 i = 0;
#pragma unroll 1
    while (i + 1 < SMR_IMAGE_MAX_JOBS && block >= B.first_tile[i + 1]) i++;
    const SurfView src = B.j[i].src, dst = B.j[i].dst;
    const int pxi = B.j[i].pxi;
    const u32 wide = B.j[i].wide;
    const u32 tiles_x = ((u32)dst.w + SMR_IMAGE_TILE_W - 1) / SMR_IMAGE_TILE_W;
    const u32 t = block - B.first_tile[i];
    const u32 tile_y = t / tiles_x, tile_x = t - tile_y * tiles_x;
    const int x0 = (int)(tile_x * SMR_IMAGE_TILE_W + 4u * (tid & 15u));
    const int y = (int)(tile_y * SMR_IMAGE_TILE_H + 4u * (tid >> 6) + ((tid >> 4) & 3u));
    if (x0 >= dst.w || y >= dst.h) return;
    const float *dec = tables, *thr = tables + 256;
    const int n = dst.w - x0 < 4 ? dst.w - x0 : 4;
    const float v = ((float)y + 0.5f) / (float)dst.h;
    u32 px[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (k < n) px[k] = in_encode_rgba8(pxi, sample_rgba_bilinear(src, pxi, ((float)(x0 + k) + 0.5f) / (float)dst.w, v, dec), thr);
    }
    u8 *p = dst.ptr + (size_t)y * dst.pitch + (size_t)x0 * 4;
    if (wide && n == 4) {
        g_st_u32x4(p, make_uint4(px[0], px[1], px[2], px[3]));
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (k < n) g_st_u32(p + 4 * k, px[k]);
    }
}

#ifndef SMR_EMU
__global__ void __launch_bounds__(SMR_IMAGE_BLOCK) k_image_nodes(const ImageBatch B, const float *__restrict__ tables) {
    in_workgroup(B, blockIdx.x, threadIdx.x, tables);
}
#endif

#endif  // __HIPCC__
