// smr_svg_nodes.h — k_svg_nodes: the colour fix-up of up to 16 freshly rasterised SVG pixmaps, in place, by ONE launch.  The host half
// (host/renderer.cpp, smr_renderer_update_scene) has the caller's rasteriser fill a pixmap per (SVG asset, node size) the new scene needs,
// uploads them into RGBA8 surfaces of the nodes' sizes and calls smr_svg_nodes once: what SvgAsset::render_to_texture does after tiny-skia
// is done (transformations/image/svg_image.rs:120-167) — the premultiplied, gamma-encoded pixmap is un-premultiplied through the linear view,
// quantised to 8 bits, and premultiplied through the sRGB view — where the two existing passes would be two launches per raster.
//
//   * Jobs by value in the kernel arguments, one 64 x 16 tile of one job's surface per workgroup, four texels of a row per lane, 16-byte
//     accesses where the surface allows: the geometry of smr_node_tiles.h.  A lane reads its group, fixes it and writes it back where it
//     was, access by access (sv_workgroup says why not through the group helpers).
//   * Per texel, exactly the two passes with the 8-bit word between them: k_premult mode 1's operations in its order
//     (remove_premultiplied_alpha.wgsl:24-35), then k_premult mode 0 with PXI_RGBA8_SRGB on that word (add_premultiplied_alpha.wgsl:24-35).
//     No special case for alpha 0 or 255: the function maps (c, alpha) to a byte, and the tests enumerate its 65 536 cases.
//   * Nothing outside [0, w) x [0, h) of a surface is read or written: not its row padding, not a byte behind its last row.
//   * No LDS, no barrier: the work is in place, one texel per owner.
// The source compiles under SMR_EMU (tests/emu/emu_svg_nodes.cpp): the CPU tests run it on guard-paged buffers.
#pragma once

#include "smr_node_tiles.h"

// (this kernel's former names for the shared geometry: emulator drivers written against them still compile; the values are smr_node_tiles.h's)
#define SMR_SVG_MAX_JOBS SMR_NODE_MAX_JOBS
#define SMR_SVG_BLOCK SMR_NODE_BLOCK
#define SMR_SVG_TILE_W SMR_NODE_TILE_W
#define SMR_SVG_TILE_H SMR_NODE_TILE_H

struct SvgJob {
    SurfView px;  // the pixmap as uploaded: premultiplied, gamma-encoded RGBA8; the node's bytes afterwards
    u32 wide;     // nt_wide(px) (sv_plan)
};

struct SvgBatch {
    SvgJob j[SMR_NODE_MAX_JOBS];
    u32 first_tile[SMR_NODE_MAX_JOBS + 1];  // first_tile[i] .. first_tile[i + 1]: the workgroups of job i
    u32 n;
};

// Fills everything of B but j[].px and n; returns the number of workgroups (0: nothing to fix).  Host code, shared with the emulator.
// A job without a texel has no tile.
static inline u32 sv_plan(SvgBatch &B) {
    return nt_plan(B, [](const SvgJob &J) { return &J.px; });
}

#ifdef __HIPCC__

// One texel through both passes (k_premult, smr_convert.hip, operation for operation).
__device__ __forceinline__ u32 sv_fix_texel(u32 p, const float *__restrict__ dec, const float *__restrict__ thr) {
    // remove_premultiplied_alpha (mode 1): unorm in, unorm out
    const float a = (float)(p >> 24) / 255.0f;
    const float am = a > 0.00001f ? a : 0.00001f;
    const u32 s0 = unorm8(((float)(p & 0xff) / 255.0f) / am);
    const u32 s1 = unorm8(((float)((p >> 8) & 0xff) / 255.0f) / am);
    const u32 s2 = unorm8(((float)((p >> 16) & 0xff) / 255.0f) / am);
    const u32 sa = unorm8(a);
    // add_premultiplied_alpha (mode 0, PXI_RGBA8_SRGB) on the word s0 | s1 << 8 | s2 << 16 | sa << 24
    const float a2 = (float)sa / 255.0f;
    const float am2 = a2 > 0.00001f ? a2 : 0.00001f;
    const u32 r = srgb_encode8(clampf(dec[s0] * am2, 0.0f, 1.0f), thr);
    const u32 g = srgb_encode8(clampf(dec[s1] * am2, 0.0f, 1.0f), thr);
    const u32 b = srgb_encode8(clampf(dec[s2] * am2, 0.0f, 1.0f), thr);
    return r | (g << 8) | (b << 16) | (unorm8(a2) << 24);
}

// What thread `tid` of workgroup `block` does.  Every branch on B's fields is uniform per workgroup.
__device__ __forceinline__ void sv_workgroup(const SvgBatch &B, u32 block, u32 tid, const float *__restrict__ tables) {
    if (block >= B.first_tile[SMR_NODE_MAX_JOBS]) return;
    const u32 i = nt_job_of(B.first_tile, block);
    const SurfView px = B.j[i].px;
    const u32 wide = B.j[i].wide;
    const NodeTile T = nt_tile_of(B.first_tile, i, block, px.w);
    const int x0 = (int)nt_lane_x(T.x * SMR_NODE_TILE_W, tid);
    const int y = (int)nt_lane_y(T.y * SMR_NODE_TILE_H, tid);
    if (x0 >= px.w || y >= px.h) return;
    const float *dec = tables, *thr = tables + 256;
    const int n = px.w - x0;  // the texels the row has from x0 on: the group is min(n, 4) of them
    u8 *p = px.ptr + (size_t)y * px.pitch + (size_t)x0 * 4;
    // (nt_load_group / nt_store_group with the texels fixed in between is other machine code — half the registers —, and this kernel's is
    // held to what it was: the group is read, fixed and written back access by access here)
    if (wide && n >= 4) {
        const uint4 v = g_ld_u32x4(p);
        g_st_u32x4(p, make_uint4(sv_fix_texel(v.x, dec, thr), sv_fix_texel(v.y, dec, thr), sv_fix_texel(v.z, dec, thr), sv_fix_texel(v.w, dec, thr)));
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (k < n) g_st_u32(p + 4 * k, sv_fix_texel(g_ld_u32(p + 4 * k), dec, thr));
    }
}

#ifndef SMR_EMU
__global__ void __launch_bounds__(SMR_NODE_BLOCK) k_svg_nodes(const SvgBatch B, const float *__restrict__ tables) {
    sv_workgroup(B, blockIdx.x, threadIdx.x, tables);
}
#endif

#endif  // __HIPCC__
