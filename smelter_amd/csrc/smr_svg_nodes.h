// smr_svg_nodes.h — k_svg_nodes: the colour fix-up of up to 16 freshly rasterised SVG pixmaps, in place, by ONE launch.  The host half
// (host/renderer.cpp, smr_renderer_update_scene) has the caller's rasteriser fill a pixmap per (SVG asset, node size) the new scene needs,
// uploads them into RGBA8 surfaces of the nodes' sizes and calls smr_svg_nodes once: what SvgAsset::render_to_texture does after tiny-skia
// is done (transformations/image/svg_image.rs:120-167) — the premultiplied, gamma-encoded pixmap is un-premultiplied through the linear view,
// quantised to 8 bits, and premultiplied through the sRGB view — where the two existing passes would be two launches per raster.
//
//   * The jobs travel BY VALUE in the kernel arguments (SvgBatch), as k_image_nodes' do: no table upload, nothing to keep alive.
//   * A workgroup takes one tile of 64 x 16 texels of one job; SvgBatch::first_tile (a prefix sum over the jobs' tile counts, made by sv_plan
//     on the host) maps blockIdx.x to (job, tile).  Every branch on a job's fields is uniform per workgroup.
//   * Lane l of wave w owns the four consecutive texels x = 4 * (l & 15) .. + 3 of row 4 * w + (l >> 4) of the tile: it reads them, fixes
//     them and writes them back where they were.  One 16-byte global load and one 16-byte global store where the group is whole and the
//     surface's base and pitch are multiples of 16 (every surface smr_surface_create makes); a row's last, partial group and any other
//     surface go texel by texel.
//   * Per texel, exactly the two passes with the 8-bit word between them: k_premult mode 1's operations in its order
//     (remove_premultiplied_alpha.wgsl:24-35), then k_premult mode 0 with PXI_RGBA8_SRGB on that word (add_premultiplied_alpha.wgsl:24-35).
//     No special case for alpha 0 or 255: the function maps (c, alpha) to a byte, and the tests enumerate its 65 536 cases.
//   * Nothing outside [0, w) x [0, h) of a surface is read or written: not its row padding, not a byte behind its last row.
//   * No LDS, no barrier: the work is in place, one texel per owner.
// The source compiles under SMR_EMU (tests/emu/emu_svg_nodes.cpp): the CPU tests run it on guard-paged buffers.
#pragma once

#include "smr_internal.h"

#define SMR_SVG_MAX_JOBS 16
#define SMR_SVG_BLOCK 256
#define SMR_SVG_TILE_W 64
#define SMR_SVG_TILE_H 16

struct SvgJob {
    SurfView px;  // the pixmap as uploaded: premultiplied, gamma-encoded RGBA8; the node's bytes afterwards
    u32 wide;     // 1: the surface's base and pitch are multiples of 16 — whole groups are one 16-byte load and one 16-byte store (sv_plan)
};

struct SvgBatch {
    SvgJob j[SMR_SVG_MAX_JOBS];
    u32 first_tile[SMR_SVG_MAX_JOBS + 1];  // first_tile[i] .. first_tile[i + 1]: the workgroups of job i
    u32 n;
};

// Fills everything of B but j[].px and n; returns the number of workgroups (0: nothing to fix).  Host code, shared with the emulator.
// A job without a texel has no tile.
static inline u32 sv_plan(SvgBatch &B) {
    u32 total = 0;
    for (u32 i = 0; i < SMR_SVG_MAX_JOBS; i++) {
        B.first_tile[i] = total;
        if (i >= B.n) continue;
        SvgJob &J = B.j[i];
        J.wide = 0;
        if (!J.px.ptr || J.px.w <= 0 || J.px.h <= 0) continue;
        J.wide = (((uintptr_t)J.px.ptr | J.px.pitch) & 15u) == 0 ? 1u : 0u;
        const u32 tx = ((u32)J.px.w + SMR_SVG_TILE_W - 1) / SMR_SVG_TILE_W, ty = ((u32)J.px.h + SMR_SVG_TILE_H - 1) / SMR_SVG_TILE_H;
        total += tx * ty;
    }
    B.first_tile[SMR_SVG_MAX_JOBS] = total;
    return total;
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
    if (block >= B.first_tile[SMR_SVG_MAX_JOBS]) return;
    u32 i = 0;
#pragma unroll 1
    while (i + 1 < SMR_SVG_MAX_JOBS && block >= B.first_tile[i + 1]) i++;
    const SurfView px = B.j[i].px;
    const u32 wide = B.j[i].wide;
    const u32 tiles_x = ((u32)px.w + SMR_SVG_TILE_W - 1) / SMR_SVG_TILE_W;
    const u32 t = block - B.first_tile[i];
    const u32 tile_y = t / tiles_x, tile_x = t - tile_y * tiles_x;
    const int x0 = (int)(tile_x * SMR_SVG_TILE_W + 4u * (tid & 15u));
    const int y = (int)(tile_y * SMR_SVG_TILE_H + 4u * (tid >> 6) + ((tid >> 4) & 3u));
    if (x0 >= px.w || y >= px.h) return;
    const float *dec = tables, *thr = tables + 256;
    const int n = px.w - x0 < 4 ? px.w - x0 : 4;
    u8 *p = px.ptr + (size_t)y * px.pitch + (size_t)x0 * 4;
    if (wide && n == 4) {
        const uint4 v = g_ld_u32x4(p);
        g_st_u32x4(p, make_uint4(sv_fix_texel(v.x, dec, thr), sv_fix_texel(v.y, dec, thr), sv_fix_texel(v.z, dec, thr), sv_fix_texel(v.w, dec, thr)));
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (k < n) g_st_u32(p + 4 * k, sv_fix_texel(g_ld_u32(p + 4 * k), dec, thr));
    }
}

#ifndef SMR_EMU
__global__ void __launch_bounds__(SMR_SVG_BLOCK) k_svg_nodes(const SvgBatch B, const float *__restrict__ tables) {
    sv_workgroup(B, blockIdx.x, threadIdx.x, tables);
}
#endif

#endif  // __HIPCC__
