// smr_text_nodes.h — k_text_nodes: up to 16 Text rasters drawn by ONE launch, every workgroup looking only at the glyphs that touch its
// tile; and tx_blend_glyph, the step "one glyph over one RGBA8 texel", stated once for this kernel and k_blit_glyphs (smr_misc.hip).
// What TextRendererNode::render does per node (transformations/text_renderer.rs:72-167): Clear(background), then the glyph quads
// alpha-blended from the coverage atlas in order, the target re-quantised to RGBA8 after every glyph like a render-target store.
//
//   * Geometry of smr_node_tiles.h: jobs by value in the kernel arguments, one 64 x 16 tile of one job's surface per workgroup, four texels
//     of a row per lane, a 16-byte store where the surface allows.
//   * A job names its glyph records (the smr_glyph rectangle and the colour smr_blit_glyphs prepares on the host), its tile bins
//     (host/text_bins.h, tx_plan) and its A8 atlas in device memory.  A workgroup walks bin_glyph[bin_first[t] .. bin_first[t + 1]) of its
//     tile t, ascending: painter's order.  Bin and records are the same for every lane — scalar loads —; a lane skips a glyph whose rows or
//     columns miss its group.
//   * Coverage is read byte by byte and only for texels inside the glyph: the atlas has tight rows and the last glyph may end on its last
//     byte.
//   * Every texel of the surface is written exactly once — the encoded background, or the background with the bin's glyphs over it —, so
//     the surface needs no clear; nothing outside [0, w) x [0, h) is touched.
//   * No LDS, no barrier: lanes do not talk to each other.
// Two translation units include this: smr_text_nodes.hip, which defines SMR_TEXT_NODES_KERNEL first and so holds k_text_nodes and its
// launcher, and smr_misc.hip, for the blend and the host helpers of smr_blit_glyphs (that file compiles without host/).
// The source compiles under SMR_EMU (tests/emu/emu_text_nodes.cpp): the CPU tests run it on guard-paged buffers.
#pragma once

#include <cmath>

#include "smr_node_tiles.h"

// One glyph as the kernel reads it: smr_glyph's rectangle, then the colour as k_blit_glyphs takes it — clamped, through srgb_to_linear_f64
// in sRGB mode — and the straight alpha, unchanged.
struct TextGlyph {
    int dst_x, dst_y, w, h, atlas_x, atlas_y;
    float r, g, b, a;
};

struct TextJob {
    SurfView dst;             // the raster: every texel of it is written
    float bg[4];              // as smr_blit_glyphs takes it
    const TextGlyph *glyphs;  // device memory, like the three below
    const u32 *bin_first;     // [tiles + 1]
    const u32 *bin_glyph;
    const u8 *atlas;          // A8, rows atlas_w bytes apart
    u32 atlas_w;
    u32 wide;                 // nt_wide(dst) (tx_batch_plan)
};

struct TextBatch {
    TextJob j[SMR_NODE_MAX_JOBS];
    u32 first_tile[SMR_NODE_MAX_JOBS + 1];  // first_tile[i] .. first_tile[i + 1]: the workgroups of job i
    u32 n;
    u32 srgb;  // the context's mode, one per launch: 1 = the target is an sRGB view (k_blit_glyphs' `srgb`)
};
static_assert(sizeof(TextBatch) <= 2048, "the batch travels in the kernel arguments");

// Fills everything of B but j[]'s own fields, n and srgb; returns the number of workgroups.  Host code, shared with the emulator.
static inline u32 tx_batch_plan(TextBatch &B) {
    return nt_plan(B, [](const TextJob &J) { return &J.dst; });
}

#ifndef SMR_EMU
// What smr_blit_glyphs and smr_text_nodes do to a run on the host.  A glyph's colour as the kernels take it: clamped, and linear
// (wgpu/utils.rs:74-81, evaluated in f64) where the target is an sRGB view
static inline void tx_glyph_colour(bool srgb, const smr_glyph &g, float c[3]) {
    for (int k = 0; k < 3; k++) {
        float v = g.color[k];
        v = !(v > 0.0f) ? 0.0f : (v > 1.0f ? 1.0f : v);
        const double d = (double)v;
        c[k] = srgb ? (float)(d < 0.04045 ? d / 12.92 : pow((d + 0.055) / 1.055, 2.4)) : v;
    }
}
// ... and the rule for its rectangles: every glyph reads inside its atlas
static inline int tx_check_glyphs(smr_ctx *ctx, const char *who, const smr_glyph *glyphs, u32 n, u32 atlas_w, u32 atlas_h) {
    for (u32 i = 0; i < n; i++) {
        const smr_glyph &g = glyphs[i];
        if (g.w < 0 || g.h < 0 || g.atlas_x < 0 || g.atlas_y < 0 || (u32)(g.atlas_x + g.w) > atlas_w || (u32)(g.atlas_y + g.h) > atlas_h)
            return smr_fail(ctx, SMR_ERR_INVALID, "%s: glyph %u reads outside the %ux%u atlas", who, i, atlas_w, atlas_h);
    }
    return SMR_OK;
}
#endif

#ifdef __HIPCC__

// One glyph of colour (cr, cg, cb) and straight alpha ca, with coverage byte `cov8`, OVER the texel (r, g, b, a) held as 8-bit codes:
// k_blit_glyphs' statements, operation for operation (everything is compiled with -ffp-contract=off).
__device__ __forceinline__ void tx_blend_glyph(u32 &r, u32 &g, u32 &b, u32 &a, u32 cov8, float cr, float cg, float cb, float ca, int srgb,
                                               const float *__restrict__ dec, const float *__restrict__ thr) {
    const float cov = (float)cov8 / 255.0f;
    const float al = ca * cov;
    const float inv = 1.0f - al;
    if (srgb) {
        r = srgb_encode8(cr * al + dec[r] * inv, thr);
        g = srgb_encode8(cg * al + dec[g] * inv, thr);
        b = srgb_encode8(cb * al + dec[b] * inv, thr);
    } else {
        r = unorm8(cr * al + ((float)r / 255.0f) * inv);
        g = unorm8(cg * al + ((float)g / 255.0f) * inv);
        b = unorm8(cb * al + ((float)b / 255.0f) * inv);
    }
    a = unorm8(al + ((float)a / 255.0f) * inv);
}

// A bin entry and a record are the same for the whole workgroup and nothing writes them while the kernel runs: read through the constant
// address space, i.e. by scalar loads.  Coverage is one byte per lane and texel, a global load.
#if !defined(SMR_EMU)
__device__ __forceinline__ u32 tx_ld_uniform_u32(const u32 *p) { return *((__attribute__((address_space(4))) const u32 *)(uintptr_t)(p)); }
__device__ __forceinline__ TextGlyph tx_ld_uniform_glyph(const TextGlyph *p) {
    const __attribute__((address_space(4))) u32 *q = (__attribute__((address_space(4))) const u32 *)(uintptr_t)(p);  // (ten dwords: the compiler merges them)
    TextGlyph g;
    g.dst_x = (int)q[0]; g.dst_y = (int)q[1]; g.w = (int)q[2]; g.h = (int)q[3]; g.atlas_x = (int)q[4]; g.atlas_y = (int)q[5];
    g.r = __uint_as_float(q[6]); g.g = __uint_as_float(q[7]); g.b = __uint_as_float(q[8]); g.a = __uint_as_float(q[9]);
    return g;
}
__device__ __forceinline__ u32 tx_ld_cov(const u8 *p) { return *SMR_GLOBAL_PTR(const u8, p); }
#else
static inline u32 tx_ld_uniform_u32(const u32 *p) { return *p; }
static inline TextGlyph tx_ld_uniform_glyph(const TextGlyph *p) { return *p; }
static inline u32 tx_ld_cov(const u8 *p) { return *p; }
#endif

// What thread `tid` of workgroup `block` does.  Every branch on B's fields and on the bin is uniform per workgroup.
__device__ __forceinline__ void tx_workgroup(const TextBatch &B, u32 block, u32 tid, const float *__restrict__ tables) {
    if (block >= B.first_tile[SMR_NODE_MAX_JOBS]) return;
    const u32 i = nt_job_of(B.first_tile, block);
    const SurfView dst = B.j[i].dst;
    const u32 wide = B.j[i].wide;
    const int srgb = (int)B.srgb;
    const NodeTile T = nt_tile_of(B.first_tile, i, block, dst.w);
    const u32 tile = block - B.first_tile[i];
    const int x0 = (int)nt_lane_x(T.x * SMR_NODE_TILE_W, tid);
    const int y = (int)nt_lane_y(T.y * SMR_NODE_TILE_H, tid);
    if (x0 >= dst.w || y >= dst.h) return;
    const float *dec = tables, *thr = tables + 256;
    const int n = dst.w - x0;  // the texels the row has from x0 on: the group is min(n, 4) of them

    u32 r, g, b, a;
    if (srgb) { r = srgb_encode8(B.j[i].bg[0], thr); g = srgb_encode8(B.j[i].bg[1], thr); b = srgb_encode8(B.j[i].bg[2], thr); }
    else { r = unorm8(B.j[i].bg[0]); g = unorm8(B.j[i].bg[1]); b = unorm8(B.j[i].bg[2]); }
    a = unorm8(B.j[i].bg[3]);
    u32 pr[4], pg[4], pb[4], pa[4];
#pragma unroll
    for (int k = 0; k < 4; k++) { pr[k] = r; pg[k] = g; pb[k] = b; pa[k] = a; }

    const TextGlyph *glyphs = B.j[i].glyphs;
    const u32 *bin_glyph = B.j[i].bin_glyph;
    const u8 *atlas = B.j[i].atlas;
    const u32 aw = B.j[i].atlas_w;
    const u32 e0 = tx_ld_uniform_u32(B.j[i].bin_first + tile), e1 = tx_ld_uniform_u32(B.j[i].bin_first + tile + 1);
#pragma unroll 1
    for (u32 e = e0; e < e1; e++) {
        const TextGlyph gl = tx_ld_uniform_glyph(glyphs + tx_ld_uniform_u32(bin_glyph + e));
        // 0 <= y - dst_y < h and 0 <= x - dst_x < w, in unsigned arithmetic: the differences of a caller's coordinates do not fit int32
        const u32 gy = (u32)y - (u32)gl.dst_y;
        if (gy >= (u32)gl.h) continue;
        const u32 gx0 = (u32)x0 - (u32)gl.dst_x;
        const u8 *row = atlas + (size_t)((u32)gl.atlas_y + gy) * aw + (u32)gl.atlas_x;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const u32 gx = gx0 + (u32)k;
            if (k < n && gx < (u32)gl.w) tx_blend_glyph(pr[k], pg[k], pb[k], pa[k], tx_ld_cov(row + gx), gl.r, gl.g, gl.b, gl.a, srgb, dec, thr);
        }
    }
    u32 px[4];
#pragma unroll
    for (int k = 0; k < 4; k++) px[k] = pr[k] | (pg[k] << 8) | (pb[k] << 16) | (pa[k] << 24);
    nt_store_group(dst.ptr + (size_t)y * dst.pitch + (size_t)x0 * 4, wide, n, px);
}

#if !defined(SMR_EMU) && defined(SMR_TEXT_NODES_KERNEL)
__global__ void __launch_bounds__(SMR_NODE_BLOCK) k_text_nodes(const TextBatch B, const float *__restrict__ tables) {
    tx_workgroup(B, blockIdx.x, threadIdx.x, tables);
}
#endif

#endif  // __HIPCC__
