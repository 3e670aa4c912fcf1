// smr_web_view.h — k_web_view: a WebView node's page and up to 16 of its children drawn into the node's texture by ONE launch.
// The reference (transformations/web_renderer/renderer.rs:78-134, shader.rs:53-114, render_website.wgsl) clears the target and issues one
// render pass per layer — the page, a BGRA bitmap the browser painted, and one rectangle per child — each a read-modify-write of the RGBA8
// target with PREMULTIPLIED_ALPHA_BLENDING: N + 1 passes over a surface that is typically 1080p and repaints up to every frame.  Host
// enqueue is half of the frame period (profiles/r06_host_rate.txt): the argument that produced k_move_rects and k_image_nodes.
//
//   * The job travels BY VALUE in the kernel arguments (WebJob): no table upload, no host synchronisation, nothing to keep alive.
//   * One 64 x 16 tile of the destination per workgroup of a 2-D grid, four texels of a row per lane (smr_node_tiles.h: the lane mapping
//     and the group load / store; not its job table — there is one job), the running colour of each held in a register as its RGBA8 word.
//   * Page texel: one dword load, B and R exchanged by a byte permute (render_website.wgsl:36-40).  As the first layer (the page below the
//     children) it IS the running colour: encode(decode(b)) == b, so a blend onto the transparent target leaves the very bytes.  As the last
//     layer (the page above the children) it is decoded and blended like any other.
//   * Child layer i covers pixel (px, py) iff x <= px + 0.5 < x + width and likewise in y — the rasteriser's rule for an axis-aligned
//     quad (the reference's rectangles always are: browser_client.rs:86-92) —, the integer bounds computed once on the host (wv_layer_set)
//     and clipped to the page.  Its fragment is sample_rgba_bilinear(src, (px + 0.5 - x) / width, (py + 0.5 - y) / height): linear filter,
//     clamp to edge.  Every layer after the first is blend_store (smr_layout_dev.h): premultiplied-alpha blending onto the 8-bit target,
//     re-encoded after each layer, in both rendering modes — the bytes of N + 1 separate passes.
//   * A layer whose bounds miss the workgroup's tile is skipped by a workgroup-uniform branch; a tile no child touches is a pure swizzled
//     copy of 16-byte groups.
//   * A node with more than 16 children continues with further launches that LOAD the destination instead of clearing it (WebJob::load).
//   * The four results leave as a group (nt_store_group); the page (and a loaded destination) is read as one (nt_load_group).  Nothing
//     outside [0, w) x [0, h) of the destination is written.
//   * No LDS, no barrier: threads do not talk to each other.  Vector stores only.
// hipcc --offload-arch=gfx950 -O3 --save-temps reports for k_web_view: 57 VGPRs, 0 AGPRs, 50 SGPRs, no scratch, no LDS, 8 waves per SIMD.
// The source compiles under SMR_EMU (tests/emu/emu_web_view.cpp): the CPU tests run it on guard-paged buffers.
#pragma once

#include <cmath>

#include "smr_layout_dev.h"
#include "smr_node_tiles.h"

// (this kernel's former names for the shared geometry: emulator drivers written against them still compile; the values are smr_node_tiles.h's)
#define SMR_WEB_BLOCK SMR_NODE_BLOCK
#define SMR_WEB_TILE_W SMR_NODE_TILE_W
#define SMR_WEB_TILE_H SMR_NODE_TILE_H

#define SMR_WEB_MAX_LAYERS 16

enum { WV_PAGE_NONE = 0, WV_PAGE_BELOW = 1, WV_PAGE_ABOVE = 2 };

struct WebLayer {
    SurfView src;        // the child's premultiplied RGBA8 node texture
    float x, y, w, h;    // its rectangle in page pixels (getBoundingClientRect)
    int x0, y0, x1, y1;  // the pixels it covers, half open, clipped to the page; x0 >= x1 or y0 >= y1: none (wv_layer_set)
};

struct WebJob {
    SurfView page, dst;  // premultiplied BGRA8 in, premultiplied RGBA8 out; the same width and height
    WebLayer l[SMR_WEB_MAX_LAYERS];
    u32 n;               // layers of l[] in use
    int pxi;             // PXI_RGBA8_SRGB / PXI_RGBA8_UNORM: how texels are decoded and encoded
    u32 page_mode;       // WV_PAGE_NONE: children only | _BELOW: the page is the first layer, on the cleared target | _ABOVE: the last layer
    u32 load;            // 1: the running colour starts from the destination's texels (a continuation launch), 0: from transparent
    u32 wide;            // nt_wide(dst): whole groups leave as one 16-byte store
    u32 page_wide;       // nt_wide(page): whole groups arrive as one 16-byte load
};

// Layer `L`'s rectangle and the pixels it covers on a page of page_w x page_h.  Host code, shared with the emulator.  Pixel px is covered
// iff x <= px + 0.5 < x + width: px from ceil(x - 0.5) up to, not including, ceil(x + width - 0.5).  A rectangle with a non-finite
// coordinate or a non-finite or non-positive size has no pixels.
static inline void wv_layer_set(WebLayer &L, float x, float y, float w, float h, int page_w, int page_h) {
    L.x = x; L.y = y; L.w = w; L.h = h;
    L.x0 = L.y0 = L.x1 = L.y1 = 0;
    if (!std::isfinite(x) || !std::isfinite(y) || !std::isfinite(w) || !std::isfinite(h) || !(w > 0.0f) || !(h > 0.0f)) return;
    if (!L.src.ptr || L.src.w <= 0 || L.src.h <= 0) return;
    auto clip = [](double v, int hi) { return v <= 0.0 ? 0 : v >= (double)hi ? hi : (int)v; };
    L.x0 = clip(std::ceil((double)x - 0.5), page_w);
    L.x1 = clip(std::ceil((double)x + (double)w - 0.5), page_w);
    L.y0 = clip(std::ceil((double)y - 0.5), page_h);
    L.y1 = clip(std::ceil((double)y + (double)h - 0.5), page_h);
}

// A node with n children takes wv_launches(n) launches; launch k draws children 16 k .. 16 k + J.n - 1.  Over content (under == 0) the
// page is the first layer of launch 0; under content it is the last layer of the last launch; every launch but the first loads the
// destination.  Without children the page alone is the first layer either way.  Host code, shared with the emulator.
static inline u32 wv_launches(u32 n) { return n ? (n + SMR_WEB_MAX_LAYERS - 1) / SMR_WEB_MAX_LAYERS : 1u; }
static inline void wv_launch_set(WebJob &J, u32 k, u32 n, int under) {
    const u32 launches = wv_launches(n), at = k * SMR_WEB_MAX_LAYERS;
    J.n = n - at < SMR_WEB_MAX_LAYERS ? n - at : SMR_WEB_MAX_LAYERS;
    J.load = k ? 1u : 0u;
    J.page_mode = (under && n) ? (k + 1 == launches ? WV_PAGE_ABOVE : WV_PAGE_NONE) : (k == 0 ? WV_PAGE_BELOW : WV_PAGE_NONE);
}

// Fills wide / page_wide; returns false when the job has no texel to write.
static inline bool wv_plan(WebJob &J) {
    J.wide = nt_wide(J.dst);
    J.page_wide = nt_wide(J.page);
    return J.dst.ptr && J.dst.w > 0 && J.dst.h > 0 && (J.page_mode == WV_PAGE_NONE || J.page.ptr);
}

#ifdef __HIPCC__

// BGRA8 -> RGBA8: bytes 0 and 2 change places
__device__ __forceinline__ u32 wv_swizzle(u32 v) {
#ifdef SMR_EMU
    return (v & 0xff00ff00u) | ((v >> 16) & 0xffu) | ((v & 0xffu) << 16);
#else
    return __builtin_amdgcn_perm(v, v, 0x03000102u);
#endif
}

// What thread `tid` of workgroup (bx, by) does.  Every branch on J's fields and on the tile is uniform per workgroup.
__device__ __forceinline__ void wv_workgroup(const WebJob &J, u32 bx, u32 by, u32 tid, const float *__restrict__ tables) {
    const SurfView dst = J.dst;
    const int tx0 = (int)(bx * SMR_NODE_TILE_W), ty0 = (int)(by * SMR_NODE_TILE_H);
    const int x0 = tx0 + (int)nt_lane_x(0u, tid);
    const int y = ty0 + (int)nt_lane_y(0u, tid);
    if (x0 >= dst.w || y >= dst.h) return;
    const float *dec = tables, *thr = tables + 256;
    const int pxi = J.pxi;
    const int srgb = pxi == PXI_RGBA8_SRGB ? 1 : 0;
    const int n = dst.w - x0;  // the texels the row has from x0 on: the group is min(n, 4) of them
    u8 *p = dst.ptr + (size_t)y * dst.pitch + (size_t)x0 * 4;
    u32 acc[4] = {0u, 0u, 0u, 0u};  // RGBA8 of the cleared target (wgpu::Color::TRANSPARENT, shader.rs:65)
    u32 pg[4] = {0u, 0u, 0u, 0u};
    if (J.page_mode != WV_PAGE_NONE) {
        nt_load_group(J.page.ptr + (size_t)y * J.page.pitch + (size_t)x0 * 4, J.page_wide, n, pg);
#pragma unroll
        for (int k = 0; k < 4; k++) pg[k] = wv_swizzle(pg[k]);
    }
    if (J.load) nt_load_group(p, J.wide, n, acc);
    if (J.page_mode == WV_PAGE_BELOW) {
#pragma unroll
        for (int k = 0; k < 4; k++) acc[k] = pg[k];
    }
    const float fy = (float)y + 0.5f;
#pragma unroll 1
    for (u32 i = 0; i < J.n; i++) {
        const int lx0 = J.l[i].x0, ly0 = J.l[i].y0, lx1 = J.l[i].x1, ly1 = J.l[i].y1;
        if (lx1 <= tx0 || lx0 >= tx0 + SMR_NODE_TILE_W || ly1 <= ty0 || ly0 >= ty0 + SMR_NODE_TILE_H || lx0 >= lx1 || ly0 >= ly1) continue;  // (uniform)
        if (y < ly0 || y >= ly1) continue;
        const SurfView src = J.l[i].src;
        const float lx = J.l[i].x, lw = J.l[i].w;
        const float v = (fy - J.l[i].y) / J.l[i].h;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int px = x0 + k;
            if (k < n && px >= lx0 && px < lx1) {
                const float4 frag = sample_rgba_bilinear(src, pxi, ((float)px + 0.5f - lx) / lw, v, dec);
                acc[k] = blend_store(acc[k], frag, srgb, dec, thr);
            }
        }
    }
    if (J.page_mode == WV_PAGE_ABOVE) {
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (k < n) acc[k] = blend_store(acc[k], decode_rgba8(pg[k], pxi, dec), srgb, dec, thr);
    }
    nt_store_group(p, J.wide, n, acc);
}

#ifndef SMR_EMU
__global__ void __launch_bounds__(SMR_NODE_BLOCK) k_web_view(const WebJob J, const float *__restrict__ tables) {
    wv_workgroup(J, blockIdx.x, blockIdx.y, threadIdx.x, tables);
}
#endif

#endif  // __HIPCC__
