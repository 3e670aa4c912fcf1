// TEST INFRASTRUCTURE — not part of the product; nothing in smelter_amd/ builds, links or loads this.
//
// k_web_view's source (smelter_amd/csrc/smr_web_view.h: wv_layer_set / wv_launch_set / wv_plan on the host, wv_workgroup per thread) compiled
// for the CPU, so that tests/test_emu_web_view.py can run a WebView node's launches — every workgroup, every thread, in turn: threads do not
// talk to each other — on buffers that are exactly as large as the surfaces they hold (emu_guard.h: the byte after, or before, them is an
// unmapped page).  Shims, tables and the alignment rule: emu_node_kernel.h.  The launches are made the way smr_web_view (smr_layout.hip) makes them.
#include "emu_node_kernel.h"
#include "smr_web_view.h"

// The page: w x h BGRA8 texels page_px (tight) in a buffer whose rows are page_pitch bytes apart (exactly page_pitch * (h - 1) + w * 4
// bytes).  Child i: the tight src_w[i] x src_h[i] RGBA8 texels src_px[i] (src_w[i] == 0: no texture) on rects[4 i .. 4 i + 3] = x, y, width,
// height.  The destination's rows are dst_pitch bytes apart and start dst_off bytes into a buffer of exactly dst_off + dst_pitch * (h - 1)
// + w * 4 bytes, 0xc3 throughout before the first launch; it comes back whole in dst_out.  info_out[0] = the launches made, [1] = 1 when
// whole groups left as 16-byte stores, [2] = 1 when the page arrived as 16-byte loads.  Returns the workgroups per launch, or < 0.
extern "C" int emu_web_view(const u8 *page_px, int w, int h, u32 page_pitch, int n, const u8 *const *src_px, const int *src_w, const int *src_h,
                            const float *rects, int under, int srgb, u32 dst_pitch, u32 dst_off, u8 *dst_out, u32 *info_out) {
    if (w <= 0 || h <= 0 || n < 0 || page_pitch < (u32)w * 4 || dst_pitch < (u32)w * 4) return -1;
    const EmuTables tables;
    if (!tables.ptr) return -9;
    const float *tab = tables.ptr;
    const size_t align = emu_surface_align();

    GuardBuf page, dst;
    page.alloc((size_t)page_pitch * (h - 1) + (size_t)w * 4, 0x5a, align);
    for (int y = 0; y < h; y++) memcpy(page.ptr + (size_t)y * page_pitch, page_px + (size_t)y * w * 4, (size_t)w * 4);
    const size_t dst_bytes = dst_off + (size_t)dst_pitch * (h - 1) + (size_t)w * 4;
    dst.alloc(dst_bytes, 0xc3, align);
    std::vector<GuardBuf> src((size_t)n);
    for (int i = 0; i < n; i++) {
        if (src_w[i] <= 0 || src_h[i] <= 0) continue;
        src[i].alloc((size_t)src_w[i] * 4 * src_h[i], 0, align);
        memcpy(src[i].ptr, src_px[i], (size_t)src_w[i] * 4 * src_h[i]);
    }
    const u32 tiles_x = nt_tiles_x(w), tiles_y = nt_tiles_y(h);
    info_out[0] = info_out[1] = info_out[2] = 0;
    for (u32 k = 0; k < wv_launches((u32)n); k++) {
        WebJob J;
        memset(&J, 0, sizeof(J));
        J.dst.ptr = dst.ptr + dst_off; J.dst.pitch = dst_pitch; J.dst.w = w; J.dst.h = h;
        J.page.ptr = page.ptr; J.page.pitch = page_pitch; J.page.w = w; J.page.h = h;
        J.pxi = srgb ? PXI_RGBA8_SRGB : PXI_RGBA8_UNORM;
        wv_launch_set(J, k, (u32)n, under);
        for (u32 i = 0; i < J.n; i++) {
            const u32 c = k * SMR_WEB_MAX_LAYERS + i;
            if (src[c].ptr) { J.l[i].src.ptr = src[c].ptr; J.l[i].src.pitch = (u32)src_w[c] * 4; J.l[i].src.w = src_w[c]; J.l[i].src.h = src_h[c]; }
            wv_layer_set(J.l[i], rects[4 * c], rects[4 * c + 1], rects[4 * c + 2], rects[4 * c + 3], w, h);
        }
        if (!wv_plan(J)) return -2;
        info_out[0]++; info_out[1] = J.wide; info_out[2] = J.page_wide;
        // (one row and one column of workgroups more than the launch has: they must do nothing)
        for (u32 by = 0; by <= tiles_y; by++)
            for (u32 bx = 0; bx <= tiles_x; bx++)
                for (u32 tid = 0; tid < SMR_NODE_BLOCK; tid++) wv_workgroup(J, bx, by, tid, tab);
    }
    memcpy(dst_out, dst.ptr, dst_bytes);
    return (int)(tiles_x * tiles_y);
}
