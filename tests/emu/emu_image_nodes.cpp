// TEST INFRASTRUCTURE — not part of the product; nothing in smelter_amd/ builds, links or loads this.
//
// k_image_nodes' source (smelter_amd/csrc/smr_image_nodes.h: in_plan on the host, in_workgroup per thread) compiled for the CPU, so that
// tests/test_emu_image_nodes.py can run one launch — every workgroup, every thread, in turn: threads do not talk to each other — on buffers
// that are exactly as large as the surfaces they hold (emu_guard.h: the byte after, or before, them is an unmapped page).  Shims, tables and
// the alignment rule: emu_node_kernel.h.  The reference it is held against is made here too: a loop over sample_rgba_bilinear and store_texel (smr_shader_dev.h),
// one texel at a time — what k_rescale_bilinear does.
#include "emu_node_kernel.h"
#include "smr_image_nodes.h"

// Job i: the tight src_w[i] x src_h[i] RGBA8 texels src_px[i] drawn into dst_w[i] x dst_h[i].  The source sits in a buffer of exactly
// src_w * 4 * src_h bytes.  The destination's rows are dst_pitch[i] bytes apart and start dst_off[i] bytes into a buffer of exactly
// dst_off + dst_pitch * (dst_h - 1) + dst_w * 4 bytes (0 texels: dst_off bytes), 0xc3 throughout before the launch; it comes back whole in
// dst_out[i].  ref_out[i]: dst_w * dst_h * 4 bytes, the texel-by-texel reference.  wide_out[i]: 1 = whole groups left as 16-byte stores.
// Returns the number of workgroups the launch has, or < 0.
extern "C" int emu_image_nodes(int n, const u8 *const *src_px, const int *src_w, const int *src_h, const int *dst_w, const int *dst_h,
                               const u32 *dst_pitch, const u32 *dst_off, int srgb, u8 *const *dst_out, u8 *const *ref_out, u32 *wide_out) {
    if (n < 0 || n > SMR_NODE_MAX_JOBS) return -1;
    const EmuTables tables;
    if (!tables.ptr) return -9;
    const float *tab = tables.ptr;
    const int pxi = srgb ? PXI_RGBA8_SRGB : PXI_RGBA8_UNORM;
    const size_t align = emu_surface_align();

    std::vector<GuardBuf> src((size_t)n), dst((size_t)n);
    std::vector<size_t> dst_bytes((size_t)n);
    ImageBatch B;
    memset(&B, 0, sizeof(B));
    B.n = (u32)n;
    for (int i = 0; i < n; i++) {
        if (src_w[i] <= 0 || src_h[i] <= 0 || dst_w[i] < 0 || dst_h[i] < 0) return -1;
        const bool empty = dst_w[i] == 0 || dst_h[i] == 0;
        if (!empty && dst_pitch[i] < (u32)dst_w[i] * 4) return -1;
        src[i].alloc((size_t)src_w[i] * 4 * src_h[i], 0, align);
        memcpy(src[i].ptr, src_px[i], (size_t)src_w[i] * 4 * src_h[i]);
        dst_bytes[i] = dst_off[i] + (empty ? 0 : (size_t)dst_pitch[i] * (dst_h[i] - 1) + (size_t)dst_w[i] * 4);
        dst[i].alloc(dst_bytes[i] ? dst_bytes[i] : 4, 0xc3, align);
        ImageJob &J = B.j[i];
        J.src.ptr = src[i].ptr; J.src.pitch = (u32)src_w[i] * 4; J.src.w = src_w[i]; J.src.h = src_h[i];
        J.dst.ptr = dst[i].ptr + dst_off[i]; J.dst.pitch = dst_pitch[i]; J.dst.w = dst_w[i]; J.dst.h = dst_h[i];
        J.pxi = pxi;
    }
    const u32 blocks = in_plan(B);
    for (int i = 0; i < n; i++) wide_out[i] = B.j[i].wide;
    // (one workgroup more than the launch has: it must do nothing)
    for (u32 blk = 0; blk <= blocks; blk++)
        for (u32 tid = 0; tid < SMR_NODE_BLOCK; tid++) in_workgroup(B, blk, tid, tab);
    for (int i = 0; i < n; i++) {
        if (dst_bytes[i]) memcpy(dst_out[i], dst[i].ptr, dst_bytes[i]);
        if (dst_w[i] == 0 || dst_h[i] == 0) continue;
        SurfView ref;
        ref.ptr = ref_out[i]; ref.pitch = (u32)dst_w[i] * 4; ref.w = dst_w[i]; ref.h = dst_h[i];
        for (int y = 0; y < ref.h; y++)
            for (int x = 0; x < ref.w; x++) {
                const float4 o = sample_rgba_bilinear(B.j[i].src, pxi, ((float)x + 0.5f) / (float)ref.w, ((float)y + 0.5f) / (float)ref.h, tab);
                store_texel(ref, pxi, x, y, o, tab + 256);
            }
    }
    return (int)blocks;
}
