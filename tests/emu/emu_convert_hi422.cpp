// TEST INFRASTRUCTURE — not part of the product; nothing in smelter_amd/ builds, links or loads this.
//
// The 10-bit 4:2:2 input converter's source (smelter_amd/csrc/smr_convert_hi422.h: cv422_run / cv210_run, a vertical run of 4 x 4 pixel blocks per
// call; cv422_share, a wave's share of a launch; cv210_pixel_codes, the general v210 kernel's fetch) compiled for the CPU, so that
// tests/test_emu_convert_hi422.py can hold it to the oracle, to tests/hi_depth_model.py and to tests/hi422_model.py byte for byte without a GPU.
// Same shims as emu_convert_hi.cpp.
#include <vector>

#include <hip/hip_runtime.h>

thread_local dim3 threadIdx, blockIdx;
dim3 gridDim, blockDim;

#include "emu_device.h"
#include "emu_guard.h"
EmuBlock *emu_blk = nullptr;
thread_local unsigned char *emu_smem = nullptr;
void __syncthreads() {}

#include "smr_convert_hi422.h"

namespace {

struct Plane {
    GuardBuf buf;
    SurfView view;
};
// `w` texels of `bpp` bytes per row on `pitch`; the buffer is exactly pitch * h bytes, padding filled with a byte no plane contains by accident
Plane make_plane(const u8 *tight, int w, int h, int bpp, u32 pitch, u8 fill, size_t align) {
    Plane p;
    p.buf.alloc((size_t)pitch * h, fill, align);
    for (int y = 0; y < h; y++) memcpy(p.buf.ptr + (size_t)y * pitch, tight + (size_t)y * w * bpp, (size_t)w * bpp);
    p.view.ptr = p.buf.ptr; p.view.pitch = pitch; p.view.w = w; p.view.h = h;
    return p;
}
// emu_set_guard(.., 1): the smallest pitch conv_route (smr_convert.hip) lets through — the row's own bytes; otherwise a wide one: the
// allocator's 256-byte pitch, and for v210 a capture card's stride ((w + 47) / 48) * 128: ONE memory contract for both.
u32 plane_pitch(size_t row_bytes) { return emu_min_pitch ? (u32)row_bytes : (u32)((row_bytes + 255) & ~(size_t)255); }
u32 v210_pitch(int w) { return emu_min_pitch ? 16u * (u32)((w + 5) / 6) : (u32)((w + 47) / 48) * 128u; }
u32 node_pitch(int w, int rgb12) {
    if (emu_min_pitch) return emu_dst_pitch(rgb12 ? (u32)((3 * w + 15) & ~15) : (u32)w * 4);  // (guard mode 3: + 32 bytes of watched padding)
    return rgb12 ? (u32)((3 * w + 255) & ~255) : (u32)w * 4;
}
size_t node_row_bytes(int w, int rgb12) { return (size_t)w * (rgb12 ? 3 : 4); }

struct Tables {
    float ylut[CVHI_CODES], ulut[CVHI_CODES];
    Tables() { cvhi_build_tables(ylut, ulut, 0u, 1u); }
};

struct Frame {
    Plane py, pu, pv;
    GuardBuf dst;
    u32 dpitch;
    int w, h, rgb12;
    ConvJob job(int layout) {
        ConvJob J;
        memset(&J, 0, sizeof(J));
        J.yp = py.view;
        J.up = layout == CV422_V210 ? py.view : pu.view;
        J.vp = layout == CV422_PLANAR ? pv.view : J.up;
        J.dst.ptr = dst.ptr; J.dst.pitch = dpitch; J.dst.w = w; J.dst.h = h;
        J.full = 0; J.nv = layout == CV422_P210; J.sx = 1; J.sy = 0; J.packed = 0; J.rgb12 = rgb12;
        return J;
    }
    void make(const u8 *y, const u8 *u, const u8 *v, int w_, int h_, int layout, int rgb12_, u32 seed) {
        w = w_; h = h_; rgb12 = rgb12_;
        if (layout == CV422_V210) {
            py = make_plane(y, 4 * ((w + 5) / 6), h, 4, v210_pitch(w), 0x5a, 8);
        } else {
            const int cbpp = layout == CV422_P210 ? 4 : 2;
            py = make_plane(y, w, h, 2, plane_pitch((size_t)w * 2), 0x5a, 8);
            pu = make_plane(u, w / 2, h, cbpp, plane_pitch((size_t)(w / 2) * cbpp), 0xa5, 4);
            if (layout == CV422_PLANAR) pv = make_plane(v, w / 2, h, 2, plane_pitch((size_t)(w / 2) * 2), 0x3c, 4);
        }
        dpitch = node_pitch(w, rgb12);
        dst.alloc((size_t)dpitch * h, 0, 16);
        emu_pad_fill(dst.ptr, dpitch, h, seed);
    }
    int finish(u8 *out, u32 seed) {
        if (int rc = emu_pad_check(dst.ptr, dpitch, node_row_bytes(w, rgb12), h, seed, rgb12 ? "RGB12 node" : "RGBA8 node")) return rc;
        const size_t row = node_row_bytes(w, rgb12);
        for (int r = 0; r < h; r++) memcpy(out + (size_t)r * row, dst.ptr + (size_t)r * dpitch, row);
        return 0;
    }
};

void run_one(const ConvJob &J, int layout, int rgb12, int g, int P, int nb, const Tables &T) {
    if (layout == CV422_V210) {
        if (rgb12) cv210_run<true>(J, g, P, nb, T.ylut, T.ulut);
        else cv210_run<false>(J, g, P, nb, T.ylut, T.ulut);
    } else if (layout == CV422_P210) {
        if (rgb12) cv422_run<true, true>(J, g, P, nb, T.ylut, T.ulut);
        else cv422_run<true, false>(J, g, P, nb, T.ylut, T.ulut);
    } else {
        if (rgb12) cv422_run<false, true>(J, g, P, nb, T.ylut, T.ulut);
        else cv422_run<false, false>(J, g, P, nb, T.ylut, T.ulut);
    }
}

bool block_geometry(int w, int h) { return w % 4 == 0 && w >= 8 && h % 2 == 0 && h >= 2; }

}  // namespace

// layout 0 planar: y: w x h words, u, v: (w / 2) x h words | 1 P210: u = interleaved (w / 2) x h x 2 words, v ignored | 2 v210: y = the
// 4 ceil(w / 6) x h dwords, u, v ignored.  out: w x h x 4 tight; rgb12 != 0: out = h rows of 3 w bytes (12-byte groups of four pixels:
// R x 4, G x 4, B x 4).  Runs of nb >= 1 block rows.
extern "C" int emu_convert_hi422_run(const u8 *y, const u8 *u, const u8 *v, int w, int h, int layout, int rgb12, int nb, u8 *out) {
    if (!block_geometry(w, h) || nb < 1 || layout < 0 || layout > 2) return -1;
    static const Tables T;
    Frame F;
    F.make(y, u, v, w, h, layout, rgb12, 0xc0de);
    const ConvJob J = F.job(layout);
    for (int P = 0; 4 * P < h; P += nb)
        for (int g = 0; 4 * g < w; g++) run_one(J, layout, rgb12, g, P, nb, T);
    return F.finish(out, 0xc0de);
}

// What a launch of k_yuv422_hi_to_rgba<layout> computes: `n` frames partitioned the way the host does (cv_plan) over `waves` WORKGROUPS,
// every lane of every wave emulated in turn.  Pointers and ints per frame; output layout per frame as emu_convert_hi422_run.
extern "C" int emu_convert_hi422_shares(int n, const u8 *const *ys, const u8 *const *us, const u8 *const *vs, const int *ws, const int *hs, int layout,
                                        const int *rgb12s, int waves, u8 *const *outs) {
    if (n < 1 || n > MAX_CONV_JOBS || waves < 1 || layout < 0 || layout > 2) return -1;
    static const Tables T;
    std::vector<Frame> F(n);
    ConvBatch B;
    memset(&B, 0, sizeof(B));
    for (int i = 0; i < n; i++) {
        if (!block_geometry(ws[i], hs[i])) return -1;
        F[i].make(ys[i], us[i], vs[i], ws[i], hs[i], layout, rgb12s[i], 0xc0de + (u32)i);
        B.j[i] = F[i].job(layout);
    }
    u32 grid = (u32)waves;
    const u32 bands = cv_plan(B, n);
    if (grid < (bands < 8u ? bands : 8u)) grid = bands < 8u ? bands : 8u;  // (as smr_frames_to_rgba_batch does: every XCD that owns a band runs a workgroup)
    for (u32 blk = 0; blk < grid; blk++)
        for (u32 wv = 0; wv < 4; wv++)
            for (u32 lane = 0; lane < 64; lane++) {
                if (layout == CV422_V210) cv422_share<CV422_V210>(B, blk, wv, grid, lane, T.ylut, T.ulut);
                else if (layout == CV422_P210) cv422_share<CV422_P210>(B, blk, wv, grid, lane, T.ylut, T.ulut);
                else cv422_share<CV422_PLANAR>(B, blk, wv, grid, lane, T.ylut, T.ulut);
            }
    for (int i = 0; i < n; i++)
        if (int rc = F[i].finish(outs[i], 0xc0de + (u32)i)) return rc;
    return 0;
}

// The general v210 kernel's fetch (k_yuv422_hi_to_rgba_any): the codes of every pixel of a w x h frame, any width: out = (h, w, 3) u16 (Y, Cb, Cr)
extern "C" int emu_v210_pixel_codes(const u8 *plane, int w, int h, unsigned short *out) {
    if (w < 1 || h < 1) return -1;
    Plane p = make_plane(plane, 4 * ((w + 5) / 6), h, 4, v210_pitch(w), 0x5a, 4);
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            u32 yc, cb, cr;
            cv210_pixel_codes(p.view.ptr + (size_t)y * p.view.pitch, x, yc, cb, cr);
            unsigned short *o = out + ((size_t)y * w + x) * 3;
            o[0] = (unsigned short)yc; o[1] = (unsigned short)cb; o[2] = (unsigned short)cr;
        }
    return 0;
}
