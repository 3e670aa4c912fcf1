// TEST INFRASTRUCTURE — not part of the product; nothing in smelter_amd/ builds, links or loads this.
//
// The 10-bit 4:2:0 input converter's source (smelter_amd/csrc/smr_convert_hi.h: cvhi_run, a vertical run of 4 x 4 pixel blocks per call; cvhi_share,
// a wave's share of a launch; sample_plane_bilinear_hi, the general kernel's sampler) compiled for the CPU, so that tests/test_emu_convert_hi.py
// can hold it to the oracle and to tests/hi_depth_model.py byte for byte without a GPU.  Same shims as emu_convert.cpp.
#include <vector>

#include <hip/hip_runtime.h>

thread_local dim3 threadIdx, blockIdx;
dim3 gridDim, blockDim;

#include "emu_device.h"
#include "emu_guard.h"
EmuBlock *emu_blk = nullptr;
thread_local unsigned char *emu_smem = nullptr;
void __syncthreads() {}

#include "smr_convert_hi.h"

namespace {

struct Plane {
    GuardBuf buf;
    SurfView view;
};
// `w` texels of `bpp` bytes per row.  Rows on a 256-byte pitch like smr_surface_create's, padding filled with a byte no plane contains by
// accident; with emu_set_guard(.., 1) on the smallest pitch conv_route (smr_convert.hip) lets through — the row's own bytes (a multiple of 8
// for luma, of 4 for chroma at the widths the block converter takes) — and the buffer exactly pitch * h bytes: ONE memory contract.
Plane make_plane(const u8 *tight, int w, int h, int bpp, u8 fill, size_t align) {
    Plane p;
    const u32 pitch = emu_min_pitch ? (u32)((size_t)w * bpp) : (u32)(((size_t)w * bpp + 255) & ~(size_t)255);
    p.buf.alloc((size_t)pitch * h, fill, align);
    for (int y = 0; y < h; y++) memcpy(p.buf.ptr + (size_t)y * pitch, tight + (size_t)y * w * bpp, (size_t)w * bpp);
    p.view.ptr = p.buf.ptr; p.view.pitch = pitch; p.view.w = w; p.view.h = h;
    return p;
}
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
    ConvJob job(int p010) {
        ConvJob J;
        memset(&J, 0, sizeof(J));
        J.yp = py.view; J.up = pu.view; J.vp = p010 ? pu.view : pv.view;
        J.dst.ptr = dst.ptr; J.dst.pitch = dpitch; J.dst.w = w; J.dst.h = h;
        J.full = 0; J.nv = p010; J.sx = 1; J.sy = 1; J.packed = 0; J.rgb12 = rgb12;
        return J;
    }
    void make(const u8 *y, const u8 *u, const u8 *v, int w_, int h_, int p010, int rgb12_, u32 seed) {
        w = w_; h = h_; rgb12 = rgb12_;
        py = make_plane(y, w, h, 2, 0x5a, 8);
        pu = make_plane(u, w / 2, h / 2, p010 ? 4 : 2, 0xa5, 4);
        if (!p010) pv = make_plane(v, w / 2, h / 2, 2, 0x3c, 4);
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

}  // namespace

// y: w x h words; planar: u, v: (w / 2) x (h / 2) words; P010: u = interleaved (w / 2) x (h / 2) x 2 words, v ignored.  out: w x h x 4 tight;
// rgb12 != 0: out = h rows of 3 w bytes (12-byte groups of four pixels: R x 4, G x 4, B x 4).  cvhi_run over runs of nb >= 1 block rows.
extern "C" int emu_convert_hi_run(const u8 *y, const u8 *u, const u8 *v, int w, int h, int p010, int rgb12, int nb, u8 *out) {
    if (w % 4 || w < 8 || h % 2 || h < 2 || nb < 1) return -1;
    static const Tables T;
    Frame F;
    F.make(y, u, v, w, h, p010, rgb12, 0xc0de);
    const ConvJob J = F.job(p010);
    for (int P = 0; 4 * P < h; P += nb)
        for (int g = 0; 4 * g < w; g++) {
            if (p010 && rgb12) cvhi_run<true, true>(J, g, P, nb, T.ylut, T.ulut);
            else if (p010) cvhi_run<true, false>(J, g, P, nb, T.ylut, T.ulut);
            else if (rgb12) cvhi_run<false, true>(J, g, P, nb, T.ylut, T.ulut);
            else cvhi_run<false, false>(J, g, P, nb, T.ylut, T.ulut);
        }
    return F.finish(out, 0xc0de);
}

// What a launch of k_yuv420_hi_to_rgba computes: `n` frames of one format partitioned the way the host does (cv_plan) over `waves`
// WORKGROUPS, every lane of every wave emulated in turn.  Pointers and ints per frame; output layout per frame as emu_convert_hi_run.
extern "C" int emu_convert_hi_shares(int n, const u8 *const *ys, const u8 *const *us, const u8 *const *vs, const int *ws, const int *hs, int p010,
                                     const int *rgb12s, int waves, u8 *const *outs) {
    if (n < 1 || n > MAX_CONV_JOBS || waves < 1) return -1;
    static const Tables T;
    std::vector<Frame> F(n);
    ConvBatch B;
    memset(&B, 0, sizeof(B));
    for (int i = 0; i < n; i++) {
        if (ws[i] % 4 || ws[i] < 8 || hs[i] % 2 || hs[i] < 2) return -1;
        F[i].make(ys[i], us[i], vs[i], ws[i], hs[i], p010, rgb12s[i], 0xc0de + (u32)i);
        B.j[i] = F[i].job(p010);
    }
    u32 grid = (u32)waves;
    const u32 bands = cv_plan(B, n);
    if (grid < (bands < 8u ? bands : 8u)) grid = bands < 8u ? bands : 8u;  // (as smr_frames_to_rgba_batch does: every XCD that owns a band runs a workgroup)
    for (u32 blk = 0; blk < grid; blk++)
        for (u32 wv = 0; wv < 4; wv++)
            for (u32 lane = 0; lane < 64; lane++) {
                if (p010) cvhi_share<true>(B, blk, wv, grid, lane, T.ylut, T.ulut);
                else cvhi_share<false>(B, blk, wv, grid, lane, T.ylut, T.ulut);
            }
    for (int i = 0; i < n; i++)
        if (int rc = F[i].finish(outs[i], 0xc0de + (u32)i)) return rc;
    return 0;
}

// The tables as the kernels build them (the code's luma range expansion, its unorm value): 2 x 1024 floats
extern "C" void emu_convert_hi_tables(float *ylut, float *ulut) {
    static const Tables T;
    memcpy(ylut, T.ylut, sizeof(T.ylut));
    memcpy(ulut, T.ulut, sizeof(T.ulut));
}
