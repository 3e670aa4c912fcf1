// TEST INFRASTRUCTURE — not part of the product; nothing in smelter_amd/ builds, links or loads this.
//
// The block converters' source per colour matrix (smr_color_matrix, include/smr.h), compiled for the CPU: cv420_run / cv420_share with the
// matrix as their trailing template argument (smr_convert_420.h: planar 4:2:0, NV12, J420), and cvhi_run / cvhi_share (smr_convert_hi.h),
// cv422_run / cv210_run / cv422_share (smr_convert_hi422.h) with the matrix in ConvJob::matrix.  tests/test_emu_convert_matrix.py holds them to
// tests/color_matrix_model.py byte for byte.  Same shims and guard plumbing as emu_convert.cpp / emu_convert_hi422.cpp.
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

// kinds: 0 planar 4:2:0 | 1 NV12 | 2 planar 4:2:0 10-bit | 3 P010 | 4 planar 4:2:2 10-bit | 5 P210 | 6 v210
enum { K_420 = 0, K_NV12, K_420P10, K_P010, K_422P10, K_P210, K_V210 };
bool kind_hi(int k) { return k >= K_420P10; }
bool kind_nv(int k) { return k == K_NV12 || k == K_P010 || k == K_P210; }
bool kind_422(int k) { return k >= K_422P10; }

struct Plane {
    GuardBuf buf;
    SurfView view;
};
// `w` texels of `bpp` bytes per row on `pitch`, `tail` spare bytes behind the last row, padding filled with a byte no plane contains by accident
Plane make_plane(const u8 *tight, int w, int h, int bpp, u32 pitch, size_t tail, u8 fill, size_t align) {
    Plane p;
    p.buf.alloc((size_t)pitch * h + tail, fill, align);
    for (int y = 0; y < h; y++) memcpy(p.buf.ptr + (size_t)y * pitch, tight + (size_t)y * w * bpp, (size_t)w * bpp);
    p.view.ptr = p.buf.ptr; p.view.pitch = pitch; p.view.w = w; p.view.h = h;
    return p;
}
// 8-bit chroma planes (emu_convert.cpp's rule): the allocator's 256-byte pitch and tail, or — emu_set_guard(.., 1) — the smallest pitch
// conv_route lets through: what the last block's window loads reach (plain build), the row's bytes rounded up to a dword (tight build)
u32 chroma_need(int w, int nv12) {
    const u32 cw = (u32)w / 2;
    return nv12 ? ((2u * (cw - 3u)) & ~3u) + 12u : ((cw - 3u) & ~3u) + 8u;
}
u32 pitch8(size_t row_bytes, u32 min_row, int tight) {
    if (!emu_min_pitch) return (u32)((row_bytes + 255) & ~(size_t)255);
    u32 pitch = (u32)((row_bytes + 3) & ~(size_t)3);
    if (pitch < min_row && !tight) pitch = (min_row + 3u) & ~3u;
    return pitch;
}
// 10-bit planes (emu_convert_hi422.cpp's rule): the row's own bytes, or wide rows (v210: a capture card's stride)
u32 pitch16(size_t row_bytes) { return emu_min_pitch ? (u32)row_bytes : (u32)((row_bytes + 255) & ~(size_t)255); }
u32 v210_pitch(int w) { return emu_min_pitch ? 16u * (u32)((w + 5) / 6) : (u32)((w + 47) / 48) * 128u; }
u32 node_pitch(int w, int rgb12) {
    if (emu_min_pitch) return emu_dst_pitch(rgb12 ? (u32)((3 * w + 15) & ~15) : (u32)w * 4);  // (guard mode 3: + 32 bytes of watched padding)
    return rgb12 ? (u32)((3 * w + 255) & ~255) : (u32)w * 4;
}
size_t node_row_bytes(int w, int rgb12) { return (size_t)w * (rgb12 ? 3 : 4); }

struct Tables {
    float ylut8[256], nlut8[256], ylut[CVHI_CODES], ulut[CVHI_CODES];
    Tables() {
        for (u32 b = 0; b < 256; b++) { ylut8[b] = cv420_luma_of_byte(b, false); nlut8[b] = unorm_of_byte(b); }
        cvhi_build_tables(ylut, ulut, 0u, 1u);
    }
};

struct Frame {
    Plane py, pu, pv;
    GuardBuf dst;
    u32 dpitch;
    int w, h, rgb12, kind;
    void make(const u8 *y, const u8 *u, const u8 *v, int w_, int h_, int kind_, int rgb12_, int tight, u32 seed) {
        w = w_; h = h_; rgb12 = rgb12_; kind = kind_;
        const int nv = kind_nv(kind), ch = kind_422(kind) ? h : h / 2;
        if (kind == K_V210) {
            py = make_plane(y, 4 * ((w + 5) / 6), h, 4, v210_pitch(w), 0, 0x5a, 8);
        } else if (kind_hi(kind)) {
            const int cbpp = nv ? 4 : 2;
            py = make_plane(y, w, h, 2, pitch16((size_t)w * 2), 0, 0x5a, 8);
            pu = make_plane(u, w / 2, ch, cbpp, pitch16((size_t)(w / 2) * cbpp), 0, 0xa5, 4);
            if (!nv) pv = make_plane(v, w / 2, ch, 2, pitch16((size_t)(w / 2) * 2), 0, 0x3c, 4);
        } else {
            const u32 need = chroma_need(w, nv);
            const size_t tail = emu_min_pitch || tight ? 0 : SMR_SURFACE_TAIL;  // (a plane the library owns may be read past a row's end: conv_route)
            py = make_plane(y, w, h, 1, pitch8((size_t)w, 0, tight), tail, 0x5a, 4);
            pu = make_plane(u, w / 2, ch, nv ? 2 : 1, pitch8((size_t)(w / 2) * (nv ? 2 : 1), need, tight), tail, 0xa5, 4);
            if (!nv) pv = make_plane(v, w / 2, ch, 1, pitch8((size_t)(w / 2), need, tight), tail, 0x3c, 4);
        }
        dpitch = node_pitch(w, rgb12);
        dst.alloc((size_t)dpitch * h, 0, 16);
        emu_pad_fill(dst.ptr, dpitch, h, seed);
    }
    ConvJob job(int full, int matrix) {
        ConvJob J;
        memset(&J, 0, sizeof(J));
        const int nv = kind_nv(kind);
        J.yp = py.view;
        J.up = kind == K_V210 ? py.view : pu.view;
        J.vp = kind == K_V210 || nv ? J.up : pv.view;
        J.dst.ptr = dst.ptr; J.dst.pitch = dpitch; J.dst.w = w; J.dst.h = h;
        J.full = full; J.nv = nv; J.sx = 1; J.sy = kind_422(kind) ? 0 : 1; J.packed = 0; J.rgb12 = rgb12;
        J.matrix = matrix;  // (read by the 10-bit converters; the 8-bit ones take the template argument)
        return J;
    }
    int finish(u8 *out, u32 seed) {
        if (int rc = emu_pad_check(dst.ptr, dpitch, node_row_bytes(w, rgb12), h, seed, rgb12 ? "RGB12 node" : "RGBA8 node")) return rc;
        const size_t row = node_row_bytes(w, rgb12);
        for (int r = 0; r < h; r++) memcpy(out + (size_t)r * row, dst.ptr + (size_t)r * dpitch, row);
        return 0;
    }
};

// cv420_run of one matrix: NV, RGB12, FULL, TIGHT as run-time flags
template <int M, bool TIGHT>
void run420(const ConvJob &J, int g, int P, int nb, const Tables &T) {
    const float *yl = J.full ? T.nlut8 : T.ylut8;
    if (J.nv) {
        if (J.rgb12) { if (J.full) cv420_run<true, true, true, TIGHT, M>(J, g, P, nb, yl, T.nlut8); else cv420_run<true, true, false, TIGHT, M>(J, g, P, nb, yl, T.nlut8); }
        else { if (J.full) cv420_run<true, false, true, TIGHT, M>(J, g, P, nb, yl, T.nlut8); else cv420_run<true, false, false, TIGHT, M>(J, g, P, nb, yl, T.nlut8); }
    } else {
        if (J.rgb12) { if (J.full) cv420_run<false, true, true, TIGHT, M>(J, g, P, nb, yl, T.nlut8); else cv420_run<false, true, false, TIGHT, M>(J, g, P, nb, yl, T.nlut8); }
        else { if (J.full) cv420_run<false, false, true, TIGHT, M>(J, g, P, nb, yl, T.nlut8); else cv420_run<false, false, false, TIGHT, M>(J, g, P, nb, yl, T.nlut8); }
    }
}
template <int M>
void share420(const ConvBatch &B, int nv, int tight, u32 blk, u32 wv, u32 grid, u32 lane, const Tables &T) {
    if (nv) { if (tight) cv420_share<true, true, M>(B, blk, wv, grid, lane, T.ylut8, T.nlut8); else cv420_share<true, false, M>(B, blk, wv, grid, lane, T.ylut8, T.nlut8); }
    else { if (tight) cv420_share<false, true, M>(B, blk, wv, grid, lane, T.ylut8, T.nlut8); else cv420_share<false, false, M>(B, blk, wv, grid, lane, T.ylut8, T.nlut8); }
}

void run_one(const ConvJob &J, int kind, int tight, int g, int P, int nb, const Tables &T) {
    const bool r12 = J.rgb12 != 0;
    switch (kind) {
    case K_420: case K_NV12:
        if (J.matrix == SMR_MATRIX_BT601) { if (tight) run420<SMR_MATRIX_BT601, true>(J, g, P, nb, T); else run420<SMR_MATRIX_BT601, false>(J, g, P, nb, T); }
        else if (J.matrix == SMR_MATRIX_BT2020_NCL) { if (tight) run420<SMR_MATRIX_BT2020_NCL, true>(J, g, P, nb, T); else run420<SMR_MATRIX_BT2020_NCL, false>(J, g, P, nb, T); }
        else { if (tight) run420<SMR_MATRIX_BT709, true>(J, g, P, nb, T); else run420<SMR_MATRIX_BT709, false>(J, g, P, nb, T); }
        break;
    case K_420P10: if (r12) cvhi_run<false, true>(J, g, P, nb, T.ylut, T.ulut); else cvhi_run<false, false>(J, g, P, nb, T.ylut, T.ulut); break;
    case K_P010: if (r12) cvhi_run<true, true>(J, g, P, nb, T.ylut, T.ulut); else cvhi_run<true, false>(J, g, P, nb, T.ylut, T.ulut); break;
    case K_422P10: if (r12) cv422_run<false, true>(J, g, P, nb, T.ylut, T.ulut); else cv422_run<false, false>(J, g, P, nb, T.ylut, T.ulut); break;
    case K_P210: if (r12) cv422_run<true, true>(J, g, P, nb, T.ylut, T.ulut); else cv422_run<true, false>(J, g, P, nb, T.ylut, T.ulut); break;
    default: if (r12) cv210_run<true>(J, g, P, nb, T.ylut, T.ulut); else cv210_run<false>(J, g, P, nb, T.ylut, T.ulut); break;
    }
}

bool args_ok(int w, int h, int kind, int matrix) { return w % 4 == 0 && w >= 8 && h % 2 == 0 && h >= 2 && kind >= 0 && kind <= K_V210 && matrix >= 0 && matrix < SMR_MATRIX_COUNT; }

}  // namespace

// Planes per kind as the frame holds them, tight (bytes, words or v210 dwords; NV12 / P010 / P210: u = the interleaved plane, v ignored; v210:
// y = the plane).  out: w x h x 4 tight; rgb12 != 0: h rows of 3 w bytes (12-byte groups of four pixels: R x 4, G x 4, B x 4).  Runs of nb >= 1
// block rows.  full / tight: kinds 0 and 1 only (J420; the _tight build).
extern "C" int emu_cm_run(const u8 *y, const u8 *u, const u8 *v, int w, int h, int kind, int full, int rgb12, int nb, int matrix, int tight, u8 *out) {
    if (!args_ok(w, h, kind, matrix) || nb < 1 || ((full || tight) && kind > K_NV12)) return -1;
    static const Tables T;
    Frame F;
    F.make(y, u, v, w, h, kind, rgb12, tight, 0xc0de);
    const ConvJob J = F.job(full, matrix);
    for (int P = 0; 4 * P < h; P += nb)
        for (int g = 0; 4 * g < w; g++) run_one(J, kind, tight, g, P, nb, T);
    return F.finish(out, 0xc0de);
}

// What a launch of the kind's kernel computes for matrix `matrix`: `n` frames partitioned the way the host does (cv_plan) over `waves`
// WORKGROUPS, every lane of every wave emulated in turn.  Pointers and ints per frame; output layout per frame as emu_cm_run.
extern "C" int emu_cm_shares(int n, const u8 *const *ys, const u8 *const *us, const u8 *const *vs, const int *ws, const int *hs, int kind, const int *fulls,
                             const int *rgb12s, int waves, int matrix, int tight, u8 *const *outs) {
    if (n < 1 || n > MAX_CONV_JOBS || waves < 1 || (tight && kind > K_NV12)) return -1;
    static const Tables T;
    std::vector<Frame> F(n);
    ConvBatch B;
    memset(&B, 0, sizeof(B));
    for (int i = 0; i < n; i++) {
        if (!args_ok(ws[i], hs[i], kind, matrix) || (fulls[i] && kind > K_NV12)) return -1;
        F[i].make(ys[i], us[i], vs[i], ws[i], hs[i], kind, rgb12s[i], tight, 0xc0de + (u32)i);
        B.j[i] = F[i].job(fulls[i], matrix);
    }
    u32 grid = (u32)waves;
    const u32 bands = cv_plan(B, n);
    if (grid < (bands < 8u ? bands : 8u)) grid = bands < 8u ? bands : 8u;  // (as smr_frames_to_rgba_batch does: every XCD that owns a band runs a workgroup)
    for (u32 blk = 0; blk < grid; blk++)
        for (u32 wv = 0; wv < 4; wv++)
            for (u32 lane = 0; lane < 64; lane++) switch (kind) {
                case K_420: case K_NV12:
                    if (matrix == SMR_MATRIX_BT601) share420<SMR_MATRIX_BT601>(B, kind == K_NV12, tight, blk, wv, grid, lane, T);
                    else if (matrix == SMR_MATRIX_BT2020_NCL) share420<SMR_MATRIX_BT2020_NCL>(B, kind == K_NV12, tight, blk, wv, grid, lane, T);
                    else share420<SMR_MATRIX_BT709>(B, kind == K_NV12, tight, blk, wv, grid, lane, T);
                    break;
                case K_420P10: cvhi_share<false>(B, blk, wv, grid, lane, T.ylut, T.ulut); break;
                case K_P010: cvhi_share<true>(B, blk, wv, grid, lane, T.ylut, T.ulut); break;
                case K_422P10: cv422_share<CV422_PLANAR>(B, blk, wv, grid, lane, T.ylut, T.ulut); break;
                case K_P210: cv422_share<CV422_P210>(B, blk, wv, grid, lane, T.ylut, T.ulut); break;
                default: cv422_share<CV422_V210>(B, blk, wv, grid, lane, T.ylut, T.ulut); break;
                }
    for (int i = 0; i < n; i++)
        if (int rc = F[i].finish(outs[i], 0xc0de + (u32)i)) return rc;
    return 0;
}

// The coefficient table as the kernels see it: 3 x 4 floats (rv, gu, gv, bu per matrix)
extern "C" void emu_cm_coefficients(float *out) {
    for (uint32_t m = 0; m < (uint32_t)SMR_MATRIX_COUNT; m++) {
        const SmrMatrixCoef C = smr_matrix_coef(m);
        out[4 * m] = C.rv; out[4 * m + 1] = C.gu; out[4 * m + 2] = C.gv; out[4 * m + 3] = C.bu;
    }
}
