// smr_convert_route.h — which kernel converts an input frame into its node texture: the one classifier smr_frames_to_rgba_batch queues by,
// validates RGB12 nodes with and smr_conv_rgb12_ok answers from.  Host code over smr_internal.h, no kernels: tests/emu/emu_convert_route.cpp
// compiles it for the CPU and tests/test_convert_route.py pins it on frames described by numbers.
#pragma once

#include "smr_internal.h"

// A route names the kernel; where the kernel carries the colour matrix as a template parameter (k_yuv420_to_rgba[_tight]) it names the matrix
// too.  The order is the order queued launches are made in at the end of a batch.
enum ConvRoute : int {
    CONV_GENERAL = -1,  // one launch per frame, any geometry (smr_frame_to_rgba_general)
    CONV_BATCH_4X2,     // k_yuv_to_rgba_batch: planar 4:2:0 / 4:2:2 / 4:4:4, NV12, UYVY / YUYV, BGRA / ARGB; reads the matrix from the job
    CONV_420_PLANAR, CONV_420_NV12, CONV_420_PLANAR_TIGHT, CONV_420_NV12_TIGHT,  // k_yuv420_to_rgba / _tight, BT.709
    CONV_HI420_PLANAR, CONV_HI420_P010,                                         // k_yuv420_hi_to_rgba (the matrix from the job)
    CONV_HI422_PLANAR, CONV_HI422_P210, CONV_HI422_V210,                        // k_yuv422_hi_to_rgba (the matrix from the job)
    CONV_420_PLANAR_601, CONV_420_NV12_601, CONV_420_PLANAR_TIGHT_601, CONV_420_NV12_TIGHT_601,      // k_yuv420_to_rgba / _tight, BT.601
    CONV_420_PLANAR_2020, CONV_420_NV12_2020, CONV_420_PLANAR_TIGHT_2020, CONV_420_NV12_TIGHT_2020,  // ... BT.2020 NCL
    CONV_ROUTES
};
// the 4 x 4 block converters (smr_convert_420.h, smr_convert_hi.h, smr_convert_hi422.h): what an RGB12 node needs
static inline bool conv_route_is_block(ConvRoute r) { return r > CONV_BATCH_4X2; }

// The block converters' geometry: width a multiple of 4 from 8, even height from 2, both within the size the coordinate argument holds for
static inline bool conv_block_geometry(const smr_frame *in) {
    return in->width % 4 == 0 && in->width >= 8 && in->height % 2 == 0 && in->height >= 2 && in->width <= 16384 && in->height <= 16384;
}
// A plane a block converter loads `a` bytes at a time from: pointer and pitch aligned to a, rows of at least row_bytes
static inline bool conv_plane_ok(const smr_surface *s, uintptr_t a, size_t row_bytes) {
    return s && (s->pitch & (a - 1)) == 0 && (((uintptr_t)s->ptr) & (a - 1)) == 0 && s->pitch >= row_bytes;
}

// k_yuv_to_rgba_batch's frames: planar 4:2:0 / 4:2:2 / 4:4:4 and NV12 whose subsampled axes are even (chroma planes exactly half), within the
// size the coordinate argument holds for
static inline bool conv_batchable(const smr_ctx *ctx, const smr_frame *in) {
    const u32 fmt = frame_base_format(in->format);  // (the colour matrix changes no route)
    if (in->width < 2 || in->height < 2 || in->width > 16384 || in->height > 16384 || ctx->convert_impl == SMR_CONVERT_GENERAL) return false;
    if (fmt == SMR_FRAME_UYVY422 || fmt == SMR_FRAME_YUYV422)
        return in->width % 2 == 0 && in->width >= 8 && in->planes[0] && (in->planes[0]->pitch & 3u) == 0 && (((uintptr_t)in->planes[0]->ptr) & 3) == 0;
    if (fmt == SMR_FRAME_BGRA || fmt == SMR_FRAME_ARGB)
        return in->planes[0] && (in->planes[0]->pitch & 15u) == 0 && (((uintptr_t)in->planes[0]->ptr) & 15) == 0;
    const bool nv = fmt == SMR_FRAME_NV12;
    const bool sx = fmt != SMR_FRAME_PLANAR_YUV444, sy = fmt == SMR_FRAME_PLANAR_YUV420 || fmt == SMR_FRAME_PLANAR_YUVJ420 || nv;
    if (fmt > SMR_FRAME_PLANAR_YUVJ420 && !nv) return false;  // (RGBA: a pass of its own; the 10-bit formats: the general kernels)
    if ((sx && in->width % 2) || (sy && in->height % 2)) return false;
    return in->planes[0] && in->planes[1] && (nv || in->planes[2]);
}

// The route of frame `in` into a node whose rows take 16-byte stores (`node16`: the node's pointer and pitch are 16-byte aligned, or it is an
// RGB12 node).  The colour matrix changes no route but the 8-bit block kernels' instantiation.
static inline ConvRoute conv_route(const smr_ctx *ctx, const smr_frame *in, bool node16) {
    const u32 fmt = frame_base_format(in->format), m = frame_matrix(in->format);
    const smr_surface *const *p = in->planes;
    const size_t w = in->width;
    if (!node16) return CONV_GENERAL;  // (the block kernels and the 4 x 2 one store 16 bytes)
    if (ctx->convert_impl == SMR_CONVERT_AUTO && conv_block_geometry(in)) {
        switch (fmt) {
        // 10-bit (smr_convert_hi.h, smr_convert_hi422.h).  A luma row of a block is one 8-byte load at 8 g, a v210 row of a block two 8-byte loads
        // at 32 (g / 3) + 8 (g % 3): the Y plane's (v210: the plane's) pointer and pitch are 8-byte aligned; the chroma loads are dwords:
        // dword-aligned; a chroma row is w / 2 columns of 2 (interleaved: 4) bytes.  Nothing else: the kernels request no byte outside a row's own
        // bytes, so owned and wrapped planes, wide and tight rows (a capture card's stride among them) are one case.
        case SMR_FRAME_PLANAR_YUV420P10: if (conv_plane_ok(p[0], 8, 2 * w) && conv_plane_ok(p[1], 4, w) && conv_plane_ok(p[2], 4, w)) return CONV_HI420_PLANAR; break;
        case SMR_FRAME_P010: if (conv_plane_ok(p[0], 8, 2 * w) && conv_plane_ok(p[1], 4, 2 * w)) return CONV_HI420_P010; break;
        case SMR_FRAME_PLANAR_YUV422P10: if (conv_plane_ok(p[0], 8, 2 * w) && conv_plane_ok(p[1], 4, w) && conv_plane_ok(p[2], 4, w)) return CONV_HI422_PLANAR; break;
        case SMR_FRAME_P210: if (conv_plane_ok(p[0], 8, 2 * w) && conv_plane_ok(p[1], 4, 2 * w)) return CONV_HI422_P210; break;
        case SMR_FRAME_V210: if (conv_plane_ok(p[0], 8, 16 * ((w + 5) / 6))) return CONV_HI422_V210; break;
        // 8-bit 4:2:0 (smr_convert_420.h): every plane dword-aligned.  The plain kernel reads up to a dword past the last block's window; the bytes
        // of that dword are never used (the window's last column is the plane's edge, repeated), but they are read: a plane the library allocated
        // may be read past a row's end — the next row, or the 16 bytes every allocation ends with (SMR_SURFACE_TAIL) — a wrapped one is read
        // inside its rows' bytes only: it takes k_yuv420_to_rgba_tight, which requests nothing behind a window's last column.
        // (a wrapped plane with a wide pitch still ends with its last ROW for many producers — pitch * (h - 1) + row bytes, not pitch * h — and the
        //  plain kernel's reach into that row's padding would leave the allocation: every plane the library does not own takes the tight kernel, + 2 %)
        case SMR_FRAME_PLANAR_YUV420:
        case SMR_FRAME_PLANAR_YUVJ420:
        case SMR_FRAME_NV12: {
            const bool nv = fmt == SMR_FRAME_NV12;
            if (!conv_plane_ok(p[0], 4, w) || !conv_plane_ok(p[1], 4, nv ? w : w / 2) || (!nv && !conv_plane_ok(p[2], 4, w / 2))) break;
            const bool tight = !(p[1]->owned && (nv || p[2]->owned));
            static const ConvRoute r[SMR_MATRIX_COUNT][2][2] = {  // [matrix][NV12][tight]
                {{CONV_420_PLANAR, CONV_420_PLANAR_TIGHT}, {CONV_420_NV12, CONV_420_NV12_TIGHT}},
                {{CONV_420_PLANAR_601, CONV_420_PLANAR_TIGHT_601}, {CONV_420_NV12_601, CONV_420_NV12_TIGHT_601}},
                {{CONV_420_PLANAR_2020, CONV_420_PLANAR_TIGHT_2020}, {CONV_420_NV12_2020, CONV_420_NV12_TIGHT_2020}}};
            return r[m < (u32)SMR_MATRIX_COUNT ? m : 0][nv][tight];  // (smr_validate_frame refuses other matrix values)
        }
        default: break;
        }
    }
    return conv_batchable(ctx, in) ? CONV_BATCH_4X2 : CONV_GENERAL;
}

// smr_conv_rgb12_ok: may this frame's node texture be RGB12 (12-byte groups of four pixels)?  A frame a block converter takes, rows of at most
// 15364 bytes
static inline bool conv_rgb12_ok(const smr_ctx *ctx, const smr_frame *in) {
    return in && conv_route_is_block(conv_route(ctx, in, true)) && 3u * in->width <= 7682u * 2u;
}
