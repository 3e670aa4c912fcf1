// smr_frame_formats.h — questions about smr_frame_format values that the device half (smr_internal.h includes this) and the host half
// (host/renderer.cpp, as "../smr_frame_formats.h") both ask.  Plain C++ over smr.h: no HIP.
#pragma once

#include <cstdint>

#include "smr.h"

// 10-bit input frames — 4:2:0 (smr_convert_hi.h): 16-bit words; 4:2:2 (smr_convert_hi422.h): 16-bit words or v210 dwords —, limited range,
// input only
static inline bool frame_format_is_hi_depth(uint32_t format) {
    return format == SMR_FRAME_P010 || format == SMR_FRAME_PLANAR_YUV420P10 || format == SMR_FRAME_PLANAR_YUV422P10 || format == SMR_FRAME_P210 ||
           format == SMR_FRAME_V210;
}
// the 4:2:2 ones among them
static inline bool frame_format_is_hi_depth_422(uint32_t format) {
    return format == SMR_FRAME_PLANAR_YUV422P10 || format == SMR_FRAME_P210 || format == SMR_FRAME_V210;
}

// "this frame format is opaque Y'CbCr": every texel of its node texture has alpha 1 (planar_yuv_to_rgba.wgsl:57) — what the opaque routes
// (RGB12 nodes, tiles without alpha, opaque layers) ask.  The formats by name: a new enum value is not opaque until it is listed here.
static inline bool frame_format_is_opaque_ycbcr(uint32_t format) {
    switch (format) {
    case SMR_FRAME_PLANAR_YUV420: case SMR_FRAME_PLANAR_YUV422: case SMR_FRAME_PLANAR_YUV444: case SMR_FRAME_PLANAR_YUVJ420:
    case SMR_FRAME_UYVY422: case SMR_FRAME_YUYV422: case SMR_FRAME_NV12:
    case SMR_FRAME_P010: case SMR_FRAME_PLANAR_YUV420P10:
    case SMR_FRAME_PLANAR_YUV422P10: case SMR_FRAME_P210: case SMR_FRAME_V210:
        return true;
    default: return false;
    }
}
