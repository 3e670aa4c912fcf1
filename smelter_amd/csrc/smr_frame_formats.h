// smr_frame_formats.h — questions about smr_frame_format values that the device half (smr_internal.h includes this) and the host half
// (host/renderer.cpp, as "../smr_frame_formats.h") both ask, the split of smr_frame.format into base format and colour matrix, and the
// matrices' coefficient table — which the kernels, the host and the lane emulator (tests/emu) all take from here.  Plain C++ over smr.h: no HIP.
#pragma once

#include <cstdint>

#include "smr.h"

// smr_frame.format = base format (bits 0 - 7) | smr_color_matrix << 8 (bits 8 - 11): include/smr.h.  Every predicate below looks at the BASE
// format, so a tagged frame takes the route of its untagged twin; code that compares `format ==` against an enum value must split first
// (frame_base_format) — or means to decline tagged frames (the resamplers that convert inside the wave: they name the formats they take).
static inline uint32_t frame_base_format(uint32_t format) { return SMR_FRAME_BASE_FORMAT(format); }
static inline uint32_t frame_matrix(uint32_t format) { return SMR_FRAME_MATRIX(format); }

// The last three statements of yuv_to_rgb_store: r = y + rv * (v - .5); g = y - gu * (u - .5) - gv * (v - .5); b = y + bu * (u - .5).
// f32 literals at the reference's four decimals (BT.709: planar_yuv_to_rgba.wgsl:50-55; BT.601: Kr 0.299, Kb 0.114; BT.2020 NCL: Kr 0.2627,
// Kb 0.0593).  constexpr: a compile-time matrix gives the kernels literals, a run-time one three selects on a uniform value.
struct SmrMatrixCoef {
    float rv, gu, gv, bu;
};
constexpr int SMR_MATRIX_COUNT = 3;
constexpr SmrMatrixCoef smr_matrix_coef(uint32_t m) {
    return m == SMR_MATRIX_BT601 ? SmrMatrixCoef{1.4020f, 0.3441f, 0.7141f, 1.7720f}
         : m == SMR_MATRIX_BT2020_NCL ? SmrMatrixCoef{1.4746f, 0.1646f, 0.5714f, 1.8814f}
                                      : SmrMatrixCoef{1.5748f, 0.1873f, 0.4681f, 1.8556f};
}

// 10-bit input frames — 4:2:0 (smr_convert_hi.h): 16-bit words; 4:2:2 (smr_convert_hi422.h): 16-bit words or v210 dwords —, limited range,
// input only
static inline bool frame_format_is_hi_depth(uint32_t format) {
    format = frame_base_format(format);
    return format == SMR_FRAME_P010 || format == SMR_FRAME_PLANAR_YUV420P10 || format == SMR_FRAME_PLANAR_YUV422P10 || format == SMR_FRAME_P210 ||
           format == SMR_FRAME_V210;
}
// the 4:2:2 ones among them
static inline bool frame_format_is_hi_depth_422(uint32_t format) {
    format = frame_base_format(format);
    return format == SMR_FRAME_PLANAR_YUV422P10 || format == SMR_FRAME_P210 || format == SMR_FRAME_V210;
}

// 8-bit packed 4:2:2, one RGBA8 plane of (w / 2) x h texels: an input of any width, an output of an even width only (include/smr.h) —
// what every output entry point says about the other widths
static inline bool frame_format_is_packed_422(uint32_t format) {
    format = frame_base_format(format);
    return format == SMR_FRAME_UYVY422 || format == SMR_FRAME_YUYV422;
}
#define SMR_PACKED_OUTPUT_WIDTH_MSG "a packed 4:2:2 output (UYVY / YUYV) needs an even width: a texel holds two pixels"

// "this frame format is opaque Y'CbCr": every texel of its node texture has alpha 1 (planar_yuv_to_rgba.wgsl:57) — what the opaque routes
// (RGB12 nodes, tiles without alpha, opaque layers) ask.  The formats by name: a new enum value is not opaque until it is listed here.
static inline bool frame_format_is_opaque_ycbcr(uint32_t format) {
    switch (frame_base_format(format)) {
    case SMR_FRAME_PLANAR_YUV420: case SMR_FRAME_PLANAR_YUV422: case SMR_FRAME_PLANAR_YUV444: case SMR_FRAME_PLANAR_YUVJ420:
    case SMR_FRAME_UYVY422: case SMR_FRAME_YUYV422: case SMR_FRAME_NV12:
    case SMR_FRAME_P010: case SMR_FRAME_PLANAR_YUV420P10:
    case SMR_FRAME_PLANAR_YUV422P10: case SMR_FRAME_P210: case SMR_FRAME_V210:
        return true;
    default: return false;
    }
}

// What is wrong with the tag of a `format` value, or nullptr: a bit above bit 11, a matrix value the library does not know, a non-zero matrix
// on a format that has no matrix (BGRA / ARGB / RGBA).  An unknown BASE format is the caller's next question (plane_geometry, smr_ctx.hip).
static inline const char *frame_format_tag_error(uint32_t format) {
    if (format & ~0xfffu) return "bits above bit 11 are set (the format is bits 0 - 7, the colour matrix bits 8 - 11)";
    if (frame_matrix(format) >= (uint32_t)SMR_MATRIX_COUNT) return "colour matrix values 3 .. 15 are not defined (0 BT.709, 1 BT.601, 2 BT.2020 NCL)";
    if (frame_matrix(format) != 0 && !frame_format_is_opaque_ycbcr(format)) return "a colour matrix applies to Y'CbCr formats only (BGRA / ARGB / RGBA carry none)";
    return nullptr;
}
