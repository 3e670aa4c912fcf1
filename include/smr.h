/*
 * smr.h — C ABI of libsmr_hip: the MI355X (gfx950) scene rasteriser that replaces the
 * wgpu back half of smelter-render (everything below scene/flatten).
 *
 * What binds to it: smelter-render's InputTexture / ResampledChild / LayoutShader /
 * OutputTexture / FramePreProcessor (see INTEGRATION.md for the Rust `extern "C"`
 * block a maintainer adds).  Each entry point names the reference interface it
 * replaces (paths relative to the smelter repository root).
 *
 * Conventions
 *   - every function returns 0 (SMR_OK) or a negative smr_status; the message is
 *     available from smr_last_error(ctx) (ctx-owned, valid until the next call).
 *     Error classes mirror smelter-render/src/wgpu.rs:78-97 WgpuError::{Validation,
 *     OutOfMemory, Internal}.
 *   - no global state, no callbacks.  A ctx may be used from any thread but calls must
 *     be externally serialised (smelter-render already holds one Mutex around the
 *     renderer: smelter-render/src/state.rs:55).
 *   - all work is enqueued on the ctx stream; only *_download, smr_sync and
 *     smr_timer_stop block the host.
 *   - surfaces live in HBM as pitched 2-D arrays (pitch is a multiple of 256 B);
 *     host buffers handed to upload/download are tightly packed unless a pitch is
 *     given (reference: wgpu/texture/base.rs:61-77, output_texture.rs:105-108).
 *   - RGBA8 node surfaces hold premultiplied alpha.  In SMR_MODE_GPU_OPTIMIZED their
 *     bytes are sRGB-encoded and every filter / blend happens in linear light
 *     (Rgba8UnormSrgb + two views: wgpu/texture/rgba_multiview.rs:17-49,
 *     state/node_texture.rs:104-142); in SMR_MODE_CPU_OPTIMIZED they are plain unorm.
 */
#ifndef SMR_H
#define SMR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SMR_API __attribute__((visibility("default")))

typedef struct smr_ctx smr_ctx;
typedef struct smr_surface smr_surface;

typedef enum smr_status {
    SMR_OK = 0,
    SMR_ERR_INVALID = -1,  /* WgpuError::Validation  */
    SMR_ERR_OOM = -2,      /* WgpuError::OutOfMemory */
    SMR_ERR_INTERNAL = -3, /* WgpuError::Internal    */
} smr_status;

/* smelter-render/src/types.rs:8-18 RenderingMode (WebGl is wasm-only: out of scope) */
typedef enum smr_mode { SMR_MODE_GPU_OPTIMIZED = 0, SMR_MODE_CPU_OPTIMIZED = 1 } smr_mode;

typedef enum smr_pixel_format {
    SMR_PX_RGBA8 = 0,   /* node texture (wgpu Rgba8UnormSrgb / Rgba8Unorm)          */
    SMR_PX_RGBA16F = 1, /* resampler intermediate (layout/resampler.rs:25-28)       */
    SMR_PX_R8 = 2,      /* Y / U / V plane (wgpu/texture/planar_yuv.rs:111-129)     */
    SMR_PX_RG8 = 3,     /* NV12 chroma plane (wgpu/texture/nv12.rs)                 */
    SMR_PX_R16 = 4,     /* one little-endian 16-bit word per texel: a 10-bit Y / U / V plane, the Y plane of P010 */
    SMR_PX_RG16 = 5,    /* two words per texel: the U V plane of P010                */
} smr_pixel_format;

/* smelter-render/src/types.rs:27-40 FrameData */
typedef enum smr_frame_format {
    SMR_FRAME_PLANAR_YUV420 = 0,
    SMR_FRAME_PLANAR_YUV422 = 1,
    SMR_FRAME_PLANAR_YUV444 = 2,
    SMR_FRAME_PLANAR_YUVJ420 = 3,
    /* 8-bit packed 4:2:2, one SMR_PX_RGBA8 plane of (w / 2) x h texels: a texel holds two pixels, U Y0 V Y1 (UYVY, the `2vuy` of SDI playout
     * cards) or Y0 U Y1 V (YUYV / YUY2, what V4L2 output and loopback devices, virtual cameras and most capture-style APIs take), in memory order.
     * As INPUTS: interleaved_{uyvy,yuyv}_to_rgba.wgsl, any width.
     * As OUTPUTS (smr_rgba_to_frame, smr_frame_fill_black, smr_render_layouts' `out`, a renderer's output_format; the reference's
     * OutputFrameFormat has no packed variant: a host opts in by passing the format): BT.709, limited range and 8-bit like every other
     * output, and nothing new numerically — for an even width the frame's bytes are an interleave of the planes SMR_FRAME_PLANAR_YUV422
     * output gives for the same node texture: texel j of row y holds U[y][j] Y[y][2j] V[y][j] Y[y][2j+1] (UYVY) or Y[y][2j] U[y][j]
     * Y[y][2j+1] V[y][j] (YUYV); Y is rgba_to_yuv.wgsl's luma of the pixel, U and V its chroma of the pair's horizontal mean
     * a * .5 + b * .5, each channel byte / 255 first; range compression and the unorm8 store unchanged.
     *   width   even and at least 2 (a packed 4:2:2 raster has no odd width): an odd-width OUTPUT frame is SMR_ERR_INVALID at every output
     *           entry point ("... needs an even width"), refused before anything is launched; for the renderer the previous scene stays
     *           active.  Input frames of odd width keep working as they do.
     *   height  any, from 1.
     *   black   smr_frame_fill_black and an empty output give Y = 16, U = V = 128: texels 80 10 80 10 (UYVY) / 10 80 10 80 (YUYV).
     *   still refused, as for every output: a matrix tag, the 10-bit formats (v210 included), a bit above bit 11, a missing plane, a plane
     *           that is not SMR_PX_RGBA8 of (w / 2) x h.
     *   memory  smr_surface_wrap's write contract holds for a packed destination: every row gets its w * 2 bytes and no other byte is written;
     *           stores wider than a texel are used only where the plane's base and pitch allow them (8-byte alignment for the compositor's
     *           own store, otherwise the frame is composed as RGBA8 and converted in one more launch: the same bytes). */
    SMR_FRAME_UYVY422 = 4,
    SMR_FRAME_YUYV422 = 5,
    SMR_FRAME_NV12 = 6,
    SMR_FRAME_BGRA = 7,
    SMR_FRAME_ARGB = 8,
    SMR_FRAME_RGBA = 9, /* Rgba8UnormWgpuTexture: straight alpha, premultiplied on ingest */
    /* 10-bit 4:2:0, what HEVC Main10 / AV1 / VP9 profile 2 decoders hand over (no FrameData variant: the reference has no 10-bit path).
     * Limited range, opaque, INPUT ONLY: smr_rgba_to_frame, smr_frame_fill_black and a renderer's output_format refuse them.
     * A 10-bit code c is the 8-bit code c / 4 with two more fractional bits: its unorm value is (c * 0.25) / 255, and from there on the
     * conversion is planar_yuv_to_rgba.wgsl / nv12_to_rgba.wgsl unchanged (limited range 64 .. 940 is exactly 16 .. 235) — a frame whose
     * codes are 4 b has, byte for byte, the node texture of the 8-bit frame with bytes b.
     * Not offered: full-range 10-bit, 4:4:4 10-bit, Y210, 12-bit, 10-bit outputs, and these formats on the plane-source
     * route (SMR_OPT_PLANE_SOURCE) or the laboratory fused conversion — both keep rejecting the formats they do not name. */
    SMR_FRAME_P010 = 10,              /* {Y: R16 w x h, UV: RG16 w/2 x h/2}; code = word >> 6, the low six bits are ignored */
    SMR_FRAME_PLANAR_YUV420P10 = 11,  /* {Y, U, V}, all R16; code = word & 0x3ff, the high six bits are ignored */
    /* 10-bit 4:2:2, what SDI capture cards (v210) and ProRes 422 / DNxHR / XAVC / H.264 Hi422 decoders (yuv422p10le, P210) hand over.
     * Limited range, opaque, INPUT ONLY like the two above, and the same value rule: a code c has the unorm value (f32(c) * 0.25f) / 255.0f.
     * Planar 10-bit and P210 continue with planar_yuv_to_rgba.wgsl as it samples a 4:2:2 frame: chroma bilinear horizontally (weights
     * .75 / .25, clamp to edge), the texel itself vertically — codes 4 b give, byte for byte, the node texture of the 8-bit
     * SMR_FRAME_PLANAR_YUV422 frame with bytes b.
     * v210 continues with interleaved_uyvy_to_rgba.wgsl: pixel x takes luma Y[x] and the chroma of pair x / 2, no interpolation, then the
     * limited-range conversion — defined that way for every width, odd ones included; for even widths from 8 up codes 4 b give, byte for
     * byte, the node texture of the UYVY frame with bytes b.
     * v210 layout: a dword holds three codes, lo in bits 0-9, mid in bits 10-19, hi in bits 20-29; bits 30-31 are ignored.  Six pixels are
     * four dwords, Cb(j) / Cr(j) belonging to the group's pixel pair j:
     *      d0 = Cb(0) Y0 Cr(0) | d1 = Y1 Cb(1) Y2 | d2 = Cr(1) Y3 Cb(2) | d3 = Y4 Cr(2) Y5          (lo mid hi)
     * The last group may be partly filled: components of pixels at or beyond the width are ignored, but the group's 16 bytes are part of
     * the row (nothing past the row is read).  A capture card's row stride, ((w + 47) / 48) * 128 bytes, is the pitch of a wrapped plane. */
    SMR_FRAME_PLANAR_YUV422P10 = 12,  /* {Y: R16 w x h, U, V: R16 w/2 x h}: SMR_FRAME_PLANAR_YUV422's geometry; code = word & 0x3ff */
    SMR_FRAME_P210 = 13,              /* {Y: R16 w x h, UV: RG16 w/2 x h}; code = word >> 6 */
    SMR_FRAME_V210 = 14,              /* one SMR_PX_RGBA8 plane of 4 * ceil(w / 6) texels x h: a texel is one little-endian dword */
} smr_frame_format;

/* The Y'CbCr matrix of an INPUT frame.  It travels in bits 8 - 11 of smr_frame.format (and of smr_frame_create's `format`); matrix 0 is
 * the value every format had before, so SMR_FRAME_WITH_MATRIX(f, SMR_MATRIX_BT709) == f and nothing that exists changes meaning.
 * Accepted on the twelve opaque Y'CbCr formats (every format above but BGRA / ARGB / RGBA).  Refused with SMR_ERR_INVALID: a matrix
 * value of 3 .. 15, any bit above bit 11, a non-zero matrix on BGRA / ARGB / RGBA, and a non-zero matrix wherever a frame is an OUTPUT
 * (smr_rgba_to_frame, smr_frame_fill_black, a renderer's output_format).
 * The value rule: everything up to and including the range step is the format's own — the texel fetch, the 8-bit sub-texel bilinear chroma
 * sample (the packed formats' snapped fetch), the 10-bit code rule (c * 0.25) / 255, the limited-range division and clamp (none for
 * YUVJ420).  The last three statements of planar_yuv_to_rgba.wgsl take their four constants from the matrix, each operation rounded to f32:
 *      r = y + c_rv * (v - 0.5)
 *      g = y - c_gu * (u - 0.5) - c_gv * (v - 0.5)          (left to right)
 *      b = y + c_bu * (u - 0.5)
 * with f32 literals at the reference's four decimals:
 *      matrix                               c_rv    c_gu    c_gv    c_bu
 *      BT.709 (the reference)               1.5748  0.1873  0.4681  1.8556
 *      BT.601 (Kr 0.299, Kb 0.114)          1.4020  0.3441  0.7141  1.7720
 *      BT.2020 NCL (Kr 0.2627, Kb 0.0593)   1.4746  0.1646  0.5714  1.8814
 * and the unorm8 store floor(clamp(x) * 255 + 0.5) unchanged.  The node texture and everything behind it are as before.
 * Not offered: matrices on outputs (outputs stay BT.709); range overrides (full-range NV12 / 4:2:2 / 4:4:4 / 10-bit, limited J420: range
 * stays what each format defines); BT.2020 constant luminance; transfer functions and primaries (the node stays the gamma-encoded R'G'B'
 * the reference treats as sRGB: no PQ / HLG, no gamut mapping); the matrix inside the plane-source route (SMR_OPT_PLANE_SOURCE), the f32
 * k_ingest route and the laboratory fused conversion, which decline tagged frames — those then take the node route, the same bytes. */
typedef enum smr_color_matrix { SMR_MATRIX_BT709 = 0, SMR_MATRIX_BT601 = 1, SMR_MATRIX_BT2020_NCL = 2 } smr_color_matrix;
#define SMR_FRAME_WITH_MATRIX(format, m) ((uint32_t)(format) | ((uint32_t)(m) << 8))
#define SMR_FRAME_BASE_FORMAT(format)    ((uint32_t)(format) & 0xffu)
#define SMR_FRAME_MATRIX(format)         (((uint32_t)(format) >> 8) & 0xfu)

/* One video frame resident in HBM: up to three pitched plane surfaces.
 * planes[] per format: planar YUV {Y,U,V}; NV12 {Y (R8), UV (RG8)}; P010 / P210 {Y (R16), UV (RG16)}; planar 10-bit {Y,U,V} (R16); packed formats {data}.
 * UYVY/YUYV planes are RGBA8 surfaces of width/2 texels (wgpu/texture/interleaved_yuv422.rs); a v210 plane is an RGBA8 surface of
 * 4 * ceil(width / 6) texels. */
typedef struct smr_frame {
    uint32_t format; /* smr_frame_format, for an input frame optionally | smr_color_matrix << 8 (SMR_FRAME_WITH_MATRIX) */
    uint32_t width;
    uint32_t height;
    smr_surface *planes[3];
} smr_frame;

typedef struct smr_surface_info {
    uint32_t width, height, format;
    uint32_t owned; /* 0 when wrapped around caller memory */
    size_t pitch;   /* bytes per row */
    void *dptr;     /* device pointer */
} smr_surface_info;

#define SMR_MAX_MASKS 20            /* layout/params.rs:15 */
#define SMR_DEFAULT_MAX_LAYOUTS 100 /* layout.rs:23 */
#define SMR_NO_SOURCE 0xffffffffu

/* layout/layout.rs:47-55 Mask + params.rs:292-300 byte order */
typedef struct smr_mask {
    float radius[4]; /* top_left, top_right, bottom_right, bottom_left */
    float top, left, width, height;
} smr_mask;

/* POD mirror of RenderLayout (layout.rs:58-96) in the conventions of
 * ParamsBindGroups::update (layout/params.rs:169-334): colours are premultiplied
 * and already mode-converted by the host (wgpu/utils.rs:51-81). */
typedef struct smr_layout {
    float top, left, width, height;
    float rotation_degrees;
    float border_radius[4]; /* tl, tr, br, bl */
    uint32_t type;          /* 0 texture (ChildNode), 1 colour, 2 box shadow */
    uint32_t source_index;  /* texture: index into sources[]; SMR_NO_SOURCE = empty 1x1 */
    float color[4];
    float border_color[4];
    float border_width;
    float crop[4]; /* top, left, width, height (layout.rs:39-45) */
    float blur_radius;
    uint32_t masks_len;
    smr_mask masks[SMR_MAX_MASKS];
} smr_layout;

/* Resampler pass plan (layout/resampler.rs:36-145, 305-378) */
typedef struct smr_resample_plan {
    int32_t kind;      /* 0 direct (layout shader samples the source 1:1), 1 single pass, 2 separable */
    int32_t levels[2]; /* box pre-decimation levels [horizontal, vertical] */
    int32_t reduced_w, reduced_h;
    int32_t axis[2]; /* per pass, in execution order: 0 horizontal, 1 vertical */
    float scale[2];
    float offset[2];
    int32_t perp_offset[2];
    int32_t mid_w, mid_h; /* separable: f16 intermediate size */
} smr_resample_plan;

/* One glyph quad of a text node (transformations/text_renderer.rs:92-132). */
typedef struct smr_glyph {
    int32_t dst_x, dst_y;
    int32_t w, h;
    int32_t atlas_x, atlas_y;
    float color[4]; /* straight RGBA 0..1, gamma-encoded */
} smr_glyph;

/* Source of a texture layout for the fused render entry point. */
typedef enum smr_source_kind {
    SMR_SOURCE_NONE = 0,
    SMR_SOURCE_SURFACE = 1,
    SMR_SOURCE_FRAME = 2,
    SMR_SOURCE_OPAQUE_SURFACE = 3 /* an RGBA8 surface the caller knows to be alpha == 255 everywhere (e.g. a tile produced by
                                     smr_ingest_resample on another GPU): lets the compositor treat it as a base layer */
} smr_source_kind;
typedef struct smr_source {
    uint32_t kind;
    const smr_surface *surface; /* RGBA8 node surface (text, image, shader output, ...) */
    const smr_frame *frame;     /* raw input frame: colour conversion is fused into the resampler */
} smr_source;

/* ---- context ---------------------------------------------------------------------
 * replaces WgpuCtx::new (smelter-render/src/wgpu/ctx.rs:34-107) + RendererOptions
 * {rendering_mode, max_layouts_count} (state.rs:43-52).
 * hip_stream: an existing hipStream_t to enqueue on, or NULL to let the ctx create one. */
SMR_API int smr_ctx_create(int hip_device, uint32_t mode, uint32_t max_layouts, void *hip_stream, smr_ctx **out);
SMR_API void smr_ctx_destroy(smr_ctx *ctx);
SMR_API const char *smr_last_error(const smr_ctx *ctx);
SMR_API uint32_t smr_ctx_mode(const smr_ctx *ctx);  /* smr_mode the context was created with (RenderingMode, types.rs:8-18) */
SMR_API int smr_sync(smr_ctx *ctx);                 /* device.poll(wait) — render_loop.rs:177-183 */
/* Context options (RendererOptions has no counterpart: these select between equivalent implementations).
 *   SMR_OPT_INGEST_IMPL         how wave A of smr_render_layouts / smr_ingest_resample* turns a Y'CbCr frame into its dst-sized tile:
 *       SMR_INGEST_AUTO      what the reference does, both halves fast (default): every frame goes through the exact converter
 *                            (k_yuv420_to_rgba / k_yuv_to_rgba_batch: the WGSL operation sequence value for value — the node texture's bytes
 *                            ARE the reference's, tests/test_emu_convert.py, tests/test_gpu_parity.py) into its RGBA8 node texture, one launch
 *                            for all frames of a call, and the matrix-core kernel (k_ingest_wave) resamples the nodes, one launch for all of
 *                            them; the general pass kernels where a plan leaves the kernel's windows (smr_debug_kernel_launches tells).
 *                            Within 1 LSB of the reference END TO END on every content class.
 *       SMR_INGEST_VALU_F32  exact f32 everywhere: bit-identical to the pass-per-launch kernels (smr_frame_to_rgba + smr_resample)
 *       SMR_INGEST_MFMA_F16, SMR_INGEST_MFMA_F16_NODE  aliases of AUTO (names of earlier revisions, kept for callers)
 *       (5, the conversion fused into the resampler with a folded-FMA BT.709 matrix — within one code per stage but not within 1 LSB end to end on
 *        adversarial content — is not part of the ABI any more: laboratory builds only, -DSMR_LAB)
 *       (3, round 2's workgroup-pipelined kernel k_ingest_mfma, was retired in round 4: smr_ctx_set_option rejects it)
 *     The matrix-core resampler keeps every quantisation point of the reference (u8 node texture, f16 between the passes,
 *     layout/resampler.rs:25-28, u8 sRGB tile); its operands are f16 pairs (texels and the weights of both passes), accumulated in f32: within
 *     1 LSB — on every byte of every content class — of resample.wgsl's passes applied to the node texture.
 *   SMR_OPT_INGEST_STRIP_WIDTH  strip width of the f32 kernel: 0 = chosen per job (default), 32 or 64 (tests, profiling)
 *   SMR_OPT_DIRECT_OUTPUT       1: when smr_render_layouts sees the same layout list again (a scene at rest), the pixels the
 *                               compositor would only copy from a freshly resampled input are converted to Y'CbCr by the resampling
 *                               kernel itself and their RGBA8 form is never stored (HBM traffic per frame 1.5x instead of 2.9x the
 *                               algorithmic bytes, at the price of vector-ALU time in a kernel that is instruction-bound: DESIGN.md); 0 (default): always through
 *                               the RGBA8 tile.  Same output bytes either way. */
typedef enum smr_ingest_impl {
    SMR_INGEST_AUTO = 0, SMR_INGEST_VALU_F32 = 1, SMR_INGEST_MFMA_F16 = 2, /* 3: retired */ SMR_INGEST_MFMA_F16_NODE = 4 /* 5: laboratory builds only */
} smr_ingest_impl;
/*   SMR_OPT_CONVERT_IMPL        which kernels smr_frame_to_rgba (InputTexture::convert_to_node_texture) runs — all of them produce the same bytes:
 *       SMR_CONVERT_AUTO       the block converters: k_yuv420_to_rgba (4:2:0 planar / NV12: a thread per 4 x 4 block, shared chroma work) and
 *                              k_yuv_to_rgba_batch (4:2:2, 4:4:4, packed YUV, BGRA / ARGB), the pass kernels for what those leave (default)
 *       SMR_CONVERT_GENERAL    one kernel per WGSL pass, one launch per frame, coordinates and divisions as the shader writes them (tests: the
 *                              block converters are held to these bit for bit)
 *       SMR_CONVERT_BLOCK_4X2  k_yuv_to_rgba_batch for 4:2:0 frames too (round 3's converter; A/B) */
typedef enum smr_convert_impl { SMR_CONVERT_AUTO = 0, SMR_CONVERT_GENERAL = 1, SMR_CONVERT_BLOCK_4X2 = 2 } smr_convert_impl;
/*   SMR_OPT_COMPACT_NODES       1 (default): the node texture of a 4:2:0 frame that only the matrix-core resampler reads is written as RGB12 — 12 bytes
 *                               per four pixels (R x 4, G x 4, B x 4; alpha is 1 for every Y'CbCr frame and is not stored): a quarter less traffic on
 *                               either side of the intermediate the default route is bound by; 0: always RGBA8.  Same codes, same tiles bit for bit. */
/*   SMR_OPT_PLANE_SOURCE        1: a planar 4:2:0 / NV12 frame whose layout plan lies inside the matrix-core resampler's class windows (scales around 1.5, 2
 *                               and 3: every input of the benchmark scenes) is read by that kernel as it is — the wave converts each chunk of its window with
 *                               the exact converter's own block arithmetic (the node texture's bytes, bit for bit) into LDS and resamples from there: the
 *                               reference's node texture never exists in memory (half the route's traffic, one launch fewer; the same pixels within the
 *                               resampler's 1 LSB).  0 (default): the converter writes the node texture (RGB12 with SMR_OPT_COMPACT_NODES) and the
 *                               resampler reads it back — faster on every measured workload: a wave converts its window's overlaps again (1.45 x) at two
 *                               waves per SIMD, the converter kernel converts every pixel once at six. */
/*   SMR_OPT_FUSED_KERNELS       1 (default): smr_render_layouts / smr_ingest_resample* run the fused kernels (waves A and B); 0: one general kernel per pass
 *                               of the reference (convert, resample passes, apply_layouts, rgba_to_yuv) — what the tests hold the fused kernels to.
 *   SMR_OPT_COMPOSE_SELECT      1 (default): compositor tiles in which every pixel is a plain copy from the topmost layer that holds it (the seams of a
 *                               grid of opaque 1:1 layers) are copied; 0: they take the compositing path.  Same output bytes either way.
 *   SMR_OPT_SHARED_DEVICE       1: other contexts run kernels on this device at the same time (a renderer's lanes: frames in flight).  The matrix-core
 *                               resampler then occupies two waves per SIMD instead of all it could hold (it is as fast from two: its time is a
 *                               dependency chain), which leaves a SIMD's remaining registers to the other lane's converter / compositor waves:
 *                               +2 % frames per second with two lanes, -3 % with one.  0 (default).  smr_renderer_add_lane sets it on every lane.
 * No option is read from the environment: a product build of the library calls getenv nowhere (laboratory builds, -DSMR_LAB, read their A/B knobs there). */
typedef enum smr_option {
    SMR_OPT_INGEST_IMPL = 0, SMR_OPT_INGEST_STRIP_WIDTH = 1, SMR_OPT_DIRECT_OUTPUT = 2, SMR_OPT_CONVERT_IMPL = 3, SMR_OPT_COMPACT_NODES = 4,
    SMR_OPT_FUSED_KERNELS = 5, SMR_OPT_COMPOSE_SELECT = 6, SMR_OPT_SHARED_DEVICE = 7, SMR_OPT_PLANE_SOURCE = 8
} smr_option;
SMR_API int smr_ctx_set_option(smr_ctx *ctx, uint32_t option, int32_t value);
SMR_API int smr_timer_start(smr_ctx *ctx);          /* hipEvent on the ctx stream */
SMR_API int smr_timer_stop(smr_ctx *ctx, float *ms); /* records, synchronises, returns elapsed ms */
/* Per-kernel-class timing with HIP events on the ctx stream (off by default).
 * stage ids: 0 ingest/convert, 1 resample, 2 layouts/compose, 3 output convert, 4 fused ingest+resample,
 * 5 fused compose+output. Accumulates ms and launch counts until reset. */
SMR_API int smr_profile_enable(smr_ctx *ctx, int enable);
SMR_API int smr_profile_read(smr_ctx *ctx, int stage, float *total_ms, uint32_t *launches);
SMR_API int smr_profile_reset(smr_ctx *ctx);
/* Which kernels a context has launched since it was created (always counted, no events): the tests assert the path a resample plan x
 * input format takes; a host can watch for scenes that leave the fast paths. */
typedef enum smr_kernel_id {
    SMR_KERNEL_INGEST_WAVE = 0,      /* k_ingest_wave with the fused conversion (laboratory builds only: always 0 in a product build) */
    SMR_KERNEL_INGEST_WAVE_RGBA = 1, /* k_ingest_wave on an RGBA8 / box-reduced RGBA16F node texture (every frame after smr_frame_to_rgba; surfaces) */
    SMR_KERNEL_FRAME_TO_RGBA_420 = 2, /* k_yuv420_to_rgba, the 4:2:0 planar / NV12 block converter: its launches (counted by FRAME_TO_RGBA as well) */
    SMR_KERNEL_INGEST_VALU = 3,      /* k_ingest_resample: fused conversion + Lanczos, every pass in f32 */
    SMR_KERNEL_RESAMPLE_GENERAL = 4, /* smr_resample on a node texture: box pre-reduction and one or two Lanczos pass kernels */
    SMR_KERNEL_FRAME_TO_RGBA = 5,    /* the input converters (InputTexture::convert_to_node_texture): launches — a block-converter launch takes up to 16 frames */
    SMR_KERNEL_COMPOSE_OUTPUT = 6,   /* k_compose_output: layout shader + output conversion */
    SMR_KERNEL_APPLY_LAYOUTS = 7,    /* k_apply_layouts: the general compositor */
    SMR_KERNEL_MOVE_RECTS = 8,       /* k_move_rects: the local gather's transport (smr_gather_tiles), one launch per sending context and 16 rectangles */
    SMR_KERNEL_INGEST_WAVE_DIRECT = 9, /* k_ingest_wave launches that carry a direct-output job (SMR_OPT_DIRECT_OUTPUT: the kernel stores Y'CbCr into the output frame) */
    SMR_KERNEL_COUNT_ = 10
} smr_kernel_id;
SMR_API int smr_debug_kernel_launches(const smr_ctx *ctx, uint32_t kernel, uint64_t *count);

/* ---- surfaces (NodeTexture / wgpu::Texture; state/node_texture.rs:11-163) -------- */
SMR_API int smr_surface_create(smr_ctx *ctx, uint32_t w, uint32_t h, uint32_t format, smr_surface **out);
/* Device memory the caller owns (a decoder's output, a torch tensor) as a surface, in place.  pitch >= w * bytes per texel; rows and the base
 * 4-byte aligned for the block converters, 16-byte aligned for the matrix-core resampler's node textures (other alignments take the general
 * kernels).  What the library READS of a wrapped surface:
 *   - 4:2:0 / NV12 planes of a frame (the input converter): the texels of each row and nothing else — every wrapped plane, tight rows
 *     (pitch == bytes per row) or wide ones, is converted by the build of the block converter that requests nothing behind a row's last
 *     column (k_yuv420_to_rgba_tight: the same bytes, ~2 % more instructions), so pitch * (h - 1) + row bytes of allocation suffice;
 *   - RGBA8 / RGBA16F surfaces handed to the resampler or the compositor: whole 16-byte groups inside a row's pitch — the allocation must
 *     back every row out to the pitch rounded down to 16 bytes, the LAST ROW TOO.
 * Planes the library allocates itself (smr_surface_create / smr_frame_create: every allocation ends with 16 spare bytes) take the plain
 * converter.
 * What the library WRITES of a wrapped surface — a node texture, a tile, the planes of an output frame, an out_rgba target, whichever
 * entry point it is handed to as a destination: the w x h texels (w * bytes per texel in each of the h rows) and NO OTHER BYTE.  Not the
 * bytes between a row's last texel and the pitch, not a byte before the base pointer, not a byte after the last row's last texel: the
 * destination may be a window inside a larger allocation (an encoder surface inside a pool, a region of a shared picture) whose
 * "padding" is somebody else's pixels.  Kernels that store in groups (four pixels, 4 x 2 blocks, 16-byte tile stores) narrow the ragged
 * last group's store; routes whose stores need an alignment the surface does not have fall back to kernels that produce the same bytes.
 * smr_surface_clear and the uploads are part of it: they touch the texels' bytes of each row, not the rows out to the pitch.
 * Held on the device by tests/test_gpu_write_footprint.py (tight / slack / window geometries; every entry point that takes a destination
 * surface or frame except smr_gather_tiles, which the sharded compositor uses between tiles the library allocated, and the renderer, which
 * allocates its own outputs) and on the CPU emulator by guard mode 3 of tests/emu. */
SMR_API int smr_surface_wrap(smr_ctx *ctx, void *dptr, size_t pitch, uint32_t w, uint32_t h, uint32_t format,
                             smr_surface **out);
SMR_API void smr_surface_destroy(smr_ctx *ctx, smr_surface *s);
SMR_API int smr_surface_info_get(const smr_surface *s, smr_surface_info *out);
/* queue.write_texture (wgpu/texture/base.rs:61-77); host_pitch 0 = tight rows */
SMR_API int smr_surface_upload(smr_ctx *ctx, smr_surface *s, const void *host, size_t host_pitch);
/* copy_texture_to_buffer + map + strip padding (texture/base.rs:97-118, output_texture.rs:85-113) */
SMR_API int smr_surface_download(smr_ctx *ctx, const smr_surface *s, void *host, size_t host_pitch);
SMR_API int smr_surface_clear(smr_ctx *ctx, smr_surface *s);

/* ---- frames (InputTexture upload side: state/input_texture.rs:69-201) ------------ */
SMR_API int smr_frame_create(smr_ctx *ctx, uint32_t format, uint32_t w, uint32_t h, smr_frame *out);
SMR_API void smr_frame_destroy(smr_ctx *ctx, smr_frame *f);
SMR_API int smr_frame_upload(smr_ctx *ctx, const smr_frame *f, const void *const host_planes[3]);
SMR_API int smr_frame_download(smr_ctx *ctx, const smr_frame *f, void *const host_planes[3]);
/* Pinned host memory and stream-ordered copies (no staging, no implicit synchronisation): what replaces the reference's
 * queue.write_texture staging (input_texture.rs:69-201) and the padded read-back + repack (output_texture.rs:68-113) for hosts
 * that can keep frames in buffers from smr_host_alloc.  Host buffers must stay untouched until smr_sync has returned. */
SMR_API int smr_host_alloc(smr_ctx *ctx, size_t bytes, void **out);
SMR_API void smr_host_free(smr_ctx *ctx, void *p);
SMR_API int smr_frame_upload_async(smr_ctx *ctx, const smr_frame *f, const void *const host_planes[3]);
SMR_API int smr_frame_download_async(smr_ctx *ctx, const smr_frame *f, void *const host_planes[3]);

/* ---- a3: InputTexture::convert_to_node_texture (input_texture.rs:203-219) ---------
 * wgpu/format/{planar_yuv,nv12,interleaved_uyvy,interleaved_yuyv,bgra,argb}_to_rgba.{rs,wgsl};
 * RGBA frames go through add_premultiplied_alpha (input_texture/rgba_texture.rs:38-63). */
SMR_API int smr_frame_to_rgba(smr_ctx *ctx, const smr_frame *in, smr_surface *node);
SMR_API int smr_add_premultiplied_alpha(smr_ctx *ctx, const smr_surface *src, smr_surface *dst);
SMR_API int smr_remove_premultiplied_alpha(smr_ctx *ctx, const smr_surface *src, smr_surface *dst);

/* ---- a11: read_outputs (render_loop.rs:59-230) -------------------------------------
 * RgbaToYuvConverter::convert (format/rgba_to_yuv.rs:67-117) for planar 420/422/444,
 * RgbaToNv12Converter::convert (format/rgba_to_nv12.rs:54-82) for NV12; SMR_FRAME_RGBA is a copy; SMR_FRAME_UYVY422 / SMR_FRAME_YUYV422 (even
 * widths; this library's own, see smr_frame_format) are the planar 4:2:2 planes interleaved, one launch, any height.  The 10-bit formats
 * and a format with a matrix tag are refused. */
SMR_API int smr_rgba_to_frame(smr_ctx *ctx, const smr_surface *node, const smr_frame *out);
/* PlanarYuvTextures::fill_with_color(BLACK) (wgpu/texture/planar_yuv.rs:190-202): Y = 16, U = V = 128 in every plane of a planar / NV12
 * frame and in every texel of a packed 4:2:2 frame (even widths); zeros for SMR_FRAME_RGBA.  Other formats are refused. */
SMR_API int smr_frame_fill_black(smr_ctx *ctx, const smr_frame *out);

/* ---- a7/a8: resampler (layout/resampler.rs) ---------------------------------------- */
/* ResampledChild::is_needed + pass planning; pure host function. crop = {top,left,width,height}. */
SMR_API int smr_resample_plan_make(uint32_t src_w, uint32_t src_h, const float crop[4], uint32_t dst_w, uint32_t dst_h,
                                   smr_resample_plan *out);
/* ResampledChild::render: box pre-reduce + 1 or 2 Lanczos3 passes. Returns the plan kind
 * (0 = direct: dst untouched) or a negative status. */
SMR_API int smr_resample(smr_ctx *ctx, const smr_surface *src, const float crop[4], smr_surface *dst);
/* single passes (resample.wgsl / downsample.wgsl), exposed for tests and the Rust seam */
SMR_API int smr_resample_pass(smr_ctx *ctx, const smr_surface *src, int axis, float scale, float offset, int perp_offset,
                              smr_surface *dst);
SMR_API int smr_downsample(smr_ctx *ctx, const smr_surface *src, uint32_t fx, uint32_t fy, smr_surface *dst);
/* format/rgba_rescale.wgsl via FramePreProcessor::rescale_node_texture (frame_pre_processor.rs:117-132) */
SMR_API int smr_rescale_bilinear(smr_ctx *ctx, const smr_surface *src, smr_surface *dst);
/* a15: FramePreProcessor::process_to_bytes (state/frame_pre_processor.rs:84-107) in one call — the frame (device-resident, any
 * smr_frame_format) through convert_to_node_texture into an RGBA8 node texture at its own resolution, the optional bilinear rescale
 * to dst_w x dst_h (0 x 0 = none; filtering in linear light in GpuOptimized mode, as rescale_node_texture does it) and the
 * read-back as tightly packed rows (host_pitch 0) or rows host_pitch bytes apart.  Blocks until the bytes are in `host`.
 * The intermediate surfaces belong to the context and are reused while the resolutions repeat (as the reference's instance does). */
SMR_API int smr_frame_preprocess(smr_ctx *ctx, const smr_frame *in, uint32_t dst_w, uint32_t dst_h, void *host, size_t host_pitch);

/* ---- a9/a10: LayoutShader::render (layout/shader.rs:93-167 + apply_layouts.wgsl) ---
 * Clears target to transparent, draws layouts back to front with premultiplied OVER.
 * sources[i] may be NULL (sampled as the 1x1 transparent texture, layout.rs:204-212). */
SMR_API int smr_apply_layouts(smr_ctx *ctx, smr_surface *target, const smr_layout *layouts, uint32_t n,
                              const smr_surface *const *sources, uint32_t n_sources);

/* ---- fused hot path: LayoutNode::render + read_outputs in (at most) two kernel waves --
 * Equivalent to: for every texture layout resample_scaled_children (layout.rs:238-278) from the
 * raw frame / surface, LayoutShader::render, then rgba_to_yuv / rgba_to_nv12 into `out`
 * (or a copy into `out_rgba` when out == NULL).  Bit-identical to the unfused sequence with SMR_INGEST_VALU_F32,
 * within 1 LSB of it with the matrix-core resampler (SMR_OPT_INGEST_IMPL). */
SMR_API int smr_render_layouts(smr_ctx *ctx, const smr_layout *layouts, uint32_t n, const smr_source *sources,
                               uint32_t n_sources, uint32_t out_w, uint32_t out_h, const smr_frame *out,
                               smr_surface *out_rgba);

/* Per-input half of the above, for sharding inputs across GPUs: InputTexture::convert_to_node_texture
 * (input_texture.rs:203-219) + ResampledChild::render (resampler.rs:305-378) in one step, frame -> dst-sized
 * RGBA8 tile.  Returns the plan kind (0 = direct: dst untouched) or a negative status. */
SMR_API int smr_ingest_resample(smr_ctx *ctx, const smr_frame *in, const float crop[4], smr_surface *dst);
/* All inputs of a shard in one launch: crops = n x {top, left, width, height}; kinds[i] (optional) = plan kind of input i. */
SMR_API int smr_ingest_resample_batch(smr_ctx *ctx, const smr_frame *const *in, const float *crops, smr_surface *const *dst, uint32_t n,
                                      int *kinds);

/* ---- multi-GPU exchange step (no counterpart in the reference, which owns one wgpu device) -------
 * Inputs are sharded over GPUs (input i -> GPU i mod N); each GPU turns its inputs into dst-sized tiles with
 * smr_ingest_resample_batch (the per-input independence of render_loop.rs:24-41, layout.rs:250-275), the tiles are gathered
 * on the GPU that composes (smr_render_layouts with the tiles as SMR_SOURCE_OPAQUE_SURFACE sources).  Everything is
 * stream-ordered on the contexts' streams: no call below blocks the host.
 *   smr_comm_create_local  ONE process driving n devices (what smelter-core's renderer thread would hold,
 *                          smelter-core/src/pipeline/instance.rs:435-503): peer copies over xGMI, one link per sender.
 *   smr_comm_create_rank   one process per GPU: RCCL point-to-point.  Rank 0 makes an id with smr_comm_unique_id and hands the
 *                          128 bytes to the others by whatever means the host has.
 * smr_gather_tiles: tile i was produced on rank owner[i] in src[i]; afterwards dst[i] on `root` holds it (tiles the root owns
 * are skipped).  Local comm: one call moves everything.  Rank comm: every rank makes the same call; src[i] is read on its
 * owner only, dst[i] written on the root only (other entries may be NULL there); in rank mode a tile travels as one block of
 * pitch * h bytes, so src[i] and dst[i] must both have the canonical pitch (w * bytes per pixel rounded up to 256, what
 * smr_surface_create gives) — anything else is SMR_ERR_INVALID. */
typedef struct smr_comm smr_comm;
#define SMR_COMM_ID_BYTES 128
SMR_API int smr_comm_create_local(smr_ctx *const *ctxs, uint32_t n, smr_comm **out);
SMR_API int smr_comm_unique_id(uint8_t id[SMR_COMM_ID_BYTES]);
SMR_API int smr_comm_create_rank(smr_ctx *ctx, uint32_t world, uint32_t rank, const uint8_t id[SMR_COMM_ID_BYTES], smr_comm **out);
SMR_API void smr_comm_destroy(smr_comm *comm);
SMR_API uint32_t smr_comm_world(const smr_comm *comm);
SMR_API uint32_t smr_comm_rank(const smr_comm *comm);
SMR_API const char *smr_comm_last_error(const smr_comm *comm);
SMR_API int smr_gather_tiles(smr_comm *comm, uint32_t root, const uint32_t *owner, const smr_surface *const *src, smr_surface *const *dst,
                             uint32_t n);

/* ---- a12: text (transformations/text_renderer.rs:72-167, 236-368) -------------------
 * TextRendererNode::render's blit: clear `target` to bg (a shader colour: convert_to_shader_color of the node's background), then
 * every glyph quad's coverage from the A8 atlas in the quad's colour, premultiplied OVER. */
SMR_API int smr_blit_glyphs(smr_ctx *ctx, smr_surface *target, const float bg[4], const smr_glyph *glyphs, uint32_t n,
                            const uint8_t *atlas_host, uint32_t atlas_w, uint32_t atlas_h);

/* The host half of the text node — font database, line layout, glyph rasteriser — behind the ABI (host code, no GPU):
 *   TextRendererCtx::new / add_font, Renderer::register_font (state.rs:168-171)  -> smr_fontbook_add_file / _add_memory / _add_dir
 *   TextRendererCtx::layout_text: Buffer::set_text + set_wrap + set_size + shape_until_scroll, get_text_resolution (text_renderer.rs:282-368)
 *                                                                                -> smr_fontbook_measure (a smr_text_measure_fn: pass the book as `user`)
 *   TextRendererNode::render's prepare(): the laid-out buffer as atlas + quads   -> smr_fontbook_rasterise
 * The reference does all of this with glyphon / cosmic-text / swash (third-party, not in its tree).  This library's reader is its own:
 * TrueType `glyf` outlines (simple + composite), `cmap` formats 0 / 4 / 6 / 12 / 13, `hmtx` advances, pair kerning from the GPOS `kern`
 * feature (PairPos 1 and 2, extension lookups), explicit newlines, Wrap::None / Glyph / Word, Left / Center / Right alignment (Justified
 * is laid out as Left), a line's ascent + descent centred in its line box, exact-area coverage at the fractional pen position.  NOT
 * restated: GSUB (ligatures, contextual alternates), mark positioning, bidi, font fallback, hinting, CFF outlines — glyph shapes and
 * sub-pixel positions are this library's, not glyphon's: PARITY FOR TEXT PIXELS IS UNPINNED (no reference artefact holds them in-tree).
 * Fonts are loaded by path or from memory; the reference bundles Inter (smelter-render/fonts/ *.ttf), hosts register the same files. */
typedef struct smr_fontbook smr_fontbook;
/* What a shaper lays out: TextComponent's text, font attributes and wrap mode (text_renderer.rs:174-233) inside max_width x max_height.
 * Strings are the reference's variant names ("Normal" | "Italic" | "Oblique", "Thin" .. "Black", "None" | "Glyph" | "Word",
 * "Left" | "Right" | "Justified" | "Center"). */
typedef struct smr_text_params {
    const char *text, *font_family, *style, *weight, *wrap, *align;
    float font_size, line_height;
    float max_width, max_height;
} smr_text_params;
typedef struct smr_text_run {
    const smr_glyph *glyphs; /* owned by the font book: valid until its next smr_fontbook_rasterise / destroy */
    uint32_t n_glyphs;
    const uint8_t *atlas;    /* A8 coverage, atlas_w x atlas_h, tight rows */
    uint32_t atlas_w, atlas_h;
} smr_text_run;
SMR_API int smr_fontbook_create(smr_fontbook **out);
SMR_API void smr_fontbook_destroy(smr_fontbook *book);
SMR_API const char *smr_fontbook_last_error(const smr_fontbook *book);
SMR_API int smr_fontbook_add_file(smr_fontbook *book, const char *path);                     /* fontdb::Source::File */
SMR_API int smr_fontbook_add_memory(smr_fontbook *book, const uint8_t *data, size_t size);   /* fontdb::Source::Binary (copied) */
SMR_API int smr_fontbook_add_dir(smr_fontbook *book, const char *dir);                       /* every *.ttf below dir, by path; returns how many, < 0 if none */
SMR_API uint32_t smr_fontbook_count(const smr_fontbook *book);
/* lays params->text out at font_size with params->wrap inside max_width; widest line (pixels) and line count — the signature of
 * smr_text_measure_fn with `user` = the font book.  Refused (SMR_ERR_INVALID, message in smr_fontbook_last_error): text that is not UTF-8,
 * font_size outside (0, 100000] or not finite, a line_height that is not finite; smr_fontbook_add_* refuse a face whose tables do not
 * hold together (directory, head / hhea / maxp / hmtx / cmap / loca / glyf bounds, unitsPerEm outside 16 .. 16384).  Fonts and text
 * are untrusted input: tests/san drives this API with corrupted faces under AddressSanitizer. */
SMR_API int smr_fontbook_measure(void *book, const smr_text_params *params, float *widest_line, uint32_t *line_count);
/* the glyph run of a Text node of width x height pixels for smr_blit_glyphs / smr_renderer_set_text; `color` = straight RGBA 0..1 */
SMR_API int smr_fontbook_rasterise(smr_fontbook *book, const smr_text_params *params, uint32_t width, uint32_t height, const float color[4],
                                   smr_text_run *out);

/* ---- a13: the Shader node — built-in kernels, and user shaders written in HIP C++ ---- */
/* Built-in kernels for ShaderNode::render (transformations/shader/node.rs:71-89, shader/pipeline.rs:81-141).  User WGSL needs a
 * compiler this library does not carry (user shaders in HIP C++: below); built in are the shaders the reference keeps in its own tree,
 * restated as HIP kernels with the node's semantics: the target is cleared to transparent, one full-target plane is drawn per
 * source texture (plane_id 0..n-1; a single plane with plane_id -1 when there are none), premultiplied-alpha OVER, each plane
 * stored to the RGBA8 target before the next is blended.  BaseShaderParameters {plane_id, time, output_resolution,
 * texture_count} (shader/base_params.rs:7-12) are supplied by the library from time_s, dst and n_src.
 *   GAUSSIAN_BLUR        params = smr_gaussian_blur_params                                     (no reference counterpart)
 *   GRADIENT             integration-tests/src/render_tests/yuv_tests/gradient.wgsl
 *   RED_BORDER           render_tests/shader/red_border.wgsl
 *   CIRCLE_LAYOUT        render_tests/shader/circle_layout.wgsl; params = smr_circle_layout[n_src] (ShaderParam::to_bytes order)
 *   FADE_TO_BALL         render_tests/shader/fade_to_ball.wgsl
 *   LAYOUT_PLANES        render_tests/shader/layout_planes.wgsl
 *   COLOR_BY_TEXTURE_COUNT  render_tests/shader/color_output_with_texture_count.wgsl
 *   SILLY                integration-tests/examples/silly.wgsl */
typedef enum smr_builtin_shader_id {
    SMR_SHADER_GAUSSIAN_BLUR = 0,
    SMR_SHADER_GRADIENT = 1,
    SMR_SHADER_RED_BORDER = 2,
    SMR_SHADER_CIRCLE_LAYOUT = 3,
    SMR_SHADER_FADE_TO_BALL = 4,
    SMR_SHADER_LAYOUT_PLANES = 5,
    SMR_SHADER_COLOR_BY_TEXTURE_COUNT = 6,
    SMR_SHADER_SILLY = 7
} smr_builtin_shader_id;
#define SMR_SHADER_MAX_SOURCES 16 /* binding_array<texture_2d<f32>, 16> */
typedef struct smr_circle_layout { uint32_t left_px, top_px, width_px, height_px; float background_color[4]; } smr_circle_layout;
typedef struct smr_gaussian_blur_params { float sigma; } smr_gaussian_blur_params;
SMR_API int smr_builtin_shader(smr_ctx *ctx, uint32_t id, const void *params, size_t params_size,
                               const smr_surface *const *src, uint32_t n_src, smr_surface *dst, float time_s);

/* User shaders.  A Shader component runs the caller's own fragment function; here it is written in HIP C++ and compiled to a gfx950
 * code object by the ROCm runtime compiler (libhiprtc.so, loaded on first use) when the shader is registered.  A shader is ONE
 * translation unit that includes nothing and defines
 *     __device__ float4 smr_fragment(const smr_shader_in &in, int plane_id, float2 uv, float2 position);
 *     // optional, announced with `#define SMR_HAS_VERTEX` at the top of the source:
 *     __device__ smr_plane smr_vertex(const smr_shader_in &in, int plane_id);
 *     // or, announced with `#define SMR_HAS_VERTEX_AFFINE` instead:
 *     __device__ smr_affine smr_vertex_affine(const smr_shader_in &in, int plane_id);
 *     // or, announced with `#define SMR_HAS_VERTEX_CLIP` instead (the clip vertex stage: below):
 *     __device__ smr_clip_vertex smr_vertex_clip(const smr_shader_in &in, int plane_id, int vertex_index, float3 position, float2 tex_coords);
 *     // and, with `#define SMR_VARYINGS N` beside SMR_HAS_VERTEX_CLIP (varyings: below), these two instead of the first and the last:
 *     __device__ smr_clip_vertex_v<SMR_VARYINGS> smr_vertex_clip(const smr_shader_in &in, int plane_id, int vertex_index, float3 position, float2 tex_coords);
 *     __device__ float4 smr_fragment(const smr_shader_in &in, int plane_id, float2 uv, float4 position, const smr_varyings<SMR_VARYINGS> &v);
 * The node's semantics are those of the built-in kernels (the same kernel with the user's functions in place of the built-in switch):
 * the target is cleared to transparent, one plane per source is drawn in order (plane_id 0 .. texture_count - 1; one plane with
 * plane_id -1 when the node has no children), every plane blended premultiplied-alpha OVER and stored to the RGBA8 target before the
 * next.  smr_fragment gets the fragment's tex_coords `uv` within the plane and its pixel-centre `position` (@builtin(position).xy) and
 * returns premultiplied RGBA in the target's blending space (linear light in SMR_MODE_GPU_OPTIMIZED, unorm values in
 * SMR_MODE_CPU_OPTIMIZED).  smr_vertex returns smr_plane {sx, sy, cx, cy}: the unit quad's corners go to clip-space position * (sx, sy) +
 * (cx, cy); a plane with sx <= 0 or sy <= 0 covers nothing.  smr_vertex_affine returns smr_affine {xx, xy, yx, yy, cx, cy}: corner
 * (px, py) of the unit quad, px, py in {-1, +1}, goes to clip space X = xx * px + xy * py + cx, Y = yx * px + yy * py + cy — a 2 x 2
 * matrix and a translation, so any parallelogram is expressible: rotated, sheared, scaled; perspective and per-vertex tex_coords need the
 * clip vertex stage below; screen-space derivatives (dpdx, dpdy, fwidth): SMR_DERIVATIVES, below.  Still NOT expressible: compute passes,
 * raw surface access, discard, WGSL text.  A pixel
 * belongs to the plane when its centre, taken back into the quad (qx, qy) = M^-1 (X - cx, Y - cy) in f32, has -1 <= qx < 1 and
 * -1 < qy <= 1: a centre exactly on an edge belongs to the plane whose left / top edge (in quad space) it is; uv = ((qx + 1) / 2,
 * (1 - qy) / 2), position stays the pixel centre.  With xy == 0 and yx == 0 the plane IS smr_plane {xx, yy, cx, cy}, byte for byte,
 * the rule for sx, sy <= 0 included: a half turn written with exact zeros, {-a, 0, 0, -b}, is NOT drawn although its det is positive
 * (a half turn by sinf / cosf, whose xy and yx are tiny but not zero, is) — write it as {a, 0, 0, b} and flip in the fragment (sample
 * at 1 - u, 1 - v).  Otherwise det = xx * yy - xy * yx decides: a plane whose det is zero, NaN or infinite covers
 * nothing, and neither does a MIRRORED plane (det < 0) — the reference draws the quad with front_face Ccw and cull_mode Some(Back)
 * (smelter-render/src/wgpu/common_pipeline.rs:104-107, the pipeline transformations/shader/pipeline.rs:63 creates), so a plane whose
 * winding is reversed is culled there too; mirror a picture in the fragment (sample at 1 - u) instead.  A source that defines both
 * SMR_HAS_VERTEX and SMR_HAS_VERTEX_AFFINE does not compile ("#error": one vertex stage per shader; smr_shader_program_create
 * returns SMR_ERR_INVALID, the message is in smr_shader_program_log).  Without a vertex stage every plane covers the target.
 *   The clip vertex stage (SMR_HAS_VERTEX_CLIP) is the reference's: it is called once for each of the four vertices of every plane's quad
 * (smelter-render/src/wgpu/common_pipeline/plane.rs:6-28; vertex_index 0..3, `position` / `tex_coords` = (1, -1, 0) / (1, 1), (1, 1, 0) /
 * (1, 0), (-1, 1, 0) / (0, 0), (-1, -1, 0) / (0, 1)) and returns smr_clip_vertex {float4 position; float2 tex_coords;}: the homogeneous
 * clip-space position (x, y, z, w) and the tex_coords varying.  It may use what smr_fragment may use except smr_sample (WGSL has no textureSample
 * outside the fragment stage): smr_load, smr_dimensions, the parameters, in.*.  Further varyings: SMR_VARYINGS, below.  Defining it together
 * with SMR_HAS_VERTEX or SMR_HAS_VERTEX_AFFINE is the same "#error" (one vertex stage per shader, SMR_ERR_INVALID, the message in the log).
 * smr_fragment keeps its signature: uv is the interpolated tex_coords, position the pixel centre.  The quad is drawn as the triangles
 * (0, 1, 2) then (2, 3, 0) by 2-D homogeneous rasterisation — no clipping step, no division before coverage.  With p_k = (x_k, y_k, w_k)
 * of vertex k, for triangle (i, j, k):
 *   - edge coefficients (a, b, c)_i = p_j x p_k, and cyclic: a_i = y_j w_k - w_j y_k, b_i = w_j x_k - x_j w_k, c_i = x_j y_k - y_j x_k.  The
 *     shared diagonal is p_2 x p_0 in the first triangle and p_0 x p_2 in the second: exact negations of each other.
 *   - D = det[p_i p_j p_k] = (x_i a_i + y_i b_i) + w_i c_i.  The triangle is drawn only if D > 0 and finite: D <= 0 is a back face (the
 *     reference culls with front_face Ccw, cull_mode Back), an edge-on or degenerate plane; NaN or infinite D, or any interpolation
 *     coefficient below that is not finite (a NaN or infinity in z or tex_coords, products that overflow), covers nothing.  The identity
 *     stage gives D = 4 for both triangles.
 *   - with the pixel centre (X, Y) in clip space (X = (x + 0.5) / W * 2 - 1, Y = 1 - (y + 0.5) / H * 2), E_i = (a_i X + b_i Y) + c_i.  The
 *     pixel is covered if every E_i is > 0, or == 0 on an inclusive edge: a_i > 0, or a_i == 0 and b_i < 0 — the top-left rule with Y
 *     pointing up, which agrees with the half-open rule of smr_plane; a centre on the diagonal belongs to exactly one triangle.  With D > 0
 *     the covered region is exactly the part of the triangle with w > 0: a vertex behind the eye (w <= 0) needs no special case.
 *   - depth clip, 0 <= z <= w as wgpu clips: the pixel is dropped unless sum E_i z_i >= 0 and sum E_i (w_i - z_i) >= 0.
 *   - uv = sum E_i tex_coords_i / sum E_i: perspective-correct (E_i / sum E are the barycentrics on the triangle in clip space).
 *   The kernel evaluates this in f32, every operation rounded on its own, in this order: the cross products as written; for each attribute
 *   t in {u, v, z, w - z} (w - z rounded first) the plane A_t = (a_0 t_0 + a_1 t_1) + a_2 t_2, B_t and C_t likewise from b and c, once per
 *   triangle; per pixel E_i as above, the sums as (A_t X + B_t Y) + C_t, sum E = (E_0 + E_1) + E_2, u and v by one division each.  A pixel
 *   covered by both triangles (possible only with contrived w: with w = 1 the second triangle of a folded quad is back-facing) is blended
 *   once per triangle in index order.  Everything after coverage is as for the other stages: premultiplied OVER, the store to the RGBA8
 *   target, the read back before the next triangle, the final transparent store.
 *   Varyings.  A shader that defines SMR_HAS_VERTEX_CLIP may also `#define SMR_VARYINGS N`, 1 <= N <= 8: f32 varyings 0 .. N - 1, the
 * reference's @location outputs.  smr_vertex_clip then returns smr_clip_vertex_v<SMR_VARYINGS> {float4 position; float2 tex_coords; float
 * varyings[N];} and smr_fragment takes (in, plane_id, uv, float4 position, const smr_varyings<SMR_VARYINGS> &v) with v.v[k] varying k at the
 * pixel and `position` the whole @builtin(position): (x + 0.5, y + 0.5, z / w, 1 / w).  Two optional bit masks choose each varying's
 * interpolation: bit k of SMR_VARYINGS_FLAT makes varying k @interpolate(flat) — the value of the triangle's FIRST vertex (WebGPU's default
 * provoking vertex: vertex 0 for triangle (0, 1, 2), vertex 2 for (2, 3, 0)); bit k of SMR_VARYINGS_LINEAR makes it @interpolate(linear),
 * linear in screen space; neither bit: @interpolate(perspective), the rule of uv.  SMR_VARYINGS without SMR_HAS_VERTEX_CLIP, N outside
 * 1 .. 8, a mask bit at or above N, or the same bit in both masks does not compile ("#error", SMR_ERR_INVALID, the message in the log).  A
 * shader that does not define SMR_VARYINGS is compiled exactly as before.  In f32, every operation rounded on its own, with E_i, sum E and
 * the depth sum Zn = sum E_i z_i as above and Wn = sum E_i w_i evaluated from its own plane ((a_0 w_0 + a_1 w_1) + a_2 w_2, likewise b, c):
 *   - perspective: exactly as u, v — the plane A_t = (a_0 t_0 + a_1 t_1) + a_2 t_2, B_t, C_t likewise; per pixel ((A_t X + B_t Y) + C_t) / sum E.
 *   - linear: the barycentrics in screen space are lambda_i = E_i w_i / sum E_j w_j; the plane is built from the products t_i * w_i, each
 *     rounded first; per pixel ((A X + B Y) + C) / Wn.
 *   - flat: the provoking vertex's 32-bit WORD, moved from the vertex stage's result to the fragment's argument as an integer: no arithmetic
 *     touches it, so a NaN payload or an integer stored with __uint_as_float arrives bit for bit.
 *   - position.z = Zn / Wn and position.w = sum E / Wn.  No pixel is dropped on account of Wn: where it is 0 (or where a vertex has
 *     w <= 0 and it nearly cancels) these quotients and the linear varyings are what IEEE division gives — infinities or NaN.
 *   A flat varying takes no part in the "every coefficient finite" rule of D above (a NaN there is data), and neither does Wn's plane; a
 *   non-finite plane coefficient of a perspective or linear varying makes the triangle cover nothing, as for tex_coords — whether or not
 *   the fragment reads that varying.  Declaring varyings changes neither coverage nor uv.
 *   Derivatives.  A shader that puts `#define SMR_DERIVATIVES` at the top of its source — alone or beside any vertex stage, with or without
 * SMR_VARYINGS — may call, from smr_fragment only, WGSL's dpdx, dpdy, fwidth and their Fine / Coarse forms:
 *     float smr_dpdx(float v)          smr_dpdy(float v)          smr_fwidth(float v)
 *     float smr_dpdx_fine(float v)     smr_dpdy_fine(float v)     smr_fwidth_fine(float v)
 *     float smr_dpdx_coarse(float v)   smr_dpdy_coarse(float v)   smr_fwidth_coarse(float v)        and float2 overloads of all nine, per component
 * The target is dealt out in 2 x 2 pixel QUADS aligned to even target coordinates: a = (x0, y0), b = (x0 + 1, y0), c = (x0, y0 + 1),
 * d = (x0 + 1, y0 + 1).  Window y grows downwards: dpdy(position.y) == +1.
 *   - coarse: for all four pixels dpdx = v_b - v_a and dpdy = v_c - v_a.
 *   - fine: dpdx is the pixel's own row's right value minus its left one (v_b - v_a for a and b, v_d - v_c for c and d), dpdy its own
 *     column's lower value minus its upper one (v_c - v_a for a and c, v_d - v_b for b and d).
 *   - plain: smr_dpdx, smr_dpdy and smr_fwidth ARE the coarse ones.  WGSL leaves the choice to the implementation; this is a definition of
 *     this library, not a measurement of any other.
 *   - fwidth = |dpdx| + |dpdy| of the same flavour.  Each derivative is one f32 subtraction, rounded once; fwidth two fabs and one add.
 *   Helper invocations.  For every plane (every triangle, in the clip stage) smr_fragment runs for all four pixels of a quad if at least
 * one of them is covered — covered by the rules above, unchanged (coverage, depth clip, sum E > 0).  A pixel of that quad that is not
 * covered is a HELPER, and so is a pixel outside the target when its width or height is odd.  A helper gets the same plane_id; its uv,
 * position, varyings and position.z / w come from the same formulas in the same operation order at its own pixel centre, with no coverage test
 * applied: extrapolated values — in the clip stage sum E may be <= 0 there and the quotients are what IEEE division gives.  A helper's
 * return value is dropped: it never stores to the target and never loads from it; smr_sample clamps and smr_load bounds-checks as always, so
 * a helper cannot touch memory outside the sources either.  Coverage, uv, blend and the picture of a shader that calls no derivative are
 * unchanged by the macro, byte for byte.
 *   Uniformity.  As in WGSL a derivative must be called in control flow that is uniform across the quad (all four invocations reach the call, or
 * none: before any branch on a per-pixel value; a branch on plane_id, the parameters or in.* is uniform).  Elsewhere its value is
 * unspecified — it is only ever a register value, never an address: an invocation that is not there reads as 0.  Calling a derivative from
 * a vertex stage is not diagnosed; its value there is unspecified.  Calling any of the nine without SMR_DERIVATIVES does not compile
 * (a static_assert whose message names SMR_DERIVATIVES; SMR_ERR_INVALID, the message in smr_shader_program_log).  A shader that does not
 * define SMR_DERIVATIVES is compiled exactly as before.  With it the launch is the same (64 x 4 pixels per 256-thread workgroup); inside, a
 * wave covers 32 x 2 pixels as sixteen quads of four consecutive lanes, and a neighbour's value is one register move.
 * What a shader may use (the library puts it in front of the source):
 *     in.time (seconds, float)   in.output_resolution (uint2)   in.texture_count (int)          BaseShaderParameters (base_params.rs:7-12)
 *     float4 smr_sample(in, i, u, v)        source i through the linear clamp-to-edge sampler, decoded to the blending space;
 *                                           (0, 0, 0, 0) when i is out of range or the source is absent
 *     uint2 smr_dimensions(in, i)           textureDimensions: source i's width and height; (0, 0) when i is out of range or absent
 *     float4 smr_load(in, i, x, y)          textureLoad, level 0: exactly texel (x, y) of source i, unfiltered, decoded like a texel of
 *                                           smr_sample; (0, 0, 0, 0) when i is out of range, the source is absent or (x, y) outside it
 *     T smr_param<T>(in)   const unsigned char *smr_param_bytes(in)   unsigned smr_param_size(in)
 *                                           the @group(1) uniform: the shader_param's values in order, little endian, no padding
 *                                           (ShaderParam::to_bytes); bytes behind smr_param_size read 0
 *     float smr_smoothstep(e0, e1, x)       WGSL smoothstep;  make_float2 / make_float4 and the HIP device math library (sqrtf, sinf, ...)
 * A shader never holds a pointer into a surface, and that stays true with smr_load: every access goes through smr_sample, which
 * clamps, or smr_load, which answers (0, 0, 0, 0) outside the source without reading — it cannot read or write outside its sources
 * and target.  It is compiled with the library's own options (--offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off):
 * every multiply and add is rounded on its own, as in the built-in kernels.  Compiling takes of the order of a second (DESIGN.md
 * section 3e): register shaders off the render thread. */
typedef struct smr_shader_program smr_shader_program;
#define SMR_SHADER_MAX_PARAM_BYTES 2048
/* Host only: needs no device and no context.  A source that does not compile returns SMR_ERR_INVALID and STILL hands out a program
 * object: smr_shader_program_log has the compiler's message ("shader:LINE:COLUMN: error: ..." — lines of the caller's source); such a
 * program cannot be registered or launched and is destroyed like any other.  No runtime compiler on the machine: SMR_ERR_INTERNAL, the
 * log names libhiprtc.so. */
SMR_API int smr_shader_program_create(const char *hip_source, smr_shader_program **out);
SMR_API const char *smr_shader_program_log(const smr_shader_program *p); /* errors and warnings, "" if none */
SMR_API int smr_shader_program_code(const smr_shader_program *p, const void **code, size_t *size); /* the gfx950 code object (tools/kernel_resources.py reads it) */
/* Launches of this program so far, over all contexts (which path rendered a Shader node is observable without a kernel counter slot) */
SMR_API int smr_shader_program_launches(const smr_shader_program *p, uint64_t *count);
/* Unloads the program's modules (after waiting for the devices that ran them).  A program must outlive its registrations. */
SMR_API void smr_shader_program_destroy(smr_shader_program *p);
/* Twin of smr_builtin_shader.  The code object is loaded once per device at the first launch there (shared by every context on the
 * device; unloaded with the program or the last of those contexts, whichever goes first); sources, target, time and the parameter
 * bytes travel by value in the kernel arguments — nothing is uploaded, nothing blocks, `params` may be freed on return.
 * SMR_ERR_INVALID: more than SMR_SHADER_MAX_PARAM_BYTES, more than SMR_SHADER_MAX_SOURCES, a target or source that is not RGBA8. */
SMR_API int smr_user_shader(smr_ctx *ctx, const smr_shader_program *p, const void *params, size_t params_size,
                            const smr_surface *const *src, uint32_t n_src, smr_surface *dst, float time_s);

/* ---- a5/a6: host scene engine (no GPU work) ------------------------------------------
 * Scene JSON (the smelter-api component schema, smelter-api/src/video/component.rs) -> stateful
 * component tree with transitions (smelter-render/src/scene/scene_state.rs:74-127) -> render graph
 * (IntermediateNode::build_tree, scene_state.rs:148-196) -> per frame the flattened smr_layout list
 * of one layout node (LayoutProvider::layouts + NestedLayout::flatten, transformations/layout.rs:176-184,
 * layout/flatten.rs:10-22).  One smr_scene == one output of the reference's SceneState. */
typedef struct smr_scene smr_scene;

typedef enum smr_node_kind {
    SMR_NODE_INPUT_STREAM = 0, /* NodeParams::InputStream */
    SMR_NODE_LAYOUT = 1,       /* NodeParams::Layout (View / Rescaler / Tiles root) */
    SMR_NODE_TEXT = 2,         /* NodeParams::Text */
    SMR_NODE_IMAGE = 3,        /* NodeParams::Image */
    SMR_NODE_SHADER = 4,       /* NodeParams::Shader */
    SMR_NODE_WEB_VIEW = 5      /* NodeParams::Web: size = the instance's resolution, children as a Shader's */
} smr_node_kind;

typedef struct smr_scene_node {
    uint32_t kind;        /* smr_node_kind */
    int32_t parent;       /* -1 for the root */
    uint32_t n_children;
    uint32_t width, height; /* intrinsic size (0,0 for an input stream that has not rendered yet) */
    const char *ref_id;   /* input_id / image_id / shader_id / instance_id, "" for layouts and text; valid until the next update */
    const char *id;       /* component id or "" */
    const char *payload;  /* Text: the string; otherwise "" */
} smr_scene_node;

#define SMR_NO_RESOLUTION 0xffffffffu /* child_wh width: the child has no texture (node_texture.rs state() == None) */

SMR_API int smr_scene_create(smr_scene **out);
SMR_API void smr_scene_destroy(smr_scene *scene);
SMR_API const char *smr_scene_last_error(const smr_scene *scene);
/* Fitted text (TextDimensions::Fitted / FittedColumn, text_renderer.rs:282-346): the renderer sizes a Text node without
 * "width"/"height" by the reference's rule (get_text_resolution, text_renderer.rs:348-368) —
 *     width  = max over the laid-out lines of ceil(line width)             (FittedColumn: the given width)
 *     height = trunc(lines * ceil(line_height) + font_size / 5)
 * — from the line metrics the caller's shaper reports through this callback (glyphon / cosmic-text in the reference, third-party):
 * lay `text` out at `font_size` with wrapping `wrap` ("None" | "Glyph" | "Word") inside max_width x max_height and return the
 * widest line and the number of lines.  Return non-zero to fail the scene update.  Without a measurer such nodes are refused. */
typedef int (*smr_text_measure_fn)(void *user, const smr_text_params *params, float *widest_line, uint32_t *line_count);
SMR_API int smr_scene_set_text_measurer(smr_scene *scene, smr_text_measure_fn fn, void *user);
/* Renderer::register_renderer(Image) as far as sizing goes (scene/image_component.rs) */
SMR_API int smr_scene_register_image(smr_scene *scene, const char *image_id, uint32_t width, uint32_t height);
/* Renderer::register_renderer(WebRenderer) as far as the scene goes: with it a `web_view` of this instance builds — a node of kind
 * SMR_NODE_WEB_VIEW whose size is width x height (web_view_component.rs:23-25, scene_state.rs:205) and whose children are built and walked
 * as a Shader's (a layout child needs a known size).  The reference's three errors, in its words (scene.rs:208-219): an instance that is
 * not registered, a child without an "id", and an instance used by more than one component of the scene (validation.rs:74-99; the renderer
 * holds the same rule across all its outputs).  Registering an id again replaces its resolution. */
SMR_API int smr_scene_register_web_renderer(smr_scene *scene, const char *instance_id, uint32_t width, uint32_t height);
/* Renderer::update_scene (state.rs:177-189).  On error the previous scene stays active. */
SMR_API int smr_scene_update(smr_scene *scene, const char *scene_json, uint32_t out_width, uint32_t out_height);
/* The API-to-scene conversion alone: `impl TryFrom<Component> for scene::Component`
 * (smelter-api/src/video/component_into.rs:8-432) with its defaults, validation and error strings.  *out_json is the
 * converted component tree as canonical JSON (owned by the scene, valid until the next call); the active scene is untouched.
 * Pinned by smelter-api/tests/scene_deserialization.rs (tests/golden/scene_api_vectors.json). */
SMR_API int smr_scene_parse(smr_scene *scene, const char *scene_json, const char **out_json);
SMR_API int smr_scene_node_count(const smr_scene *scene); /* nodes in pre-order, 0 is the root */
SMR_API int smr_scene_node_info(const smr_scene *scene, int node, smr_scene_node *out);
SMR_API int smr_scene_node_children(const smr_scene *scene, int node, int32_t *out, uint32_t cap);
/* LayoutNode::render up to the flattened list.  child_wh = {w0,h0,w1,h1,...} one pair per child node in order
 * (w == SMR_NO_RESOLUTION: no texture).  mode selects convert_to_shader_color's sRGB handling (wgpu/utils.rs:51-72).
 * Writes min(*n_out, cap) layouts; also advances the scene clock used by the next smr_scene_update
 * (SceneState::register_render_event, scene_state.rs:59-67). */
SMR_API int smr_scene_node_layouts(smr_scene *scene, int node, int64_t pts_ns, const uint32_t *child_wh, uint32_t n_children,
                                   uint32_t mode, smr_layout *out, uint32_t cap, uint32_t *n_out, uint32_t *out_width,
                                   uint32_t *out_height);
/* Host only. ImageRenderParams::start_pts of node `node` (an Image node, else SMR_ERR_INVALID): the pts its animation clock counts from.
 * An Image component with an `id` keeps it across smr_scene_update while the previous scene holds an Image of the same id, image_id, width
 * and height (scene/image_component.rs:91-120); otherwise, and for every component without an id, it is the pts of the last render before the
 * update (smr_scene_node_layouts' clock; 0 before any render).  Static images carry it too, as in the reference. */
SMR_API int smr_scene_node_start_pts(const smr_scene *scene, int node, int64_t *start_pts_ns);
/* Host only. AnimatedAsset::render's choice (animated_image.rs:127-136) in exact integers.  With pts_0 = 0, pts_k = delays_ns[0] + .. +
 * delays_ns[k - 1] and D = the sum of all delays (1 if that is 0: the reference's 1 ns rule): t = max(pts_ns - start_pts_ns, 0) mod D (the
 * reference would underflow on a negative difference; the clamp is this library's definition), and the result is the k that minimises
 * |pts_k - t|, the FIRST such k on a tie (Rust's min_by_key).  No wrap-around: near the end of the loop the last frame shows, not frame 0.
 * < 0 on null / n_frames == 0. */
SMR_API int smr_animated_frame_index(const uint64_t *delays_ns, uint32_t n_frames, int64_t pts_ns, int64_t start_pts_ns);
/* scene/transition/{cubic_bezier,bounce}.rs and smelter-api/src/video/color.rs, exported for the parity tests */
SMR_API double smr_cubic_bezier_easing(double progress, double x1, double y1, double x2, double y2);
SMR_API double smr_bounce_easing(double progress);
SMR_API int smr_parse_color(const char *text, uint8_t rgba[4]);

/* ---- a14 (+ a2, a4): the renderer ---------------------------------------------------
 * `Renderer` of smelter-render/src/state.rs:96-252 over the scene engine and the kernels above:
 *   Renderer::new              -> smr_renderer_create (stream_fallback_timeout: state.rs:43-52, render_loop.rs:29)
 *   register_input / unregister_input / unregister_output (state.rs:102-121)
 *   register_renderer(Image)   -> smr_renderer_register_image (bitmap pixels; decoding is the caller's),
 *                                 smr_renderer_register_animated_image (the decoded frames of a GIF and their delays)
 *   register_renderer(Shader)  -> smr_renderer_register_shader (a built-in kernel id), smr_renderer_register_shader_source /
 *                                 _program (a user shader written in HIP C++; WGSL text is out of scope)
 *   register_renderer(WebRenderer) -> smr_renderer_register_web_renderer + smr_renderer_web_paint / _web_positions (the page's pixels and
 *                                 the children's rectangles are the caller's; the node's compositing is here: "WebView nodes" below)
 *   update_scene               -> smr_renderer_update_scene(output_id, resolution, OutputFrameFormat, scene JSON) (state.rs:177-189)
 *   render(FrameSet<InputId>)  -> smr_renderer_render: populate_inputs (stale frames dropped), depth-first walk of every output's
 *                                 render graph (input refs, images, text, shader and nested layout nodes), read_outputs fused
 *                                 into the root layout node (state.rs:220-252, render_loop.rs:19-230)
 * Text nodes: with a font book (smr_renderer_set_fontbook) the renderer lays out, rasterises and draws them itself at every update_scene;
 * without one the caller supplies each Text node's glyph run once after every update_scene (smr_renderer_node_info lists the nodes,
 * smr_renderer_set_text takes the run) — text_renderer.rs renders once per update either way.
 * Output frames live in HBM, two per output, alternating: a returned frame stays valid until the render after the next. */
typedef struct smr_renderer smr_renderer;
typedef struct smr_input_frame {
    const char *input_id;
    const smr_frame *frame; /* resident in HBM (smr_frame_upload or wrapped decoder output) */
    int64_t pts_ns;
} smr_input_frame;
typedef struct smr_output_frame {
    const char *output_id;
    const smr_frame *frame; /* owned by the renderer; valid until the lane that rendered it has rendered two more frames */
    smr_ctx *ctx;           /* the context (stream) the frame's GPU work was issued on: sync / download through this one */
} smr_output_frame;

SMR_API int smr_renderer_create(smr_ctx *ctx, int64_t stream_fallback_timeout_ns /* < 0: 500 ms */, smr_renderer **out);
SMR_API void smr_renderer_destroy(smr_renderer *r);
SMR_API const char *smr_renderer_last_error(const smr_renderer *r);
SMR_API int smr_renderer_register_input(smr_renderer *r, const char *input_id);
SMR_API int smr_renderer_unregister_input(smr_renderer *r, const char *input_id);
SMR_API int smr_renderer_register_image(smr_renderer *r, const char *image_id, const uint8_t *rgba_straight, uint32_t width, uint32_t height);
/* AnimatedAsset::new (transformations/image/animated_image.rs:41-118): n_frames straight-alpha RGBA8 frames of width x height, tightly
 * packed one after the other, and their delays.  Every frame is premultiplied once, here, and kept on the renderer's own context; an Image
 * node of this asset shows, at every render, frame smr_animated_frame_index(delays_ns, n_frames, pts, the node's start_pts) — at its own size
 * the frame itself, at another size the frame drawn into the node's resolution by the image pass.  SMR_ERR_INVALID: n_frames == 0 ("Animated
 * image does not contain any frames."), n_frames > 1000 ("Detected over 1000 frames inside the animated image. This case is not currently
 * supported."), a delay sum above INT64_MAX, and whatever smr_renderer_register_image refuses (null arguments, a zero size, an id that
 * names a static or animated image already).  n_frames == 1 registers exactly what smr_renderer_register_image would (the reference's
 * SingleFrame fallback; the delay is ignored).  A failed allocation is SMR_ERR_OOM and registers nothing. */
SMR_API int smr_renderer_register_animated_image(smr_renderer *r, const char *image_id, const uint8_t *rgba_straight_frames,
                                                 uint32_t width, uint32_t height, uint32_t n_frames, const uint64_t *delays_ns);
/* Launches of the image pass so far, all lanes (which path drew the Image nodes is observable without a kernel counter slot).  The image
 * pass runs once per output and render, before the graph walk: every Image node whose size differs from its asset's is drawn into the
 * node's resolution — animated assets at every render, static ones once per node surface — by ONE launch per 16 such nodes. */
SMR_API int smr_renderer_image_launches(const smr_renderer *r, uint64_t *count);
/* SVG image assets: SvgAsset (transformations/image/svg_image.rs) without the vector library.  Parsing and rasterising stay the caller's — a
 * host that owns resvg registers the tree's size and a callback; "decoding is the caller's", as for bitmaps and the browser.  Everything
 * after the pixmap exists is the library's: when to rasterise, at which size, the colour fix-up, caching, the node's place in the graph.
 *   smr_renderer_register_svg_image: width / height are SvgAsset::resolution() — tree.size truncated (svg_image.rs:89-94) — and size Image
 *     nodes exactly as a bitmap's do (scene/image_component.rs:67-89, integer aspect ratio included).  SMR_ERR_INVALID: whatever
 *     smr_renderer_register_image refuses (null arguments, a zero size, an id that names a static, animated or SVG image already) and a
 *     null fn.  Nothing is rasterised at registration.
 *   fn runs only inside smr_renderer_update_scene, on the calling thread, never from smr_renderer_render: once for every (SVG asset, node
 *     width, node height) the new scene needs and no resident raster covers — the reference rasterises at the NODE's resolution
 *     (svg_image.rs:262-292, scale = node size / tree size), it does not rescale a bitmap —, after the definition has been validated and
 *     before the new scene becomes active.  The buffer is pinned staging (smr_host_alloc), tight (pitch_bytes == 4 * width) and zero-filled.
 *     A non-zero return refuses the update as a whole, like a validation error (SMR_ERR_INVALID): the previous scene stays active,
 *     smr_renderer_last_error names the image and the size, and what was rasterised for the refused update is released.  So does a staging
 *     or raster allocation that fails (SMR_ERR_OOM), and a node above MAX_NODE_RESOLUTION.  A node of zero width or height gets no call and
 *     samples transparent.  fn MUST NOT call into the same renderer.
 *   After all calls of one update every new pixmap is uploaded into an RGBA8 surface of the node's size on the renderer's own context and
 *     fixed up in place — un-premultiplied through the linear view, quantised to 8 bits, premultiplied through the sRGB view
 *     (svg_image.rs:120-167) — by ONE k_svg_nodes launch per 16 new rasters in SMR_MODE_GPU_OPTIMIZED, and by none in
 *     SMR_MODE_CPU_OPTIMIZED, where the pixmap's bytes are the node's (svg_image.rs:73-76); one smr_sync follows.  A pixmap whose alpha is 255
 *     everywhere is handed on as an opaque layer.  Rasters are keyed by (registration, width, height) and shared by all nodes, outputs and
 *     lanes of that size; the node never goes through the image pass (smr_renderer_image_launches does not move).  A raster that no active
 *     scene of any output shows after an update (or smr_renderer_unregister_output) is released, once frames in flight are done with it.
 *     With shards, Image nodes render on the root, as ever.
 *   smr_renderer_unregister_image: unregister_renderer(id, RegistryType::Image) (state.rs:154-171) for static, animated and SVG images
 *     alike.  Refused (SMR_ERR_INVALID) while an active scene uses the id; an unknown id is not an error.  Frees the asset's surfaces and
 *     rasters; after it returns fn is never called for that id again, and the id may be registered anew.
 *   smr_renderer_svg_stats: calls of fn so far, k_svg_nodes launches so far, rasters resident now (no kernel counter slot, like
 *     smr_renderer_image_launches).  Any out-pointer may be null.
 * Out of scope: parsing or rasterising SVG in the library; re-rasterising while a parent Rescaler animates (the reference does not either:
 * the node's size is the component's); WebGl mode. */
/* Rasterise image `image_id` at width x height into `rgba`: premultiplied, gamma-encoded RGBA8, rows pitch_bytes apart, zero-filled by the
 * library before the call — what render_to_texture (svg_image.rs:262-292) leaves in its BytesMut.  0 = done; anything else fails the update. */
typedef int (*smr_svg_rasterise_fn)(void *user, const char *image_id, uint32_t width, uint32_t height, uint8_t *rgba, size_t pitch_bytes);
SMR_API int smr_renderer_register_svg_image(smr_renderer *r, const char *image_id, uint32_t width, uint32_t height,
                                            smr_svg_rasterise_fn fn, void *user);
SMR_API int smr_renderer_unregister_image(smr_renderer *r, const char *image_id);
SMR_API int smr_renderer_svg_stats(const smr_renderer *r, uint64_t *rasterise_calls, uint64_t *launches, uint32_t *resident);
/* WebView nodes: the compositing half of the reference's web renderer (transformations/web_renderer/renderer.rs:78-134, shader.rs:53-114,
 * render_website.wgsl).  The browser is the caller's — no CEF, no process, no shared memory here: a host that
 * owns one registers an instance, hands over the latest paint and the latest rectangles of the children, and a `web_view` component of that
 * instance draws.  "Decoding is the caller's", as for images.
 *   register_renderer(WebRenderer)  -> smr_renderer_register_web_renderer: WebRendererSpec's resolution and embedding_method
 *                                      (web_renderer.rs; renderer.rs:43-76).  SMR_ERR_INVALID: a null or registered id, a zero size, a size
 *                                      above MAX_NODE_RESOLUTION (7682 x 4320, types.rs:146-149), an unknown method.
 *   RenderHandler::on_paint         -> smr_renderer_web_paint (browser_client.rs:96-130): width x height premultiplied BGRA8 texels in caller
 *                                      memory, rows pitch_bytes apart (0 = tight; below 4 * width is refused).  The bitmap is copied before
 *                                      the call returns, into pinned staging (smr_host_alloc); each lane uploads it with a stream-ordered copy
 *                                      (smr_frame_upload_async's) at its next render of the node when its own copy is older.  The latest
 *                                      paint wins; nothing blocks the host.
 *   GET_FRAME_POSITIONS' reply      -> smr_renderer_web_positions (browser_client.rs:60-93): one rectangle per child in child order, in page
 *                                      pixels, axis-aligned (the reference's always are: rotation_degrees: 0.0).  n may be 0.
 * Until the first paint the node has no texture (renderer.rs:89, retrieve_frame) and its parent samples transparent.  After one, every
 * render redraws the node at the instance's resolution: children zipped with the rectangles (renderer.rs:105-114: a child beyond n is not
 * drawn, a rectangle beyond the children is ignored, before the first smr_renderer_web_positions nothing but the page is), layered by the
 * embedding method (renderer.rs:119-131): over content — page, then children in order; under content — children, then the page; Chromium
 * embedding — the page alone (sending the children's pixels to the browser is out of scope; they are still rendered by the graph walk).
 * The first layer lands on a transparent target, every later one is blended with PREMULTIPLIED_ALPHA_BLENDING onto the 8-bit target — by
 * ONE launch per node and 16 children (k_web_view) where the reference makes a render pass per layer.  A child covers pixel (px, py) iff
 * x <= px + 0.5 < x + width and likewise in y; it is sampled bilinearly, clamped to its edge.  Input-stream children become node textures
 * first, as a Shader's do; a child without a texture draws nothing.  The node renders on the renderer's own context (lanes keep a page copy
 * each; with shards it is the root), in both rendering modes, and its output is never treated as opaque.
 * smr_renderer_unregister_web_renderer is refused while a scene uses the instance. */
typedef enum smr_web_embedding {
    SMR_WEB_CHROMIUM_EMBEDDING = 0,   /* WebEmbeddingMethod::ChromiumEmbedding */
    SMR_WEB_NATIVE_OVER_CONTENT = 1,  /* WebEmbeddingMethod::NativeEmbeddingOverContent */
    SMR_WEB_NATIVE_UNDER_CONTENT = 2  /* WebEmbeddingMethod::NativeEmbeddingUnderContent */
} smr_web_embedding;
typedef struct smr_web_rect {
    float x, y, width, height; /* getBoundingClientRect of the child's element, page pixels */
} smr_web_rect;
SMR_API int smr_renderer_register_web_renderer(smr_renderer *r, const char *instance_id, uint32_t width, uint32_t height, uint32_t embedding);
SMR_API int smr_renderer_unregister_web_renderer(smr_renderer *r, const char *instance_id);
SMR_API int smr_renderer_web_paint(smr_renderer *r, const char *instance_id, const uint8_t *bgra_premultiplied, size_t pitch_bytes);
SMR_API int smr_renderer_web_positions(smr_renderer *r, const char *instance_id, const smr_web_rect *rects, uint32_t n);
/* k_web_view launches so far, all lanes: one per WebView node and render with up to 16 children, one more per further 16 (modelled on
 * smr_renderer_image_launches: no kernel counter slot). */
SMR_API int smr_renderer_web_launches(const smr_renderer *r, uint64_t *count);
SMR_API int smr_renderer_register_shader(smr_renderer *r, const char *shader_id, uint32_t builtin_id);
/* A user shader ("user shaders" above) under `shader_id`; registering an id again replaces what it named (built-in or not).
 * _source compiles (blocking, host only) and the renderer owns the program; a source that does not compile fails with the status of
 * smr_shader_program_create, the compiler's log in smr_renderer_last_error (RegisterRendererError), and the registry unchanged.
 * _program registers a compiled program the caller keeps: it must outlive the registration (until the id is re-registered or the
 * renderer destroyed).  Works with lanes and shards (Shader nodes render on the renderer's own context) and in both rendering modes;
 * a user shader's output is never treated as opaque. */
SMR_API int smr_renderer_register_shader_source(smr_renderer *r, const char *shader_id, const char *hip_source);
SMR_API int smr_renderer_register_shader_program(smr_renderer *r, const char *shader_id, const smr_shader_program *p);
/* An update is refused as a whole — the previous scene stays active — for everything the scene definition can get wrong: validation errors,
 * unknown shader ids, (with a font book) Text nodes no run can be made of (empty font book, text that is not UTF-8, absurd sizes), and an
 * SVG asset's raster that could not be made (the rasteriser said no, or an allocation failed: "SVG image assets" above).  One
 * failure is reported AFTER the new scene is in place: a device allocation that fails while the output's frames or a Text node's surface are
 * created (SMR_ERR_OOM): the new scene is active, the nodes that could not be drawn render transparent.
 * output_format: SMR_FRAME_PLANAR_YUV420 / _YUV422 / _YUV444, SMR_FRAME_NV12, SMR_FRAME_RGBA, or packed 4:2:2 — SMR_FRAME_UYVY422 /
 * SMR_FRAME_YUYV422, an even `width` only (see smr_frame_format).  Anything else — a 10-bit format, a matrix tag, an odd width of a packed
 * format — is refused like a scene error: the previous scene stays active. */
SMR_API int smr_renderer_update_scene(smr_renderer *r, const char *output_id, uint32_t width, uint32_t height, uint32_t output_format,
                                      const char *scene_json);
SMR_API int smr_renderer_unregister_output(smr_renderer *r, const char *output_id);
SMR_API int smr_renderer_node_count(const smr_renderer *r, const char *output_id);
SMR_API int smr_renderer_node_info(smr_renderer *r, const char *output_id, int node, smr_scene_node *out);
SMR_API int smr_renderer_set_text_measurer(smr_renderer *r, smr_text_measure_fn fn, void *user);
/* TextRendererCtx for this renderer: with a font book (not owned; it must outlive the renderer) fitted Text nodes are measured with it
 * and EVERY Text node is laid out, rasterised and drawn by smr_renderer_update_scene itself — once per update, as
 * TextRendererNode::render does — in the node's colour over its background_color.  smr_renderer_set_text still replaces a node's run.
 * NULL detaches the book (and its measurer). */
SMR_API int smr_renderer_set_fontbook(smr_renderer *r, smr_fontbook *book);
/* Text nodes: cached rasters (with a font book).  What smr_renderer_update_scene draws of a Text node depends on the component alone, so the
 * renderer keeps it: a raster is keyed by text, font_family, style, weight, wrap, align, font_size, line_height, the node's width x height,
 * the text colour and the background colour (the scene's bytes) and the font book — a generation that smr_renderer_set_fontbook bumps,
 * together with smr_fontbook_count — and shared by every node, output and lane that shows that key.
 *   smr_renderer_update_scene: a node whose raster is resident points at it; every MISSING key is rasterised once (smr_fontbook_rasterise),
 *     however many nodes share it, and all new rasters are drawn on the renderer's own context from ONE upload by ONE k_text_nodes launch
 *     per 16 rasters and ONE synchronisation (each workgroup looks only at the glyphs that touch its 64 x 16 tile), in both rendering
 *     modes.  An update that changes one label of forty rasterises, uploads and draws one.  A raster that no active scene of any output
 *     shows after an update (or smr_renderer_unregister_output) is released, once frames in flight are done with it.
 *   smr_renderer_set_text (the caller's own shaper): the node gets a surface of its OWN, never a cached one — a raster it shared stays as
 *     it is for the other nodes —, drawn by the same kernel with one job.  After an update the caller supplies its runs again, as ever.
 *   smr_renderer_set_fontbook: rasters made with the previous book are not reused; they go as their scenes are replaced.
 *   smr_renderer_text_stats: smr_fontbook_rasterise calls so far, k_text_nodes launches so far (smr_renderer_set_text's included), rasters
 *     resident now (no kernel counter slot, like smr_renderer_svg_stats).  Any out-pointer may be null.
 * Hosts need change nothing: the pixels are those of one smr_blit_glyphs call per node, which is what the renderer made before.  Errors
 * are as stated at smr_renderer_update_scene below.  Out of scope: glyph shapes and shaping; a device-resident glyph atlas across runs. */
SMR_API int smr_renderer_text_stats(const smr_renderer *r, uint64_t *rasterise_calls, uint64_t *launches, uint32_t *resident);
SMR_API int smr_renderer_set_text(smr_renderer *r, const char *output_id, int node, const float bg[4], const smr_glyph *glyphs, uint32_t n,
                                  const uint8_t *atlas_host, uint32_t atlas_w, uint32_t atlas_h);
SMR_API int smr_renderer_render(smr_renderer *r, int64_t pts_ns, const smr_input_frame *inputs, uint32_t n_inputs,
                                smr_output_frame *outputs, uint32_t cap, uint32_t *n_outputs);
/* Frames in flight.  The reference submits one frame at a time (one wgpu queue); here a renderer may own several lanes — extra
 * contexts on the same device (own HIP stream, own scratch).  Consecutive smr_renderer_render calls rotate through the lanes, so
 * the latency-bound tail of one frame overlaps the next frame's kernels, while the scene stays ONE state: one update_scene call,
 * one pts sequence, transitions identical to the single-lane renderer.  Each lane keeps its own pair of output frames and node
 * surfaces; smr_output_frame.ctx says which context produced a frame.  smr_renderer_sync waits for every lane. */
SMR_API int smr_renderer_add_lane(smr_renderer *r, smr_ctx *ctx);
/* Inputs sharded over several contexts — usually one per device — behind the one renderer (the library's scaling axis beyond a single
 * GPU: SURVEY.md section 8e).  Per layout node and frame every remote input that exactly one texture layout resamples becomes its dst-sized
 * tile on the context that owns it (smr_ingest_resample_batch, one call per owner), the tiles are gathered on the renderer's own context
 * (smr_gather_tiles over a local communicator the renderer creates: one k_move_rects launch per owner) and composed there; an input that
 * does not fit that rule (1:1, sampled twice, a Shader node's child, the output's root, SMR_MODE_CPU_OPTIMIZED, a frame with an alpha channel,
 * a one-axis or box-pre-reduced resample plan: those the owner would not run on the root's route) has its raw planes moved
 * to a root-resident frame by the same gather.  Every scene renders to the bytes the single-context renderer produces; smr_renderer_render
 * keeps its meaning (the frame of THIS pts, nothing blocks the host, smr_output_frame.ctx is the renderer's own context) and
 * smr_renderer_sync also waits for the shards.  Contexts on the root's own device get SMR_OPT_SHARED_DEVICE.
 * Lanes and shards do not combine: smr_renderer_add_shard on a renderer with lanes and smr_renderer_add_lane on one with shards fail. */
/* A further context (usually another device) that takes a share of the renderer's inputs.  Call before the first
 * smr_renderer_register_input.  Same rendering mode as the renderer's context, else refused. */
SMR_API int smr_renderer_add_shard(smr_renderer *r, smr_ctx *ctx);
/* The context an input's frames must be resident on (smr_frame_create / upload / wrap there).  k-th registered input ->
 * context k mod N of {the renderer's own, shards in the order added}; fixed until the input is unregistered. */
SMR_API int smr_renderer_input_ctx(smr_renderer *r, const char *input_id, smr_ctx **out);
SMR_API int smr_renderer_sync(smr_renderer *r);

/* ABI version: a host checks smr_abi_version() == SMR_ABI_VERSION when it loads the library.
 *   1  rounds 1 - 4.
 *   2  SMR_INGEST_MFMA_F16_FUSED (ingest implementation 5, the fused one-code-per-stage conversion) left the product enum: a product build
 *      rejects 5, a laboratory build (smr_build_flags() & 1) keeps it under an internal name.  Kernel counter slot 2, once
 *      SMR_KERNEL_INGEST_MFMA_WG, counts SMR_KERNEL_FRAME_TO_RGBA_420.  smr_text_params moved in front of the font-book entry points.  The
 *      SMR_CONVERT_GENERAL / SMR_DISABLE_FUSED / SMR_COMPOSE_SELECT environment knobs are smr_ctx_set_option options in a product build
 *      (the environment is read by laboratory builds only).
 *      Added since, without a new version (additions only: nothing a version-2 host calls changed) — the latest first: packed 4:2:2
 *      OUTPUT frames (SMR_FRAME_UYVY422 / SMR_FRAME_YUYV422 where a frame is an output: two values every version-2 host was refused; no new
 *      symbol, struct, option or kernel counter slot, no frame that was accepted before is converted differently); input colour
 *      matrices (smr_color_matrix, SMR_FRAME_WITH_MATRIX / _BASE_FORMAT / _MATRIX: bits 8 - 11 of smr_frame.format, which every version-2
 *      host leaves zero = BT.709; no struct changed, no kernel counter slot was added, no untagged frame converts differently); then, oldest
 *      first: SMR_KERNEL_MOVE_RECTS (counter slot 8),
 *      SMR_KERNEL_INGEST_WAVE_DIRECT (counter slot 9),
 *      smr_renderer_add_shard, smr_renderer_input_ctx; user shaders (smr_shader_program_*, smr_user_shader,
 *      smr_renderer_register_shader_source / _program); in the user-shader language, no new C symbol: the affine vertex stage
 *      (smr_affine, smr_vertex_affine under SMR_HAS_VERTEX_AFFINE), smr_load and smr_dimensions; the clip vertex stage (smr_clip_vertex,
 *      smr_vertex_clip under SMR_HAS_VERTEX_CLIP: perspective and per-vertex tex_coords, drawn as two triangles); varyings (SMR_VARYINGS,
 *      SMR_VARYINGS_FLAT, SMR_VARYINGS_LINEAR, smr_clip_vertex_v<N>, smr_varyings<N>, the float4 position); screen-space derivatives
 *      (SMR_DERIVATIVES: smr_dpdx, smr_dpdy, smr_fwidth and their _fine / _coarse forms, on 2 x 2 pixel quads with helper invocations):
 *      again no new C symbol — UserShaderArgs, smr_user_shader and its launch, the renderer's registry and the bindings are unchanged;
 *      animated images (smr_renderer_register_animated_image, smr_animated_frame_index, smr_scene_node_start_pts,
 *      smr_renderer_image_launches: no struct changed, smr_scene_node keeps its layout, no kernel counter slot was added);
 *      WebView nodes (smr_scene_register_web_renderer, smr_renderer_register_web_renderer / _unregister_web_renderer, smr_renderer_web_paint,
 *      smr_renderer_web_positions, smr_renderer_web_launches, smr_web_rect, smr_web_embedding, SMR_NODE_WEB_VIEW = 5: a node kind no
 *      version-2 scene could produce — `web_view` was refused —, no struct changed, no kernel counter slot was added);
 *      SVG image assets and image unregistration (smr_svg_rasterise_fn, smr_renderer_register_svg_image, smr_renderer_unregister_image,
 *      smr_renderer_svg_stats: no struct changed, no kernel counter slot was added, no existing scene renders differently);
 *      the Text raster cache (smr_renderer_text_stats: no struct changed, no kernel counter slot was added, no existing scene renders
 *      differently);
 *      10-bit 4:2:0 input frames (SMR_PX_R16, SMR_PX_RG16, SMR_FRAME_P010, SMR_FRAME_PLANAR_YUV420P10: input only, no struct changed, no
 *      kernel counter slot was added, no 8-bit frame converts differently);
 *      10-bit 4:2:2 input frames (SMR_FRAME_PLANAR_YUV422P10, SMR_FRAME_P210, SMR_FRAME_V210: likewise).
 * The two removed names are kept as macros that do not compile, so that a source written against version 1 fails where it uses them
 * instead of silently meaning something else. */
#define SMR_ABI_VERSION 2
#define SMR_INGEST_MFMA_F16_FUSED SMR_REMOVED_IN_ABI_2__the_fused_conversion_is_a_laboratory_route__use_SMR_INGEST_AUTO
#define SMR_KERNEL_INGEST_MFMA_WG SMR_REMOVED_IN_ABI_2__slot_2_counts_SMR_KERNEL_FRAME_TO_RGBA_420
SMR_API uint32_t smr_abi_version(void);
/* bit 0: a laboratory build (-DSMR_LAB: environment knobs, the fused-conversion route, profiling hooks); 0 for a product build */
SMR_API uint32_t smr_build_flags(void);
SMR_API uint32_t smr_sizeof_layout(void);

#ifdef __cplusplus
}
#endif
#endif /* SMR_H */
