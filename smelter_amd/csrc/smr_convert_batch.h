// smr_convert_batch.h — what every block converter of input frames shares (smr_convert_420.h: 8-bit 4:2:0; smr_convert_hi.h: 10-bit 4:2:0;
// smr_convert_hi422.h: 10-bit 4:2:2): the jobs of a launch and their partition (ConvJob, ConvBatch, cv_plan), a wave's walk over its share
// (cv_share_walk), the pixel tail — chroma range expansion, matrix, x * 255 + 0.5 (cv_chroma_expand, cv_pixel) — and a row's way out
// (cv_row_bytes_*, cv_pack_row, CvStoreNode).  Compiled for the CPU by the emulator's drivers (tests/emu/emu_convert*.cpp), the very source.
#pragma once

#include "smr_convert_dev.h"

#ifdef SMR_EMU
#define cv_perm(hi, lo, sel) dev_perm((hi), (lo), (sel))
#define cv_alignbyte(hi, lo, sh) dev_alignbyte((hi), (lo), (sh))
#define cv_clamp01(x) dev_fmed3((x), 0.0f, 1.0f)
#define cv_mad24(a, b, c) dev_mad24((a), (b), (c))
#define cv_uniform(x) (x)
#else
#define cv_uniform(x) __builtin_amdgcn_readfirstlane(x)  // a value every lane of the wave holds alike, moved to a scalar register
#define cv_perm(hi, lo, sel) __builtin_amdgcn_perm((hi), (lo), (sel))
#define cv_alignbyte(hi, lo, sh) __builtin_amdgcn_alignbyte((hi), (lo), (sh))
#define cv_clamp01(x) __builtin_amdgcn_fmed3f((x), 0.0f, 1.0f)
#define cv_mad24(a, b, c) ((u32)__umul24((a), (b)) + (c))  // row * pitch + offset with both factors below 2^24: one full-rate v_mad_u32_u24 (a 32 x 32 multiply is a quarter-rate v_mad_u64_u32)
#endif

// ---- the unorm8 store of a row's twelve values: floor(clamp(x, 0, 1) * 255 + 0.5) (planar_yuv_to_rgba.wgsl:57 through the Rgba8Unorm target).
// v_cvt_pk_u8_f32 converts, saturates to [0, 255] and inserts the byte into a dword in ONE instruction — with the wave's f32 rounding mode:
// round-to-nearest-even by default (tools/ubench/cvt_pk_u8.hip: not the reference's truncation), but under round-toward-zero exactly the
// truncation (tools/ubench/cvt_pk_u8_mode.hip on the device: every f32 within 4 ulp of every integer and half-integer of [0, 258), a sweep of
// [-2, 298] and the specials — 4.2 M values, no difference from trunc(clamp(x, 0, 255))).  The operands t = x * 255 + 0.5 are computed before, in the
// default mode, WITHOUT the clamp (t <= 0.5 truncates / saturates to 0 like clamp's 0.5, t >= 255.5 saturates to 255 like clamp's 255.5; NaN
// cannot occur); the mode is switched inside one asm block around the twelve conversions, so no other float instruction can be scheduled into
// the switched region.  Three instructions per value (multiply, add, convert) instead of five (median, multiply, add, convert, shift-or).
// dst[c] |= byte i of channel c for the row's pixel i: RGB12 rows are (R x 4, G x 4, B x 4) dwords; RGBA8 rows take cv_store_px.
#ifdef SMR_EMU
static inline u32 cv_emu_u8(float t) { return t >= 255.0f ? 255u : (t > 0.0f ? (u32)t : 0u); }
#define CV_U8X4(d, t0, t1, t2, t3) do { (d) = cv_emu_u8(t0) | (cv_emu_u8(t1) << 8) | (cv_emu_u8(t2) << 16) | (cv_emu_u8(t3) << 24); } while (0)
static inline void cv_row_bytes_planar(const float (&t)[3][4], u32 &r4, u32 &g4, u32 &b4) {
    CV_U8X4(r4, t[0][0], t[0][1], t[0][2], t[0][3]); CV_U8X4(g4, t[1][0], t[1][1], t[1][2], t[1][3]); CV_U8X4(b4, t[2][0], t[2][1], t[2][2], t[2][3]);
}
static inline void cv_row_bytes_packed(const float (&t)[3][4], u32 (&px)[4]) {
    for (int i = 0; i < 4; i++) px[i] = cv_emu_u8(t[0][i]) | (cv_emu_u8(t[1][i]) << 8) | (cv_emu_u8(t[2][i]) << 16) | 0xff000000u;
}
#else
__device__ __forceinline__ void cv_row_bytes_planar(const float (&t)[3][4], u32 &r4, u32 &g4, u32 &b4) {
    u32 r = 0u, g = 0u, b = 0u;
    asm volatile("s_setreg_imm32_b32 hwreg(HW_REG_MODE, 0, 2), 3\n\ts_nop 1\n\t"
                 "v_cvt_pk_u8_f32 %0, %3, 0, %0\n\tv_cvt_pk_u8_f32 %1, %7, 0, %1\n\tv_cvt_pk_u8_f32 %2, %11, 0, %2\n\t"
                 "v_cvt_pk_u8_f32 %0, %4, 1, %0\n\tv_cvt_pk_u8_f32 %1, %8, 1, %1\n\tv_cvt_pk_u8_f32 %2, %12, 1, %2\n\t"
                 "v_cvt_pk_u8_f32 %0, %5, 2, %0\n\tv_cvt_pk_u8_f32 %1, %9, 2, %1\n\tv_cvt_pk_u8_f32 %2, %13, 2, %2\n\t"
                 "v_cvt_pk_u8_f32 %0, %6, 3, %0\n\tv_cvt_pk_u8_f32 %1, %10, 3, %1\n\tv_cvt_pk_u8_f32 %2, %14, 3, %2\n\t"
                 "s_setreg_imm32_b32 hwreg(HW_REG_MODE, 0, 2), 0\n\ts_nop 1"
                 : "+v"(r), "+v"(g), "+v"(b)
                 : "v"(t[0][0]), "v"(t[0][1]), "v"(t[0][2]), "v"(t[0][3]), "v"(t[1][0]), "v"(t[1][1]), "v"(t[1][2]), "v"(t[1][3]), "v"(t[2][0]), "v"(t[2][1]),
                   "v"(t[2][2]), "v"(t[2][3]));
    r4 = r; g4 = g; b4 = b;
}
__device__ __forceinline__ void cv_row_bytes_packed(const float (&t)[3][4], u32 (&px)[4]) {
    u32 p0 = 0xff000000u, p1 = 0xff000000u, p2 = 0xff000000u, p3 = 0xff000000u;
    asm volatile("s_setreg_imm32_b32 hwreg(HW_REG_MODE, 0, 2), 3\n\ts_nop 1\n\t"
                 "v_cvt_pk_u8_f32 %0, %4, 0, %0\n\tv_cvt_pk_u8_f32 %1, %5, 0, %1\n\tv_cvt_pk_u8_f32 %2, %6, 0, %2\n\tv_cvt_pk_u8_f32 %3, %7, 0, %3\n\t"
                 "v_cvt_pk_u8_f32 %0, %8, 1, %0\n\tv_cvt_pk_u8_f32 %1, %9, 1, %1\n\tv_cvt_pk_u8_f32 %2, %10, 1, %2\n\tv_cvt_pk_u8_f32 %3, %11, 1, %3\n\t"
                 "v_cvt_pk_u8_f32 %0, %12, 2, %0\n\tv_cvt_pk_u8_f32 %1, %13, 2, %1\n\tv_cvt_pk_u8_f32 %2, %14, 2, %2\n\tv_cvt_pk_u8_f32 %3, %15, 2, %3\n\t"
                 "s_setreg_imm32_b32 hwreg(HW_REG_MODE, 0, 2), 0\n\ts_nop 1"
                 : "+v"(p0), "+v"(p1), "+v"(p2), "+v"(p3)
                 : "v"(t[0][0]), "v"(t[0][1]), "v"(t[0][2]), "v"(t[0][3]), "v"(t[1][0]), "v"(t[1][1]), "v"(t[1][2]), "v"(t[1][3]), "v"(t[2][0]), "v"(t[2][1]),
                   "v"(t[2][2]), "v"(t[2][3]));
    px[0] = p0; px[1] = p1; px[2] = p2; px[3] = p3;
}
#endif

struct ConvJob {
    SurfView yp, up, vp, dst;
    int full, nv;  // full range (J420) | NV12 (interleaved chroma in `up`)
    int sx, sy;    // chroma subsampling: 4:2:0 = (1, 1), 4:2:2 = (1, 0), 4:4:4 = (0, 0)
    int rgb12;     // the block converters only: dst is an R8 surface of 3 w x h — the node texture as 12-byte groups of four pixels (R x 4, G x 4, B x 4)
    int packed;    // 0 planar / NV12 | 1 UYVY | 2 YUYV: `yp` is the (w / 2) x h plane of U Y0 V Y1 / Y0 U Y1 V groups | 3 BGRA | 4 ARGB: `yp` is the w x h plane, bytes permuted (bgra_to_rgba.wgsl / argb_to_rgba.wgsl:24-28)
    int matrix;    // smr_color_matrix of the frame (0 = BT.709, what a zeroed job means).  k_yuv420_to_rgba[_tight] do NOT read it: their matrix is a template parameter and the host queues their jobs per matrix
};
constexpr int MAX_CONV_JOBS = 16;
struct ConvBatch {
    ConvJob j[MAX_CONV_JOBS];
    // The block converters: the launch's work in UNITS — a unit = 64 column groups (256 pixels) x one block row (4 rows) of one job, what a wave
    // computes per step of a run — dealt to the XCDs in BANDS (cv_plan): a band = `band` consecutive block rows of a job across all its
    // column blocks, band g of the launch (jobs one after the other) belongs to XCD g % 8.  Inside an XCD the units are ordered band by band,
    // column block by column block, block rows fastest, and cut into equal contiguous shares, one per wave the XCD runs (workgroup b runs on
    // XCD b % 8 — observed, used for locality only: the partition is arithmetic on blockIdx and complete whatever the placement).
    // Why bands: a column block's chroma window reaches a byte or two into its neighbours' cache lines; neighbours on different XCDs made
    // every L2 fetch three lines for one (counters: 62 MB for 24.9 MB of planes with shares dealt without regard to the XCDs).
    int n;
    u32 band;                                  // block rows per band
    u32 rows[MAX_CONV_JOBS];                   // block rows of job j
    u32 cols[MAX_CONV_JOBS];                   // column blocks of job j
    u32 band0[MAX_CONV_JOBS];                  // launch-wide index of job j's first band
    u32 first_unit[8][MAX_CONV_JOBS + 1];      // per XCD x: job j owns units [first_unit[x][j], first_unit[x][j + 1]) of x's sequence
};

// Fills the partition tables of a launch of n jobs (j[].dst.w / .h set); returns the number of bands (the launch needs at least
// min(8, bands) workgroups: every XCD that owns units must run a wave).
inline u32 cv_plan(ConvBatch &B, int n) {
    B.n = n;
    u32 total = 0;
    for (int j = 0; j < n; j++) {
        B.cols[j] = ((u32)B.j[j].dst.w + 255u) / 256u;
        B.rows[j] = ((u32)B.j[j].dst.h + 3u) / 4u;
        total += B.cols[j] * B.rows[j];
    }
    // Band height: every share of a band runs on the band's XCD whatever its length, so a band may be much taller than a share — and the
    // taller, the fewer chroma rows two XCDs both fetch (a band's window reaches one chroma row into the bands above and below: 2 rows per
    // band of 2 * band).  Against that, the XCDs' totals differ by up to one band: sixteen bands per XCD and more keeps that under a
    // sixteenth (8 x 1080p: bands of 16 block rows, 17 per XCD, 6 % of the chroma rows fetched twice).
    u32 cols_max = 1;
    for (int j = 0; j < n; j++) cols_max = B.cols[j] > cols_max ? B.cols[j] : cols_max;
    const u32 band = total / (128u * cols_max);
    B.band = band < 1u ? 1u : (band > 64u ? 64u : band);
    u32 g = 0;
    for (int x = 0; x < 8; x++) B.first_unit[x][0] = 0;
    for (int j = 0; j < n; j++) {
        B.band0[j] = g;
        const u32 bands = (B.rows[j] + B.band - 1u) / B.band;
        u32 units[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (u32 b = 0; b < bands; b++) {
            const u32 h = B.rows[j] - b * B.band < B.band ? B.rows[j] - b * B.band : B.band;
            units[(g + b) & 7u] += B.cols[j] * h;
        }
        for (int x = 0; x < 8; x++) B.first_unit[x][j + 1] = B.first_unit[x][j] + units[x];
        g += bands;
    }
    return g;
}

// The name and signature the plan had while it lived in smr_convert_420.h (`waves` was never read): emulator drivers written against that
// header keep compiling against this one.
inline u32 cv420_plan(ConvBatch &B, int n, u32 /* waves */) { return cv_plan(B, n); }

#ifndef CV_ABL
#define CV_ABL 0  // laboratory builds (tools/variant.sh NAME -DCV_ABL=n): 1 no stores | 2 no chroma loads | 4 no luma loads | 8 no per-pixel arithmetic
#endif

#ifdef __HIPCC__

// A job's geometry as VALUES in scalar registers.  Read in place (B.j[j].dst.pitch ...) the compiler treats the kernel-argument segment as
// memory it may re-read whenever that is cheaper than keeping a register: it did, behind every row's store — an s_load_dword plus
// s_waitcnt lgkmcnt(0) (scalar loads return out of order, so the wait also drains the table gathers in flight) per row, ~200 cycles
// each, in every wave at once.  A value that went through v_readfirstlane is a computed value: it stays where it is.
__device__ __forceinline__ SurfView cv_view_in_registers(const SurfView &v) {
#ifdef SMR_EMU
    return v;
#else
    SurfView r;
    const unsigned long long p = (unsigned long long)(uintptr_t)v.ptr;
    const u32 lo = cv_uniform((u32)p), hi = cv_uniform((u32)(p >> 32));
    r.ptr = (u8 *)(uintptr_t)(((unsigned long long)hi << 32) | lo);
    r.pitch = cv_uniform(v.pitch);
    r.w = cv_uniform(v.w);
    r.h = cv_uniform(v.h);
    return r;
#endif
}
__device__ __forceinline__ ConvJob cv_job_in_registers(const ConvJob &j) {
    ConvJob J = j;
    J.yp = cv_view_in_registers(j.yp); J.up = cv_view_in_registers(j.up); J.vp = cv_view_in_registers(j.vp); J.dst = cv_view_in_registers(j.dst);
    J.matrix = (int)cv_uniform((u32)j.matrix);  // (read by the 10-bit converters only)
    return J;
}

// Wave `wave` (0 .. 3) of workgroup `block` of a launch of `grid` workgroups: XCD x = block % 8 runs the workgroups x, x + 8, ...; its
// waves cut x's unit sequence (ConvBatch) into equal contiguous shares — total / waves units, the first total % waves waves one more.  A
// share is a vertical run of blocks inside one (band, column block) cell, or the end of a cell and the start of the next (in the next
// band or job, too).  run(J, g, P0, nrun): column group g = col * 64 + lane of job J (its geometry in scalar registers), block rows
// P0 .. P0 + nrun - 1 — called for every run of the share whose column group exists.
template <typename RUN>
__device__ __forceinline__ void cv_share_walk(const ConvBatch &B, u32 block, u32 wave, u32 grid, u32 lane, const RUN &run) {
    const u32 x = block & 7u;
    const u32 waves = ((grid - x + 7u) >> 3) * 4u, w = (block >> 3) * 4u + wave;  // of this XCD
    const u32 total = B.first_unit[x][B.n];
    const u32 share = total / waves, extra = total - share * waves;
    u32 lo = w * share + (w < extra ? w : extra);
    const u32 hi = lo + share + (w < extra ? 1u : 0u);
    int j = 0;
    while (lo < hi) {  // (uniform: one or two runs per share, more only across tiny jobs)
#pragma unroll 1
        while (lo >= B.first_unit[x][j + 1]) j++;
        const ConvJob J = cv_job_in_registers(B.j[j]);
        const u32 rows = B.rows[j], cols = B.cols[j], band = B.band;
        // x's bands of job j: b0, b0 + 8, ...; all but the job's last band (which, if x owns it, is the last of them) hold cols * band units
        const u32 b0 = (x - B.band0[j]) & 7u;
        const u32 local = lo - B.first_unit[x][j];
        const u32 t = local / (cols * band), b = b0 + 8u * t;
        const u32 in_band = local - t * cols * band;
        const u32 band_rows = rows - b * band < band ? rows - b * band : band;
        const u32 col = in_band / band_rows, r = in_band - col * band_rows;
        const u32 nrun = hi - lo < band_rows - r ? hi - lo : band_rows - r;
        const int g = (int)(col * 64u + lane);
        if (4 * g < J.dst.w) run(J, g, (int)(b * band + r), (int)nrun);
        lo += nrun;
    }
}

// ---- the pixel tail: what every block converter does with a pixel's y', u, v, and with a row's twelve values

// planar_yuv_to_rgba.wgsl:47-48: (c - 16/255) / 0.8784, clamp — as RN(a * rc_hi + RN(a * rc_lo)) with rc_hi + rc_lo = 1 / 0.8784 to 48 bits:
// the IEEE quotient for EVERY f32 a in [-16/255, 1] — all 636 524 221 of them checked against the division (tools/check_div_by_constant.py),
// as unorm_of_byte's form is for the 256 bytes.  One multiply and one fused multiply-add; the clamp rides on the FMA's result.  The 10-bit
// operands stay inside that interval: u <= 255.75 / 255 (a lerp of unorm values of codes <= 1023, weights summing to 1, each rounding monotone).
__device__ __forceinline__ void cv_chroma_expand(float &u, float &v) {
    constexpr float kc = 0.87843137254f;
    constexpr float rc_hi = 1.0f / kc, rc_lo = (float)(1.0 / (double)kc - (double)rc_hi);
    const float au = u - (16.0f / 255.0f), av = v - (16.0f / 255.0f);
    u = cv_clamp01(__builtin_fmaf(au, rc_hi, au * rc_lo));
    v = cv_clamp01(__builtin_fmaf(av, rc_hi, av * rc_lo));
}
// x * 255 + 0.5 of a pixel's three values into column i of the row's t (cv_row_bytes_* truncates and packs them)
__device__ __forceinline__ void cv_scale_px(float R, float G, float B, float (&t)[3][4], int i) {
    t[0][i] = R * 255.0f + 0.5f;
    t[1][i] = G * 255.0f + 0.5f;
    t[2][i] = B * 255.0f + 0.5f;
}
// y' (range-expanded already: a table), u, v (FULL: as they are; else range-expanded here) -> the matrix -> column i of t
template <bool FULL>
__device__ __forceinline__ void cv_pixel(float yy, float u, float v, const SmrMatrixCoef &C, float (&t)[3][4], int i) {
    if (!FULL) cv_chroma_expand(u, v);
    const float um = u - 0.5f, vm = v - 0.5f;
    const float R = yy + C.rv * vm;
    const float G = yy - C.gu * um - C.gv * vm;
    const float B = yy + C.bu * um;
    cv_scale_px(R, G, B, t, i);
}

// SINK: where a finished row goes — sink(r, y, r4, g4, b4, px): row r of the block = frame row y, as RGB12 dwords (RGB12) or four RGBA8 pixels.
// CvStoreNode stores into the job's node texture; k_ingest_wave's plane-source builds (smr_ingest_wave.h) hand the rows to LDS instead.
struct CvStoreNode {
    const ConvJob &J;
    int g;
    bool rgb12;
    __device__ __forceinline__ void operator()(int, int y, u32 r4, u32 g4, u32 b4, const u32 (&px)[4]) const {
        if (rgb12) g_st_u32x3(J.dst.ptr + cv_mad24((u32)y, J.dst.pitch, 12u * (u32)g), r4, g4, b4);
        else g_st_u32x4(J.dst.ptr + cv_mad24((u32)y, J.dst.pitch, 16u * (u32)g), make_uint4(px[0], px[1], px[2], px[3]));
    }
};
template <typename SINK>
__device__ __forceinline__ void cv_sink_row(int r, int y, u32 r4, u32 g4, u32 b4, const u32 (&px)[4], const SINK &sink) {
    if ((CV_ABL & 1) && (r4 ^ g4 ^ b4 ^ px[0] ^ px[3]) != 0x12345677u) return;  // (never equal in practice: the values stay live)
    sink(r, y, r4, g4, b4, px);
}
// a row's twelve values t -> its bytes (RGB12: three dwords, else four RGBA8 pixels) -> the sink
template <bool RGB12, typename SINK>
__device__ __forceinline__ void cv_pack_row(const float (&t)[3][4], int r, int y, const SINK &sink) {
    u32 px[4] = {0u, 0u, 0u, 0u}, r4 = 0u, g4 = 0u, b4 = 0u;
    if (RGB12) cv_row_bytes_planar(t, r4, g4, b4);
    else cv_row_bytes_packed(t, px);
    cv_sink_row(r, y, r4, g4, b4, px, sink);
}

#endif  // __HIPCC__
