// smr_convert_hi422.h — the input converter of 10-bit 4:2:2 frames: planar 10-bit (three planes of 16-bit words, the code is the word's LOW
// ten bits; what ProRes 422 / DNxHR / XAVC / H.264 Hi422 decoders write as yuv422p10le), P210 (Y plane of words, interleaved U V words, the
// code is the word's HIGH ten bits) and v210 (an SDI capture card's rows: three codes per dword, six pixels in four dwords).  Included by
// smr_convert.hip (k_yuv422_hi_to_rgba, k_yuv422_hi_to_rgba_any) and, for the CPU, by tests/emu/emu_convert_hi422.cpp (the very source).
//
// The value rule is smr_convert_hi.h's (include/smr.h): a code c has the unorm value (f32(c) * 0.25f) / 255.0f, and from there on
//   * planar and P210 are planar_yuv_to_rgba.wgsl on a 4:2:2 frame as oracle/smr_oracle.c restates it: the chroma planes are w / 2 x h, so
//     the sampler interpolates horizontally (weights .75 / .25, clamp to edge) and takes the texel itself vertically (its vertical fraction
//     is 0 or 1 at every row: top * 1 + bot * 0 is top) — a frame whose codes are 4 b has the node texture of the 8-bit PLANAR_YUV422 frame
//     with bytes b;
//   * v210 is interleaved_uyvy_to_rgba.wgsl: pixel x takes Y[x] and the chroma of pair x / 2, no interpolation, then yuv_to_rgb_store
//     (limited range) — for even widths from 8 a frame whose codes are 4 b has the node texture of the UYVY frame with bytes b.
//
// The block converter has k_yuv420_hi_to_rgba's shape: a thread owns a 4 x 4 pixel block, cv_plan's XCD bands and equal shares, block
// P + 1's loads requested before block P is computed, all of a block's loads in flight before its first store, one 16-byte (RGB12: 12-byte)
// store per thread and row through CvStoreNode, the two 1024-entry tables of cvhi_build_tables.  What differs from 4:2:0 is the fetch:
//   * planar / P210: each of the block's four luma rows has its OWN chroma row — no vertical lerp, nothing carried between blocks.  The
//     window and its horizontal lerps are cvhi_window's and cvhi_hrow's (they never ask for the row count); the load is cvhi_load_chroma's
//     with h rows instead of h / 2;
//   * v210: thread g's pixels 4 g .. 4 g + 3 live in the 16 bytes at byte 32 (g / 3) + 8 (g % 3) of the row — a 12-pixel, 32-byte period
//     against the 4-pixel column groups — which always lie inside the row's 16 ceil(w / 6) bytes.  Which of the twelve 10-bit fields are
//     Y0 .. Y3 and the two chroma pairs depends on g % 3 only: selects, no divergent paths.
// From the chroma values on it is the shared pixel tail and share walk (smr_convert_batch.h), without cvhi_rows's two vertical FMAs.  v210 runs
// the chroma range division and the matrix products once per pixel pair.
//
// ONE MEMORY CONTRACT, for planes the library owns and planes it wraps alike: no byte outside [0, row bytes) of any plane row is requested.
#pragma once

#include "smr_convert_hi.h"

#ifdef __HIPCC__

constexpr int CV422_PLANAR = 0, CV422_P210 = 1, CV422_V210 = 2;

// ---- planar / P210: the pieces of a block

// cvhi_load_chroma with the 4:2:2 row count: chroma row `crow` is luma row `crow`
template <bool P210>
__device__ __forceinline__ CvHiRaw<P210> cv422_load_chroma(const ConvJob &J, const CvHiWin &W, int crow) {
    const int cy = min(crow, J.dst.h - 1);
    CvHiRaw<P210> R;
    const u8 *ur = J.up.ptr + cv_mad24((u32)cy, J.up.pitch, 0u);  // (a plane is far below 4 GiB)
    if (P210) {
#pragma unroll
        for (int k = 0; k < 4; k++) R.d[k] = g_ld_u32(ur + W.off[k]);
    } else {
        const u8 *vr = J.vp.ptr + cv_mad24((u32)cy, J.vp.pitch, 0u);
#pragma unroll
        for (int k = 0; k < 3; k++) { R.d[k] = g_ld_u32(ur + W.off[k]); R.d[3 + k] = g_ld_u32(vr + W.off[k]); }
    }
    return R;
}

// everything block (g, P) reads: four luma rows of 8 bytes, their four chroma windows
template <bool P210>
struct Cv422Blk {
    uint2 y[4];
    CvHiRaw<P210> c[4];
};
template <bool P210>
__device__ __forceinline__ void cv422_load(const ConvJob &J, const CvHiWin &W, int g, int P, Cv422Blk<P210> &K) {
    cvhi_load_luma(J, g, P, K.y);  // (rows behind the frame's last are its last again)
#pragma unroll
    for (int r = 0; r < 4; r++) K.c[r] = cv422_load_chroma<P210>(J, W, 4 * P + r);
}

// The four rows of block (g, P): the row's own horizontal lerps as u and v into the shared pixel tail (limited range).
template <bool P210, bool RGB12, bool ALLROWS>
__device__ __forceinline__ void cv422_rows(const ConvJob &J, int g, int P, const Cv422Blk<P210> &K, const CvHiWin &W, const float *ylut, const float *ulut) {
    const int h = J.dst.h;
    const SmrMatrixCoef C = smr_matrix_coef((u32)J.matrix);  // (uniform, as in cvhi_rows)
    const CvStoreNode sink{J, g, RGB12};
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int y = 4 * P + r;
        if (!ALLROWS && y >= h) break;
        float H[2][4];
        cvhi_hrow<P210>(K.c[r], W, ulut, H);
        u32 yc[4];
        cvhi_row_codes<P210>(K.y[r], yc);
        float t[3][4];
#pragma unroll
        for (int i = 0; i < 4; i++) cv_pixel<false>(ylut[yc[i]], H[0][i], H[1][i], C, t, i);
        cv_pack_row<RGB12>(t, r, y, sink);
    }
}

// A vertical run of blocks: columns 4 g .. 4 g + 3, block rows P0 .. P0 + nb - 1 (those that exist).  Block P + 1's words are requested
// before block P's rows are computed and stored; the run's last block requests nothing.
template <bool P210, bool RGB12>
__device__ __forceinline__ void cv422_run(const ConvJob &J, int g, int P0, int nb, const float *ylut, const float *ulut) {
    const int Pend = min(P0 + nb, (J.dst.h + 3) >> 2);
    if (P0 >= Pend) return;
    const CvHiWin W = cvhi_window<P210>(J, g);
    Cv422Blk<P210> cur;
    cv422_load<P210>(J, W, g, P0, cur);
    int P = P0;
    for (; P + 1 < Pend; P++) {
        Cv422Blk<P210> next;
        cv422_load<P210>(J, W, g, P + 1, next);
        cv422_rows<P210, RGB12, true>(J, g, P, cur, W, ylut, ulut);  // (P + 1 < Pend: not the frame's last block row — all four rows exist)
        cur = next;
    }
    cv422_rows<P210, RGB12, false>(J, g, P, cur, W, ylut, ulut);
}

// ---- v210: the pieces of a block

// the 16 bytes of a row that hold column group g's pixels, as two 8-byte loads (the plane and its pitch are 8-byte aligned: conv_route)
struct Cv210Blk {
    uint2 d[4][2];
};
__device__ __forceinline__ u32 cv210_offset(int g) {
    const u32 period = (u32)g / 3u;
    return 32u * period + 8u * ((u32)g - 3u * period);
}
__device__ __forceinline__ void cv210_load(const ConvJob &J, u32 off, int P, Cv210Blk &K) {
    const int h = J.dst.h;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const u8 *row = J.yp.ptr + cv_mad24((u32)min(4 * P + r, h - 1), J.yp.pitch, off);
        K.d[r][0] = g_ld_u32x2(row);
        K.d[r][1] = g_ld_u32x2(row + 8);
    }
}
// One 10-bit field of the four dwords e: dword da / db / dc at shift sa / sb / sc for g % 3 = 0 / 1 / 2.  The mask comes BEFORE any table
// lookup: whatever the dwords hold (bits 30 - 31 included), the index is < 1024.
__device__ __forceinline__ u32 cv210_field(const u32 (&e)[4], u32 m, int da, u32 sa, int db, u32 sb, int dc, u32 sc) {
    const u32 dw = m == 0u ? e[da] : (m == 1u ? e[db] : e[dc]);
    const u32 sh = m == 0u ? sa : (m == 1u ? sb : sc);  // (of g alone: computed once per run)
    return (dw >> sh) & 0x3ffu;
}
// The twelve pixels of a period in its eight dwords D0 .. D7 (lo mid hi):
//   D0 = Cb0 Y0 Cr0 | D1 = Y1 Cb1 Y2 | D2 = Cr1 Y3 Cb2 | D3 = Y4 Cr2 Y5 | D4 = Cb3 Y6 Cr3 | D5 = Y7 Cb4 Y8 | D6 = Cr4 Y9 Cb5 | D7 = Y10 Cr5 Y11
// and the thread's e0 .. e3 are D0 .. D3 (g % 3 = 0: pixels 0 - 3), D2 .. D5 (1: pixels 4 - 7), D4 .. D7 (2: pixels 8 - 11).
template <bool RGB12, bool ALLROWS>
__device__ __forceinline__ void cv210_rows(const ConvJob &J, int g, u32 m, int P, const Cv210Blk &K, const float *ylut, const float *ulut) {
    const int h = J.dst.h;
    const SmrMatrixCoef C = smr_matrix_coef((u32)J.matrix);  // (uniform, as in cvhi_rows)
    const CvStoreNode sink{J, g, RGB12};
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int y = 4 * P + r;
        if (!ALLROWS && y >= h) break;
        const u32 e[4] = {K.d[r][0].x, K.d[r][0].y, K.d[r][1].x, K.d[r][1].y};
        const u32 yc[4] = {cv210_field(e, m, 0, 10u, 1, 0u, 1, 20u), cv210_field(e, m, 1, 0u, 1, 20u, 2, 10u),
                           cv210_field(e, m, 1, 20u, 2, 10u, 3, 0u), cv210_field(e, m, 2, 10u, 3, 0u, 3, 20u)};
        const u32 cb[2] = {cv210_field(e, m, 0, 0u, 0, 20u, 1, 10u), cv210_field(e, m, 1, 10u, 2, 0u, 2, 20u)};
        const u32 cr[2] = {cv210_field(e, m, 0, 20u, 1, 10u, 2, 0u), cv210_field(e, m, 2, 0u, 2, 20u, 3, 10u)};
        float t[3][4];
#pragma unroll
        for (int p = 0; p < 2; p++) {
            // interleaved_uyvy_to_rgba.wgsl: the pair's own chroma texel (a code's unorm value: inside cv_chroma_expand's proven interval);
            // cv_pixel's statements with the range expansion and the matrix products once per pair
            float u = ulut[cb[p]], v = ulut[cr[p]];
            cv_chroma_expand(u, v);
            const float um = u - 0.5f, vm = v - 0.5f;
            const float rv = C.rv * vm, gu = C.gu * um, gv = C.gv * vm, bu = C.bu * um;
#pragma unroll
            for (int i = 2 * p; i < 2 * p + 2; i++) {
                const float yy = ylut[yc[i]];
                cv_scale_px(yy + rv, yy - gu - gv, yy + bu, t, i);
            }
        }
        cv_pack_row<RGB12>(t, r, y, sink);
    }
}
template <bool RGB12>
__device__ __forceinline__ void cv210_run(const ConvJob &J, int g, int P0, int nb, const float *ylut, const float *ulut) {
    const int Pend = min(P0 + nb, (J.dst.h + 3) >> 2);
    if (P0 >= Pend) return;
    const u32 off = cv210_offset(g), m = (off >> 3) & 3u;  // (8 (g % 3) is the offset's bits 3 - 4)
    Cv210Blk cur;
    cv210_load(J, off, P0, cur);
    int P = P0;
    for (; P + 1 < Pend; P++) {
        Cv210Blk next;
        cv210_load(J, off, P + 1, next);
        cv210_rows<RGB12, true>(J, g, m, P, cur, ylut, ulut);
        cur = next;
    }
    cv210_rows<RGB12, false>(J, g, m, P, cur, ylut, ulut);
}

// a wave's share of a launch (cv_share_walk) over cv422_run / cv210_run
template <int LAYOUT>
__device__ __forceinline__ void cv422_share(const ConvBatch &B, u32 block, u32 wave, u32 grid, u32 lane, const float *ylut, const float *ulut) {
    cv_share_walk(B, block, wave, grid, lane, [&](const ConvJob &J, int g, int P0, int nrun) {
        if (LAYOUT == CV422_V210) {
            if (J.rgb12) cv210_run<true>(J, g, P0, nrun, ylut, ulut);
            else cv210_run<false>(J, g, P0, nrun, ylut, ulut);
        } else {
            if (J.rgb12) cv422_run<LAYOUT == CV422_P210, true>(J, g, P0, nrun, ylut, ulut);
            else cv422_run<LAYOUT == CV422_P210, false>(J, g, P0, nrun, ylut, ulut);
        }
    });
}

// ---- v210, any geometry: one pixel.  interleaved_uyvy_to_rgba.wgsl's rule as include/smr.h defines it for every width: luma Y[x], the
// chroma of pair x / 2.  Pixel x is pixel i = x % 6 of group x / 6 (four dwords): Y at field 2 i + 1, Cb / Cr of pair j = i / 2 at fields
// 4 j and 4 j + 2, counting the group's twelve fields (lo mid hi of d0 .. d3) from 0.
__device__ __forceinline__ u32 cv210_group_field(const u8 *group, u32 field) {
    const u32 k = field / 3u;
    const u32 dw = g_ld_u32(group + 4u * k);
    return (dw >> (10u * (field - 3u * k))) & 0x3ffu;
}
__device__ __forceinline__ void cv210_pixel_codes(const u8 *row, int x, u32 &yc, u32 &cb, u32 &cr) {
    const u32 grp = (u32)x / 6u, i = (u32)x - 6u * grp, j = i >> 1;
    const u8 *group = row + 16u * (size_t)grp;
    yc = cv210_group_field(group, 2u * i + 1u);
    cb = cv210_group_field(group, 4u * j);
    cr = cv210_group_field(group, 4u * j + 2u);
}

#endif  // __HIPCC__
