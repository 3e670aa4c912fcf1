// smr_convert_hi.h — the input converter of 10-bit 4:2:0 frames: P010 (Y plane of 16-bit words, interleaved U V words; the code is the
// word's HIGH ten bits) and planar 10-bit (three planes of words; the code is the word's LOW ten bits).  Included by smr_convert.hip
// (k_yuv420_hi_to_rgba, k_yuv_hi_to_rgba) and, for the CPU, by tests/emu/emu_convert_hi.cpp (the very source).
//
// The value rule (include/smr.h): a 10-bit code c is the 8-bit code c / 4 with two more fractional bits — its unorm value is
// (f32(c) * 0.25f) / 255.0f, product exact, quotient IEEE — and from there on the conversion is planar_yuv_to_rgba.wgsl / nv12_to_rgba.wgsl
// as oracle/smr_oracle.c restates them (sample_plane_bilinear, yuv_to_rgb_store, limited range), operation for operation, with the 8-bit
// constants (limited range 64 .. 940 is exactly 16 .. 235: (c - 64) / 876 = (c / 4 - 16) / 219).  A frame whose codes are 4 b therefore has,
// byte for byte, the node texture of the 8-bit frame with bytes b; the node texture itself is the 8-bit converter's RGBA8 / RGB12, so the
// resampler, the compositor, the node cache and the gather see nothing new.
//
// The block converter has k_yuv420_to_rgba's shape (smr_convert_420.h): a thread owns a 4 x 4 pixel block, cv_plan's XCD bands and equal
// shares, vertical runs that keep the two chroma window rows neighbouring blocks share, all of a block's loads in flight before its first
// store, one 16-byte (RGB12: 12-byte) store per thread and row.  What differs is the fetch — a luma row of a block is 8 bytes, a P010 chroma
// window four U V dwords, a planar window 8 bytes starting on an odd word — and the tables: two of 1024 entries (8 KB of LDS per workgroup).
// The lerps are cv420_hrow's and cv420_rows_to's, statement for statement; the share walk, the pixel tail and the row's way out are the
// shared ones (smr_convert_batch.h).
//
// ONE MEMORY CONTRACT, for planes the library owns and planes it wraps alike: no byte outside [0, row bytes) of any plane row is requested.
// Where a window's last column is the plane's edge the load of the column behind it is aimed at the edge column again.
#pragma once

#include "smr_convert_420.h"

#ifdef __HIPCC__

// the 10-bit code of a 16-bit word — mask or shift BEFORE any table lookup: whatever bytes the caller's planes hold, the index is < 1024
template <bool P010>
__device__ __forceinline__ u32 cvhi_code_lo(u32 d) { return P010 ? (d >> 6) & 0x3ffu : d & 0x3ffu; }  // of the dword's low word
template <bool P010>
__device__ __forceinline__ u32 cvhi_code_hi(u32 d) { return P010 ? d >> 22 : (d >> 16) & 0x3ffu; }    // of its high word

// the unorm value of a code: (c * 0.25) / 255 with a TRUE division (unorm_of_byte's reciprocal form is proven for the 256 bytes only)
__device__ __forceinline__ float cvhi_unorm_of_code(u32 c) { return ((float)c * 0.25f) / 255.0f; }
// y' of a luma code: cv420_luma_of_byte's statements on the code's unorm value (limited range)
__device__ __forceinline__ float cvhi_luma_of_code(u32 c) {
    const float y = cvhi_unorm_of_code(c);
    constexpr float ky = 0.85882352941f;
    const float ry = 1.0f / ky;
    const float a = y - (16.0f / 255.0f), q = a * ry;
    return cv_clamp01(__builtin_fmaf(__builtin_fmaf(-q, ky, a), ry, q));
}
constexpr int CVHI_CODES = 1024;
// both tables of a workgroup of `nthreads` threads (ylut, ulut: CVHI_CODES floats each)
__device__ __forceinline__ void cvhi_build_tables(float *ylut, float *ulut, u32 tid, u32 nthreads) {
    for (u32 c = tid; c < (u32)CVHI_CODES; c += nthreads) {
        ylut[c] = cvhi_luma_of_code(c);
        ulut[c] = cvhi_unorm_of_code(c);
    }
}

// textureSample of one channel of a plane of 16-bit words (comps interleaved channels): sample_plane_bilinear (smr_internal.h) with the
// 16-bit fetch, statement for statement.  Returns the unorm value.
template <bool P010>
__device__ __forceinline__ float cvhi_fetch(const u8 *row, int word) {
    const u32 wv = (u32)row[2 * word] | ((u32)row[2 * word + 1] << 8);  // (little-endian, any alignment)
    return cvhi_unorm_of_code(cvhi_code_lo<P010>(wv));
}
template <bool P010>
__device__ __forceinline__ float sample_plane_bilinear_hi(const SurfView &p, int comps, int c, float u, float v) {
    float sx = u * (float)p.w - 0.5f;
    float sy = v * (float)p.h - 0.5f;
    float fx0 = floorf(sx), fy0 = floorf(sy);
    float fx = subtexel(sx - fx0), fy = subtexel(sy - fy0);
    int x0 = clampi((int)fx0, 0, p.w - 1), x1 = clampi((int)fx0 + 1, 0, p.w - 1);
    int y0 = clampi((int)fy0, 0, p.h - 1), y1 = clampi((int)fy0 + 1, 0, p.h - 1);
    const u8 *r0 = p.ptr + (size_t)y0 * p.pitch, *r1 = p.ptr + (size_t)y1 * p.pitch;
    float a = cvhi_fetch<P010>(r0, x0 * comps + c);
    float b = cvhi_fetch<P010>(r0, x1 * comps + c);
    float cc = cvhi_fetch<P010>(r1, x0 * comps + c);
    float d = cvhi_fetch<P010>(r1, x1 * comps + c);
    float top = a * (1.0f - fx) + b * fx;
    float bot = cc * (1.0f - fx) + d * fx;
    return top * (1.0f - fy) + bot * fy;
}

// ---- the pieces of a block

// Where column group g's chroma window (columns 2 g - 1 .. 2 g + 2, clamped to the plane like the sampler clamps) sits in a chroma row.
// P010: a column is one dword (U | V << 16): four dword loads, each aimed at its clamped column — the clamp costs nothing more.
// Planar: the window is four words from word max(2 g - 1, 0): the dwords at base, base + 4, base + 8 (the third aimed at the row's last
// dword where it would lie behind it) and an alignbyte by sh = 0 (g = 0) or 2; the edge columns are then selects.
struct CvHiWin {
    u32 off[4];  // P010: byte offsets of the four columns' dwords | planar: base, min(4, lim), min(8, lim) from base, -
    u32 sh;      // planar: the first word's byte offset inside its dword
    bool left;   // planar: the window starts left of the plane: columns 0 1 2 3 -> 0 0 1 2
    bool right;  // planar: the window's last column lies behind the plane: it repeats the one before it
};
template <bool P010>
__device__ __forceinline__ CvHiWin cvhi_window(const ConvJob &J, int g) {
    const int cw = J.dst.w >> 1;
    const int first = 2 * g - 1;
    CvHiWin W;
    W.sh = 0u; W.left = false; W.right = false;
    if (P010) {
#pragma unroll
        for (int k = 0; k < 4; k++) W.off[k] = 4u * (u32)min(max(first + k, 0), cw - 1);
    } else {
        const int first_ld = first < 0 ? 0 : first;
        const int byte0 = 2 * first_ld, base = byte0 & ~3;
        const int nvalid = cw - first;  // window columns 0 .. nvalid - 1 exist (>= 3: the last block's window starts at cw - 3)
        // the last column the loaded window can hold is min(first_ld + 3, cw - 1): the dword of its word is the last one worth loading
        const int last_col = first_ld + 3 < cw - 1 ? first_ld + 3 : cw - 1;
        const u32 lim = (u32)((2 * last_col - base) & ~3);
        W.off[0] = (u32)base; W.off[1] = (u32)base + (lim < 4u ? lim : 4u); W.off[2] = (u32)base + (lim < 8u ? lim : 8u); W.off[3] = 0u;
        W.sh = (u32)(byte0 - base); W.left = first < 0; W.right = nvalid < 4;
    }
    return W;
}

// The dwords of one chroma row that hold the window, as loaded (P010: four U V dwords; planar: U x 3, V x 3)
template <bool P010>
struct CvHiRaw {
    u32 d[P010 ? 4 : 6];
};
template <bool P010>
__device__ __forceinline__ CvHiRaw<P010> cvhi_load_chroma(const ConvJob &J, const CvHiWin &W, int crow) {
    const int ch = J.dst.h >> 1;
    const int cy = min(max(crow, 0), ch - 1);
    CvHiRaw<P010> R;
    const u8 *ur = J.up.ptr + cv_mad24((u32)cy, J.up.pitch, 0u);  // (a plane is far below 4 GiB)
    if (P010) {
#pragma unroll
        for (int k = 0; k < 4; k++) R.d[k] = g_ld_u32(ur + W.off[k]);
    } else {
        const u8 *vr = J.vp.ptr + cv_mad24((u32)cy, J.vp.pitch, 0u);
#pragma unroll
        for (int k = 0; k < 3; k++) { R.d[k] = g_ld_u32(ur + W.off[k]); R.d[3 + k] = g_ld_u32(vr + W.off[k]); }
    }
    return R;
}
// a luma row of a block: four words, 8 bytes (rows and the plane are 8-byte aligned: conv_route)
__device__ __forceinline__ void cvhi_load_luma(const ConvJob &J, int g, int P, uint2 yrow[4]) {
    const int h = J.dst.h;
#pragma unroll
    for (int r = 0; r < 4; r++) yrow[r] = g_ld_u32x2(J.yp.ptr + cv_mad24((u32)min(4 * P + r, h - 1), J.yp.pitch, 8u * (u32)g));
}

// One chroma row of the window -> its horizontal lerps at the block's four luma columns, per plane: H[plane][column]
template <bool P010>
__device__ __forceinline__ void cvhi_hrow(const CvHiRaw<P010> &R, const CvHiWin &W, const float *ulut, float H[2][4]) {
    u32 q[2][4];  // codes: [plane][window column]
    if (P010) {
#pragma unroll
        for (int k = 0; k < 4; k++) { q[0][k] = cvhi_code_lo<true>(R.d[k]); q[1][k] = cvhi_code_hi<true>(R.d[k]); }
    } else {
#pragma unroll
        for (int c = 0; c < 2; c++) {
            const u32 lo = cv_alignbyte(R.d[3 * c + 1], R.d[3 * c], W.sh), hi = cv_alignbyte(R.d[3 * c + 2], R.d[3 * c + 1], W.sh);  // words 0 1 | 2 3
            const u32 c0 = cvhi_code_lo<false>(lo), c1 = cvhi_code_hi<false>(lo), c2 = cvhi_code_lo<false>(hi), c3 = cvhi_code_hi<false>(hi);
            q[c][0] = c0;
            q[c][1] = W.left ? c0 : c1;
            q[c][2] = W.left ? c1 : c2;
            q[c][3] = W.left || W.right ? c2 : c3;  // (left: columns 0 0 1 2; right: the last existing column again)
        }
    }
#pragma unroll
    for (int c = 0; c < 2; c++) {
        const float n0 = ulut[q[c][0]], n1 = ulut[q[c][1]], n2 = ulut[q[c][2]], n3 = ulut[q[c][3]];
        // a * (1 - fx) + b * fx with fx = .75, .25, .75, .25 (sample_plane_bilinear): the 1/4 products are exact
        const float m1 = n1 * 0.75f, m2 = n2 * 0.75f;
        H[c][0] = __builtin_fmaf(n0, 0.25f, m1);
        H[c][1] = __builtin_fmaf(n2, 0.25f, m1);
        H[c][2] = __builtin_fmaf(n1, 0.25f, m2);
        H[c][3] = __builtin_fmaf(n3, 0.25f, m2);
    }
}

// the four luma codes of a row of a block
template <bool P010>
__device__ __forceinline__ void cvhi_row_codes(uint2 y4, u32 (&c)[4]) {
    c[0] = cvhi_code_lo<P010>(y4.x); c[1] = cvhi_code_hi<P010>(y4.x); c[2] = cvhi_code_lo<P010>(y4.y); c[3] = cvhi_code_hi<P010>(y4.y);
}

// The four luma rows of block (g, P) from its luma words and the window's four chroma rows H[window row][plane][column]: cv420_rows_to's
// vertical lerps, then the shared pixel tail (limited range) with the luma table indexed by the 10-bit code.
template <bool P010, bool RGB12, bool ALLROWS>
__device__ __forceinline__ void cvhi_rows(const ConvJob &J, int g, int P, const uint2 yrow[4], const float H[4][2][4], const float *ylut) {
    const int h = J.dst.h;
    const SmrMatrixCoef C = smr_matrix_coef((u32)J.matrix);  // (uniform: the job's matrix sits in a scalar register, cv_job_in_registers; not on the benchmark's path, so no instantiation per matrix)
    const CvStoreNode sink{J, g, RGB12};
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int y = 4 * P + r;
        if (!ALLROWS && y >= h) break;
        const int j34 = r < 2 ? 1 : 2, j14 = r == 0 ? 0 : (r == 1 ? 2 : (r == 2 ? 1 : 3));
        u32 yc[4];
        cvhi_row_codes<P010>(yrow[r], yc);
        float t[3][4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const float u = __builtin_fmaf(H[j14][0][i], 0.25f, H[j34][0][i] * 0.75f);
            const float v = __builtin_fmaf(H[j14][1][i], 0.25f, H[j34][1][i] * 0.75f);
            cv_pixel<false>(ylut[yc[i]], u, v, C, t, i);
        }
        cv_pack_row<RGB12>(t, r, y, sink);
    }
}

// A vertical run of blocks: columns 4 g .. 4 g + 3, block rows P0 .. P0 + nb - 1 (those that exist) — cv420_run's order: block P + 1's luma
// words and its two new chroma rows are requested before block P's rows are computed and stored; the run's last block requests nothing.
template <bool P010, bool RGB12>
__device__ __forceinline__ void cvhi_run(const ConvJob &J, int g, int P0, int nb, const float *ylut, const float *ulut) {
    const int Pend = min(P0 + nb, (J.dst.h + 3) >> 2);
    if (P0 >= Pend) return;
    const CvHiWin W = cvhi_window<P010>(J, g);
    uint2 yrow[4];
    cvhi_load_luma(J, g, P0, yrow);
    float H[4][2][4];
    {
        CvHiRaw<P010> raw[4];
#pragma unroll
        for (int j = 0; j < 4; j++) raw[j] = cvhi_load_chroma<P010>(J, W, 2 * P0 - 1 + j);
#pragma unroll
        for (int j = 0; j < 4; j++) cvhi_hrow<P010>(raw[j], W, ulut, H[j]);
    }
    int P = P0;
    for (; P + 1 < Pend; P++) {
        uint2 ynext[4];
        cvhi_load_luma(J, g, P + 1, ynext);
        const CvHiRaw<P010> n2 = cvhi_load_chroma<P010>(J, W, 2 * P + 3), n3 = cvhi_load_chroma<P010>(J, W, 2 * P + 4);
        cvhi_rows<P010, RGB12, true>(J, g, P, yrow, H, ylut);  // (P + 1 < Pend: not the frame's last block row — all four rows exist)
#pragma unroll
        for (int c = 0; c < 2; c++)
#pragma unroll
            for (int i = 0; i < 4; i++) { H[0][c][i] = H[2][c][i]; H[1][c][i] = H[3][c][i]; }
        cvhi_hrow<P010>(n2, W, ulut, H[2]);
        cvhi_hrow<P010>(n3, W, ulut, H[3]);
#pragma unroll
        for (int r = 0; r < 4; r++) yrow[r] = ynext[r];
    }
    cvhi_rows<P010, RGB12, false>(J, g, P, yrow, H, ylut);
}

// a wave's share of a launch (cv_share_walk) over cvhi_run
template <bool P010>
__device__ __forceinline__ void cvhi_share(const ConvBatch &B, u32 block, u32 wave, u32 grid, u32 lane, const float *ylut, const float *ulut) {
    cv_share_walk(B, block, wave, grid, lane, [&](const ConvJob &J, int g, int P0, int nrun) {
        if (J.rgb12) cvhi_run<P010, true>(J, g, P0, nrun, ylut, ulut);
        else cvhi_run<P010, false>(J, g, P0, nrun, ylut, ulut);
    });
}

#endif  // __HIPCC__
