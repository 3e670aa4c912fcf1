// smr_move_rects.h — k_move_rects: up to 16 pitched byte rectangles moved by ONE launch.  The per-frame transport of the local gather
// (smr_gather_tiles, smr_comm.hip): all the tiles — or raw frame planes — one owner context sends to the root go out in one launch on the
// owner's stream instead of one hipMemcpy2DAsync per tile (host enqueue is half of the frame period: profiles/r06_host_rate.txt).
//
//   * The rectangles travel BY VALUE in the kernel arguments (MoveBatch): no table upload, no host synchronisation, nothing to keep alive.
//   * A workgroup takes a band of rows of one rectangle; MoveBatch::first_band (a prefix sum over the rectangles' band counts, made by
//     mv_plan on the host) maps blockIdx.x to (rectangle, band).
//   * FAST path — src, dst, both pitches and the row length are multiples of 16 (every surface smr_surface_create makes, RGBA8 tiles, the
//     planes of even-sized frames): 2^lpr_log2 lanes walk a row 16 bytes each, the 256 >> lpr_log2 row groups of the workgroup take rows side
//     by side, and every lane has four rows' loads in flight before its first store.  Plain 16-byte global loads and stores (plain stores
//     keep the line in the XCD's L2 for the compositor that reads the tile next; narrower stores cost 2.7 - 12 x per byte).
//   * BYTE path — anything else (wrapped surfaces, odd widths), chosen per rectangle and therefore uniform per workgroup: a wave per row;
//     when source and destination row share their phase modulo 16 the row is a byte head up to the destination's next 16-byte boundary, a
//     16-byte body and a byte tail; otherwise bytes throughout.
//   * Row padding is neither read nor written (what hipMemcpy2DAsync guarantees): only [row, row + row_bytes) of rows [0, rows).
// Another device's memory is written with the same stores (peer access is enabled by smr_comm_create_local).
// The source compiles under SMR_EMU (tests/emu/emu_move.cpp): the CPU tests run it on guard-paged buffers.
#pragma once

#include "smr_internal.h"

#define SMR_MOVE_MAX_RECTS 16
#define SMR_MOVE_BLOCK 256
#define SMR_MOVE_BAND_BYTES 32768u  // what one workgroup moves, about (a 1280 x 720 RGBA8 tile: 103 bands of 7 rows)

struct MoveRect {
    const u8 *src;
    u8 *dst;
    u32 src_pitch, dst_pitch;
    u32 row_bytes, rows;
};

struct MoveBatch {
    MoveRect r[SMR_MOVE_MAX_RECTS];
    u32 first_band[SMR_MOVE_MAX_RECTS + 1];  // first_band[i] .. first_band[i + 1]: the workgroups of rectangle i
    u16 band_rows[SMR_MOVE_MAX_RECTS];       // rows per band (>= 1)
    u8 lpr_log2[SMR_MOVE_MAX_RECTS];         // fast path: log2 of the lanes that share a row (0 .. 8)
    u8 fast[SMR_MOVE_MAX_RECTS];             // 1: the 16-byte path
    u32 n;
};

// Fills everything of B but r[] and n; returns the number of workgroups (0: nothing to move).  Host code, shared with the emulator.
static inline u32 mv_plan(MoveBatch &B) {
    u32 total = 0;
    for (u32 i = 0; i < SMR_MOVE_MAX_RECTS; i++) {
        B.first_band[i] = total;
        B.band_rows[i] = 1; B.lpr_log2[i] = 0; B.fast[i] = 0;
        if (i >= B.n) continue;
        const MoveRect &R = B.r[i];
        if (!R.rows || !R.row_bytes) continue;
        const bool fast = (((uintptr_t)R.src | (uintptr_t)R.dst | R.src_pitch | R.dst_pitch | R.row_bytes) & 15u) == 0;
        B.fast[i] = fast ? 1 : 0;
        u32 band = (SMR_MOVE_BAND_BYTES + R.row_bytes - 1) / R.row_bytes;
        if (fast) {
            const u32 chunks = R.row_bytes / 16u;
            u32 lg = 0;
            while (lg < 8 && (1u << lg) < chunks) lg++;
            B.lpr_log2[i] = (u8)lg;
            const u32 pass = 4u * (SMR_MOVE_BLOCK >> lg);  // rows one pass of the workgroup covers, four in flight per lane
            band = (band + pass - 1) / pass * pass;
        }
        if (band > 4096u) band = 4096u;
        if (band > R.rows) band = R.rows;
        B.band_rows[i] = (u16)band;
        total += (R.rows + band - 1) / band;
    }
    B.first_band[SMR_MOVE_MAX_RECTS] = total;
    return total;
}

#ifdef __HIPCC__

#if !defined(SMR_EMU)
__device__ __forceinline__ u32 mv_ld_u8(const u8 *p) { return *SMR_GLOBAL_PTR(const u8, p); }
__device__ __forceinline__ void mv_st_u8(u8 *p, u32 v) { *SMR_GLOBAL_PTR(u8, p) = (u8)v; }
#else
static inline u32 mv_ld_u8(const u8 *p) { return *p; }
static inline void mv_st_u8(u8 *p, u32 v) { *p = (u8)v; }
#endif

// What thread `tid` of workgroup `block` does.  Every branch on B's fields is uniform per workgroup.
__device__ __forceinline__ void mv_workgroup(const MoveBatch &B, u32 block, u32 tid) {
    if (block >= B.first_band[SMR_MOVE_MAX_RECTS]) return;
    u32 i = 0;
#pragma unroll 1
    while (i + 1 < SMR_MOVE_MAX_RECTS && block >= B.first_band[i + 1]) i++;
    const u8 *src = B.r[i].src;
    u8 *dst = B.r[i].dst;
    const size_t sp = B.r[i].src_pitch, dp = B.r[i].dst_pitch;
    const u32 row_bytes = B.r[i].row_bytes, rows = B.r[i].rows, band = B.band_rows[i];
    const u32 y0 = (block - B.first_band[i]) * band;
    const u32 y1 = y0 + band < rows ? y0 + band : rows;
    if (B.fast[i]) {
        const u32 lg = B.lpr_log2[i];
        const u32 lanes = 1u << lg, groups = SMR_MOVE_BLOCK >> lg;  // lanes per row, rows side by side
        const u32 chunks = row_bytes >> 4;
        for (u32 c = tid & (lanes - 1u); c < chunks; c += lanes) {
            for (u32 y = y0 + (tid >> lg); y < y1; y += 4u * groups) {
                uint4 v[4];
#pragma unroll
                for (u32 k = 0; k < 4; k++) {
                    const u32 yy = y + k * groups;
                    if (yy < y1) v[k] = g_ld_u32x4(src + (size_t)yy * sp + 16u * (size_t)c);
                }
#pragma unroll
                for (u32 k = 0; k < 4; k++) {
                    const u32 yy = y + k * groups;
                    if (yy < y1) g_st_u32x4(dst + (size_t)yy * dp + 16u * (size_t)c, v[k]);
                }
            }
        }
        return;
    }
    const u32 lane = tid & 63u, wave = tid >> 6, waves = SMR_MOVE_BLOCK / 64;
    for (u32 y = y0 + wave; y < y1; y += waves) {
        const u8 *s = src + (size_t)y * sp;
        u8 *d = dst + (size_t)y * dp;
        u32 head = row_bytes;
        if ((((uintptr_t)s ^ (uintptr_t)d) & 15u) == 0) {  // same phase: the body moves as 16-byte groups
            head = (u32)((16u - ((uintptr_t)d & 15u)) & 15u);
            if (head > row_bytes) head = row_bytes;
        }
        const u32 chunks = (row_bytes - head) >> 4;
        const u32 tail0 = head + 16u * chunks;
        for (u32 b = lane; b < head; b += 64u) mv_st_u8(d + b, mv_ld_u8(s + b));
        for (u32 c = lane; c < chunks; c += 64u) g_st_u32x4(d + head + 16u * (size_t)c, g_ld_u32x4(s + head + 16u * (size_t)c));
        for (u32 b = tail0 + lane; b < row_bytes; b += 64u) mv_st_u8(d + b, mv_ld_u8(s + b));
    }
}

#ifndef SMR_EMU
__global__ void __launch_bounds__(SMR_MOVE_BLOCK) k_move_rects(const MoveBatch B) { mv_workgroup(B, blockIdx.x, threadIdx.x); }
#endif

#endif  // __HIPCC__
