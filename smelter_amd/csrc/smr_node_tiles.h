// smr_node_tiles.h — the tile geometry of the batched node kernels (k_image_nodes, k_svg_nodes, k_web_view), stated once.
//
//   * A workgroup of 256 takes one tile of 64 x 16 texels of a surface.  Lane l of wave w owns the four consecutive texels
//     x = 4 * (l & 15) .. + 3 of row 4 * w + (l >> 4) of the tile (nt_lane_x, nt_lane_y); a row's last group may have fewer than four.
//   * A group is moved as one 16-byte access when it is whole and the surface's base and pitch are multiples of 16 (nt_wide: every surface
//     smr_surface_create makes); a partial group and any other surface go texel by texel (nt_load_group, nt_store_group).  Nothing outside
//     [0, w) x [0, h) of a surface is touched: not its row padding, not a byte behind its last row.
//   * Up to 16 jobs travel BY VALUE in the kernel arguments of ONE launch — no table upload, no host synchronisation, nothing to keep
//     alive —: a batch is { Job j[16]; u32 first_tile[17]; u32 n; } with a `wide` in every job, first_tile the prefix sum over the jobs'
//     tile counts (nt_plan, on the host), which maps blockIdx.x to (job, tile) (nt_job_of, nt_tile_of).  Every branch on a job's fields is
//     uniform per workgroup.  nt_launch_batches is the launcher's loop over batches of 16.
// The kernels' machine code is held to the hand-inlined statements these helpers replaced (profiles/ quote counters by the device code's
// hash), and that is why some of them look the way they do: see NT_CONST and nt_store_group.
// The source compiles under SMR_EMU like its users (tests/emu/emu_node_kernel.h).
#pragma once

#include "smr_internal.h"

#define SMR_NODE_MAX_JOBS 16
#define SMR_NODE_BLOCK 256
#define SMR_NODE_TILE_W 64
#define SMR_NODE_TILE_H 16

// Until it has inlined a helper the compiler must know that the call touches no memory (NT_CONST) or only reads it (NT_PURE), or it orders a
// kernel's argument loads around the call differently from the statements written out.
#define NT_CONST __attribute__((const))
#define NT_PURE __attribute__((pure))

__host__ __device__ __forceinline__ u32 nt_wide(const SurfView &s) { return (((uintptr_t)s.ptr | s.pitch) & 15u) == 0 ? 1u : 0u; }
__host__ __device__ __forceinline__ NT_CONST u32 nt_tiles_x(int w) { return ((u32)w + SMR_NODE_TILE_W - 1) / SMR_NODE_TILE_W; }
__host__ __device__ __forceinline__ NT_CONST u32 nt_tiles_y(int h) { return ((u32)h + SMR_NODE_TILE_H - 1) / SMR_NODE_TILE_H; }

// Fills B.first_tile and every j[i].wide; returns the number of workgroups (0: nothing to do).  extent(job): the surface whose texels the
// job's workgroups tile, or null for a job that has none.  Host code, shared with the emulator.
template <class Batch, class Extent>
static inline u32 nt_plan(Batch &B, Extent extent) {
    u32 total = 0;
    for (u32 i = 0; i < SMR_NODE_MAX_JOBS; i++) {
        B.first_tile[i] = total;
        if (i >= B.n) continue;
        B.j[i].wide = 0;
        const SurfView *s = extent(B.j[i]);
        if (!s || !s->ptr || s->w <= 0 || s->h <= 0) continue;
        B.j[i].wide = nt_wide(*s);
        total += nt_tiles_x(s->w) * nt_tiles_y(s->h);
    }
    B.first_tile[SMR_NODE_MAX_JOBS] = total;
    return total;
}

#ifdef __HIPCC__

#ifndef SMR_EMU
// The launcher's loop: n jobs in batches of 16, one launch of `kernel` per batch that has a tile.  fill(job, k) sets what nt_plan does not
// of job k; plan(batch) is the kernel's nt_plan.
template <class Batch, class Fill, class Plan>
static inline int nt_launch_batches(smr_ctx *ctx, void (*kernel)(const Batch, const float *), u32 n, Fill fill, Plan plan) {
    for (u32 at = 0; at < n; at += SMR_NODE_MAX_JOBS) {
        Batch B;
        memset(&B, 0, sizeof(B));
        B.n = n - at < SMR_NODE_MAX_JOBS ? n - at : SMR_NODE_MAX_JOBS;
        for (u32 i = 0; i < B.n; i++) fill(B.j[i], at + i);
        const u32 blocks = plan(B);
        if (!blocks) continue;
        hipLaunchKernelGGL(kernel, dim3(blocks), dim3(SMR_NODE_BLOCK), 0, ctx->stream, B, ctx->d_tables);
        SMR_HIP(ctx, hipGetLastError());
    }
    return SMR_OK;
}
#endif

// The job of workgroup `block` (which is below first_tile[16])
__device__ __forceinline__ NT_PURE u32 nt_job_of(const u32 *first_tile, u32 block) {
    u32 i = 0;
#pragma unroll 1
    while (i + 1 < SMR_NODE_MAX_JOBS && block >= first_tile[i + 1]) i++;
    return i;
}

// The tile of workgroup `block` of job i, whose surface is `w` wide: (x, y) in tiles
struct NodeTile {
    u32 x, y;
};
__device__ __forceinline__ NT_PURE NodeTile nt_tile_of(const u32 *first_tile, u32 i, u32 block, int w) {
    const u32 tiles_x = nt_tiles_x(w);
    const u32 t = block - first_tile[i];
    NodeTile T;
    T.y = t / tiles_x;
    T.x = t - T.y * tiles_x;
    return T;
}

// The first texel (x, y) of the group thread `tid` owns in the tile whose first texel is (tile_x0, tile_y0).  (The origin is a term of the
// sum, not added by the caller, because the order of the additions decides what the compiler makes of them.)
__device__ __forceinline__ NT_CONST u32 nt_lane_x(u32 tile_x0, u32 tid) { return tile_x0 + 4u * (tid & 15u); }
__device__ __forceinline__ NT_CONST u32 nt_lane_y(u32 tile_y0, u32 tid) { return tile_y0 + 4u * (tid >> 6) + ((tid >> 4) & 3u); }

// The group at p of a row that has n (> 0) texels left from there, w - x: its min(n, 4) texels, as one 16-byte access where the surface
// allows and the group is whole.  (nt_store_group takes n by reference: as a by-value argument it is known not to be poison, the
// condition becomes a plain `and`, and k_web_view's last scalar OR comes out with its operands exchanged.)
__device__ __forceinline__ void nt_load_group(const u8 *p, u32 wide, int n, u32 out[4]) {
    if (wide && n >= 4) {
        const uint4 v = g_ld_u32x4(p);
        out[0] = v.x; out[1] = v.y; out[2] = v.z; out[3] = v.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (k < n) out[k] = g_ld_u32(p + 4 * k);
    }
}
__device__ __forceinline__ void nt_store_group(u8 *p, u32 wide, const int &n, const u32 px[4]) {
    if (wide && n >= 4) {
        g_st_u32x4(p, make_uint4(px[0], px[1], px[2], px[3]));
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (k < n) g_st_u32(p + 4 * k, px[k]);
    }
}

#endif  // __HIPCC__
