// smr_fused_compose.h — wave B of the hot path: k_compose_output (included by smr_fused.hip only).
//
// LayoutShader::render + RgbaToYuvConverter / RgbaToNv12Converter in one launch.  A 256-thread workgroup
// owns a 128x16 pixel tile.  The layout list (copied once into LDS) is classified per tile with the exact
// "solid region" test of smr_layout_dev.h (one thread per layout): touch / solid / start = last solid layer whose
// base value is opaque — every earlier layer is overwritten by it (dst * (1 - 1) == 0 exactly).
//   * copy tiles — the start layer is a 1:1 texel-aligned opaque texture (the resampled video tile) or an opaque
//     colour and nothing above it touches the tile: each thread moves a 4x2 pixel block straight from the
//     source texels to Y'CbCr.  No tables, no blending arithmetic.
//   * general tiles — one pixel per thread, eight sweeps of the tile: per-pixel start search (topmost opaque
//     solid layer at that pixel), then the same per-pixel code as the general compositor; results go to an
//     8 KB RGBA8 tile in LDS, from which the 4x2 Y'CbCr conversion runs.  (One inlined copy of the compositor
//     keeps the kernel inside the instruction cache — eight unrolled copies did not.)
#pragma once

#include <type_traits>

#include "smr_convert_dev.h"
#include "smr_layout_dev.h"

namespace {

// A per-lane value the compiler can neither prove loop-invariant nor compute ahead of this point: what is derived from it (a block's
// position, its store addresses) is formed where it is used instead of being held in registers from the top of the loop or the function.
#ifdef SMR_EMU
#define B_KEEP_IN_LOOP(x) do { } while (0)
#else
#define B_KEEP_IN_LOOP(x) asm volatile("" : "+v"(x))
#endif

// row * pitch + offset as one full-rate v_mad_u32_u24 (rows and pitches are below 2^24, a surface below 4 GiB); the 64-bit form is a
// quarter-rate 32 x 32 multiply per address
__device__ __forceinline__ u32 b_off(int row, u32 pitch, int col_bytes) { return (u32)__umul24((u32)row, pitch) + (u32)col_bytes; }

constexpr int B_TILE_W = 128, B_TILE_H = 16;  // pixels; 32 x 8 threads, one 4x2 pixel block each
constexpr int B_MAX_LAYOUTS = 48;             // LDS-resident layout list (larger lists take the general compositor)
constexpr int B_MAX_MASKS = 96;
static_assert(sizeof(DevLayout) % 16 == 0 && sizeof(DevMask) % 16 == 0, "LDS copies move 16 B words");

// How many workgroups the compositor's band list gets.  The tiles that need compositing are latency-bound (layer records through
// scalar registers, one pixel per thread); started last they would be the tail of the kernel, so the first workgroups of the grid
// take them band by band from the classifier's list (TileList).  The host sizes that part of the grid from the list's length once
// it has come back from the device; for a list that is new this frame (a scene in transition) from this prediction — an upper
// bound: a workgroup beyond the list's end returns at once, a listed tile beyond the prediction is composited by the workgroup that
// owns it, band after band.
// A tile that needs compositing is rendered band by band, a workgroup per band, each starting from the classifier's per-band record (touching
// layers, start layer) instead of classifying again; how many bands a tile is cut into is the classifier's decision (B_AREA_BANDS / B_EDGE_BANDS
// below).  Round 3 measured the first compositor with four bands for every tile at 23.2 us on configs[2] and 48.3 us on configs[4], with eight at
// 25.0 / 57.1 us (profiles/r03_compose_ab.txt).
#ifndef SMR_COMPOSE_MIN_WAVES
#define SMR_COMPOSE_MIN_WAVES 6
#endif
// waves per SIMD the register allocation must leave room for.  Round 3 measured the first compositor (~106 VGPRs unconstrained) at 5 / 6 waves
// (96 / 80 VGPRs, scratch in the compositing path): slower ALONE on configs[2], faster on configs[4] (profiles/r03_compose_occupancy.txt).
// Round 6: with two frames in flight the kernel runs beside the other lane's resampler, whose two waves per SIMD leave 160 registers — at 96
// the frame gained 7 %.  The list compositor (compose_full below) fits 79 registers without scratch: six waves, and two of them beside the
// resampler — configs[4] + 3 % over five waves (84 registers), configs[2] unchanged (profiles/r06_sensitivity.txt section 9).
constexpr int B_MIN_WAVES = SMR_COMPOSE_MIN_WAVES;
constexpr int B_BAND_ROWS = SMR_COMPOSE_BAND_ROWS;       // rows of the workgroup's LDS pixel state: a band is at most this tall
static_assert(B_TILE_H % B_BAND_ROWS == 0 && B_BAND_ROWS >= 2, "a band fits the LDS pixel state");

// Host: tiles likely to need compositing -> their number.  A layer that can never be solid over a tile (translucent colour, texture
// with an alpha channel, rotated quad) marks its whole pixel box; every other layer marks the corner squares of its rounded rect and
// of its masks, and the bands along its edges where border / blur / fractional coordinates keep the fragment from being the base
// value.  `bitmap`: scratch, one bit per tile.
inline u32 compose_predict(const PackedLayouts &p, int tiles_x, int tiles_y, std::vector<u32> &bitmap) {
    const int tiles = tiles_x * tiles_y, words = (tiles + 31) / 32;
    bitmap.assign((size_t)words, 0u);
    auto mark = [&](float x0, float y0, float x1, float y1) {  // pixel-space box, clipped to the tile grid
        int tx0 = (int)floorf(x0 / (float)B_TILE_W), tx1 = (int)floorf(x1 / (float)B_TILE_W);
        int ty0 = (int)floorf(y0 / (float)B_TILE_H), ty1 = (int)floorf(y1 / (float)B_TILE_H);
        tx0 = tx0 < 0 ? 0 : tx0; ty0 = ty0 < 0 ? 0 : ty0;
        tx1 = tx1 >= tiles_x ? tiles_x - 1 : tx1; ty1 = ty1 >= tiles_y ? tiles_y - 1 : ty1;
        for (int ty = ty0; ty <= ty1; ty++)
            for (int tx = tx0; tx <= tx1; tx++) {
                const int t = ty * tiles_x + tx;
                bitmap[t >> 5] |= 1u << (t & 31);
            }
    };
    auto corners = [&](float left, float top, float w, float h, float c, const DevLayout &L) {
        if (!(c > 0.0f)) return;
        const float bx0 = (float)L.bx0, by0 = (float)L.by0, bx1 = (float)L.bx1 - 1.0f, by1 = (float)L.by1 - 1.0f;  // only where L draws
        const float xs[2][2] = {{left, left + c}, {left + w - c, left + w}}, ys[2][2] = {{top, top + c}, {top + h - c, top + h}};
        for (int a = 0; a < 2; a++)
            for (int b = 0; b < 2; b++) {
                const float x0 = fmaxf(xs[a][0], bx0), x1 = fminf(xs[a][1], bx1), y0 = fmaxf(ys[b][0], by0), y1 = fminf(ys[b][1], by1);
                if (x0 <= x1 && y0 <= y1) mark(x0, y0, x1, y1);
            }
    };
    for (int i = 0; i < p.n; i++) {
        const DevLayout &L = p.host_layouts[i];
        if (L.bx1 <= L.bx0 || L.by1 <= L.by0) continue;
        // (an opaque texture at a fractional position or another scale is sampled, not copied — TC_SAMPLED — but solid all the same)
        const bool solid_capable = (L.flags & DL_UNROTATED) && (L.type == 0 ? L.src_kind == 2 : (L.flags & DL_COLOR_OPAQUE) != 0);
        if (!solid_capable) {
            mark((float)L.bx0, (float)L.by0, (float)L.bx1 - 1.0f, (float)L.by1 - 1.0f);
            continue;
        }
        corners(L.left, L.top, L.width, L.height, L.corner, L);
        for (u32 m = 0; m < L.masks_len; m++) {
            const DevMask &K = p.host_masks[L.masks_off + m];
            corners(K.left, K.top, K.width, K.height, K.corner, L);
            // a mask edge that cuts through the layer leaves a band of partially covered / uncovered pixels
            if (K.left > L.left || K.top > L.top || K.left + K.width < L.left + L.width || K.top + K.height < L.top + L.height)
                mark((float)L.bx0, (float)L.by0, (float)L.bx1 - 1.0f, (float)L.by1 - 1.0f);
        }
        if (L.inset != 0.5f) {  // border, blur or fractional coordinates: bands along the four edges
            const float d = ceilf(L.inset);
            const float x0 = (float)L.bx0, y0 = (float)L.by0, x1 = (float)L.bx1 - 1.0f, y1 = (float)L.by1 - 1.0f;
            mark(x0, y0, x1, fminf(y0 + d, y1)); mark(x0, fmaxf(y1 - d, y0), x1, y1);
            mark(x0, y0, fminf(x0 + d, x1), y1); mark(fmaxf(x1 - d, x0), y0, x1, y1);
        }
    }
    u32 nf = 0;
    for (int w = 0; w < words; w++) nf += (u32)__builtin_popcount(bitmap[w]);
    return nf;
}

__device__ __forceinline__ void classify_layouts(u32 *s_touch, u32 *s_solid, int *s_start, const DevLayout *__restrict__ layouts,
                                                 const DevMask *__restrict__ masks, int n, int x0, int y0, int x1, int y1, int tid,
                                                 int nthreads) {
    if (tid < MAX_LAYOUT_WORDS) { s_touch[tid] = 0; s_solid[tid] = 0; }
    if (tid == 0) *s_start = -1;
    __syncthreads();
    const float cx0 = (float)x0 + 0.5f, cx1 = (float)x1 - 0.5f, cy0 = (float)y0 + 0.5f, cy1 = (float)y1 - 0.5f;
    for (int i = tid; i < n; i += nthreads) {
        const DevLayout &L = layouts[i];
        if (!(L.bx0 < x1 && L.bx1 > x0 && L.by0 < y1 && L.by1 > y0)) continue;
        atomicOr(&s_touch[i >> 5], 1u << (i & 31));
        if (!layout_solid_box(L, masks, cx0, cy0, cx1, cy1)) continue;
        atomicOr(&s_solid[i >> 5], 1u << (i & 31));
        if (layout_base_opaque(L)) atomicMax(s_start, i);
    }
    __syncthreads();
}

// What a tile needs beyond its start layer (after classify_layouts; the caller zeroes *s_general and syncs afterwards):
// bit 0 — some touched layer at or above the start needs blending arithmetic, 2 — the start layer is an opaque texture that is not
// a 1:1 blit.  0 = copy tile.
__device__ __forceinline__ void tile_needs(const u32 *s_touch, int start, int *s_general, const DevLayout *__restrict__ layouts, int n, int tid,
                                           int nthreads) {
    for (int i = tid; i < n; i += nthreads) {
        if (!((s_touch[i >> 5] >> (i & 31)) & 1u) || i < start) continue;
        const DevLayout &L = layouts[i];
        const bool copy_layer = i == start && (L.type != 0 || (L.flags & DL_ALIGNED));
        const bool sample_layer = i == start && L.type == 0 && !(L.flags & DL_ALIGNED);  // opaque texture, solid over the tile, not a 1:1 blit
        if (sample_layer) atomicOr(s_general, 2);
        else if (!copy_layer) atomicOr(s_general, 1);
        // 4: a layer that can blend over an area (translucent, an alpha channel, rotated, a shadow): the tile's list of pixels to composite may
        // be most of the tile.  Without it the layers are opaque and unrotated and only their edges and corners blend.
        if (!(layout_base_opaque(L) && (L.flags & DL_UNROTATED))) atomicOr(s_general, 4);
    }
}

// The class of every 128x16 tile, computed once per layout list (smr_render_layouts keeps it while the list repeats — a scene at
// rest — and recomputes it when the list changes): what k_compose_output needs to know to finish a copy tile without reading the
// layout list at all.  Same classification code as the compositor's own (classify_layouts / tile_needs), one 64-thread workgroup
// per tile.
//   TC_CLEAR    no opaque layer and nothing touching: transparent black
//   TC_COLOUR   an opaque colour, nothing above: px = its encoded bytes
//   TC_TEXTURE  a 1:1 blit of an opaque texture, nothing above: base / pitch = the texel under the tile's top-left pixel
//   TC_FULL     anything else: the compositor classifies and composites the tile itself; px = the tile's index in the list of
//               such tiles (TileList), which the compositor's first workgroups take band by band
//   TC_SKIP     wave A writes the tile's Y'CbCr (direct output)
//   TC_SAMPLED  the whole tile lies in the solid region of one opaque texture layer that is not a 1:1 blit (a video tile at a
//               fractional position or another scale: every tile of a grid in mid-transition), nothing above: px = that layer
//   TC_SELECT   every layer that touches the tile (from the start layer up; at most four) is an opaque 1:1 texture or an opaque colour
//               and SOLID wherever it touches it — the seam between two video tiles of a grid, a tile's edge on the background:
//               a pixel is a copy from the topmost of them whose pixel box holds it (dst * (1 - 1) == 0 wipes what is below, and a
//               layer draws nothing outside its box), no blending arithmetic.  px = the layers, topmost first, a byte each, 0xff = none
enum { TC_CLEAR = 0, TC_COLOUR = 1, TC_TEXTURE = 2, TC_FULL = 3, TC_SKIP = 4, TC_SAMPLED = 5, TC_SELECT = 6 };
struct alignas(16) TileClass {
    const u8 *base;
    u32 pitch_or_px;
    u32 kind;
};
// A tile that needs compositing, with what the classification found out about it (the compositor's workgroups start from this
// record instead of classifying their band again): the touching layers, the last opaque solid layer, tile_needs' bits.
struct TileFull {
    u32 tile;
    int start;
    u32 general;
    u32 band;  // first row of the band within the tile | rows << 8
    u32 touch[MAX_LAYOUT_WORDS];
};
// Bands — list entries, workgroups — of a tile that needs compositing.  A workgroup's time is its round trips to memory (the layout list, the
// start values, a trip per layer of the listed pixels) while its listed pixels fit a pass or two; a tile whose layers are all opaque and unrotated
// blends along their edges and corners only — a few dozen listed pixels — and is two workgroups' (configs[4] in motion: 993 such tiles; root
// compositor 52.5 -> 47.8 us).  A tile under a layer that blends over an area (a translucent label, text, a texture with an alpha channel) lists
// most of its pixels: four shorter bands, four workgroups (configs[2]: alone 17.9 us; 25 us with two bands for every tile).
constexpr int B_AREA_BANDS = 4, B_EDGE_BANDS = B_TILE_H / B_BAND_ROWS;
static_assert(B_TILE_H / B_AREA_BANDS <= B_BAND_ROWS && B_EDGE_BANDS <= B_AREA_BANDS, "a band fits the workgroup's pixel state");
constexpr int B_LIST_COUNTERS = 64;
struct TileList {
    u32 count[B_LIST_COUNTERS];  // the list's length, one counter per classification (a ring: the host zeroes all of them once per
                                 // B_LIST_COUNTERS classifications instead of one before every k_classify_tiles — a fill kernel on the stream
                                 // of every frame of a scene in motion)
    TileFull e[1];               // really one per tile
};
// Direct output: direct[tile] = the start layer when the tile is a copy tile of a texture layer in `direct_layers` (the tiles wave A
// resamples in the same call, at even output positions) — wave A then writes that tile's Y'CbCr itself, the RGBA8 bytes of those
// pixels never exist in memory — else 0xff.
constexpr u32 B_CLASS_NONE = 0xffu;
constexpr int B_CLASSIFY_TILES = 16;  // tiles per workgroup of k_classify_tiles, one wave each: the tiles that need compositing take their
                                      // list slots with ONE atomic per workgroup (a thousand atomics on one counter were most of the
                                      // kernel: 15.3 -> 7.7 us for a 4K output in transition)
__global__ __launch_bounds__(64 * B_CLASSIFY_TILES) void k_classify_tiles(const DevLayout *__restrict__ layouts, const DevMask *__restrict__ masks, int n,
                                                                          int W, int H, int tiles_x, int tiles, unsigned long long direct_layers,
                                                                          TileClass *__restrict__ tc, u8 *__restrict__ direct, TileList *__restrict__ full,
                                                                          int allow_select, int counter) {
    __shared__ u32 s_touch_w[B_CLASSIFY_TILES][MAX_LAYOUT_WORDS], s_solid_w[B_CLASSIFY_TILES][MAX_LAYOUT_WORDS];
    __shared__ int s_start_w[B_CLASSIFY_TILES], s_general_w[B_CLASSIFY_TILES], s_slot_w[B_CLASSIFY_TILES];
    __shared__ TileClass s_class_w[B_CLASSIFY_TILES];
    __shared__ u32 s_direct_w[B_CLASSIFY_TILES];
    // (every wave runs the same barriers: a wave past the last tile classifies the last tile again and writes nothing)
    const int wave = threadIdx.x >> 6, tid = threadIdx.x & 63;
    const bool live = (int)blockIdx.x * B_CLASSIFY_TILES + wave < tiles;
    const int tile = min((int)blockIdx.x * B_CLASSIFY_TILES + wave, tiles - 1);
    u32 *s_touch = s_touch_w[wave], *s_solid = s_solid_w[wave];
    int &s_start = s_start_w[wave], &s_general = s_general_w[wave], &s_slot = s_slot_w[wave];
    const int tile_y = tile / tiles_x;
    const int tx0 = (tile - tile_y * tiles_x) * B_TILE_W, ty0 = tile_y * B_TILE_H;
    if (tid == 0) s_general = 0;
    classify_layouts(s_touch, s_solid, &s_start, layouts, masks, n, tx0, ty0, min(tx0 + B_TILE_W, W), min(ty0 + B_TILE_H, H), tid, 64);
    const int start = s_start;
    tile_needs(s_touch, start, &s_general, layouts, n, tid, 64);
    __syncthreads();
    if (tid == 0) {
        TileClass c;
        c.base = nullptr; c.pitch_or_px = 0u; c.kind = TC_FULL;
        u32 d = B_CLASS_NONE;
        if ((s_general & 3) == 1 && allow_select) {  // some layer above the start: a tile of plain copies all the same?  (serial: a handful of layers)
            const int x1 = min(tx0 + B_TILE_W, W), y1 = min(ty0 + B_TILE_H, H);
            u32 ids = 0xffffffffu;
            int cnt = 0;
            bool ok = true;
            for (int wi = (n + 31) / 32 - 1; ok && wi >= 0; wi--) {
                u32 bits = s_touch[wi];
                while (ok && bits) {
                    const int b = 31 - __clz(bits);
                    bits &= ~(1u << b);
                    const int i = wi * 32 + b;
                    if (i < start) continue;
                    const DevLayout &L = layouts[i];
                    const int ax0 = max(L.bx0, tx0), ay0 = max(L.by0, ty0), ax1 = min(L.bx1, x1), ay1 = min(L.by1, y1);  // (touching: not empty)
                    ok = cnt < 4 && i < 255 && layout_base_opaque(L) && (L.type != 0 || (L.flags & DL_ALIGNED)) &&
                         layout_solid_box(L, masks, (float)ax0 + 0.5f, (float)ay0 + 0.5f, (float)ax1 - 0.5f, (float)ay1 - 0.5f);
                    if (ok) {
                        ids = (ids & ~(0xffu << (8 * cnt))) | ((u32)i << (8 * cnt));
                        cnt++;
                    }
                }
            }
            if (ok && cnt > 0) {
                c.kind = TC_SELECT;
                c.pitch_or_px = ids;
            }
        } else if ((s_general & 3) == 2 && start >= 0) {
            c.kind = TC_SAMPLED;
            c.pitch_or_px = (u32)start;
        } else if ((s_general & 3) == 0) {
            if (start < 0) {
                c.kind = TC_CLEAR;
            } else if (layouts[start].type != 0) {
                c.kind = TC_COLOUR;
                c.pitch_or_px = layouts[start].solid_px;
            } else {
                const DevLayout &L = layouts[start];
                c.kind = TC_TEXTURE;
                c.base = L.src.ptr + (ptrdiff_t)(ty0 - L.iy) * (ptrdiff_t)L.src.pitch + (ptrdiff_t)(tx0 - L.ix) * 4;
                c.pitch_or_px = (u32)L.src.pitch;
                if (start < 64 && ((direct_layers >> start) & 1ull) && tx0 + B_TILE_W <= W && ty0 + B_TILE_H <= H) {
                    c.kind = TC_SKIP;
                    d = (u32)start;
                }
            }
        }
        // (a request; the slots themselves below)  A tile that needs compositing is B_AREA_BANDS bands' work when one of its layers blends over an
        // area, B_EDGE_BANDS longer ones when all of them are opaque and unrotated: one list entry — one workgroup of the compositor — per band
        s_slot = (live && c.kind == TC_FULL) ? ((s_general & 4) ? B_AREA_BANDS : B_EDGE_BANDS) : 0;
        s_class_w[wave] = c;
        s_direct_w[wave] = d;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int want = 0;
        for (int w = 0; w < B_CLASSIFY_TILES; w++) want += s_slot_w[w];
        const u32 base = want ? atomicAdd(&full->count[counter], (u32)want) : 0u;
        int at = 0;
        for (int w = 0; w < B_CLASSIFY_TILES; w++) {
            const int mine = s_slot_w[w] ? (int)base + at : -1;
            at += s_slot_w[w];
            s_slot_w[w] = mine;
        }
    }
    __syncthreads();
    const int bands = (s_general & 4) ? B_AREA_BANDS : B_EDGE_BANDS;
    if (tid == 0 && live) {
        TileClass c = s_class_w[wave];
        if (c.kind == TC_FULL) { c.pitch_or_px = (u32)s_slot; c.base = (const u8 *)(uintptr_t)bands; }  // (first entry, number of entries)
        tc[tile] = c;
        direct[tile] = (u8)s_direct_w[wave];
    }
    if (s_slot >= 0) {  // (uniform per wave) the records the compositor's bands of this tile start from
        const int rows = B_TILE_H / bands;
        for (int j = 0; j < bands; j++) {
            TileFull &E = full->e[s_slot + j];
            if (tid < MAX_LAYOUT_WORDS) E.touch[tid] = tid < ((n + 31) >> 5) ? s_touch[tid] : 0u;
            if (tid == 0) { E.tile = (u32)tile; E.start = start; E.general = (u32)s_general; E.band = (u32)(j * rows) | ((u32)rows << 8); }
        }
    }
}

// Wave-uniform copy of a record (LDS or global) into scalar registers: the dword loads are issued back to back
// (one wait), v_readfirstlane moves them to SGPRs, and every later use is a scalar operand / a uniform branch.
template <typename T>
__device__ __forceinline__ T load_uniform(const T *p) {
    static_assert(sizeof(T) % 4 == 0, "dword records only");
    T out;  // (through memcpy both ways: the record's fields are floats and ints, not u32 objects)
#pragma unroll
    for (int i = 0; i < (int)(sizeof(T) / 4); i++) {
        u32 w;
        __builtin_memcpy(&w, (const char *)p + 4 * i, 4);
        w = __builtin_amdgcn_readfirstlane(w);
        __builtin_memcpy((char *)&out + 4 * i, &w, 4);
    }
    return out;
}

__device__ __forceinline__ float4 decode_texel(u32 raw, int srgb, const float *__restrict__ dec) {
    const u32 r = raw & 0xff, g = (raw >> 8) & 0xff, b = (raw >> 16) & 0xff, a = raw >> 24;
    float4 o;
    if (srgb) { o.x = dec[r]; o.y = dec[g]; o.z = dec[b]; }
    else { o.x = (float)r / 255.0f; o.y = (float)g / 255.0f; o.z = (float)b / 255.0f; }
    o.w = div_cr((float)a, 255.0f, 1.0f / 255.0f);
    return o;
}

// composite_layout() for one pixel with the exact shortcuts the fused kernel can take:
//   * an opaque colour in its solid region stores its pre-encoded bytes (dst * 0 vanishes);
//   * an aligned opaque texel whose fragment came out equal to the sample (coverage, border and every mask evaluated
//     to exactly 1) stores its own bytes: encode(decode(b)) == b;
//   * `is_base`: the caller established that this layer is opaque and solid at the pixel.
__device__ __forceinline__ u32 aligned_texel(const DevLayout &L, int px, int py) {
    return g_ld_u32(L.src.ptr + b_off(clampi(py - L.iy, 0, L.tex_h - 1), L.src.pitch, clampi(px - L.ix, 0, L.tex_w - 1) * 4));  // (a global load: the layer record came through LDS / scalar registers)
}

// `raw_pre`: the texel of an aligned texture layer, fetched by the caller ahead of the arithmetic (aligned_texel)
__device__ __forceinline__ u32 compose_px(u32 a, const DevLayout &L, const DevMask *__restrict__ masks, int px, int py, bool is_base,
                                          u32 raw_pre, int srgb, const float *__restrict__ dec, const float *__restrict__ thr) {
    float fx, fy, lx, ly;
    if (!layout_covers(L, px, py, fx, fy, lx, ly)) return a;
    const bool solid = is_base || layout_solid_box(L, masks, fx, fy, fx, fy);
    if (L.type != 0) {
        if (solid && (L.flags & DL_COLOR_OPAQUE)) return L.solid_px;
        const float4 frag = solid ? make_float4(L.color[0], L.color[1], L.color[2], L.color[3])
                                  : layout_fragment(L, masks, fx, fy, lx, ly, make_float4(0.f, 0.f, 0.f, 0.f));
        return blend_store(a, frag, srgb, dec, thr);
    }
    const bool aligned = (L.flags & DL_ALIGNED) && L.src_kind != 0;
    u32 raw = 0u;
    float4 sample;
    if (aligned) {
        raw = raw_pre;
        sample = decode_texel(raw, srgb, dec);
    } else {
        sample = layout_texture_sample(L, px, py, lx, ly, srgb, dec);
    }
    const float4 frag = solid ? sample : layout_fragment(L, masks, fx, fy, lx, ly, sample);
    if (aligned && (raw >> 24) == 255u && frag.x == sample.x && frag.y == sample.y && frag.z == sample.z && frag.w == sample.w) return raw;
    return blend_store(a, frag, srgb, dec, thr);
}

// The cold half of store_yuv_block's conversion: a lane with a guard flag among its block's twelve plane values (2.4 values in 10 000 raise
// one) computes those values again with the reference sequence itself (unorm_of_byte, yuv_byte, the ((a + b) + (c + d)) / 4 mean of
// smr_convert_dev.h) and replaces their bytes in the packed results.  Everything the sequence needs — byte / 255 of all 24 channel bytes —
// is computed here, behind the block's ONE branch: with a branch per value (yuv_luma_byte / yuv_chroma_bytes) the compiler hoisted these
// operands, common to all twelve branches, above them, onto every pixel's path.  It starts again from the block's bytes (opaque copies:
// nothing of the fast path — the bytes as floats, the flags — is kept alive for it), constant indices only (no scratch).
__device__ __forceinline__ void yuv_block_repair(const u32 (&acc)[8], u32 &yrow0, u32 &yrow1, u32 &u2, u32 &v2) {
    u32 px[8];
    float r[8], g[8], b[8];
#pragma unroll
    for (int k = 0; k < 8; k++) {
        px[k] = acc[k];
        B_KEEP_IN_LOOP(px[k]);
        r[k] = unorm_of_byte(px[k] & 0xffu);
        g[k] = unorm_of_byte((px[k] >> 8) & 0xffu);
        b[k] = unorm_of_byte((px[k] >> 16) & 0xffu);
    }
#pragma unroll
    for (int k = 0; k < 8; k++) {
        bool f;
        (void)yuvfast::convert<0>((float)(px[k] & 0xffu), (float)((px[k] >> 8) & 0xffu), (float)((px[k] >> 16) & 0xffu), &f);
        const u32 exact = yuv_byte(r[k], g[k], b[k], 0), sh = 8u * (u32)(k & 3);
        u32 &row = k < 4 ? yrow0 : yrow1;
        row = f ? ((row & ~(0xffu << sh)) | (exact << sh)) : row;
    }
#pragma unroll
    for (int j = 0; j < 2; j++) {
        const int a = 2 * j, c = 4 + 2 * j;
        float sum[3];
#pragma unroll
        for (int ch = 0; ch < 3; ch++)
            sum[ch] = ((float)((px[a] >> (8 * ch)) & 0xffu) + (float)((px[a + 1] >> (8 * ch)) & 0xffu)) +
                      ((float)((px[c] >> (8 * ch)) & 0xffu) + (float)((px[c + 1] >> (8 * ch)) & 0xffu));
        bool f1, f2;
        (void)yuvfast::convert<1>(sum[0], sum[1], sum[2], &f1);
        (void)yuvfast::convert<2>(sum[0], sum[1], sum[2], &f2);
        const float mr = ((r[a] + r[a + 1]) + (r[c] + r[c + 1])) * 0.25f, mg = ((g[a] + g[a + 1]) + (g[c] + g[c + 1])) * 0.25f,
                    mb = ((b[a] + b[a + 1]) + (b[c] + b[c + 1])) * 0.25f;
        const u32 eu = yuv_byte(mr, mg, mb, 1), ev = yuv_byte(mr, mg, mb, 2), sh = 8u * (u32)j;
        u2 = f1 ? ((u2 & ~(0xffu << sh)) | (eu << sh)) : u2;
        v2 = f2 ? ((v2 & ~(0xffu << sh)) | (ev << sh)) : v2;
    }
}

// ---- packed 4:2:2 outputs (NV 3: UYVY, NV 4: YUYV; include/smr.h): a lane's 4 x 2 block is two texels in each of two rows — per row four Y',
// and the Cb and Cr of its two horizontal pixel pairs.  Luma is the fast path of the planar stores (yuvfast::convert<0>), chroma its pair twin
// (convert422: the pair's byte sums, the / 2 of the mean folded in; tools/check_yuv_fast_422.cpp proves it over the complete domain), sixteen
// guard flags per block behind ONE branch.  All of it is reached from store_yuv_block only behind `NV >= 3`: the builds for NV 0 .. 2 hold
// none of it.

// The cold half, yuv_block_repair's twin for two pairs per row: the flagged values again with the reference sequence (unorm_of_byte, the 4:2:2
// chroma sample a * .5 + b * .5 of k_rgba_to_planes, yuv_byte).  uv0 / uv1: a row's chroma bytes U(pair 0) U(pair 1) V(pair 0) V(pair 1).
__device__ __forceinline__ void yuv_block_repair_422(const u32 (&acc)[8], u32 &yrow0, u32 &yrow1, u32 &uv0, u32 &uv1) {
    u32 px[8];
    float r[8], g[8], b[8];
#pragma unroll
    for (int k = 0; k < 8; k++) {
        px[k] = acc[k];
        B_KEEP_IN_LOOP(px[k]);
        r[k] = unorm_of_byte(px[k] & 0xffu);
        g[k] = unorm_of_byte((px[k] >> 8) & 0xffu);
        b[k] = unorm_of_byte((px[k] >> 16) & 0xffu);
    }
#pragma unroll
    for (int k = 0; k < 8; k++) {
        bool f;
        (void)yuvfast::convert<0>((float)(px[k] & 0xffu), (float)((px[k] >> 8) & 0xffu), (float)((px[k] >> 16) & 0xffu), &f);
        const u32 exact = yuv_byte(r[k], g[k], b[k], 0), sh = 8u * (u32)(k & 3);
        u32 &row = k < 4 ? yrow0 : yrow1;
        row = f ? ((row & ~(0xffu << sh)) | (exact << sh)) : row;
    }
#pragma unroll
    for (int q = 0; q < 4; q++) {  // pair q & 1 of row q >> 1
        const int a = 4 * (q >> 1) + 2 * (q & 1);
        float sum[3];
#pragma unroll
        for (int ch = 0; ch < 3; ch++) sum[ch] = (float)((px[a] >> (8 * ch)) & 0xffu) + (float)((px[a + 1] >> (8 * ch)) & 0xffu);
        bool f1, f2;
        (void)yuvfast::convert422<1>(sum[0], sum[1], sum[2], &f1);
        (void)yuvfast::convert422<2>(sum[0], sum[1], sum[2], &f2);
        const float mr = r[a] * 0.5f + r[a + 1] * 0.5f, mg = g[a] * 0.5f + g[a + 1] * 0.5f, mb = b[a] * 0.5f + b[a + 1] * 0.5f;
        const u32 eu = yuv_byte(mr, mg, mb, 1), ev = yuv_byte(mr, mg, mb, 2), su = 8u * (u32)(q & 1), sv = su + 16u;
        u32 &uv = q < 2 ? uv0 : uv1;
        uv = f1 ? ((uv & ~(0xffu << su)) | (eu << su)) : uv;
        uv = f2 ? ((uv & ~(0xffu << sv)) | (ev << sv)) : uv;
    }
}

// Texel `j` (0, 1) of a block row: y4 = its four Y' bytes, uv = U0 U1 V0 V1.  ORDER 3: U Y V Y, 4: Y U Y V — byte moves.
template <int NV>
__device__ __forceinline__ u32 packed422_texel(u32 y4, u32 uv, int j) {
    const u32 ya = (y4 >> (16 * j)) & 0xffu, yb = (y4 >> (16 * j + 8)) & 0xffu, u = (uv >> (8 * j)) & 0xffu, v = (uv >> (16 + 8 * j)) & 0xffu;
    return NV == 3 ? u | (ya << 8) | (v << 16) | (yb << 24) : ya | (u << 8) | (yb << 16) | (v << 24);
}

// Whether a packed plane takes the paired stores (16 bytes of one row per lane): the twin of planes_pair_aligned for one plane of texels
__device__ __forceinline__ bool plane_pair_aligned_422(const SurfView &p) { return ((((uintptr_t)p.ptr) | p.pitch) & 15u) == 0; }

// The block's store.  The plane's base and pitch are 8-byte aligned (smr_render_layouts routes other planes through smr_rgba_to_frame): a
// full block is one 8-byte store per row at row * pitch + px0 * 2, the half block of a width with W % 4 == 2 one texel per row.
// `pair` (wave-uniform, as for store_yuv_block; base and pitch 16-byte aligned): lanes l and l ^ 1 exchange rows — the even lane stores 16
// bytes of row 0, the odd lane 16 bytes of row 1: two store instructions per lane pair and row instead of four, the same bytes.
template <int NV>
__device__ __forceinline__ void store_packed422_block(const u32 (&acc)[8], int px0, int py0, int W, const SurfView &p, bool pair) {
    float cr[8], cg[8], cb[8];
#pragma unroll
    for (int k = 0; k < 8; k++) {
        cr[k] = (float)(acc[k] & 0xffu);
        cg[k] = (float)((acc[k] >> 8) & 0xffu);
        cb[k] = (float)((acc[k] >> 16) & 0xffu);
    }
    u32 yrow0 = 0, yrow1 = 0, uv0 = 0, uv1 = 0;
    bool flagged = false;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        bool f0, f1;
        yrow0 |= yuvfast::convert<0>(cr[k], cg[k], cb[k], &f0) << (8 * k);
        yrow1 |= yuvfast::convert<0>(cr[4 + k], cg[4 + k], cb[4 + k], &f1) << (8 * k);
        flagged |= f0 | f1;
    }
    // chroma: the tap at the 4:2:2 chroma texel centre = weights (1/2, 1/2) on the pair, a * .5 + b * .5 == (a + b) * .5 bit for bit (a power
    // of two scales exactly); the fast path takes the pair's byte sums (exact in f32)
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int a = 4 * (q >> 1) + 2 * (q & 1);
        const float sr = cr[a] + cr[a + 1], sg = cg[a] + cg[a + 1], sb = cb[a] + cb[a + 1];
        bool f1, f2;
        const u32 c = (yuvfast::convert422<1>(sr, sg, sb, &f1) << (8 * (q & 1))) | (yuvfast::convert422<2>(sr, sg, sb, &f2) << (16 + 8 * (q & 1)));
        if (q < 2) uv0 |= c; else uv1 |= c;
        flagged |= f1 | f2;
    }
    if (flagged) {
        YUV_SLOW_PATH_STAYS_A_BRANCH();
        yuv_block_repair_422(acc, yrow0, yrow1, uv0, uv1);
    }
    const u32 t00 = packed422_texel<NV>(yrow0, uv0, 0), t01 = packed422_texel<NV>(yrow0, uv0, 1);
    const u32 t10 = packed422_texel<NV>(yrow1, uv1, 0), t11 = packed422_texel<NV>(yrow1, uv1, 1);
    if (pair) {  // (an interior tile: no half block, px0 = 4 * lane within the row)
        const bool odd = (px0 & 4) != 0;
        // the even lane gets its right neighbour's row 0, the odd lane its left neighbour's row 1
        const u32 n0 = (u32)dev_mov_dpp_quad_swap((int)(odd ? t00 : t10)), n1 = (u32)dev_mov_dpp_quad_swap((int)(odd ? t01 : t11));
        g_st_u32x4(p.ptr + b_off(py0 + (odd ? 1 : 0), p.pitch, (px0 & ~7) * 2), odd ? make_uint4(n0, n1, t10, t11) : make_uint4(t00, t01, n0, n1));
        return;
    }
    u8 *o = p.ptr + b_off(py0, p.pitch, px0 * 2);
    if (px0 + 3 >= W) {  // (W is even: the last block of a row holds four or two pixels)
        g_st_u32(o, t00);
        g_st_u32(o + p.pitch, t10);
    } else {
        g_st_u32x2(o, t00, t01);
        g_st_u32x2(o + p.pitch, t10, t11);
    }
}

// Whether a tile's blocks may be stored by lane pairs (store_yuv_block's `pair`, decided once per tile, wave-uniformly): the tile lies wholly
// inside the output — every lane of every wave holds a whole 4 x 2 block — and the planes' bases and pitches keep a pair's 8 bytes of Y'
// and 4 bytes of U / V naturally aligned (the library's own planes always; a wrapped frame with tight rows of odd width does not).
template <int NV>
__device__ __forceinline__ bool planes_pair_aligned(const SurfView &yp, const SurfView &up, const SurfView &vp) {
#if defined(SMR_EMU) && !defined(SMR_EMU_WAVE_EXCHANGE)
    return false;  // (a harness of the lane emulator that sets up no per-wave exchange — tests/emu/emu_compose.cpp: the per-lane stores everywhere)
#else
    if (NV >= 3) return plane_pair_aligned_422(yp);  // (its own predicate: one plane of texels, 16 bytes per lane)
    if (NV == 2) return false;
    bool ok = ((((uintptr_t)yp.ptr) | yp.pitch) & 7u) == 0;
    if (NV == 0) ok = ok && ((((uintptr_t)up.ptr) | up.pitch | ((uintptr_t)vp.ptr) | vp.pitch) & 3u) == 0;
    return ok;
#endif
}

// `pair` (wave-uniform; only where every lane of the wave makes this call): lanes l and l ^ 1 — horizontally adjacent blocks — exchange
// halves, so that the even lane stores 8 bytes of Y' row 0 and the odd lane 8 bytes of row 1, and for planar output the even lane 4 bytes of
// U and the odd lane 4 bytes of V: two store instructions per lane instead of four, the same bytes.
template <int NV>
__device__ __forceinline__ void store_yuv_block(const u32 (&acc)[8], int px0, int py0, int W, const SurfView &yp, const SurfView &up, const SurfView &vp,
                                                bool pair = false) {
    if (NV >= 3) {  // a packed 4:2:2 frame's plane (in `yp`)
        store_packed422_block<NV>(acc, px0, py0, W, yp, pair);
        return;
    }
    // (W is even: the last block of a row holds four or two pixels)
    const bool half = px0 + 3 >= W;
    if (NV == 2) {  // an RGBA8 node texture (LayoutNode::render into a NodeTexture): the composited bytes as they are
        u8 *o = yp.ptr + b_off(py0, yp.pitch, px0 * 4);
        if (half) {
            *(uint2 *)o = make_uint2(acc[0], acc[1]);
            *(uint2 *)(o + yp.pitch) = make_uint2(acc[4], acc[5]);
        } else {
            *(uint4 *)o = make_uint4(acc[0], acc[1], acc[2], acc[3]);
            *(uint4 *)(o + yp.pitch) = make_uint4(acc[4], acc[5], acc[6], acc[7]);
        }
        return;
    }
    // RGBA -> Y'CbCr on the raw (gamma-encoded) bytes: rgba_to_yuv.wgsl:26-54 / rgba_to_nv12.wgsl:24-52 — the bytes yuv_component() /
    // unorm8() compute, through the fast path of smr_yuv_fast.h: three FMAs per value on the bytes as floats.  The twelve guard flags of the
    // block are gathered into one condition per lane and ONE branch leads to the reference sequence (yuv_block_repair).
    float cr[8], cg[8], cb[8];
#pragma unroll
    for (int k = 0; k < 8; k++) {
        cr[k] = (float)(acc[k] & 0xffu);
        cg[k] = (float)((acc[k] >> 8) & 0xffu);
        cb[k] = (float)((acc[k] >> 16) & 0xffu);
    }
    u32 yrow0 = 0, yrow1 = 0, u2 = 0, v2 = 0;  // Y' of the block's two rows, its two U and its two V bytes
    bool flagged = false;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        bool f0, f1;
        yrow0 |= yuvfast::convert<0>(cr[k], cg[k], cb[k], &f0) << (8 * k);
        yrow1 |= yuvfast::convert<0>(cr[4 + k], cg[4 + k], cb[4 + k], &f1) << (8 * k);
        flagged |= f0 | f1;
    }
    // chroma: the bilinear tap at the chroma texel centre = weights (1/2, 1/2) x (1/2, 1/2):
    //     (a * .5 + b * .5) * .5 + (c * .5 + d * .5) * .5  ==  ((a + b) + (c + d)) * .25   bit for bit
    // (a power of two scales exactly and commutes with rounding — the operands are 0 or >= 1/255, nowhere near the subnormals);
    // the fast path takes the block's byte sums (exact in f32)
#pragma unroll
    for (int j = 0; j < 2; j++) {
        const int a = 2 * j, b = 2 * j + 1, c = 4 + 2 * j, d = 4 + 2 * j + 1;
        const float sr = (cr[a] + cr[b]) + (cr[c] + cr[d]), sg = (cg[a] + cg[b]) + (cg[c] + cg[d]), sb = (cb[a] + cb[b]) + (cb[c] + cb[d]);
        bool f1, f2;
        u2 |= yuvfast::convert<1>(sr, sg, sb, &f1) << (8 * j);
        v2 |= yuvfast::convert<2>(sr, sg, sb, &f2) << (8 * j);
        flagged |= f1 | f2;
    }
    if (flagged) {
        YUV_SLOW_PATH_STAYS_A_BRANCH();
        yuv_block_repair(acc, yrow0, yrow1, u2, v2);
    }
    const u32 uv4 = (u2 & 0xffu) | ((v2 & 0xffu) << 8) | ((u2 & 0xff00u) << 8) | ((v2 & 0xff00u) << 16);  // NV12: U V U V
    const int cx = px0 >> 1, cy = py0 >> 1;
    if (pair) {  // (an interior tile: no half block, px0 = 4 * lane within the row)
        const bool odd = (px0 & 4) != 0;
        // the even lane gets its right neighbour's row 0, the odd lane its left neighbour's row 1
        const u32 ny = (u32)dev_mov_dpp_quad_swap((int)(odd ? yrow0 : yrow1));
        g_st_u32x2(yp.ptr + b_off(py0 + (odd ? 1 : 0), yp.pitch, px0 & ~7), odd ? ny : yrow0, odd ? yrow1 : ny);
        if (NV == 0) {
            const u32 nc = (u32)dev_mov_dpp_quad_swap((int)(odd ? u2 : v2));  // even: the neighbour's U pair, odd: the neighbour's V pair
            u8 *o = odd ? vp.ptr + b_off(cy, vp.pitch, cx & ~3) : up.ptr + b_off(cy, up.pitch, cx);
            g_st_u32(o, odd ? (nc | (v2 << 16)) : (u2 | (nc << 16)));
        } else {
            *(u32 *)(up.ptr + b_off(cy, up.pitch, cx * 2)) = uv4;
        }
        return;
    }
    if (half) {
        *(u16 *)(yp.ptr + b_off(py0, yp.pitch, px0)) = (u16)yrow0;
        *(u16 *)(yp.ptr + b_off(py0 + 1, yp.pitch, px0)) = (u16)yrow1;
    } else {
        *(u32 *)(yp.ptr + b_off(py0, yp.pitch, px0)) = yrow0;
        *(u32 *)(yp.ptr + b_off(py0 + 1, yp.pitch, px0)) = yrow1;
    }
    if (NV == 0) {
        if (half) {
            up.ptr[b_off(cy, up.pitch, cx)] = (u8)u2;
            vp.ptr[b_off(cy, vp.pitch, cx)] = (u8)v2;
        } else {
            *(u16 *)(up.ptr + b_off(cy, up.pitch, cx)) = (u16)u2;
            *(u16 *)(vp.ptr + b_off(cy, vp.pitch, cx)) = (u16)v2;
        }
    } else if (half) {
        *(u16 *)(up.ptr + b_off(cy, up.pitch, cx * 2)) = (u16)uv4;
    } else {
        *(u32 *)(up.ptr + b_off(cy, up.pitch, cx * 2)) = uv4;
    }
}

// One LDS atomic per wave hands the wave's flagged pixels their slots on the workgroup's list (uniform call).
__device__ __forceinline__ u32 list_slot(u32 *count, bool want) {
#ifdef SMR_EMU
    return want ? atomicAdd(count, 1u) : 0u;  // (the lane emulator has no wave votes)
#else
    const unsigned long long m = __ballot(want);
    if (m == 0ull) return 0u;
    const u32 rank = __builtin_amdgcn_mbcnt_hi((u32)(m >> 32), __builtin_amdgcn_mbcnt_lo((u32)m, 0u));  // flagged lanes below this one
    u32 base = 0u;
    if (want && rank == 0u) base = atomicAdd(count, (u32)__popcll(m));
    return (u32)__builtin_amdgcn_readlane((int)base, (int)__builtin_ctzll(m)) + rank;
#endif
}
__device__ __forceinline__ bool wave_any(bool v) {
#ifdef SMR_EMU
    return true;
#else
    return __ballot(v) != 0ull;
#endif
}

// Rows [band, band + rh) of tile `tile`, composited by the whole workgroup (uniform call; may be called again).
// NV = 0: planar Y,U,V (4:2:0); NV = 1: NV12 (Y + interleaved UV); NV = 2: RGBA8 surface (in `yp`); NV = 3 / 4: packed 4:2:2, UYVY / YUYV (the plane in `yp`)
// BIG: the layout list is longer than the LDS copy (B_MAX_LAYOUTS / B_MAX_MASKS) and is read where it lies in memory
// `pre`: the tile's record from k_classify_tiles — touching layers, start layer and tile_needs' bits of the WHOLE tile, valid for every
// band of it (a layer solid over the tile is solid over the band; a superset of the band's touching layers composites to the same
// pixels) — so a band's workgroup does not classify again.
//
// Three steps, one pixel per thread and sweep (a wave covers 64 consecutive pixels of a row), layer records through scalar registers:
//   A  every pixel's START: the topmost touched layer that is opaque, unrotated and solid at the pixel (else the tile's own start layer),
//      and that layer's value there — an opaque colour's bytes, a 1:1 texel, a filtered sample of a texture at a fractional position:
//      what compositing from the start layer upwards begins with (dst * (1 - 1) wipes what is below).  The layers are walked first and
//      each pixel keeps where its value lies (address, weights); then ALL fetches go out together: one round trip whatever the number
//      of layers (the earlier kernel composited layer after layer, sweep after sweep: a round trip for each).
//   B  the pixels that some layer above their start touches (the layers' pixel boxes) go on a list in LDS — the edge of a video tile,
//      a rounded corner, a label: a few dozen of a band's 512 pixels in a grid in motion.
//   C  the listed pixels are composited upwards from their start value, a thread per listed pixel, by compose_px — the one copy of the
//      general per-pixel code — and written back; the band is then converted and stored as 4 x 2 blocks.
template <int NV, bool BIG>
__device__ __forceinline__ void compose_full(const TileFull *__restrict__ pre, int band, int rh, const SurfView &yp, const SurfView &up, const SurfView &vp, int W, int H,
                                             const DevLayout *__restrict__ layouts_g, const DevMask *__restrict__ masks_g, int n, int n_masks,
                                             int srgb_and_ablate, const float *__restrict__ tables, int tiles_x, float *s_tab) {
    const int tile = (int)pre->tile;
    constexpr int BAND_PX = B_TILE_W * B_BAND_ROWS;
    constexpr int SWEEPS = 2;  // pixels per thread of steps A and B at a time (rows y and y + 2 of a four-row slab): the band is walked slab by slab
    static_assert(BAND_PX % 512 == 0 && BAND_PX <= 2048, "whole slabs; a list entry keeps the pixel's index in IDX_BITS bits");
    // a list entry: pixel index | (start layer + 1) << IDX_BITS — 16 bits while the list's layers fit the LDS copy, 32 for the build that reads the list in place
    constexpr int IDX_BITS = BIG ? 11 : (BAND_PX <= 1024 ? 10 : 11);
    constexpr bool WIDE = BIG || ((B_MAX_LAYOUTS + 1) > (1 << (16 - IDX_BITS)));
    typedef typename std::conditional<WIDE, u32, u16>::type entry_t;
    __shared__ u32 s_touch[MAX_LAYOUT_WORDS];
    __shared__ u32 s_px[BAND_PX];         // the band's RGBA8: every pixel's start value, then the listed pixels composited
    __shared__ entry_t s_list[BAND_PX];   // pixels some layer above their start touches
    __shared__ u32 s_count;
    // the whole layout list lives in LDS for the lifetime of the workgroup: one coalesced copy instead of a
    // dependent scalar-memory round trip per field per layer per wave
    __shared__ __attribute__((aligned(16))) DevLayout s_lay[B_MAX_LAYOUTS];
    __shared__ __attribute__((aligned(16))) DevMask s_mask[B_MAX_MASKS];
    int tid = threadIdx.x;
    B_KEEP_IN_LOOP(tid);  // (called band after band: the copy addresses below are formed per call, not held in registers across the calls)
    tid &= 255;           // (what the compiler knew about threadIdx.x)
    u32 acc[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};  // this thread's 4x2 output block, [row][col]: acc[r * 4 + c]
    const int tile_y = tile / tiles_x;
    const int tx0 = (tile - tile_y * tiles_x) * B_TILE_W, ty0 = tile_y * B_TILE_H + band;
    const int px0 = tx0 + 4 * (tid & 31), py0 = ty0 + 2 * (tid >> 5);  // this thread's 4x2 output block
    __syncthreads();  // (a previous call's readers of the shared tile are done)
    // (one round trip: every load of the list, the masks and the tables is issued before the first store — as loops with a load and a
    //  store per trip they were eight dependent trips to the L2)
    {
        static_assert(SMR_TABLE_FLOATS % 4 == 0 && SMR_TABLE_FLOATS / 4 <= 256, "one 16 B word of the tables per thread");
        constexpr int LW = (B_MAX_LAYOUTS * (int)(sizeof(DevLayout) / 16) + 255) / 256, MW = (B_MAX_MASKS * (int)(sizeof(DevMask) / 16) + 255) / 256;
        const uint4 *gl = (const uint4 *)layouts_g, *gm = (const uint4 *)masks_g, *gt = (const uint4 *)tables;
        const int nl = BIG ? 0 : n * (int)(sizeof(DevLayout) / 16), nm = BIG ? 0 : n_masks * (int)(sizeof(DevMask) / 16);
        uint4 wl[LW], wm[MW], wt = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
        for (int k = 0; k < LW; k++) {
            wl[k] = wt;
            if (tid + 256 * k < nl) wl[k] = gl[tid + 256 * k];
        }
#pragma unroll
        for (int k = 0; k < MW; k++) {
            wm[k] = wt;
            if (tid + 256 * k < nm) wm[k] = gm[tid + 256 * k];
        }
        if (tid < SMR_TABLE_FLOATS / 4) wt = gt[tid];
        u32 touch_w = 0u;
        if (tid < MAX_LAYOUT_WORDS) touch_w = pre->touch[tid];
#pragma unroll
        for (int k = 0; k < LW; k++)
            if (tid + 256 * k < nl) ((uint4 *)s_lay)[tid + 256 * k] = wl[k];
#pragma unroll
        for (int k = 0; k < MW; k++)
            if (tid + 256 * k < nm) ((uint4 *)s_mask)[tid + 256 * k] = wm[k];
        if (tid < SMR_TABLE_FLOATS / 4) ((uint4 *)s_tab)[tid] = wt;
        if (tid < MAX_LAYOUT_WORDS) s_touch[tid] = touch_w;
        if (tid == 0) s_count = 0u;
    }
    const DevLayout *layouts = BIG ? layouts_g : s_lay;
    const DevMask *masks = BIG ? masks_g : s_mask;
    const int srgb = srgb_and_ablate & 1;
    const int ablate = srgb_and_ablate >> 8;  // profiling only (SMR_ABLATE bits 8..): 1 dispatch only, 2 list only, 4 no per-pixel start, 8 start values only, 16 no compositing
    const int start = pre->start;
    __syncthreads();
    if (ablate & (1 | 2 | 16)) return;
    if (ty0 >= H) return;
    const int words = (n + 31) >> 5;
    const bool no_block = px0 >= W || py0 >= H || 2 * (tid >> 5) >= rh;      // (W, H even: a block has four or two columns, always two rows)
    const int nsweeps = (B_TILE_W * rh) / 256;
    const float *dec = s_tab, *thr = s_tab + 256;
    const int sx = tx0 + (tid & (B_TILE_W - 1));  // this thread's pixels: column sx, rows ty0 + (tid >> 7) + 2 * sweep

    // ---- A. start layer and start value of every pixel, B. the list — a slab of four rows at a time
#pragma unroll 1
    for (int slab = 0; slab < nsweeps; slab += SWEEPS) {
    enum { K_NONE = 0, K_COLOUR = 1, K_TEXEL = 2, K_QUAD = 3 };
    int sp[SWEEPS];          // the layer the pixel starts from (-1: none, a cleared pixel)
    u32 kind[SWEEPS];        // where its start value lies
    const u8 *sbase[SWEEPS];
    u32 so[SWEEPS][4];       // K_COLOUR: [0] = the encoded bytes; K_TEXEL: [0] = byte offset; K_QUAD: the footprint's four byte offsets
    float swx[SWEEPS], swy[SWEEPS];
#pragma unroll
    for (int s = 0; s < SWEEPS; s++) { sp[s] = -1; kind[s] = K_NONE; sbase[s] = nullptr; so[s][0] = so[s][1] = so[s][2] = so[s][3] = 0u; swx[s] = swy[s] = 0.0f; }
    const auto claim = [&](const DevLayout &L, int li, int s, int py) {
        sp[s] = li;
        if (L.type != 0) {
            kind[s] = K_COLOUR;
            so[s][0] = L.solid_px;
        } else if (L.flags & DL_ALIGNED) {
            kind[s] = K_TEXEL;
            sbase[s] = L.src.ptr;
            so[s][0] = (u32)b_off(clampi(py - L.iy, 0, L.tex_h - 1), L.src.pitch, clampi(sx - L.ix, 0, L.tex_w - 1) * 4);
        } else {
            kind[s] = K_QUAD;
            sbase[s] = L.src.ptr;
            const SampledAxis X = sampled_axis_x(L, sx), Y = sampled_axis_y(L, py);
            so[s][0] = Y.o0 + X.o0; so[s][1] = Y.o0 + X.o1; so[s][2] = Y.o1 + X.o0; so[s][3] = Y.o1 + X.o1;
            swx[s] = X.f; swy[s] = Y.f;
        }
    };
    // (topmost first: a pixel is claimed once)
    for (int wi = (ablate & 4) ? -1 : words - 1; wi >= (start < 0 ? 0 : (start >> 5)); wi--) {  // (4: profiling, the tile's start layer only)
        u32 bits = __builtin_amdgcn_readfirstlane(s_touch[wi]);
        if (start >= 0 && wi == (start >> 5)) bits &= ~((2u << (start & 31)) - 1u);  // strictly above start
        while (bits) {
            const int b = 31 - __builtin_clz(bits);
            bits &= ~(1u << b);
            const int li = (wi << 5) + b;
            const DevLayout L = load_uniform(&layouts[li]);
            if (!layout_base_opaque(L) || !(L.flags & DL_UNROTATED)) continue;
#pragma unroll
            for (int s = 0; s < SWEEPS; s++) {
                const int py = ty0 + (tid >> 7) + 2 * (slab + s);
                const float fx = (float)sx + 0.5f, fy = (float)py + 0.5f;
                if (slab + s < nsweeps && kind[s] == K_NONE && layout_solid_box(L, masks, fx, fy, fx, fy)) claim(L, li, s, py);
            }
        }
    }
    if (start >= 0) {  // (opaque, unrotated and solid over the whole tile: classify_layouts)
        const DevLayout L = load_uniform(&layouts[start]);
#pragma unroll
        for (int s = 0; s < SWEEPS; s++)
            if (slab + s < nsweeps && kind[s] == K_NONE) claim(L, start, s, ty0 + (tid >> 7) + 2 * (slab + s));
    }
    u32 st[SWEEPS][4];
#pragma unroll
    for (int s = 0; s < SWEEPS; s++) {  // (every fetch of the band before the first use)
        st[s][0] = st[s][1] = st[s][2] = st[s][3] = 0u;
        if (kind[s] >= K_TEXEL) st[s][0] = g_ld_u32(sbase[s] + so[s][0]);
        if (kind[s] == K_QUAD) { st[s][1] = g_ld_u32(sbase[s] + so[s][1]); st[s][2] = g_ld_u32(sbase[s] + so[s][2]); st[s][3] = g_ld_u32(sbase[s] + so[s][3]); }
    }
    u32 val[SWEEPS];
#pragma unroll
    for (int s = 0; s < SWEEPS; s++) {
        // (compose_px's results for a layer that is opaque and solid at the pixel: an opaque colour stores its bytes; an opaque 1:1 texel
        //  stores its own bytes, encode(decode(b)) == b; an opaque sample is filtered and encoded: composite_sampled_opaque)
        val[s] = kind[s] == K_COLOUR ? so[s][0] : kind[s] == K_TEXEL ? st[s][0] : 0u;
        if (kind[s] == K_QUAD) val[s] = filter_opaque_quad(st[s][0], st[s][1], st[s][2], st[s][3], swx[s], swy[s], srgb, dec, thr);
    }

    // ---- B. the pixels a layer above their start touches
    bool listed[SWEEPS];
#pragma unroll
    for (int s = 0; s < SWEEPS; s++) listed[s] = false;
    if (!(ablate & 8))
        for (int wi = start < 0 ? 0 : (start >> 5); wi < words; wi++) {
            u32 bits = __builtin_amdgcn_readfirstlane(s_touch[wi]);
            if (start >= 0 && wi == (start >> 5)) bits &= ~((2u << (start & 31)) - 1u);
            while (bits) {
                const int li = (wi << 5) + __builtin_ctz(bits);
                bits &= bits - 1;
                const DevLayout *Lp = &layouts[li];
                const int bx0 = __builtin_amdgcn_readfirstlane(Lp->bx0), bx1 = __builtin_amdgcn_readfirstlane(Lp->bx1);
                const int by0 = __builtin_amdgcn_readfirstlane(Lp->by0), by1 = __builtin_amdgcn_readfirstlane(Lp->by1);
#pragma unroll
                for (int s = 0; s < SWEEPS; s++) {
                    const int py = ty0 + (tid >> 7) + 2 * (slab + s);
                    if (li > sp[s] && sx >= bx0 && sx < bx1 && py >= by0 && py < by1) listed[s] = true;
                }
            }
        }
#pragma unroll
    for (int s = 0; s < SWEEPS; s++) {
        if (slab + s >= nsweeps) break;  // (uniform)
        const int idx = (slab + s) * 256 + tid, py = ty0 + (tid >> 7) + 2 * (slab + s);
        s_px[idx] = val[s];
        const bool want = listed[s] && sx < W && py < H;
        const u32 slot = list_slot(&s_count, want);
        if (want) s_list[slot] = (entry_t)((u32)idx | ((u32)(sp[s] + 1) << IDX_BITS));
    }
    }
    __syncthreads();

    // ---- C. the listed pixels, composited upwards from their start value
    const u32 total = s_count;
#pragma unroll 1
    for (u32 k0 = 0; k0 < total; k0 += 256u) {
        const bool act = k0 + (u32)tid < total;
        const u32 e = act ? (u32)s_list[k0 + tid] : 0u;
        const int idx = (int)(e & ((1u << IDX_BITS) - 1u)), from = (int)(e >> IDX_BITS) - 1;
        const int px = tx0 + (idx & (B_TILE_W - 1)), py = ty0 + (idx >> 7);
        u32 a = s_px[idx];
        for (int wi = start < 0 ? 0 : (start >> 5); wi < words; wi++) {
            u32 bits = __builtin_amdgcn_readfirstlane(s_touch[wi]);
            if (start >= 0 && wi == (start >> 5)) bits &= ~((2u << (start & 31)) - 1u);
            while (bits) {
                const int li = (wi << 5) + __builtin_ctz(bits);
                bits &= bits - 1;
                const DevLayout *Lp = &layouts[li];
                const int bx0 = __builtin_amdgcn_readfirstlane(Lp->bx0), bx1 = __builtin_amdgcn_readfirstlane(Lp->bx1);
                const int by0 = __builtin_amdgcn_readfirstlane(Lp->by0), by1 = __builtin_amdgcn_readfirstlane(Lp->by1);
                const bool need = act && li > from && px >= bx0 && px < bx1 && py >= by0 && py < by1;
                if (!wave_any(need)) continue;  // (none of this wave's pixels: the layer's record stays where it is)
                const DevLayout L = load_uniform(Lp);
                u32 raw = 0u;
                if (need && L.type == 0 && (L.flags & DL_ALIGNED) && L.src_kind != 0) raw = aligned_texel(L, px, py);
                if (need) a = compose_px(a, L, masks, px, py, false, raw, srgb, dec, thr);
            }
        }
        if (act) s_px[idx] = a;
    }
    __syncthreads();
    if (!no_block) {
        int ltid = tid;
        B_KEEP_IN_LOOP(ltid);  // (the block's position again, here: its store addresses are not carried through the three steps above)
        const int lx0 = 4 * (ltid & 31), ly0 = 2 * (ltid >> 5), px0 = tx0 + lx0, py0 = ty0 + ly0;
        const uint4 t0 = *(const uint4 *)&s_px[ly0 * B_TILE_W + lx0], t1 = *(const uint4 *)&s_px[(ly0 + 1) * B_TILE_W + lx0];
        acc[0] = t0.x; acc[1] = t0.y; acc[2] = t0.z; acc[3] = t0.w;
        acc[4] = t1.x; acc[5] = t1.y; acc[6] = t1.z; acc[7] = t1.w;
        // (an interior tile's band of four or eight rows: whole waves hold blocks, the others skipped this branch together)
        const bool pair = tx0 + B_TILE_W <= W && tile_y * B_TILE_H + B_TILE_H <= H && (rh & 3) == 0 && planes_pair_aligned<NV>(yp, up, vp);
        store_yuv_block<NV>(acc, px0, py0, W, yp, up, vp, pair);
    }
}

// Copy tiles per workgroup: B_COPY_TILES is the number of tiles a workgroup holds AT ONCE (one: measured with two and four, whose texels were
// all live and converted back to back — 29 -> 37 us in round 3, 22.5 -> 29.9 us in round 4); the lane emulator's harness sizes its grid by it.
// B_COPY_RUN is the number of consecutive row-major tiles the product launch gives a copy workgroup, which walks them ONE AFTER THE OTHER
// with the next tile's texels on their way while it converts this one's: a wave's start-up (kernel arguments, the division by tiles_x, the
// class record, and only then the texel request) is paid once per run instead of once per tile, and the conversion overlaps the trip.
// Even values: two adjacent tiles' 64-byte chroma rows complete 128-byte lines from one CU.  The grid stays several times what is resident
// (configs[2]: 4 050 tiles -> 2 025 workgroups against 256 CUs x 6): the hardware still balances the workgroups.
constexpr int B_COPY_TILES = 1;
#ifndef SMR_COPY_RUN
#define SMR_COPY_RUN 2
#endif
constexpr int B_COPY_RUN = SMR_COPY_RUN;
static_assert(B_COPY_RUN >= 1 && B_COPY_RUN <= 4, "a short run: the grid stays larger than what is resident");

// The eight texels of this lane's 4 x 2 block of a copy tile (clear / colour: the fill value), requested and not waited for.
// `aligned` (uniform): the tile's texel rows can be read 16 bytes at a time; a lane with nothing to read reads the tables instead — no
// branch between the loads.  A 1:1 blit of an opaque texture: decode -> encode is the identity.
__device__ __forceinline__ void copy_tile_texels(const TileClass &c, bool on, int cols, int bx, int by, const float *__restrict__ tables, u32 (&t)[8]) {
    const u32 fill = c.kind == TC_COLOUR ? c.pitch_or_px : 0u;
#pragma unroll
    for (int q = 0; q < 8; q++) t[q] = fill;
    if (c.kind != TC_TEXTURE) return;  // (uniform)
    // (cols = the output's columns from the tile's first on; a width of 2 mod 4 makes the row's last block two pixels wide)
    const bool aligned = ((((uintptr_t)c.base) | c.pitch_or_px) & 15) == 0 && !((cols & 3) != 0 && cols < B_TILE_W);
    if (aligned) {
        const u8 *r0 = on ? c.base + b_off(by, c.pitch_or_px, bx * 4) : (const u8 *)tables;
        const u8 *r1 = on ? r0 + c.pitch_or_px : (const u8 *)tables;
        const uint4 ra = g_ld_u32x4(r0), rb = g_ld_u32x4(r1);  // (global loads: a base from a record in memory is a generic pointer to the compiler — smr_internal.h)
        t[0] = ra.x; t[1] = ra.y; t[2] = ra.z; t[3] = ra.w;
        t[4] = rb.x; t[5] = rb.y; t[6] = rb.z; t[7] = rb.w;
    } else if (on) {
        const u8 *r0 = c.base + b_off(by, c.pitch_or_px, bx * 4), *r1 = r0 + c.pitch_or_px;
#pragma unroll
        for (int q = 0; q < 4; q++)
            if (bx + q < cols) { t[q] = g_ld_u32(r0 + 4 * q); t[4 + q] = g_ld_u32(r1 + 4 * q); }
    }
}

template <int NV, bool BIG>
__global__ __launch_bounds__(256, B_MIN_WAVES) void k_compose_output(SurfView yp, SurfView up, SurfView vp, int W, int H,
                                                        const DevLayout *__restrict__ layouts_g, const DevMask *__restrict__ masks_g,
                                                        int n, int n_masks, int srgb_and_ablate, const float *__restrict__ tables,
                                                        int tiles_x, int tiles, const TileClass *__restrict__ tc, const TileList *__restrict__ full,
                                                        int n_banded, int counter) {
    const int tid = threadIdx.x;
#if defined(SMR_PRIO_COMPOSE) && !defined(SMR_EMU)
    __builtin_amdgcn_s_setprio(SMR_PRIO_COMPOSE);
#endif
    __shared__ __attribute__((aligned(16))) float s_tab[SMR_TABLE_FLOATS];  // decode / encode tables (whoever needs them loads them)
    // The first `n_banded` workgroups take the bands of the tiles that need compositing, an entry of the TileList each (the host sized the
    // grid from the list's length when it knows it, from its own prediction otherwise) — they are latency-bound and would be the tail of
    // the kernel.  Every other workgroup g = blockIdx.x - n_banded takes the run of consecutive row-major tiles [g T, min((g + 1) T, tiles)),
    // T = ceil(tiles / (gridDim.x - n_banded)): the product launch sizes the grid for T = B_COPY_RUN, a grid of n_banded + tiles gives T = 1.
    // (the compositing path is most of the kernel's code: it is instantiated once, inside the walk, and both ways into it — a band of a
    //  listed tile; a tile the list had no room for — only choose its arguments)
    const int rest = (int)blockIdx.x - n_banded;
    int t_begin = 0, t_end = 0;  // the run
    bool later = false, left_out = false;  // (uniform) tiles of the run that are sampled or select tiles / that are composited here: after the walk
    if (rest < 0) {
        if (blockIdx.x >= full->count[counter]) return;
    } else {
        const int groups = (int)gridDim.x - n_banded;
        const int run = (tiles + groups - 1) / groups;
        t_begin = rest * run;
        t_end = min(t_begin + run, tiles);
        if (t_begin >= t_end) return;
        // ---- copy tiles, straight from their class records (k_classify_tiles): no layout list, no classification, no barrier.
        // c0 = this tile's record, c1 = the next one's (its texels are requested before this tile is converted), c2 = on its way;
        // cur = this tile's texels, nxt = the next one's.
        const bool ablate_copy = ((srgb_and_ablate >> 8) & 64) != 0;  // (profiling)
        const bool planes_ok = planes_pair_aligned<NV>(yp, up, vp);
        int t = t_begin;
        const int ty = t / tiles_x;
        int tx0 = (t - ty * tiles_x) * B_TILE_W, ty0 = ty * B_TILE_H;  // this tile's first pixel: computed once, stepped
        TileClass c0 = tc[t], c1 = tc[min(t + 1, tiles - 1)], c2;
        u32 cur[8];
        copy_tile_texels(c0, tx0 + 4 * (tid & 31) < W && ty0 + 2 * (tid >> 5) < H && !ablate_copy, W - tx0, 4 * (tid & 31), 2 * (tid >> 5), tables, cur);
#pragma unroll 1
        for (;;) {
            // (the lane's position is formed again for every tile: what is derived from it is not held in registers across the walk)
            int ltid = tid;
            B_KEEP_IN_LOOP(ltid);
            const int bx = 4 * (ltid & 31), by = 2 * (ltid >> 5);
            const int px0 = tx0 + bx, py0 = ty0 + by;
            const bool inside = px0 < W && py0 < H;
            const bool pair = planes_ok && tx0 + B_TILE_W <= W && ty0 + B_TILE_H <= H;  // (uniform) every lane holds a whole block
            c2 = tc[min(t + 2, tiles - 1)];
            // the next tile's texels, requested before this tile's arithmetic
            u32 nxt[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
            const bool wrap = tx0 + B_TILE_W >= tiles_x * B_TILE_W;
            const int nx0 = wrap ? 0 : tx0 + B_TILE_W, ny0 = wrap ? ty0 + B_TILE_H : ty0;
            if (t + 1 < t_end) copy_tile_texels(c1, nx0 + bx < W && ny0 + by < H && !ablate_copy, W - nx0, bx, by, tables, nxt);
            if (c0.kind <= TC_TEXTURE) {
                if (inside && !ablate_copy) store_yuv_block<NV>(cur, px0, py0, W, yp, up, vp, pair);
            } else if (c0.kind == TC_SAMPLED || c0.kind == TC_SELECT) {
                later = true;  // (below, once the run's copies are on their way: those paths want the registers the walk holds)
            } else if (c0.kind == TC_FULL && (int)c0.pitch_or_px + (int)(uintptr_t)c0.base > n_banded) {
                left_out = true;
            }
            // (TC_SKIP: wave A writes the tile; TC_FULL with a workgroup per band: nothing to do here)
            if (++t >= t_end) break;
#pragma unroll
            for (int q = 0; q < 8; q++) cur[q] = nxt[q];
            c0 = c1; c1 = c2;
            tx0 = nx0; ty0 = ny0;
        }
        if (!later && !left_out) return;
    }
    // ---- the run's sampled and select tiles as they are met (uniform).  Nothing of the walk above is alive here but the run itself.
    if (later) {
#pragma unroll 1
        for (int t = t_begin; t < t_end; t++) {
            const TileClass c = tc[t];
            if (c.kind != TC_SAMPLED && c.kind != TC_SELECT) continue;
            int ltid = tid;
            B_KEEP_IN_LOOP(ltid);  // (as above)
            const int ty = t / tiles_x, tx0 = (t - ty * tiles_x) * B_TILE_W, ty0 = ty * B_TILE_H;
            const int px0 = tx0 + 4 * (ltid & 31), py0 = ty0 + 2 * (ltid >> 5);
            const bool inside = px0 < W && py0 < H;
            const bool pair = tx0 + B_TILE_W <= W && ty0 + B_TILE_H <= H && planes_pair_aligned<NV>(yp, up, vp);  // (uniform)
            if (c.kind == TC_SAMPLED) {
                // sampled tiles: one layer's record straight from the list in memory, eight independent pixels per thread
                if ((srgb_and_ablate >> 8) & 32) continue;  // (32: profiling, no sampled tiles)
                __syncthreads();
                for (int i = ltid; i < SMR_TABLE_FLOATS; i += 256) s_tab[i] = tables[i];
                __syncthreads();
                const DevLayout L = load_uniform(&layouts_g[c.pitch_or_px]);
                if (inside) {
                    u32 a[8];
                    composite_sampled_opaque_block(L, px0, py0, srgb_and_ablate & 1, s_tab, s_tab + 256, a);  // (column / row halves of the sample positions once each)
                    store_yuv_block<NV>(a, px0, py0, W, yp, up, vp, pair);
                }
            } else if (c.kind == TC_SELECT) {
                // select tiles: every pixel a copy from the topmost listed layer whose pixel box holds it (records through scalar loads: the
                // layer numbers are the workgroup's)
                u32 a[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
                u32 open_px = 0xffu;  // pixels no layer has claimed yet
#pragma unroll 1
                for (int q = 0; q < 4; q++) {
                    const u32 li = (c.pitch_or_px >> (8 * q)) & 0xffu;
                    if (li == 0xffu) break;  // (uniform)
                    const DevLayout &L = layouts_g[li];
                    const int lx0 = L.bx0, ly0 = L.by0, lx1 = L.bx1, ly1 = L.by1;
                    const bool colour = L.type != 0;
                    const u32 solid = L.solid_px;
#pragma unroll
                    for (int i = 0; i < 8; i++) {
                        const int px = px0 + (i & 3), py = py0 + (i >> 2);
                        if (((open_px >> i) & 1u) && px >= lx0 && px < lx1 && py >= ly0 && py < ly1) {
                            a[i] = colour ? solid : aligned_texel(L, px, py);
                            open_px &= ~(1u << i);
                        }
                    }
                }
                if (inside) store_yuv_block<NV>(a, px0, py0, W, yp, up, vp, pair);
            }
        }
        if (!left_out) return;
    }
    // ---- compositing (uniform): one band of a listed tile, or — band after band — the bands of every tile of the run that the list's bound left
    // out (the host's bound was short)
#pragma unroll 1
    for (int t = t_begin;; t++) {
        const TileFull *e;
        int entries = 1;
        if (rest < 0) {
            e = &full->e[blockIdx.x];
        } else {
            if (t >= t_end) break;
            const TileClass c = tc[t];
            if (!(c.kind == TC_FULL && (int)c.pitch_or_px + (int)(uintptr_t)c.base > n_banded)) continue;
            e = &full->e[c.pitch_or_px];
            entries = (int)(uintptr_t)c.base;
        }
#ifndef SMR_COMPOSE_NO_FULL  // (profiling builds only: the compositing path compiled out — what the copy paths alone need in registers and time)
#pragma unroll 1
        for (int j = 0; j < entries; j++) {
            if (rest >= 0 && (int)(e - full->e) + j < n_banded) continue;  // (that band has a workgroup of its own)
            const u32 bw = __builtin_amdgcn_readfirstlane(e[j].band);
            compose_full<NV, BIG>(&e[j], (int)(bw & 0xffu), (int)(bw >> 8), yp, up, vp, W, H, layouts_g, masks_g, n, n_masks, srgb_and_ablate, tables, tiles_x, s_tab);
        }
#endif
        if (rest < 0) break;
    }
}

}  // namespace
