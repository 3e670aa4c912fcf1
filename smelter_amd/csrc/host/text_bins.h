// text_bins.h — tx_plan: the tile bins of one Text job of k_text_nodes (smr_text_nodes.h), made on the host.
//
// A job's surface is cut into the 64 x 16 tiles of smr_node_tiles.h, row-major.  Tile t's bin is bin_glyph[bin_first[t] .. bin_first[t + 1]):
// the indices, ASCENDING (painter's order), of the glyphs whose rectangle, clipped to the surface, intersects the tile.  A workgroup of the
// kernel walks its own bin and nothing else.  A glyph with w <= 0 or h <= 0, or wholly outside the surface, lands in no bin.
//
// Plain C++17 without HIP: the launcher (smr_text_nodes.hip), the emulator driver (tests/emu/emu_text_nodes.cpp) and the sanitizer driver
// (tests/san/text_bins_driver.cpp, under g++) all include it.  Clipping and tile ranges are computed in 64 bits: dst_x + w of a caller's
// glyph may overflow int32.
#pragma once

#include <cstdint>

#include "smr.h"

#define SMR_TEXT_TILE_W 64  // == SMR_NODE_TILE_W / _H (smr_text_nodes.h asserts it)
#define SMR_TEXT_TILE_H 16

static inline uint32_t tx_tiles_x(int w) { return w > 0 ? ((uint32_t)w + SMR_TEXT_TILE_W - 1) / SMR_TEXT_TILE_W : 0; }
static inline uint32_t tx_tiles_y(int h) { return h > 0 ? ((uint32_t)h + SMR_TEXT_TILE_H - 1) / SMR_TEXT_TILE_H : 0; }
static inline uint32_t tx_tiles(int w, int h) { return tx_tiles_x(w) * tx_tiles_y(h); }

// The tiles glyph g touches on a w x h surface: [tx0, tx1] x [ty0, ty1], or false for none
struct TxRange {
    uint32_t tx0, tx1, ty0, ty1;
};
static inline bool tx_range(int w, int h, const smr_glyph &g, TxRange &r) {
    if (w <= 0 || h <= 0 || g.w <= 0 || g.h <= 0) return false;
    const int64_t x0 = g.dst_x > 0 ? (int64_t)g.dst_x : 0, y0 = g.dst_y > 0 ? (int64_t)g.dst_y : 0;
    int64_t x1 = (int64_t)g.dst_x + g.w, y1 = (int64_t)g.dst_y + g.h;  // (one past the last texel)
    if (x1 > w) x1 = w;
    if (y1 > h) y1 = h;
    if (x0 >= x1 || y0 >= y1) return false;
    r.tx0 = (uint32_t)(x0 / SMR_TEXT_TILE_W); r.tx1 = (uint32_t)((x1 - 1) / SMR_TEXT_TILE_W);
    r.ty0 = (uint32_t)(y0 / SMR_TEXT_TILE_H); r.ty1 = (uint32_t)((y1 - 1) / SMR_TEXT_TILE_H);
    return true;
}

// The length bin_glyph needs (the sum over the glyphs of the tiles each touches), in time linear in n: what the launcher sizes its block by
// before it bins anything.
static inline uint64_t tx_entries(int w, int h, const smr_glyph *glyphs, uint32_t n) {
    uint64_t total = 0;
    TxRange r;
    for (uint32_t i = 0; i < n; i++)
        if (tx_range(w, h, glyphs[i], r)) total += (uint64_t)(r.tx1 - r.tx0 + 1) * (r.ty1 - r.ty0 + 1);
    return total;
}

// Fills bin_first[tx_tiles(w, h) + 1] and bin_glyph[tx_entries(w, h, glyphs, n)].  False (nothing usable written) when the entries do not fit
// 32 bits.  A counting sort in two passes over the glyphs in index order, so every bin comes out ascending.
static inline bool tx_plan(int w, int h, const smr_glyph *glyphs, uint32_t n, uint32_t *bin_first, uint32_t *bin_glyph) {
    const uint32_t tiles_x = tx_tiles_x(w), tiles = tx_tiles(w, h);
    if (tx_entries(w, h, glyphs, n) > UINT32_MAX) return false;
    for (uint32_t t = 0; t <= tiles; t++) bin_first[t] = 0;
    TxRange r;
    // counts, one slot up: bin_first[t + 1] = the glyphs of tile t
    for (uint32_t i = 0; i < n; i++) {
        if (!tx_range(w, h, glyphs[i], r)) continue;
        for (uint32_t ty = r.ty0; ty <= r.ty1; ty++)
            for (uint32_t tx = r.tx0; tx <= r.tx1; tx++) bin_first[ty * tiles_x + tx + 1]++;
    }
    for (uint32_t t = 0; t < tiles; t++) bin_first[t + 1] += bin_first[t];
    // fill: bin_first[t] runs up to the start of tile t + 1 ...
    for (uint32_t i = 0; i < n; i++) {
        if (!tx_range(w, h, glyphs[i], r)) continue;
        for (uint32_t ty = r.ty0; ty <= r.ty1; ty++)
            for (uint32_t tx = r.tx0; tx <= r.tx1; tx++) bin_glyph[bin_first[ty * tiles_x + tx]++] = i;
    }
    // ... and is moved back one slot
    for (uint32_t t = tiles; t > 0; t--) bin_first[t] = bin_first[t - 1];
    bin_first[0] = 0;
    return true;
}
