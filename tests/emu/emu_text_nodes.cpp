// TEST INFRASTRUCTURE — not part of the product; nothing in smelter_amd/ builds, links or loads this.
//
// k_text_nodes' source (smelter_amd/csrc/smr_text_nodes.h: tx_plan and tx_batch_plan on the host, tx_workgroup per thread) compiled for the
// CPU, so that tests/test_emu_text_nodes.py can run one launch — every workgroup, every thread, in turn: threads do not talk to each other —
// on buffers that are exactly as large as what they hold (emu_guard.h: the byte after, or before, them is an unmapped page).  Shims, tables
// and the alignment rule: emu_node_kernel.h.  Surface, records, bin_first, bin_glyph and atlas of a job are five buffers of their own: in
// guard mode 1 each ENDS on an unmapped page (the atlas on its last byte).  Every byte of a surface's buffer outside the job's texels — the
// bytes before its base, its row padding — is compared with what it held before the launch (a seeded pattern in guard mode 3, as
// emu_pad_fill makes it; a sentinel otherwise), and every texel inside starts from a value the kernel must replace.
#include <cmath>

#include "emu_node_kernel.h"
#include "smr_text_nodes.h"
#include "host/text_bins.h"

static inline u8 outside_byte(size_t off, u32 seed) { return emu_guard_mode == 3 ? emu_pad_byte(off, seed) : (u8)0xc3; }

// What smr_text_nodes does to a colour on the host (smr_text_nodes.h, tx_glyph_colour): clamp, and sRGB -> linear in f64
static inline float prepared(float v, int srgb) {
    v = !(v > 0.0f) ? 0.0f : (v > 1.0f ? 1.0f : v);
    if (!srgb) return v;
    const double c = (double)v;
    return (float)(c < 0.04045 ? c / 12.92 : pow((c + 0.055) / 1.055, 2.4));
}

// Job i: a w[i] x h[i] RGBA8 surface in a buffer of exactly off[i] + pitch[i] * (h[i] - 1) + w[i] * 4 bytes (0 texels: off[i] bytes) whose
// rows are pitch[i] bytes apart and start off[i] bytes in; background bg[4 i ..]; glyphs[i][0 .. n_glyphs[i]) over the tight
// atlas_w[i] x atlas_h[i] coverage atlas[i].  After the launch the texels come back tight in px_out[i]; wide_out[i]: 1 = whole groups went
// as 16-byte stores.  Returns the number of workgroups the launch has, -77 after naming a byte outside a job's texels that changed, -78
// after naming a bin that is not what the kernel may rely on, or another value < 0.
extern "C" int emu_text_nodes(int n, const int *w, const int *h, const u32 *pitch, const u32 *off, const float *bg, const smr_glyph *const *glyphs,
                              const u32 *n_glyphs, const u8 *const *atlas, const u32 *atlas_w, const u32 *atlas_h, int srgb, u8 *const *px_out, u32 *wide_out) {
    if (n < 0 || n > SMR_NODE_MAX_JOBS) return -1;
    const EmuTables tables;
    if (!tables.ptr) return -9;
    const float *tab = tables.ptr;
    const size_t align = emu_surface_align();

    std::vector<GuardBuf> buf((size_t)n), rec((size_t)n), first((size_t)n), bin((size_t)n), atl((size_t)n);
    std::vector<size_t> bytes((size_t)n);
    TextBatch B;
    memset(&B, 0, sizeof(B));
    B.n = (u32)n;
    B.srgb = srgb ? 1u : 0u;
    for (int i = 0; i < n; i++) {
        if (w[i] < 0 || h[i] < 0) return -1;
        const bool empty = w[i] == 0 || h[i] == 0;
        if (!empty && (pitch[i] < (u32)w[i] * 4 || (pitch[i] & 3u) || (off[i] & 3u))) return -1;
        bytes[i] = off[i] + (empty ? 0 : (size_t)pitch[i] * (h[i] - 1) + (size_t)w[i] * 4);
        buf[i].alloc(bytes[i] ? bytes[i] : 4, 0, align);
        for (size_t k = 0; k < bytes[i]; k++) buf[i].ptr[k] = outside_byte(k, 2000u + (u32)i);
        const u32 ng = n_glyphs[i];
        for (u32 k = 0; k < ng; k++) {
            const smr_glyph &g = glyphs[i][k];
            if (g.w < 0 || g.h < 0 || g.atlas_x < 0 || g.atlas_y < 0 || (u32)(g.atlas_x + g.w) > atlas_w[i] || (u32)(g.atlas_y + g.h) > atlas_h[i]) return -2;
        }
        // records, bins and atlas as the launcher packs them, each in a buffer of exactly its size
        const u32 tiles = tx_tiles(w[i], h[i]);
        const uint64_t entries = tx_entries(w[i], h[i], glyphs[i], ng);
        rec[i].alloc(ng ? (size_t)ng * sizeof(TextGlyph) : 4, 0, 4);
        first[i].alloc(((size_t)tiles + 1) * 4, 0, 4);
        bin[i].alloc(entries ? (size_t)entries * 4 : 4, 0, 4);
        const size_t a_bytes = (size_t)atlas_w[i] * atlas_h[i];
        atl[i].alloc(a_bytes ? a_bytes : 1, 0, 1);
        if (a_bytes) memcpy(atl[i].ptr, atlas[i], a_bytes);
        TextGlyph *R = (TextGlyph *)rec[i].ptr;
        for (u32 k = 0; k < ng; k++) {
            const smr_glyph &g = glyphs[i][k];
            R[k] = TextGlyph{g.dst_x, g.dst_y, g.w, g.h, g.atlas_x, g.atlas_y, prepared(g.color[0], srgb), prepared(g.color[1], srgb), prepared(g.color[2], srgb), g.color[3]};
        }
        u32 *F = (u32 *)first[i].ptr, *G = (u32 *)bin[i].ptr;
        if (!tx_plan(w[i], h[i], glyphs[i], ng, F, G)) return -3;
        // what the kernel relies on: monotone firsts that end on the entry count; indices in range, ascending within a bin
        if (F[0] != 0 || F[tiles] != entries) { fprintf(stderr, "bins: job %d: first[0] %u, first[%u] %u, %llu entries\n", i, F[0], tiles, F[tiles], (unsigned long long)entries); return -78; }
        for (u32 t = 0; t < tiles; t++) {
            if (F[t] > F[t + 1]) { fprintf(stderr, "bins: job %d: first[%u] %u > first[%u] %u\n", i, t, F[t], t + 1, F[t + 1]); return -78; }
            for (u32 e = F[t]; e < F[t + 1]; e++)
                if (G[e] >= ng || (e > F[t] && G[e] <= G[e - 1])) { fprintf(stderr, "bins: job %d, tile %u: entry %u is glyph %u after %u of %u\n", i, t, e, G[e], e > F[t] ? G[e - 1] : 0u, ng); return -78; }
        }
        TextJob &J = B.j[i];
        J.dst.ptr = buf[i].ptr + off[i]; J.dst.pitch = pitch[i]; J.dst.w = w[i]; J.dst.h = h[i];
        for (int c = 0; c < 4; c++) J.bg[c] = bg[4 * i + c];
        J.glyphs = R; J.bin_first = F; J.bin_glyph = G; J.atlas = atl[i].ptr; J.atlas_w = atlas_w[i];
    }
    const u32 blocks = tx_batch_plan(B);
    for (int i = 0; i < n; i++) wide_out[i] = B.j[i].wide;
    // (one workgroup more than the launch has: it must do nothing)
    for (u32 blk = 0; blk <= blocks; blk++)
        for (u32 tid = 0; tid < SMR_NODE_BLOCK; tid++) tx_workgroup(B, blk, tid, tab);
    for (int i = 0; i < n; i++) {
        const bool empty = w[i] == 0 || h[i] == 0;
        const size_t row = empty ? 0 : (size_t)w[i] * 4;
        for (size_t k = 0; k < bytes[i]; k++) {
            const bool inside = !empty && k >= off[i] && (k - off[i]) % pitch[i] < row;
            if (inside || buf[i].ptr[k] == outside_byte(k, 2000u + (u32)i)) continue;
            fprintf(stderr, "write footprint: job %d (%d x %d, pitch %u, base + %u): byte %zu outside its texels was written: 0x%02x, it held 0x%02x\n", i, w[i], h[i],
                    pitch[i], off[i], k, buf[i].ptr[k], outside_byte(k, 2000u + (u32)i));
            return -77;
        }
        for (int y = 0; !empty && y < h[i]; y++) memcpy(px_out[i] + (size_t)y * row, buf[i].ptr + off[i] + (size_t)y * pitch[i], row);
    }
    return (int)blocks;
}
