// TEST INFRASTRUCTURE — not part of the product; nothing in smelter_amd/ builds, links or loads this.
//
// k_svg_nodes' source (smelter_amd/csrc/smr_svg_nodes.h: sv_plan on the host, sv_workgroup per thread) compiled for the CPU, so that
// tests/test_emu_svg_nodes.py can run one launch — every workgroup, every thread, in turn: threads do not talk to each other — on buffers
// that are exactly as large as the surfaces they hold (emu_guard.h: the byte after, or before, them is an unmapped page).  Shims, tables and the
// alignment rule: emu_node_kernel.h.  The work is in place, so the store mask is held here: every byte of a buffer outside the job's texels — the bytes
// before its base, its row padding — is compared with what it held before the launch (a seeded pattern in guard mode 3, as emu_pad_fill
// makes it; a sentinel otherwise).
#include "emu_node_kernel.h"
#include "smr_svg_nodes.h"

static inline u8 outside_byte(size_t off, u32 seed) { return emu_guard_mode == 3 ? emu_pad_byte(off, seed) : (u8)0xc3; }

// Job i: the tight w[i] x h[i] RGBA8 texels px_in[i], in a buffer of exactly off[i] + pitch[i] * (h[i] - 1) + w[i] * 4 bytes (0 texels:
// off[i] bytes) whose rows are pitch[i] bytes apart and start off[i] bytes in.  After the launch the texels come back tight in px_out[i];
// wide_out[i]: 1 = whole groups went as 16-byte accesses.  Returns the number of workgroups the launch has, -77 after naming a byte outside
// a job's texels that changed, or another value < 0.
extern "C" int emu_svg_nodes(int n, const u8 *const *px_in, const int *w, const int *h, const u32 *pitch, const u32 *off, u8 *const *px_out, u32 *wide_out) {
    if (n < 0 || n > SMR_NODE_MAX_JOBS) return -1;
    const EmuTables tables;
    if (!tables.ptr) return -9;
    const float *tab = tables.ptr;
    const size_t align = emu_surface_align();

    std::vector<GuardBuf> buf((size_t)n);
    std::vector<size_t> bytes((size_t)n);
    SvgBatch B;
    memset(&B, 0, sizeof(B));
    B.n = (u32)n;
    for (int i = 0; i < n; i++) {
        if (w[i] < 0 || h[i] < 0) return -1;
        const bool empty = w[i] == 0 || h[i] == 0;
        if (!empty && (pitch[i] < (u32)w[i] * 4 || (pitch[i] & 3u) || (off[i] & 3u))) return -1;
        bytes[i] = off[i] + (empty ? 0 : (size_t)pitch[i] * (h[i] - 1) + (size_t)w[i] * 4);
        buf[i].alloc(bytes[i] ? bytes[i] : 4, 0, align);
        for (size_t k = 0; k < bytes[i]; k++) buf[i].ptr[k] = outside_byte(k, 1000u + (u32)i);
        for (int y = 0; !empty && y < h[i]; y++) memcpy(buf[i].ptr + off[i] + (size_t)y * pitch[i], px_in[i] + (size_t)y * w[i] * 4, (size_t)w[i] * 4);
        SvgJob &J = B.j[i];
        J.px.ptr = buf[i].ptr + off[i]; J.px.pitch = pitch[i]; J.px.w = w[i]; J.px.h = h[i];
    }
    const u32 blocks = sv_plan(B);
    for (int i = 0; i < n; i++) wide_out[i] = B.j[i].wide;
    // (one workgroup more than the launch has: it must do nothing)
    for (u32 blk = 0; blk <= blocks; blk++)
        for (u32 tid = 0; tid < SMR_NODE_BLOCK; tid++) sv_workgroup(B, blk, tid, tab);
    for (int i = 0; i < n; i++) {
        const bool empty = w[i] == 0 || h[i] == 0;
        const size_t row = empty ? 0 : (size_t)w[i] * 4;
        for (size_t k = 0; k < bytes[i]; k++) {
            const bool inside = !empty && k >= off[i] && (k - off[i]) % pitch[i] < row;
            if (inside || buf[i].ptr[k] == outside_byte(k, 1000u + (u32)i)) continue;
            fprintf(stderr, "write footprint: job %d (%d x %d, pitch %u, base + %u): byte %zu outside its texels was written: 0x%02x, it held 0x%02x\n", i, w[i], h[i],
                    pitch[i], off[i], k, buf[i].ptr[k], outside_byte(k, 1000u + (u32)i));
            return -77;
        }
        for (int y = 0; !empty && y < h[i]; y++) memcpy(px_out[i] + (size_t)y * row, buf[i].ptr + off[i] + (size_t)y * pitch[i], row);
    }
    return (int)blocks;
}
