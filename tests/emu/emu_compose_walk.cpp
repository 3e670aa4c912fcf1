// TEST INFRASTRUCTURE — not part of the product; nothing in smelter_amd/ builds, links or loads this.
//
// The lane emulator's launch of wave B (emu_compose.cpp: k_classify_tiles + k_compose_output of smelter_amd/csrc/smr_fused_compose.h compiled
// for the CPU) with what that harness leaves out:
//   * a caller-chosen number of COPY WORKGROUPS — the kernel gives workgroup g the run of tiles [g T, min((g + 1) T, tiles)),
//     T = ceil(tiles / workgroups): runs of unequal length, a short last run, runs that cross the end of a tile row, empty workgroups;
//   * the per-wave exchange (emu_device.h's dev_mov_dpp_quad_swap meets at a barrier per wave, which this launch sets up), so the
//     compositor's PAIRED stores run here (SMR_EMU_WAVE_EXCHANGE) — and, on pitches that do not admit them, its per-lane stores;
//   * source textures whose base is not 16-byte aligned (the dword texel loads of a copy tile).
// And the enumeration helpers of the guard-coverage test: inputs on which smr_yuv_fast.h's fast path raises its flag.
// tests/test_emu_compose_walk.py holds every byte to the oracle.
#include <pthread.h>

#include <memory>
#include <thread>
#include <vector>

#include <hip/hip_runtime.h>

thread_local dim3 threadIdx, blockIdx;
dim3 gridDim, blockDim;

#include "emu_device.h"
#include "emu_guard.h"
EmuBlock *emu_blk = nullptr;
thread_local unsigned char *emu_smem = nullptr;
void __syncthreads() { pthread_barrier_wait(&emu_blk->bar); }

#define SMR_EMU_WAVE_EXCHANGE 1
#include "smr_fused_compose.h"
#include "smr_tables.h"

namespace {

// (emu_compose.cpp's launch, plus a barrier per wave for the lane exchanges)
template <typename F>
void run_grid(unsigned blocks, unsigned threads, F kernel) {
    gridDim = dim3(blocks);
    blockDim = dim3(threads);
    auto blk = std::make_unique<EmuBlock>();
    pthread_barrier_t step;
    pthread_barrier_init(&blk->bar, nullptr, threads);
    pthread_barrier_init(&step, nullptr, threads);
    const unsigned waves = (threads + 63) / 64;
    for (unsigned w = 0; w < waves; w++) pthread_barrier_init(&blk->waves[w].bar, nullptr, threads - 64 * w < 64 ? threads - 64 * w : 64);
    emu_blk = blk.get();
    std::vector<std::thread> ts;
    ts.reserve(threads);
    for (unsigned t = 0; t < threads; t++)
        ts.emplace_back([&, t] {
            threadIdx = dim3(t);
            for (unsigned b = 0; b < blocks; b++) {
                blockIdx = dim3(b);
                kernel();
                pthread_barrier_wait(&step);
            }
        });
    for (auto &t : ts) t.join();
    for (unsigned w = 0; w < waves; w++) pthread_barrier_destroy(&blk->waves[w].bar);
    pthread_barrier_destroy(&blk->bar);
    pthread_barrier_destroy(&step);
}

struct Surface {
    GuardBuf buf;
    SurfView view;
};
// as emu_compose.cpp's; `shift`: bytes between the allocation's start and the surface's base (a texture whose base is not 16-byte aligned)
void make_surface(Surface &s, const u8 *tight, int w, int h, int bpp, u32 align, u8 fill, u32 shift = 0) {
    u32 pitch = (u32)(((size_t)w * bpp + 255) & ~(size_t)255);
    if (emu_min_pitch) pitch = (u32)(((size_t)w * bpp + align - 1) & ~(size_t)(align - 1));
    if (emu_min_pitch && !tight) pitch = emu_dst_pitch(pitch);
    s.buf.alloc((size_t)pitch * h + shift, fill, align);
    u8 *base = s.buf.ptr + shift;
    if (!tight) emu_pad_fill(base, pitch, h, 0x0a7 + (u32)bpp * 16 + align);
    if (tight)
        for (int y = 0; y < h; y++) memcpy(base + (size_t)y * pitch, tight + (size_t)y * w * bpp, (size_t)w * bpp);
    s.view.ptr = base; s.view.pitch = pitch; s.view.w = w; s.view.h = h;
}
int check_padding(const Surface &s, int bpp, u32 align, const char *what) {
    return emu_pad_check(s.view.ptr, s.view.pitch, (size_t)s.view.w * bpp, s.view.h, 0x0a7 + (u32)bpp * 16 + align, what);
}
void read_back(const Surface &s, u8 *tight, int bpp) {
    for (int y = 0; y < s.view.h; y++) memcpy(tight + (size_t)y * s.view.w * bpp, s.view.ptr + (size_t)y * s.view.pitch, (size_t)s.view.w * bpp);
}

}  // namespace

// emu_compose's arguments (emu_compose.cpp) with: src_shift[i] = bytes by which source i's base is moved off its 16-byte alignment (a
// multiple of 4), copy_groups = workgroups of the grid's copy part (>= 1).  The band list gets the classifier's own count.
// info[0..6] = tiles per class, info[7] = bands on the list, info[8] = workgroups of the compositor, info[9] = 1 when the output planes admit
// the paired stores (bases and pitches).
extern "C" int emu_compose_walk(const smr_layout *layouts, int n, int n_sources, const u8 *const *src_px, const int *src_w, const int *src_h, const int *src_kind,
                                const int *src_shift, int W, int H, int nv, int srgb, int copy_groups, u8 *out0, u8 *out1, u8 *out2, int *info) {
    if (W < 2 || H < 2 || (W & 1) || (H & 1) || n < 0 || n > MAX_LAYOUT_WORDS * 32 || nv < 0 || nv > 2 || copy_groups < 1) return -1;
    static float tables_src[SMR_TABLE_FLOATS];
    static u32 lut16[SMR_LUT16_WORDS];
    static bool have_tables = false;
    if (!have_tables) {
        if (!smr_build_tables(tables_src, lut16)) return -9;
        have_tables = true;
    }
    GuardBuf tables;
    tables.alloc(sizeof(tables_src), 0, 16);
    memcpy(tables.ptr, tables_src, sizeof(tables_src));

    std::vector<Surface> srcs((size_t)n_sources);
    std::vector<SurfView> views((size_t)n_sources);
    std::vector<int> kinds((size_t)n_sources, 0);
    for (int i = 0; i < n_sources; i++) {
        if (!src_px[i]) continue;
        if (src_shift[i] < 0 || (src_shift[i] & 3)) return -2;
        make_surface(srcs[i], src_px[i], src_w[i], src_h[i], 4, 16, 0x77, (u32)src_shift[i]);
        views[i] = srcs[i].view;
        kinds[i] = src_kind[i];
    }
    size_t total_masks = 0;
    for (int i = 0; i < n; i++) total_masks += layouts[i].masks_len > SMR_MAX_MASKS ? SMR_MAX_MASKS : layouts[i].masks_len;
    GuardBuf dl, dm;
    dl.alloc((size_t)(n ? n : 1) * sizeof(DevLayout), 0, 16);
    dm.alloc((total_masks ? total_masks : 1) * sizeof(DevMask), 0, 16);
    DevLayout *hl = (DevLayout *)dl.ptr;
    DevMask *hm = (DevMask *)dm.ptr;
    u32 mo = 0;
    for (int i = 0; i < n; i++) smr_pack_one_layout(layouts[i], views.data(), kinds.data(), (u32)n_sources, W, H, srgb != 0, tables_src + 256, hl[i], hm, mo);

    const int tiles_x = (W + B_TILE_W - 1) / B_TILE_W, tiles_y = (H + B_TILE_H - 1) / B_TILE_H, tiles = tiles_x * tiles_y;
    GuardBuf tcb, directb, listb;
    tcb.alloc((size_t)tiles * sizeof(TileClass), 0, 16);
    directb.alloc(((size_t)tiles + 15) & ~(size_t)15, 0xff, 16);
    listb.alloc(sizeof(TileList) + (size_t)tiles * B_AREA_BANDS * sizeof(TileFull), 0, 16);
    TileClass *tc = (TileClass *)tcb.ptr;
    TileList *full = (TileList *)listb.ptr;
    run_grid((unsigned)((tiles + B_CLASSIFY_TILES - 1) / B_CLASSIFY_TILES), 64 * B_CLASSIFY_TILES,
             [&] { k_classify_tiles(hl, hm, n, W, H, tiles_x, tiles, 0ull, tc, directb.ptr, full, 1, 0); });
    for (int k = 0; k < 10; k++) info[k] = 0;
    for (int t = 0; t < tiles; t++)
        if (tc[t].kind <= TC_SELECT) info[tc[t].kind]++;
    info[7] = (int)full->count[0];
    u32 n_banded = full->count[0];
    if (n_banded > (u32)tiles * B_AREA_BANDS) n_banded = (u32)tiles * B_AREA_BANDS;

    Surface p0, p1, p2;
    if (nv == 2) {
        make_surface(p0, nullptr, W, H, 4, 16, 0xe1);
        p1.view = p2.view = p0.view;
    } else {
        make_surface(p0, nullptr, W, H, 1, 4, 0xe1);
        if (nv == 1) {
            make_surface(p1, nullptr, W / 2, H / 2, 2, 4, 0xe1);
            p2.view = p1.view;
        } else {
            make_surface(p1, nullptr, W / 2, H / 2, 1, 2, 0xe1);
            make_surface(p2, nullptr, W / 2, H / 2, 1, 2, 0xe1);
        }
    }
    const bool big = n > B_MAX_LAYOUTS || (int)mo > B_MAX_MASKS;
    const unsigned grid = n_banded + (unsigned)copy_groups;
    info[8] = (int)grid;
    info[9] = nv == 0 ? (int)planes_pair_aligned<0>(p0.view, p1.view, p2.view) : nv == 1 ? (int)planes_pair_aligned<1>(p0.view, p1.view, p2.view) : 0;
    const float *tab = (const float *)tables.ptr;
    const int flags = srgb ? 1 : 0;
#define EMU_COMPOSE(NVv, BIGv) \
    run_grid(grid, 256, [&] { k_compose_output<NVv, BIGv>(p0.view, p1.view, p2.view, W, H, hl, hm, n, (int)mo, flags, tab, tiles_x, tiles, tc, full, (int)n_banded, 0); })
    if (nv == 0) { if (big) EMU_COMPOSE(0, true); else EMU_COMPOSE(0, false); }
    else if (nv == 1) { if (big) EMU_COMPOSE(1, true); else EMU_COMPOSE(1, false); }
    else { if (big) EMU_COMPOSE(2, true); else EMU_COMPOSE(2, false); }
#undef EMU_COMPOSE
    if (nv == 2) {
        if (int rc = check_padding(p0, 4, 16, "RGBA8 output")) return rc;
    } else {
        if (int rc = check_padding(p0, 1, 4, "Y plane")) return rc;
        if (nv == 1) {
            if (int rc = check_padding(p1, 2, 4, "UV plane")) return rc;
        } else {
            if (int rc = check_padding(p1, 1, 2, "U plane")) return rc;
            if (int rc = check_padding(p2, 1, 2, "V plane")) return rc;
        }
    }
    if (nv == 2) read_back(p0, out0, 4);
    else {
        read_back(p0, out0, 1);
        if (nv == 1) read_back(p1, out1, 2);
        else { read_back(p1, out1, 1); read_back(p2, out2, 1); }
    }
    return 0;
}

// ---- guard coverage: inputs of the fast path (smr_yuv_fast.h, the header the kernels compile) that raise its flag.
// plane 0: (R, G, B) byte triples — all 2^24, visited in a scrambled order; planes 1 / 2: a 2x2 block's byte sums (0..1020 per channel),
// a scrambled sample of the 1021^3 combinations.  out: three ints per find, at most `max` finds; -> the number found.
extern "C" int emu_yuv_flagged(int plane, int *out, int max) {
    int found = 0;
    if (plane == 0) {
        for (u32 i = 0; i < (1u << 24) && found < max; i++) {
            const u32 v = (i * 2654435761u) & 0xffffffu;  // (an odd multiplier: a permutation of the 2^24 triples)
            const int r = (int)(v & 0xffu), g = (int)((v >> 8) & 0xffu), b = (int)(v >> 16);
            bool f;
            (void)yuvfast::convert<0>((float)r, (float)g, (float)b, &f);
            if (f) { out[3 * found] = r; out[3 * found + 1] = g; out[3 * found + 2] = b; found++; }
        }
        return found;
    }
    uint64_t z = 0x2545f4914f6cdd1dull;
    for (u32 i = 0; i < (1u << 24) && found < max; i++) {
        z ^= z << 13; z ^= z >> 7; z ^= z << 17;  // (xorshift64)
        const int r = (int)(z % 1021u), g = (int)((z >> 20) % 1021u), b = (int)((z >> 40) % 1021u);
        bool f;
        if (plane == 1) (void)yuvfast::convert<1>((float)r, (float)g, (float)b, &f);
        else (void)yuvfast::convert<2>((float)r, (float)g, (float)b, &f);
        if (f) { out[3 * found] = r; out[3 * found + 1] = g; out[3 * found + 2] = b; found++; }
    }
    return found;
}
// Per 4 x 2 block of a tight RGBA8 image (w % 4 == 0, h % 2 == 0): how many of its eight luma values and of its four chroma values (two
// 2x2 blocks x Cb, Cr) the fast path flags.  luma / chroma: (w / 4) * (h / 2) counts, row-major.
extern "C" void emu_yuv_block_flags(const u8 *rgba, int w, int h, int *luma, int *chroma) {
    for (int by = 0; by < h / 2; by++)
        for (int bx = 0; bx < w / 4; bx++) {
            int nl = 0, nc = 0;
            float s[2][3] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};
            for (int y = 0; y < 2; y++)
                for (int x = 0; x < 4; x++) {
                    const u8 *p = rgba + ((size_t)(2 * by + y) * w + 4 * bx + x) * 4;
                    bool f;
                    (void)yuvfast::convert<0>((float)p[0], (float)p[1], (float)p[2], &f);
                    nl += f ? 1 : 0;
                    for (int ch = 0; ch < 3; ch++) s[x >> 1][ch] += (float)p[ch];
                }
            for (int j = 0; j < 2; j++) {
                bool f1, f2;
                (void)yuvfast::convert<1>(s[j][0], s[j][1], s[j][2], &f1);
                (void)yuvfast::convert<2>(s[j][0], s[j][1], s[j][2], &f2);
                nc += (f1 ? 1 : 0) + (f2 ? 1 : 0);
            }
            luma[by * (w / 4) + bx] = nl;
            chroma[by * (w / 4) + bx] = nc;
        }
}
