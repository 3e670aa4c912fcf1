// TEST INFRASTRUCTURE — not part of the product; nothing in smelter_amd/ builds, links or loads this.
//
// The lane emulator's launch of wave B (emu_compose_walk.cpp: k_classify_tiles + k_compose_output of smelter_amd/csrc/smr_fused_compose.h
// compiled for the CPU, with the per-wave exchange set up so that the paired stores run) for the PACKED 4:2:2 builds of the compositor:
// k_compose_output<3, *> (UYVY) and <4, *> (YUYV), and <2, *> (the RGBA8 node the expected picture is made from) through the same launch.
// The packed plane's pitch is the caller's: a multiple of 8 (what smr_render_layouts lets through to these builds), of 16 for the paired
// stores.  With emu_set_guard(3, ..) the whole plane is filled from a seeded pattern before the launch and every byte outside each row's
// first W * 2 bytes is compared afterwards (emu_guard.h).  And the guard-coverage helper of the pair chroma's fast path.
// tests/test_emu_compose_packed.py holds every byte to the reference sequence.
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

// (emu_compose_walk.cpp's launch: a barrier per wave for the lane exchanges)
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
constexpr u32 PAD_SEED = 0x422u;
// a source: tight rows copied onto a 16-byte aligned pitch | a destination: `pitch` bytes per row (0: the allocator's 256-byte multiple), the
// whole buffer pattern-filled in guard mode 3
void make_surface(Surface &s, const u8 *tight, int w, int h, int bpp, u32 pitch, u8 fill) {
    if (!pitch) pitch = (u32)(((size_t)w * bpp + 255) & ~(size_t)255);
    s.buf.alloc((size_t)pitch * h, fill, 16);
    if (!tight) emu_pad_fill(s.buf.ptr, pitch, h, PAD_SEED);
    if (tight)
        for (int y = 0; y < h; y++) memcpy(s.buf.ptr + (size_t)y * pitch, tight + (size_t)y * w * bpp, (size_t)w * bpp);
    s.view.ptr = s.buf.ptr; s.view.pitch = pitch; s.view.w = w; s.view.h = h;
}

}  // namespace

// emu_compose's arguments (emu_compose.cpp).  nv: 2 -> out = the RGBA8 node (W * 4 bytes per row), 3 / 4 -> out = the UYVY / YUYV plane
// (W * 2 bytes per row: W / 2 texels).  pitch: the destination's (0: a multiple of 256).  copy_groups: workgroups of the grid's copy part
// (0: one per B_COPY_RUN tiles, the product launch).  banded: -1 the classifier's own count, >= 0 that many band workgroups.
// info[0..6] = tiles per class, info[7] = bands on the list, info[8] = workgroups, info[9] = 1 when the plane admits the paired stores.
extern "C" int emu_compose_packed(const smr_layout *layouts, int n, int n_sources, const u8 *const *src_px, const int *src_w, const int *src_h, const int *src_kind,
                                  int W, int H, int nv, int srgb, int banded, int copy_groups, int pitch, u8 *out, int *info) {
    if (W < 2 || H < 2 || (W & 1) || (H & 1) || n < 0 || n > MAX_LAYOUT_WORDS * 32 || nv < 2 || nv > 4 || copy_groups < 0) return -1;
    const int bpp = nv == 2 ? 4 : 2;  // bytes per PIXEL of the destination row
    if (pitch && (pitch < W * bpp || (pitch & (nv == 2 ? 15 : 7)))) return -2;  // (what smr_render_layouts lets through to the fused builds)
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
        make_surface(srcs[i], src_px[i], src_w[i], src_h[i], 4, emu_min_pitch ? (u32)(((size_t)src_w[i] * 4 + 15) & ~(size_t)15) : 0u, 0x77);
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
    u32 n_banded = banded < 0 ? full->count[0] : (u32)banded;
    if (n_banded > (u32)tiles * B_AREA_BANDS) n_banded = (u32)tiles * B_AREA_BANDS;

    // the destination: an RGBA8 surface of W x H, or a plane of W / 2 texels per row
    Surface p;
    make_surface(p, nullptr, nv == 2 ? W : W / 2, H, 4, (u32)pitch, 0xe1);
    const bool big = n > B_MAX_LAYOUTS || (int)mo > B_MAX_MASKS;
    if (!copy_groups) copy_groups = (tiles + B_COPY_RUN - 1) / B_COPY_RUN;
    const unsigned grid = n_banded + (unsigned)copy_groups;
    info[8] = (int)grid;
    info[9] = nv == 2 ? 0 : (int)planes_pair_aligned<3>(p.view, p.view, p.view);
    const float *tab = (const float *)tables.ptr;
    const int flags = srgb ? 1 : 0;
#define EMU_COMPOSE(NVv, BIGv) \
    run_grid(grid, 256, [&] { k_compose_output<NVv, BIGv>(p.view, p.view, p.view, W, H, hl, hm, n, (int)mo, flags, tab, tiles_x, tiles, tc, full, (int)n_banded, 0); })
    if (nv == 2) { if (big) EMU_COMPOSE(2, true); else EMU_COMPOSE(2, false); }
    else if (nv == 3) { if (big) EMU_COMPOSE(3, true); else EMU_COMPOSE(3, false); }
    else { if (big) EMU_COMPOSE(4, true); else EMU_COMPOSE(4, false); }
#undef EMU_COMPOSE
    if (int rc = emu_pad_check(p.view.ptr, p.view.pitch, (size_t)W * bpp, H, PAD_SEED, nv == 2 ? "RGBA8 output" : "packed 4:2:2 plane")) return rc;
    for (int y = 0; y < H; y++) memcpy(out + (size_t)y * W * bpp, p.view.ptr + (size_t)y * p.view.pitch, (size_t)W * bpp);
    return 0;
}

// Per 4 x 2 block of a tight RGBA8 image (w % 4 == 0, h % 2 == 0): how many of its eight chroma values (four pixel pairs x Cb, Cr) the pair
// fast path (yuvfast::convert422, the header the kernels compile) flags.  flags: (w / 4) * (h / 2) counts, row-major.
extern "C" void emu_yuv422_block_flags(const u8 *rgba, int w, int h, int *flags) {
    for (int by = 0; by < h / 2; by++)
        for (int bx = 0; bx < w / 4; bx++) {
            int nc = 0;
            for (int y = 0; y < 2; y++)
                for (int j = 0; j < 2; j++) {
                    const u8 *a = rgba + ((size_t)(2 * by + y) * w + 4 * bx + 2 * j) * 4, *b = a + 4;
                    bool f1, f2;
                    (void)yuvfast::convert422<1>((float)a[0] + (float)b[0], (float)a[1] + (float)b[1], (float)a[2] + (float)b[2], &f1);
                    (void)yuvfast::convert422<2>((float)a[0] + (float)b[0], (float)a[1] + (float)b[1], (float)a[2] + (float)b[2], &f2);
                    nc += (f1 ? 1 : 0) + (f2 ? 1 : 0);
                }
            flags[by * (w / 4) + bx] = nc;
        }
}
