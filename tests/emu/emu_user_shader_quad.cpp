// TEST INFRASTRUCTURE — not part of the product; nothing in smelter_amd/ builds, links or loads this.
//
// The user-shader kernel in QUAD mode (SMR_DERIVATIVES: smelter_amd/csrc/smr_user_shader_prelude.h) compiled for the CPU with one fixture
// shader of tests/user_shader_sources_derivatives.py in the place of the user's source.  Four consecutive lanes are one 2 x 2 pixel quad
// and exchange registers (v_mov_b32_dpp quad_perm on the device), so a workgroup here is 256 host threads, one per lane — the run_grid
// pattern of emu_user_shader_clip.cpp, with its real __syncthreads for the clip stage's table — and a quad exchange meets at a barrier of
// its own quad: four threads, 64 quads per workgroup.  (A per-wave barrier would deadlock: a quad none of whose pixels a plane covers
// skips the fragment and never arrives.)  The exported emu_user_shader has the signature of emu_user_shader.cpp's and the same guard-paged
// buffers (emu_guard.h), so tests/test_emu_user_shader_affine.py's run() drives it.
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

// v_mov_b32_dpp quad_perm:[c & 3, (c >> 2) & 3, (c >> 4) & 3, c >> 6]: lane k of a quad reads lane (c >> 2 k) & 3 of the same quad.  Every
// lane of the quad must call it (a derivative in control flow that is not uniform across the quad is unspecified; here it would wait).
namespace {
struct EmuQuads {
    pthread_barrier_t bar[64];
    int xchg[256];
};
EmuQuads *emu_quads = nullptr;
}  // namespace
static inline int dev_mov_dpp_quad_perm(int x, int ctrl) {
    const int tid = (int)threadIdx.x;
    pthread_barrier_t *bar = &emu_quads->bar[tid >> 2];
    emu_quads->xchg[tid] = x;
    pthread_barrier_wait(bar);
    const int r = emu_quads->xchg[(tid & ~3) + ((ctrl >> (2 * (tid & 3))) & 3)];
    pthread_barrier_wait(bar);
    return r;
}

// (what the shim does not carry: the vertex stage's `position` argument)
struct float3 { float x, y, z; };
static inline float3 make_float3(float x, float y, float z) { return {x, y, z}; }

#include "smr_internal.h"  // (SMR_TABLE_FLOATS, SMR_LUT16_WORDS for smr_tables.h; includes smr_shader_dev.h)
#include "smr_tables.h"

#include "smr_user_shader_prelude.h"
#include SMR_EMU_USER_SOURCE
#define SMR_USER_SHADER_KERNEL
#include "smr_user_shader_prelude.h"

namespace {

// A launch: `threads` host threads — one per lane — live for the whole grid and run its workgroups one after the other (a barrier between
// two workgroups: the LDS statics, the EmuBlock and the quad slots are the workgroup's).
template <typename F>
void run_grid(dim3 grid, unsigned threads, F kernel) {
    gridDim = grid;
    blockDim = dim3(threads);
    auto blk = std::make_unique<EmuBlock>();
    auto quads = std::make_unique<EmuQuads>();
    pthread_barrier_t step;
    pthread_barrier_init(&blk->bar, nullptr, threads);
    pthread_barrier_init(&step, nullptr, threads);
    for (auto &b : quads->bar) pthread_barrier_init(&b, nullptr, 4);
    emu_blk = blk.get();
    emu_quads = quads.get();
    std::vector<std::thread> ts;
    ts.reserve(threads);
    for (unsigned t = 0; t < threads; t++)
        ts.emplace_back([&, t] {
            threadIdx = dim3(t);
            for (unsigned by = 0; by < grid.y; by++)
                for (unsigned bx = 0; bx < grid.x; bx++) {
                    blockIdx = dim3(bx, by);
                    kernel();
                    pthread_barrier_wait(&step);
                }
        });
    for (auto &t : ts) t.join();
    pthread_barrier_destroy(&blk->bar);
    pthread_barrier_destroy(&step);
    for (auto &b : quads->bar) pthread_barrier_destroy(&b);
    emu_blk = nullptr;
    emu_quads = nullptr;
}

}  // namespace

// sources: n_src premultiplied RGBA8 textures, tight rows (src_px[i] == NULL: absent).  out: W x H x 4, tight; the target starts as 0x4d
// throughout (stale contents must not show through the clear).  Returns 0, or -9 if the table block cannot be built.
extern "C" int emu_user_shader(int n_src, const u8 *const *src_px, const int *src_w, const int *src_h, int W, int H, int srgb, float time_s,
                               const u8 *params, u32 params_size, u8 *out) {
    if (n_src < 0 || n_src > SMR_USER_SHADER_SOURCES || params_size > SMR_USER_SHADER_PARAM_BYTES || W <= 0 || H <= 0) return -1;
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

    UserShaderArgs a;
    memset(&a, 0, sizeof(a));
    std::vector<GuardBuf> bufs((size_t)n_src + 1);
    auto surface = [&](GuardBuf &b, const u8 *tight, int w, int h, u8 fill) {
        u32 pitch = (u32)(((size_t)w * 4 + 255) & ~(size_t)255);
        if (emu_min_pitch) pitch = (u32)w * 4;
        b.alloc((size_t)pitch * h, fill, 4);
        if (tight)
            for (int y = 0; y < h; y++) memcpy(b.ptr + (size_t)y * pitch, tight + (size_t)y * w * 4, (size_t)w * 4);
        SurfView v;
        v.ptr = b.ptr; v.pitch = pitch; v.w = w; v.h = h;
        return v;
    };
    a.dst = surface(bufs[(size_t)n_src], nullptr, W, H, 0x4d);
    for (int i = 0; i < n_src; i++)
        if (src_px[i]) a.src[i] = surface(bufs[(size_t)i], src_px[i], src_w[i], src_h[i], 0);
    a.n_src = n_src;
    a.pxi = srgb ? PXI_RGBA8_SRGB : PXI_RGBA8_UNORM;
    a.time = time_s;
    a.param_size = params_size;
    if (params_size) memcpy(a.params, params, params_size);

    const float *tab = (const float *)tables.ptr;
    run_grid(dim3((unsigned)(W + 63) / 64, (unsigned)(H + 3) / 4), 256, [&] { smr_user_shader_kernel(a, tab); });
    for (int y = 0; y < H; y++) memcpy(out + (size_t)y * W * 4, a.dst.ptr + (size_t)y * a.dst.pitch, (size_t)W * 4);
    return 0;
}
