// TEST INFRASTRUCTURE — not part of the product; nothing in smelter_amd/ builds, links or loads this.
//
// The user-shader kernel (smelter_amd/csrc/smr_user_shader_prelude.h over smr_shader_dev.h — the two files the library embeds and hands
// the runtime compiler) compiled for the CPU with ONE fixture shader of tests/user_shader_sources.py in the place of the user's source:
// the same three-part sandwich the library builds (host/shader_program.cpp), by #include instead of by string.  tests/test_emu_user_shader.py
// builds one library per fixture (-DSMR_EMU_USER_SOURCE="file") and holds each against the oracle; sources, target and tables sit in
// guard-paged buffers (emu_guard.h), so a sample or store that leaves its surface is a segmentation fault.  Threads of this kernel do not
// talk to each other: every lane of every workgroup runs in turn.
#include <vector>

#include <hip/hip_runtime.h>

thread_local dim3 threadIdx, blockIdx;
dim3 gridDim, blockDim;

#include "emu_device.h"
#include "emu_guard.h"
EmuBlock *emu_blk = nullptr;
thread_local unsigned char *emu_smem = nullptr;
void __syncthreads() {}

#include "smr_internal.h"  // (SMR_TABLE_FLOATS, SMR_LUT16_WORDS for smr_tables.h; includes smr_shader_dev.h)
#include "smr_tables.h"

#include "smr_user_shader_prelude.h"
#include SMR_EMU_USER_SOURCE
#define SMR_USER_SHADER_KERNEL
#include "smr_user_shader_prelude.h"

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

    gridDim = dim3((unsigned)(W + 63) / 64, (unsigned)(H + 3) / 4);
    blockDim = dim3(256);
    for (unsigned by = 0; by < gridDim.y; by++)
        for (unsigned bx = 0; bx < gridDim.x; bx++)
            for (unsigned t = 0; t < 256; t++) {
                blockIdx = dim3(bx, by);
                threadIdx = dim3(t);
                smr_user_shader_kernel(a, (const float *)tables.ptr);
            }
    for (int y = 0; y < H; y++) memcpy(out + (size_t)y * W * 4, a.dst.ptr + (size_t)y * a.dst.pitch, (size_t)W * 4);
    return 0;
}
