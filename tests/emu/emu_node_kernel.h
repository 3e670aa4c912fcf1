// TEST INFRASTRUCTURE — not part of the product; nothing in smelter_amd/ builds, links or loads this.
//
// What the drivers of the three batched node kernels (emu_image_nodes.cpp, emu_svg_nodes.cpp, emu_web_view.cpp) have in common, before
// their own job set-up: the shims a kernel header needs to compile for the CPU (the same as emu_move.cpp's; these kernels have no LDS and no
// barrier: threads do not talk to each other, and a driver runs them one after the other), the sRGB table block, and the alignment rule of
// the guard modes.  One translation unit per driver: include this once, then the kernel's header.
#pragma once

#include <vector>

#include <hip/hip_runtime.h>

thread_local dim3 threadIdx, blockIdx;
dim3 gridDim, blockDim;

#include "emu_device.h"
#include "emu_guard.h"
EmuBlock *emu_blk = nullptr;
thread_local unsigned char *emu_smem = nullptr;
void __syncthreads() {}

#include "smr_internal.h"
#include "smr_tables.h"
#include "smr_node_tiles.h"

// The table block every context builds once, copied behind a guard page for this call: ptr is null if it could not be built.
struct EmuTables {
    GuardBuf buf;
    const float *ptr = nullptr;
    EmuTables() {
        static float tables_src[SMR_TABLE_FLOATS];
        static u32 lut16[SMR_LUT16_WORDS];
        static bool have_tables = false;
        if (!have_tables) {
            if (!smr_build_tables(tables_src, lut16)) return;
            have_tables = true;
        }
        buf.alloc(sizeof(tables_src), 0, 16);
        memcpy(buf.ptr, tables_src, sizeof(tables_src));
        ptr = (const float *)buf.ptr;
    }
};

// (guard mode 1 puts a buffer's END on the guard page: its start then has the alignment of its size, 4 at least)
static inline size_t emu_surface_align() { return emu_guard_mode == 1 ? 4 : 16; }
