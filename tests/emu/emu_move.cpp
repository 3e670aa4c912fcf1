// TEST INFRASTRUCTURE — not part of the product; nothing in smelter_amd/ builds, links or loads this.
//
// k_move_rects' source (smelter_amd/csrc/smr_move_rects.h: mv_plan on the host, mv_workgroup per thread) compiled for the CPU, so that
// tests/test_emu_move.py can run one launch — every workgroup, every thread, in turn: threads do not talk to each other — on buffers that
// are exactly as large as the rectangles they hold (emu_guard.h: the byte after, or before, them is an unmapped page; red zones in the
// instrumented build).  Same shims as emu_convert.cpp.
#include <vector>

#include <hip/hip_runtime.h>

thread_local dim3 threadIdx, blockIdx;
dim3 gridDim, blockDim;

#include "emu_device.h"
#include "emu_guard.h"
EmuBlock *emu_blk = nullptr;
thread_local unsigned char *emu_smem = nullptr;
void __syncthreads() {}

#include "smr_move_rects.h"

// Rectangle i: `rows[i]` rows of `row_bytes[i]` bytes (data[i]: tight rows), the source rows src_pitch[i] apart starting src_off[i] bytes into a
// buffer whose start is aligned to src_align[i]; likewise the destination.  Either buffer holds off + pitch * (rows - 1) + row_bytes bytes and
// not one more.  Source padding is 0x5a, the destination starts as 0xc3 throughout and comes back whole in dst_out[i] (off + extent bytes).
// fast_out[i]: 1 = the 16-byte path, 0 = the byte path, rows that share their phase, 2 = the byte path, rows that do not (by the first row).
// Returns the number of workgroups the launch has, or -1.
extern "C" int emu_move_rects(int n, const u8 *const *data, const u32 *row_bytes, const u32 *rows, const u32 *src_pitch, const u32 *dst_pitch,
                              const u32 *src_off, const u32 *dst_off, const u32 *src_align, const u32 *dst_align, u8 *const *dst_out, u32 *fast_out) {
    if (n < 0 || n > SMR_MOVE_MAX_RECTS) return -1;
    std::vector<GuardBuf> src(n), dst(n);
    std::vector<size_t> dst_bytes(n);
    MoveBatch B;
    memset(&B, 0, sizeof(B));
    B.n = (u32)n;
    for (int i = 0; i < n; i++) {
        if (rows[i] && (src_pitch[i] < row_bytes[i] || dst_pitch[i] < row_bytes[i])) return -1;
        const size_t se = rows[i] ? (size_t)src_pitch[i] * (rows[i] - 1) + row_bytes[i] : 0, de = rows[i] ? (size_t)dst_pitch[i] * (rows[i] - 1) + row_bytes[i] : 0;
        src[i].alloc(src_off[i] + se, 0x5a, src_align[i]);
        dst[i].alloc(dst_off[i] + de, 0xc3, dst_align[i]);
        dst_bytes[i] = dst_off[i] + de;
        for (u32 y = 0; y < rows[i]; y++) memcpy(src[i].ptr + src_off[i] + (size_t)y * src_pitch[i], data[i] + (size_t)y * row_bytes[i], row_bytes[i]);
        MoveRect &R = B.r[i];
        R.src = src[i].ptr + src_off[i]; R.dst = dst[i].ptr + dst_off[i];
        R.src_pitch = src_pitch[i]; R.dst_pitch = dst_pitch[i]; R.row_bytes = row_bytes[i]; R.rows = rows[i];
    }
    const u32 blocks = mv_plan(B);
    for (int i = 0; i < n; i++) fast_out[i] = B.fast[i] ? 1u : ((((uintptr_t)B.r[i].src ^ (uintptr_t)B.r[i].dst) & 15u) ? 2u : 0u);
    // (one workgroup more than the launch has: it must do nothing)
    for (u32 blk = 0; blk <= blocks; blk++)
        for (u32 tid = 0; tid < SMR_MOVE_BLOCK; tid++) mv_workgroup(B, blk, tid);
    for (int i = 0; i < n; i++)
        if (dst_bytes[i]) memcpy(dst_out[i], dst[i].ptr, dst_bytes[i]);
    return (int)blocks;
}
