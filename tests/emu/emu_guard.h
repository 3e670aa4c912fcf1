// TEST INFRASTRUCTURE — not part of the product.  Buffers for the emulated kernels' "device memory" with the page after (or before)
// them unmapped: a load or store that leaves the allocation is a segmentation fault instead of a silent read of slack.  What the
// library promises about memory it does not own (include/smr.h, smr_surface_wrap): an allocation covers pitch * h bytes and no kernel
// reads past a row's pitch — with a plane of exactly pitch * h bytes ending at the guard page, the last row's last block proves it.
//   emu_set_guard(mode, min_pitch)   mode 0: heap buffers with slack (the default)   1: the buffer ENDS at a guard page   2: it STARTS behind one
//                                         3: WRITE FOOTPRINT — buffers as in mode 2, and every destination the emulated kernels write (node
//                                            textures, tiles, output planes) on the smallest admitted pitch + 32 (emu_dst_pitch), the whole
//                                            buffer pre-filled from a seeded pattern (emu_pad_fill) and its row padding compared after the
//                                            launch (emu_pad_check): what include/smr.h promises about the bytes the library WRITES of a
//                                            surface it does not own — the w x h texels and no other byte.  Modes 1 / 2 use the smallest
//                                            pitch, where a store that spills past a row's last texel lands in the next row and is
//                                            overwritten; here it lands in padding that is looked at.
//                                    min_pitch != 0: the smallest pitch the host code lets through instead of the allocator's 256-byte pitch
#pragma once
#include <sys/mman.h>
#include <unistd.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

static int emu_guard_mode = 0, emu_min_pitch = 0;
extern "C" void emu_set_guard(int mode, int min_pitch) { emu_guard_mode = mode; emu_min_pitch = min_pitch; }

// mode 3: a destination's pitch (32 more than the smallest admitted: alignment is kept, 32 bytes hold any group store of the kernels) and
// its seeded pattern.  The pattern depends on the offset only, so the check needs no copy of the buffer.
inline uint32_t emu_dst_pitch(uint32_t min_pitch) { return emu_guard_mode == 3 ? min_pitch + 32u : min_pitch; }
inline unsigned char emu_pad_byte(size_t off, uint32_t seed) {
    uint64_t z = (uint64_t)off * 0x9e3779b97f4a7c15ull + (uint64_t)seed * 0xbf58476d1ce4e5b9ull + 0x94d049bb133111ebull;  // (splitmix64's mixer)
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return (unsigned char)((z ^ (z >> 31)) >> 24);
}
inline void emu_pad_fill(unsigned char *ptr, size_t pitch, int h, uint32_t seed) {
    if (emu_guard_mode != 3) return;
    for (size_t i = 0; i < pitch * (size_t)h; i++) ptr[i] = emu_pad_byte(i, seed);
}
// 0, or -77 after naming the first byte outside the h rows' first row_bytes bytes that differs from the pattern
inline int emu_pad_check(const unsigned char *ptr, size_t pitch, size_t row_bytes, int h, uint32_t seed, const char *what) {
    if (emu_guard_mode != 3) return 0;
    for (int y = 0; y < h; y++)
        for (size_t x = row_bytes; x < pitch; x++) {
            const size_t off = (size_t)y * pitch + x;
            if (ptr[off] != emu_pad_byte(off, seed)) {
                fprintf(stderr, "write footprint: %s: row %d, byte %zu of the row (row bytes %zu, pitch %zu) was written: 0x%02x, the pattern has 0x%02x\n", what, y, x,
                        row_bytes, pitch, ptr[off], emu_pad_byte(off, seed));
                return -77;
            }
        }
    return 0;
}

struct GuardBuf {
    unsigned char *map = nullptr, *ptr = nullptr;
    size_t map_len = 0, size = 0;
    GuardBuf() = default;
    GuardBuf(const GuardBuf &) = delete;
    GuardBuf &operator=(const GuardBuf &) = delete;
    GuardBuf(GuardBuf &&o) noexcept { *this = static_cast<GuardBuf &&>(o); }
    GuardBuf &operator=(GuardBuf &&o) noexcept {
        release();
        map = o.map; ptr = o.ptr; map_len = o.map_len; size = o.size;
        o.map = o.ptr = nullptr; o.map_len = o.size = 0;
        return *this;
    }
    ~GuardBuf() { release(); }
    void release() {
        if (map) munmap(map, map_len);
        else free(ptr);
        map = ptr = nullptr;
    }
    // `bytes` usable bytes filled with `fill`, the start aligned to `align` (a power of two <= 256)
    void alloc(size_t bytes, unsigned char fill, size_t align = 16) {
        release();
        size = bytes;
        if (!emu_guard_mode) {
#ifdef SMR_EMU_ASAN  // (an instrumented build: the exact size, AddressSanitizer's red zones around it)
            if (posix_memalign((void **)&ptr, 256, bytes ? bytes : 1)) abort();
            memset(ptr, fill, bytes);
#else
            if (posix_memalign((void **)&ptr, 256, bytes + 64)) abort();  // (slack: the pre-guard behaviour)
            memset(ptr, fill, bytes + 64);
#endif
            return;
        }
        const size_t page = (size_t)sysconf(_SC_PAGESIZE);
        const size_t body = (bytes + align - 1 + page - 1) / page * page;
        map_len = body + 2 * page;
        map = (unsigned char *)mmap(nullptr, map_len, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
        if (map == MAP_FAILED) abort();
        memset(map, fill, map_len);
        if (emu_guard_mode == 1) ptr = map + page + ((body - bytes) & ~(align - 1));  // the end on (or within `align` of) the guard page
        else ptr = map + page;
        // (mode 1: callers pass sizes that are multiples of `align` — pitch * h — so that the last byte is the page's last)
        mprotect(map, page, PROT_NONE);
        mprotect(map + page + body, page, PROT_NONE);
    }
};
