// TEST INFRASTRUCTURE — not part of the product.  What the stand-alone renderer drivers of tests/san share: CHECK, touch, and the BODIES of
// the stand-ins for the staging entry points the renderer reaches through weak references.  A driver that wants one of those entry points in
// its link defines it itself (extern "C", one line around the body here); a driver that defines none links none, and the renderer takes its
// route without the GPU half.  Define SAN_DRIVER (the program's name, a string literal) before including this.
#pragma once

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "smr.h"

static long g_checks = 0;
#define CHECK(cond)                                                                              \
    do {                                                                                         \
        g_checks++;                                                                              \
        if (!(cond)) { fprintf(stderr, SAN_DRIVER ":%d: %s does not hold\n", __LINE__, #cond); exit(1); } \
    } while (0)

// reads every byte of [p, p + n): one outside the allocation is a report
static volatile uint64_t g_sink;
static inline void touch(const void *p, size_t n) {
    const uint8_t *b = (const uint8_t *)p;
    uint64_t s = 0;
    for (size_t i = 0; i < n; i++) s += b[i];
    g_sink = s;
}

// ---- staging: buffers of exactly the size asked for (a copy, a rasteriser or an upload that overruns one is a report)
static long g_live_staging = 0, g_uploads = 0;
static long g_staging_fail = -1;  // the n-th san_host_alloc from now fails

static inline int san_host_alloc(smr_ctx *ctx, size_t bytes, void **out) {
    if (!ctx || !out || !bytes) return SMR_ERR_INVALID;
    *out = nullptr;
    if (g_staging_fail >= 0 && g_staging_fail-- == 0) return SMR_ERR_OOM;
    *out = malloc(bytes);
    if (!*out) return SMR_ERR_OOM;
    memset(*out, 0xee, bytes);
    g_live_staging++;
    return SMR_OK;
}
static inline void san_host_free(smr_ctx *ctx, void *p) {
    (void)ctx;
    if (!p) return;
    g_live_staging--;
    free(p);
}
// An upload into a frame of `format` (one packed plane): dereferences the frame and reads every byte of the buffer it is handed.  (A driver
// holds its own conditions first.)
static inline int san_frame_upload(smr_ctx *ctx, const smr_frame *f, const void *const host_planes[3], int format) {
    if (!ctx || !f || !host_planes || !host_planes[0]) return SMR_ERR_INVALID;
    smr_surface_info si;
    if ((int)f->format != format || smr_surface_info_get(f->planes[0], &si) != 0 || si.width != f->width || si.height != f->height) return SMR_ERR_INVALID;
    touch(host_planes[0], (size_t)f->width * 4 * f->height);
    g_uploads++;
    return SMR_OK;
}
