// TEST INFRASTRUCTURE — not part of the product.  SVG image assets through the renderer (smelter_amd/csrc/host/renderer.cpp:
// smr_renderer_register_svg_image / _unregister_image / _svg_stats, the rasteriser's calls inside smr_renderer_update_scene, the raster
// cache, the node's place in the image pass) with the scene engine, compiled by g++ under AddressSanitizer + UBSan and linked against
// tests/san/null_device.cpp instead of the GPU half of the library.  The entry points the renderer reaches through weak references for this
// feature are defined HERE, as stand-ins of the null device's kind: staging buffers of exactly the size asked for (a rasteriser or an upload
// that overruns one is a report), an upload that reads every byte of the buffer it is handed and dereferences the frame, and an
// smr_svg_nodes that checks every surface it is given.
// A fixed sequence: register / update / unregister churn, a callback that fails on its k-th call for every k, the same asset at 40 sizes
// over 40 updates, unregister refused while in use, the renderer destroyed with rasters resident, then the same with every device
// allocation (and every staging allocation) failing in turn.
//   svg_driver            (prints one JSON line; exit status 0 = everything held)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#define SAN_DRIVER "svg_driver"
#include "san_driver.h"

extern "C" long null_device_live_surfaces();
extern "C" void null_device_fail_after(long n);

// ---- the stand-ins (staging and upload: san_driver.h)
static long g_fix_calls = 0, g_fixed = 0;

extern "C" {
int smr_host_alloc(smr_ctx *ctx, size_t bytes, void **out) { return san_host_alloc(ctx, bytes, out); }
void smr_host_free(smr_ctx *ctx, void *p) { san_host_free(ctx, p); }
int smr_frame_upload_async(smr_ctx *ctx, const smr_frame *f, const void *const host_planes[3]) {
    smr_surface_info si;
    if (!f || smr_surface_info_get(f->planes[0], &si) != 0 || si.format != SMR_PX_RGBA8) return SMR_ERR_INVALID;
    return san_frame_upload(ctx, f, host_planes, SMR_FRAME_RGBA);
}
int smr_svg_nodes(smr_ctx *ctx, smr_surface *const *surfaces, uint32_t n) {
    if (!ctx || (n && !surfaces)) return SMR_ERR_INVALID;
    if (smr_ctx_mode(ctx) != SMR_MODE_GPU_OPTIMIZED) return SMR_ERR_INVALID;
    for (uint32_t i = 0; i < n; i++) {
        smr_surface_info si;
        if (smr_surface_info_get(surfaces[i], &si) != 0 || si.format != SMR_PX_RGBA8) return SMR_ERR_INVALID;
        for (uint32_t k = 0; k < i; k++)
            if (surfaces[k] == surfaces[i]) return SMR_ERR_INVALID;
    }
    g_fix_calls++;
    g_fixed += n;
    return SMR_OK;
}
}

// ---- the host's "rasteriser": fills exactly the w x h texels it was asked for, and checks what the library promises about the buffer
struct Raster {
    long calls = 0, fail_at = -1;  // fail_at >= 0: the call with that index (from the last reset) returns 1
    std::vector<std::pair<uint32_t, uint32_t>> sizes;
    uint8_t alpha = 200;
};
static int rasterise(void *user, const char *image_id, uint32_t w, uint32_t h, uint8_t *rgba, size_t pitch) {
    Raster *R = (Raster *)user;
    CHECK(R && image_id && rgba && w && h && pitch == (size_t)w * 4);
    CHECK(strncmp(image_id, "logo", 4) == 0);
    for (size_t i = 0; i < pitch * h; i++)
        if (rgba[i] != 0) { fprintf(stderr, "svg_driver: the pixmap was not zero-filled\n"); exit(1); }
    g_checks++;
    R->sizes.push_back({w, h});
    const long k = R->calls++;
    for (uint32_t y = 0; y < h; y++)
        for (uint32_t x = 0; x < w; x++) {
            uint8_t *p = rgba + pitch * y + 4 * (size_t)x;
            p[0] = p[1] = p[2] = (uint8_t)((x + y) % (R->alpha + 1u));
            p[3] = R->alpha;
        }
    return k == R->fail_at ? 1 : 0;
}

static bool has(const smr_renderer *r, const char *text) { return strstr(smr_renderer_last_error(r), text) != nullptr; }
static void stats(const smr_renderer *r, uint64_t *calls, uint64_t *launches, uint32_t *resident) { CHECK(smr_renderer_svg_stats(r, calls, launches, resident) == 0); }
static uint32_t resident(const smr_renderer *r) {
    uint32_t n = 0;
    stats(r, nullptr, nullptr, &n);
    return n;
}

static std::string scene_of(const std::vector<std::pair<int, int>> &sizes, const char *image = "logo") {
    std::string s = R"({"type":"view","children":[)";
    for (size_t i = 0; i < sizes.size(); i++) {
        if (i) s += ",";
        s += std::string(R"({"type":"image","image_id":")") + image + "\"";
        if (sizes[i].first >= 0) s += ",\"width\":" + std::to_string(sizes[i].first);
        if (sizes[i].second >= 0) s += ",\"height\":" + std::to_string(sizes[i].second);
        s += "}";
    }
    return s + "]}";
}
static const char *SCENE_PLAIN = R"({"type":"view","children":[{"type":"image","image_id":"bitmap","width":9,"height":7}]})";
static const char *SCENE_EMPTY = R"({"type":"view"})";

static long g_refused_calls = 0, g_size_updates = 0;

// one renderer's life; `fail_at` >= 0: the fail_at-th device allocation from the first scene on fails, `staging_fail_at` likewise for staging
static void life(uint32_t mode, long fail_at, long staging_fail_at, long *refused) {
    smr_ctx *ctx[2];
    for (auto &c : ctx) CHECK(smr_ctx_create(0, mode, 100, nullptr, &c) == 0);
    smr_renderer *r = nullptr;
    CHECK(smr_renderer_create(ctx[0], -1, &r) == 0);
    const bool strict = fail_at < 0 && staging_fail_at < 0, gpu_mode = mode == SMR_MODE_GPU_OPTIMIZED;
    Raster R, R2;
    R2.alpha = 255;
    std::vector<uint8_t> px(12 * 10 * 4, 9);
    // registration: what smr_renderer_register_image refuses, and a null fn
    CHECK(smr_renderer_register_svg_image(nullptr, "logo", 64, 64, rasterise, &R) == SMR_ERR_INVALID);
    CHECK(smr_renderer_register_svg_image(r, nullptr, 64, 64, rasterise, &R) == SMR_ERR_INVALID && has(r, "null argument"));
    CHECK(smr_renderer_register_svg_image(r, "logo", 0, 64, rasterise, &R) == SMR_ERR_INVALID);
    CHECK(smr_renderer_register_svg_image(r, "logo", 64, 0, rasterise, &R) == SMR_ERR_INVALID);
    CHECK(smr_renderer_register_svg_image(r, "logo", 64, 64, nullptr, &R) == SMR_ERR_INVALID);
    CHECK(smr_renderer_register_image(r, "bitmap", px.data(), 12, 10) == 0);
    CHECK(smr_renderer_register_svg_image(r, "bitmap", 64, 64, rasterise, &R) == SMR_ERR_INVALID && has(r, "already registered"));
    CHECK(smr_renderer_register_svg_image(r, "logo", 64, 32, rasterise, &R) == 0);
    CHECK(smr_renderer_register_svg_image(r, "logo", 64, 32, rasterise, &R) == SMR_ERR_INVALID && has(r, "already registered"));
    CHECK(smr_renderer_register_image(r, "logo", px.data(), 12, 10) == SMR_ERR_INVALID && has(r, "already registered"));
    CHECK(smr_renderer_register_svg_image(r, "logo2", 10, 10, rasterise, &R2) == 0);
    CHECK(R.calls == 0 && R2.calls == 0 && g_live_staging == 0 && resident(r) == 0);  // nothing is rasterised at registration
    CHECK(smr_renderer_svg_stats(nullptr, nullptr, nullptr, nullptr) == SMR_ERR_INVALID && smr_renderer_svg_stats(r, nullptr, nullptr, nullptr) == 0);
    CHECK(smr_renderer_unregister_image(nullptr, "logo") == SMR_ERR_INVALID && smr_renderer_unregister_image(r, nullptr) == SMR_ERR_INVALID);
    CHECK(smr_renderer_unregister_image(r, "nobody") == 0);
    CHECK(smr_renderer_add_lane(r, ctx[1]) == 0);
    auto answer = [&](int rc) {
        if (strict) CHECK(rc == 0);
        else if (rc < 0) { CHECK(rc == SMR_ERR_OOM); (*refused)++; }
        return rc;
    };
    int64_t pts = 0;
    auto render = [&]() {
        smr_output_frame out[4];
        uint32_t n = 0;
        const int rc = smr_renderer_render(r, pts, nullptr, 0, out, 4, &n);
        pts += 40000000;
        return rc;
    };
    if (fail_at >= 0) null_device_fail_after(fail_at);
    g_staging_fail = staging_fail_at;

    // the first scene: the asset at its own size, at (w, -), at a size twice, and a node without texels — three rasters, one launch
    const long fix0 = g_fix_calls;
    int rc = answer(smr_renderer_update_scene(r, "o", 64, 36, SMR_FRAME_PLANAR_YUV420, scene_of({{-1, -1}, {20, -1}, {33, 17}, {33, 17}, {0, 5}}).c_str()));
    CHECK(g_live_staging == 0);  // (staging goes once the update is over, however it ended)
    if (rc == 0) {
        CHECK(R.calls == 3 && resident(r) == 3);
        CHECK(R.sizes[0] == std::make_pair(64u, 32u) && R.sizes[1] == std::make_pair(20u, 10u) && R.sizes[2] == std::make_pair(33u, 17u));
        CHECK(g_fix_calls - fix0 == (gpu_mode ? 1 : 0));
        uint64_t calls = 0, launches = 0;
        stats(r, &calls, &launches, nullptr);
        CHECK(calls == 3 && launches == (gpu_mode ? 1u : 0u));
        CHECK(smr_renderer_unregister_image(r, "logo") == SMR_ERR_INVALID && has(r, "a scene uses"));
    } else if (smr_renderer_node_count(r, "o") == -1) {
        CHECK(resident(r) == 0);  // a refused first update leaves nothing behind
    } else {
        CHECK(resident(r) == 3);  // (the output's own frames could not be made: reported with the new scene in place, include/smr.h)
    }
    for (int k = 0; k < 3; k++) answer(render());
    uint64_t image_launches = 7;
    CHECK(smr_renderer_image_launches(r, &image_launches) == 0 && image_launches == 0);  // SVG nodes never go through the image pass
    // the same scene again: nothing to rasterise
    {
        const long before = R.calls;
        const uint32_t had = resident(r);
        rc = answer(smr_renderer_update_scene(r, "o", 64, 36, SMR_FRAME_PLANAR_YUV420, scene_of({{-1, -1}, {20, -1}, {33, 17}, {33, 17}, {0, 5}}).c_str()));
        if (rc == 0 && had == 3) CHECK(R.calls == before && resident(r) == 3);
    }
    // a second output shares the rasters; dropping nodes releases what nobody shows
    {
        const long before = R.calls;
        rc = answer(smr_renderer_update_scene(r, "p", 32, 32, SMR_FRAME_RGBA, scene_of({{33, 17}}).c_str()));
        if (strict) CHECK(R.calls == before && resident(r) == 3);
        rc = answer(smr_renderer_update_scene(r, "o", 64, 36, SMR_FRAME_PLANAR_YUV420, scene_of({{20, -1}}).c_str()));
        if (strict) CHECK(R.calls == before && resident(r) == 2);  // 20 x 10 for "o", 33 x 17 for "p"
        answer(render());
        CHECK(smr_renderer_unregister_output(r, "p") == 0);
        if (strict) CHECK(resident(r) == 1);
    }
    if (strict) {
        // a callback that fails on its k-th call, for every k: the previous scene stays, nothing leaks, no raster of the refused update stays
        const std::vector<std::pair<int, int>> five = {{5, 5}, {6, 5}, {7, 5}, {8, 5}, {9, 5}};
        for (long k = 0; k < 5; k++) {
            const long live = null_device_live_surfaces(), calls = R.calls;
            R.fail_at = calls + k;
            CHECK(smr_renderer_update_scene(r, "o", 64, 36, SMR_FRAME_PLANAR_YUV420, scene_of(five).c_str()) == SMR_ERR_INVALID);
            CHECK(has(r, "SVG image \"logo\"") && has(r, (std::to_string(5 + k) + "x5").c_str()));
            CHECK(R.calls == calls + k + 1 && null_device_live_surfaces() == live && g_live_staging == 0 && resident(r) == 1);
            CHECK(smr_renderer_node_count(r, "o") == 2);  // the previous scene: the view and one image
            CHECK(render() == 0);
            g_refused_calls++;
        }
        R.fail_at = -1;
        // ... and on a first update of an output: no output is left behind
        R.fail_at = R.calls;
        CHECK(smr_renderer_update_scene(r, "q", 16, 16, SMR_FRAME_RGBA, scene_of({{3, 3}}).c_str()) == SMR_ERR_INVALID && smr_renderer_node_count(r, "q") == -1);
        R.fail_at = -1;
        // a node above MAX_NODE_RESOLUTION: refused before the rasteriser is asked
        const long calls = R.calls;
        CHECK(smr_renderer_update_scene(r, "o", 64, 36, SMR_FRAME_PLANAR_YUV420, scene_of({{8000, 10}}).c_str()) == SMR_ERR_INVALID && has(r, "MAX_NODE_RESOLUTION"));
        CHECK(R.calls == calls && resident(r) == 1);
        // 17 sizes in one update: two launches
        std::vector<std::pair<int, int>> many;
        for (int i = 0; i < 17; i++) many.push_back({3 + i, 2 + (i % 5)});
        const long fix = g_fix_calls, fixed = g_fixed;
        uint64_t l0 = 0, l1 = 0;
        stats(r, nullptr, &l0, nullptr);
        CHECK(smr_renderer_update_scene(r, "o", 64, 36, SMR_FRAME_PLANAR_YUV420, scene_of(many).c_str()) == 0);
        stats(r, nullptr, &l1, nullptr);
        CHECK(R.calls == calls + 17 && resident(r) == 17);
        CHECK(g_fix_calls - fix == (gpu_mode ? 1 : 0) && g_fixed - fixed == (gpu_mode ? 17 : 0) && l1 - l0 == (gpu_mode ? 2u : 0u));
        CHECK(render() == 0 && render() == 0);
        // the same asset at 40 sizes over 40 updates: `resident` returns to what the last scene uses
        for (int k = 0; k < 40; k++) {
            CHECK(smr_renderer_update_scene(r, "o", 64, 36, SMR_FRAME_PLANAR_YUV420, scene_of({{10 + k, 7}, {4, 4}}).c_str()) == 0);
            CHECK(resident(r) == 2);
            if (k % 8 == 0) CHECK(render() == 0);
            g_size_updates++;
        }
        CHECK(R.calls == calls + 17 + 40 + 1);  // (4 x 4 was rasterised once: it stayed resident all along)
        // an opaque asset under a rescaler, two assets in one scene
        CHECK(smr_renderer_update_scene(r, "o", 64, 36, SMR_FRAME_PLANAR_YUV420,
                                        R"({"type":"view","children":[{"type":"rescaler","child":{"type":"image","image_id":"logo2"}},{"type":"image","image_id":"logo","width":4,"height":4}]})") == 0);
        CHECK(R2.calls == 1 && R2.sizes[0] == std::make_pair(10u, 10u) && resident(r) == 2);
        for (int k = 0; k < 4; k++) CHECK(render() == 0);
        // unregister: refused while in use, for every kind of image; fine afterwards, and the id can be registered anew
        CHECK(smr_renderer_unregister_image(r, "logo2") == SMR_ERR_INVALID && has(r, "a scene uses"));
        CHECK(smr_renderer_update_scene(r, "o", 64, 36, SMR_FRAME_PLANAR_YUV420, SCENE_PLAIN) == 0 && resident(r) == 0);
        CHECK(smr_renderer_unregister_image(r, "bitmap") == SMR_ERR_INVALID && has(r, "a scene uses"));
        CHECK(render() == 0);
        CHECK(smr_renderer_unregister_image(r, "logo2") == 0 && smr_renderer_unregister_image(r, "logo2") == 0);
        CHECK(smr_renderer_update_scene(r, "o", 64, 36, SMR_FRAME_PLANAR_YUV420, scene_of({{3, 3}}, "logo2").c_str()) == SMR_ERR_INVALID && has(r, "does not exist"));
        CHECK(smr_renderer_update_scene(r, "o", 64, 36, SMR_FRAME_PLANAR_YUV420, SCENE_EMPTY) == 0);
        {
            const long live = null_device_live_surfaces();
            CHECK(smr_renderer_unregister_image(r, "bitmap") == 0 && null_device_live_surfaces() == live - 1);
        }
        CHECK(smr_renderer_register_svg_image(r, "logo2", 12, 6, rasterise, &R2) == 0);
        CHECK(smr_renderer_update_scene(r, "o", 64, 36, SMR_FRAME_PLANAR_YUV420, scene_of({{-1, -1}, {-1, 3}}, "logo2").c_str()) == 0);
        CHECK(R2.calls == 3 && R2.sizes[1] == std::make_pair(12u, 6u) && R2.sizes[2] == std::make_pair(6u, 3u) && resident(r) == 2);
        CHECK(render() == 0);
    } else {
        for (int k = 0; k < 3; k++) {
            answer(smr_renderer_update_scene(r, "o", 64, 36, SMR_FRAME_PLANAR_YUV420, scene_of({{10 + k, 7}, {4, 4}, {-1, -1}}).c_str()));
            CHECK(g_live_staging == 0);
            answer(render());
        }
        answer(smr_renderer_update_scene(r, "o", 48, 30, SMR_FRAME_NV12, scene_of({{5, 5}}, "logo2").c_str()));
        answer(render());
    }
    null_device_fail_after(-1);
    g_staging_fail = -1;
    // destroyed with rasters resident
    CHECK(smr_renderer_update_scene(r, "z", 64, 36, SMR_FRAME_RGBA, scene_of({{11, 3}, {12, 3}}).c_str()) == 0 && resident(r) >= 2);
    CHECK(smr_renderer_sync(r) == 0);
    smr_renderer_destroy(r);
    for (auto &c : ctx) smr_ctx_destroy(c);
    CHECK(null_device_live_surfaces() == 0 && g_live_staging == 0);
}

int main() {
    long refused = 0, lives = 0;
    for (uint32_t mode = 0; mode < 2; mode++) { life(mode, -1, -1, &refused); lives++; }
    CHECK(refused == 0);
    for (long k = 0; k < 40; k++) { life((uint32_t)(k & 1), k, -1, &refused); lives++; }
    for (long k = 0; k < 12; k++) { life((uint32_t)(k & 1), -1, k, &refused); lives++; }
    CHECK(refused > 20);
    printf("{\"lives\": %ld, \"refused_with_oom\": %ld, \"checks\": %ld, \"uploads\": %ld, \"fix_calls\": %ld, \"refused_callbacks\": %ld, \"size_updates\": %ld}\n", lives,
           refused, g_checks, g_uploads, g_fix_calls, g_refused_calls, g_size_updates);
    return 0;
}
