// TEST INFRASTRUCTURE — not part of the product.  Animated images through the renderer (smelter_amd/csrc/host/renderer.cpp:
// smr_renderer_register_animated_image, the image pass in front of every output's graph walk, the per-lane node surfaces and their
// was_rendered flags) with the scene engine, compiled by g++ under AddressSanitizer + UBSan and linked against tests/san/null_device.cpp
// instead of the GPU half of the library — so smr_image_nodes is absent and the pass takes its one-rescale-per-job route.
// A fixed sequence: hostile registrations, scenes with animated nodes at their own size and scaled, alone and under Shader and View nodes,
// over two lanes with updates in between, then the same with every device allocation failing in turn.  The null device dereferences every
// surface it is handed (a destroyed one is a use-after-free report) and counts the ones it handed out: none may be left.
//   animated_driver            (prints one JSON line; exit status 0 = everything held)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#define SAN_DRIVER "animated_driver"
#include "san_driver.h"

extern "C" long null_device_live_surfaces();
extern "C" void null_device_fail_after(long n);

static const uint32_t W = 12, H = 10, N = 4;
static const uint64_t MS = 1000000ull;
static const uint64_t DELAYS[N] = {100 * MS, 200 * MS, 50 * MS, 150 * MS};

static std::vector<uint8_t> frames_of(uint32_t n, bool alternate_opaque) {
    std::vector<uint8_t> px((size_t)W * H * 4 * n);
    for (size_t i = 0; i < px.size(); i++) px[i] = (uint8_t)(i * 37 + i / 97);
    if (alternate_opaque)
        for (uint32_t k = 0; k < n; k += 2)
            for (size_t i = 0; i < (size_t)W * H; i++) px[((size_t)k * W * H + i) * 4 + 3] = 255;
    return px;
}

static bool has(const smr_renderer *r, const char *text) { return strstr(smr_renderer_last_error(r), text) != nullptr; }

static const char *SCENE_ALL =
    R"({"type":"view","children":[
        {"type":"image","id":"own","image_id":"gif"},
        {"type":"image","id":"scaled","image_id":"gif","width":37,"height":21},
        {"type":"shader","shader_id":"s1","resolution":{"width":64,"height":36},"children":[{"type":"image","image_id":"gif","width":20,"height":9},{"type":"image","image_id":"gif2"}]},
        {"type":"view","width":50,"height":40,"children":[{"type":"image","id":"inner","image_id":"gif2","width":33,"height":17},{"type":"image","image_id":"still","width":5,"height":5}]},
        {"type":"rescaler","child":{"type":"image","image_id":"still"}},
        {"type":"image","image_id":"still","width":24,"height":20}]})";
static const char *SCENE_CHANGED =
    R"({"type":"view","children":[
        {"type":"image","id":"scaled","image_id":"gif2","width":37,"height":21},
        {"type":"image","id":"own","image_id":"gif","width":13,"height":11},
        {"type":"image","image_id":"still","width":24,"height":20}]})";
static const char *SCENE_ROOT_IMAGE = R"({"type":"image","image_id":"gif","width":37,"height":21})";
static const char *SCENE_ROOT_OWN = R"({"type":"image","image_id":"gif2"})";
static const char *SCENE_STATIC_ONLY =
    R"({"type":"view","children":[{"type":"image","image_id":"still","width":24,"height":20},{"type":"image","image_id":"still","width":7,"height":9}]})";

static std::string many(int n) {
    std::string s = R"({"type":"view","children":[)";
    for (int i = 0; i < n; i++) {
        if (i) s += ",";
        s += R"({"type":"image","image_id":"gif","width":)" + std::to_string(14 + i) + R"(,"height":)" + std::to_string(11 + i) + "}";
    }
    return s + "]}";
}

static int render(smr_renderer *r, int64_t pts) {
    smr_output_frame out[4];
    uint32_t n = 0;
    const int rc = smr_renderer_render(r, pts, nullptr, 0, out, 4, &n);
    if (rc == 0)
        for (uint32_t k = 0; k < n && k < 4; k++) {
            smr_surface_info si;
            CHECK(smr_surface_info_get(out[k].frame->planes[0], &si) == 0);  // (the frame is the renderer's and alive)
        }
    return rc;
}
static uint64_t launches(const smr_renderer *r) {
    uint64_t n = 0;
    CHECK(smr_renderer_image_launches(r, &n) == 0);
    return n;
}

static void hostile_registrations(smr_renderer *r) {
    const std::vector<uint8_t> px = frames_of(N, false);
    std::vector<uint64_t> many_delays(1001, 1);
    CHECK(smr_renderer_register_animated_image(r, "none", px.data(), W, H, 0, DELAYS) == SMR_ERR_INVALID && has(r, "Animated image does not contain any frames."));
    CHECK(smr_renderer_register_animated_image(r, "none", nullptr, W, H, 0, nullptr) == SMR_ERR_INVALID && has(r, "does not contain any frames"));
    CHECK(smr_renderer_register_animated_image(r, "many", px.data(), 1, 1, 1001, many_delays.data()) == SMR_ERR_INVALID && has(r, "Detected over 1000 frames"));
    const uint64_t over[3] = {(uint64_t)INT64_MAX, 1, 0}, wrap[3] = {UINT64_MAX, UINT64_MAX, 2}, most[3] = {(uint64_t)INT64_MAX - 1, 1, 0};
    CHECK(smr_renderer_register_animated_image(r, "over", px.data(), W, H, 3, over) == SMR_ERR_INVALID && has(r, "INT64_MAX"));
    CHECK(smr_renderer_register_animated_image(r, "over", px.data(), W, H, 3, wrap) == SMR_ERR_INVALID);
    CHECK(smr_renderer_register_animated_image(r, "most", px.data(), W, H, 3, most) == 0);  // exactly INT64_MAX is a duration
    CHECK(smr_renderer_register_animated_image(nullptr, "x", px.data(), W, H, N, DELAYS) == SMR_ERR_INVALID);
    CHECK(smr_renderer_register_animated_image(r, nullptr, px.data(), W, H, N, DELAYS) == SMR_ERR_INVALID && has(r, "null argument"));
    CHECK(smr_renderer_register_animated_image(r, "x", nullptr, W, H, N, DELAYS) == SMR_ERR_INVALID && has(r, "null argument"));
    CHECK(smr_renderer_register_animated_image(r, "x", px.data(), W, H, N, nullptr) == SMR_ERR_INVALID);
    CHECK(smr_renderer_register_animated_image(r, "x", px.data(), 0, H, N, DELAYS) == SMR_ERR_INVALID);
    CHECK(smr_renderer_register_animated_image(r, "x", px.data(), W, 0, N, DELAYS) == SMR_ERR_INVALID);
    // one frame: a static image (the delay is not even read), and the id is taken like any other
    CHECK(smr_renderer_register_animated_image(r, "single", px.data(), W, H, 1, nullptr) == 0);
    CHECK(smr_renderer_register_image(r, "single", px.data(), W, H) == SMR_ERR_INVALID && has(r, "already registered"));
    CHECK(smr_renderer_register_animated_image(r, "single", px.data(), W, H, N, DELAYS) == SMR_ERR_INVALID && has(r, "already registered"));
    CHECK(smr_renderer_register_animated_image(r, "gif", px.data(), W, H, N, DELAYS) == 0);
    CHECK(smr_renderer_register_animated_image(r, "gif", px.data(), W, H, N, DELAYS) == SMR_ERR_INVALID && has(r, "Image \"gif\" is already registered"));
    CHECK(smr_renderer_register_animated_image(r, "gif", px.data(), W, H, 1, DELAYS) == SMR_ERR_INVALID && has(r, "already registered"));
    CHECK(smr_renderer_register_image(r, "gif", px.data(), W, H) == SMR_ERR_INVALID && has(r, "already registered"));
    uint64_t n = 5;
    CHECK(smr_renderer_image_launches(nullptr, &n) == SMR_ERR_INVALID && smr_renderer_image_launches(r, nullptr) == SMR_ERR_INVALID && n == 5);
}

// one renderer's life; `fail_at` >= 0: the fail_at-th device allocation from the first scene on fails (and whatever is refused is an answer)
static void life(uint32_t mode, long fail_at, long *refused) {
    smr_ctx *ctx[2];
    for (auto &c : ctx) CHECK(smr_ctx_create(0, mode, 100, nullptr, &c) == 0);
    smr_renderer *r = nullptr;
    CHECK(smr_renderer_create(ctx[0], -1, &r) == 0);
    hostile_registrations(r);
    const std::vector<uint8_t> alt = frames_of(N, true);
    CHECK(smr_renderer_register_animated_image(r, "gif2", alt.data(), W, H, N, DELAYS) == 0);
    CHECK(smr_renderer_register_image(r, "still", alt.data(), W, H) == 0);
    CHECK(smr_renderer_register_shader(r, "s1", SMR_SHADER_LAYOUT_PLANES) == 0);
    CHECK(smr_renderer_add_lane(r, ctx[1]) == 0);
    const bool strict = fail_at < 0;
    auto answer = [&](int rc) {
        if (strict) CHECK(rc == 0);
        else if (rc < 0) { CHECK(rc == SMR_ERR_OOM); (*refused)++; }
    };
    if (!strict) null_device_fail_after(fail_at);

    int64_t pts = 0;
    answer(smr_renderer_update_scene(r, "out", 128, 72, SMR_FRAME_PLANAR_YUV420, SCENE_ALL));
    answer(smr_renderer_update_scene(r, "rgba", 64, 36, SMR_FRAME_RGBA, SCENE_ROOT_IMAGE));  // a root Image of its own size, not the output's
    answer(smr_renderer_update_scene(r, "own", 12, 10, SMR_FRAME_NV12, SCENE_ROOT_OWN));
    if (strict) {
        // "out": 3 scaled animated nodes + 2 scaled static ones, "rgba": 1 scaled animated node; without smr_image_nodes one launch per job
        uint64_t before = launches(r);
        CHECK(render(r, pts) == 0);
        CHECK(launches(r) - before == 6);
        before = launches(r);
        CHECK(render(r, pts += 40 * MS) == 0);  // (lane 1: its own surfaces, nothing drawn yet)
        CHECK(launches(r) - before == 6);
        before = launches(r);
        CHECK(render(r, pts += 40 * MS) == 0);  // lane 0 again: the static nodes are there
        CHECK(launches(r) - before == 4);
    }
    for (int k = 0; k < 6; k++) answer(render(r, pts += 70 * MS));
    answer(smr_renderer_update_scene(r, "out", 128, 72, SMR_FRAME_PLANAR_YUV420, SCENE_ALL));  // the same scene: clocks run on, surfaces start over
    if (strict) {
        const uint64_t before = launches(r);
        CHECK(render(r, pts += 70 * MS) == 0);
        CHECK(launches(r) - before == 6);  // (the graph changed hands: the static nodes are drawn again)
    }
    for (int k = 0; k < 3; k++) answer(render(r, pts += 70 * MS));
    answer(smr_renderer_update_scene(r, "out", 130, 72, SMR_FRAME_PLANAR_YUV444, SCENE_CHANGED));
    for (int k = 0; k < 4; k++) answer(render(r, pts += 70 * MS));
    answer(smr_renderer_update_scene(r, "out", 130, 72, SMR_FRAME_PLANAR_YUV444, SCENE_STATIC_ONLY));
    for (int k = 0; k < 2; k++) answer(render(r, pts += 70 * MS));
    if (strict) {
        const uint64_t before = launches(r);
        CHECK(smr_renderer_unregister_output(r, "rgba") == 0);
        CHECK(render(r, pts += 70 * MS) == 0 && render(r, pts += 70 * MS) == 0);
        CHECK(launches(r) == before);  // only static nodes remain, both lanes have drawn them
    }
    answer(smr_renderer_update_scene(r, "out", 128, 72, SMR_FRAME_PLANAR_YUV420, many(17).c_str()));
    for (int k = 0; k < 3; k++) answer(render(r, pts += 70 * MS));
    CHECK(render(r, INT64_MIN) == 0 || !strict);  // a pts before every clock's start: time 0
    // a registration while outputs exist, with the device failing: nothing may be half registered
    {
        const std::vector<uint8_t> px = frames_of(N, false);
        const int rc = smr_renderer_register_animated_image(r, "late", px.data(), W, H, N, DELAYS);
        answer(rc);
        null_device_fail_after(-1);
        if (rc < 0) CHECK(smr_renderer_register_animated_image(r, "late", px.data(), W, H, N, DELAYS) == 0);  // the id was not taken
        CHECK(smr_renderer_update_scene(r, "late", 64, 36, SMR_FRAME_RGBA, R"({"type":"image","image_id":"late","width":30,"height":30})") == 0);
    }
    null_device_fail_after(-1);
    // with the device well again everything renders
    CHECK(smr_renderer_update_scene(r, "out", 128, 72, SMR_FRAME_PLANAR_YUV420, SCENE_ALL) == 0);
    for (int k = 0; k < 4; k++) CHECK(render(r, pts += 70 * MS) == 0);
    CHECK(smr_renderer_sync(r) == 0);
    smr_renderer_destroy(r);
    for (auto &c : ctx) smr_ctx_destroy(c);
    CHECK(null_device_live_surfaces() == 0);
}

int main() {
    long refused = 0, lives = 0;
    for (uint32_t mode = 0; mode < 2; mode++) { life(mode, -1, &refused); lives++; }
    CHECK(refused == 0);
    // registration alone under a failing device: SMR_ERR_OOM, nothing registered, nothing leaked
    {
        smr_ctx *ctx = nullptr;
        CHECK(smr_ctx_create(0, 0, 100, nullptr, &ctx) == 0);
        smr_renderer *r = nullptr;
        CHECK(smr_renderer_create(ctx, -1, &r) == 0);
        const std::vector<uint8_t> px = frames_of(N, false);
        long ooms = 0;
        for (long k = 0; k < 8; k++) {
            null_device_fail_after(k);
            const int rc = smr_renderer_register_animated_image(r, "gif", px.data(), W, H, N, DELAYS);
            null_device_fail_after(-1);
            if (rc == 0) { CHECK(k == (long)N + 1); break; }  // a staging surface and one per frame
            CHECK(rc == SMR_ERR_OOM && null_device_live_surfaces() == 0);
            CHECK(smr_renderer_update_scene(r, "o", 16, 16, SMR_FRAME_RGBA, R"({"type":"image","image_id":"gif"})") == SMR_ERR_INVALID);  // not registered
            ooms++;
        }
        CHECK(ooms == (long)N + 1 && null_device_live_surfaces() == (long)N);
        smr_renderer_destroy(r);
        smr_ctx_destroy(ctx);
        CHECK(null_device_live_surfaces() == 0);
    }
    for (long k = 0; k < 90; k++) { life((uint32_t)(k & 1), k, &refused); lives++; }
    CHECK(refused > 60);
    printf("{\"lives\": %ld, \"refused_with_oom\": %ld, \"checks\": %ld}\n", lives, refused, g_checks);
    return 0;
}
