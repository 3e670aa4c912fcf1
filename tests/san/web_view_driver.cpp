// TEST INFRASTRUCTURE — not part of the product.  WebView nodes through the renderer (smelter_amd/csrc/host/renderer.cpp:
// smr_renderer_register_web_renderer / _web_paint / _web_positions, the pinned staging ring, the per-lane page copies, the node's place in
// the graph walk, exclusivity across outputs) with the scene engine, compiled by g++ under AddressSanitizer + UBSan and linked against
// tests/san/null_device.cpp instead of the GPU half of the library.  The five entry points the renderer reaches through weak references for
// this feature are defined HERE, as stand-ins of the null device's kind: staging buffers of exactly the size asked for (a copy that
// overruns one is a report), an upload that reads every byte of the buffer it is handed and dereferences the frame, a stream that is idle or
// busy as the sequence says, and an smr_web_view that checks and reads everything it is given.
// A fixed sequence: register / paint / positions / unregister churn, hostile sizes and pitches, more and fewer rectangles than children, a
// repaint between updates, a busy stream that makes the staging ring grow and then wait, the renderer destroyed with paints pending, then
// the same with every device allocation failing in turn.
//   web_view_driver            (prints one JSON line; exit status 0 = everything held)
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#define SAN_DRIVER "web_view_driver"
#include "san_driver.h"

extern "C" long null_device_live_surfaces();
extern "C" void null_device_fail_after(long n);

// ---- the stand-ins (staging and upload: san_driver.h)
static long g_web_calls = 0, g_web_children = 0, g_idle_queries = 0, g_syncs_seen = 0;
static int g_stream_idle = 1;      // what smr_ctx_stream_idle answers
static size_t g_page_bytes = 0;    // what an upload must be able to read

extern "C" {
int smr_host_alloc(smr_ctx *ctx, size_t bytes, void **out) { return san_host_alloc(ctx, bytes, out); }
void smr_host_free(smr_ctx *ctx, void *p) { san_host_free(ctx, p); }
int smr_frame_upload_async(smr_ctx *ctx, const smr_frame *f, const void *const host_planes[3]) {
    if (!f || (size_t)f->width * 4 * f->height != g_page_bytes) return SMR_ERR_INVALID;
    return san_frame_upload(ctx, f, host_planes, SMR_FRAME_BGRA);
}
int smr_ctx_stream_idle(smr_ctx *ctx) {
    if (!ctx) return SMR_ERR_INVALID;
    g_idle_queries++;
    return g_stream_idle;
}
int smr_web_view(smr_ctx *ctx, const void *page, size_t page_pitch, smr_surface *dst, const smr_surface *const *srcs, const smr_web_rect *rects, uint32_t n, int under) {
    smr_surface_info di, si;
    if (!ctx || !page || smr_surface_info_get(dst, &di) != 0 || di.format != SMR_PX_RGBA8 || (n && (!srcs || !rects)) || (under != 0 && under != 1)) return SMR_ERR_INVALID;
    if (page_pitch < (size_t)di.width * 4) return SMR_ERR_INVALID;
    touch(page, 1);
    touch(rects, (size_t)n * sizeof(smr_web_rect));
    for (uint32_t i = 0; i < n; i++) {
        if (!srcs[i]) continue;
        if (smr_surface_info_get(srcs[i], &si) != 0 || si.format != SMR_PX_RGBA8 || srcs[i] == dst) return SMR_ERR_INVALID;
    }
    g_web_calls++;
    g_web_children += n;
    return SMR_OK;
}
}

static const uint32_t W = 40, H = 24;
static bool has(const smr_renderer *r, const char *text) { return strstr(smr_renderer_last_error(r), text) != nullptr; }

static const char *SCENE_WEB =
    R"({"type":"view","children":[
        {"type":"web_view","id":"w","instance_id":"page","children":[
            {"type":"image","id":"c0","image_id":"img"},
            {"type":"input_stream","id":"c1","input_id":"cam"},
            {"type":"view","id":"c2","width":20,"height":10,"children":[{"type":"image","image_id":"img"}]}]},
        {"type":"image","image_id":"img","width":9,"height":7}]})";
static const char *SCENE_WEB_ROOT = R"({"type":"web_view","instance_id":"page","children":[{"type":"input_stream","id":"c0","input_id":"missing"}]})";
static const char *SCENE_IN_RESCALER = R"({"type":"rescaler","child":{"type":"web_view","instance_id":"page"}})";
static const char *SCENE_OTHER = R"({"type":"view","children":[{"type":"web_view","instance_id":"other"}]})";
static const char *SCENE_PLAIN = R"({"type":"view","children":[{"type":"image","image_id":"img"}]})";
static const char *SCENE_TWICE = R"({"type":"view","children":[{"type":"web_view","instance_id":"page"},{"type":"web_view","instance_id":"page"}]})";

static std::string many(int n) {
    std::string s = R"({"type":"web_view","instance_id":"page","children":[)";
    for (int i = 0; i < n; i++) {
        if (i) s += ",";
        s += R"({"type":"image","id":"k)" + std::to_string(i) + R"(","image_id":"img"})";
    }
    return s + "]}";
}

static uint64_t launches(const smr_renderer *r) {
    uint64_t n = 0;
    CHECK(smr_renderer_web_launches(r, &n) == 0);
    return n;
}

static void hostile(smr_renderer *r, const std::vector<uint8_t> &px) {
    CHECK(smr_renderer_register_web_renderer(nullptr, "x", W, H, SMR_WEB_NATIVE_OVER_CONTENT) == SMR_ERR_INVALID);
    CHECK(smr_renderer_register_web_renderer(r, nullptr, W, H, SMR_WEB_NATIVE_OVER_CONTENT) == SMR_ERR_INVALID && has(r, "null argument"));
    CHECK(smr_renderer_register_web_renderer(r, "x", 0, H, SMR_WEB_NATIVE_OVER_CONTENT) == SMR_ERR_INVALID);
    CHECK(smr_renderer_register_web_renderer(r, "x", W, 0, SMR_WEB_NATIVE_OVER_CONTENT) == SMR_ERR_INVALID);
    CHECK(smr_renderer_register_web_renderer(r, "x", 7683, H, SMR_WEB_NATIVE_OVER_CONTENT) == SMR_ERR_INVALID && has(r, "MAX_NODE_RESOLUTION"));
    CHECK(smr_renderer_register_web_renderer(r, "x", W, 4321, SMR_WEB_NATIVE_OVER_CONTENT) == SMR_ERR_INVALID);
    CHECK(smr_renderer_register_web_renderer(r, "x", UINT32_MAX, UINT32_MAX, SMR_WEB_NATIVE_OVER_CONTENT) == SMR_ERR_INVALID);
    CHECK(smr_renderer_register_web_renderer(r, "x", W, H, 3) == SMR_ERR_INVALID && has(r, "embedding"));
    CHECK(smr_renderer_register_web_renderer(r, "x", W, H, UINT32_MAX) == SMR_ERR_INVALID);
    CHECK(smr_renderer_register_web_renderer(r, "page", W, H, SMR_WEB_NATIVE_OVER_CONTENT) == 0);
    CHECK(smr_renderer_register_web_renderer(r, "page", W, H, SMR_WEB_NATIVE_UNDER_CONTENT) == SMR_ERR_INVALID && has(r, "already registered"));
    // paints
    CHECK(smr_renderer_web_paint(nullptr, "page", px.data(), 0) == SMR_ERR_INVALID);
    CHECK(smr_renderer_web_paint(r, nullptr, px.data(), 0) == SMR_ERR_INVALID);
    CHECK(smr_renderer_web_paint(r, "page", nullptr, 0) == SMR_ERR_INVALID);
    CHECK(smr_renderer_web_paint(r, "nobody", px.data(), 0) == SMR_ERR_INVALID && has(r, "not registered"));
    CHECK(smr_renderer_web_paint(r, "page", px.data(), W * 4 - 1) == SMR_ERR_INVALID && has(r, "pitch"));
    CHECK(smr_renderer_web_paint(r, "page", px.data(), 1) == SMR_ERR_INVALID);
    CHECK(g_live_staging == 0);  // (a refused paint allocates nothing)
    // positions
    const smr_web_rect q[2] = {{1, 2, 3, 4}, {NAN, INFINITY, -1, 0}};
    CHECK(smr_renderer_web_positions(nullptr, "page", q, 2) == SMR_ERR_INVALID);
    CHECK(smr_renderer_web_positions(r, nullptr, q, 2) == SMR_ERR_INVALID);
    CHECK(smr_renderer_web_positions(r, "page", nullptr, 2) == SMR_ERR_INVALID);
    CHECK(smr_renderer_web_positions(r, "nobody", q, 2) == SMR_ERR_INVALID && has(r, "not registered"));
    CHECK(smr_renderer_web_positions(r, "page", nullptr, 0) == 0);
    CHECK(smr_renderer_web_positions(r, "page", q, 2) == 0);
    uint64_t n = 5;
    CHECK(smr_renderer_web_launches(nullptr, &n) == SMR_ERR_INVALID && smr_renderer_web_launches(r, nullptr) == SMR_ERR_INVALID && n == 5);
    CHECK(smr_renderer_unregister_web_renderer(r, "nobody") == 0 && smr_renderer_unregister_web_renderer(r, nullptr) == SMR_ERR_INVALID);
}

// one renderer's life; `fail_at` >= 0: the fail_at-th device allocation from the first scene on fails (and whatever is refused is an answer)
static void life(uint32_t mode, long fail_at, long *refused) {
    smr_ctx *ctx[2];
    for (auto &c : ctx) CHECK(smr_ctx_create(0, mode, 100, nullptr, &c) == 0);
    smr_renderer *r = nullptr;
    CHECK(smr_renderer_create(ctx[0], -1, &r) == 0);
    g_page_bytes = (size_t)W * 4 * H;
    g_stream_idle = 1;
    // a paint in a buffer of exactly its size: tight, and with a pitch larger than the row (the last row is not padded)
    std::vector<uint8_t> px((size_t)W * 4 * H), pitched((size_t)(W * 4 + 12) * (H - 1) + W * 4);
    for (size_t i = 0; i < px.size(); i++) px[i] = (uint8_t)(i * 31 + i / 89);
    for (size_t i = 0; i < pitched.size(); i++) pitched[i] = (uint8_t)(i * 17);
    hostile(r, px);
    CHECK(smr_renderer_register_image(r, "img", px.data(), 12, 10) == 0);
    CHECK(smr_renderer_register_input(r, "cam") == 0);
    CHECK(smr_renderer_add_lane(r, ctx[1]) == 0);
    smr_frame cam;
    CHECK(smr_frame_create(ctx[0], SMR_FRAME_PLANAR_YUV420, 16, 16, &cam) == 0);
    const bool strict = fail_at < 0;
    auto answer = [&](int rc) {
        if (strict) CHECK(rc == 0);
        else if (rc < 0) { CHECK(rc == SMR_ERR_OOM); (*refused)++; }
    };
    int64_t pts = 0;
    auto render = [&]() {
        smr_output_frame out[4];
        uint32_t n = 0;
        const smr_input_frame in = {"cam", &cam, pts};
        const int rc = smr_renderer_render(r, pts, &in, 1, out, 4, &n);
        pts += 40000000;
        return rc;
    };
    if (!strict) null_device_fail_after(fail_at);

    // not registered / used twice / a child without an id: refused, nothing changes hands
    CHECK(smr_renderer_update_scene(r, "o", 64, 36, SMR_FRAME_PLANAR_YUV420, SCENE_OTHER) == SMR_ERR_INVALID && has(r, "Instance of web renderer \"other\" does not exist"));
    CHECK(smr_renderer_update_scene(r, "o", 64, 36, SMR_FRAME_PLANAR_YUV420, SCENE_TWICE) == SMR_ERR_INVALID && has(r, "was used more than once"));
    CHECK(smr_renderer_update_scene(r, "o", 64, 36, SMR_FRAME_PLANAR_YUV420, R"({"type":"web_view","instance_id":"page","children":[{"type":"view"}]})") == SMR_ERR_INVALID &&
          has(r, "has children without \"id\" property"));
    CHECK(smr_renderer_node_count(r, "o") == -1);  // (a failed first update leaves no output behind)

    answer(smr_renderer_update_scene(r, "o", 64, 36, SMR_FRAME_PLANAR_YUV420, SCENE_WEB));
    const bool have_o = smr_renderer_node_count(r, "o") > 0;
    if (have_o) {
        smr_scene_node info;
        CHECK(smr_renderer_node_info(r, "o", 1, &info) == 0 && info.kind == SMR_NODE_WEB_VIEW && info.width == W && info.height == H && info.n_children == 3);
        // across outputs: the instance is taken; the refused update leaves "o" as it is and no second output behind
        CHECK(smr_renderer_update_scene(r, "p", 64, 36, SMR_FRAME_RGBA, SCENE_WEB_ROOT) == SMR_ERR_INVALID && has(r, "Instance of web renderer \"page\" was used more than once"));
        CHECK(smr_renderer_node_count(r, "p") == -1 && smr_renderer_node_count(r, "o") == 7);
        CHECK(smr_renderer_unregister_web_renderer(r, "page") == SMR_ERR_INVALID && has(r, "a scene uses"));
    }
    // before the first paint: no texture, no launch, no upload
    uint64_t before = launches(r);
    long uploads = g_uploads;
    answer(render());
    answer(render());
    CHECK(launches(r) == before && g_uploads == uploads && g_web_calls == 0);
    // the first paint: each lane uploads once, then not again; one launch per render
    answer(smr_renderer_web_paint(r, "page", px.data(), 0));
    if (strict) {
        CHECK(g_live_staging == 1);
        before = launches(r); uploads = g_uploads;
        const long children = g_web_children;
        for (int k = 0; k < 4; k++) CHECK(render() == 0);
        CHECK(launches(r) - before == 4 && g_uploads - uploads == 2 && g_web_calls == 4);
        CHECK(g_web_children - children == 4 * 2);  // two rectangles were handed over (hostile()), three children: zipped
        // more rectangles than children, fewer, none
        const smr_web_rect five[5] = {{0, 0, 10, 10}, {5.25f, 5.75f, 8, 8}, {-100, -100, 1e9f, 1e9f}, {1, 1, 1, 1}, {2, 2, 2, 2}};
        CHECK(smr_renderer_web_positions(r, "page", five, 5) == 0);
        long c0 = g_web_children;
        CHECK(render() == 0 && g_web_children - c0 == 3);
        CHECK(smr_renderer_web_positions(r, "page", five, 1) == 0);
        c0 = g_web_children;
        CHECK(render() == 0 && g_web_children - c0 == 1);
        CHECK(smr_renderer_web_positions(r, "page", nullptr, 0) == 0);
        c0 = g_web_children;
        CHECK(render() == 0 && g_web_children - c0 == 0);
        CHECK(smr_renderer_web_positions(r, "page", five, 5) == 0);
        // a repaint (pitched): both lanes upload again, the staging buffer is reused while every stream is idle
        uploads = g_uploads;
        CHECK(smr_renderer_web_paint(r, "page", pitched.data(), W * 4 + 12) == 0 && g_live_staging == 1);
        CHECK(render() == 0 && render() == 0 && render() == 0 && g_uploads - uploads == 2);
        // busy streams: a buffer an upload was queued from is not written again — the ring grows to four, then the paint waits
        g_stream_idle = 0;
        for (int k = 0; k < 7; k++) {
            CHECK(smr_renderer_web_paint(r, "page", px.data(), 0) == 0);
            CHECK(render() == 0);
        }
        CHECK(g_live_staging == 4);
        g_stream_idle = 1;
        CHECK(smr_renderer_web_paint(r, "page", px.data(), 0) == 0 && g_live_staging == 4);
    } else {
        for (int k = 0; k < 3; k++) answer(render());
        answer(smr_renderer_web_paint(r, "page", pitched.data(), W * 4 + 12));
        for (int k = 0; k < 2; k++) answer(render());
    }
    // a repaint between updates; the node as the root, inside a rescaler, with 17 children
    answer(smr_renderer_update_scene(r, "o", 64, 36, SMR_FRAME_PLANAR_YUV420, SCENE_IN_RESCALER));
    answer(smr_renderer_web_paint(r, "page", px.data(), 0));
    answer(render());
    answer(smr_renderer_update_scene(r, "o", 64, 36, SMR_FRAME_RGBA, SCENE_WEB_ROOT));
    answer(render());
    answer(smr_renderer_update_scene(r, "o", 48, 30, SMR_FRAME_NV12, many(17).c_str()));
    {
        std::vector<smr_web_rect> q(17);
        for (int i = 0; i < 17; i++) q[i] = {(float)i, (float)(i / 2), 6.0f, 5.0f};
        CHECK(smr_renderer_web_positions(r, "page", q.data(), 17) == 0);
        before = launches(r);
        const int rc = render();
        answer(rc);
        if (strict) CHECK(launches(r) - before == 2);
        CHECK(smr_renderer_web_positions(r, "page", q.data(), 16) == 0);
        before = launches(r);
        if (strict) CHECK(render() == 0 && launches(r) - before == 1);
    }
    null_device_fail_after(-1);
    // the instance moves to another output once the first lets go of it; then it can be unregistered and registered at another size
    CHECK(smr_renderer_update_scene(r, "o", 64, 36, SMR_FRAME_PLANAR_YUV420, SCENE_PLAIN) == 0);
    CHECK(smr_renderer_update_scene(r, "p", 64, 36, SMR_FRAME_RGBA, SCENE_WEB_ROOT) == 0);
    CHECK(render() == 0);
    CHECK(smr_renderer_unregister_output(r, "p") == 0);
    CHECK(smr_renderer_unregister_web_renderer(r, "page") == 0 && g_live_staging == 0);
    CHECK(smr_renderer_update_scene(r, "p", 64, 36, SMR_FRAME_RGBA, SCENE_WEB_ROOT) == SMR_ERR_INVALID && has(r, "does not exist"));
    CHECK(smr_renderer_register_web_renderer(r, "page", 7, 5, SMR_WEB_CHROMIUM_EMBEDDING) == 0);
    CHECK(smr_renderer_register_web_renderer(r, "other", 1, 1, SMR_WEB_NATIVE_UNDER_CONTENT) == 0);
    g_page_bytes = 7 * 4 * 5;
    CHECK(smr_renderer_update_scene(r, "p", 64, 36, SMR_FRAME_RGBA, many(3).c_str()) == 0);
    CHECK(smr_renderer_web_paint(r, "page", px.data(), 64) == 0);
    {
        const smr_web_rect q[3] = {{0, 0, 1, 1}, {1, 1, 1, 1}, {2, 2, 2, 2}};
        CHECK(smr_renderer_web_positions(r, "page", q, 3) == 0);
        const long c0 = g_web_children;
        CHECK(render() == 0 && g_web_children == c0);  // Chromium embedding: the page alone
    }
    // destroyed with paints pending: one nobody rendered, one on an instance no scene uses, a busy stream
    CHECK(smr_renderer_web_paint(r, "page", px.data(), 0) == 0);
    g_page_bytes = 4;
    CHECK(smr_renderer_web_paint(r, "other", px.data(), 0) == 0);
    g_stream_idle = 0;
    CHECK(smr_renderer_sync(r) == 0);
    smr_renderer_destroy(r);
    g_stream_idle = 1;
    smr_frame_destroy(ctx[0], &cam);
    for (auto &c : ctx) smr_ctx_destroy(c);
    CHECK(null_device_live_surfaces() == 0 && g_live_staging == 0);
    g_web_calls = 0;
    (void)g_syncs_seen;
}

int main() {
    long refused = 0, lives = 0;
    for (uint32_t mode = 0; mode < 2; mode++) { life(mode, -1, &refused); lives++; }
    CHECK(refused == 0);
    // a staging allocation that fails: SMR_ERR_OOM, the previous paint stays the latest, nothing leaks
    {
        smr_ctx *ctx = nullptr;
        CHECK(smr_ctx_create(0, 0, 100, nullptr, &ctx) == 0);
        smr_renderer *r = nullptr;
        CHECK(smr_renderer_create(ctx, -1, &r) == 0);
        std::vector<uint8_t> px((size_t)W * 4 * H, 7);
        g_page_bytes = px.size();
        CHECK(smr_renderer_register_web_renderer(r, "page", W, H, SMR_WEB_NATIVE_UNDER_CONTENT) == 0);
        g_staging_fail = 0;
        CHECK(smr_renderer_web_paint(r, "page", px.data(), 0) == SMR_ERR_OOM && g_live_staging == 0);
        g_staging_fail = -1;
        CHECK(smr_renderer_web_paint(r, "page", px.data(), 0) == 0 && g_live_staging == 1);
        smr_renderer_destroy(r);
        smr_ctx_destroy(ctx);
        CHECK(null_device_live_surfaces() == 0 && g_live_staging == 0);
    }
    for (long k = 0; k < 40; k++) { life((uint32_t)(k & 1), k, &refused); lives++; }
    CHECK(refused > 20);
    printf("{\"lives\": %ld, \"refused_with_oom\": %ld, \"checks\": %ld, \"uploads\": %ld, \"idle_queries\": %ld}\n", lives, refused, g_checks, g_uploads, g_idle_queries);
    return 0;
}
