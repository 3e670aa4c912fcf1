// TEST INFRASTRUCTURE — not part of the product.  Two host pieces of the batched Text path, compiled by g++ under AddressSanitizer + UBSan
// into a stand-alone program with its own main:
//   * tx_plan (smelter_amd/csrc/host/text_bins.h): the tile bins k_text_nodes walks, fed glyphs with INT32_MAX / INT32_MIN coordinates and
//     sizes, 10^5 glyphs in one tile, random runs — bin_first monotone and ending on the entry count, every listed index in range and
//     ascending within its bin, and every bin exactly the glyphs a 64-bit brute-force intersection test puts there;
//   * the Text raster cache of smelter_amd/csrc/host/renderer.cpp against tests/san/null_device.cpp (the renderer's route without the GPU
//     half: one smr_blit_glyphs call per new raster): updates that add, drop and duplicate Text nodes over two outputs, smr_renderer_set_text
//     on a node whose raster is shared, a font-book swap, both outputs unregistered — the reference counts recounted after every step
//     (smr_renderer_text_cache_check), `resident` what the active scenes show, 0 at the end, no surface left.
//   text_bins_driver <directory of .ttf files>        (prints one JSON line; exit status 0 = everything held)
#include <algorithm>
#include <climits>
#include <string>
#include <vector>

#define SAN_DRIVER "text_bins_driver"
#include "san_driver.h"
#include "text_bins.h"

extern "C" long null_device_live_surfaces();
struct smr_renderer;
int smr_renderer_text_cache_check(const smr_renderer *r);  // renderer.cpp

// ---- tx_plan
static uint64_t g_seed = 0x243f6a8885a308d3ull;
static uint32_t rnd() {
    g_seed = g_seed * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(g_seed >> 33);
}

static long g_plans = 0, g_entries = 0;

// does glyph g, clipped to w x h, intersect tile (tx, ty)?  (64-bit, written without tx_range)
static bool touches(int w, int h, const smr_glyph &g, uint32_t tx, uint32_t ty) {
    if (g.w <= 0 || g.h <= 0) return false;
    const int64_t gx0 = g.dst_x, gx1 = (int64_t)g.dst_x + g.w, gy0 = g.dst_y, gy1 = (int64_t)g.dst_y + g.h;
    const int64_t x0 = (int64_t)tx * SMR_TEXT_TILE_W, x1 = std::min<int64_t>(x0 + SMR_TEXT_TILE_W, w);
    const int64_t y0 = (int64_t)ty * SMR_TEXT_TILE_H, y1 = std::min<int64_t>(y0 + SMR_TEXT_TILE_H, h);
    return gx0 < x1 && gx1 > x0 && gy0 < y1 && gy1 > y0;
}

static void check_plan(int w, int h, const std::vector<smr_glyph> &glyphs, bool brute) {
    const uint32_t n = (uint32_t)glyphs.size(), tiles = tx_tiles(w, h), tiles_x = tx_tiles_x(w);
    const uint64_t entries = tx_entries(w, h, glyphs.data(), n);
    CHECK(entries <= (uint64_t)n * tiles);
    // buffers of exactly the sizes the launcher gives them: an index or a count too many is a report
    std::vector<uint32_t> first((size_t)tiles + 1, 0xdeadbeefu), bin((size_t)entries, 0xdeadbeefu);
    CHECK(tx_plan(w, h, glyphs.data(), n, first.data(), bin.data()));
    CHECK(first[0] == 0 && first[tiles] == entries);
    for (uint32_t t = 0; t < tiles; t++) {
        CHECK(first[t] <= first[t + 1]);
        for (uint32_t e = first[t]; e < first[t + 1]; e++) {
            CHECK(bin[e] < n);
            if (e > first[t]) CHECK(bin[e] > bin[e - 1]);
        }
        if (!brute) continue;
        uint32_t e = first[t];
        for (uint32_t i = 0; i < n; i++)
            if (touches(w, h, glyphs[i], t % tiles_x, t / tiles_x)) { CHECK(e < first[t + 1] && bin[e] == i); e++; }
        CHECK(e == first[t + 1]);
    }
    g_plans++;
    g_entries += (long)entries;
}

static smr_glyph glyph(int32_t x, int32_t y, int32_t w, int32_t h) {
    smr_glyph g;
    memset(&g, 0, sizeof(g));
    g.dst_x = x; g.dst_y = y; g.w = w; g.h = h;
    g.color[3] = 1.0f;
    return g;
}

static void plans() {
    const int32_t ends[] = {INT32_MIN, INT32_MIN + 1, -65, -64, -1, 0, 1, 63, 64, 65, 130, 131, INT32_MAX - 1, INT32_MAX};
    const int32_t sizes[] = {INT32_MIN, -1, 0, 1, 2, 64, 65, 200, INT32_MAX - 1, INT32_MAX};
    // every pairing of an extreme origin with an extreme size, on both axes, in one run per surface
    for (const auto &wh : std::vector<std::pair<int, int>>{{131, 34}, {1, 1}, {64, 16}, {65, 17}, {7682, 4320}, {0, 5}, {5, 0}, {-3, 9}}) {
        std::vector<smr_glyph> run;
        for (int32_t x : ends)
            for (int32_t s : sizes) {
                run.push_back(glyph(x, 3, s, 5));
                run.push_back(glyph(3, x, 5, s));
                run.push_back(glyph(x, x, s, s));
            }
        check_plan(wh.first, wh.second, run, wh.first <= 200);
    }
    // 10^5 glyphs in one tile (and its neighbours empty)
    {
        std::vector<smr_glyph> run;
        for (int i = 0; i < 100000; i++) run.push_back(glyph(64 + (int)(rnd() % 60), 16 + (int)(rnd() % 12), 1 + (int)(rnd() % 4), 1 + (int)(rnd() % 4)));
        check_plan(200, 50, run, false);
        std::vector<uint32_t> first(tx_tiles(200, 50) + 1), bin(tx_entries(200, 50, run.data(), 100000));
        CHECK(tx_plan(200, 50, run.data(), 100000, first.data(), bin.data()));
        const uint32_t t = 1 * tx_tiles_x(200) + 1;
        CHECK(first[t + 1] - first[t] == 100000 && bin.size() == 100000);
    }
    // a hostile run of full-node quads: the entries are glyphs x tiles, counted without being made
    {
        std::vector<smr_glyph> run(140000, glyph(INT32_MIN, INT32_MIN, INT32_MAX, INT32_MAX));
        for (smr_glyph &g : run) { g.dst_x = -5; g.dst_y = -5; }
        CHECK(tx_entries(7682, 4320, run.data(), 140000) == 140000ull * tx_tiles(7682, 4320));
        std::vector<uint32_t> first(tx_tiles(7682, 4320) + 1);
        CHECK(!tx_plan(7682, 4320, run.data(), 140000, first.data(), nullptr));  // more than 2^32 entries: refused before anything is written
    }
    // random runs on random surfaces, against the brute-force test
    for (int k = 0; k < 300; k++) {
        const int w = 1 + (int)(rnd() % 200), h = 1 + (int)(rnd() % 60);
        std::vector<smr_glyph> run;
        for (uint32_t i = 0, n = rnd() % 40; i < n; i++) {
            const bool wild = rnd() % 8 == 0;
            run.push_back(wild ? glyph((int32_t)((rnd() << 1) | (rnd() & 1u)), (int32_t)(rnd() << 1), (int32_t)(rnd() % 3 ? rnd() : rnd() % 90), (int32_t)(rnd() % 50))
                               : glyph((int)(rnd() % 260) - 40, (int)(rnd() % 100) - 20, (int)(rnd() % 90) - 5, (int)(rnd() % 40) - 3));
        }
        check_plan(w, h, run, true);
    }
}

// ---- the raster cache
static void stats(const smr_renderer *r, uint64_t *calls, uint64_t *launches, uint32_t *resident) { CHECK(smr_renderer_text_stats(r, calls, launches, resident) == 0); }
static uint32_t resident(const smr_renderer *r) {
    uint32_t n = 0;
    stats(r, nullptr, nullptr, &n);
    return n;
}
static uint64_t calls(const smr_renderer *r) {
    uint64_t n = 0;
    stats(r, &n, nullptr, nullptr);
    return n;
}

static std::string scene_of(const std::vector<std::string> &labels, int font_size = 14) {
    std::string s = R"({"type":"view","children":[)";
    for (size_t i = 0; i < labels.size(); i++) {
        if (i) s += ",";
        s += R"({"type":"text","text":")" + labels[i] + R"(","font_size":)" + std::to_string(font_size) + R"(,"width":90,"height":20,"color":"#FFFFFFFF","background_color":"#00204080"})";
    }
    return s + "]}";
}

static long g_steps = 0;

static void cache(uint32_t mode, const char *font_dir) {
    smr_ctx *ctx[2];
    for (auto &c : ctx) CHECK(smr_ctx_create(0, mode, 100, nullptr, &c) == 0);
    smr_renderer *r = nullptr;
    CHECK(smr_renderer_create(ctx[0], -1, &r) == 0);
    CHECK(smr_renderer_add_lane(r, ctx[1]) == 0);
    smr_fontbook *book = nullptr, *other = nullptr;
    CHECK(smr_fontbook_create(&book) == 0 && smr_fontbook_create(&other) == 0);
    CHECK(smr_fontbook_add_dir(book, font_dir) > 0 && smr_fontbook_add_dir(other, font_dir) > 0);
    CHECK(smr_renderer_set_fontbook(r, book) == 0);
    CHECK(smr_renderer_text_stats(nullptr, nullptr, nullptr, nullptr) == SMR_ERR_INVALID && smr_renderer_text_stats(r, nullptr, nullptr, nullptr) == 0);
    int64_t pts = 0;
    auto step = [&](uint32_t want_resident) {
        CHECK(smr_renderer_text_cache_check(r) == 0);
        CHECK(resident(r) == want_resident);
        smr_output_frame out[4];
        uint32_t n = 0;
        CHECK(smr_renderer_render(r, pts, nullptr, 0, out, 4, &n) == 0);
        pts += 40000000;
        g_steps++;
    };
    auto update = [&](const char *output, const std::vector<std::string> &labels, int font_size = 14) {
        CHECK(smr_renderer_update_scene(r, output, 128, 72, SMR_FRAME_RGBA, scene_of(labels, font_size).c_str()) == 0);
    };
    step(0);
    // add: three labels, two alike — two rasters, two rasterise calls
    update("a", {"one", "two", "one"});
    CHECK(calls(r) == 2);
    step(2);
    // the same scene on a second output: nothing new
    update("b", {"one", "two", "one"});
    CHECK(calls(r) == 2);
    step(2);
    // drop a node on one output: "two" stays for the other
    update("a", {"one"});
    step(2);
    // duplicate and add
    update("a", {"one", "one", "one", "three", "two"});
    CHECK(calls(r) == 3);
    step(3);
    // the same text at another size is another key
    update("b", {"one"}, 15);
    CHECK(calls(r) == 4);
    step(4);
    update("b", {"one", "two", "one"});
    CHECK(calls(r) == 4);  // (14 px "one" and "two" were resident on "a")
    step(3);
    // smr_renderer_set_text on a node whose raster is shared (three nodes of "a" and two of "b" show "one"): the node gets its own surface
    {
        const long live = null_device_live_surfaces();
        std::vector<uint8_t> atlas(8 * 8, 200);
        smr_glyph g = glyph(2, 2, 8, 8);
        const float bg[4] = {0, 0, 0, 0};
        int text_node = -1;
        for (int i = 0; i < smr_renderer_node_count(r, "a") && text_node < 0; i++) {
            smr_scene_node info;
            CHECK(smr_renderer_node_info(r, "a", i, &info) == 0);
            if (info.kind == SMR_NODE_TEXT) text_node = i;
        }
        CHECK(text_node >= 0);
        CHECK(smr_renderer_set_text(r, "a", text_node, bg, &g, 1, atlas.data(), 8, 8) == 0);
        CHECK(null_device_live_surfaces() == live + 1);
        step(3);
        const long live_again = null_device_live_surfaces();  // (a lane makes its own node surfaces when it first renders)
        CHECK(smr_renderer_set_text(r, "a", text_node, bg, &g, 1, atlas.data(), 8, 8) == 0);  // again: the same surface is redrawn
        CHECK(null_device_live_surfaces() == live_again);
        step(3);
        // set_text on the ONLY node that shows a raster releases it
        update("a", {"solo", "two"});
        CHECK(calls(r) == 5);
        step(3);  // one, two, solo
        for (int i = 0; i < smr_renderer_node_count(r, "a"); i++) {
            smr_scene_node info;
            CHECK(smr_renderer_node_info(r, "a", i, &info) == 0);
            if (info.kind == SMR_NODE_TEXT && std::string(info.payload) == "solo") CHECK(smr_renderer_set_text(r, "a", i, bg, &g, 1, atlas.data(), 8, 8) == 0);
        }
        step(2);
    }
    // a font-book swap: nothing made with the previous book is found again, and what the replaced scenes showed goes
    {
        const uint64_t before = calls(r);
        CHECK(smr_renderer_set_fontbook(r, other) == 0);
        step(2);  // (the active scenes keep their rasters until they are replaced)
        update("a", {"one", "two"});
        CHECK(calls(r) == before + 2);
        step(4);  // "b" still shows the previous book's one and two
        update("b", {"one", "two", "one"});
        CHECK(calls(r) == before + 2);
        step(2);
        CHECK(smr_renderer_set_fontbook(r, book) == 0);
        update("b", {"two"});
        CHECK(calls(r) == before + 3);
        step(3);
    }
    // without a book Text nodes are the caller's: nothing is borrowed
    CHECK(smr_renderer_set_fontbook(r, nullptr) == 0 && smr_renderer_set_text_measurer(r, smr_fontbook_measure, book) == 0);
    update("b", {"two"});
    step(2);
    CHECK(smr_renderer_set_fontbook(r, book) == 0);
    update("b", {"two", "four"});
    step(4);
    // unregistering both outputs
    CHECK(smr_renderer_unregister_output(r, "a") == 0);
    CHECK(smr_renderer_text_cache_check(r) == 0 && resident(r) == 2);
    CHECK(smr_renderer_unregister_output(r, "b") == 0);
    CHECK(smr_renderer_text_cache_check(r) == 0 && resident(r) == 0);
    // destroyed with rasters resident
    update("z", {"left", "behind"});
    CHECK(resident(r) == 2 && smr_renderer_sync(r) == 0);
    smr_renderer_destroy(r);
    smr_fontbook_destroy(book);
    smr_fontbook_destroy(other);
    for (auto &c : ctx) smr_ctx_destroy(c);
    CHECK(null_device_live_surfaces() == 0);
}

int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: text_bins_driver <font directory>\n"); return 2; }
    plans();
    for (uint32_t mode = 0; mode < 2; mode++) cache(mode, argv[1]);
    printf("{\"plans\": %ld, \"entries\": %ld, \"cache_steps\": %ld, \"checks\": %ld}\n", g_plans, g_entries, g_steps, g_checks);
    return 0;
}
