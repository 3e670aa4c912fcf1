// renderer.cpp — the reference's `Renderer` (smelter-render/src/state.rs:96-252) over the scene engine and the smr_* kernels:
// register inputs / images / built-in shaders, update_scene(output, resolution, format, JSON), render(FrameSet) -> FrameSet.
// Per frame (InnerRenderer::render, state.rs:220-252): populate_inputs (staleness filter, render_loop.rs:19-42), a depth-first
// walk of every output's render graph (render_graph.rs, node.rs:22-181) — input refs, images, text, shader nodes, nested
// layout nodes into RGBA8 node surfaces — and read_outputs (render_loop.rs:59-230) fused into the root layout node's launch.
// SURVEY.md §8 a14 (+ a2, a4); no GPU code here, only calls into the C ABI of this library.
//
// Sharded renderer (smr_renderer_add_shard): inputs are dealt to several contexts, usually one per device.  Per layout node and frame every
// remote input that exactly one texture layout resamples is turned into its dst-sized tile ON ITS OWNER (smr_ingest_resample_batch, one call
// per owner), the tiles travel to the root in one smr_gather_tiles (k_move_rects: one launch per owner) and the root's smr_render_layouts
// samples the tile where a single context would have made it itself — the same bytes.  Whatever does not fit that rule (a 1:1 input, one
// sampled twice, a Shader node's child, the output's root, SMR_MODE_CPU_OPTIMIZED, a resample plan the owner would run on another route than
// the root: owner_takes_the_roots_route below) has its raw planes moved to a root-resident frame by the same gather and is rendered exactly
// as on one context.
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <map>
#include <set>
#include <tuple>

#include "../smr_frame_formats.h"  // (beside smr_internal.h, which needs HIP; this one does not)
#include "scene.h"
#include "shader_program.h"

using namespace smr_host;

// The entry points only a sharded renderer calls are weak references: the host half also links without the GPU half (tests/san runs this file
// against a stand-in device under the sanitizers); smr_renderer_add_shard refuses there.
#pragma weak smr_comm_create_local
#pragma weak smr_comm_destroy
#pragma weak smr_comm_last_error
#pragma weak smr_gather_tiles
#pragma weak smr_ingest_resample_batch
#pragma weak smr_resample_plan_make
extern "C" int smr_ctx_device_index(const smr_ctx *ctx) __attribute__((weak));  // smr_ctx.hip; not part of the ABI
extern "C" uint32_t smr_ctx_drawn_layouts(const smr_ctx *ctx, uint32_t n) __attribute__((weak));  // smr_ctx.hip; not part of the ABI
// The image pass's kernel (k_image_nodes, smr_resample.hip; not part of the ABI): n rescales in one launch per 16.  Without the GPU half the
// pass makes one smr_rescale_bilinear call per job instead.
extern "C" int smr_image_nodes(smr_ctx *ctx, const smr_surface *const *src, smr_surface *const *dst, uint32_t n) __attribute__((weak));
// A WebView node's kernel (k_web_view, smr_layout.hip; not part of the ABI): the page and n children in one launch per 16 children.  Without
// the GPU half nothing is drawn (as everywhere else there).  The page's way to the device — pinned staging, a stream-ordered copy, "is this
// context's stream idle" (smr_ctx.hip; not part of the ABI) — is weak for the same reason: staging is then plain memory and nothing is copied.
extern "C" int smr_web_view(smr_ctx *ctx, const void *page, size_t page_pitch, smr_surface *dst, const smr_surface *const *srcs, const smr_web_rect *rects,
                            uint32_t n, int under) __attribute__((weak));
extern "C" int smr_ctx_stream_idle(smr_ctx *ctx) __attribute__((weak));
// The colour fix-up of new SVG rasters (k_svg_nodes, smr_convert.hip; not part of the ABI): n surfaces in place, one launch per 16.  Without
// the GPU half the rasters keep the pixmap's bytes (nothing is drawn there either).
extern "C" int smr_svg_nodes(smr_ctx *ctx, smr_surface *const *surfaces, uint32_t n) __attribute__((weak));
// New Text rasters (k_text_nodes, smr_text_nodes.hip; not part of the ABI): n runs drawn from one upload by one launch per 16 and one
// synchronisation.  Without the GPU half the renderer makes one smr_blit_glyphs call per run instead.
extern "C" int smr_text_nodes(smr_ctx *ctx, smr_surface *const *targets, const float (*bg)[4], const smr_glyph *const *glyphs, const uint32_t *n_glyphs,
                              const uint8_t *const *atlas_host, const uint32_t *atlas_w, const uint32_t *atlas_h, uint32_t n) __attribute__((weak));
#pragma weak smr_host_alloc
#pragma weak smr_host_free
#pragma weak smr_frame_upload_async

namespace {

// MAX_NODE_RESOLUTION (smelter-render/src/types.rs:146-149)
constexpr uint32_t MAX_NODE_W = 7682, MAX_NODE_H = 4320;

// Host memory that texels go to the device from — a painted page, a rasterised pixmap: tight rows of four bytes a texel.  Pinned where the GPU
// half of the library is linked (smr_host_alloc: an upload is then a stream-ordered copy), plain memory without it.
struct Staging {
    void *host = nullptr;
    size_t bytes = 0;
    bool pinned = false;
    static bool pinnable() { return smr_host_alloc && smr_host_free; }
    // 0, or the status: smr_host_alloc's (c's last error says why), -2 when there is no plain memory
    int alloc(smr_ctx *c, size_t n) {
        if (pinnable()) {
            const int rc = smr_host_alloc(c, n, &host);
            if (rc < 0) return rc;
            pinned = true;
        } else {
            host = malloc(n);
            if (!host) return -2;
        }
        bytes = n;
        return 0;
    }
    void release(smr_ctx *c) {
        if (pinned) smr_host_free(c, host);
        else free(host);
        host = nullptr;
    }
    // Queues the copy into `f`, a frame of one packed plane of these texels, on c: stream-ordered from pinned memory, else smr_surface_upload
    int upload(smr_ctx *c, const smr_frame &f) const {
        if (pinned && smr_frame_upload_async) {
            const void *const planes[3] = {host, nullptr, nullptr};
            return smr_frame_upload_async(c, &f, planes);
        }
        return smr_surface_upload(c, f.planes[0], host, (size_t)f.width * 4);
    }
};

// One registered web renderer instance (transformations/web_renderer/renderer.rs:27-35): the spec, the latest paint (frame_data) in pinned
// staging, the latest rectangles (source_transforms) and, per lane, the page as that lane's context last uploaded it (website_texture).
struct WebStaging {
    Staging mem;                      // w * 4 * h bytes
    std::vector<smr_ctx *> in_flight; // contexts that queued an upload from it and were not seen idle since
};
struct WebLanePage {
    smr_frame page = {};              // SMR_FRAME_BGRA: the bytes as the browser painted them
    smr_ctx *ctx = nullptr;           // the lane's context (what made the frame)
    bool have = false;
    uint64_t gen = 0;                 // the paint it holds
};
struct WebInstance {
    uint32_t w = 0, h = 0, embedding = SMR_WEB_CHROMIUM_EMBEDDING;
    std::vector<WebStaging> staging;
    int latest = -1;                  // the staging buffer of the latest paint; -1 until the first
    uint64_t gen = 0;                 // paints so far
    std::vector<smr_web_rect> rects;
    std::deque<WebLanePage> lanes;    // one per renderer lane, grown on demand
};

struct ImageRes {
    smr_surface *surface = nullptr;  // premultiplied RGBA8 node texture at the image's own resolution (a static image; null for an animated one)
    uint32_t w = 0, h = 0;
    bool opaque = false;             // every pixel's alpha is 255 (seen at registration; premultiplication keeps the alpha byte)
    // AnimatedAsset (animated_image.rs:41-118): one such texture per frame, whether that frame is opaque, and the frames' delays
    std::vector<smr_surface *> frames;
    std::vector<uint8_t> frame_opaque;
    std::vector<uint64_t> delays_ns;
    bool animated() const { return !frames.empty(); }
    // SvgAsset (svg_image.rs:20-118) without the vector library: the caller's rasteriser, and one node texture per node size an active scene
    // shows the asset at — made by smr_renderer_update_scene, shared by every node, output and lane of that size, released when no active
    // scene is left that needs it.  w / h above are SvgAsset::resolution().
    smr_svg_rasterise_fn svg_fn = nullptr;
    void *svg_user = nullptr;
    struct Raster {
        smr_surface *surface = nullptr;
        bool opaque = false;  // every alpha byte of the pixmap was 255 (the fix-up keeps the alpha byte)
    };
    std::map<std::pair<uint32_t, uint32_t>, Raster> rasters;  // by (node width, node height)
    bool svg() const { return svg_fn != nullptr; }
};

// What a Text node's raster depends on (with a font book: smr_renderer_update_scene draws the node itself): TextComponent's fields as
// smr_fontbook_rasterise takes them, the node's size, both colours as the scene's bytes, and which font book — its generation (bumped by
// smr_renderer_set_fontbook) and how many fonts it held when the raster was made.
struct TextKey {
    std::string text, family, style, weight, wrap, align;
    float font_size = 0, line_height = 0;
    uint32_t w = 0, h = 0;
    uint8_t color[4] = {0, 0, 0, 0}, background[4] = {0, 0, 0, 0};
    uint64_t book_generation = 0;
    uint32_t book_fonts = 0;
    auto tie() const {
        return std::tie(w, h, font_size, line_height, book_generation, book_fonts, color[0], color[1], color[2], color[3], background[0], background[1],
                        background[2], background[3], text, family, style, weight, wrap, align);
    }
    bool operator<(const TextKey &o) const { return tie() < o.tie(); }
};
// One resident Text raster: shared by every node, output and lane that shows the key; `refs` counts the (output, node) pairs of ACTIVE scenes
// that point at it, and a raster nobody points at is released once frames in flight are done with it (release_unused_text).
struct TextRaster {
    smr_surface *surface = nullptr;
    uint32_t refs = 0;
};

struct Source {
    uint32_t kind = SMR_SOURCE_NONE;
    const smr_surface *surface = nullptr;
    const smr_frame *frame = nullptr;
    uint32_t w = 0, h = 0;
    uint32_t owner = 0;   // SMR_SOURCE_FRAME: index of the context the frame is resident on (0 = the renderer's own)
    int node = -1;        // ... and the graph node of its InputStream component (the key of its tile / staging slots)
    bool opaque = false;  // every texel's alpha is 255 (the renderer writes its node surfaces itself, so it may know): the compositor then copies
                          // or samples the layer where it would otherwise blend it (SMR_SOURCE_OPAQUE_SURFACE) — the same bytes, fewer of them touched
};

// every YUV-family FrameData variant converts to alpha == 1 (wgpu/format/*_to_rgba.wgsl return vec4(.., 1.0)); BGRA / ARGB / RGBA carry their own
bool frame_opaque(const smr_frame *f) { return f && frame_format_is_opaque_ycbcr(f->format); }

// Does a LayoutNode's output have alpha 255 everywhere?  Yes when one of its layers is opaque — a colour with alpha 1, a texture whose source
// is opaque: bilinear weights are 8-bit fractions and sum to 1 exactly, so an opaque texture samples alpha exactly 1 —, has no rotation, rounded
// corner, border or mask, lies on half-integer coordinates (the coverage arithmetic is then exact) and covers every pixel centre by at least half
// a pixel: its fragment's alpha is exactly 1 there, and whatever is blended above leaves src.a + 1 * (1 - src.a), which stores 255.
// Only the first `drawn` layouts count: the compositor skips what lies beyond the context's max_layouts (smr_render_layouts), and a cover
// in that tail is never drawn.  Conservative: `false` only costs the compositor its shortcut.
bool layouts_leave_an_opaque_surface(const std::vector<smr_layout> &layouts, size_t drawn, const std::vector<Source> &kids, uint32_t w, uint32_t h) {
    auto half_int = [](float v) { return v * 2.0f == std::floor(v * 2.0f) && std::fabs(v) < 32768.0f; };
    for (size_t i = 0; i < layouts.size() && i < drawn; i++) {
        const smr_layout &L = layouts[i];
        if (L.rotation_degrees != 0.0f || L.border_width != 0.0f || L.masks_len != 0) continue;
        if (L.border_radius[0] != 0.0f || L.border_radius[1] != 0.0f || L.border_radius[2] != 0.0f || L.border_radius[3] != 0.0f) continue;
        if (L.type == 1) {
            if (L.color[3] != 1.0f) continue;
        } else if (L.type == 0) {
            if (L.source_index >= kids.size()) continue;
            const Source &k = kids[L.source_index];
            const bool src_opaque = (k.kind == SMR_SOURCE_FRAME && frame_opaque(k.frame)) || (k.kind == SMR_SOURCE_SURFACE && k.opaque);
            if (!src_opaque) continue;
        } else {
            continue;
        }
        if (!(half_int(L.left) && half_int(L.top) && half_int(L.width) && half_int(L.height))) continue;
        if (L.left <= 0.0f && L.top <= 0.0f && L.left + L.width >= (float)w && L.top + L.height >= (float)h) return true;
    }
    return false;
}

// What one frame in flight owns of an output: its two alternating output frames and the per-node intermediate surfaces.
// (One lane = the reference's renderer; with more lanes consecutive frames are enqueued on different contexts / HIP streams
// and overlap on the device, while the scene — and with it every transition — stays one state advanced by one pts sequence.)
// What a remote InputStream node owns of one of the two alternating sets (an owner may resample frame k + 1 while the root composes frame k)
struct ShardSlot {
    smr_surface *tile_src = nullptr;  // the dst-sized tile where the owner resamples it
    smr_ctx *tile_ctx = nullptr;      // ... and the owner's context
    smr_surface *tile_dst = nullptr;  // the same tile on the root
    smr_frame staged = {};            // fallback: a root-resident frame of the input's own format and size
    bool have_staged = false;
};

struct OutputLane {
    std::vector<ShardSlot> shard[2];           // per graph node, sharded renderers only; the set of a frame is the output's `flip`
    smr_frame frames[2];
    bool have_frames = false;
    int flip = 0;
    std::vector<smr_surface *> node_surface;   // per graph node, (re)allocated on size change (NodeTexture::ensure_size)
    std::vector<smr_surface *> scaled_image;   // per graph node: an Image node whose size differs from the image's
    std::vector<uint8_t> image_drawn;          // ... and whether a STATIC image has been drawn into that surface (BitmapNodeState::was_rendered)
    std::vector<Source> image_source;          // per graph node: what the image pass of this frame left for the walk (Image nodes only)
};

struct Output {
    Scene scene;
    uint32_t w = 0, h = 0, format = SMR_FRAME_PLANAR_YUV420;
    std::deque<OutputLane> lanes;              // one per renderer lane, grown on demand (a deque: callers hold pointers to `frames`)
    OutputLane *l = nullptr;                   // the lane of the frame being rendered
    std::vector<smr_surface *> text_surface;   // per graph node: the rendered glyph run of a Text node (read-only per frame) — a cached raster's
                                               // surface, borrowed (text_raster[node] names it), or the node's own (smr_renderer_set_text)
    std::vector<TextRaster *> text_raster;     // per graph node: the cached raster text_surface[node] is borrowed from, or null
};

}  // namespace

struct smr_renderer {
    smr_ctx *ctx = nullptr;           // the context GPU work is issued on: lane_ctx[0] outside smr_renderer_render, the frame's lane inside
    std::vector<smr_ctx *> lane_ctx;  // [0] = the context given to smr_renderer_create, then smr_renderer_add_lane's
    std::vector<smr_ctx *> shard_ctx; // sharded: [0] = lane_ctx[0], then smr_renderer_add_shard's; empty otherwise
    smr_comm *comm = nullptr;         // local communicator over shard_ctx (root = 0), rebuilt when a shard is added
    std::map<std::string, uint32_t> input_owner;  // input_id -> index into shard_ctx (0 while not sharded)
    uint64_t registrations = 0;       // the k of "k-th registered input -> context k mod N"
    uint64_t frame_no = 0;
    int64_t timeout_ns = 500000000;  // stream_fallback_timeout
    std::set<std::string> inputs;
    std::map<std::string, ImageRes> images;
    struct ShaderReg {                // a built-in kernel id, or (hook.launch set) a user shader program: shader_program.h
        uint32_t builtin = 0;
        smr_shader_hook hook;
    };
    std::map<std::string, ShaderReg> shaders;
    smr_text_measure_fn measure = nullptr;    // the caller's text shaper (fitted Text nodes)
    void *measure_user = nullptr;
    smr_fontbook *fontbook = nullptr;         // TextRendererCtx: with a book, Text nodes are measured and drawn here (not owned)
    std::map<std::string, Output> outputs;
    std::string err;
    std::vector<smr_layout> layouts;  // scratch
    uint64_t image_launches = 0;      // smr_renderer_image_launches
    std::map<std::string, WebInstance> web;   // smr_renderer_register_web_renderer
    uint64_t web_launches = 0;        // smr_renderer_web_launches
    uint64_t svg_calls = 0, svg_launches = 0;  // smr_renderer_svg_stats
    std::map<TextKey, TextRaster> text_rasters;    // the Text raster cache (std::map: the nodes' pointers to its values stay valid)
    uint64_t fontbook_generation = 0;              // smr_renderer_set_fontbook calls so far
    uint64_t text_calls = 0, text_launches = 0;    // smr_renderer_text_stats
    size_t lane = 0;                  // the lane of the frame being rendered (index into lane_ctx)
};

namespace {

int fail(smr_renderer *r, int code, const std::string &msg) {
    if (r) r->err = msg;
    return code;
}
int gpu(smr_renderer *r, int rc, const char *what) {
    if (rc >= 0) return rc;
    return fail(r, rc, std::string(what) + ": " + smr_last_error(r->ctx));
}

void free_surfaces(smr_renderer *r, std::vector<smr_surface *> &v) {
    for (smr_surface *s : v)
        if (s) smr_surface_destroy(r->ctx, s);
    v.clear();
}
void sync_lanes(smr_renderer *r) {
    for (smr_ctx *c : r->lane_ctx) smr_sync(c);
    for (size_t i = 1; i < r->shard_ctx.size(); i++) smr_sync(r->shard_ctx[i]);
}
// (callers have synchronised every context: sync_lanes)
void free_shard_slots(smr_renderer *r, OutputLane &l) {
    for (auto &set : l.shard) {
        for (ShardSlot &s : set) {
            if (s.tile_src) smr_surface_destroy(s.tile_ctx, s.tile_src);
            if (s.tile_dst) smr_surface_destroy(r->lane_ctx[0], s.tile_dst);
            if (s.have_staged) smr_frame_destroy(r->lane_ctx[0], &s.staged);
        }
        set.clear();
    }
}
void free_lane_frames(smr_renderer *r, OutputLane &l) {
    if (!l.have_frames) return;
    smr_frame_destroy(r->ctx, &l.frames[0]);
    smr_frame_destroy(r->ctx, &l.frames[1]);
    l.have_frames = false;
}
// per-node surfaces belong to one render graph: dropped (and re-created on demand) when the graph changes
void free_node_surfaces(smr_renderer *r, Output &o) {
    const size_t n = o.scene.nodes().size();
    for (OutputLane &l : o.lanes) {
        free_surfaces(r, l.node_surface);
        free_surfaces(r, l.scaled_image);
        free_shard_slots(r, l);
        l.node_surface.assign(n, nullptr);
        l.scaled_image.assign(n, nullptr);
        l.image_drawn.assign(n, 0);
    }
    // Text: a borrowed raster loses a reference (release_unused_text lets it go when nobody is left), a node's own surface is destroyed
    for (size_t i = 0; i < o.text_surface.size(); i++) {
        if (i < o.text_raster.size() && o.text_raster[i]) o.text_raster[i]->refs--;
        else if (o.text_surface[i]) smr_surface_destroy(r->ctx, o.text_surface[i]);
    }
    o.text_surface.assign(n, nullptr);
    o.text_raster.assign(n, nullptr);
}
void free_output(smr_renderer *r, Output &o) {
    free_node_surfaces(r, o);
    for (OutputLane &l : o.lanes) free_lane_frames(r, l);
}
// the lane's share of an output, created the first time the lane renders it
int enter_lane(smr_renderer *r, Output &o, size_t lane) {
    if (o.lanes.size() <= lane) o.lanes.resize(lane + 1);
    OutputLane &l = o.lanes[lane];
    o.l = &l;
    const size_t n = o.scene.nodes().size();
    if (l.node_surface.size() != n) { l.node_surface.assign(n, nullptr); l.scaled_image.assign(n, nullptr); }
    if (l.image_drawn.size() != n) l.image_drawn.assign(n, 0);
    if (r->shard_ctx.size() > 1 && l.shard[0].size() != n) { l.shard[0].assign(n, ShardSlot()); l.shard[1].assign(n, ShardSlot()); }
    if (!l.have_frames) {
        int rc = gpu(r, smr_frame_create(r->ctx, o.format, o.w, o.h, &l.frames[0]), "output frame");
        if (rc < 0) return rc;
        rc = gpu(r, smr_frame_create(r->ctx, o.format, o.w, o.h, &l.frames[1]), "output frame");
        if (rc < 0) {  // (both or neither: the next attempt starts from nothing)
            smr_frame_destroy(r->ctx, &l.frames[0]);
            return rc;
        }
        l.have_frames = true;
    }
    return 0;
}

// NodeTexture::ensure_size (state/node_texture.rs:22-42)
int ensure_surface(smr_renderer *r, smr_surface *&slot, uint32_t w, uint32_t h, bool *created = nullptr) {
    smr_surface_info info;
    if (created) *created = false;
    if (slot && smr_surface_info_get(slot, &info) == 0 && info.width == w && info.height == h) return 0;
    if (slot) { smr_surface_destroy(r->ctx, slot); slot = nullptr; }
    if (created) *created = true;
    return gpu(r, smr_surface_create(r->ctx, w, h, SMR_PX_RGBA8, &slot), "node surface");
}

// ---- web renderer instances
// (callers have synchronised every context: sync_lanes)
void free_web_instance(smr_renderer *r, WebInstance &wi) {
    for (WebLanePage &lp : wi.lanes)
        if (lp.have) smr_frame_destroy(lp.ctx, &lp.page);
    wi.lanes.clear();
    for (WebStaging &s : wi.staging) s.mem.release(r->lane_ctx[0]);
    wi.staging.clear();
    wi.latest = -1;
}
// A staging buffer no upload can still be reading: the latest one again where it is idle (a host that waits for every frame keeps one
// buffer), another idle one, a new one (up to four), and only then a wait for the oldest upload.
int web_staging_for_paint(smr_renderer *r, WebInstance &wi) {
    for (WebStaging &s : wi.staging) {
        auto &f = s.in_flight;
        for (size_t i = 0; i < f.size();)
            if (!smr_ctx_stream_idle || smr_ctx_stream_idle(f[i]) > 0) f.erase(f.begin() + (ptrdiff_t)i);
            else i++;
    }
    if (wi.latest >= 0 && wi.staging[wi.latest].in_flight.empty()) return wi.latest;
    for (size_t i = 0; i < wi.staging.size(); i++)
        if (wi.staging[i].in_flight.empty()) return (int)i;
    if (wi.staging.size() < 4) {
        WebStaging s;
        const int rc = s.mem.alloc(r->lane_ctx[0], (size_t)wi.w * 4 * wi.h);
        if (rc < 0) return Staging::pinnable() ? gpu(r, rc, "web page staging") : fail(r, -2, "web page staging: out of memory");
        wi.staging.push_back(s);
        return (int)wi.staging.size() - 1;
    }
    const int k = (wi.latest + 1) % (int)wi.staging.size();  // (the one painted longest ago)
    for (smr_ctx *c : wi.staging[k].in_flight) (void)smr_sync(c);
    wi.staging[k].in_flight.clear();
    return k;
}
bool web_instance_in_use(const smr_renderer *r, const std::string &instance_id, const std::string *except_output = nullptr) {
    for (const auto &kv : r->outputs) {
        if (except_output && kv.first == *except_output) continue;
        for (const GraphNode &g : kv.second.scene.nodes())
            if (g.kind == Kind::WebView && g.component->ref_id == instance_id) return true;
    }
    return false;
}

// ---- SVG image assets
bool image_in_use(const smr_renderer *r, const std::string &image_id) {
    for (const auto &kv : r->outputs)
        for (const GraphNode &g : kv.second.scene.nodes())
            if (g.kind == Kind::Image && g.component->ref_id == image_id) return true;
    return false;
}
// (callers have synchronised every context: sync_lanes)
void free_image(smr_renderer *r, ImageRes &img) {
    if (img.surface) smr_surface_destroy(r->lane_ctx[0], img.surface);
    for (smr_surface *f : img.frames) smr_surface_destroy(r->lane_ctx[0], f);
    for (auto &kv : img.rasters) smr_surface_destroy(r->lane_ctx[0], kv.second.surface);
    img.surface = nullptr;
    img.frames.clear();
    img.rasters.clear();
}
// Rasters no active scene of any output shows any more.  (Callers have synchronised every context, as for the Text surfaces of a replaced
// scene: frames in flight may still sample them.)
void release_unused_rasters(smr_renderer *r) {
    std::set<std::pair<std::string, std::pair<uint32_t, uint32_t>>> used;
    for (const auto &kv : r->outputs)
        for (const GraphNode &g : kv.second.scene.nodes())
            if (g.kind == Kind::Image) used.insert({g.component->ref_id, {as_u32(g.component->leaf_size.width), as_u32(g.component->leaf_size.height)}});
    for (auto &kv : r->images) {
        auto &rasters = kv.second.rasters;
        for (auto it = rasters.begin(); it != rasters.end();) {
            if (used.count({kv.first, it->first})) { ++it; continue; }
            smr_surface_destroy(r->lane_ctx[0], it->second.surface);
            it = rasters.erase(it);
        }
    }
}

// ---- the Text raster cache
// Rasters no node of an active scene points at any more.  (Callers have synchronised every context: frames in flight may still sample them.)
void release_unused_text(smr_renderer *r) {
    for (auto it = r->text_rasters.begin(); it != r->text_rasters.end();) {
        if (it->second.refs) { ++it; continue; }
        smr_surface_destroy(r->lane_ctx[0], it->second.surface);
        it = r->text_rasters.erase(it);
    }
}
// Draws n runs into n surfaces on the renderer's own context: ONE smr_text_nodes call (one upload, one launch per 16, one synchronisation;
// every lane's stream may read the surfaces afterwards), or, without the GPU half, one smr_blit_glyphs call per run.
int draw_text_runs(smr_renderer *r, smr_surface *const *targets, const float (*bg)[4], const smr_glyph *const *glyphs, const uint32_t *n_glyphs,
                   const uint8_t *const *atlas, const uint32_t *atlas_w, const uint32_t *atlas_h, uint32_t n) {
    if (!n) return 0;
    smr_ctx *c = r->lane_ctx[0];
    if (smr_text_nodes) {
        const int rc = smr_text_nodes(c, targets, bg, glyphs, n_glyphs, atlas, atlas_w, atlas_h, n);
        if (rc < 0) return fail(r, rc, std::string("text node: ") + smr_last_error(c));
        r->text_launches += (n + 15) / 16;
        return 0;
    }
    for (uint32_t i = 0; i < n; i++) {
        const int rc = smr_blit_glyphs(c, targets[i], bg[i], glyphs[i], n_glyphs[i], atlas[i], atlas_w[i], atlas_h[i]);
        if (rc < 0) return fail(r, rc, std::string("text node: ") + smr_last_error(c));
        r->text_launches++;
    }
    return 0;
}

// One pixmap on its way to a raster: what the rasteriser filled, and the surface it is uploaded into
struct SvgPending {
    std::string id;
    uint32_t w = 0, h = 0;
    Staging mem;           // w * 4 * h bytes, zero-filled before the call
    smr_surface *surface = nullptr;
    bool opaque = false;
};
// The rasters a new render graph needs and no resident one covers (SvgAsset::render_to_texture at the NODE's resolution, svg_image.rs:262-292):
// the caller's rasteriser runs once per (asset, node width, node height), every new pixmap is uploaded into a surface of the node's size,
// the colour fix-up runs in place — one smr_svg_nodes call, i.e. one launch per 16 rasters; none in CPU-optimized mode, where the pixmap's
// bytes are the node's (svg_image.rs:73-76) — and one smr_sync lets the staging go and every lane read.  Anything that fails leaves nothing
// behind: 0, or the status with `err` set.
int make_svg_rasters(smr_renderer *r, const std::vector<GraphNode> &nodes, std::string &err) {
    std::vector<SvgPending> pend;
    int rc = 0;
    for (const GraphNode &g : nodes) {
        if (g.kind != Kind::Image) continue;
        auto it = r->images.find(g.component->ref_id);
        if (it == r->images.end() || !it->second.svg()) continue;
        const ImageRes &img = it->second;
        const uint32_t w = as_u32(g.component->leaf_size.width), h = as_u32(g.component->leaf_size.height);
        if (!w || !h || img.rasters.count({w, h})) continue;  // (a node without texels samples transparent)
        bool queued = false;
        for (const SvgPending &p : pend) queued = queued || (p.id == it->first && p.w == w && p.h == h);
        if (queued) continue;
        const std::string what = "SVG image \"" + it->first + "\" at " + std::to_string(w) + "x" + std::to_string(h);
        if (w > MAX_NODE_W || h > MAX_NODE_H) { err = what + ": the node is above 7682 x 4320 (MAX_NODE_RESOLUTION)"; rc = -1; break; }
        SvgPending p;
        p.id = it->first; p.w = w; p.h = h;
        rc = p.mem.alloc(r->lane_ctx[0], (size_t)w * 4 * h);
        if (rc < 0) { err = what + ": pixmap staging: " + (Staging::pinnable() ? smr_last_error(r->lane_ctx[0]) : "out of memory"); break; }
        memset(p.mem.host, 0, p.mem.bytes);
        pend.push_back(p);
        r->svg_calls++;
        const int answer = img.svg_fn(img.svg_user, p.id.c_str(), w, h, (uint8_t *)p.mem.host, (size_t)w * 4);
        if (answer != 0) { err = what + ": the rasteriser failed (" + std::to_string(answer) + ")"; rc = -1; break; }
    }
    bool queued_work = false;
    std::vector<smr_surface *> fresh;
    for (size_t i = 0; i < pend.size() && rc >= 0; i++) {
        SvgPending &p = pend[i];
        const std::string what = "SVG image \"" + p.id + "\" at " + std::to_string(p.w) + "x" + std::to_string(p.h);
        rc = smr_surface_create(r->lane_ctx[0], p.w, p.h, SMR_PX_RGBA8, &p.surface);
        if (rc < 0) { p.surface = nullptr; err = what + ": raster: " + smr_last_error(r->lane_ctx[0]); break; }
        fresh.push_back(p.surface);
        smr_frame f = {};
        f.format = SMR_FRAME_RGBA; f.width = p.w; f.height = p.h; f.planes[0] = p.surface;
        rc = p.mem.upload(r->lane_ctx[0], f);
        queued_work = true;
        if (rc < 0) { err = what + ": upload: " + smr_last_error(r->lane_ctx[0]); break; }
        const uint8_t *px = (const uint8_t *)p.mem.host;
        p.opaque = true;
        for (size_t k = 0, n = (size_t)p.w * p.h; k < n && p.opaque; k++) p.opaque = px[4 * k + 3] == 255;
    }
    if (rc >= 0 && !fresh.empty() && smr_svg_nodes && smr_ctx_mode(r->lane_ctx[0]) == SMR_MODE_GPU_OPTIMIZED) {
        rc = smr_svg_nodes(r->lane_ctx[0], fresh.data(), (uint32_t)fresh.size());
        if (rc < 0) err = std::string("SVG rasters: ") + smr_last_error(r->lane_ctx[0]);
        else r->svg_launches += (fresh.size() + 15) / 16;
    }
    if (queued_work) {  // (also after a failure: an upload may still read the staging, the fix-up the surfaces)
        const int e = smr_sync(r->lane_ctx[0]);
        if (e < 0 && rc >= 0) { rc = e; err = std::string("SVG rasters: ") + smr_last_error(r->lane_ctx[0]); }
    }
    for (SvgPending &p : pend) p.mem.release(r->lane_ctx[0]);
    if (rc < 0) {
        for (smr_surface *s : fresh) smr_surface_destroy(r->lane_ctx[0], s);
        return rc;
    }
    for (const SvgPending &p : pend) {
        ImageRes::Raster ra;
        ra.surface = p.surface; ra.opaque = p.opaque;
        r->images[p.id].rasters[{p.w, p.h}] = ra;
    }
    return 0;
}

// ---- sharded renderers
bool sharded(const smr_renderer *r) { return r->shard_ctx.size() > 1; }
int shard_gpu(smr_renderer *r, smr_ctx *c, int rc, const char *what) {
    if (rc >= 0) return rc;
    return fail(r, rc, std::string(what) + ": " + smr_last_error(c));
}
struct Gather {  // what one smr_gather_tiles call moves
    std::vector<uint32_t> owner;
    std::vector<const smr_surface *> src;
    std::vector<smr_surface *> dst;
};
int run_gather(smr_renderer *r, Gather &g) {
    if (g.owner.empty()) return 0;
    const int rc = smr_gather_tiles(r->comm, 0, g.owner.data(), g.src.data(), g.dst.data(), (uint32_t)g.owner.size());
    if (rc < 0) return fail(r, rc, std::string("shard gather: ") + smr_comm_last_error(r->comm));
    return 0;
}
// The root-resident stand-in of a remote frame: same format and size, its planes queued on `g`.  `s` then names the stand-in.
int stage_remote_frame(smr_renderer *r, Output &o, Source &s, Gather &g) {
    ShardSlot &slot = o.l->shard[o.l->flip][s.node];
    const smr_frame *f = s.frame;
    // (an input may change its colour matrix from one frame to the next: the planes are the base format's, the stand-in just takes the new tag)
    if (slot.have_staged && frame_base_format(slot.staged.format) == frame_base_format(f->format) && !frame_format_tag_error(f->format)) slot.staged.format = f->format;
    if (slot.have_staged && (slot.staged.format != f->format || slot.staged.width != f->width || slot.staged.height != f->height)) {
        sync_lanes(r);  // (an owner may still be writing it)
        smr_frame_destroy(r->lane_ctx[0], &slot.staged);
        slot.have_staged = false;
    }
    if (!slot.have_staged) {
        int rc = gpu(r, smr_frame_create(r->ctx, f->format, f->width, f->height, &slot.staged), "staged input frame");
        if (rc < 0) return rc;
        slot.have_staged = true;
    }
    for (int p = 0; p < 3; p++) {
        if (!f->planes[p] != !slot.staged.planes[p]) return fail(r, -1, "sharded renderer: a remote input frame does not have the planes of its format");
        if (!f->planes[p]) continue;
        g.owner.push_back(s.owner); g.src.push_back(f->planes[p]); g.dst.push_back(slot.staged.planes[p]);
    }
    s.frame = &slot.staged;
    s.owner = 0;
    return 0;
}
// ... for one frame outside a layout node (a Shader node's child, the output's root): a gather of its own
int localize_frame(smr_renderer *r, Output &o, Source &s) {
    if (!sharded(r) || s.kind != SMR_SOURCE_FRAME || s.owner == 0) return 0;
    Gather g;
    int rc = stage_remote_frame(r, o, s, g);
    if (rc < 0) return rc;
    return run_gather(r, g);
}
int ensure_tile(smr_renderer *r, smr_ctx *ctx, smr_surface *&slot, uint32_t w, uint32_t h) {
    smr_surface_info info;
    if (slot && smr_surface_info_get(slot, &info) == 0 && info.width == w && info.height == h) return 0;
    return shard_gpu(r, ctx, smr_surface_create(ctx, w, h, SMR_PX_RGBA8, &slot), "shard tile");
}
// "The same bytes" holds for a tile only where the owner's smr_ingest_resample_batch runs the plan on the route the root's smr_render_layouts
// would (smr_fused.hip: each walks a cascade of its own).  The cascades agree for a two-pass plan without box pre-reduction of a Y'CbCr
// frame: fused conversion, plane source, RGB12 node, RGBA8 node (a vertical-first plan: the transposed node), the f32 kernel, the general
// passes, in that order in both.  smr_render_layouts has matrix-core routes the batch entry point has not — the one-axis plans (kind 1), the
// box-pre-reduced ones (levels != 0), the alpha builds for frames with an alpha channel: there the owner's tile is the general passes' (the
// oracle's bytes) where the root's is the matrix-core kernel's (within 1 LSB of them), and a byte of the output could differ by one code from
// the single-context renderer's.  Such an input travels as its raw planes.
bool owner_takes_the_roots_route(const smr_frame *f, const smr_resample_plan &p) {
    return frame_opaque(f) && p.kind == 2 && p.levels[0] == 0 && p.levels[1] == 0;
}
// A layout node's remote children, between its layout list (r->layouts) and its smr_render_layouts: tiles where the rule allows, staged
// frames otherwise, ONE gather.  Rewrites r->layouts (crop = the whole tile) and srcs; kids keep describing the inputs themselves.
int shard_layout_sources(smr_renderer *r, Output &o, std::vector<Source> &kids, std::vector<smr_source> &srcs) {
    if (!sharded(r)) return 0;
    const bool resampler = smr_ctx_mode(r->ctx) == SMR_MODE_GPU_OPTIMIZED;  // CpuOptimized has no resampler (layout/layout_renderer.rs:22-27)
    Gather g;
    struct Batch { std::vector<const smr_frame *> in; std::vector<float> crops; std::vector<smr_surface *> dst; };
    std::vector<Batch> batch(r->shard_ctx.size());
    for (size_t k = 0; k < kids.size(); k++) {
        Source &s = kids[k];
        if (s.kind != SMR_SOURCE_FRAME || s.owner == 0) continue;
        int uses = 0;
        smr_layout *L = nullptr;
        for (smr_layout &l : r->layouts)
            if (l.type == 0 && l.source_index == k) { uses++; L = &l; }
        if (uses == 0) { srcs[k].kind = SMR_SOURCE_NONE; srcs[k].frame = nullptr; continue; }  // nothing samples it: nothing to move
        bool tiled = false;
        if (uses == 1 && resampler) {
            // resample_scaled_children (layout.rs:258-261), the rule smr_render_layouts itself applies to a frame source
            const float rw = roundf(L->width), rh = roundf(L->height);
            const uint32_t dw = rw >= 1.0f ? (uint32_t)rw : 1u, dh = rh >= 1.0f ? (uint32_t)rh : 1u;
            smr_resample_plan plan;
            const int kind = smr_resample_plan_make(s.w, s.h, L->crop, dw, dh, &plan);
            if (kind > 0 && dw <= 16384 && dh <= 16384 && owner_takes_the_roots_route(s.frame, plan)) {
                ShardSlot &slot = o.l->shard[o.l->flip][s.node];
                smr_ctx *oc = r->shard_ctx[s.owner];
                smr_surface_info info;
                const bool fits = slot.tile_src && slot.tile_dst && slot.tile_ctx == oc && smr_surface_info_get(slot.tile_src, &info) == 0 &&
                                  info.width == dw && info.height == dh;
                if (!fits) {
                    if (slot.tile_src || slot.tile_dst) {
                        sync_lanes(r);  // (the owner may still be sending the old tile, the root composing from it)
                        if (slot.tile_src) smr_surface_destroy(slot.tile_ctx, slot.tile_src);
                        if (slot.tile_dst) smr_surface_destroy(r->lane_ctx[0], slot.tile_dst);
                        slot.tile_src = slot.tile_dst = nullptr;
                    }
                    slot.tile_ctx = oc;
                    int rc = ensure_tile(r, oc, slot.tile_src, dw, dh);
                    if (rc >= 0) rc = ensure_tile(r, r->ctx, slot.tile_dst, dw, dh);
                    if (rc < 0) return rc;
                }
                Batch &b = batch[s.owner];
                b.in.push_back(s.frame);
                b.crops.insert(b.crops.end(), L->crop, L->crop + 4);
                b.dst.push_back(slot.tile_src);
                g.owner.push_back(s.owner); g.src.push_back(slot.tile_src); g.dst.push_back(slot.tile_dst);
                srcs[k].kind = SMR_SOURCE_OPAQUE_SURFACE;  // (a Y'CbCr frame: owner_takes_the_roots_route)
                srcs[k].surface = slot.tile_dst; srcs[k].frame = nullptr;
                L->crop[0] = 0.0f; L->crop[1] = 0.0f; L->crop[2] = (float)dw; L->crop[3] = (float)dh;
                tiled = true;
            }
        }
        if (!tiled) {
            Source staged = s;
            int rc = stage_remote_frame(r, o, staged, g);
            if (rc < 0) return rc;
            srcs[k].frame = staged.frame;
        }
    }
    for (size_t c = 1; c < batch.size(); c++) {
        Batch &b = batch[c];
        if (b.in.empty()) continue;
        std::vector<int> kinds(b.in.size(), 0);
        int rc = shard_gpu(r, r->shard_ctx[c], smr_ingest_resample_batch(r->shard_ctx[c], b.in.data(), b.crops.data(), b.dst.data(), (uint32_t)b.in.size(), kinds.data()),
                           "shard ingest");
        if (rc < 0) return rc;
        for (int kd : kinds)
            if (kd <= 0) return fail(r, -3, "sharded renderer: a tile's resample plan changed between planning and ingest");
    }
    return run_gather(r, g);
}

struct FrameSetView {
    const smr_input_frame *frames;
    uint32_t n;
    int64_t pts_ns;
};

// RenderNode::render (state/node.rs) for one node of one output; returns what its parent samples
// ShaderParam::to_bytes (shader/node.rs:95-112) over the API form {"type": f32|u32|i32|list|struct, "value": ...}
static void flatten_shader_param(const Json &j, std::vector<uint8_t> &out) {
    const Json *ty = j.get("type"), *v = j.get("value");
    if (!ty || !v) return;
    auto put = [&](const void *p) { const uint8_t *b = (const uint8_t *)p; out.insert(out.end(), b, b + 4); };
    if (ty->str == "f32") { float f = (float)v->num; put(&f); }
    else if (ty->str == "u32") { uint32_t u = as_u32(v->num); put(&u); }
    else if (ty->str == "i32") { int32_t n = as_i32(v->num); put(&n); }
    else if (v->kind == Json::Array) for (const Json &e : v->arr) flatten_shader_param(e, out);
}

// The image pass of one output and frame, before the graph walk.  Every Image node gets its source: the asset itself (a static image) or
// the frame of this pts on the node's own clock (AnimatedAsset::render, animated_image.rs:120-149) where the node has the asset's size;
// otherwise the lane's surface of the node's size, into which the asset is drawn bilinearly (bitmap_image.rs:65-88) — an animated one at
// every render, a static one only until it has been drawn into the surface the lane holds (was_rendered, bitmap_image.rs:71-73).  All the
// drawing of the pass is ONE smr_image_nodes call: one launch per 16 nodes where there was one per node.  An SVG asset's node takes the
// raster smr_renderer_update_scene made for its size and is never drawn here.
int image_pass(smr_renderer *r, Output &o, const FrameSetView &fs) {
    const std::vector<GraphNode> &nodes = o.scene.nodes();
    OutputLane &l = *o.l;
    l.image_source.assign(nodes.size(), Source());
    std::vector<const smr_surface *> src;
    std::vector<smr_surface *> dst;
    std::vector<int> job_node;
    for (int idx = 0; idx < (int)nodes.size(); idx++) {
        if (nodes[idx].kind != Kind::Image) continue;
        const Stateful &c = *nodes[idx].component;
        auto it = r->images.find(c.ref_id);
        if (it == r->images.end()) continue;
        const ImageRes &img = it->second;
        const smr_surface *asset = img.surface;
        bool opaque = img.opaque;
        if (img.animated()) {
            const int k = animated_frame_index(img.delays_ns.data(), (uint32_t)img.delays_ns.size(), fs.pts_ns, c.start_pts_ns);
            if (k < 0 || k >= (int)img.frames.size()) continue;
            asset = img.frames[k];
            opaque = img.frame_opaque[k] != 0;
        }
        const uint32_t w = as_u32(c.leaf_size.width), h = as_u32(c.leaf_size.height);
        Source &out = l.image_source[idx];
        if (img.svg()) {
            // the raster smr_renderer_update_scene made for this node size: never rescaled, never drawn here (no raster: transparent)
            auto ra = img.rasters.find({w, h});
            if (ra != img.rasters.end()) { out.kind = SMR_SOURCE_SURFACE; out.surface = ra->second.surface; out.w = w; out.h = h; out.opaque = ra->second.opaque; }
            continue;
        }
        if (w == img.w && h == img.h) {
            out.kind = SMR_SOURCE_SURFACE; out.surface = asset; out.w = w; out.h = h; out.opaque = opaque;
            continue;
        }
        if (w == 0 || h == 0) continue;
        bool created = false;
        int rc = ensure_surface(r, l.scaled_image[idx], w, h, &created);
        if (created) l.image_drawn[idx] = 0;
        if (rc < 0) return rc;
        if (img.animated() || !l.image_drawn[idx]) { src.push_back(asset); dst.push_back(l.scaled_image[idx]); job_node.push_back(idx); }
        out.kind = SMR_SOURCE_SURFACE; out.surface = l.scaled_image[idx]; out.w = w; out.h = h;
    }
    if (src.empty()) return 0;
    if (smr_image_nodes) {
        int rc = gpu(r, smr_image_nodes(r->ctx, src.data(), dst.data(), (uint32_t)src.size()), "image pass");
        if (rc < 0) return rc;
        r->image_launches += (src.size() + 15) / 16;
    } else {
        for (size_t i = 0; i < src.size(); i++) {
            int rc = gpu(r, smr_rescale_bilinear(r->ctx, src[i], dst[i]), "image node");
            if (rc < 0) return rc;
            r->image_launches++;
        }
    }
    for (int idx : job_node) l.image_drawn[idx] = 1;  // (an animated node is drawn again whatever this says)
    return 0;
}

int render_node(smr_renderer *r, Output &o, int idx, const FrameSetView &fs, Source &out) {
    const GraphNode &g = o.scene.nodes()[idx];
    const Stateful &c = *g.component;
    out = Source();
    switch (g.kind) {
    case Kind::InputStream: {
        // populate_inputs: a registered input with a fresh enough frame, else the node has no texture
        if (!r->inputs.count(c.ref_id)) return 0;
        for (uint32_t i = 0; i < fs.n; i++) {
            const smr_input_frame &f = fs.frames[i];
            if (!f.input_id || !f.frame || c.ref_id != f.input_id) continue;
            const int64_t oldest = fs.pts_ns > r->timeout_ns ? fs.pts_ns - r->timeout_ns : 0;  // Duration::saturating_sub
            if (oldest > f.pts_ns) return 0;
            out.kind = SMR_SOURCE_FRAME; out.frame = f.frame; out.w = f.frame->width; out.h = f.frame->height;
            out.node = idx;
            if (sharded(r)) { auto ow = r->input_owner.find(c.ref_id); out.owner = ow == r->input_owner.end() ? 0u : ow->second; }
            return 0;
        }
        return 0;
    }
    case Kind::Image:
        out = o.l->image_source[idx];  // drawn, where it had to be, by this frame's image pass
        return 0;
    case Kind::Text: {
        if (o.text_surface[idx]) {
            out.kind = SMR_SOURCE_SURFACE; out.surface = o.text_surface[idx];
            out.w = as_u32(c.leaf_size.width); out.h = as_u32(c.leaf_size.height);
        }
        return 0;
    }
    default: break;
    }
    // nodes with children: render them first (depth first, node.rs:167-181)
    std::vector<Source> kids(g.children.size());
    for (size_t k = 0; k < g.children.size(); k++) {
        int rc = render_node(r, o, g.children[k], fs, kids[k]);
        if (rc < 0) return rc;
    }
    if (g.kind == Kind::WebView) {
        // WebRenderer::render (web_renderer/renderer.rs:78-134): without a paint yet the node has no texture; with one, the lane's copy of the
        // page is brought up to the latest paint and the page and the children that have a rectangle are drawn in ONE smr_web_view call
        auto it = r->web.find(c.ref_id);
        if (it == r->web.end()) return fail(r, -1, "Instance of web renderer \"" + c.ref_id + "\" does not exist. You have to register it first before using it in the scene definition.");
        WebInstance &wi = it->second;
        if (wi.latest < 0) return 0;
        int rc = ensure_surface(r, o.l->node_surface[idx], wi.w, wi.h);
        if (rc < 0) return rc;
        if (wi.lanes.size() <= r->lane) wi.lanes.resize(r->lane + 1);
        WebLanePage &lp = wi.lanes[r->lane];
        if (!lp.have) {
            rc = gpu(r, smr_frame_create(r->ctx, SMR_FRAME_BGRA, wi.w, wi.h, &lp.page), "web page");
            if (rc < 0) return rc;
            lp.have = true; lp.ctx = r->ctx; lp.gen = 0;
        }
        if (lp.gen != wi.gen) {
            WebStaging &st = wi.staging[wi.latest];
            if (smr_frame_upload_async) {  // (without the GPU half nothing is copied)
                rc = gpu(r, st.mem.upload(r->ctx, lp.page), "web page upload");
                if (rc < 0) return rc;
                bool known = false;
                for (smr_ctx *q : st.in_flight) known = known || q == r->ctx;
                if (!known) st.in_flight.push_back(r->ctx);
            }
            lp.gen = wi.gen;
        }
        // children zipped with the rectangles (renderer.rs:105-114); Chromium embedding draws the page alone (:128-130)
        const size_t n = wi.embedding == SMR_WEB_CHROMIUM_EMBEDDING ? 0 : std::min(kids.size(), wi.rects.size());
        std::vector<const smr_surface *> srcs(n, nullptr);
        for (size_t k = 0; k < n; k++) {
            if (kids[k].kind == SMR_SOURCE_FRAME) {  // (a Shader node's rule: InputTexture::convert_to_node_texture)
                rc = localize_frame(r, o, kids[k]);
                if (rc < 0) return rc;
                smr_surface *&t = o.l->node_surface[g.children[k]];
                rc = ensure_surface(r, t, kids[k].w, kids[k].h);
                if (rc < 0) return rc;
                rc = gpu(r, smr_frame_to_rgba(r->ctx, kids[k].frame, t), "input node texture");
                if (rc < 0) return rc;
                srcs[k] = t;
            } else if (kids[k].kind == SMR_SOURCE_SURFACE) {
                srcs[k] = kids[k].surface;
            }  // (no texture: the 1 x 1 transparent one — no pixel of the rectangle changes)
        }
        if (smr_web_view) {
            smr_surface_info pi;
            if (smr_surface_info_get(lp.page.planes[0], &pi) != 0) return fail(r, -3, "web page: the lane's copy has no plane");
            rc = gpu(r, smr_web_view(r->ctx, pi.dptr, pi.pitch, o.l->node_surface[idx], srcs.data(), wi.rects.data(), (uint32_t)n,
                                     wi.embedding == SMR_WEB_NATIVE_UNDER_CONTENT ? 1 : 0),
                     "web view node");
            if (rc < 0) return rc;
        }
        r->web_launches += n ? (n + 15) / 16 : 1;
        out.kind = SMR_SOURCE_SURFACE; out.surface = o.l->node_surface[idx]; out.w = wi.w; out.h = wi.h;  // (never known to be opaque)
        return 0;
    }
    if (g.kind == Kind::Shader) {
        auto it = r->shaders.find(c.ref_id);
        if (it == r->shaders.end()) return fail(r, -1, "Shader \"" + c.ref_id + "\" does not exist. You have to register it first before using it in the scene definition.");
        const uint32_t w = as_u32(c.leaf_size.width), h = as_u32(c.leaf_size.height);
        if (w == 0 || h == 0) return 0;
        int rc = ensure_surface(r, o.l->node_surface[idx], w, h);
        if (rc < 0) return rc;
        // shader nodes sample RGBA node textures: raw input frames are converted first (InputTexture::convert_to_node_texture)
        std::vector<const smr_surface *> srcs;
        std::vector<bool> src_opaque;
        for (size_t k = 0; k < kids.size(); k++) {
            if (kids[k].kind == SMR_SOURCE_FRAME) {
                rc = localize_frame(r, o, kids[k]);
                if (rc < 0) return rc;
                smr_surface *&t = o.l->node_surface[g.children[k]];
                rc = ensure_surface(r, t, kids[k].w, kids[k].h);
                if (rc < 0) return rc;
                rc = gpu(r, smr_frame_to_rgba(r->ctx, kids[k].frame, t), "input node texture");
                if (rc < 0) return rc;
                srcs.push_back(t);
                src_opaque.push_back(frame_opaque(kids[k].frame));
            } else if (kids[k].kind == SMR_SOURCE_SURFACE) {
                srcs.push_back(kids[k].surface);
                src_opaque.push_back(kids[k].opaque);
            }
        }
        bool out_opaque = false;
        // the @group(1) uniform: ShaderParam::to_bytes (shader/node.rs:95-112), the values in order, little endian, no padding
        std::vector<uint8_t> params;
        flatten_shader_param(c.shader_param, params);
        const smr_renderer::ShaderReg &reg = it->second;
        if (reg.hook.launch) {
            // a user shader: the same sources, parameter bytes and pts; its output is never known to be opaque
            rc = gpu(r, reg.hook.launch(reg.hook.user, r->ctx, params.data(), params.size(), srcs.data(), (uint32_t)srcs.size(), o.l->node_surface[idx],
                                        (float)((double)fs.pts_ns / 1e9)),
                     "shader node");
            if (rc < 0) return rc;
            out.kind = SMR_SOURCE_SURFACE; out.surface = o.l->node_surface[idx]; out.w = w; out.h = h;
            return 0;
        }
        if (reg.builtin == SMR_SHADER_GAUSSIAN_BLUR) {
            if (srcs.empty()) return 0;  // nothing to sample: the node stays empty
            // the blur kernel maps texel to texel: a source of another size is first brought to the node's resolution
            const smr_surface *src0 = srcs[0];
            smr_surface_info si;
            smr_surface_info_get(src0, &si);
            if (si.width != w || si.height != h) {
                smr_surface *&t = o.l->scaled_image[idx];
                rc = ensure_surface(r, t, w, h);
                if (rc < 0) return rc;
                rc = gpu(r, smr_rescale_bilinear(r->ctx, src0, t), "shader source");
                if (rc < 0) return rc;
                srcs[0] = t;
            } else {
                // The blur of an opaque texture is opaque: both passes accumulate alpha as sum += 1 * w in the very order they accumulate the
                // weights' own sum, so alpha = sum / sum == 1 exactly and the store writes 255 (k_gauss_axis, smr_misc.hip).  (Not claimed
                // through the rescale above: its weights are not 8-bit fractions.)
                out_opaque = src_opaque[0];
            }
            if (params.size() < sizeof(smr_gaussian_blur_params)) params.assign(sizeof(smr_gaussian_blur_params), 0);
        }
        rc = gpu(r, smr_builtin_shader(r->ctx, reg.builtin, params.data(), params.size(), srcs.data(), (uint32_t)srcs.size(), o.l->node_surface[idx],
                                       (float)((double)fs.pts_ns / 1e9)),
                 "shader node");
        if (rc < 0) return rc;
        out.kind = SMR_SOURCE_SURFACE; out.surface = o.l->node_surface[idx]; out.w = w; out.h = h; out.opaque = out_opaque;
        return 0;
    }
    // layout node (nested): LayoutNode::render into an RGBA8 node surface
    std::vector<std::optional<Size>> res(kids.size());
    std::vector<smr_source> srcs(kids.size());
    for (size_t k = 0; k < kids.size(); k++) {
        if (kids[k].kind != SMR_SOURCE_NONE) res[k] = Size{(float)kids[k].w, (float)kids[k].h};
        srcs[k].kind = (kids[k].kind == SMR_SOURCE_SURFACE && kids[k].opaque) ? (uint32_t)SMR_SOURCE_OPAQUE_SURFACE : kids[k].kind;
        srcs[k].surface = kids[k].surface; srcs[k].frame = kids[k].frame;
    }
    uint32_t w = 0, h = 0;
    std::string err;
    if (!o.scene.node_layouts(idx, fs.pts_ns, res, smr_ctx_mode(r->ctx) == SMR_MODE_GPU_OPTIMIZED, r->layouts, w, h, err)) return fail(r, -1, err);
    if (w == 0 || h == 0) return 0;
    // (without the GPU half — tests/san — nothing is drawn at all and the whole list is scanned)
    const size_t drawn = smr_ctx_drawn_layouts ? smr_ctx_drawn_layouts(r->ctx, (uint32_t)r->layouts.size()) : r->layouts.size();
    const bool node_opaque = layouts_leave_an_opaque_surface(r->layouts, drawn, kids, w, h);
    int rc = ensure_surface(r, o.l->node_surface[idx], w, h);
    if (rc < 0) return rc;
    rc = shard_layout_sources(r, o, kids, srcs);
    if (rc < 0) return rc;
    rc = gpu(r, smr_render_layouts(r->ctx, r->layouts.data(), (uint32_t)r->layouts.size(), srcs.data(), (uint32_t)srcs.size(), w, h, nullptr,
                                   o.l->node_surface[idx]),
             "layout node");
    if (rc < 0) return rc;
    out.kind = SMR_SOURCE_SURFACE; out.surface = o.l->node_surface[idx]; out.w = w; out.h = h; out.opaque = node_opaque;
    return 0;
}

int render_output(smr_renderer *r, Output &o, const FrameSetView &fs, const smr_frame **result) {
    o.l->flip ^= 1;
    smr_frame *target = &o.l->frames[o.l->flip];
    *result = target;
    if (o.scene.nodes().empty()) return gpu(r, smr_frame_fill_black(r->ctx, target), "empty output");
    if (int rc = image_pass(r, o, fs); rc < 0) return rc;
    const GraphNode &root = o.scene.nodes()[0];
    if (root.component->is_layout()) {
        std::vector<Source> kids(root.children.size());
        for (size_t k = 0; k < root.children.size(); k++) {
            int rc = render_node(r, o, root.children[k], fs, kids[k]);
            if (rc < 0) return rc;
        }
        std::vector<std::optional<Size>> res(kids.size());
        std::vector<smr_source> srcs(kids.size());
        for (size_t k = 0; k < kids.size(); k++) {
            if (kids[k].kind != SMR_SOURCE_NONE) res[k] = Size{(float)kids[k].w, (float)kids[k].h};
            srcs[k].kind = (kids[k].kind == SMR_SOURCE_SURFACE && kids[k].opaque) ? (uint32_t)SMR_SOURCE_OPAQUE_SURFACE : kids[k].kind;
            srcs[k].surface = kids[k].surface; srcs[k].frame = kids[k].frame;
        }
        uint32_t w = 0, h = 0;
        std::string err;
        if (!o.scene.node_layouts(0, fs.pts_ns, res, smr_ctx_mode(r->ctx) == SMR_MODE_GPU_OPTIMIZED, r->layouts, w, h, err)) return fail(r, -1, err);
        if (w != 0 && h != 0) {
            int rc = shard_layout_sources(r, o, kids, srcs);
            if (rc < 0) return rc;
        }
        if (w == o.w && h == o.h && o.format != SMR_FRAME_RGBA) {
            // LayoutNode::render + read_outputs in one go: the root's RGBA target never exists
            return gpu(r, smr_render_layouts(r->ctx, r->layouts.data(), (uint32_t)r->layouts.size(), srcs.data(), (uint32_t)srcs.size(), w, h,
                                             target, nullptr),
                       "root layout node");
        }
        // a root whose own width/height differ from the output resolution: render the node, then convert like any other root
        if (w == 0 || h == 0) return gpu(r, smr_frame_fill_black(r->ctx, target), "empty output");
        int rc = ensure_surface(r, o.l->node_surface[0], w, h);
        if (rc < 0) return rc;
        rc = gpu(r, smr_render_layouts(r->ctx, r->layouts.data(), (uint32_t)r->layouts.size(), srcs.data(), (uint32_t)srcs.size(), w, h, nullptr,
                                       o.l->node_surface[0]),
                 "root layout node");
        if (rc < 0) return rc;
        smr_surface *&t = o.l->scaled_image[0];
        rc = ensure_surface(r, t, o.w, o.h);
        if (rc < 0) return rc;
        rc = gpu(r, smr_rescale_bilinear(r->ctx, o.l->node_surface[0], t), "root rescale");
        if (rc < 0) return rc;
        return gpu(r, smr_rgba_to_frame(r->ctx, t, target), "output conversion");
    }
    Source s;
    int rc = render_node(r, o, 0, fs, s);
    if (rc < 0) return rc;
    if (s.kind == SMR_SOURCE_NONE) return gpu(r, smr_frame_fill_black(r->ctx, target), "empty output");  // render_loop.rs:127-139
    rc = localize_frame(r, o, s);
    if (rc < 0) return rc;
    const smr_surface *rgba = s.surface;
    if (s.kind == SMR_SOURCE_FRAME) {
        rc = ensure_surface(r, o.l->node_surface[0], s.w, s.h);
        if (rc < 0) return rc;
        rc = gpu(r, smr_frame_to_rgba(r->ctx, s.frame, o.l->node_surface[0]), "input node texture");
        if (rc < 0) return rc;
        rgba = o.l->node_surface[0];
    }
    if (s.w != o.w || s.h != o.h) {  // the output converters sample the root texture over the whole output (rgba_to_yuv.rs:74-117)
        // (a root Image node of its own size was drawn into scaled_image[0] by the image pass: the output-sized copy then takes the other slot)
        smr_surface *&t = rgba == o.l->scaled_image[0] ? o.l->node_surface[0] : o.l->scaled_image[0];
        rc = ensure_surface(r, t, o.w, o.h);
        if (rc < 0) return rc;
        rc = gpu(r, smr_rescale_bilinear(r->ctx, rgba, t), "root rescale");
        if (rc < 0) return rc;
        rgba = t;
    }
    return gpu(r, smr_rgba_to_frame(r->ctx, rgba, target), "output conversion");
}

}  // namespace

// Renderer::register_renderer(Shader) for everything that is not a built-in id (shader_program.cpp); re-registering an id replaces it
int smr_renderer_register_shader_hook(smr_renderer *r, const char *shader_id, const smr_shader_hook &hook) {
    if (!r || !shader_id) return fail(r, -1, "smr_renderer_register_shader: null argument");
    smr_renderer::ShaderReg &reg = r->shaders[shader_id];
    if (reg.hook.release) {
        sync_lanes(r);  // frames in flight may still run the program that goes
        reg.hook.release(reg.hook.user);
    }
    reg.builtin = 0;
    reg.hook = hook;
    return 0;
}
int smr_renderer_fail(smr_renderer *r, int code, const std::string &msg) { return fail(r, code, msg); }
// The Text raster cache's bookkeeping, recounted (tests/san/text_bins_driver.cpp; not exported): 0 when every raster's `refs` is the number
// of (output, node) pairs that point at it, every such pointer is a resident raster whose surface the node shows, and no raster is
// resident without a reference; else -1.
int smr_renderer_text_cache_check(const smr_renderer *r) {
    std::map<const TextRaster *, uint32_t> seen;
    for (const auto &kv : r->text_rasters) {
        if (!kv.second.surface || !kv.second.refs) return -1;
        seen[&kv.second] = 0;
    }
    for (const auto &kv : r->outputs) {
        const Output &o = kv.second;
        if (o.text_raster.size() != o.text_surface.size()) return -1;
        for (size_t i = 0; i < o.text_raster.size(); i++) {
            if (!o.text_raster[i]) continue;
            auto it = seen.find(o.text_raster[i]);
            if (it == seen.end() || o.text_surface[i] != o.text_raster[i]->surface) return -1;
            it->second++;
        }
    }
    for (const auto &kv : seen)
        if (kv.second != kv.first->refs) return -1;
    return 0;
}

extern "C" {

SMR_API int smr_renderer_create(smr_ctx *ctx, int64_t stream_fallback_timeout_ns, smr_renderer **out) {
    if (!ctx || !out) return -1;
    smr_renderer *r = new smr_renderer();
    r->ctx = ctx;
    r->lane_ctx.push_back(ctx);
    if (stream_fallback_timeout_ns >= 0) r->timeout_ns = stream_fallback_timeout_ns;
    r->shaders["gaussian_blur"].builtin = SMR_SHADER_GAUSSIAN_BLUR;
    *out = r;
    return 0;
}

SMR_API void smr_renderer_destroy(smr_renderer *r) {
    if (!r) return;
    sync_lanes(r);
    for (auto &kv : r->outputs) free_output(r, kv.second);
    release_unused_text(r);  // (every output is gone: every Text raster)
    for (auto &kv : r->images) free_image(r, kv.second);  // (resident SVG rasters included)
    for (auto &kv : r->web) free_web_instance(r, kv.second);  // (paints nobody rendered included)
    if (r->comm) smr_comm_destroy(r->comm);
    for (auto &kv : r->shaders)
        if (kv.second.hook.release) kv.second.hook.release(kv.second.hook.user);
    delete r;
}

SMR_API const char *smr_renderer_last_error(const smr_renderer *r) { return r ? r->err.c_str() : "null renderer"; }

SMR_API int smr_renderer_register_input(smr_renderer *r, const char *input_id) {
    if (!r || !input_id) return fail(r, -1, "smr_renderer_register_input: null argument");
    if (r->inputs.insert(input_id).second) {
        const uint64_t k = r->registrations++;
        r->input_owner[input_id] = sharded(r) ? (uint32_t)(k % r->shard_ctx.size()) : 0u;
    }
    return 0;
}
SMR_API int smr_renderer_unregister_input(smr_renderer *r, const char *input_id) {
    if (!r || !input_id) return fail(r, -1, "smr_renderer_unregister_input: null argument");
    r->inputs.erase(input_id);
    r->input_owner.erase(input_id);
    return 0;
}

SMR_API int smr_renderer_register_image(smr_renderer *r, const char *image_id, const uint8_t *rgba, uint32_t width, uint32_t height) {
    if (!r || !image_id || !rgba || !width || !height) return fail(r, -1, "smr_renderer_register_image: null argument");
    if (r->images.count(image_id)) return fail(r, -1, std::string("Failed to register an image. Image \"") + image_id + "\" is already registered.");
    // BitmapAsset: straight-alpha pixels uploaded once, premultiplied into the node texture format (bitmap_image.rs:20-88)
    smr_surface *raw = nullptr, *pm = nullptr;
    int rc = gpu(r, smr_surface_create(r->ctx, width, height, SMR_PX_RGBA8, &raw), "image upload");
    if (rc < 0) return rc;
    rc = gpu(r, smr_surface_upload(r->ctx, raw, rgba, (size_t)width * 4), "image upload");
    if (rc >= 0) rc = gpu(r, smr_surface_create(r->ctx, width, height, SMR_PX_RGBA8, &pm), "image upload");
    if (rc >= 0) rc = gpu(r, smr_add_premultiplied_alpha(r->ctx, raw, pm), "image premultiply");
    if (rc >= 0) rc = gpu(r, smr_sync(r->ctx), "image upload");
    smr_surface_destroy(r->ctx, raw);
    if (rc < 0) {
        if (pm) smr_surface_destroy(r->ctx, pm);
        return rc;
    }
    ImageRes res;
    res.surface = pm; res.w = width; res.h = height;
    res.opaque = true;
    for (size_t i = 0, n = (size_t)width * height; i < n && res.opaque; i++) res.opaque = rgba[4 * i + 3] == 255;
    r->images[image_id] = res;
    for (auto &kv : r->outputs) kv.second.scene.register_image(image_id, (float)width, (float)height);
    return 0;
}

// AnimatedAsset::new (animated_image.rs:41-118) after the decoder: every frame uploaded and premultiplied once, like BitmapAsset's one
SMR_API int smr_renderer_register_animated_image(smr_renderer *r, const char *image_id, const uint8_t *rgba, uint32_t width, uint32_t height,
                                                 uint32_t n_frames, const uint64_t *delays_ns) {
    if (!r || !image_id) return fail(r, -1, "smr_renderer_register_image: null argument");
    if (n_frames == 0) return fail(r, -1, "Animated image does not contain any frames.");
    if (n_frames > 1000) return fail(r, -1, "Detected over 1000 frames inside the animated image. This case is not currently supported.");
    if (n_frames == 1) return smr_renderer_register_image(r, image_id, rgba, width, height);  // AnimatedAsset's SingleFrame fallback
    if (!rgba || !width || !height || !delays_ns) return fail(r, -1, "smr_renderer_register_image: null argument");
    if (r->images.count(image_id)) return fail(r, -1, std::string("Failed to register an image. Image \"") + image_id + "\" is already registered.");
    uint64_t duration = 0;
    for (uint32_t k = 0; k < n_frames; k++) {
        if (delays_ns[k] > (uint64_t)INT64_MAX - duration) return fail(r, -1, "smr_renderer_register_animated_image: the delays add up to more than INT64_MAX ns");
        duration += delays_ns[k];
    }
    ImageRes res;
    res.w = width; res.h = height;
    res.delays_ns.assign(delays_ns, delays_ns + n_frames);
    const size_t frame_px = (size_t)width * height;
    smr_surface *raw = nullptr;
    int rc = gpu(r, smr_surface_create(r->ctx, width, height, SMR_PX_RGBA8, &raw), "image upload");
    for (uint32_t k = 0; k < n_frames && rc >= 0; k++) {
        const uint8_t *px = rgba + 4 * frame_px * k;
        smr_surface *pm = nullptr;
        rc = gpu(r, smr_surface_create(r->ctx, width, height, SMR_PX_RGBA8, &pm), "image upload");
        if (rc < 0) break;
        res.frames.push_back(pm);
        rc = gpu(r, smr_surface_upload(r->ctx, raw, px, (size_t)width * 4), "image upload");
        if (rc >= 0) rc = gpu(r, smr_add_premultiplied_alpha(r->ctx, raw, pm), "image premultiply");
        bool opaque = true;
        for (size_t i = 0; i < frame_px && opaque; i++) opaque = px[4 * i + 3] == 255;
        res.frame_opaque.push_back(opaque ? 1 : 0);
    }
    if (raw) {
        // (also after a failure, before `raw` goes: a premultiply may still read it)
        if (rc >= 0) rc = gpu(r, smr_sync(r->ctx), "image upload");
        else (void)smr_sync(r->ctx);
        smr_surface_destroy(r->ctx, raw);
    }
    if (rc < 0) {
        for (smr_surface *f : res.frames) smr_surface_destroy(r->ctx, f);
        return rc;
    }
    r->images[image_id] = res;
    for (auto &kv : r->outputs) kv.second.scene.register_image(image_id, (float)width, (float)height);
    return 0;
}

SMR_API int smr_renderer_image_launches(const smr_renderer *r, uint64_t *count) {
    if (!r || !count) return -1;
    *count = r->image_launches;
    return 0;
}

// SvgAsset::new after the parser (svg_image.rs:31-94): the tree's size and the way back to the host's rasteriser.  Nothing is rasterised here.
SMR_API int smr_renderer_register_svg_image(smr_renderer *r, const char *image_id, uint32_t width, uint32_t height, smr_svg_rasterise_fn fn, void *user) {
    if (!r || !image_id || !fn || !width || !height) return fail(r, -1, "smr_renderer_register_svg_image: null argument");
    if (r->images.count(image_id)) return fail(r, -1, std::string("Failed to register an image. Image \"") + image_id + "\" is already registered.");
    ImageRes res;
    res.w = width; res.h = height;
    res.svg_fn = fn; res.svg_user = user;
    r->images[image_id] = res;
    for (auto &kv : r->outputs) kv.second.scene.register_image(image_id, (float)width, (float)height);
    return 0;
}

// unregister_renderer(id, RegistryType::Image) (state.rs:154-171), for a static, an animated and an SVG image alike
SMR_API int smr_renderer_unregister_image(smr_renderer *r, const char *image_id) {
    if (!r || !image_id) return fail(r, -1, "smr_renderer_unregister_image: null argument");
    auto it = r->images.find(image_id);
    if (it == r->images.end()) return 0;
    if (image_in_use(r, image_id)) return fail(r, -1, std::string("smr_renderer_unregister_image: a scene uses the image \"") + image_id + "\"");
    sync_lanes(r);  // frames in flight may still sample a scene that was replaced a moment ago
    free_image(r, it->second);
    r->images.erase(it);
    for (auto &kv : r->outputs) kv.second.scene.unregister_image(image_id);
    return 0;
}

SMR_API int smr_renderer_svg_stats(const smr_renderer *r, uint64_t *rasterise_calls, uint64_t *launches, uint32_t *resident) {
    if (!r) return -1;
    if (rasterise_calls) *rasterise_calls = r->svg_calls;
    if (launches) *launches = r->svg_launches;
    if (resident) {
        size_t n = 0;
        for (const auto &kv : r->images) n += kv.second.rasters.size();
        *resident = (uint32_t)n;
    }
    return 0;
}

SMR_API int smr_renderer_text_stats(const smr_renderer *r, uint64_t *rasterise_calls, uint64_t *launches, uint32_t *resident) {
    if (!r) return -1;
    if (rasterise_calls) *rasterise_calls = r->text_calls;
    if (launches) *launches = r->text_launches;
    if (resident) *resident = (uint32_t)r->text_rasters.size();
    return 0;
}

// WebRenderer::new (web_renderer/renderer.rs:43-76) without the browser: the spec's resolution and embedding method
SMR_API int smr_renderer_register_web_renderer(smr_renderer *r, const char *instance_id, uint32_t width, uint32_t height, uint32_t embedding) {
    if (!r || !instance_id) return fail(r, -1, "smr_renderer_register_web_renderer: null argument");
    if (!width || !height) return fail(r, -1, "smr_renderer_register_web_renderer: a web renderer's resolution cannot be zero");
    if (width > MAX_NODE_W || height > MAX_NODE_H) return fail(r, -1, "smr_renderer_register_web_renderer: the resolution is above 7682 x 4320 (MAX_NODE_RESOLUTION)");
    if (embedding > SMR_WEB_NATIVE_UNDER_CONTENT) return fail(r, -1, "smr_renderer_register_web_renderer: unknown embedding method");
    if (r->web.count(instance_id)) return fail(r, -1, std::string("Failed to register a web renderer instance. Instance \"") + instance_id + "\" is already registered.");
    WebInstance &wi = r->web[instance_id];
    wi.w = width; wi.h = height; wi.embedding = embedding;
    for (auto &kv : r->outputs) kv.second.scene.register_web_renderer(instance_id, (float)width, (float)height);
    return 0;
}

SMR_API int smr_renderer_unregister_web_renderer(smr_renderer *r, const char *instance_id) {
    if (!r || !instance_id) return fail(r, -1, "smr_renderer_unregister_web_renderer: null argument");
    auto it = r->web.find(instance_id);
    if (it == r->web.end()) return 0;
    if (web_instance_in_use(r, instance_id)) return fail(r, -1, std::string("smr_renderer_unregister_web_renderer: a scene uses the web renderer instance \"") + instance_id + "\"");
    sync_lanes(r);  // frames in flight may still read the lanes' pages, uploads the staging
    free_web_instance(r, it->second);
    r->web.erase(it);
    for (auto &kv : r->outputs) kv.second.scene.unregister_web_renderer(instance_id);
    return 0;
}

// RenderHandler::on_paint (browser_client.rs:111-130): the bitmap is copied here, uploaded by each lane when it next renders the node
SMR_API int smr_renderer_web_paint(smr_renderer *r, const char *instance_id, const uint8_t *bgra, size_t pitch_bytes) {
    if (!r || !instance_id || !bgra) return fail(r, -1, "smr_renderer_web_paint: null argument");
    auto it = r->web.find(instance_id);
    if (it == r->web.end()) return fail(r, -1, std::string("smr_renderer_web_paint: web renderer instance \"") + instance_id + "\" is not registered");
    WebInstance &wi = it->second;
    const size_t row = (size_t)wi.w * 4;
    if (pitch_bytes == 0) pitch_bytes = row;
    if (pitch_bytes < row) return fail(r, -1, "smr_renderer_web_paint: the pitch is below 4 * width");
    const int k = web_staging_for_paint(r, wi);
    if (k < 0) return k;
    uint8_t *dst = (uint8_t *)wi.staging[k].mem.host;
    if (pitch_bytes == row) memcpy(dst, bgra, row * wi.h);
    else for (uint32_t y = 0; y < wi.h; y++) memcpy(dst + row * y, bgra + pitch_bytes * y, row);
    wi.latest = k;
    wi.gen++;
    return 0;
}

// BrowserClient's GET_FRAME_POSITIONS reply (browser_client.rs:60-93): source_transforms, one rectangle per child
SMR_API int smr_renderer_web_positions(smr_renderer *r, const char *instance_id, const smr_web_rect *rects, uint32_t n) {
    if (!r || !instance_id || (n && !rects)) return fail(r, -1, "smr_renderer_web_positions: null argument");
    auto it = r->web.find(instance_id);
    if (it == r->web.end()) return fail(r, -1, std::string("smr_renderer_web_positions: web renderer instance \"") + instance_id + "\" is not registered");
    it->second.rects.assign(rects, rects + n);
    return 0;
}

SMR_API int smr_renderer_web_launches(const smr_renderer *r, uint64_t *count) {
    if (!r || !count) return -1;
    *count = r->web_launches;
    return 0;
}

SMR_API int smr_renderer_set_text_measurer(smr_renderer *r, smr_text_measure_fn fn, void *user) {
    if (!r) return -1;
    r->measure = fn;
    r->measure_user = user;
    for (auto &kv : r->outputs) kv.second.scene.set_text_measurer(fn, user);
    return 0;
}

SMR_API int smr_renderer_set_fontbook(smr_renderer *r, smr_fontbook *book) {
    if (!r) return -1;
    r->fontbook = book;
    r->fontbook_generation++;  // (Text rasters made with the previous book are no longer found: TextKey)
    r->measure = book ? smr_fontbook_measure : nullptr;
    r->measure_user = book;
    for (auto &kv : r->outputs) kv.second.scene.set_text_measurer(r->measure, r->measure_user);
    return 0;
}

SMR_API int smr_renderer_register_shader(smr_renderer *r, const char *shader_id, uint32_t builtin_id) {
    if (!r || !shader_id) return fail(r, -1, "smr_renderer_register_shader: null argument");
    if (builtin_id > SMR_SHADER_SILLY) return fail(r, -1, "smr_renderer_register_shader: unknown built-in shader (user WGSL is not supported)");
    smr_shader_hook none;
    smr_renderer_register_shader_hook(r, shader_id, none);
    r->shaders[shader_id].builtin = builtin_id;
    return 0;
}

// TextRendererNode::render for one node with the caller's own run (text_renderer.rs:72-167): clear to the background colour, blend the glyph
// run — into a surface of the node's OWN, never a cached raster: a raster the node borrowed so far goes back to the cache (and is released
// when no other node shows it).
static int set_text_run(smr_renderer *r, Output &o, int node, const float bg[4], const smr_glyph *glyphs, uint32_t n, const uint8_t *atlas,
                        uint32_t atlas_w, uint32_t atlas_h) {
    const Stateful &c = *o.scene.nodes()[node].component;
    const uint32_t w = as_u32(c.leaf_size.width), h = as_u32(c.leaf_size.height);
    if (!w || !h) return 0;  // (a zero-sized text node is the 1x1 transparent texture: text_renderer.rs:77-85)
    if (o.text_raster[node]) {
        TextRaster *shared = o.text_raster[node];
        o.text_raster[node] = nullptr;
        o.text_surface[node] = nullptr;
        if (--shared->refs == 0) {
            sync_lanes(r);  // frames in flight may still sample it
            release_unused_text(r);
        }
    }
    int rc = ensure_surface(r, o.text_surface[node], w, h);
    if (rc < 0) return rc;
    // (smr_text_nodes / smr_blit_glyphs return synchronised: every lane's stream reads the run from its next frame on)
    smr_surface *const target = o.text_surface[node];
    const float (*bgs)[4] = (const float (*)[4])bg;
    return draw_text_runs(r, &target, bgs, &glyphs, &n, &atlas, &atlas_w, &atlas_h, 1);
}

// With a font book the renderer is its own TextRendererCtx: every Text node of the new scene is laid out at its resolved size
// (layout_text's final set_size: the node's width, text_renderer.rs:333-343), rasterised and drawn — in TextComponent's colour
// (glyphon::Color::rgba of the straight bytes, text_renderer.rs:176-177) over convert_to_shader_color(background_color) (:62, 371-374) —
// ONCE PER KEY (TextKey), not once per node and update: a node whose raster is resident points at it, every missing key is rasterised once
// however many nodes share it, and all new rasters are drawn by one draw_text_runs call.  (The caller has dropped the replaced scene's
// references, free_node_surfaces, and releases what nobody points at afterwards: a raster both scenes show is simply found again.)
static int draw_text_nodes(smr_renderer *r, Output &o) {
    const auto &nodes = o.scene.nodes();
    struct Pending {
        TextKey key;
        std::vector<int> nodes;
        float bg[4];
        std::vector<smr_glyph> glyphs;  // (a font book's run lives until its next rasterise call: copied)
        std::vector<uint8_t> atlas;
        uint32_t atlas_w = 0, atlas_h = 0;
        smr_surface *surface = nullptr;
    };
    std::vector<Pending> pend;
    const bool srgb = smr_ctx_mode(r->lane_ctx[0]) == SMR_MODE_GPU_OPTIMIZED;
    for (int i = 0; i < (int)nodes.size(); i++) {
        if (nodes[i].kind != Kind::Text) continue;
        const Stateful &c = *nodes[i].component;
        const Stateful::TextSpec &t = c.text_spec;
        TextKey k;
        k.text = c.text; k.family = t.family; k.style = t.style; k.weight = t.weight; k.wrap = t.wrap; k.align = t.align;
        k.font_size = t.font_size; k.line_height = t.line_height;
        k.w = as_u32(c.leaf_size.width); k.h = as_u32(c.leaf_size.height);
        k.color[0] = t.color.r; k.color[1] = t.color.g; k.color[2] = t.color.b; k.color[3] = t.color.a;
        k.background[0] = t.background.r; k.background[1] = t.background.g; k.background[2] = t.background.b; k.background[3] = t.background.a;
        k.book_generation = r->fontbook_generation; k.book_fonts = smr_fontbook_count(r->fontbook);
        if (!k.w || !k.h) continue;  // (a zero-sized text node is the 1x1 transparent texture: text_renderer.rs:77-85)
        auto hit = r->text_rasters.find(k);
        if (hit != r->text_rasters.end()) {
            hit->second.refs++;
            o.text_raster[i] = &hit->second;
            o.text_surface[i] = hit->second.surface;
            continue;
        }
        bool queued = false;
        for (Pending &p : pend)
            if (!queued && !(p.key < k) && !(k < p.key)) { p.nodes.push_back(i); queued = true; }
        if (queued) continue;
        smr_text_params p;
        memset(&p, 0, sizeof(p));
        p.text = c.text.c_str(); p.font_family = t.family.c_str(); p.style = t.style.c_str(); p.weight = t.weight.c_str(); p.wrap = t.wrap.c_str();
        p.align = t.align.c_str();
        p.font_size = t.font_size; p.line_height = t.line_height;
        p.max_width = c.leaf_size.width; p.max_height = c.leaf_size.height;
        const float color[4] = {t.color.r / 255.0f, t.color.g / 255.0f, t.color.b / 255.0f, t.color.a / 255.0f};
        smr_text_run run;
        r->text_calls++;
        if (smr_fontbook_rasterise(r->fontbook, &p, k.w, k.h, color, &run) != 0)
            return fail(r, -1, std::string("text node: ") + smr_fontbook_last_error(r->fontbook));
        pend.emplace_back();
        Pending &q = pend.back();
        q.key = k;
        q.nodes.push_back(i);
        convert_to_shader_color(t.background, srgb, q.bg);
        if (run.n_glyphs) {
            q.glyphs.assign(run.glyphs, run.glyphs + run.n_glyphs);
            q.atlas.assign(run.atlas, run.atlas + (size_t)run.atlas_w * run.atlas_h);
        }
        q.atlas_w = run.atlas_w; q.atlas_h = run.atlas_h;
    }
    // the new rasters' surfaces: what cannot be made leaves its nodes transparent (include/smr.h), the rest is drawn
    int rc = 0;
    std::vector<smr_surface *> targets;
    std::vector<std::array<float, 4>> bgs;
    std::vector<const smr_glyph *> glyphs;
    std::vector<const uint8_t *> atlases;
    std::vector<uint32_t> counts, aw, ah;
    std::vector<Pending *> made;
    for (Pending &q : pend) {
        const int e = gpu(r, smr_surface_create(r->lane_ctx[0], q.key.w, q.key.h, SMR_PX_RGBA8, &q.surface), "text node");
        if (e < 0) { q.surface = nullptr; rc = e; break; }
        made.push_back(&q);
        targets.push_back(q.surface);
        bgs.push_back({q.bg[0], q.bg[1], q.bg[2], q.bg[3]});
        glyphs.push_back(q.glyphs.data()); counts.push_back((uint32_t)q.glyphs.size());
        atlases.push_back(q.atlas.data()); aw.push_back(q.atlas_w); ah.push_back(q.atlas_h);
    }
    const int drawn = draw_text_runs(r, targets.data(), (const float (*)[4])bgs.data(), glyphs.data(), counts.data(), atlases.data(), aw.data(), ah.data(),
                                     (uint32_t)targets.size());
    if (drawn < 0) {  // (nothing of this update's rasters is kept: their nodes render transparent)
        (void)smr_sync(r->lane_ctx[0]);
        for (Pending *q : made) smr_surface_destroy(r->lane_ctx[0], q->surface);
        return drawn;
    }
    for (Pending *q : made) {
        TextRaster &ra = r->text_rasters[q->key];
        ra.surface = q->surface;
        ra.refs = (uint32_t)q->nodes.size();
        for (int i : q->nodes) { o.text_raster[i] = &ra; o.text_surface[i] = ra.surface; }
    }
    return rc;
}

SMR_API int smr_renderer_update_scene(smr_renderer *r, const char *output_id, uint32_t width, uint32_t height, uint32_t output_format,
                                      const char *scene_json) {
    if (!r || !output_id || !scene_json || !width || !height) return fail(r, -1, "smr_renderer_update_scene: null argument");
    if (output_format > 0xffu)  // (the previous scene of this output stays active, as after every refusal here)
        return fail(r, -1, frame_format_tag_error(output_format) ? "smr_renderer_update_scene: output format has bits outside a colour matrix the library knows; and an output format carries no colour matrix at all"
                                                                  : "smr_renderer_update_scene: output format carries a colour matrix: outputs are BT.709, a matrix applies to input frames only");
    if (output_format != SMR_FRAME_PLANAR_YUV420 && output_format != SMR_FRAME_PLANAR_YUV422 && output_format != SMR_FRAME_PLANAR_YUV444 &&
        output_format != SMR_FRAME_NV12 && output_format != SMR_FRAME_RGBA && !frame_format_is_packed_422(output_format))
        return fail(r, -1, frame_format_is_hi_depth(output_format) ? "smr_renderer_update_scene: the 10-bit frame formats are input only; output format must be planar YUV 4:2:0 / 4:2:2 / 4:4:4, NV12, UYVY, YUYV or RGBA"
                                                                   : "smr_renderer_update_scene: output format must be planar YUV 4:2:0 / 4:2:2 / 4:4:4, NV12, UYVY, YUYV or RGBA");
    if (frame_format_is_packed_422(output_format) && width % 2 != 0)
        return fail(r, -1, "smr_renderer_update_scene: " SMR_PACKED_OUTPUT_WIDTH_MSG);
    Output &o = r->outputs[output_id];
    for (auto &kv : r->images) o.scene.register_image(kv.first, (float)kv.second.w, (float)kv.second.h);
    for (auto &kv : r->web) o.scene.register_web_renderer(kv.first, (float)kv.second.w, (float)kv.second.h);
    o.scene.set_text_measurer(r->measure, r->measure_user);
    std::string err;
    {
        // Shader ids are resolved while the new scene is built (ShaderComponent::stateful_component, shader_component.rs:44-52):
        // an unknown id is SceneError::ShaderNotFound and the previous scene stays.  So: convert the definition without
        // touching the active scene (Scene::parse), look the ids up, and only then update.
        std::string converted;
        if (!o.scene.parse(scene_json, converted, err)) {
            if (o.w == 0) r->outputs.erase(output_id);  // a failed first update leaves no output behind
            return fail(r, -1, err);
        }
        Json tree;
        JsonParser jp(converted);
        std::string missing, text_err;
        const bool have_tree = jp.parse(tree, err);
        if (have_tree) {
            // validate_web_renderer_ids_uniqueness (scene/validation.rs:74-99) over the scenes of ALL outputs with this one replaced: a web
            // renderer instance serves one component at a time.  It runs before the stateful tree is built (state.rs:177-189), so before
            // the lookups below.
            std::vector<std::string> web;
            std::string twice;
            collect_web_instances(tree, web);
            const std::string this_output = output_id;
            if (!first_repeated(web, twice))
                for (const std::string &id : web)
                    if (twice.empty() && web_instance_in_use(r, id, &this_output)) twice = id;
            if (!twice.empty()) {
                if (o.w == 0) r->outputs.erase(output_id);
                return fail(r, -1, web_renderer_not_exclusive(twice));
            }
        }
        if (have_tree) {
            std::vector<const Json *> stack{&tree};
            while (!stack.empty() && missing.empty() && text_err.empty()) {
                const Json *j = stack.back();
                stack.pop_back();
                for (const Json &a : j->arr) stack.push_back(&a);
                for (const auto &kv : j->obj) stack.push_back(&kv.second);
                const Json *type = j->get("type"), *sid = j->get("shader_id");
                if (type && sid && type->str == "Shader" && !r->shaders.count(sid->str)) missing = sid->str;
                // The renderer draws its Text nodes itself (smr_renderer_set_fontbook) once the new scene is in place; what can make that fail for
                // reasons the scene carries — an empty font book, text that is not UTF-8, sizes no run can have — is found HERE, while the previous
                // scene is still the active one (the reference fails an update as a whole: state.rs:177-189).  smr_fontbook_measure runs
                // the rasteriser's own checks (text.cpp: measure / rasterise share sane_sizes, the font match and the decoder).
                if (type && type->str == "Text" && r->fontbook) {
                    auto str = [&](const char *k) { const Json *v = j->get(k); return v ? v->str : std::string(); };
                    auto num = [&](const char *k, double d) { const Json *v = j->get(k); return v ? v->num : d; };
                    const std::string text = str("text"), family = str("font_family"), style = str("style"), weight = str("weight"), wrap = str("wrap");
                    smr_text_params p;
                    memset(&p, 0, sizeof(p));
                    p.text = text.c_str(); p.font_family = family.c_str(); p.style = style.c_str(); p.weight = weight.c_str(); p.wrap = wrap.c_str();
                    p.align = "Left";
                    p.font_size = (float)num("font_size", 0.0); p.line_height = (float)num("line_height", num("font_size", 0.0));
                    p.max_width = 7682.0f; p.max_height = 4320.0f;
                    float widest = 0.0f;
                    uint32_t lines = 0;
                    if (smr_fontbook_measure(r->fontbook, &p, &widest, &lines) != 0) text_err = std::string("text node: ") + smr_fontbook_last_error(r->fontbook);
                }
            }
        }
        if (!missing.empty()) {
            if (o.w == 0) r->outputs.erase(output_id);
            return fail(r, -1, "Shader \"" + missing + "\" does not exist. You have to register it first before using it in the scene definition.");
        }
        if (!text_err.empty()) {
            if (o.w == 0) r->outputs.erase(output_id);
            return fail(r, -1, text_err);
        }
    }
    // SVG assets are rasterised at the sizes the NEW graph shows them at — on this thread, once everything about the definition has been
    // validated and before the graph replaces the active one: a rasteriser (or a raster's allocation) that fails refuses the update as a whole.
    int svg_rc = 0;
    const Scene::BeforeCommit rasterise = [&](const std::vector<GraphNode> &new_nodes, std::string &why) {
        svg_rc = make_svg_rasters(r, new_nodes, why);
        return svg_rc >= 0;
    };
    if (!o.scene.update(scene_json, width, height, err, rasterise)) {
        if (o.w == 0) r->outputs.erase(output_id);  // a failed first update leaves no output behind
        return fail(r, svg_rc < 0 ? svg_rc : -1, err);
    }
    // frames in flight read the surfaces dropped below
    sync_lanes(r);
    if (o.w != width || o.h != height || o.format != output_format)
        for (OutputLane &l : o.lanes) free_lane_frames(r, l);  // re-created at the new geometry when the lane next renders
    o.w = width; o.h = height; o.format = output_format;
    // node indices belong to the new graph: per-node surfaces are re-created on demand, text runs must be supplied again
    free_node_surfaces(r, o);
    release_unused_rasters(r);  // (the replaced scene's SVG rasters, where no output shows them any more)
    int rc = enter_lane(r, o, 0);  // the output's first frames exist after a successful update, as before
    // (what is left to fail below is a device allocation — the frames, a text node's surface: SMR_ERR_OOM with the NEW scene active and the
    //  nodes that could not be drawn transparent; include/smr.h says so.  Everything the scene itself can get wrong was refused above.)
    // (Text rasters: the new scene's are found or made first, then those only the replaced scene showed go — every context is idle since
    //  sync_lanes above, and smr_text_nodes returns synchronised)
    if (rc >= 0 && r->fontbook) rc = draw_text_nodes(r, o);
    release_unused_text(r);
    return rc;
}

SMR_API int smr_renderer_unregister_output(smr_renderer *r, const char *output_id) {
    if (!r || !output_id) return fail(r, -1, "smr_renderer_unregister_output: null argument");
    auto it = r->outputs.find(output_id);
    if (it == r->outputs.end()) return 0;
    sync_lanes(r);
    free_output(r, it->second);
    r->outputs.erase(it);
    release_unused_rasters(r);
    release_unused_text(r);
    return 0;
}

SMR_API int smr_renderer_node_count(const smr_renderer *r, const char *output_id) {
    if (!r || !output_id) return -1;
    auto it = r->outputs.find(output_id);
    return it == r->outputs.end() ? -1 : (int)it->second.scene.nodes().size();
}

SMR_API int smr_renderer_node_info(smr_renderer *r, const char *output_id, int node, smr_scene_node *out) {
    if (!r || !output_id || !out) return fail(r, -1, "smr_renderer_node_info: null argument");
    auto it = r->outputs.find(output_id);
    if (it == r->outputs.end()) return fail(r, -1, "smr_renderer_node_info: unknown output");
    const auto &nodes = it->second.scene.nodes();
    if (node < 0 || node >= (int)nodes.size()) return fail(r, -1, "smr_renderer_node_info: node index out of range");
    const GraphNode &g = nodes[node];
    const Stateful &c = *g.component;
    memset(out, 0, sizeof(*out));
    out->kind = g.kind == Kind::InputStream ? SMR_NODE_INPUT_STREAM : g.kind == Kind::Text ? SMR_NODE_TEXT : g.kind == Kind::Image ? SMR_NODE_IMAGE
              : g.kind == Kind::Shader ? SMR_NODE_SHADER : g.kind == Kind::WebView ? SMR_NODE_WEB_VIEW : SMR_NODE_LAYOUT;
    out->parent = g.parent;
    out->n_children = (uint32_t)g.children.size();
    const Size sz = g.has_forced_size ? g.forced_size : c.leaf_size;
    out->width = as_u32(sz.width); out->height = as_u32(sz.height);
    out->ref_id = c.ref_id.c_str(); out->id = c.id.c_str();
    out->payload = c.kind == Kind::Text ? c.text.c_str() : "";
    return 0;
}

SMR_API int smr_renderer_set_text(smr_renderer *r, const char *output_id, int node, const float bg[4], const smr_glyph *glyphs, uint32_t n,
                                  const uint8_t *atlas, uint32_t atlas_w, uint32_t atlas_h) {
    if (!r || !output_id || !bg) return fail(r, -1, "smr_renderer_set_text: null argument");
    auto it = r->outputs.find(output_id);
    if (it == r->outputs.end()) return fail(r, -1, "smr_renderer_set_text: unknown output");
    Output &o = it->second;
    if (node < 0 || node >= (int)o.scene.nodes().size() || o.scene.nodes()[node].kind != Kind::Text)
        return fail(r, -1, "smr_renderer_set_text: not a text node");
    return set_text_run(r, o, node, bg, glyphs, n, atlas, atlas_w, atlas_h);
}

SMR_API int smr_renderer_render(smr_renderer *r, int64_t pts_ns, const smr_input_frame *inputs, uint32_t n_inputs, smr_output_frame *outputs,
                                uint32_t cap, uint32_t *n_outputs) {
    if (!r || (n_inputs && !inputs) || !n_outputs) return fail(r, -1, "smr_renderer_render: null argument");
    FrameSetView fs{inputs, n_inputs, pts_ns};
    // consecutive frames rotate through the lanes: this frame's GPU work goes to its lane's context (stream, scratch) and
    // into the lane's own output frames and node surfaces; the scene state is shared and advances with pts as ever
    const size_t lane = (size_t)(r->frame_no++ % r->lane_ctx.size());
    smr_ctx *base = r->ctx;
    r->ctx = r->lane_ctx[lane];
    r->lane = lane;
    uint32_t k = 0;
    int rc = 0;
    for (auto &kv : r->outputs) {
        const smr_frame *frame = nullptr;
        rc = enter_lane(r, kv.second, lane);
        if (rc >= 0) rc = render_output(r, kv.second, fs, &frame);
        if (rc < 0) break;
        if (k < cap && outputs) { outputs[k].output_id = kv.first.c_str(); outputs[k].frame = frame; outputs[k].ctx = r->ctx; }
        k++;
    }
    r->ctx = base;
    if (rc < 0) return rc;
    *n_outputs = k;
    return 0;
}

SMR_API int smr_renderer_add_lane(smr_renderer *r, smr_ctx *ctx) {
    if (!r || !ctx) return fail(r, -1, "smr_renderer_add_lane: null argument");
    for (smr_ctx *c : r->lane_ctx)
        if (c == ctx) return fail(r, -1, "smr_renderer_add_lane: this context is a lane already");
    if (smr_ctx_mode(ctx) != smr_ctx_mode(r->ctx)) return fail(r, -1, "smr_renderer_add_lane: the lane's context has another rendering mode");
    if (sharded(r)) return fail(r, -1, "smr_renderer_add_lane: this renderer has shards; lanes and shards do not combine");
    r->lane_ctx.push_back(ctx);
    // frames in flight: every lane's kernels run beside another lane's from now on
    for (smr_ctx *c : r->lane_ctx) (void)smr_ctx_set_option(c, SMR_OPT_SHARED_DEVICE, 1);
    return 0;
}

SMR_API int smr_renderer_add_shard(smr_renderer *r, smr_ctx *ctx) {
    if (!r || !ctx) return fail(r, -1, "smr_renderer_add_shard: null argument");
    if (!smr_comm_create_local || !smr_comm_destroy || !smr_comm_last_error || !smr_gather_tiles || !smr_ingest_resample_batch || !smr_resample_plan_make)
        return fail(r, -1, "smr_renderer_add_shard: this build of the renderer has no device half");
    if (r->lane_ctx.size() > 1) return fail(r, -1, "smr_renderer_add_shard: this renderer has lanes; lanes and shards do not combine");
    if (r->registrations) return fail(r, -1, "smr_renderer_add_shard: call it before the first smr_renderer_register_input");
    if (ctx == r->lane_ctx[0]) return fail(r, -1, "smr_renderer_add_shard: this context is the renderer's own");
    for (smr_ctx *c : r->shard_ctx)
        if (c == ctx) return fail(r, -1, "smr_renderer_add_shard: this context is a shard already");
    if (smr_ctx_mode(ctx) != smr_ctx_mode(r->ctx)) return fail(r, -1, "smr_renderer_add_shard: the shard's context has another rendering mode");
    std::vector<smr_ctx *> all = r->shard_ctx;
    if (all.empty()) all.push_back(r->lane_ctx[0]);
    all.push_back(ctx);
    smr_comm *comm = nullptr;
    const int rc = smr_comm_create_local(all.data(), (uint32_t)all.size(), &comm);
    if (rc < 0) {
        const char *a = smr_last_error(ctx), *b = smr_last_error(r->ctx);
        return fail(r, rc, std::string("smr_renderer_add_shard: ") + (a && *a ? a : b && *b ? b : "the contexts cannot form a local communicator"));
    }
    sync_lanes(r);  // (outputs rendered so far: their per-node sets gain the shard slots at the next frame)
    if (r->comm) smr_comm_destroy(r->comm);
    r->comm = comm;
    r->shard_ctx = all;
    // contexts that share the root's device run their kernels beside the root's from now on (as smr_renderer_add_lane's do)
    if (smr_ctx_device_index) {
        const int root_dev = smr_ctx_device_index(r->lane_ctx[0]);
        bool shared = false;
        for (size_t i = 1; i < all.size(); i++)
            if (smr_ctx_device_index(all[i]) == root_dev) { (void)smr_ctx_set_option(all[i], SMR_OPT_SHARED_DEVICE, 1); shared = true; }
        if (shared) (void)smr_ctx_set_option(r->lane_ctx[0], SMR_OPT_SHARED_DEVICE, 1);
    }
    return 0;
}

SMR_API int smr_renderer_input_ctx(smr_renderer *r, const char *input_id, smr_ctx **out) {
    if (!r || !input_id || !out) return fail(r, -1, "smr_renderer_input_ctx: null argument");
    *out = nullptr;
    auto it = r->input_owner.find(input_id);
    if (it == r->input_owner.end()) return fail(r, -1, std::string("smr_renderer_input_ctx: input \"") + input_id + "\" is not registered");
    *out = sharded(r) ? r->shard_ctx[it->second] : r->lane_ctx[0];
    return 0;
}

SMR_API int smr_renderer_sync(smr_renderer *r) {
    if (!r) return -1;
    int rc = 0;
    for (smr_ctx *c : r->lane_ctx) {
        const int e = smr_sync(c);
        if (e < 0 && rc >= 0) rc = gpu(r, e, "sync");
    }
    for (size_t i = 1; i < r->shard_ctx.size(); i++) {
        const int e = smr_sync(r->shard_ctx[i]);
        if (e < 0 && rc >= 0) rc = shard_gpu(r, r->shard_ctx[i], e, "sync");
    }
    return rc;
}

}  // extern "C"
