// smr_text_nodes.hip — smr_text_nodes: the launcher of k_text_nodes (smr_text_nodes.h), the renderer's way to draw all new Text rasters of
// one scene update (host/renderer.cpp; exported, not part of smr.h).
#define SMR_TEXT_NODES_KERNEL 1
#include "smr_text_nodes.h"
#include "host/text_bins.h"

static_assert(SMR_TEXT_TILE_W == SMR_NODE_TILE_W && SMR_TEXT_TILE_H == SMR_NODE_TILE_H, "tx_plan bins by the tiles the kernel walks");

namespace {

constexpr size_t TEXT_BLOCK_LIMIT = (size_t)64 << 20;  // the pinned block of one smr_text_nodes call
constexpr int TEXT_SCRATCH_SLOT = 4;
inline uint64_t up256(uint64_t v) { return (v + 255) & ~(uint64_t)255; }

}  // namespace

extern "C" {

// Up to n Text rasters (host/renderer.cpp; not part of smr.h): targets[i] is cleared to bg[i] and glyphs[i][0 .. n_glyphs[i]) are blended over
// it from the A8 atlas atlas_host[i], as n smr_blit_glyphs calls would — the same bytes — but from ONE pinned block holding every job's
// records, tile bins (host/text_bins.h) and atlas, ONE stream-ordered copy of it, one k_text_nodes launch per 16 jobs and ONE
// hipStreamSynchronize.  The block is the context's and grows on demand; a job that would push it past `limit` bytes (a hostile run of
// full-node quads: its bins are glyphs x tiles) is drawn by smr_blit_glyphs instead.  smr_text_nodes is the entry; _limit lets a test lower
// the limit.
__attribute__((visibility("default"))) int smr_text_nodes_limit(smr_ctx *ctx, smr_surface *const *targets, const float (*bg)[4], const smr_glyph *const *glyphs,
                                                                const uint32_t *n_glyphs, const uint8_t *const *atlas_host, const uint32_t *atlas_w,
                                                                const uint32_t *atlas_h, uint32_t n, size_t limit) {
    SMR_ENTER(ctx);
    if (!ctx || (n && (!targets || !bg || !glyphs || !n_glyphs || !atlas_host || !atlas_w || !atlas_h))) return SMR_ERR_INVALID;
    for (u32 i = 0; i < n; i++) {
        if (!targets[i] || (n_glyphs[i] && (!glyphs[i] || !atlas_host[i]))) return smr_fail(ctx, SMR_ERR_INVALID, "smr_text_nodes: entry %u lacks a target, its glyphs or its atlas", i);
        if (targets[i]->fmt != SMR_PX_RGBA8) return smr_fail(ctx, SMR_ERR_INVALID, "smr_text_nodes: target must be RGBA8");
        if (const int rc = tx_check_glyphs(ctx, "smr_text_nodes", glyphs[i], n_glyphs[i], atlas_w[i], atlas_h[i])) return rc;
        for (u32 k = 0; k < i; k++)
            if (targets[k] == targets[i]) return smr_fail(ctx, SMR_ERR_INVALID, "smr_text_nodes: entry %u repeats entry %u (every texel is written once)", i, k);
    }
    // where job i's parts lie in the block; a job without a texel has none, a job that does not fit goes the old way
    struct Part {
        size_t rec = 0, first = 0, bin = 0, atlas = 0;
        u32 tiles = 0;
    };
    std::vector<Part> part(n);
    std::vector<u32> batched, single;
    uint64_t total = 0;
    for (u32 i = 0; i < n; i++) {
        const smr_surface *t = targets[i];
        if (!t->ptr || !t->w || !t->h) continue;
        const u32 ng = n_glyphs[i];
        Part &P = part[i];
        P.tiles = tx_tiles((int)t->w, (int)t->h);
        const uint64_t rec = up256((uint64_t)ng * sizeof(TextGlyph)), first = up256(((uint64_t)P.tiles + 1) * 4);
        const uint64_t bin = up256(tx_entries((int)t->w, (int)t->h, glyphs[i], ng) * 4), atlas = ng ? up256((uint64_t)atlas_w[i] * atlas_h[i]) : 0;
        if (bin > limit || total + rec + first + bin + atlas > limit) { single.push_back(i); continue; }
        P.rec = (size_t)total; P.first = P.rec + (size_t)rec; P.bin = P.first + (size_t)first; P.atlas = P.bin + (size_t)bin;
        total += rec + first + bin + atlas;
        batched.push_back(i);
    }
    if (!batched.empty()) {
        if (ctx->text_host_bytes < total) {
            if (ctx->text_host) smr_host_free(ctx, ctx->text_host);  // (no copy is in flight: every call ends synchronised)
            ctx->text_host = nullptr; ctx->text_host_bytes = 0;
            const size_t want = ((size_t)total + ((size_t)1 << 20) - 1) & ~(((size_t)1 << 20) - 1);
            if (const int rc = smr_host_alloc(ctx, want, &ctx->text_host)) return rc;
            ctx->text_host_bytes = want;
        }
        u8 *host = (u8 *)ctx->text_host;
        u8 *dev = (u8 *)smr_scratch(ctx, TEXT_SCRATCH_SLOT, (size_t)total);
        if (!dev) return SMR_ERR_OOM;
        for (u32 i : batched) {
            const Part &P = part[i];
            const smr_surface *t = targets[i];
            const u32 ng = n_glyphs[i];
            TextGlyph *rec = (TextGlyph *)(host + P.rec);
            for (u32 k = 0; k < ng; k++) {
                const smr_glyph &g = glyphs[i][k];
                float c[3];
                tx_glyph_colour(ctx->srgb(), g, c);
                rec[k] = TextGlyph{g.dst_x, g.dst_y, g.w, g.h, g.atlas_x, g.atlas_y, c[0], c[1], c[2], g.color[3]};
            }
            if (!tx_plan((int)t->w, (int)t->h, glyphs[i], ng, (u32 *)(host + P.first), (u32 *)(host + P.bin))) return smr_fail(ctx, SMR_ERR_INTERNAL, "smr_text_nodes: bins of entry %u", i);
            if (ng) memcpy(host + P.atlas, atlas_host[i], (size_t)atlas_w[i] * atlas_h[i]);
        }
        SMR_HIP(ctx, hipMemcpyAsync(dev, host, (size_t)total, hipMemcpyHostToDevice, ctx->stream));
        const u32 srgb = ctx->srgb() ? 1u : 0u;
        const int rc = nt_launch_batches<TextBatch>(ctx, k_text_nodes, (u32)batched.size(),
            [&](TextJob &J, u32 k) {
                const u32 i = batched[k];
                const Part &P = part[i];
                J.dst = view_of(targets[i]);
                for (int c = 0; c < 4; c++) J.bg[c] = bg[i][c];
                J.glyphs = (const TextGlyph *)(dev + P.rec); J.bin_first = (const u32 *)(dev + P.first); J.bin_glyph = (const u32 *)(dev + P.bin);
                J.atlas = dev + P.atlas; J.atlas_w = atlas_w[i];
            },
            [&](TextBatch &B) { B.srgb = srgb; return tx_batch_plan(B); });
        const hipError_t e = hipStreamSynchronize(ctx->stream);  // (also after a failed launch: the copy reads the block, kernels the scratch)
        if (rc < 0) return rc;
        SMR_HIP(ctx, e);
    }
    for (u32 i : single)
        if (const int rc = smr_blit_glyphs(ctx, targets[i], bg[i], glyphs[i], n_glyphs[i], atlas_host[i], atlas_w[i], atlas_h[i])) return rc;
    return SMR_OK;
}

__attribute__((visibility("default"))) int smr_text_nodes(smr_ctx *ctx, smr_surface *const *targets, const float (*bg)[4], const smr_glyph *const *glyphs,
                                                          const uint32_t *n_glyphs, const uint8_t *const *atlas_host, const uint32_t *atlas_w,
                                                          const uint32_t *atlas_h, uint32_t n) {
    return smr_text_nodes_limit(ctx, targets, bg, glyphs, n_glyphs, atlas_host, atlas_w, atlas_h, n, TEXT_BLOCK_LIMIT);
}

}  // extern "C"
