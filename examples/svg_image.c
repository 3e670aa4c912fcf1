/* svg_image.c — an SVG image asset from plain C: the vector library is the caller's, everything after the pixmap exists is the library's
 * (include/smr.h, "SVG image assets").
 *
 *   gcc -std=c11 -Iinclude examples/svg_image.c -o svg_image -Lsmelter_amd -l:libsmr_hip.so -Wl,-rpath,$PWD/smelter_amd -lm
 *   ./svg_image out.rgba        # the same scene at two Image sizes; the last frame (400x400 RGBA) is written to out.rgba
 *
 * The "rasteriser" below draws an anti-aliased disc analytically at whatever size it is asked for: it shows the contract without a vector
 * library.  A host that owns resvg wraps resvg::render(&tree, Transform::from_scale(w / tree.size().width(), h / tree.size().height()),
 * &mut pixmap) over the buffer it is handed and registers tree.size() truncated (SvgAsset::resolution, svg_image.rs:89-94). */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "smr.h"

#define CHECK(call, what, errfn)                                          \
    do {                                                                  \
        int rc_ = (call);                                                 \
        if (rc_ < 0) {                                                    \
            fprintf(stderr, "%s failed (%d): %s\n", what, rc_, errfn);    \
            return 1;                                                     \
        }                                                                 \
    } while (0)

enum { OUT = 400 };

/* smr_svg_rasterise_fn: premultiplied, gamma-encoded RGBA8 into the zero-filled buffer, rows pitch_bytes apart.  Runs inside
 * smr_renderer_update_scene, on its thread; it must not call into the renderer. */
static double root(double v) {  /* (Newton's iteration: the example needs no libm) */
    double s = v > 1.0 ? v : 1.0;
    for (int i = 0; i < 40; i++) s = 0.5 * (s + v / s);
    return s;
}

static int draw_disc(void *user, const char *image_id, uint32_t w, uint32_t h, uint8_t *rgba, size_t pitch_bytes) {
    int *calls = user;
    (*calls)++;
    printf("  rasterise(\"%s\", %u x %u)\n", image_id, w, h);
    const double rx = w / 2.0, ry = h / 2.0, r = rx < ry ? rx : ry;
    for (uint32_t y = 0; y < h; y++)
        for (uint32_t x = 0; x < w; x++) {
            /* coverage of the pixel by the ellipse that fills the box: the distance to its edge in pixels, clamped to one pixel */
            const double dx = (x + 0.5 - rx) / rx, dy = (y + 0.5 - ry) / ry, d = root(dx * dx + dy * dy);
            double cover = (1.0 - d) * r + 0.5;
            cover = cover < 0.0 ? 0.0 : cover > 1.0 ? 1.0 : cover;
            const unsigned a = (unsigned)(cover * 255.0 + 0.5);
            uint8_t *p = rgba + pitch_bytes * y + 4 * (size_t)x;
            p[0] = (uint8_t)((230u * a + 127u) / 255u);  /* colour <= alpha: premultiplied */
            p[1] = (uint8_t)((120u * a + 127u) / 255u);
            p[2] = (uint8_t)((40u * a + 127u) / 255u);
            p[3] = (uint8_t)a;
        }
    return 0;
}

int main(int argc, char **argv) {
    smr_ctx *ctx = NULL;
    if (smr_ctx_create(0, SMR_MODE_GPU_OPTIMIZED, 0, NULL, &ctx) != 0) {
        fprintf(stderr, "no HIP device (there is no CPU fallback)\n");
        return 2;
    }
    smr_renderer *r = NULL;
    int calls = 0;
    CHECK(smr_renderer_create(ctx, -1, &r), "smr_renderer_create", smr_last_error(ctx));
    /* the tree's size: 64 x 64.  Nothing is rasterised here. */
    CHECK(smr_renderer_register_svg_image(r, "logo", 64, 64, draw_disc, &calls), "register_svg_image", smr_renderer_last_error(r));

    unsigned char *out = malloc((size_t)OUT * OUT * 4);
    const int sizes[2] = {64, 360};
    for (int k = 0; k < 2; k++) {
        char scene[256];
        snprintf(scene, sizeof scene,
                 "{\"type\": \"view\", \"background_color\": \"#102030FF\", \"children\": ["
                 " {\"type\": \"image\", \"image_id\": \"logo\", \"width\": %d, \"height\": %d}]}", sizes[k], sizes[k]);
        printf("update_scene with the logo at %d x %d:\n", sizes[k], sizes[k]);
        CHECK(smr_renderer_update_scene(r, "out", OUT, OUT, SMR_FRAME_RGBA, scene), "update_scene", smr_renderer_last_error(r));
        smr_output_frame outs[1];
        uint32_t n_out = 0;
        CHECK(smr_renderer_render(r, k * 33333333ll, NULL, 0, outs, 1, &n_out), "render", smr_renderer_last_error(r));
        void *oplanes[3] = {out, NULL, NULL};
        CHECK(smr_frame_download(ctx, outs[0].frame, oplanes), "smr_frame_download", smr_last_error(ctx));
        uint64_t rasterised = 0, launches = 0;
        uint32_t resident = 0;
        CHECK(smr_renderer_svg_stats(r, &rasterised, &launches, &resident), "svg_stats", smr_renderer_last_error(r));
        /* the edge of the disc is as sharp at 360 as at 64: texels that are neither background nor full colour, per row crossed */
        unsigned long soft = 0;
        for (int i = 0; i < sizes[k] * OUT; i++) soft += out[4 * i] != 0x10 && out[4 * i] != 230;
        printf("  rasteriser calls %llu, k_svg_nodes launches %llu, rasters resident %u; %.2f soft texels per row\n", (unsigned long long)rasterised,
               (unsigned long long)launches, resident, (double)soft / sizes[k]);
    }
    if (argc > 1) {
        FILE *f = fopen(argv[1], "wb");
        if (f) {
            fwrite(out, 1, (size_t)OUT * OUT * 4, f);
            fclose(f);
        }
    }
    /* refused while the scene shows it; fine once the output is gone */
    if (smr_renderer_unregister_image(r, "logo") == 0) fprintf(stderr, "unregister_image should have been refused\n");
    CHECK(smr_renderer_unregister_output(r, "out"), "unregister_output", smr_renderer_last_error(r));
    CHECK(smr_renderer_unregister_image(r, "logo"), "unregister_image", smr_renderer_last_error(r));
    smr_renderer_destroy(r);
    smr_ctx_destroy(ctx);
    free(out);
    return calls == 2 ? 0 : 1;
}
