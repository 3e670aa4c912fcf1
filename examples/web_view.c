/* web_view.c — a WebView node from plain C: the browser is the caller's, the node's compositing is the library's (include/smr.h,
 * "WebView nodes").
 *
 *   gcc -std=c11 -Iinclude examples/web_view.c -o web_view -Lsmelter_amd -l:libsmr_hip.so -Wl,-rpath,$PWD/smelter_amd -lm
 *   ./web_view out.rgba        # a 640x360 "page" painted here in place of a browser, one camera embedded in it, three frames
 *
 * What a host that owns a CEF browser does with the three calls (transformations/web_renderer/browser_client.rs, renderer.rs:78-134):
 *   RenderHandler::OnPaint(buffer, width, height)        -> smr_renderer_web_paint(r, id, buffer, 4 * width)
 *   the page's GET_FRAME_POSITIONS reply                  -> smr_renderer_web_positions(r, id, rects, n)      (child order)
 *   WebRendererSpec { resolution, embedding_method }      -> smr_renderer_register_web_renderer(r, id, w, h, method) */
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

enum { PW = 640, PH = 360, CW = 320, CH = 180 };

/* the "browser": a translucent scoreboard bar along the bottom and a frame around the hole the camera shows through, premultiplied BGRA */
static void paint(unsigned char *bgra, int score) {
    memset(bgra, 0, (size_t)PW * PH * 4);
    for (int y = 0; y < PH; y++)
        for (int x = 0; x < PW; x++) {
            unsigned char *p = bgra + ((size_t)y * PW + x) * 4;
            const int in_hole = x >= 40 && x < 40 + CW && y >= 30 && y < 30 + CH;
            const int in_frame = x >= 32 && x < 48 + CW && y >= 22 && y < 38 + CH;
            if (y >= PH - 60) { p[0] = 96; p[1] = 32; p[2] = (unsigned char)(16 + (x * score) % 64); p[3] = 160; }  /* colour <= alpha */
            else if (in_frame && !in_hole) { p[0] = 255; p[1] = 255; p[2] = 255; p[3] = 255; }
        }
}

int main(int argc, char **argv) {
    smr_ctx *ctx = NULL;
    if (smr_ctx_create(0, SMR_MODE_GPU_OPTIMIZED, 0, NULL, &ctx) != 0) {
        fprintf(stderr, "no HIP device (there is no CPU fallback)\n");
        return 2;
    }
    smr_renderer *r = NULL;
    CHECK(smr_renderer_create(ctx, -1, &r), "smr_renderer_create", smr_last_error(ctx));
    CHECK(smr_renderer_register_web_renderer(r, "scoreboard", PW, PH, SMR_WEB_NATIVE_UNDER_CONTENT), "register_web_renderer", smr_renderer_last_error(r));
    CHECK(smr_renderer_register_input(r, "cam"), "register_input", smr_renderer_last_error(r));

    /* the camera: a gradient, planar YUV 4:2:0 resident in HBM */
    smr_frame cam;
    unsigned char *y = malloc(CW * CH), *u = malloc(CW * CH / 4), *v = malloc(CW * CH / 4);
    for (int i = 0; i < CW * CH; i++) y[i] = (unsigned char)(16 + (i % CW) * 219 / CW);
    memset(u, 100, CW * CH / 4);
    memset(v, 170, CW * CH / 4);
    CHECK(smr_frame_create(ctx, SMR_FRAME_PLANAR_YUV420, CW, CH, &cam), "smr_frame_create", smr_last_error(ctx));
    const void *planes[3] = {y, u, v};
    CHECK(smr_frame_upload(ctx, &cam, planes), "smr_frame_upload", smr_last_error(ctx));

    /* children of a web_view need an id: the page finds their elements by it */
    CHECK(smr_renderer_update_scene(r, "out", PW, PH, SMR_FRAME_RGBA,
                                    "{\"type\": \"web_view\", \"instance_id\": \"scoreboard\", \"children\": ["
                                    " {\"type\": \"input_stream\", \"id\": \"cam\", \"input_id\": \"cam\"}]}"),
          "update_scene", smr_renderer_last_error(r));

    unsigned char *page = malloc((size_t)PW * PH * 4), *out = malloc((size_t)PW * PH * 4);
    const smr_web_rect where = {40.0f, 30.0f, (float)CW, (float)CH};   /* getBoundingClientRect of the element with id "cam" */
    CHECK(smr_renderer_web_positions(r, "scoreboard", &where, 1), "web_positions", smr_renderer_last_error(r));
    for (int frame = 0; frame < 3; frame++) {
        const int64_t pts = frame * 33333333ll;
        paint(page, 3 + frame);                                         /* OnPaint: the page changed */
        CHECK(smr_renderer_web_paint(r, "scoreboard", page, (size_t)PW * 4), "web_paint", smr_renderer_last_error(r));
        const smr_input_frame in = {"cam", &cam, pts};
        smr_output_frame outs[1];
        uint32_t n_out = 0;
        CHECK(smr_renderer_render(r, pts, &in, 1, outs, 1, &n_out), "render", smr_renderer_last_error(r));
        void *oplanes[3] = {out, NULL, NULL};
        CHECK(smr_frame_download(ctx, outs[0].frame, oplanes), "smr_frame_download", smr_last_error(ctx));
    }
    uint64_t launches = 0;
    CHECK(smr_renderer_web_launches(r, &launches), "web_launches", smr_renderer_last_error(r));
    unsigned long alpha = 0;
    for (int i = 0; i < PW * PH; i++) alpha += out[4 * i + 3];
    printf("3 frames of a %dx%d web view with one embedded camera: %llu k_web_view launches, mean alpha %.2f\n", PW, PH, (unsigned long long)launches,
           (double)alpha / (PW * PH));
    if (argc > 1) {
        FILE *f = fopen(argv[1], "wb");
        if (f) {
            fwrite(out, 1, (size_t)PW * PH * 4, f);
            fclose(f);
        }
    }
    smr_frame_destroy(ctx, &cam);
    smr_renderer_destroy(r);
    smr_ctx_destroy(ctx);
    free(y); free(u); free(v); free(page); free(out);
    return 0;
}
