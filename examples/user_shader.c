/* A user shader from C: a fragment function written in HIP C++ is compiled when it is registered (include/smr.h "user shaders") and
 * drawn by a Shader node.  The first shader here is a vignette: source 0 darkened towards the corners, `strength` from the node's
 * shader_param.  The second has an affine vertex stage: its last source turns by in.time radians about the target's centre, its aspect
 * ratio kept (smr_dimensions); outside that plane the target shows eight bands whose colours are the texels of a palette strip (smr_load).
 * The third has a clip vertex stage (a homogeneous position and tex_coords per vertex of the quad): the same picture as a card turning
 * about its vertical axis by in.time radians, in perspective; once it has turned its back it is culled and only the bands show.
 * The fourth is that card lit: its vertex stage also returns four varyings (SMR_VARYINGS) — a normal that turns with the card, interpolated
 * perspective-correct, and a flat tint per triangle — and the fragment applies a diffuse factor.
 * The fifth uses screen-space derivatives (SMR_DERIVATIVES): the camera picture through a disc whose edge is anti-aliased over exactly one
 * pixel at any resolution — the distance to the edge measured in units of smr_fwidth of that distance.
 *   gcc -std=c11 -Iinclude examples/user_shader.c -o user_shader -Lsmelter_amd -l:libsmr_hip.so -Wl,-rpath,$PWD/smelter_amd -lm
 * Exit codes: 0 ok, 2 no HIP device (the shader was still compiled: that needs none), 1 anything else. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "smr.h"

static const char *VIGNETTE =
    "__device__ float4 smr_fragment(const smr_shader_in &in, int plane_id, float2 uv, float2 position) {\n"
    "    const float strength = smr_param<float>(in);\n"
    "    const float dx = uv.x - 0.5f, dy = uv.y - 0.5f;\n"
    "    const float k = 1.0f - strength * smr_smoothstep(0.2f, 0.75f, sqrtf(dx * dx + dy * dy));\n"
    "    const float4 s = smr_sample(in, plane_id, uv.x, uv.y);\n"
    "    return make_float4(s.x * k, s.y * k, s.z * k, s.w);\n"
    "}\n";

/* (tests/user_shader_sources_affine.py carries the same text as ROTATE) */
static const char *ROTATE =
    "#define SMR_HAS_VERTEX_AFFINE\n"
    "__device__ smr_affine smr_vertex_affine(const smr_shader_in &in, int plane_id) {\n"
    "    smr_affine m = {1.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f};\n"
    "    if (plane_id != in.texture_count - 1) return m;\n"
    "    const uint2 d = smr_dimensions(in, plane_id);\n"
    "    const float W = (float)in.output_resolution.x, H = (float)in.output_resolution.y;\n"
    "    const float fit = fminf(W / (float)d.x, H / (float)d.y) * 0.6f;\n"
    "    const float hw = 0.5f * fit * (float)d.x, hh = 0.5f * fit * (float)d.y;  // the plane's half extent in pixels\n"
    "    const float c = cosf(in.time), s = sinf(in.time);\n"
    "    m.xx = 2.0f * hw * c / W; m.xy = -2.0f * hh * s / W;\n"
    "    m.yx = 2.0f * hw * s / H; m.yy = 2.0f * hh * c / H;\n"
    "    return m;\n"
    "}\n"
    "__device__ float4 smr_fragment(const smr_shader_in &in, int plane_id, float2 uv, float2 position) {\n"
    "    const uint2 d = smr_dimensions(in, plane_id);\n"
    "    if (plane_id != in.texture_count - 1) {\n"
    "        int band = (int)(uv.x * 8.0f);\n"
    "        if (band > (int)d.x - 1) band = (int)d.x - 1;\n"
    "        return smr_load(in, plane_id, band, 0);\n"
    "    }\n"
    "    int tx = (int)floorf(uv.x * (float)d.x), ty = (int)floorf(uv.y * (float)d.y);\n"
    "    if (tx > (int)d.x - 1) tx = (int)d.x - 1;\n"
    "    if (ty > (int)d.y - 1) ty = (int)d.y - 1;\n"
    "    return smr_load(in, plane_id, tx, ty);\n"
    "}\n";

/* (tests/user_shader_sources_clip.py carries the same text as FLIP) */
static const char *FLIP =
    "#define SMR_HAS_VERTEX_CLIP\n"
    "__device__ smr_clip_vertex smr_vertex_clip(const smr_shader_in &in, int plane_id, int vertex_index, float3 position, float2 tex_coords) {\n"
    "    smr_clip_vertex o;\n"
    "    o.position = make_float4(position.x, position.y, 0.0f, 1.0f);\n"
    "    o.tex_coords = tex_coords;\n"
    "    if (plane_id != in.texture_count - 1) return o;\n"
    "    const uint2 d = smr_dimensions(in, plane_id);\n"
    "    const float W = (float)in.output_resolution.x, H = (float)in.output_resolution.y;\n"
    "    const float fit = fminf(W / (float)d.x, H / (float)d.y) * 0.6f;\n"
    "    const float sx = fit * (float)d.x / W, sy = fit * (float)d.y / H;  // the card's half extent in clip space\n"
    "    const float xr = position.x * sx * cosf(in.time), zr = position.x * sx * sinf(in.time);\n"
    "    const float w = 1.0f + zr / 2.5f;\n"
    "    o.position = make_float4(xr, position.y * sy, 0.5f * w, w);\n"
    "    return o;\n"
    "}\n"
    "__device__ float4 smr_fragment(const smr_shader_in &in, int plane_id, float2 uv, float2 position) {\n"
    "    const uint2 d = smr_dimensions(in, plane_id);\n"
    "    if (plane_id != in.texture_count - 1) {\n"
    "        int band = (int)(uv.x * 8.0f);\n"
    "        if (band > (int)d.x - 1) band = (int)d.x - 1;\n"
    "        return smr_load(in, plane_id, band, 0);\n"
    "    }\n"
    "    int tx = (int)floorf(uv.x * (float)d.x), ty = (int)floorf(uv.y * (float)d.y);\n"
    "    if (tx > (int)d.x - 1) tx = (int)d.x - 1;\n"
    "    if (ty > (int)d.y - 1) ty = (int)d.y - 1;\n"
    "    return smr_load(in, plane_id, tx, ty);\n"
    "}\n";

/* (tests/user_shader_sources_varyings.py carries the same text as LIT) */
static const char *LIT =
    "#define SMR_HAS_VERTEX_CLIP\n"
    "#define SMR_VARYINGS 4\n"
    "#define SMR_VARYINGS_FLAT 0x8\n"
    "__device__ smr_clip_vertex_v<SMR_VARYINGS> smr_vertex_clip(const smr_shader_in &in, int plane_id, int vertex_index, float3 position, float2 tex_coords) {\n"
    "    smr_clip_vertex_v<SMR_VARYINGS> o;\n"
    "    o.position = make_float4(position.x, position.y, 0.0f, 1.0f);\n"
    "    o.tex_coords = tex_coords;\n"
    "    o.varyings[0] = 0.0f; o.varyings[1] = 0.0f; o.varyings[2] = -1.0f;  // the normal: towards the eye\n"
    "    o.varyings[3] = 1.0f;\n"
    "    if (plane_id != in.texture_count - 1) return o;\n"
    "    const uint2 d = smr_dimensions(in, plane_id);\n"
    "    const float W = (float)in.output_resolution.x, H = (float)in.output_resolution.y;\n"
    "    const float fit = fminf(W / (float)d.x, H / (float)d.y) * 0.6f;\n"
    "    const float sx = fit * (float)d.x / W, sy = fit * (float)d.y / H;  // the card's half extent in clip space\n"
    "    const float c = cosf(in.time), s = sinf(in.time);\n"
    "    const float xr = position.x * sx * c, zr = position.x * sx * s;\n"
    "    const float w = 1.0f + zr / 2.5f;\n"
    "    o.position = make_float4(xr, position.y * sy, 0.5f * w, w);\n"
    "    const float nx = 0.5f * position.x, ny = 0.25f * position.y, nz = -1.0f;  // leaning outwards, then turned with the card\n"
    "    o.varyings[0] = nx * c - nz * s; o.varyings[1] = ny; o.varyings[2] = nx * s + nz * c;\n"
    "    o.varyings[3] = vertex_index == 0 ? 1.0f : 0.875f;  // the provoking vertex's value: triangle (0, 1, 2) full, (2, 3, 0) a shade darker\n"
    "    return o;\n"
    "}\n"
    "__device__ float4 smr_fragment(const smr_shader_in &in, int plane_id, float2 uv, float4 position, const smr_varyings<SMR_VARYINGS> &v) {\n"
    "    const uint2 d = smr_dimensions(in, plane_id);\n"
    "    if (plane_id != in.texture_count - 1) {\n"
    "        int band = (int)(uv.x * 8.0f);\n"
    "        if (band > (int)d.x - 1) band = (int)d.x - 1;\n"
    "        return smr_load(in, plane_id, band, 0);\n"
    "    }\n"
    "    int tx = (int)floorf(uv.x * (float)d.x), ty = (int)floorf(uv.y * (float)d.y);\n"
    "    if (tx > (int)d.x - 1) tx = (int)d.x - 1;\n"
    "    if (ty > (int)d.y - 1) ty = (int)d.y - 1;\n"
    "    const float4 texel = smr_load(in, plane_id, tx, ty);\n"
    "    const float len = sqrtf(v.v[0] * v.v[0] + v.v[1] * v.v[1] + v.v[2] * v.v[2]);\n"
    "    const float diffuse = fmaxf((v.v[0] * -0.48f + v.v[1] * 0.6f + v.v[2] * -0.64f) / len, 0.0f);  // the light's direction is a unit vector\n"
    "    const float k = (0.25f + 0.75f * diffuse) * v.v[3];\n"
    "    return make_float4(texel.x * k, texel.y * k, texel.z * k, texel.w);\n"
    "}\n";

/* (tests/user_shader_sources_derivatives.py carries the same text as DISC) */
static const char *DISC =
    "#define SMR_DERIVATIVES\n"
    "__device__ float4 smr_fragment(const smr_shader_in &in, int plane_id, float2 uv, float2 position) {\n"
    "    const float W = (float)in.output_resolution.x, H = (float)in.output_resolution.y;\n"
    "    const float dx = position.x - (0.5f * W + 0.3f), dy = position.y - (0.5f * H + 0.1f);\n"
    "    const float d = sqrtf(dx * dx + dy * dy);\n"
    "    const float footprint = smr_fwidth(d);  // (before any branch: a derivative wants the whole quad)\n"
    "    const float cover = fminf(fmaxf(0.5f - (d - 0.4f * fminf(W, H)) / footprint, 0.0f), 1.0f);\n"
    "    const uint2 s = smr_dimensions(in, plane_id);\n"
    "    int tx = (int)floorf(uv.x * (float)s.x), ty = (int)floorf(uv.y * (float)s.y);\n"
    "    if (tx > (int)s.x - 1) tx = (int)s.x - 1;\n"
    "    if (ty > (int)s.y - 1) ty = (int)s.y - 1;\n"
    "    const float4 t = smr_load(in, plane_id, tx, ty);\n"
    "    return make_float4(t.x * cover, t.y * cover, t.z * cover, t.w * cover);\n"
    "}\n";

static const char *SCENE =
    "{\"type\":\"shader\",\"shader_id\":\"vignette\",\"resolution\":{\"width\":640,\"height\":360},"
    "\"shader_param\":{\"type\":\"f32\",\"value\":0.8},\"children\":[{\"type\":\"input_stream\",\"input_id\":\"cam\"}]}";

static const char *FLIP_SCENE =
    "{\"type\":\"shader\",\"shader_id\":\"flip\",\"resolution\":{\"width\":640,\"height\":360},"
    "\"children\":[{\"type\":\"input_stream\",\"input_id\":\"palette\"},{\"type\":\"input_stream\",\"input_id\":\"cam\"}]}";

static const char *LIT_SCENE =
    "{\"type\":\"shader\",\"shader_id\":\"lit\",\"resolution\":{\"width\":640,\"height\":360},"
    "\"children\":[{\"type\":\"input_stream\",\"input_id\":\"palette\"},{\"type\":\"input_stream\",\"input_id\":\"cam\"}]}";

static const char *DISC_SCENE =
    "{\"type\":\"shader\",\"shader_id\":\"disc\",\"resolution\":{\"width\":640,\"height\":360},"
    "\"children\":[{\"type\":\"input_stream\",\"input_id\":\"cam\"}]}";

static const char *SPIN_SCENE =
    "{\"type\":\"shader\",\"shader_id\":\"rotate\",\"resolution\":{\"width\":640,\"height\":360},"
    "\"children\":[{\"type\":\"input_stream\",\"input_id\":\"palette\"},{\"type\":\"input_stream\",\"input_id\":\"cam\"}]}";

int main(void) {
    /* host only: compile, show what the compiler said */
    smr_shader_program *prog = NULL;
    int rc = smr_shader_program_create(VIGNETTE, &prog);
    if (rc != SMR_OK) {
        fprintf(stderr, "the shader did not compile (%d):\n%s\n", rc, prog ? smr_shader_program_log(prog) : "");
        smr_shader_program_destroy(prog);
        return 1;
    }
    const void *code = NULL;
    size_t code_size = 0;
    smr_shader_program_code(prog, &code, &code_size);
    printf("vignette: %zu bytes of gfx950 code\n", code_size);
    smr_shader_program *spin = NULL;
    rc = smr_shader_program_create(ROTATE, &spin);
    if (rc != SMR_OK) {
        fprintf(stderr, "the rotating shader did not compile (%d):\n%s\n", rc, spin ? smr_shader_program_log(spin) : "");
        smr_shader_program_destroy(spin);
        smr_shader_program_destroy(prog);
        return 1;
    }
    smr_shader_program *flip = NULL;
    rc = smr_shader_program_create(FLIP, &flip);
    if (rc != SMR_OK) {
        fprintf(stderr, "the card shader did not compile (%d):\n%s\n", rc, flip ? smr_shader_program_log(flip) : "");
        smr_shader_program_destroy(flip);
        smr_shader_program_destroy(spin);
        smr_shader_program_destroy(prog);
        return 1;
    }
    smr_shader_program *lit = NULL;
    rc = smr_shader_program_create(LIT, &lit);
    if (rc != SMR_OK) {
        fprintf(stderr, "the lit card shader did not compile (%d):\n%s\n", rc, lit ? smr_shader_program_log(lit) : "");
        smr_shader_program_destroy(lit);
        smr_shader_program_destroy(flip);
        smr_shader_program_destroy(spin);
        smr_shader_program_destroy(prog);
        return 1;
    }
    smr_shader_program *disc = NULL;
    rc = smr_shader_program_create(DISC, &disc);
    if (rc != SMR_OK) {
        fprintf(stderr, "the disc shader did not compile (%d):\n%s\n", rc, disc ? smr_shader_program_log(disc) : "");
        smr_shader_program_destroy(disc);
        smr_shader_program_destroy(lit);
        smr_shader_program_destroy(flip);
        smr_shader_program_destroy(spin);
        smr_shader_program_destroy(prog);
        return 1;
    }

    smr_ctx *ctx = NULL;
    if (smr_ctx_create(0, SMR_MODE_GPU_OPTIMIZED, SMR_DEFAULT_MAX_LAYOUTS, NULL, &ctx) != SMR_OK) {
        fprintf(stderr, "no HIP device\n");
        smr_shader_program_destroy(disc);
        smr_shader_program_destroy(lit);
        smr_shader_program_destroy(flip);
        smr_shader_program_destroy(spin);
        smr_shader_program_destroy(prog);
        return 2;
    }
    smr_renderer *r = NULL;
    int status = 1;
    smr_frame cam, palette;
    memset(&cam, 0, sizeof(cam));
    memset(&palette, 0, sizeof(palette));
    if (smr_renderer_create(ctx, -1, &r) != 0) goto out;
    if (smr_renderer_register_input(r, "cam") != 0 || smr_renderer_register_shader_program(r, "vignette", prog) != 0 ||
        smr_renderer_update_scene(r, "out", 640, 360, SMR_FRAME_RGBA, SCENE) != 0) {
        fprintf(stderr, "%s\n", smr_renderer_last_error(r));
        goto out;
    }
    if (smr_frame_create(ctx, SMR_FRAME_RGBA, 320, 180, &cam) != SMR_OK) goto out;
    {
        uint8_t *px = malloc(320 * 180 * 4);
        const void *planes[3] = {px, NULL, NULL};
        memset(px, 200, 320 * 180 * 4);
        smr_frame_upload(ctx, &cam, planes);
        free(px);
        smr_input_frame in = {"cam", &cam, 0};
        smr_output_frame out[1];
        uint32_t n = 0;
        if (smr_renderer_render(r, 0, &in, 1, out, 1, &n) != 0 || n != 1) {
            fprintf(stderr, "%s\n", smr_renderer_last_error(r));
            goto out;
        }
        uint8_t *got = malloc(640 * 360 * 4);
        void *dst[3] = {got, NULL, NULL};
        smr_frame_download(out[0].ctx, out[0].frame, dst);
        uint64_t launches = 0;
        smr_shader_program_launches(prog, &launches);
        printf("centre %u, corner %u, launches %llu\n", got[(180 * 640 + 320) * 4], got[0], (unsigned long long)launches);
        status = got[(180 * 640 + 320) * 4] > got[0] && launches == 1 ? 0 : 1;

        /* the same output with the rotating shader: an 8 x 1 palette strip behind the camera picture, 0.7 s into the turn */
        static const uint8_t strip[8][4] = {{255, 0, 0, 255},   {255, 128, 0, 255}, {255, 255, 0, 255}, {0, 255, 0, 255},
                                            {0, 255, 255, 255}, {0, 0, 255, 255},   {128, 0, 255, 255}, {255, 0, 255, 255}};
        const void *strip_planes[3] = {strip, NULL, NULL};
        if (status != 0 || smr_frame_create(ctx, SMR_FRAME_RGBA, 8, 1, &palette) != SMR_OK) {
            status = 1;
            free(got);
            goto out;
        }
        smr_frame_upload(ctx, &palette, strip_planes);
        status = 1;
        if (smr_renderer_register_input(r, "palette") != 0 || smr_renderer_register_shader_program(r, "rotate", spin) != 0 ||
            smr_renderer_update_scene(r, "out", 640, 360, SMR_FRAME_RGBA, SPIN_SCENE) != 0) {
            fprintf(stderr, "%s\n", smr_renderer_last_error(r));
            free(got);
            goto out;
        }
        smr_input_frame both[2] = {{"cam", &cam, 700000000}, {"palette", &palette, 700000000}};
        if (smr_renderer_render(r, 700000000, both, 2, out, 1, &n) != 0 || n != 1) {
            fprintf(stderr, "%s\n", smr_renderer_last_error(r));
            free(got);
            goto out;
        }
        smr_frame_download(out[0].ctx, out[0].frame, dst);
        smr_shader_program_launches(spin, &launches);
        const uint8_t *corner = got, *centre = got + (180 * 640 + 320) * 4;
        printf("rotating: corner %u %u %u, centre %u %u %u, launches %llu\n", corner[0], corner[1], corner[2], centre[0], centre[1], centre[2],
               (unsigned long long)launches);
        /* the corner is the palette's first band, the centre the camera picture */
        status = corner[0] == 255 && corner[1] == 0 && corner[2] == 0 && centre[1] > 0 && launches == 1 ? 0 : 1;

        /* the same two inputs with the card shader, 0.7 s into the turn: the card still faces the eye */
        if (status != 0 || smr_renderer_register_shader_program(r, "flip", flip) != 0 ||
            smr_renderer_update_scene(r, "out", 640, 360, SMR_FRAME_RGBA, FLIP_SCENE) != 0 ||
            smr_renderer_render(r, 700000000, both, 2, out, 1, &n) != 0 || n != 1) {
            if (status == 0) fprintf(stderr, "%s\n", smr_renderer_last_error(r));
            status = 1;
            free(got);
            goto out;
        }
        smr_frame_download(out[0].ctx, out[0].frame, dst);
        smr_shader_program_launches(flip, &launches);
        printf("card: corner %u %u %u, centre %u %u %u, launches %llu\n", corner[0], corner[1], corner[2], centre[0], centre[1], centre[2],
               (unsigned long long)launches);
        status = corner[0] == 255 && corner[1] == 0 && corner[2] == 0 && centre[1] > 0 && launches == 1 ? 0 : 1;

        /* and with the lit card: the same coverage, the camera picture (200 throughout) darkened by the diffuse factor */
        const unsigned unlit = centre[1];
        if (status != 0 || smr_renderer_register_shader_program(r, "lit", lit) != 0 ||
            smr_renderer_update_scene(r, "out", 640, 360, SMR_FRAME_RGBA, LIT_SCENE) != 0 ||
            smr_renderer_render(r, 700000000, both, 2, out, 1, &n) != 0 || n != 1) {
            if (status == 0) fprintf(stderr, "%s\n", smr_renderer_last_error(r));
            status = 1;
            free(got);
            goto out;
        }
        smr_frame_download(out[0].ctx, out[0].frame, dst);
        smr_shader_program_launches(lit, &launches);
        printf("lit card: corner %u %u %u, centre %u %u %u, launches %llu\n", corner[0], corner[1], corner[2], centre[0], centre[1], centre[2],
               (unsigned long long)launches);
        status = corner[0] == 255 && corner[1] == 0 && corner[2] == 0 && centre[1] > 0 && centre[1] < unlit && launches == 1 ? 0 : 1;

        /* the camera picture alone through the anti-aliased disc: transparent in the corner, the picture (alpha 200) in the centre, and on
         * the disc's rightmost pixel (the centre is at 320.3, the radius 144) a coverage strictly between the two */
        if (status != 0 || smr_renderer_register_shader_program(r, "disc", disc) != 0 ||
            smr_renderer_update_scene(r, "out", 640, 360, SMR_FRAME_RGBA, DISC_SCENE) != 0 ||
            smr_renderer_render(r, 700000000, both, 1, out, 1, &n) != 0 || n != 1) {
            if (status == 0) fprintf(stderr, "%s\n", smr_renderer_last_error(r));
            status = 1;
            free(got);
            goto out;
        }
        smr_frame_download(out[0].ctx, out[0].frame, dst);
        smr_shader_program_launches(disc, &launches);
        const uint8_t *rim = got + (180 * 640 + 464) * 4;
        printf("disc: corner alpha %u, centre %u alpha %u, rim alpha %u, launches %llu\n", corner[3], centre[0], centre[3], rim[3], (unsigned long long)launches);
        status = corner[3] == 0 && centre[3] == 200 && rim[3] > 0 && rim[3] < centre[3] && launches == 1 ? 0 : 1;
        free(got);
    }
out:
    if (r) smr_renderer_destroy(r);
    smr_frame_destroy(ctx, &cam);
    smr_frame_destroy(ctx, &palette);
    smr_ctx_destroy(ctx);
    smr_shader_program_destroy(disc);
    smr_shader_program_destroy(lit);
    smr_shader_program_destroy(flip);
    smr_shader_program_destroy(spin);
    smr_shader_program_destroy(prog); /* after the renderer it was registered in */
    return status;
}
