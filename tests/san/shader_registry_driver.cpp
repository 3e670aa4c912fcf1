// TEST INFRASTRUCTURE — not part of the product.  The user-shader side of the renderer's registry (smelter_amd/csrc/host/shader_program.cpp
// + renderer.cpp) on the null device (null_device.cpp), under AddressSanitizer + UBSan: the real runtime compiler compiles the sources —
// that needs no GPU — and a stand-in for smr_user_shader (the only entry point of the device half the host half calls) reads the program
// and the parameter block it is handed, so a program that was freed while still registered is a use-after-free report.
//   register source -> render; a source that does not compile -> refused with the log, the id still renders; replacing a source frees the
//   old program; a caller-owned program in two renderers, one destroyed; the id re-registered as a built-in, then the program destroyed.
// Prints one JSON line; exit code 0 = every expectation held.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

#include "smr.h"

extern "C" long null_device_live_surfaces();

static long g_user_launches = 0;
static volatile uint64_t g_sink;

extern "C" int smr_user_shader(smr_ctx *ctx, const smr_shader_program *p, const void *params, size_t params_size, const smr_surface *const *src,
                               uint32_t n_src, smr_surface *dst, float time_s) {
    (void)time_s; (void)src; (void)n_src;
    if (!ctx || !p || !dst || params_size > SMR_SHADER_MAX_PARAM_BYTES) return SMR_ERR_INVALID;
    const void *code = nullptr;
    size_t size = 0;
    if (smr_shader_program_code(p, &code, &size) != SMR_OK) return SMR_ERR_INVALID;  // (reads the program: freed -> ASan)
    uint64_t s = 0;
    for (size_t i = 0; i < size; i++) s += ((const uint8_t *)code)[i];
    for (size_t i = 0; i < params_size; i++) s += ((const uint8_t *)params)[i];
    g_sink = s;
    g_user_launches++;
    return SMR_OK;
}

static const char *GOOD_A =
    "__device__ float4 smr_fragment(const smr_shader_in &in, int plane_id, float2 uv, float2 position) {\n"
    "    return make_float4(uv.x, uv.y, 0.0f, 1.0f);\n}\n";
static const char *GOOD_B =
    "struct Fill { float r, g, b, a; };\n"
    "__device__ float4 smr_fragment(const smr_shader_in &in, int plane_id, float2 uv, float2 position) {\n"
    "    const Fill f = smr_param<Fill>(in);\n    return make_float4(f.r, f.g, f.b, f.a);\n}\n";
static const char *BROKEN =
    "__device__ float4 smr_fragment(const smr_shader_in &in, int plane_id, float2 uv, float2 position) {\n"
    "    return make_float4(uv.x, 0.0f, 0.0f, no_such_thing);\n}\n";

static int failures = 0;
#define EXPECT(cond)                                                         \
    do {                                                                     \
        if (!(cond)) { fprintf(stderr, "line %d: %s\n", __LINE__, #cond); failures++; } \
    } while (0)

static std::string scene(const char *shader_id) {
    return std::string("{\"type\":\"shader\",\"shader_id\":\"") + shader_id +
           "\",\"resolution\":{\"width\":64,\"height\":36},\"shader_param\":{\"type\":\"list\",\"value\":["
           "{\"type\":\"f32\",\"value\":0.5},{\"type\":\"f32\",\"value\":0.25},{\"type\":\"f32\",\"value\":0.0},{\"type\":\"f32\",\"value\":1.0}]}}";
}
static int render(smr_renderer *r) {
    smr_output_frame out[4];
    uint32_t n = 0;
    return smr_renderer_render(r, 0, nullptr, 0, out, 4, &n);
}

int main() {
    smr_ctx *ctx = nullptr;
    EXPECT(smr_ctx_create(0, SMR_MODE_GPU_OPTIMIZED, 100, nullptr, &ctx) == SMR_OK);
    smr_shader_program *probe = nullptr;
    const int first = smr_shader_program_create(GOOD_A, &probe);
    if (first == SMR_ERR_INTERNAL) {  // no runtime compiler on this machine: the message must say so
        const bool named = probe && strstr(smr_shader_program_log(probe), "libhiprtc.so");
        smr_shader_program_destroy(probe);
        smr_ctx_destroy(ctx);
        printf("{\"compiler\": false, \"named\": %s}\n", named ? "true" : "false");
        return named ? 0 : 1;
    }
    EXPECT(first == SMR_OK);
    smr_shader_program_destroy(probe);

    smr_renderer *a = nullptr, *b = nullptr;
    EXPECT(smr_renderer_create(ctx, -1, &a) == 0 && smr_renderer_create(ctx, -1, &b) == 0);
    // an id that is not registered is refused, the id registered from source renders through the user path
    EXPECT(smr_renderer_update_scene(a, "out", 64, 36, SMR_FRAME_RGBA, scene("fx").c_str()) < 0);
    EXPECT(smr_renderer_register_shader_source(a, "fx", GOOD_A) == SMR_OK);
    EXPECT(smr_renderer_update_scene(a, "out", 64, 36, SMR_FRAME_RGBA, scene("fx").c_str()) == 0);
    EXPECT(render(a) == 0 && g_user_launches == 1);
    // a source that does not compile: refused with the compiler's log, the registry as it was
    EXPECT(smr_renderer_register_shader_source(a, "fx", BROKEN) == SMR_ERR_INVALID);
    EXPECT(strstr(smr_renderer_last_error(a), "no_such_thing") && strstr(smr_renderer_last_error(a), "shader:2"));
    EXPECT(smr_renderer_register_shader_source(a, "other", BROKEN) == SMR_ERR_INVALID);
    EXPECT(smr_renderer_update_scene(a, "out2", 64, 36, SMR_FRAME_RGBA, scene("other").c_str()) < 0);  // ... and no new id
    EXPECT(render(a) == 0 && g_user_launches == 2);
    // replacing the source frees the program it replaces
    EXPECT(smr_renderer_register_shader_source(a, "fx", GOOD_B) == SMR_OK);
    EXPECT(render(a) == 0 && g_user_launches == 3);
    // a built-in id over a user shader and back
    EXPECT(smr_renderer_register_shader(a, "fx", SMR_SHADER_GRADIENT) == 0);
    EXPECT(render(a) == 0 && g_user_launches == 3);
    EXPECT(smr_renderer_register_shader(a, "fx", 99) < 0 && strstr(smr_renderer_last_error(a), "unknown built-in shader"));
    EXPECT(smr_renderer_register_shader_source(a, "fx", GOOD_A) == SMR_OK);
    EXPECT(render(a) == 0 && g_user_launches == 4);

    // a program the caller owns, registered in two renderers
    smr_shader_program *p = nullptr, *bad = nullptr;
    EXPECT(smr_shader_program_create(GOOD_B, &p) == SMR_OK && p && smr_shader_program_log(p)[0] == 0);
    EXPECT(smr_shader_program_create(BROKEN, &bad) == SMR_ERR_INVALID && bad && strstr(smr_shader_program_log(bad), "no_such_thing"));
    const void *code = nullptr;
    size_t size = 0;
    EXPECT(smr_shader_program_code(bad, &code, &size) == SMR_ERR_INVALID);
    EXPECT(smr_renderer_register_shader_program(b, "bad", bad) == SMR_ERR_INVALID);
    smr_shader_program_destroy(bad);
    EXPECT(smr_renderer_register_shader_program(a, "p", p) == SMR_OK && smr_renderer_register_shader_program(b, "p", p) == SMR_OK);
    EXPECT(smr_renderer_update_scene(b, "out", 64, 36, SMR_FRAME_RGBA, scene("p").c_str()) == 0);
    EXPECT(render(b) == 0 && g_user_launches == 5);
    smr_renderer_destroy(a);  // owns "fx" (freed with it), does not own p
    EXPECT(render(b) == 0 && g_user_launches == 6);
    // the id becomes a built-in: the program may go while the renderer lives on
    EXPECT(smr_renderer_register_shader(b, "p", SMR_SHADER_COLOR_BY_TEXTURE_COUNT) == 0);
    smr_shader_program_destroy(p);
    EXPECT(render(b) == 0 && g_user_launches == 6);
    EXPECT(smr_renderer_register_shader_source(b, nullptr, GOOD_A) < 0 && smr_renderer_register_shader_source(b, "x", nullptr) < 0);
    EXPECT(smr_renderer_register_shader_program(b, "x", nullptr) < 0);
    smr_renderer_destroy(b);
    smr_ctx_destroy(ctx);
    EXPECT(null_device_live_surfaces() == 0);
    printf("{\"compiler\": true, \"user_launches\": %ld, \"failures\": %d}\n", g_user_launches, failures);
    return failures ? 1 : 0;
}
