"""User shader sources for the affine vertex stage, smr_load and smr_dimensions (include/smr.h "user shaders"): what
tests/test_emu_user_shader_affine.py runs on the lane emulator and tests/test_gpu_user_shader_affine.py on the device.  Their expected
pictures follow from the contract alone (the numpy model in the former).  No loops; nothing here is meant to fault."""

# the texel of source plane_id nearest uv, through smr_dimensions + smr_load: no filtering, so a model needs no bilinear arithmetic
_NEAREST = r"""
__device__ float4 smr_fragment(const smr_shader_in &in, int plane_id, float2 uv, float2 position) {
    const uint2 d = smr_dimensions(in, plane_id);
    int tx = (int)floorf(uv.x * (float)d.x), ty = (int)floorf(uv.y * (float)d.y);
    if (tx > (int)d.x - 1) tx = (int)d.x - 1;  // (u just below 1 may round up to the width)
    if (ty > (int)d.y - 1) ty = (int)d.y - 1;
    return smr_load(in, plane_id, tx, ty);
}
"""

# params: six f32 {xx, xy, yx, yy, cx, cy} per source
AFFINE_PARAM = r"""
#define SMR_HAS_VERTEX_AFFINE
__device__ smr_affine smr_vertex_affine(const smr_shader_in &in, int plane_id) {
    const int i = plane_id < 0 ? 0 : plane_id;
    smr_affine m;
    __builtin_memcpy(&m, smr_param_bytes(in) + (size_t)(i & 15) * sizeof(smr_affine), sizeof(smr_affine));
    return m;
}
""" + _NEAREST

# params: four f32 {sx, sy, cx, cy} per source — the axis-aligned stage with the same fragment
PLANE_PARAM = r"""
#define SMR_HAS_VERTEX
__device__ smr_plane smr_vertex(const smr_shader_in &in, int plane_id) {
    const int i = plane_id < 0 ? 0 : plane_id;
    smr_plane p;
    __builtin_memcpy(&p, smr_param_bytes(in) + (size_t)(i & 15) * sizeof(smr_plane), sizeof(smr_plane));
    return p;
}
""" + _NEAREST

# no vertex stage: the target is source 0 tiled, texel (x mod w, y mod h)
TILE = r"""
__device__ float4 smr_fragment(const smr_shader_in &in, int plane_id, float2 uv, float2 position) {
    if (plane_id > 0) return make_float4(0.f, 0.f, 0.f, 0.f);
    const uint2 d = smr_dimensions(in, 0);
    if (d.x == 0u || d.y == 0u) return make_float4(0.f, 0.f, 0.f, 0.f);
    return smr_load(in, 0, (int)((unsigned int)position.x % d.x), (int)((unsigned int)position.y % d.y));
}
"""

# row 0: column k is smr_load(in, i, x, y) of the k-th {i32 i, x, y} of the parameter block
# row 1: column k is (w / 255, h / 255, 0, 1) of smr_dimensions(in, k - 1)
# drawn by the first plane only (the later ones add nothing), so what a pixel holds is one call's result
PROBE = r"""
struct Probe { int i, x, y; };
__device__ float4 smr_fragment(const smr_shader_in &in, int plane_id, float2 uv, float2 position) {
    if (plane_id > 0) return make_float4(0.f, 0.f, 0.f, 0.f);
    const int k = (int)position.x;
    if (position.y < 1.0f) {
        if ((unsigned int)(k + 1) * (unsigned int)sizeof(Probe) > smr_param_size(in)) return make_float4(0.f, 0.f, 0.f, 0.f);
        Probe p;
        __builtin_memcpy(&p, smr_param_bytes(in) + (size_t)k * sizeof(Probe), sizeof(Probe));
        return smr_load(in, p.i, p.x, p.y);
    }
    const uint2 d = smr_dimensions(in, k - 1);
    return make_float4((float)d.x / 255.0f, (float)d.y / 255.0f, 0.0f, 1.0f);
}
"""

# The rotating shader (examples/user_shader.c carries the same text).  The LAST source is the picture: it turns by in.time radians
# about the target's centre at 0.6 of the size that would fit, its aspect ratio kept (smr_dimensions); every source before it is a
# palette strip, drawn over the whole target as eight vertical bands whose colours are its first row's texels (smr_load).
ROTATE = r"""
#define SMR_HAS_VERTEX_AFFINE
__device__ smr_affine smr_vertex_affine(const smr_shader_in &in, int plane_id) {
    smr_affine m = {1.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f};
    if (plane_id != in.texture_count - 1) return m;
    const uint2 d = smr_dimensions(in, plane_id);
    const float W = (float)in.output_resolution.x, H = (float)in.output_resolution.y;
    const float fit = fminf(W / (float)d.x, H / (float)d.y) * 0.6f;
    const float hw = 0.5f * fit * (float)d.x, hh = 0.5f * fit * (float)d.y;  // the plane's half extent in pixels
    const float c = cosf(in.time), s = sinf(in.time);
    m.xx = 2.0f * hw * c / W; m.xy = -2.0f * hh * s / W;
    m.yx = 2.0f * hw * s / H; m.yy = 2.0f * hh * c / H;
    return m;
}
__device__ float4 smr_fragment(const smr_shader_in &in, int plane_id, float2 uv, float2 position) {
    const uint2 d = smr_dimensions(in, plane_id);
    if (plane_id != in.texture_count - 1) {
        int band = (int)(uv.x * 8.0f);
        if (band > (int)d.x - 1) band = (int)d.x - 1;
        return smr_load(in, plane_id, band, 0);
    }
    int tx = (int)floorf(uv.x * (float)d.x), ty = (int)floorf(uv.y * (float)d.y);
    if (tx > (int)d.x - 1) tx = (int)d.x - 1;
    if (ty > (int)d.y - 1) ty = (int)d.y - 1;
    return smr_load(in, plane_id, tx, ty);
}
"""

ALL = {"affine_param": AFFINE_PARAM, "plane_param": PLANE_PARAM, "tile": TILE, "probe": PROBE, "rotate": ROTATE}

BOTH_DEFINES_ERROR = "SMR_HAS_VERTEX or SMR_HAS_VERTEX_AFFINE, not both"
BOTH_DEFINES = "#define SMR_HAS_VERTEX\n" + AFFINE_PARAM
