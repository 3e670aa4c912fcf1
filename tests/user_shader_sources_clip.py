"""User shader sources for the clip vertex stage (include/smr.h "user shaders", SMR_HAS_VERTEX_CLIP): what tests/test_emu_user_shader_clip.py
runs on the lane emulator and tests/test_gpu_user_shader_clip.py on the device.  Their expected pictures follow from the contract alone (the
numpy model in the former).  No loops; nothing here is meant to fault."""
from tests.user_shader_sources_affine import _NEAREST, PLANE_PARAM

# params: six f32 {x, y, z, w, u, v} per vertex, four vertices per source: 96 B per plane, 1 536 B for 16 planes
_CLIP_VERTEX = r"""
#define SMR_HAS_VERTEX_CLIP
__device__ smr_clip_vertex smr_vertex_clip(const smr_shader_in &in, int plane_id, int vertex_index, float3 position, float2 tex_coords) {
    const int i = plane_id < 0 ? 0 : plane_id;
    float f[6];
    __builtin_memcpy(f, smr_param_bytes(in) + (size_t)((i & 15) * 4 + (vertex_index & 3)) * sizeof(f), sizeof(f));
    smr_clip_vertex o;
    o.position = make_float4(f[0], f[1], f[2], f[3]);
    o.tex_coords = make_float2(f[4], f[5]);
    return o;
}
"""

# the fragment of the affine fixtures: the texel of source plane_id nearest uv
CLIP_PARAM = _CLIP_VERTEX + _NEAREST

# a constant premultiplied colour: a pixel blended twice, or not at all, holds a different byte
CLIP_HALF = _CLIP_VERTEX + r"""
__device__ float4 smr_fragment(const smr_shader_in &in, int plane_id, float2 uv, float2 position) {
    return make_float4(0.25f, 0.5f, 0.125f, 0.5f);
}
"""

# The card shader (examples/user_shader.c carries the same text).  The LAST source is the picture: a card at 0.6 of the size that would fit
# the target, its aspect ratio kept (smr_dimensions), turning about its vertical axis by in.time radians, seen in perspective from a
# distance of 2.5 half target widths — the side that comes towards the eye grows, and from a quarter turn on the card shows its back and is
# culled.  Every source before it is a palette strip, drawn over the whole target as eight vertical bands (smr_load).
FLIP = r"""
#define SMR_HAS_VERTEX_CLIP
__device__ smr_clip_vertex smr_vertex_clip(const smr_shader_in &in, int plane_id, int vertex_index, float3 position, float2 tex_coords) {
    smr_clip_vertex o;
    o.position = make_float4(position.x, position.y, 0.0f, 1.0f);
    o.tex_coords = tex_coords;
    if (plane_id != in.texture_count - 1) return o;
    const uint2 d = smr_dimensions(in, plane_id);
    const float W = (float)in.output_resolution.x, H = (float)in.output_resolution.y;
    const float fit = fminf(W / (float)d.x, H / (float)d.y) * 0.6f;
    const float sx = fit * (float)d.x / W, sy = fit * (float)d.y / H;  // the card's half extent in clip space
    const float xr = position.x * sx * cosf(in.time), zr = position.x * sx * sinf(in.time);
    const float w = 1.0f + zr / 2.5f;
    o.position = make_float4(xr, position.y * sy, 0.5f * w, w);
    return o;
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

ALL = {"clip_param": CLIP_PARAM, "clip_half": CLIP_HALF, "flip": FLIP, "plane_param": PLANE_PARAM}

ONE_STAGE_ERROR = "one vertex stage per shader"
CLIP_ERROR = "SMR_HAS_VERTEX_CLIP or one of SMR_HAS_VERTEX and SMR_HAS_VERTEX_AFFINE, not both"
WITH_PLANE = "#define SMR_HAS_VERTEX\n" + CLIP_PARAM
WITH_AFFINE = "#define SMR_HAS_VERTEX_AFFINE\n" + CLIP_PARAM
