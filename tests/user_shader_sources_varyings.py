"""User shader sources with varyings (include/smr.h "user shaders", SMR_VARYINGS beside SMR_HAS_VERTEX_CLIP): what
tests/test_emu_user_shader_varyings.py runs on the lane emulator and tests/test_gpu_user_shader_varyings.py on the device.  Their expected
pictures follow from the contract alone (the numpy model in the former).  No loops over anything but the varyings; nothing here is meant to
fault: a NaN below is a word in a register, never part of an address."""
from tests.user_shader_sources_affine import _NEAREST
from tests.user_shader_sources_clip import _CLIP_VERTEX


def _head(n, flat=0, linear=0, clip=True):
    return ("#define SMR_HAS_VERTEX_CLIP\n" if clip else "") + f"#define SMR_VARYINGS {n}\n" + \
        (f"#define SMR_VARYINGS_FLAT {flat:#x}\n" if flat else "") + (f"#define SMR_VARYINGS_LINEAR {linear:#x}\n" if linear else "")


# params: 6 + N f32 {x, y, z, w, u, v, varyings} per vertex, four vertices per plane; at most eight planes (8 * 4 * 14 * 4 = 1 792 B at N = 8:
# sixteen planes with five varyings would need 2 816 B, more than a parameter block holds — VARY_GRID below)
_PARAM_VERTEX = r"""
__device__ smr_clip_vertex_v<SMR_VARYINGS> smr_vertex_clip(const smr_shader_in &in, int plane_id, int vertex_index, float3 position, float2 tex_coords) {
    const int i = plane_id < 0 ? 0 : plane_id;
    float f[6 + SMR_VARYINGS];
    __builtin_memcpy(f, smr_param_bytes(in) + (size_t)((i & 7) * 4 + (vertex_index & 3)) * sizeof(f), sizeof(f));
    smr_clip_vertex_v<SMR_VARYINGS> o;
    o.position = make_float4(f[0], f[1], f[2], f[3]);
    o.tex_coords = make_float2(f[4], f[5]);
    for (int j = 0; j < SMR_VARYINGS; j++) o.varyings[j] = f[6 + j];
    return o;
}
"""

# a premultiplied colour that encodes the five varyings: r from 0, scaled by 3; g from 1, scaled by one of two constants that the lowest
# bit of varying 4's word selects; b from 2; alpha 0.5, so the order of the blend shows
_ENCODE_FRAGMENT = r"""
__device__ float4 smr_fragment(const smr_shader_in &in, int plane_id, float2 uv, float4 position, const smr_varyings<SMR_VARYINGS> &v) {
    const float pick = (__float_as_uint(v.v[4]) & 1u) ? 0.75f : 0.5f;
    return make_float4(0.5f * v.v[0] * v.v[3], 0.5f * v.v[1] * pick, 0.5f * v.v[2], 0.5f);
}
"""

VARY_MODES = "PPLFF"  # varyings 0, 1 perspective, 2 linear, 3, 4 flat
VARY_PARAM = _head(5, flat=0x18, linear=0x4) + _PARAM_VERTEX + _ENCODE_FRAGMENT
# the same with varying 2 perspective: for a plane with a vertex behind the eye, where a linear varying is not compared
PERSP_MODES = "PPPFF"
VARY_PERSP = _head(5, flat=0x18) + _PARAM_VERTEX + _ENCODE_FRAGMENT

# Sixteen planes: the positions and tex_coords in CLIP_PARAM's layout (1 536 B), then eight f32 per plane (512 B: the block is full).  Varying
# j of vertex k is word j + k of the plane's eight: every vertex its own values, no arithmetic in between.
VARY_GRID = _head(5, flat=0x18, linear=0x4) + r"""
__device__ smr_clip_vertex_v<SMR_VARYINGS> smr_vertex_clip(const smr_shader_in &in, int plane_id, int vertex_index, float3 position, float2 tex_coords) {
    const int i = plane_id < 0 ? 0 : plane_id;
    float f[6], t[SMR_VARYINGS];
    __builtin_memcpy(f, smr_param_bytes(in) + (size_t)((i & 15) * 4 + (vertex_index & 3)) * sizeof(f), sizeof(f));
    __builtin_memcpy(t, smr_param_bytes(in) + 1536 + (size_t)((i & 15) * 8 + (vertex_index & 3)) * sizeof(float), sizeof(t));
    smr_clip_vertex_v<SMR_VARYINGS> o;
    o.position = make_float4(f[0], f[1], f[2], f[3]);
    o.tex_coords = make_float2(f[4], f[5]);
    for (int j = 0; j < SMR_VARYINGS; j++) o.varyings[j] = t[j];
    return o;
}
""" + _ENCODE_FRAGMENT

# @builtin(position).zw and one perspective varying; 1 / w of the planes used lies within 0.6 .. 1.7
POSITION_K = 0.5
VARY_POSITION = _head(1) + _PARAM_VERTEX + r"""
__device__ float4 smr_fragment(const smr_shader_in &in, int plane_id, float2 uv, float4 position, const smr_varyings<SMR_VARYINGS> &v) {
    return make_float4(position.z, position.w * 0.5f, v.v[0], 1.0f);
}
"""

# CLIP_PARAM with three varyings that the vertex stage writes and the fragment ignores: the same parameter block, the same picture
VARY_UNUSED = _head(3, linear=0x2) + _CLIP_VERTEX.replace("#define SMR_HAS_VERTEX_CLIP\n", "").replace("smr_clip_vertex ", "smr_clip_vertex_v<SMR_VARYINGS> ").replace(
    "    return o;", "    o.varyings[0] = f[4];\n    o.varyings[1] = f[5] + f[3];\n    o.varyings[2] = (float)vertex_index;\n    return o;") + _NEAREST.replace(
    "float2 position)", "float4 position, const smr_varyings<SMR_VARYINGS> &v)")

# one flat varying whose word is compared as an integer: a quiet NaN with a payload, and a negative denormal (flushed to zero, or moved through
# an arithmetic instruction, it would arrive as another word)
WORD_NAN, WORD_DENORMAL, WORD_OTHER = 0x7FC12345, 0x80000001, 0x3F800000
RED, GREEN, WRONG = (1.0, 0.0, 0.0, 1.0), (0.0, 1.0, 0.0, 1.0), (0.0, 0.0, 1.0, 1.0)
VARY_FLAT_BITS = _head(1, flat=0x1) + _PARAM_VERTEX + r"""
__device__ float4 smr_fragment(const smr_shader_in &in, int plane_id, float2 uv, float4 position, const smr_varyings<SMR_VARYINGS> &v) {
    const unsigned int word = __float_as_uint(v.v[0]);
    if (word == 0x7FC12345u) return make_float4(1.0f, 0.0f, 0.0f, 1.0f);
    if (word == 0x80000001u) return make_float4(0.0f, 1.0f, 0.0f, 1.0f);
    return make_float4(0.0f, 0.0f, 1.0f, 1.0f);
}
"""

# The lit card (examples/user_shader.c carries the same text): FLIP of tests/user_shader_sources_clip.py with a per-vertex normal — the card
# is slightly domed, its normals lean outwards at the corners and turn with it — as three perspective varyings, and a flat tint per
# triangle.  The fragment applies a diffuse factor from a light above and to the left of the eye.
LIT = r"""
#define SMR_HAS_VERTEX_CLIP
#define SMR_VARYINGS 4
#define SMR_VARYINGS_FLAT 0x8
__device__ smr_clip_vertex_v<SMR_VARYINGS> smr_vertex_clip(const smr_shader_in &in, int plane_id, int vertex_index, float3 position, float2 tex_coords) {
    smr_clip_vertex_v<SMR_VARYINGS> o;
    o.position = make_float4(position.x, position.y, 0.0f, 1.0f);
    o.tex_coords = tex_coords;
    o.varyings[0] = 0.0f; o.varyings[1] = 0.0f; o.varyings[2] = -1.0f;  // the normal: towards the eye
    o.varyings[3] = 1.0f;
    if (plane_id != in.texture_count - 1) return o;
    const uint2 d = smr_dimensions(in, plane_id);
    const float W = (float)in.output_resolution.x, H = (float)in.output_resolution.y;
    const float fit = fminf(W / (float)d.x, H / (float)d.y) * 0.6f;
    const float sx = fit * (float)d.x / W, sy = fit * (float)d.y / H;  // the card's half extent in clip space
    const float c = cosf(in.time), s = sinf(in.time);
    const float xr = position.x * sx * c, zr = position.x * sx * s;
    const float w = 1.0f + zr / 2.5f;
    o.position = make_float4(xr, position.y * sy, 0.5f * w, w);
    const float nx = 0.5f * position.x, ny = 0.25f * position.y, nz = -1.0f;  // leaning outwards, then turned with the card
    o.varyings[0] = nx * c - nz * s; o.varyings[1] = ny; o.varyings[2] = nx * s + nz * c;
    o.varyings[3] = vertex_index == 0 ? 1.0f : 0.875f;  // the provoking vertex's value: triangle (0, 1, 2) full, (2, 3, 0) a shade darker
    return o;
}
__device__ float4 smr_fragment(const smr_shader_in &in, int plane_id, float2 uv, float4 position, const smr_varyings<SMR_VARYINGS> &v) {
    const uint2 d = smr_dimensions(in, plane_id);
    if (plane_id != in.texture_count - 1) {
        int band = (int)(uv.x * 8.0f);
        if (band > (int)d.x - 1) band = (int)d.x - 1;
        return smr_load(in, plane_id, band, 0);
    }
    int tx = (int)floorf(uv.x * (float)d.x), ty = (int)floorf(uv.y * (float)d.y);
    if (tx > (int)d.x - 1) tx = (int)d.x - 1;
    if (ty > (int)d.y - 1) ty = (int)d.y - 1;
    const float4 texel = smr_load(in, plane_id, tx, ty);
    const float len = sqrtf(v.v[0] * v.v[0] + v.v[1] * v.v[1] + v.v[2] * v.v[2]);
    const float diffuse = fmaxf((v.v[0] * -0.48f + v.v[1] * 0.6f + v.v[2] * -0.64f) / len, 0.0f);  // the light's direction is a unit vector
    const float k = (0.25f + 0.75f * diffuse) * v.v[3];
    return make_float4(texel.x * k, texel.y * k, texel.z * k, texel.w);
}
"""

ALL = {"vary_param": VARY_PARAM, "vary_persp": VARY_PERSP, "vary_grid": VARY_GRID, "vary_position": VARY_POSITION, "vary_unused": VARY_UNUSED,
       "vary_flat_bits": VARY_FLAT_BITS, "lit": LIT}

# sources that do not compile, and what smr_shader_program_log says about each
_OLD_FRAGMENT = r"""
__device__ float4 smr_fragment(const smr_shader_in &in, int plane_id, float2 uv, float2 position) {
    return make_float4(0.25f, 0.5f, 0.125f, 0.5f);
}
"""
_BODY = _PARAM_VERTEX + VARY_POSITION[VARY_POSITION.index("__device__ float4 smr_fragment"):]
BROKEN = {
    "without_the_clip_stage": (_head(2, clip=False) + _OLD_FRAGMENT, "SMR_VARYINGS needs the clip vertex stage"),
    "no_varyings": (_head(0) + _BODY, "SMR_VARYINGS is the number of f32 varyings, 1 to 8"),
    "nine_varyings": (_head(9) + _BODY, "SMR_VARYINGS is the number of f32 varyings, 1 to 8"),
    "a_mask_bit_at_n": (_head(3, flat=0x8) + _BODY, "bits at or above SMR_VARYINGS are not allowed"),
    "a_bit_in_both_masks": (_head(3, flat=0x1, linear=0x5) + _BODY, "a varying is flat or linear, not both"),
}
