"""User shader sources that use screen-space derivatives (include/smr.h "user shaders", SMR_DERIVATIVES): what
tests/test_emu_user_shader_derivatives.py runs on the lane emulator and tests/test_gpu_user_shader_derivatives.py on the device.  Their
expected pictures follow from the contract alone (the numpy model in the former).  Every derivative is called in control flow that is
uniform across the quad (before any branch of the fragment); each fixture scales a derivative into mid-range, 0.5 + k * d or k * d, so that
the f32-against-f64 error of the difference (a few 1e-7 of the differenced value) times k stays far under one LSB (3.9e-3).  No loops; nothing
here is meant to fault: a helper's extrapolated value is a register, never an address."""
from tests.user_shader_sources_affine import _NEAREST, AFFINE_PARAM, PLANE_PARAM
from tests.user_shader_sources_clip import CLIP_PARAM
from tests.user_shader_sources_varyings import _PARAM_VERTEX, VARY_PARAM, _head

DEFINE = "#define SMR_DERIVATIVES\n"
FLAVOURS = {"plain": "", "fine": "_fine", "coarse": "_coarse"}

# case 1: (dpdx(position.x), dpdy(position.y), dpdx(position.y), dpdy(position.x)) = (1, 1, 0, 0) on every pixel.  No vertex stage
_POSITION = DEFINE + r"""
__device__ float4 smr_fragment(const smr_shader_in &in, int plane_id, float2 uv, float2 position) {
    return make_float4(smr_dpdx@(position.x), smr_dpdy@(position.y), smr_dpdx@(position.y), smr_dpdy@(position.x));
}
"""

# case 2: an smr_plane from the parameter block; (0.5 + 8 dpdx(uv.x), 0.5 + dpdy(uv.y), 0.5 + dpdy(uv.x) + dpdx(uv.y), 1).  On a plane of
# 32 x 4 pixels with dyadic edges every value is exact: (0.75, 0.75, 0.5, 1)
EDGE_KX, EDGE_KY = 8.0, 1.0
_EDGE = DEFINE + PLANE_PARAM[:PLANE_PARAM.index("__device__ float4 smr_fragment")] + r"""
__device__ float4 smr_fragment(const smr_shader_in &in, int plane_id, float2 uv, float2 position) {
    const float2 dx = smr_dpdx@(uv), dy = smr_dpdy@(uv);
    return make_float4(0.5f + 8.0f * dx.x, 0.5f + dy.y, 0.5f + dy.x + dx.y, 1.0f);
}
"""

# case 3: t = position.x * position.y (exact: half-integers below 8); (fine, coarse, plain) derivative of t along one axis, / 8
_PRODUCT = DEFINE + r"""
__device__ float4 smr_fragment(const smr_shader_in &in, int plane_id, float2 uv, float2 position) {
    const float t = position.x * position.y;
    return make_float4(smr_dpd@_fine(t) * 0.125f, smr_dpd@_coarse(t) * 0.125f, smr_dpd@(t) * 0.125f, 1.0f);
}
"""

# case 4, the renderer case and the example (examples/user_shader.c carries the same text): every source drawn over the whole target through
# an anti-aliased disc — centre a little off the target's, radius 0.4 of its smaller side — whose edge is one pixel wide at any size: the
# distance to the edge in units of its own screen-space footprint, smr_fwidth.  The texel is the nearest one (smr_dimensions + smr_load).
DISC = r"""
#define SMR_DERIVATIVES
__device__ float4 smr_fragment(const smr_shader_in &in, int plane_id, float2 uv, float2 position) {
    const float W = (float)in.output_resolution.x, H = (float)in.output_resolution.y;
    const float dx = position.x - (0.5f * W + 0.3f), dy = position.y - (0.5f * H + 0.1f);
    const float d = sqrtf(dx * dx + dy * dy);
    const float footprint = smr_fwidth(d);  // (before any branch: a derivative wants the whole quad)
    const float cover = fminf(fmaxf(0.5f - (d - 0.4f * fminf(W, H)) / footprint, 0.0f), 1.0f);
    const uint2 s = smr_dimensions(in, plane_id);
    int tx = (int)floorf(uv.x * (float)s.x), ty = (int)floorf(uv.y * (float)s.y);
    if (tx > (int)s.x - 1) tx = (int)s.x - 1;
    if (ty > (int)s.y - 1) ty = (int)s.y - 1;
    const float4 t = smr_load(in, plane_id, tx, ty);
    return make_float4(t.x * cover, t.y * cover, t.z * cover, t.w * cover);
}
"""

# case 5: the affine stage from the parameter block.  Plane 0 is the nearest texel; every later plane is half transparent and shows
# fwidth(uv) in red and green (k = 1: the narrowest plane used is 2.5 pixels, fwidth below 0.75) over its texel's blue
OVERLAP = DEFINE + AFFINE_PARAM[:AFFINE_PARAM.index("__device__ float4 smr_fragment")] + r"""
__device__ float4 smr_fragment(const smr_shader_in &in, int plane_id, float2 uv, float2 position) {
    const float2 fw = smr_fwidth(uv);
    const uint2 d = smr_dimensions(in, plane_id);
    int tx = (int)floorf(uv.x * (float)d.x), ty = (int)floorf(uv.y * (float)d.y);
    if (tx > (int)d.x - 1) tx = (int)d.x - 1;
    if (ty > (int)d.y - 1) ty = (int)d.y - 1;
    const float4 t = smr_load(in, plane_id, tx, ty);
    if (plane_id < 1) return t;
    return make_float4(0.5f * (0.25f + fw.x), 0.5f * (0.25f + fw.y), 0.5f * t.z, 0.5f);
}
"""

# case 6: the clip stage with five varyings (three perspective, two flat: VARY_PERSP's head and vertex stage).  Half transparent:
# red 0.5 + k dpdx(u), green 0.5 + k dpdy(v) (coarse), blue 0.5 + k * the FINE dpdx of the perspective varying 0
PERSPECTIVE_K = 0.75
PERSPECTIVE = DEFINE + _head(5, flat=0x18) + _PARAM_VERTEX + r"""
__device__ float4 smr_fragment(const smr_shader_in &in, int plane_id, float2 uv, float4 position, const smr_varyings<SMR_VARYINGS> &v) {
    const float2 dx = smr_dpdx(uv), dy = smr_dpdy(uv);
    const float dv = smr_dpdx_fine(v.v[0]);
    return make_float4(0.5f * (0.5f + 0.75f * dx.x), 0.5f * (0.5f + 0.75f * dy.y), 0.5f * (0.5f + 0.75f * dv), 0.5f);
}
"""

ALL = {"disc": DISC, "overlap": OVERLAP, "perspective": PERSPECTIVE}
for _name, _suffix in FLAVOURS.items():
    ALL[f"position_{_name}"] = _POSITION.replace("@", _suffix)
    ALL[f"edge_{_name}"] = _EDGE.replace("@", _suffix)
for _axis in "xy":
    ALL[f"product_{_axis}"] = _PRODUCT.replace("@", _axis)

# case 7: an existing fixture per stage with the macro and no derivative call: the same picture from the other lane map
ORIGINALS = {"plane_param": PLANE_PARAM, "affine_param": AFFINE_PARAM, "clip_param": CLIP_PARAM, "vary_param": VARY_PARAM}
for _name, _src in ORIGINALS.items():
    ALL[f"remap_{_name}"] = DEFINE + _src

# case 8: a derivative call without the macro
MISUSE = {name: src.replace(DEFINE, "") for name, src in ALL.items() if name in ("position_plain", "edge_fine", "product_x", "disc", "perspective")}
MISUSE_ERROR = "SMR_DERIVATIVES"
