"""User shader sources for the tests (include/smr.h "user shaders"): the library's seven built-in plane shaders restated from
smelter_amd/csrc/smr_shaders.hip in the user-shader language, and original ones whose output follows from the contract alone.  Loops,
where there are any, have small constant bounds; nothing here is meant to fault."""

GRADIENT = r"""
__device__ float4 smr_fragment(const smr_shader_in &in, int plane_id, float2 uv, float2 position) {
    return make_float4(uv.x, 0.0f, 0.0f, 1.0f);
}
"""

RED_BORDER = r"""
__device__ float4 smr_fragment(const smr_shader_in &in, int plane_id, float2 uv, float2 position) {
    const float4 sample = smr_sample(in, 0, uv.x, uv.y);
    const float border = 50.0f;
    const float fx = position.x, fy = position.y;
    if (fx > border && fx < (float)in.output_resolution.x - border && fy > border && fy < (float)in.output_resolution.y - border) return sample;
    return make_float4(1.0f, 0.0f, 0.0f, 1.0f);
}
"""

# params: one {u32 left_px, top_px, width_px, height_px; f32 background_color[4]} per source
CIRCLE_LAYOUT = r"""
#define SMR_HAS_VERTEX
struct Circle { unsigned int left_px, top_px, width_px, height_px; float background_color[4]; };

__device__ Circle circle_of(const smr_shader_in &in, int plane_id) {
    const int i = plane_id < 0 ? 0 : plane_id;
    Circle c;
    __builtin_memcpy(&c, smr_param_bytes(in) + (size_t)(i & 15) * sizeof(Circle), sizeof(Circle));
    return c;
}

__device__ smr_plane smr_vertex(const smr_shader_in &in, int plane_id) {
    const Circle c = circle_of(in, plane_id);
    const float W = (float)in.output_resolution.x, H = (float)in.output_resolution.y;
    smr_plane p;
    p.sx = (float)c.width_px / W;
    p.sy = (float)c.height_px / H;
    p.cx = (((float)c.left_px + ((float)c.width_px / 2.0f)) / W) * 2.0f - 1.0f;
    p.cy = 1.0f - (((float)c.top_px + ((float)c.height_px / 2.0f)) / H) * 2.0f;
    return p;
}

__device__ float4 smr_fragment(const smr_shader_in &in, int plane_id, float2 uv, float2 position) {
    const Circle c = circle_of(in, plane_id);
    const float du = uv.x - 0.5f, dv = uv.y - 0.5f;
    const float in_circle = sqrtf(du * du + dv * dv) < 0.5f ? 1.0f : 0.0f;
    const float4 s = smr_sample(in, plane_id, uv.x, uv.y);
    return make_float4(s.x * in_circle + c.background_color[0] * (1.0f - in_circle), s.y * in_circle + c.background_color[1] * (1.0f - in_circle),
                       s.z * in_circle + c.background_color[2] * (1.0f - in_circle), s.w * in_circle + c.background_color[3] * (1.0f - in_circle));
}
"""

FADE_TO_BALL = r"""
__device__ float4 smr_fragment(const smr_shader_in &in, int plane_id, float2 uv, float2 position) {
    const float4 s = smr_sample(in, 0, uv.x, uv.y);
    const float radius = in.time / 5.0f, eps = 0.15f;
    const float du = uv.x - 0.5f, dv = uv.y - 0.5f;
    const float t = smr_smoothstep(radius + eps, radius - eps, sqrtf(du * du + dv * dv));
    return make_float4(s.x * t, s.y * t, s.z * t, s.w * t);
}
"""

LAYOUT_PLANES = r"""
#define SMR_HAS_VERTEX
__device__ smr_plane smr_vertex(const smr_shader_in &in, int plane_id) {
    smr_plane p = {1.0f, 1.0f, 0.0f, 0.0f};
    if (plane_id != -1) {
        p.sx = 0.5f; p.sy = 0.5f;
        if (plane_id == 0) { p.cx = -0.5f; p.cy = 0.5f; }
        else if (plane_id == 1) { p.cx = 0.5f; p.cy = 0.5f; }
        else if (plane_id == 2) { p.cx = -0.5f; p.cy = -0.5f; }
        else if (plane_id == 3) { p.cx = 0.5f; p.cy = -0.5f; }
    }
    return p;
}

__device__ float4 smr_fragment(const smr_shader_in &in, int plane_id, float2 uv, float2 position) {
    if (plane_id == -1) return make_float4(1.0f, 0.0f, 0.0f, 1.0f);
    return smr_sample(in, plane_id, uv.x, uv.y);
}
"""

COLOR_BY_TEXTURE_COUNT = r"""
__device__ float4 smr_fragment(const smr_shader_in &in, int plane_id, float2 uv, float2 position) {
    if (in.texture_count == 0) return make_float4(1.0f, 0.0f, 0.0f, 1.0f);
    if (in.texture_count == 1) return make_float4(0.0f, 1.0f, 0.0f, 1.0f);
    return make_float4(0.0f, 0.0f, 1.0f, 1.0f);
}
"""

SILLY = r"""
__device__ float4 smr_fragment(const smr_shader_in &in, int plane_id, float2 uv, float2 position) {
    if (in.texture_count != 1) return make_float4(0.f, 0.f, 0.f, 0.f);
    const float pi = 3.14159f;
    const float effect_radius = fabsf(sinf(in.time) / 2.0f);
    const float effect_angle = 2.0f * pi * fabsf(sinf(in.time) / 2.0f);
    const float du = uv.x - 0.5f, dv = uv.y - 0.5f;
    const float len = sqrtf(du * du + dv * dv);
    const float angle = atan2f(dv, du) + effect_angle * smr_smoothstep(effect_radius, 0.0f, len);
    return smr_sample(in, 0, len * cosf(angle) + 0.5f, len * sinf(angle) + 0.5f);
}
"""

# name -> (source, smr_builtin_shader_id): what Context.builtin_shader / orc.builtin_shader call the same arithmetic
RESTATED = {
    "gradient": (GRADIENT, 1),
    "red_border": (RED_BORDER, 2),
    "circle_layout": (CIRCLE_LAYOUT, 3),
    "fade_to_ball": (FADE_TO_BALL, 4),
    "layout_planes": (LAYOUT_PLANES, 5),
    "color_by_texture_count": (COLOR_BY_TEXTURE_COUNT, 6),
    "silly": (SILLY, 7),
}

# ---- original shaders

# red and blue of source 0 change places.  On a source of the target's size every sample lands on a texel centre (sub-texel weights 0):
# decode and encode are inverse on 8-bit codes, so the output is tex[..., [2, 1, 0, 3]] exactly, in both rendering modes.
SWAP_RB = r"""
__device__ float4 smr_fragment(const smr_shader_in &in, int plane_id, float2 uv, float2 position) {
    const float4 s = smr_sample(in, 0, uv.x, uv.y);
    return make_float4(s.z, s.y, s.x, s.w);
}
"""

# no children: every pixel is the four f32 of the parameter block
PARAM_FILL = r"""
struct Fill { float r, g, b, a; };
__device__ float4 smr_fragment(const smr_shader_in &in, int plane_id, float2 uv, float2 position) {
    const Fill f = smr_param<Fill>(in);
    return make_float4(f.r, f.g, f.b, f.a);
}
"""

# SMR_HAS_VERTEX: source i fills quadrant i (row-major from the top left) with the constant colour i names; sources beyond four cover nothing
QUADRANT_COLORS = r"""
#define SMR_HAS_VERTEX
__device__ smr_plane smr_vertex(const smr_shader_in &in, int plane_id) {
    smr_plane p = {0.0f, 0.0f, 0.0f, 0.0f};
    if (plane_id < 0 || plane_id > 3) return p;
    p.sx = 0.5f; p.sy = 0.5f;
    p.cx = (plane_id & 1) ? 0.5f : -0.5f;
    p.cy = (plane_id & 2) ? -0.5f : 0.5f;
    return p;
}
__device__ float4 smr_fragment(const smr_shader_in &in, int plane_id, float2 uv, float2 position) {
    return make_float4(plane_id == 0 ? 1.0f : 0.0f, plane_id == 1 ? 1.0f : 0.0f, plane_id == 2 ? 1.0f : 0.0f, 1.0f);
}
"""

# a struct-list parameter: one {u32 first_row, rows; f32 color[4]} per band (the list's length is smr_param_size / 24, eight at most);
# a pixel takes the colour of the last band that holds its row, transparent outside every band
BANDS = r"""
struct Band { unsigned int first_row, rows; float color[4]; };
__device__ float4 smr_fragment(const smr_shader_in &in, int plane_id, float2 uv, float2 position) {
    const unsigned int n = smr_param_size(in) / (unsigned int)sizeof(Band);
    const unsigned int row = (unsigned int)position.y;
    float4 out = make_float4(0.f, 0.f, 0.f, 0.f);
    for (unsigned int i = 0; i < 8; i++) {
        if (i >= n) break;
        Band b;
        __builtin_memcpy(&b, smr_param_bytes(in) + i * sizeof(Band), sizeof(Band));
        if (row >= b.first_row && row < b.first_row + b.rows) out = make_float4(b.color[0], b.color[1], b.color[2], b.color[3]);
    }
    return out;
}
"""

# the renderer scene's shader: CIRCLE_LAYOUT above with TWO circle lists in its struct-list parameter (texture_count entries each) — the
# first while in.time < 1 s, the second from then on.  So the oracle of circle_layout, handed the list of the moment, is its oracle too.
CIRCLES_BY_TIME = CIRCLE_LAYOUT.replace("const int i = plane_id < 0 ? 0 : plane_id;",
                                        "const int i = (plane_id < 0 ? 0 : plane_id) + (in.time >= 1.0f ? (in.texture_count > 0 ? in.texture_count : 1) : 0);")
assert CIRCLES_BY_TIME != CIRCLE_LAYOUT

ORIGINAL = {"swap_rb": SWAP_RB, "param_fill": PARAM_FILL, "quadrant_colors": QUADRANT_COLORS, "bands": BANDS, "circles_by_time": CIRCLES_BY_TIME}
ALL = dict({k: v[0] for k, v in RESTATED.items()}, **ORIGINAL)

# ---- sources that must NOT compile (host-only tests): name -> (source, what the log must mention)
BROKEN = {
    "syntax_error": ("__device__ float4 smr_fragment(const smr_shader_in &in, int plane_id, float2 uv, float2 position) {\n"
                     "    return make_float4(uv.x, 0.0f, 0.0f 1.0f);\n}\n", ["shader:2"]),
    "no_fragment": ("__device__ float4 my_fragment(const smr_shader_in &in, int plane_id, float2 uv, float2 position) {\n"
                    "    return make_float4(0.f, 0.f, 0.f, 1.f);\n}\n", ["smr_fragment"]),
    "unknown_identifier": ("__device__ float4 smr_fragment(const smr_shader_in &in, int plane_id, float2 uv, float2 position) {\n"
                           "    return smr_sample_nearest(in, 0, uv.x, uv.y);\n}\n", ["smr_sample_nearest", "shader:2"]),
}
