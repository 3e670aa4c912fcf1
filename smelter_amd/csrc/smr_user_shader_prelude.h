// smr_user_shader_prelude.h — what the library puts around a user shader (include/smr.h "user shaders").
// A program is compiled from
//     #include "smr_shader_dev.h"              the texel helpers of the built-in shaders, the same text
//     #include "smr_user_shader_prelude.h"     PART 1: smr_shader_in, smr_plane, smr_affine, the accessors
//     <the user's translation unit>            smr_fragment, optionally smr_vertex, smr_vertex_affine or smr_vertex_clip (with SMR_VARYINGS: varyings)
//     #define SMR_USER_SHADER_KERNEL
//     #include "smr_user_shader_prelude.h"     PART 2: the kernel — k_shader_planes (smr_shaders.hip) with its two switches replaced by
//                                              calls to the user's functions
// by the ROCm runtime compiler with the library's own flags; the lane emulator (tests/emu/emu_user_shader.cpp) includes the same file
// the same way for the host compiler.  No `#pragma once`: the file is read twice on purpose.
#ifndef SMR_USER_SHADER_KERNEL
// ---------------------------------------------------------------------------------------------------------------------- PART 1

// BaseShaderParameters (shader/base_params.rs:7-12) without plane_id, which is an argument of the stages.  The members below the
// three public ones belong to the accessors: a user function reaches surfaces only through smr_sample, smr_load and smr_dimensions.
struct smr_shader_in;
__device__ __forceinline__ float4 smr_sample(const smr_shader_in &in, int i, float u, float v);
__device__ __forceinline__ uint2 smr_dimensions(const smr_shader_in &in, int i);
__device__ __forceinline__ float4 smr_load(const smr_shader_in &in, int i, int x, int y);
__device__ __forceinline__ const unsigned char *smr_param_bytes(const smr_shader_in &in);
__device__ __forceinline__ unsigned int smr_param_size(const smr_shader_in &in);
struct smr_shader_in {
    float time;               // pts of the frame in seconds
    uint2 output_resolution;  // of the target
    int texture_count;        // sources of this pass: plane_id runs 0 .. texture_count - 1, or is -1 when there is none

    __device__ smr_shader_in(const UserShaderArgs &a, const float *dec) : time(a.time), texture_count(a.n_src), args_(a), dec_(dec) {
        output_resolution.x = (u32)a.dst.w;
        output_resolution.y = (u32)a.dst.h;
    }

private:
    const UserShaderArgs &args_;
    const float *dec_;
    friend __device__ float4 smr_sample(const smr_shader_in &in, int i, float u, float v);
    friend __device__ uint2 smr_dimensions(const smr_shader_in &in, int i);
    friend __device__ float4 smr_load(const smr_shader_in &in, int i, int x, int y);
    friend __device__ const unsigned char *smr_param_bytes(const smr_shader_in &in);
    friend __device__ unsigned int smr_param_size(const smr_shader_in &in);
};

// vertex stage: clip-space position of the unit quad's corner (x, y) = position * (sx, sy) + (cx, cy)
struct smr_plane {
    float sx, sy, cx, cy;
};

// affine vertex stage: corner (px, py) of the unit quad, px, py in {-1, +1}, goes to clip space
//   X = xx * px + xy * py + cx,   Y = yx * px + yy * py + cy          (any parallelogram; no perspective)
struct smr_affine {
    float xx, xy, yx, yy, cx, cy;
};

// clip vertex stage (SMR_HAS_VERTEX_CLIP): what smr_vertex_clip returns for one vertex of the quad — the homogeneous clip-space position
// (x, y, z, w) and the tex_coords varying, interpolated perspective-correct over the quad's two triangles (include/smr.h)
struct smr_clip_vertex {
    float4 position;
    float2 tex_coords;
};

// varyings (SMR_VARYINGS N beside SMR_HAS_VERTEX_CLIP, 1 <= N <= 8: f32 varyings 0 .. N - 1; include/smr.h).  Part 1 is read before the user's text
// and cannot see N: the carriers are templates, the user names them smr_clip_vertex_v<SMR_VARYINGS> and smr_varyings<SMR_VARYINGS>
template <int N>
struct smr_clip_vertex_v {
    float4 position;
    float2 tex_coords;
    float varyings[N];
};
template <int N>
struct smr_varyings {
    float v[N];
};

// textureSample(textures[i], linear clamp-to-edge sampler, (u, v)): premultiplied RGBA in the target's blending space (linear light in
// SMR_MODE_GPU_OPTIMIZED, the unorm values in SMR_MODE_CPU_OPTIMIZED); (0, 0, 0, 0) when i is out of range or the source is absent
__device__ __forceinline__ float4 smr_sample(const smr_shader_in &in, int i, float u, float v) {
    if (i < 0 || i >= in.args_.n_src || i >= SMR_USER_SHADER_SOURCES || !in.args_.src[i].ptr) return make_float4(0.f, 0.f, 0.f, 0.f);
    return sample_rgba_bilinear(in.args_.src[i], in.args_.pxi, u, v, in.dec_);
}

// textureDimensions(textures[i]): (0, 0) when i is out of range or the source is absent
__device__ __forceinline__ uint2 smr_dimensions(const smr_shader_in &in, int i) {
    if (i < 0 || i >= in.args_.n_src || i >= SMR_USER_SHADER_SOURCES || !in.args_.src[i].ptr) return make_uint2(0u, 0u);
    return make_uint2((u32)in.args_.src[i].w, (u32)in.args_.src[i].h);
}

// textureLoad(textures[i], (x, y), 0): the one texel, unfiltered, decoded to the blending space as smr_sample decodes its four;
// (0, 0, 0, 0) when i is out of range, the source is absent or (x, y) lies outside it — the surface is never read outside
__device__ __forceinline__ float4 smr_load(const smr_shader_in &in, int i, int x, int y) {
    if (i < 0 || i >= in.args_.n_src || i >= SMR_USER_SHADER_SOURCES || !in.args_.src[i].ptr) return make_float4(0.f, 0.f, 0.f, 0.f);
    const SurfView &s = in.args_.src[i];
    if (x < 0 || y < 0 || x >= s.w || y >= s.h) return make_float4(0.f, 0.f, 0.f, 0.f);
    return load_texel(s, in.args_.pxi, x, y, in.dec_);
}

// the @group(1) uniform: ShaderParam::to_bytes — the values in order, little endian, no padding; bytes behind smr_param_size() read 0
__device__ __forceinline__ const unsigned char *smr_param_bytes(const smr_shader_in &in) { return (const unsigned char *)in.args_.params; }
__device__ __forceinline__ unsigned int smr_param_size(const smr_shader_in &in) { return in.args_.param_size; }
template <typename T>
__device__ __forceinline__ T smr_param(const smr_shader_in &in) {
    static_assert(sizeof(T) <= SMR_USER_SHADER_PARAM_BYTES, "a shader parameter block holds at most SMR_SHADER_MAX_PARAM_BYTES bytes");
    T v;
    __builtin_memcpy(&v, smr_param_bytes(in), sizeof(T));
    return v;
}

__device__ __forceinline__ float smr_smoothstep(float e0, float e1, float x) {
    // WGSL smoothstep: t = clamp((x - e0) / (e1 - e0), 0, 1); t * t * (3 - 2 t)  (edges may be given high-to-low)
    float t = clampf((x - e0) / (e1 - e0), 0.0f, 1.0f);
    return t * t * (3.0f - 2.0f * t);
}

// screen-space derivatives on 2 x 2 pixel quads (a shader that puts `#define SMR_DERIVATIVES` at its top; include/smr.h): WGSL's dpdx, dpdy,
// fwidth and their Fine / Coarse forms, of a float or, component by component, a float2.  Callable from smr_fragment only.  Part 1 is read
// before the user's text and cannot see the macro: the eighteen functions are templates with a defaulted parameter (a call names none),
// declared here and defined in part 2 — with the macro by quad exchanges, without it by a static_assert that names the macro.
template <typename T>
struct smr_derivatives_enabled { static constexpr bool value = false; };
#define SMR_DERIVATIVE_DECLARE(name)                                  \
    template <typename T = void> __device__ __forceinline__ float name(float v); \
    template <typename T = void> __device__ __forceinline__ float2 name(float2 v);
SMR_DERIVATIVE_DECLARE(smr_dpdx) SMR_DERIVATIVE_DECLARE(smr_dpdy) SMR_DERIVATIVE_DECLARE(smr_fwidth)
SMR_DERIVATIVE_DECLARE(smr_dpdx_fine) SMR_DERIVATIVE_DECLARE(smr_dpdy_fine) SMR_DERIVATIVE_DECLARE(smr_fwidth_fine)
SMR_DERIVATIVE_DECLARE(smr_dpdx_coarse) SMR_DERIVATIVE_DECLARE(smr_dpdy_coarse) SMR_DERIVATIVE_DECLARE(smr_fwidth_coarse)
#undef SMR_DERIVATIVE_DECLARE

// what the user's translation unit defines (with SMR_VARYINGS it defines the overload that part 2 declares, and this one stays undefined)
__device__ float4 smr_fragment(const smr_shader_in &in, int plane_id, float2 uv, float2 position);

#else
// ---------------------------------------------------------------------------------------------------------------------- PART 2
#if defined(SMR_HAS_VERTEX) && defined(SMR_HAS_VERTEX_AFFINE)
#error "a shader defines SMR_HAS_VERTEX or SMR_HAS_VERTEX_AFFINE, not both: one vertex stage per shader"
#endif
#if defined(SMR_HAS_VERTEX_CLIP) && (defined(SMR_HAS_VERTEX) || defined(SMR_HAS_VERTEX_AFFINE))
#error "a shader defines SMR_HAS_VERTEX_CLIP or one of SMR_HAS_VERTEX and SMR_HAS_VERTEX_AFFINE, not both: one vertex stage per shader"
#endif
#ifdef SMR_VARYINGS
#ifndef SMR_HAS_VERTEX_CLIP
#error "SMR_VARYINGS needs the clip vertex stage: only a shader that defines SMR_HAS_VERTEX_CLIP has per-vertex calls"
#endif
#if SMR_VARYINGS < 1 || SMR_VARYINGS > 8
#error "SMR_VARYINGS is the number of f32 varyings, 1 to 8"
#endif
#ifndef SMR_VARYINGS_FLAT
#define SMR_VARYINGS_FLAT 0
#endif
#ifndef SMR_VARYINGS_LINEAR
#define SMR_VARYINGS_LINEAR 0
#endif
#if ((SMR_VARYINGS_FLAT) | (SMR_VARYINGS_LINEAR)) >> (SMR_VARYINGS)
#error "SMR_VARYINGS_FLAT and SMR_VARYINGS_LINEAR have a bit per varying: bits at or above SMR_VARYINGS are not allowed"
#endif
#if (SMR_VARYINGS_FLAT) & (SMR_VARYINGS_LINEAR)
#error "a varying is flat or linear, not both: SMR_VARYINGS_FLAT and SMR_VARYINGS_LINEAR share a bit"
#endif
#endif
#ifdef SMR_HAS_VERTEX
__device__ smr_plane smr_vertex(const smr_shader_in &in, int plane_id);
#endif
#ifdef SMR_HAS_VERTEX_AFFINE
__device__ smr_affine smr_vertex_affine(const smr_shader_in &in, int plane_id);
#endif

#ifdef SMR_DERIVATIVES
// ------------------------------------------------------------------------------------------------- derivatives: quad mode
// With SMR_DERIVATIVES the 64 x 4 pixels of a workgroup are dealt out in 2 x 2 quads, aligned to even target coordinates: wave w covers the
// 32 x 2 block at (32 (w & 1), 2 (w >> 1)), lane l is pixel (2 (l >> 2) + (l & 1), (l >> 1) & 1) of it — four consecutive lanes are the quad
//     a = (x0, y0)   b = (x0 + 1, y0)   c = (x0, y0 + 1)   d = (x0 + 1, y0 + 1)          lanes 0, 1, 2, 3 of the quad
// which is what v_mov_b32_dpp quad_perm permutes: a neighbour's value is one register move away, no LDS, no ds_bpermute.  No lane leaves for
// being outside the target or outside a plane: per plane (per triangle) the fragment function runs on all four lanes of every quad with a
// covered pixel — the others are HELPERS, whose inputs are the same formulas at their own pixel centres, whose result is dropped, and
// which neither store to the target nor load from it.  row_mask = bank_mask = 0xf; bound_ctrl: a disabled lane reads as 0 (a derivative
// called where the quad's control flow has diverged is unspecified — and only ever a value, never an address).
#ifdef SMR_EMU
#define SMR_QUAD_PERM(x, ctrl) dev_mov_dpp_quad_perm((x), (ctrl))  // (the lane emulator's: tests/emu/emu_user_shader_quad.cpp)
#else
#define SMR_QUAD_PERM(x, ctrl) __builtin_amdgcn_mov_dpp((x), (ctrl), 0xf, 0xf, true)
#endif
// quad_perm control c: lane k of the quad reads lane (c >> 2 k) & 3.  0x00 / 0x55 / 0xAA: lanes 0 / 1 / 2 for all four
template <int CTRL>
__device__ __forceinline__ float smr_quad_read(float v) {
    return __int_as_float(SMR_QUAD_PERM(__float_as_int(v), CTRL));
}
// does any pixel of the quad hold `c`?  Two exchanges: with the horizontal neighbour [1, 0, 3, 2], then with the other row [2, 3, 0, 1].  Called
// with all of the wave's lanes active
__device__ __forceinline__ bool smr_quad_any(bool c) {
    int m = c ? 1 : 0;
    m |= SMR_QUAD_PERM(m, 0xB1);
    m |= SMR_QUAD_PERM(m, 0x4E);
    return m != 0;
}
// Each derivative is ONE f32 subtraction.  Coarse: b - a and c - a for all four pixels.  Fine: the pixel's own row's right minus left
// ([1, 1, 3, 3] - [0, 0, 2, 2]), its own column's lower minus upper ([2, 3, 2, 3] - [0, 1, 0, 1]).  Window y grows downwards.  The plain forms are
// the coarse ones (a definition: include/smr.h).  fwidth = |dpdx| + |dpdy| of the same flavour.
template <typename T> __device__ __forceinline__ float smr_dpdx_coarse(float v) { return smr_quad_read<0x55>(v) - smr_quad_read<0x00>(v); }
template <typename T> __device__ __forceinline__ float smr_dpdy_coarse(float v) { return smr_quad_read<0xAA>(v) - smr_quad_read<0x00>(v); }
template <typename T> __device__ __forceinline__ float smr_dpdx_fine(float v) { return smr_quad_read<0xF5>(v) - smr_quad_read<0xA0>(v); }
template <typename T> __device__ __forceinline__ float smr_dpdy_fine(float v) { return smr_quad_read<0xEE>(v) - smr_quad_read<0x44>(v); }
template <typename T> __device__ __forceinline__ float smr_dpdx(float v) { return smr_dpdx_coarse<T>(v); }
template <typename T> __device__ __forceinline__ float smr_dpdy(float v) { return smr_dpdy_coarse<T>(v); }
template <typename T> __device__ __forceinline__ float smr_fwidth_coarse(float v) { return __builtin_fabsf(smr_dpdx_coarse<T>(v)) + __builtin_fabsf(smr_dpdy_coarse<T>(v)); }
template <typename T> __device__ __forceinline__ float smr_fwidth_fine(float v) { return __builtin_fabsf(smr_dpdx_fine<T>(v)) + __builtin_fabsf(smr_dpdy_fine<T>(v)); }
template <typename T> __device__ __forceinline__ float smr_fwidth(float v) { return smr_fwidth_coarse<T>(v); }
#define SMR_DERIVATIVE_DEFINE(name) \
    template <typename T> __device__ __forceinline__ float2 name(float2 v) { return make_float2(name<T>(v.x), name<T>(v.y)); }
#else
#define SMR_DERIVATIVE_DEFINE(name)                                                                                                              \
    template <typename T> __device__ __forceinline__ float name(float) {                                                                         \
        static_assert(smr_derivatives_enabled<T>::value, #name ": derivatives need `#define SMR_DERIVATIVES` at the top of the shader source"); \
        return 0.0f;                                                                                                                             \
    }                                                                                                                                            \
    template <typename T> __device__ __forceinline__ float2 name(float2) {                                                                       \
        static_assert(smr_derivatives_enabled<T>::value, #name ": derivatives need `#define SMR_DERIVATIVES` at the top of the shader source"); \
        return make_float2(0.0f, 0.0f);                                                                                                          \
    }
#endif
SMR_DERIVATIVE_DEFINE(smr_dpdx) SMR_DERIVATIVE_DEFINE(smr_dpdy) SMR_DERIVATIVE_DEFINE(smr_fwidth)
SMR_DERIVATIVE_DEFINE(smr_dpdx_fine) SMR_DERIVATIVE_DEFINE(smr_dpdy_fine) SMR_DERIVATIVE_DEFINE(smr_fwidth_fine)
SMR_DERIVATIVE_DEFINE(smr_dpdx_coarse) SMR_DERIVATIVE_DEFINE(smr_dpdy_coarse) SMR_DERIVATIVE_DEFINE(smr_fwidth_coarse)
#undef SMR_DERIVATIVE_DEFINE

#ifdef SMR_HAS_VERTEX_CLIP
// ------------------------------------------------------------------------------------------------- the clip vertex stage and its rasteriser
// The reference's vertex stage runs once per vertex of the quad of wgpu/common_pipeline/plane.rs:6-28 (four vertices, triangles 0 1 2 and
// 2 3 0) and returns a vec4 clip position and the tex_coords varying.  Here it runs once per vertex per WORKGROUP: the 64 lanes of wave 0
// call it (lane l: vertex l & 3 of plane first + (l >> 2) — 16 planes x 4 vertices), one lane per triangle turns the results into a record of
// the table below, and after a barrier every lane reads the records (all lanes the same address: LDS broadcast reads).  Coverage is 2-D
// homogeneous rasterisation (edge functions of (X, Y, 1) from cross products of the (x, y, w) vertices): no clipping step, no division
// before coverage, a vertex behind the eye needs no special case.  include/smr.h states the contract and the order of the f32 operations.
#ifdef SMR_VARYINGS
// with varyings the stages carry them: the vertex stage returns N more floats, the fragment gets them interpolated (flat, linear or
// perspective by the two masks) and the whole @builtin(position) = (x + 0.5, y + 0.5, z / w, 1 / w)
__device__ smr_clip_vertex_v<SMR_VARYINGS> smr_vertex_clip(const smr_shader_in &in, int plane_id, int vertex_index, float3 position, float2 tex_coords);
__device__ float4 smr_fragment(const smr_shader_in &in, int plane_id, float2 uv, float4 position, const smr_varyings<SMR_VARYINGS> &v);
#else
__device__ smr_clip_vertex smr_vertex_clip(const smr_shader_in &in, int plane_id, int vertex_index, float3 position, float2 tex_coords);
#endif

// one triangle: 32 words, 16-byte aligned.  e[i] = (a, b, c) of the edge opposite vertex i; u, v, z, q = the planes (A, B, C) of
// sum E_i * {u_i, v_i, z_i, w_i - z_i}: all affine in (X, Y); box = clip-space bounds of the triangle widened by one pixel (the whole range
// when a vertex of the plane has w <= 0); flags bit i: edge i is inclusive, bit 3: drawn
#ifdef SMR_VARYINGS
// with N varyings the six pad words and what N needs beyond them: wn = the plane of Wn = sum E_i w_i (the divisor of linear varyings and of
// position.z, position.w), vary[k] = the plane (A, B, C) of varying k — of sum E_i t_i (perspective), of sum E_i (t_i w_i) (linear) — or, for
// a flat varying, the provoking vertex's word in vary[k][0].  29 + 3 N words, rounded up to 16 bytes: 32 words for N = 1, 56 for N = 8
struct alignas(16) smr_clip_tri {
    float e[3][3];
    float u[3], v[3], z[3], q[3];
    float box[4];  // x0, x1, y0, y1
    unsigned int flags;
    float wn[3];
    unsigned int vary[SMR_VARYINGS][3];  // (words: a flat varying is moved, never computed with)
};
static_assert(sizeof(smr_clip_tri) == (29 + 3 * SMR_VARYINGS + 3) / 4 * 16 && sizeof(smr_clip_tri) <= 256, "a triangle record is at most 64 words");
#else
struct alignas(16) smr_clip_tri {
    float e[3][3];
    float u[3], v[3], z[3], q[3];
    float box[4];  // x0, x1, y0, y1
    unsigned int flags;
    unsigned int pad[6];
};
static_assert(sizeof(smr_clip_tri) == 128, "a triangle record is 32 words");
#endif

extern "C" __global__ __launch_bounds__(256) void smr_user_shader_kernel(const UserShaderArgs a, const float *__restrict__ tables) {
#ifdef SMR_VARYINGS
    __shared__ float s_vert[64][6 + SMR_VARYINGS];  // x, y, z, w, u, v and the varyings of vertex (lane & 3) of plane slot (lane >> 2)
    __shared__ smr_clip_tri s_tri[32];               // triangle (i & 1) of plane slot (i >> 1).  Both: 5 888 B for N = 1, 10 752 B for N = 8
#else
    __shared__ float s_vert[64][6];      // x, y, z, w, u, v of vertex (lane & 3) of plane slot (lane >> 2): 1 536 B
    __shared__ smr_clip_tri s_tri[32];   // triangle (i & 1) of plane slot (i >> 1): 4 096 B
#endif
    const float *dec = tables, *thr = tables + 256;
    const int tid = (int)threadIdx.x;
#ifdef SMR_DERIVATIVES
    // quad mode: the lane-to-pixel map above.  The vertex stage and the table below do not depend on it
    const int x = blockIdx.x * 64 + 32 * ((tid >> 6) & 1) + 2 * ((tid & 63) >> 2) + (tid & 1), y = blockIdx.y * 4 + 2 * (tid >> 7) + ((tid >> 1) & 1);
#else
    const int x = blockIdx.x * 64 + (tid & 63), y = blockIdx.y * 4 + (tid >> 6);
#endif
    const smr_shader_in in(a, dec);
    const float W = (float)a.dst.w, H = (float)a.dst.h;
    const int first = a.n_src == 0 ? -1 : 0, last = a.n_src == 0 ? -1 : a.n_src - 1;
    // (no lane leaves before the second barrier: wave 0 of the last block column has lanes outside the target that own a vertex)
    if (tid < 64) {
        const int plane = first + (tid >> 2), k = tid & 3;
        if (plane <= last) {
            // plane.rs:11-28: (1, -1, 0) / (1, 1), (1, 1, 0) / (1, 0), (-1, 1, 0) / (0, 0), (-1, -1, 0) / (0, 1)
            const float px = k < 2 ? 1.0f : -1.0f, py = (k == 1 || k == 2) ? 1.0f : -1.0f;
#ifdef SMR_VARYINGS
            const smr_clip_vertex_v<SMR_VARYINGS> r = smr_vertex_clip(in, plane, k, make_float3(px, py, 0.0f), make_float2(k < 2 ? 1.0f : 0.0f, (k == 0 || k == 3) ? 1.0f : 0.0f));
#else
            const smr_clip_vertex r = smr_vertex_clip(in, plane, k, make_float3(px, py, 0.0f), make_float2(k < 2 ? 1.0f : 0.0f, (k == 0 || k == 3) ? 1.0f : 0.0f));
#endif
            float *o = s_vert[tid];
            o[0] = r.position.x; o[1] = r.position.y; o[2] = r.position.z; o[3] = r.position.w;
            o[4] = r.tex_coords.x; o[5] = r.tex_coords.y;
#ifdef SMR_VARYINGS
            for (int j = 0; j < SMR_VARYINGS; j++) o[6 + j] = r.varyings[j];  // (a copy: the word, whatever it holds)
#endif
        }
    }
    __syncthreads();
    if (tid < 32) {
        const int slot = tid >> 1, t = tid & 1;
        if (first + slot <= last) {
            // triangle t: vertices (0, 1, 2) or (2, 3, 0)
            const float *P[3] = {s_vert[slot * 4 + 2 * t], s_vert[slot * 4 + 2 * t + 1], s_vert[slot * 4 + ((2 * t + 2) & 3)]};
            smr_clip_tri T;
            for (int i = 0; i < 3; i++) {
                // (a, b, c)_i = p_j x p_k with p = (x, y, w).  The diagonal is p_2 x p_0 in triangle 0 and p_0 x p_2 in triangle 1: the same
                // products with the subtraction's operands exchanged — exact negations of each other
                const float *pj = P[(i + 1) % 3], *pk = P[(i + 2) % 3];
                T.e[i][0] = pj[1] * pk[3] - pj[3] * pk[1];
                T.e[i][1] = pj[3] * pk[0] - pj[0] * pk[3];
                T.e[i][2] = pj[0] * pk[1] - pj[1] * pk[0];
            }
            const float D = (P[0][0] * T.e[0][0] + P[0][1] * T.e[0][1]) + P[0][3] * T.e[0][2];
            for (int c = 0; c < 3; c++) {
                T.u[c] = (T.e[0][c] * P[0][4] + T.e[1][c] * P[1][4]) + T.e[2][c] * P[2][4];
                T.v[c] = (T.e[0][c] * P[0][5] + T.e[1][c] * P[1][5]) + T.e[2][c] * P[2][5];
                T.z[c] = (T.e[0][c] * P[0][2] + T.e[1][c] * P[1][2]) + T.e[2][c] * P[2][2];
                T.q[c] = (T.e[0][c] * (P[0][3] - P[0][2]) + T.e[1][c] * (P[1][3] - P[1][2])) + T.e[2][c] * (P[2][3] - P[2][2]);
            }
            // drawn: D > 0 and finite (front_face Ccw, cull_mode Back: wgpu/common_pipeline.rs:104-107; D <= 0 is a back face, an edge-on
            // or degenerate plane, NaN a NaN in x, y or w) and every coefficient finite (an infinity or NaN in z, u, v; products that
            // overflowed): such a triangle covers nothing
            bool drawn = D > 0.0f && D <= 3.40282347e+38f;
            for (int i = 0; i < 3; i++)
                for (int c = 0; c < 3; c++) drawn = drawn && __builtin_fabsf(T.e[i][c]) <= 3.40282347e+38f;
            for (int c = 0; c < 3; c++)
                drawn = drawn && __builtin_fabsf(T.u[c]) <= 3.40282347e+38f && __builtin_fabsf(T.v[c]) <= 3.40282347e+38f &&
                        __builtin_fabsf(T.z[c]) <= 3.40282347e+38f && __builtin_fabsf(T.q[c]) <= 3.40282347e+38f;
#ifdef SMR_VARYINGS
            // Wn's plane is not part of `drawn`, and neither is a flat varying: a NaN there is data.  A perspective or linear varying's
            // plane must be finite as u's and v's must.
            for (int c = 0; c < 3; c++) T.wn[c] = (T.e[0][c] * P[0][3] + T.e[1][c] * P[1][3]) + T.e[2][c] * P[2][3];
            for (int j = 0; j < SMR_VARYINGS; j++) {
                if (((SMR_VARYINGS_FLAT) >> j) & 1) {
                    // the provoking vertex is the triangle's first: vertex 0 of (0, 1, 2), vertex 2 of (2, 3, 0)
                    T.vary[j][0] = (unsigned int)__float_as_int(P[0][6 + j]);
                    T.vary[j][1] = T.vary[j][2] = 0u;
                    continue;
                }
                const bool linear = ((SMR_VARYINGS_LINEAR) >> j) & 1;
                const float t0 = linear ? P[0][6 + j] * P[0][3] : P[0][6 + j], t1 = linear ? P[1][6 + j] * P[1][3] : P[1][6 + j],
                            t2 = linear ? P[2][6 + j] * P[2][3] : P[2][6 + j];
                for (int c = 0; c < 3; c++) {
                    const float coef = (T.e[0][c] * t0 + T.e[1][c] * t1) + T.e[2][c] * t2;
                    drawn = drawn && __builtin_fabsf(coef) <= 3.40282347e+38f;
                    T.vary[j][c] = (unsigned int)__float_as_int(coef);
                }
            }
#endif
            unsigned int flags = drawn ? 8u : 0u;
            // top-left rule with clip-space Y pointing up: an edge owns the centres on it if a > 0, or a == 0 and b < 0
            for (int i = 0; i < 3; i++)
                if (T.e[i][0] > 0.0f || (T.e[i][0] == 0.0f && T.e[i][1] < 0.0f)) flags |= 1u << i;
            T.flags = flags;
            // With the plane's four w > 0 the triangle lies within the box of its vertices' x / w, y / w; widened by one pixel, which is far
            // more than the divisions' rounding.  A NaN or infinite bound compares false below: no early-out on that side.
            T.box[0] = T.box[2] = -3.40282347e+38f;
            T.box[1] = T.box[3] = 3.40282347e+38f;
            if (s_vert[slot * 4][3] > 0.0f && s_vert[slot * 4 + 1][3] > 0.0f && s_vert[slot * 4 + 2][3] > 0.0f && s_vert[slot * 4 + 3][3] > 0.0f) {
                const float x0 = P[0][0] / P[0][3], x1 = P[1][0] / P[1][3], x2 = P[2][0] / P[2][3];
                const float y0 = P[0][1] / P[0][3], y1 = P[1][1] / P[1][3], y2 = P[2][1] / P[2][3];
                T.box[0] = fminf(fminf(x0, x1), x2) - 2.0f / W;
                T.box[1] = fmaxf(fmaxf(x0, x1), x2) + 2.0f / W;
                T.box[2] = fminf(fminf(y0, y1), y2) - 2.0f / H;
                T.box[3] = fmaxf(fmaxf(y0, y1), y2) + 2.0f / H;
            }
#ifndef SMR_VARYINGS
            for (int i = 0; i < 6; i++) T.pad[i] = 0u;
#endif
            s_tri[tid] = T;
        }
    }
    __syncthreads();
#ifdef SMR_DERIVATIVES
    const bool in_target = x < a.dst.w && y < a.dst.h;  // (a lane outside an odd target lives on as a helper: it never touches the target)
#else
    if (x >= a.dst.w || y >= a.dst.h) return;
#endif
    const float fx = (float)x + 0.5f, fy = (float)y + 0.5f;          // @builtin(position).xy
    const float X = fx / W * 2.0f - 1.0f, Y = 1.0f - fy / H * 2.0f;  // the pixel centre in clip space
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);                     // LoadOp::Clear(TRANSPARENT)
#ifdef SMR_DERIVATIVES
    // the wave's 32 x 2 pixel block in clip space, from wave-uniform values: its two end columns' X, its two rows' Y (wY0 the upper, > wY1)
    const int wv = (int)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wx = blockIdx.x * 64 + 32 * (wv & 1), wy = blockIdx.y * 4 + 2 * (wv >> 1);
    const float wX0 = ((float)wx + 0.5f) / W * 2.0f - 1.0f, wX1 = ((float)(wx + 31) + 0.5f) / W * 2.0f - 1.0f;  // X is monotone in x
    const float wY0 = 1.0f - ((float)wy + 0.5f) / H * 2.0f, wY1 = 1.0f - ((float)(wy + 1) + 0.5f) / H * 2.0f;    // Y is monotone in y
#else
    // the wave's 64 x 1 pixel span in clip space, from wave-uniform values (as in the affine stage's early-out below)
    const int wx = blockIdx.x * 64, wy = blockIdx.y * 4 + (int)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const float wX0 = ((float)wx + 0.5f) / W * 2.0f - 1.0f, wX1 = ((float)(wx + 63) + 0.5f) / W * 2.0f - 1.0f;  // X is monotone in x
    const float wY = 1.0f - ((float)wy + 0.5f) / H * 2.0f;                                                       // == Y of every lane
#endif
    const int n_tri = min(2 * (last - first + 1), 2 * SMR_USER_SHADER_SOURCES);  // (the table's 32 records: smr_user_shader admits no more sources)
    for (int i = 0; i < n_tri; i++) {  // plane first + (i >> 1), triangle i & 1: index order
        const smr_clip_tri &T = s_tri[i];
        // wave-uniform (every lane read the same words): scalar branches.  A wave none of whose pixels can be covered evaluates no edge
        // function and no fragment code for this triangle.
        const unsigned int flags = (unsigned int)__builtin_amdgcn_readfirstlane((int)T.flags);
        if (!(flags & 8u)) continue;
        const float bx0 = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(T.box[0])));
        const float bx1 = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(T.box[1])));
        const float by0 = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(T.box[2])));
        const float by1 = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(T.box[3])));
#ifdef SMR_DERIVATIVES
        if (wX1 < bx0 || wX0 > bx1 || wY0 < by0 || wY1 > by1) continue;  // (the box is a pixel wider than the triangle: a quad that straddles it keeps its helpers)
#else
        if (wX1 < bx0 || wX0 > bx1 || wY < by0 || wY > by1) continue;
#endif
        const float E0 = (T.e[0][0] * X + T.e[0][1] * Y) + T.e[0][2];
        const float E1 = (T.e[1][0] * X + T.e[1][1] * Y) + T.e[1][2];
        const float E2 = (T.e[2][0] * X + T.e[2][1] * Y) + T.e[2][2];
#ifdef SMR_DERIVATIVES
        // the same three rules, as a value: every lane of the wave is still here, the quad's four answers are combined, and a quad with a
        // covered pixel goes on whole — its other pixels as helpers, with this triangle's planes extrapolated to their centres
        const float Zn = (T.z[0] * X + T.z[1] * Y) + T.z[2], Qn = (T.q[0] * X + T.q[1] * Y) + T.q[2];
        const float S = (E0 + E1) + E2;
        const bool covered = in_target && (E0 > 0.0f || (E0 == 0.0f && (flags & 1u))) && (E1 > 0.0f || (E1 == 0.0f && (flags & 2u))) &&
                             (E2 > 0.0f || (E2 == 0.0f && (flags & 4u))) && Zn >= 0.0f && Qn >= 0.0f && S > 0.0f;
        if (!smr_quad_any(covered)) continue;
#else
        // covered: every E_i > 0, or == 0 on an inclusive edge (a NaN compares false)
        if (!((E0 > 0.0f || (E0 == 0.0f && (flags & 1u))) && (E1 > 0.0f || (E1 == 0.0f && (flags & 2u))) && (E2 > 0.0f || (E2 == 0.0f && (flags & 4u)))))
            continue;
        // depth clip 0 <= z <= w, multiplied through by sum E > 0
        const float Zn = (T.z[0] * X + T.z[1] * Y) + T.z[2], Qn = (T.q[0] * X + T.q[1] * Y) + T.q[2];
        if (!(Zn >= 0.0f) || !(Qn >= 0.0f)) continue;
        const float S = (E0 + E1) + E2;
        if (!(S > 0.0f)) continue;  // (three concurrent edges through this centre: a triangle of no area that rounding let through)
#endif
        const float u = ((T.u[0] * X + T.u[1] * Y) + T.u[2]) / S, v = ((T.v[0] * X + T.v[1] * Y) + T.v[2]) / S;
#ifdef SMR_VARYINGS
        // Wn = sum E_i w_i: lambda_i = E_i w_i / Wn are the barycentrics in screen space.  No pixel is dropped on its account: where it is 0
        // the quotients below are what IEEE division gives
        const float Wn = (T.wn[0] * X + T.wn[1] * Y) + T.wn[2];
        smr_varyings<SMR_VARYINGS> vy;
#pragma unroll
        for (int j = 0; j < SMR_VARYINGS; j++) {
            if (((SMR_VARYINGS_FLAT) >> j) & 1) {
                vy.v[j] = __int_as_float((int)T.vary[j][0]);
            } else {
                const float n = (__int_as_float((int)T.vary[j][0]) * X + __int_as_float((int)T.vary[j][1]) * Y) + __int_as_float((int)T.vary[j][2]);
                vy.v[j] = n / ((((SMR_VARYINGS_LINEAR) >> j) & 1) ? Wn : S);
            }
        }
        const float4 f = smr_fragment(in, first + (i >> 1), make_float2(u, v), make_float4(fx, fy, Zn / Wn, S / Wn), vy);
#else
        const float4 f = smr_fragment(in, first + (i >> 1), make_float2(u, v), make_float2(fx, fy));
#endif
#ifdef SMR_DERIVATIVES
        if (!covered) continue;  // a helper's result is dropped
#endif
        const float k = 1.0f - f.w;  // PREMULTIPLIED_ALPHA_BLENDING (common_pipeline.rs:125)
        float4 o = make_float4(f.x + acc.x * k, f.y + acc.y * k, f.z + acc.z * k, f.w + acc.w * k);
        // render-target store, then what the next triangle's blend reads back
        store_texel(a.dst, a.pxi, x, y, o, thr);
        acc = load_texel(a.dst, a.pxi, x, y, dec);
    }
#ifdef SMR_DERIVATIVES
    if (!in_target) return;
#endif
    if (acc.x == 0.f && acc.y == 0.f && acc.z == 0.f && acc.w == 0.f) *(u32 *)(a.dst.ptr + (size_t)y * a.dst.pitch + (size_t)x * 4) = 0u;
}
#else
extern "C" __global__ __launch_bounds__(256) void smr_user_shader_kernel(const UserShaderArgs a, const float *__restrict__ tables) {
    const float *dec = tables, *thr = tables + 256;
#ifdef SMR_DERIVATIVES
    // quad mode (above): wave w covers the 32 x 2 block at (32 (w & 1), 2 (w >> 1)), four consecutive lanes a 2 x 2 quad; no lane leaves
    const int tid = (int)threadIdx.x;
    const int x = blockIdx.x * 64 + 32 * ((tid >> 6) & 1) + 2 * ((tid & 63) >> 2) + (tid & 1), y = blockIdx.y * 4 + 2 * (tid >> 7) + ((tid >> 1) & 1);
    const bool in_target = x < a.dst.w && y < a.dst.h;  // (a lane outside an odd target lives on as a helper: it never touches the target)
#else
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= a.dst.w || y >= a.dst.h) return;
#endif
    const smr_shader_in in(a, dec);
    const float W = (float)a.dst.w, H = (float)a.dst.h;
    const float fx = (float)x + 0.5f, fy = (float)y + 0.5f;          // @builtin(position).xy
    const float X = fx / W * 2.0f - 1.0f, Y = 1.0f - fy / H * 2.0f;  // the pixel centre in clip space
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);                     // LoadOp::Clear(TRANSPARENT)
    const int first = a.n_src == 0 ? -1 : 0, last = a.n_src == 0 ? -1 : a.n_src - 1;
#if defined(SMR_HAS_VERTEX_AFFINE) && defined(SMR_DERIVATIVES)
    // the wave's 32 x 2 pixel block in clip space, from wave-uniform values only: its two end columns' X, its two rows' Y (wY0 the upper, > wY1)
    const int wv = (int)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wx = blockIdx.x * 64 + 32 * (wv & 1), wy = blockIdx.y * 4 + 2 * (wv >> 1);
    const float wX0 = ((float)wx + 0.5f) / W * 2.0f - 1.0f, wX1 = ((float)(wx + 31) + 0.5f) / W * 2.0f - 1.0f;  // X is monotone in x
    const float wY0 = 1.0f - ((float)wy + 0.5f) / H * 2.0f, wY1 = 1.0f - ((float)(wy + 1) + 0.5f) / H * 2.0f;    // Y is monotone in y
    const float px_w = 2.0f / W, px_h = 2.0f / H;  // one pixel in clip space
#elif defined(SMR_HAS_VERTEX_AFFINE)
    // The wave's 64 x 1 pixel span in clip space, from wave-uniform values only (the row of a wave is threadIdx.x >> 6 of any of its
    // lanes): with smr_vertex_affine's result — a function of the kernel arguments and the plane — the early-out below is a scalar branch.
    const int wx = blockIdx.x * 64, wy = blockIdx.y * 4 + (int)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const float wX0 = ((float)wx + 0.5f) / W * 2.0f - 1.0f, wX1 = ((float)(wx + 63) + 0.5f) / W * 2.0f - 1.0f;  // X is monotone in x
    const float wY = 1.0f - ((float)wy + 0.5f) / H * 2.0f;                                                       // == Y of every lane
    const float px_w = 2.0f / W, px_h = 2.0f / H;  // one pixel in clip space
#endif
    for (int plane = first; plane <= last; plane++) {
#ifdef SMR_HAS_VERTEX_AFFINE
        const smr_affine m = smr_vertex_affine(in, plane);
        float qx, qy;  // position within the unit quad [-1, 1]^2
        if (m.xy == 0.0f && m.yx == 0.0f) {
            // axis-aligned: the smr_plane path below with sx = xx, sy = yy, operation for operation — the same bytes
            if (!(m.xx > 0.0f) || !(m.yy > 0.0f)) continue;
            qx = (X - m.cx) / m.xx;
            qy = (Y - m.cy) / m.yy;
        } else {
            // The reference draws the quad with front_face Ccw and cull_mode Some(Back) (wgpu/common_pipeline.rs:104-107,
            // create_render_pipeline, which transformations/shader/pipeline.rs:63 calls): a mirrored plane (det < 0) winds clockwise and
            // is culled.  det zero, NaN or infinite: nothing to invert, nothing covered.
            const float det = m.xx * m.yy - m.xy * m.yx;
            if (!(det > 0.0f) || !(det <= 3.40282347e+38f)) continue;
            // wave early-out: the plane lies within cx +- (|xx| + |xy|), cy +- (|yx| + |yy|).  The span's dx are bracketed by its two
            // ends' (the same subtraction the lanes do, monotone), its dy is the lanes' own; the box is widened by one pixel.  The
            // rounding of qx, qy below moves an edge by about 2^-23 * (|xx * yy| + |xy * yx|) / det of the plane's extent in clip space:
            // far less than a pixel for any plane wider than one, so there the early-out skips only what the exact test rejects.  For
            // a near-singular sliver (entries near 1 with det near 1e-4: about a tenth of a pixel wide at 1920, edges uncertain by
            // about one) the two tests may disagree on the sliver's few pixels.  A NaN compares false: no early-out, the exact test decides.
            const float ex = __builtin_fabsf(m.xx) + __builtin_fabsf(m.xy) + px_w, ey = __builtin_fabsf(m.yx) + __builtin_fabsf(m.yy) + px_h;
#ifdef SMR_DERIVATIVES
            // (the block's dy lie between its two rows'; the box is a pixel wider than the plane: a quad that straddles it keeps its helpers)
            if (wX1 - m.cx < -ex || wX0 - m.cx > ex || wY0 - m.cy < -ey || wY1 - m.cy > ey) continue;
#else
            const float wdy = wY - m.cy;
            if (wX1 - m.cx < -ex || wX0 - m.cx > ex || wdy < -ey || wdy > ey) continue;
#endif
            const float dx = X - m.cx, dy = Y - m.cy;
            qx = (dx * m.yy - dy * m.xy) / det;
            qy = (dy * m.xx - dx * m.yx) / det;
        }
#else
        float sx = 1.0f, sy = 1.0f, cx = 0.0f, cy = 0.0f;
#ifdef SMR_HAS_VERTEX
        const smr_plane p = smr_vertex(in, plane);
        sx = p.sx; sy = p.sy; cx = p.cx; cy = p.cy;
#endif
        if (!(sx > 0.0f) || !(sy > 0.0f)) continue;  // a degenerate plane covers no pixel centre
        const float qx = (X - cx) / sx, qy = (Y - cy) / sy;  // position within the unit quad [-1, 1]^2
#endif
        // coverage: pixel centre inside the quad; a centre exactly on an edge belongs to the quad whose left / top edge it is
#ifdef SMR_DERIVATIVES
        // the same rule, as a value: every lane of the wave is still here (the `continue`s above are the plane's, the same for all of them),
        // and a quad with a covered pixel goes on whole — its other pixels as helpers, uv from the same formulas at their own centres
        const bool covered = in_target && qx >= -1.0f && qx < 1.0f && qy > -1.0f && qy <= 1.0f;
        if (!smr_quad_any(covered)) continue;
#else
        if (!(qx >= -1.0f && qx < 1.0f && qy > -1.0f && qy <= 1.0f)) continue;
#endif
        const float u = (qx + 1.0f) * 0.5f, v = (1.0f - qy) * 0.5f;  // plane.rs:11-28: (1, -1) <-> tex (1, 1)
        const float4 f = smr_fragment(in, plane, make_float2(u, v), make_float2(fx, fy));
#ifdef SMR_DERIVATIVES
        if (!covered) continue;  // a helper's result is dropped
#endif
        const float k = 1.0f - f.w;  // PREMULTIPLIED_ALPHA_BLENDING (common_pipeline.rs:125)
        float4 o = make_float4(f.x + acc.x * k, f.y + acc.y * k, f.z + acc.z * k, f.w + acc.w * k);
        // render-target store, then what the next plane's blend reads back
        store_texel(a.dst, a.pxi, x, y, o, thr);
        acc = load_texel(a.dst, a.pxi, x, y, dec);
    }
#ifdef SMR_DERIVATIVES
    if (!in_target) return;
#endif
    if (acc.x == 0.f && acc.y == 0.f && acc.z == 0.f && acc.w == 0.f) *(u32 *)(a.dst.ptr + (size_t)y * a.dst.pitch + (size_t)x * 4) = 0u;
}
#endif  // SMR_HAS_VERTEX_CLIP

#endif  // SMR_USER_SHADER_KERNEL
