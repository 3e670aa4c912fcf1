// smr_user_shader_prelude.h — what the library puts around a user shader (include/smr.h "user shaders").
// A program is compiled from
//     #include "smr_shader_dev.h"              the texel helpers of the built-in shaders, the same text
//     #include "smr_user_shader_prelude.h"     PART 1: smr_shader_in, smr_plane, smr_affine, the accessors
//     <the user's translation unit>            smr_fragment, optionally smr_vertex or smr_vertex_affine
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

// what the user's translation unit defines
__device__ float4 smr_fragment(const smr_shader_in &in, int plane_id, float2 uv, float2 position);

#else
// ---------------------------------------------------------------------------------------------------------------------- PART 2
#if defined(SMR_HAS_VERTEX) && defined(SMR_HAS_VERTEX_AFFINE)
#error "a shader defines SMR_HAS_VERTEX or SMR_HAS_VERTEX_AFFINE, not both: one vertex stage per shader"
#endif
#ifdef SMR_HAS_VERTEX
__device__ smr_plane smr_vertex(const smr_shader_in &in, int plane_id);
#endif
#ifdef SMR_HAS_VERTEX_AFFINE
__device__ smr_affine smr_vertex_affine(const smr_shader_in &in, int plane_id);
#endif

extern "C" __global__ __launch_bounds__(256) void smr_user_shader_kernel(const UserShaderArgs a, const float *__restrict__ tables) {
    const float *dec = tables, *thr = tables + 256;
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= a.dst.w || y >= a.dst.h) return;
    const smr_shader_in in(a, dec);
    const float W = (float)a.dst.w, H = (float)a.dst.h;
    const float fx = (float)x + 0.5f, fy = (float)y + 0.5f;          // @builtin(position).xy
    const float X = fx / W * 2.0f - 1.0f, Y = 1.0f - fy / H * 2.0f;  // the pixel centre in clip space
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);                     // LoadOp::Clear(TRANSPARENT)
    const int first = a.n_src == 0 ? -1 : 0, last = a.n_src == 0 ? -1 : a.n_src - 1;
#ifdef SMR_HAS_VERTEX_AFFINE
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
            const float wdy = wY - m.cy;
            if (wX1 - m.cx < -ex || wX0 - m.cx > ex || wdy < -ey || wdy > ey) continue;
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
        if (!(qx >= -1.0f && qx < 1.0f && qy > -1.0f && qy <= 1.0f)) continue;
        const float u = (qx + 1.0f) * 0.5f, v = (1.0f - qy) * 0.5f;  // plane.rs:11-28: (1, -1) <-> tex (1, 1)
        const float4 f = smr_fragment(in, plane, make_float2(u, v), make_float2(fx, fy));
        const float k = 1.0f - f.w;  // PREMULTIPLIED_ALPHA_BLENDING (common_pipeline.rs:125)
        float4 o = make_float4(f.x + acc.x * k, f.y + acc.y * k, f.z + acc.z * k, f.w + acc.w * k);
        // render-target store, then what the next plane's blend reads back
        store_texel(a.dst, a.pxi, x, y, o, thr);
        acc = load_texel(a.dst, a.pxi, x, y, dec);
    }
    if (acc.x == 0.f && acc.y == 0.f && acc.z == 0.f && acc.w == 0.f) *(u32 *)(a.dst.ptr + (size_t)y * a.dst.pitch + (size_t)x * 4) = 0u;
}

#endif  // SMR_USER_SHADER_KERNEL
