// smr_shader_dev.h — the texel helpers of the shader node, ONE text for two compilers: the library's own kernels include it through
// smr_internal.h (hipcc, when the library is built), and it is the first header of every user shader program (smr_user_shader_prelude.h,
// compiled by the ROCm runtime compiler when a shader is registered; smelter_amd/build.py embeds both files in the library).  So a fragment
// restated from a built-in samples, blends and quantises with the very instructions the built-in does.
// Self-contained on purpose: the runtime compiler has no include path — nothing here may need a header beyond what it provides itself.
#pragma once

typedef unsigned char u8;
typedef unsigned short u16;
typedef unsigned int u32;

// where the byte-wide sRGB estimate table sits behind the thresholds (the table block's layout: srgb_encode8 below, smr_internal.h)
#define SMR_ENC_OFFSET_FROM_THR 260

// Device-side view of a surface.
struct SurfView {
    u8 *ptr;
    u32 pitch;
    int w, h;
};

// Kernel arguments of a user shader (smr_user_shader.hip fills them, the prelude's kernel reads them): sources, target, time and the
// parameter bytes travel by value — no upload, no synchronisation, nothing on the host to keep alive.
#define SMR_USER_SHADER_SOURCES 16       // == SMR_SHADER_MAX_SOURCES
#define SMR_USER_SHADER_PARAM_BYTES 2048  // == SMR_SHADER_MAX_PARAM_BYTES
struct UserShaderArgs {
    SurfView dst;
    SurfView src[SMR_USER_SHADER_SOURCES];
    int n_src, pxi;
    float time;
    u32 param_size;
    u32 params[SMR_USER_SHADER_PARAM_BYTES / 4];  // the bytes of the @group(1) uniform, zero behind param_size
};

// ------------------------------------------------------------------ device helpers
#if defined(__HIPCC__) || defined(__HIPCC_RTC__)

// Pixel interpretation used by filter kernels (same numbering as the oracle).
enum { PXI_RGBA8_SRGB = 0, PXI_RGBA8_UNORM = 1, PXI_RGBA16F = 2 };

__device__ __forceinline__ float clampf(float x, float lo, float hi) {
    // WGSL clamp: min(max(x, lo), hi); NaN -> lo
    if (!(x > lo)) return lo;
    if (x > hi) return hi;
    return x;
}
__device__ __forceinline__ int clampi(int x, int lo, int hi) { return x < lo ? lo : (x > hi ? hi : x); }

__device__ __forceinline__ u32 unorm8(float x) {
    x = clampf(x, 0.0f, 1.0f);
    return (u32)(int)(x * 255.0f + 0.5f);
}

// sRGB encode as the monotone step function u8 = #{i : thr[i] <= x}.  Table block layout
// (SMR_TABLE_FLOATS floats, built in smr_ctx_create, copied to LDS by the hot kernels):
//   [0,256)    decode LUT            [256,513)  thr[0..256] (thr[0] = -inf, thr[256] = +inf)
//   [516,932)  enc: 1664 bytes, enc[((bits(x) - bits(2^-13)) >> 16)] = code of the bucket's lowest x
// A bucket (7 mantissa bits) straddles at most two thresholds (checked when the table is built),
// so the estimate needs at most two upward fix-up steps: exact, branch-free, no transcendental.
__device__ __forceinline__ u32 srgb_encode8(float x, const float *__restrict__ thr) {
    // branch-free (independent encodes overlap their table latencies): the estimate index is taken from x clamped
    // into [2^-13, 1); below 2^-13 (< thr[1]; also NaN, negatives) the bucket code is 0 and no threshold is reached,
    // at and above 1 the last bucket's code steps up to 255 through thr[255] (thr[256] = +inf ends the count).
    const u8 *enc = (const u8 *)(thr + SMR_ENC_OFFSET_FROM_THR);
    const float xc = fminf(fmaxf(x, 1.220703125e-4f), 0.99999994f);
    u32 c = enc[(__float_as_uint(xc) - 0x39000000u) >> 16];
    c += thr[c + 1] <= x ? 1u : 0u;
    return c;
}

__device__ __forceinline__ float subtexel(float f) { return floorf(f * 256.0f + 0.5f) / 256.0f; }

// The 8-bit halves of load_texel / store_texel: an RGBA8 word <-> its float4, per `pxi` (PXI_RGBA8_SRGB or PXI_RGBA8_UNORM), for kernels
// that hold the word in a register.
__device__ __forceinline__ float4 decode_rgba8(u32 raw, int pxi, const float *__restrict__ dec) {
    const u32 r = raw & 0xff, g = (raw >> 8) & 0xff, b = (raw >> 16) & 0xff, a = raw >> 24;
    float4 o;
    if (pxi == PXI_RGBA8_SRGB) {
        o.x = dec[r]; o.y = dec[g]; o.z = dec[b];
    } else {
        o.x = (float)r / 255.0f; o.y = (float)g / 255.0f; o.z = (float)b / 255.0f;
    }
    o.w = (float)a / 255.0f;
    return o;
}
__device__ __forceinline__ u32 encode_rgba8(int pxi, const float4 &v, const float *__restrict__ thr) {
    u32 r, g, b;
    if (pxi == PXI_RGBA8_SRGB) {
        r = srgb_encode8(v.x, thr); g = srgb_encode8(v.y, thr); b = srgb_encode8(v.z, thr);
    } else {
        r = unorm8(v.x); g = unorm8(v.y); b = unorm8(v.z);
    }
    u32 a = unorm8(v.w);
    return r | (g << 8) | (b << 16) | (a << 24);
}

__device__ __forceinline__ float4 load_texel(const SurfView &s, int pxi, int x, int y, const float *__restrict__ dec) {
    float4 o;
    if (pxi == PXI_RGBA16F) {
        const uint2 raw = *(const uint2 *)(s.ptr + (size_t)y * s.pitch + (size_t)x * 8);
        __half2 lo = *(const __half2 *)&raw.x, hi = *(const __half2 *)&raw.y;
        float2 a = __half22float2(lo), b = __half22float2(hi);
        o = make_float4(a.x, a.y, b.x, b.y);
    } else {
        return decode_rgba8(*(const u32 *)(s.ptr + (size_t)y * s.pitch + (size_t)x * 4), pxi, dec);
    }
    return o;
}

__device__ __forceinline__ void store_texel(const SurfView &s, int pxi, int x, int y, float4 v,
                                            const float *__restrict__ thr) {
    if (pxi == PXI_RGBA16F) {
        __half2 lo = __floats2half2_rn(v.x, v.y), hi = __floats2half2_rn(v.z, v.w);
        uint2 raw;
        raw.x = *(const u32 *)&lo;
        raw.y = *(const u32 *)&hi;
        *(uint2 *)(s.ptr + (size_t)y * s.pitch + (size_t)x * 8) = raw;
    } else {
        const u32 word = encode_rgba8(pxi, v, thr);
        *(u32 *)(s.ptr + (size_t)y * s.pitch + (size_t)x * 4) = word;
    }
}

// textureSample of an RGBA8 (or RGBA16F) surface, bilinear + clamp, texels decoded per `pxi`.
__device__ __forceinline__ float4 sample_rgba_bilinear(const SurfView &s, int pxi, float u, float v,
                                                       const float *__restrict__ dec) {
    float sx = u * (float)s.w - 0.5f, sy = v * (float)s.h - 0.5f;
    float fx0 = floorf(sx), fy0 = floorf(sy);
    float fx = subtexel(sx - fx0), fy = subtexel(sy - fy0);
    int x0 = clampi((int)fx0, 0, s.w - 1), x1 = clampi((int)fx0 + 1, 0, s.w - 1);
    int y0 = clampi((int)fy0, 0, s.h - 1), y1 = clampi((int)fy0 + 1, 0, s.h - 1);
    float4 a = load_texel(s, pxi, x0, y0, dec), b = load_texel(s, pxi, x1, y0, dec);
    float4 c = load_texel(s, pxi, x0, y1, dec), d = load_texel(s, pxi, x1, y1, dec);
    float4 o;
    float gx = 1.0f - fx, gy = 1.0f - fy;
    o.x = (a.x * gx + b.x * fx) * gy + (c.x * gx + d.x * fx) * fy;
    o.y = (a.y * gx + b.y * fx) * gy + (c.y * gx + d.y * fx) * fy;
    o.z = (a.z * gx + b.z * fx) * gy + (c.z * gx + d.z * fx) * fy;
    o.w = (a.w * gx + b.w * fx) * gy + (c.w * gx + d.w * fx) * fy;
    return o;
}

#endif  // __HIPCC__ || __HIPCC_RTC__
