"""The node texture of a 10-bit 4:2:0 frame (test infrastructure): the witness of smelter_amd/csrc/smr_convert_hi.h.

The reference has no 10-bit path, so the value rule of include/smr.h is the specification: a 10-bit code c is the 8-bit code c / 4 with two
more fractional bits — its unorm value is (f32(c) * 0.25f) / 255.0f — and from there on the conversion is planar_yuv_to_rgba.wgsl /
nv12_to_rgba.wgsl as oracle/smr_oracle.c restates them, operation for operation, limited range.  This module restates the oracle's sequence
in numpy float32 (every product, sum and quotient individually rounded, as the oracle's C is compiled):

    subtexel                 floor(f * 256 + 0.5) / 256
    sample_plane_bilinear    clamp-to-edge fetch of four texels, a * (1 - fx) + b * fx per row, top * (1 - fy) + bot * fy
    yuv_to_rgb_store         clamp((x - 16/255) / k), the BT.709 matrix, floor(clamp(x) * 255 + 0.5)

On codes 4 b it is the oracle bit for bit (tests/test_emu_convert_hi.py holds it to orc.planar_yuv_to_rgba there); on true 10-bit codes it
is what the kernels are held to."""
import numpy as np

f32 = np.float32


def codes_of_words(words, p010: bool):
    """The 10-bit codes of 16-bit words: P010 keeps the high ten bits, planar the low ten."""
    words = np.asarray(words, np.uint16)
    return (words >> 6) if p010 else (words & 0x3FF)


def unorm_of_code(c):
    return (np.asarray(c).astype(f32) * f32(0.25)) / f32(255.0)


def _subtexel(f):
    return np.floor(f * f32(256.0) + f32(0.5)) / f32(256.0)


def _clamp01(x):
    # WGSL clamp = min(max(x, 0), 1) (the oracle's clampf; no NaN occurs here)
    return np.minimum(np.maximum(x, f32(0.0)), f32(1.0))


def _sample_plane_bilinear(plane, w, h):
    """plane: (ph, pw) codes -> (h, w) f32: the plane sampled at the centres of a w x h grid (oracle sample_plane_bilinear)."""
    ph, pw = plane.shape
    t = unorm_of_code(plane)
    tu = (np.arange(w, dtype=f32) + f32(0.5)) / f32(w)
    tv = (np.arange(h, dtype=f32) + f32(0.5)) / f32(h)
    sx = tu * f32(pw) - f32(0.5)
    sy = tv * f32(ph) - f32(0.5)
    fx0, fy0 = np.floor(sx), np.floor(sy)
    fx, fy = _subtexel(sx - fx0), _subtexel(sy - fy0)
    x0, x1 = np.clip(fx0.astype(np.int64), 0, pw - 1), np.clip(fx0.astype(np.int64) + 1, 0, pw - 1)
    y0, y1 = np.clip(fy0.astype(np.int64), 0, ph - 1), np.clip(fy0.astype(np.int64) + 1, 0, ph - 1)
    fx, fy = fx[None, :], fy[:, None]
    a, b = t[y0][:, x0], t[y0][:, x1]
    c, d = t[y1][:, x0], t[y1][:, x1]
    one = f32(1.0)
    top = a * (one - fx) + b * fx
    bot = c * (one - fx) + d * fx
    return top * (one - fy) + bot * fy


def _unorm8(x):
    return (_clamp01(x) * f32(255.0) + f32(0.5)).astype(np.int32).astype(np.uint8)


def node_rgba(y, u, v):
    """(h, w, 4) u8: the RGBA8 node texture of 10-bit codes y (h, w), u, v (chroma planes as the frame holds them: (h/2, w/2), or 1 x 1
    placeholders where that is empty), limited range."""
    y, u, v = np.asarray(y), np.asarray(u), np.asarray(v)
    assert y.max(initial=0) < 1024 and u.max(initial=0) < 1024 and v.max(initial=0) < 1024
    h, w = y.shape
    yy = unorm_of_code(y)
    uu = _sample_plane_bilinear(u, w, h)
    vv = _sample_plane_bilinear(v, w, h)
    k16 = f32(16.0) / f32(255.0)
    yy = _clamp01((yy - k16) / f32(0.85882352941))
    uu = _clamp01((uu - k16) / f32(0.87843137254))
    vv = _clamp01((vv - k16) / f32(0.87843137254))
    half = f32(0.5)
    r = yy + f32(1.5748) * (vv - half)
    g = yy - f32(0.1873) * (uu - half) - f32(0.4681) * (vv - half)
    b = yy + f32(1.8556) * (uu - half)
    out = np.empty((h, w, 4), np.uint8)
    out[..., 0], out[..., 1], out[..., 2], out[..., 3] = _unorm8(r), _unorm8(g), _unorm8(b), 255
    return out


def node_rgba_p010(y_words, uv_words):
    """The same from P010 words: y (h, w), uv (h/2, w/2, 2)."""
    uv = codes_of_words(uv_words, True)
    return node_rgba(codes_of_words(y_words, True), uv[..., 0], uv[..., 1])


def node_rgba_planar(y_words, u_words, v_words):
    return node_rgba(codes_of_words(y_words, False), codes_of_words(u_words, False), codes_of_words(v_words, False))


def rgb12_rows_to_rgba(packed, w, h):
    """(h, 3 w) bytes of an RGB12 node (12-byte groups: R x 4, G x 4, B x 4) -> (h, w, 4) RGBA8 with alpha 255."""
    rgb = np.asarray(packed).reshape(h, w // 4, 3, 4).transpose(0, 1, 3, 2).reshape(h, w, 3)
    return np.concatenate([rgb, np.full((h, w, 1), 255, np.uint8)], -1)
