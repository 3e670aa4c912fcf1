"""The node texture of a Y'CbCr frame under each colour matrix (test infrastructure): the witness of the input converters for
SMR_MATRIX_BT601 and SMR_MATRIX_BT2020_NCL, where the reference has no path (its WGSL hard-codes BT.709).

include/smr.h's value rule is the specification: everything up to and including the range step is the format's own — texel fetch, the 8-bit
sub-texel bilinear chroma sample (the packed formats' snapped fetch), the 10-bit code rule (c * 0.25) / 255, the limited-range division and
clamp (none for YUVJ420) — and the last three statements of yuv_to_rgb_store take their four constants from the matrix:

    r = y + c_rv * (v - 0.5);  g = y - c_gu * (u - 0.5) - c_gv * (v - 0.5);  b = y + c_bu * (u - 0.5)

This module is the oracle's sequence (oracle/smr_oracle.c: sample_plane_bilinear, interleaved422's fetch, yuv_to_rgb_store) in numpy float32,
every operation individually rounded, built on tests/hi_depth_model.py and tests/hi422_model.py (an 8-bit byte b is the 10-bit code 4 b:
(4 b * 0.25) / 255 is b / 255 exactly).  tests/test_color_matrix_model.py holds it at BT.709 to the oracle byte for byte — which pins
everything the three matrices share — and anchors each matrix to the colour bars computed from (Kr, Kb) in float64."""
import numpy as np

from tests import hi422_model as h422
from tests import hi_depth_model as hdm

f32 = np.float32

BT709, BT601, BT2020_NCL = 0, 1, 2
# c_rv, c_gu, c_gv, c_bu: f32 literals at the reference's four decimals (smelter_amd/csrc/smr_frame_formats.h holds the library's copy)
COEF = {BT709: (1.5748, 0.1873, 0.4681, 1.8556), BT601: (1.4020, 0.3441, 0.7141, 1.7720), BT2020_NCL: (1.4746, 0.1646, 0.5714, 1.8814)}
KR_KB = {BT709: (0.2126, 0.0722), BT601: (0.299, 0.114), BT2020_NCL: (0.2627, 0.0593)}
NAMES = {BT709: "bt709", BT601: "bt601", BT2020_NCL: "bt2020"}

# base formats (include/smr.h)
(PLANAR_YUV420, PLANAR_YUV422, PLANAR_YUV444, PLANAR_YUVJ420, UYVY422, YUYV422, NV12, BGRA, ARGB, RGBA, P010, PLANAR_YUV420P10, PLANAR_YUV422P10, P210,
 V210) = range(15)
YCBCR_FORMATS = (PLANAR_YUV420, PLANAR_YUV422, PLANAR_YUV444, PLANAR_YUVJ420, UYVY422, YUYV422, NV12, P010, PLANAR_YUV420P10, PLANAR_YUV422P10, P210, V210)


def store(yy, uu, vv, matrix, full=False):
    """yuv_to_rgb_store on unorm values (h, w) f32 -> (h, w, 4) u8."""
    if not full:
        k16 = f32(16.0) / f32(255.0)
        yy = hdm._clamp01((yy - k16) / f32(0.85882352941))
        uu = hdm._clamp01((uu - k16) / f32(0.87843137254))
        vv = hdm._clamp01((vv - k16) / f32(0.87843137254))
    rv, gu, gv, bu = (f32(c) for c in COEF[matrix])
    half = f32(0.5)
    r = yy + rv * (vv - half)
    g = yy - gu * (uu - half) - gv * (vv - half)
    b = yy + bu * (uu - half)
    out = np.empty(yy.shape + (4,), np.uint8)
    out[..., 0], out[..., 1], out[..., 2], out[..., 3] = hdm._unorm8(r), hdm._unorm8(g), hdm._unorm8(b), 255
    return out


def node_planar_codes(y, u, v, matrix, full=False):
    """10-bit codes y (h, w), chroma planes of any subsampling (as the frame holds them; 1 x 1 placeholders where empty)."""
    y, u, v = np.asarray(y), np.asarray(u), np.asarray(v)
    h, w = y.shape
    return store(hdm.unorm_of_code(y), hdm._sample_plane_bilinear(u, w, h), hdm._sample_plane_bilinear(v, w, h), matrix, full)


def node_pairs_codes(y, cb, cr, matrix):
    """v210's rule: pixel x takes luma Y[x] and the chroma of pair x / 2 — codes y (h, w), cb, cr (h, ceil(w / 2)); limited range."""
    y, cb, cr = np.asarray(y), np.asarray(cb), np.asarray(cr)
    pair = np.arange(y.shape[1]) // 2
    return store(hdm.unorm_of_code(y), hdm.unorm_of_code(cb)[:, pair], hdm.unorm_of_code(cr)[:, pair], matrix)


def node_interleaved8(plane, w, order, matrix):
    """interleaved_{uyvy,yuyv}_to_rgba.wgsl:24-62 as the oracle restates it: plane (h, tw, 4) bytes, order 0 = U Y0 V Y1, 1 = Y0 U Y1 V."""
    plane = np.asarray(plane, np.uint8)
    h, tw = plane.shape[0], plane.shape[1]
    dimx = f32(tw)
    hpw = f32(0.5) / dimx
    tcx = (np.arange(w, dtype=f32) + f32(0.5)) / f32(w)
    xf = (tcx * dimx - hpw + f32(0.0001)) * f32(2.0)
    x_pos = xf.astype(np.int64)
    tx = np.clip(x_pos // 2, 0, tw - 1)
    odd = (x_pos % 2) != 0
    t = plane[:, tx, :].astype(f32) / f32(255.0)  # (h, w, 4)
    if order == 0:
        uu, vv, yy = t[..., 0], t[..., 2], np.where(odd[None, :], t[..., 3], t[..., 1])
    else:
        uu, vv, yy = t[..., 1], t[..., 3], np.where(odd[None, :], t[..., 2], t[..., 0])
    return store(yy, uu, vv, matrix)


def node_rgba(fmt, w, h, planes, matrix):
    """The RGBA8 node texture (h, w, 4) of a frame of base format `fmt` whose planes are the arrays smelter_amd.hip.DeviceFrame uploads
    (bytes, 16-bit words or v210 dwords)."""
    p = [np.asarray(a) for a in planes]
    c4 = lambda a: a.astype(np.uint16) * 4  # noqa: E731  (a byte as the 10-bit code with the same unorm value)
    if fmt in (PLANAR_YUV420, PLANAR_YUV422, PLANAR_YUV444, PLANAR_YUVJ420):
        return node_planar_codes(c4(p[0].reshape(h, w)), c4(p[1]), c4(p[2]), matrix, full=fmt == PLANAR_YUVJ420)
    if fmt == NV12:
        return node_planar_codes(c4(p[0].reshape(h, w)), c4(p[1][..., 0]), c4(p[1][..., 1]), matrix)
    if fmt in (UYVY422, YUYV422):
        return node_interleaved8(p[0], w, 0 if fmt == UYVY422 else 1, matrix)
    if fmt in (P010, P210):
        uv = hdm.codes_of_words(p[1], True)
        return node_planar_codes(hdm.codes_of_words(p[0], True), uv[..., 0], uv[..., 1], matrix)
    if fmt in (PLANAR_YUV420P10, PLANAR_YUV422P10):
        return node_planar_codes(*(hdm.codes_of_words(a, False) for a in p), matrix)
    if fmt == V210:
        return node_pairs_codes(*h422.v210_unpack(p[0], w), matrix)
    raise ValueError(f"no Y'CbCr format {fmt}")


def rgb12_rows(rgba):
    """(h, w, 4) RGBA8 -> the (h, 3 w) bytes of the RGB12 node: 12-byte groups of four pixels (R x 4, G x 4, B x 4); w a multiple of 4."""
    h, w = rgba.shape[:2]
    return np.ascontiguousarray(rgba[..., :3].reshape(h, w // 4, 4, 3).transpose(0, 1, 3, 2).reshape(h, 3 * w))


# ---- frames for the tests: planes of a format from 8-bit content (the 10-bit formats take codes 4 b + extra two bits where given)

def chroma_shape(fmt, w, h):
    if fmt in (PLANAR_YUV420, PLANAR_YUVJ420, NV12, P010, PLANAR_YUV420P10):
        return max(h // 2, 1), max(w // 2, 1)
    if fmt in (PLANAR_YUV422, PLANAR_YUV422P10, P210):
        return h, max(w // 2, 1)
    if fmt == PLANAR_YUV444:
        return h, w
    return h, (w + 1) // 2  # the packed formats: one chroma pair per two pixels


def planes_of(fmt, y, u, v):
    """Planes of a frame of `fmt` from codes y (h, w), u, v (chroma_shape): bytes for the 8-bit formats (codes 0 .. 255), 10-bit codes
    (0 .. 1023) for the others."""
    y, u, v = np.asarray(y), np.asarray(u), np.asarray(v)
    if fmt in (PLANAR_YUV420, PLANAR_YUV422, PLANAR_YUV444, PLANAR_YUVJ420):
        return [y.astype(np.uint8), u.astype(np.uint8), v.astype(np.uint8)]
    if fmt == NV12:
        return [y.astype(np.uint8), np.ascontiguousarray(np.stack([u, v], -1).astype(np.uint8))]
    if fmt == UYVY422:
        return [np.ascontiguousarray(np.stack([u, y[:, 0::2], v, y[:, 1::2]], -1).astype(np.uint8))]
    if fmt == YUYV422:
        return [np.ascontiguousarray(np.stack([y[:, 0::2], u, y[:, 1::2], v], -1).astype(np.uint8))]
    if fmt in (P010, P210):
        return [(y.astype(np.uint16) << 6), np.ascontiguousarray(np.stack([u, v], -1).astype(np.uint16) << 6)]
    if fmt in (PLANAR_YUV420P10, PLANAR_YUV422P10):
        return [y.astype(np.uint16), u.astype(np.uint16), v.astype(np.uint16)]
    if fmt == V210:
        return [h422.v210_pack(y, u, v)]
    raise ValueError(fmt)


def is_hi(fmt):
    return fmt in (P010, PLANAR_YUV420P10, PLANAR_YUV422P10, P210, V210)


def noise_planes(fmt, w, h, seed):
    """Uniform noise over the whole code range of the format."""
    rng = np.random.default_rng(seed)
    top = 1024 if is_hi(fmt) else 256
    ch = chroma_shape(fmt, w, h)
    return planes_of(fmt, rng.integers(0, top, (h, w)), rng.integers(0, top, ch), rng.integers(0, top, ch))


# ---- the anchor: the eight 100 % bars' limited-range codes from (Kr, Kb) in float64

BARS = [(1, 1, 1), (1, 1, 0), (0, 1, 1), (0, 1, 0), (1, 0, 1), (1, 0, 0), (0, 0, 1), (0, 0, 0)]


def bar_codes(matrix, rgb, bits):
    """(Y', Cb, Cr) integer codes of R'G'B' in {0, 1}^3 at `bits` bits, limited range, rounded to nearest."""
    kr, kb = KR_KB[matrix]
    r, g, b = (float(c) for c in rgb)
    yy = kr * r + (1.0 - kr - kb) * g + kb * b
    cb = (b - yy) / (2.0 * (1.0 - kb))
    cr = (r - yy) / (2.0 * (1.0 - kr))
    s = 1 << (bits - 8)
    return int(round((16.0 + 219.0 * yy) * s)), int(round((128.0 + 224.0 * cb) * s)), int(round((128.0 + 224.0 * cr) * s))
