"""The v210 half of the 10-bit 4:2:2 witness (test infrastructure): smelter_amd/csrc/smr_convert_hi422.h is held to this.

Planar 10-bit 4:2:2 and P210 need nothing new: tests/hi_depth_model.py::node_rgba samples chroma planes of any shape, and with (h, w / 2)
planes it is planar_yuv_to_rgba.wgsl on a 4:2:2 frame.  v210 follows interleaved_uyvy_to_rgba.wgsl as include/smr.h defines it for every
width: pixel x takes luma Y[x] and the chroma of pair x / 2, no interpolation, then yuv_to_rgb_store (limited range) — the sequence below,
in numpy float32 with every operation individually rounded, built on hi_depth_model's functions.

The layout: a dword holds three 10-bit codes (lo: bits 0-9, mid: 10-19, hi: 20-29; bits 30-31 are ignored), six pixels are four dwords,

    d0 = Cb(0) Y0 Cr(0)    d1 = Y1 Cb(1) Y2    d2 = Cr(1) Y3 Cb(2)    d3 = Y4 Cr(2) Y5        (lo mid hi)

and a row is ceil(w / 6) such groups; components of pixels at or beyond w are ignored."""
import numpy as np

from tests import hi_depth_model as hdm

f32 = np.float32

# the group's twelve fields (lo mid hi of d0 .. d3), by what they hold: (component, index inside the group)
_FIELDS = [("cb", 0), ("y", 0), ("cr", 0), ("y", 1), ("cb", 1), ("y", 2), ("cr", 1), ("y", 3), ("cb", 2), ("y", 4), ("cr", 2), ("y", 5)]


def groups(w):
    return (w + 5) // 6


def v210_pack(y, cb, cr, junk=None, beyond=None):
    """Codes y (h, w), cb, cr (h, ceil(w / 2)) -> the (h, 4 ceil(w / 6)) uint32 plane.  junk: (h, 4 ceil(w / 6)) values for bits 30-31
    (zero by default); beyond: an (h, 6 ceil(w / 6)) array of codes for the components of pixels at or beyond w (luma at its pixel, both
    chroma codes of a pair beyond the last one from the pair's first pixel; zero by default)."""
    y, cb, cr = np.asarray(y, np.uint32), np.asarray(cb, np.uint32), np.asarray(cr, np.uint32)
    h, w = y.shape
    n = groups(w)
    assert cb.shape == cr.shape == (h, (w + 1) // 2) and max(y.max(initial=0), cb.max(initial=0), cr.max(initial=0)) < 1024
    fill = np.zeros((h, 6 * n), np.uint32) if beyond is None else np.asarray(beyond, np.uint32) & 0x3FF
    yy = fill.copy()
    yy[:, :w] = y
    cbb, crr = fill[:, 0::2].copy(), fill[:, 0::2].copy()
    cbb[:, :cb.shape[1]], crr[:, :cr.shape[1]] = cb, cr
    comp = {"y": yy.reshape(h, n, 6), "cb": cbb.reshape(h, n, 3), "cr": crr.reshape(h, n, 3)}
    out = np.zeros((h, n, 4), np.uint32)
    for k, (name, i) in enumerate(_FIELDS):
        out[:, :, k // 3] |= comp[name][:, :, i] << np.uint32(10 * (k % 3))
    out = out.reshape(h, 4 * n)
    if junk is not None:
        out |= (np.asarray(junk, np.uint32) & 3) << np.uint32(30)
    return np.ascontiguousarray(out)


def v210_unpack(plane, w):
    """The (h, 4 ceil(w / 6)) uint32 plane -> codes y (h, w), cb, cr (h, ceil(w / 2)), uint16."""
    plane = np.asarray(plane, np.uint32)
    h, n = plane.shape[0], groups(w)
    assert plane.shape == (h, 4 * n)
    d = plane.reshape(h, n, 4)
    comp = {"y": np.zeros((h, n, 6), np.uint16), "cb": np.zeros((h, n, 3), np.uint16), "cr": np.zeros((h, n, 3), np.uint16)}
    for k, (name, i) in enumerate(_FIELDS):
        comp[name][:, :, i] = (d[:, :, k // 3] >> np.uint32(10 * (k % 3))) & 0x3FF
    c = (w + 1) // 2
    return comp["y"].reshape(h, 6 * n)[:, :w].copy(), comp["cb"].reshape(h, 3 * n)[:, :c].copy(), comp["cr"].reshape(h, 3 * n)[:, :c].copy()


def node_rgba_v210(y, cb, cr):
    """(h, w, 4) u8: the RGBA8 node texture of v210 codes y (h, w), cb, cr (h, ceil(w / 2)): the pair's own chroma, limited range."""
    y, cb, cr = np.asarray(y), np.asarray(cb), np.asarray(cr)
    assert y.max(initial=0) < 1024 and cb.max(initial=0) < 1024 and cr.max(initial=0) < 1024
    h, w = y.shape
    pair = np.arange(w) // 2
    yy = hdm.unorm_of_code(y)
    uu = hdm.unorm_of_code(cb)[:, pair]
    vv = hdm.unorm_of_code(cr)[:, pair]
    k16 = f32(16.0) / f32(255.0)
    yy = hdm._clamp01((yy - k16) / f32(0.85882352941))
    uu = hdm._clamp01((uu - k16) / f32(0.87843137254))
    vv = hdm._clamp01((vv - k16) / f32(0.87843137254))
    half = f32(0.5)
    r = yy + f32(1.5748) * (vv - half)
    g = yy - f32(0.1873) * (uu - half) - f32(0.4681) * (vv - half)
    b = yy + f32(1.8556) * (uu - half)
    out = np.empty((h, w, 4), np.uint8)
    out[..., 0], out[..., 1], out[..., 2], out[..., 3] = hdm._unorm8(r), hdm._unorm8(g), hdm._unorm8(b), 255
    return out


def node_rgba_v210_plane(plane, w):
    return node_rgba_v210(*v210_unpack(plane, w))


def uyvy_of(y8, cb8, cr8):
    """Bytes y (h, w), cb, cr (h, w / 2) (w even) -> the (h, w / 2, 4) U Y0 V Y1 plane of the 8-bit frame."""
    return np.ascontiguousarray(np.stack([cb8, y8[:, 0::2], cr8, y8[:, 1::2]], -1).astype(np.uint8))
