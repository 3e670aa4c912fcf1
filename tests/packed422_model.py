"""Packed 4:2:2 output frames (SMR_FRAME_UYVY422 / SMR_FRAME_YUYV422 where a frame is an output, include/smr.h): the expected picture.

Nothing is defined numerically that the planar 4:2:2 output does not define: a packed frame is an interleave of its planes.  Texel j of row y
— one RGBA8 texel of the frame's single (w / 2) x h plane — holds U[y][j] Y[y][2j] V[y][j] Y[y][2j+1] (UYVY) or Y[y][2j] U[y][j] Y[y][2j+1]
V[y][j] (YUYV), so every test takes its expected bytes from `interleave` over the oracle's rgba_to_planar_yuv(px, YUV422) (or over the
library's own planar 4:2:2 output of the same call).  Even widths from 2, any height from 1."""
import functools

import numpy as np

UYVY, YUYV = 0, 1
ORDERS = (UYVY, YUYV)
NAMES = {UYVY: "uyvy", YUYV: "yuyv"}
BLACK = {UYVY: (0x80, 0x10, 0x80, 0x10), YUYV: (0x10, 0x80, 0x10, 0x80)}  # Y = 16, U = V = 128, in memory order


def frame_format(hip, order):
    return hip.FRAME_UYVY422 if order == UYVY else hip.FRAME_YUYV422


def interleave(y, u, v, order):
    """(h, w) luma and (h, w / 2) chroma planes -> the (h, w / 2, 4) texels of the packed frame."""
    y, u, v = (np.asarray(p, np.uint8) for p in (y, u, v))
    h, w = y.shape
    assert w % 2 == 0 and w >= 2 and u.shape == v.shape == (h, w // 2), (y.shape, u.shape, v.shape)
    out = np.empty((h, w // 2, 4), np.uint8)
    ya, yb = y[:, 0::2], y[:, 1::2]
    if order == UYVY:
        out[..., 0], out[..., 1], out[..., 2], out[..., 3] = u, ya, v, yb
    else:
        out[..., 0], out[..., 1], out[..., 2], out[..., 3] = ya, u, yb, v
    return out


def expected(orc, rgba, order):
    """The oracle's picture of an (h, w, 4) RGBA8 node texture as a packed frame."""
    rgba = np.ascontiguousarray(rgba, np.uint8)
    h, w = rgba.shape[:2]
    y, u, v = orc.rgba_to_planar_yuv(rgba, orc.YUV422)
    return interleave(np.asarray(y).reshape(h, w), np.asarray(u).reshape(h, w // 2), np.asarray(v).reshape(h, w // 2), order)


@functools.lru_cache(maxsize=None)
def near_boundary_pairs(per_plane=256):
    """An (n, 2, 3) uint8 array of pixel pairs (R, G, B each) whose pair chroma lies nearest a code boundary in real arithmetic, chosen in
    f64 as tests/test_yuv_fast.py::_near_boundary_triples chooses luma: the `per_plane` nearest for Cb, then the `per_plane` nearest for Cr,
    over all 511^3 channel sums.  The guard of smr_yuv_fast.h flags a value within 2^-13 code units of a boundary (about 2 in 10 000 of the
    sums): the nearest few hundred of 133 million all raise it, so a picture of these pairs runs the repair branch on every block."""
    f = lambda c: np.float64(np.float32(c))
    kc, c16 = f(0.87843137254), f(16.0 / 255.0)
    coef = {1: (f(-0.1146), f(-0.3854), f(0.5)), 2: (f(0.5), f(-0.4542), f(-0.0458))}
    s = np.arange(511, dtype=np.float64)
    out = []
    for plane in (1, 2):
        cr, cg, cb = coef[plane]
        best_d, best_i = np.empty(0), np.empty((0, 3), np.int64)
        rg = (s[:, None] * cr + s[None, :] * cg) / 510.0  # (sr, sg): the mean of the pair's byte / 255 values
        for sb in range(511):
            x = ((rg + sb * cb / 510.0 + 0.5) * kc + c16) * 255.0 + 0.5
            d = np.abs(x - np.round(x)).ravel()
            k = np.argpartition(d, per_plane)[:per_plane]
            best_d = np.concatenate([best_d, d[k]])
            best_i = np.concatenate([best_i, np.stack([k // 511, k % 511, np.full(per_plane, sb)], -1)])
            if best_d.size > 8 * per_plane:
                keep = np.argsort(best_d)[:per_plane]
                best_d, best_i = best_d[keep], best_i[keep]
        out.append(best_i[np.argsort(best_d)[:per_plane]])
    sums = np.concatenate(out)                       # (n, 3) channel sums
    lo = np.where(np.arange(len(sums))[:, None] % 2 == 0, sums // 2, np.maximum(sums - 255, 0))  # two ways to split a sum into two bytes
    return np.stack([lo, sums - lo], 1).astype(np.uint8)


def near_boundary_picture(w=512, h=2):
    """near_boundary_pairs as an opaque (h, w, 4) RGBA8 picture: pair j of row y at pixels 2j, 2j + 1."""
    pairs = near_boundary_pairs(w * h // 4)
    assert len(pairs) == w * h // 2
    px = np.full((h, w, 4), 255, np.uint8)
    px[..., :3] = pairs.reshape(h, w, 3)
    return px


def black(w, h, order):
    return np.broadcast_to(np.array(BLACK[order], np.uint8), (h, w // 2, 4)).copy()
