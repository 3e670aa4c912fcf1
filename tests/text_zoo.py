"""The Text jobs k_text_nodes is held on, shared by tests/test_emu_text_nodes.py (the kernel's source on the CPU, against oracle.blit_glyphs)
and tests/test_gpu_text_nodes.py (the kernel on the device, against smr_blit_glyphs).  A job is (w, h, bg, glyphs, atlas): a w x h RGBA8
surface, the background as smr_blit_glyphs takes it, oracle.Glyph quads and their A8 coverage atlas.  Surfaces stay within 131 x 34: three
tiles across, three down — the smallest sizes at which the kernel's tiles, groups and bins branch.  Test infrastructure only."""
import ctypes as C

import numpy as np

from oracle.oracle import Glyph

WIDTHS = (1, 3, 4, 5, 63, 64, 65, 67)
HEIGHTS = (1, 15, 16, 17)
TILE_W, TILE_H = 64, 16


class CGlyph(C.Structure):  # field for field include/smr.h smr_glyph
    _fields_ = [("dst_x", C.c_int32), ("dst_y", C.c_int32), ("w", C.c_int32), ("h", C.c_int32),
                ("atlas_x", C.c_int32), ("atlas_y", C.c_int32), ("color", C.c_float * 4)]


def pack(glyphs):
    arr = (CGlyph * max(len(glyphs), 1))()
    for i, g in enumerate(glyphs):
        arr[i].dst_x, arr[i].dst_y, arr[i].w, arr[i].h, arr[i].atlas_x, arr[i].atlas_y = g.dst_x, g.dst_y, g.w, g.h, g.atlas_x, g.atlas_y
        arr[i].color[:] = list(g.color)
    return arr


def tiles(w, h):
    return ((w + TILE_W - 1) // TILE_W) * ((h + TILE_H - 1) // TILE_H) if w > 0 and h > 0 else 0


def atlas_of(rng, aw, ah):
    """Coverage noise with both ends of the range present."""
    a = rng.integers(0, 256, (ah, aw), dtype=np.uint8)
    a[rng.random((ah, aw)) < 0.15] = 255
    a[rng.random((ah, aw)) < 0.15] = 0
    return a


def colour(rng):
    c = rng.random(4)
    return (float(c[0]), float(c[1]), float(c[2]), float(0.3 + 0.7 * c[3]))


def random_job(rng, w, h, n_glyphs=6, aw=48, ah=24):
    """Quads of up to 24 x 12 scattered over (and a little beyond) the surface."""
    atlas = atlas_of(rng, aw, ah)
    glyphs = []
    for _ in range(n_glyphs):
        gw, gh = int(rng.integers(1, 25)), int(rng.integers(1, 13))
        glyphs.append(Glyph(int(rng.integers(-6, max(w, 1) + 3)), int(rng.integers(-4, max(h, 1) + 2)), gw, gh,
                            int(rng.integers(0, aw - gw + 1)), int(rng.integers(0, ah - gh + 1)), colour(rng)))
    bg = tuple(float(x) for x in rng.random(4))
    return (w, h, bg, glyphs, atlas)


def sizes():
    """Every width x height at which a row's last group or a surface's last tile row is partial, whole or one over."""
    rng = np.random.default_rng(4242)
    return [random_job(rng, w, h) for w in WIDTHS for h in HEIGHTS]


def painter(order):
    """Two overlapping glyphs of different colours at alpha 0.7, in either order."""
    rng = np.random.default_rng(77)
    atlas = np.maximum(atlas_of(rng, 32, 16), 64).astype(np.uint8)  # (coverage everywhere: the order shows on every shared texel)
    a = Glyph(60, 10, 12, 10, 0, 0, (1.0, 0.2, 0.1, 0.7))
    b = Glyph(66, 14, 12, 10, 16, 0, (0.1, 0.9, 0.3, 0.7))
    return (80, 30, (0.1, 0.2, 0.4, 0.8), [a, b] if order == 0 else [b, a], atlas)


def edge_cases():
    """name -> job"""
    rng = np.random.default_rng(99)
    atlas = atlas_of(rng, 40, 20)
    wide_atlas = atlas_of(rng, 257, 9)
    col = [colour(rng) for _ in range(8)]
    bg = (0.2, 0.5, 0.1, 0.6)
    out = {}
    out["no glyphs"] = (65, 17, bg, [], atlas)
    out["no glyphs, opaque black"] = (131, 34, (0.0, 0.0, 0.0, 1.0), [], atlas)
    # x = 62 .. 66, y = 14 .. 18: four bins
    out["straddles four tiles"] = (131, 34, bg, [Glyph(62, 14, 5, 5, 3, 2, col[0])], atlas)
    out["starts at x mod 4 = 1, 2, 3"] = (67, 17, bg, [Glyph(1, 0, 9, 6, 0, 0, col[0]), Glyph(14, 3, 9, 6, 5, 1, col[1]), Glyph(27, 9, 9, 6, 9, 3, col[2]),
                                                     Glyph(61, 2, 6, 13, 20, 5, col[3])], atlas)
    out["ends on the last texel"] = (67, 17, bg, [Glyph(60, 12, 7, 5, 11, 7, col[4])], atlas)
    out["ends on the last texel of a whole tile"] = (128, 32, bg, [Glyph(117, 21, 11, 11, 11, 7, col[4])], atlas)
    # the atlas is 257 wide and the glyph's last row ends on its last byte
    out["coverage ends on the atlas' last byte"] = (70, 18, bg, [Glyph(3, 2, 21, 9, 257 - 21, 0, col[5]), Glyph(40, 9, 1, 1, 256, 8, col[6])], wide_atlas)
    out["glyphs without an area"] = (65, 17, bg, [Glyph(2, 2, 0, 7, 0, 0, col[0]), Glyph(5, 3, 10, 8, 4, 4, col[1]), Glyph(9, 4, 7, 0, 33, 20, col[2]),
                                                Glyph(0, 0, 0, 0, 0, 0, col[3])], atlas)
    out["partly and wholly outside"] = (70, 20, bg, [Glyph(-3, -2, 10, 8, 0, 0, col[0]), Glyph(64, 15, 12, 5, 6, 6, col[1]), Glyph(-100, 5, 30, 10, 1, 1, col[2]),
                                                   Glyph(75, 0, 20, 10, 2, 2, col[3]), Glyph(10, -40, 20, 15, 3, 3, col[4]), Glyph(10, 20, 20, 15, 4, 4, col[5]),
                                                   Glyph(-39, 4, 40, 6, 0, 7, col[6]), Glyph(-100000, -100000, 40, 20, 0, 0, col[7])], atlas)
    # 131 x 16 has three tiles: the middle one gets nothing
    out["an empty bin between full ones"] = (131, 16, bg, [Glyph(2, 1, 30, 12, 0, 0, col[0]), Glyph(20, 5, 30, 10, 4, 3, col[1]), Glyph(129, 0, 2, 16, 7, 1, col[2]),
                                                        Glyph(130, 3, 8, 8, 9, 9, col[3])], atlas)
    out["many glyphs on one texel"] = (9, 3, bg, [Glyph(4, 1, 1 + k % 3, 1 + k % 2, k % 30, k % 15, col[k % 8]) for k in range(40)], atlas)
    out["painter's order a, b"] = painter(0)
    out["painter's order b, a"] = painter(1)
    return out


def batch(n):
    """n jobs of mixed sizes with a job without a texel in the middle (n > 2)."""
    rng = np.random.default_rng(7 + n)
    jobs = []
    for i in range(n):
        w, h = WIDTHS[(3 * i) % len(WIDTHS)] + 2 * (i // 8), HEIGHTS[i % len(HEIGHTS)] + (i // 4)
        jobs.append(random_job(rng, w, h, n_glyphs=3 + i % 4))
    if n > 2:
        w0, h0, bg, glyphs, atlas = jobs[n // 2]
        jobs[n // 2] = (0, 5, bg, glyphs, atlas)
    return jobs
