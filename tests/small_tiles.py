"""Tiles that grow from nothing, shared by tests/test_emu_small_tiles.py (k_ingest_wave on the lane emulator) and tests/test_gpu_small_tiles.py
(smr_render_layouts on the device).  A tile that opens in a transition passes through 1 x 1, 2 x 1, 3 x 2 ...: the sizes at which the
per-layout route choice of smr_render_layouts changes its mind most often — box levels 6 .. 0, either pass order, reduced sources at and
under the wave kernel's minimum of 8 x 2, one tile per wave, single-axis plans with and without a box level — and at which a context is
asked for a new weight band on every frame.  Contents, the f64 witness, check_case and Pool are tests/resample_zoo.py's.  Pure numpy, seeded;
nothing here touches a device.

A path is an ordered list of resample_zoo.Geo, each seeded by its own name, sizes and crop (so that two neighbouring frames of a path never
hold the same texels: a reduced or transposed texture left over from the frame before is a wrong tile, not a lucky one)."""
import math

from oracle import oracle as orc
from tests import resample_zoo as zoo

KINDS = ("yuv420", "opaque", "alpha")
CONTENTS = {
    "yuv420": ["const_5_16_64", "const_255_255_255", "white_impulses", "bilevel_blocks", "noise_0_8", "white_noise"],
    "opaque": ["const_5_16_64", "const_255_255_255", "white_impulses", "bilevel_blocks", "noise_0_8", "white_noise"],
    "alpha": ["alpha_0", "alpha_blocks", "noise_under_noise"],
}
WAVE_MIN = (8, 2)   # can_fuse_wave_rgba (smr_ingest_wave.h): the smallest source k_ingest_wave reads


def _dh(dw):
    return max(1, math.floor(dw * 9 / 16 + 0.5))


def _geo(path, src, dst, crop=None):
    return zoo.Geo(f"{path}_{src[0]}x{src[1]}_{dst[0]}x{dst[1]}", src, dst, lambda p: p.kind > 0, crop=crop)


def _paths():
    big, ragged, tiny_dst = (256, 144), (130, 74), [(1, 1), (3, 1), (5, 3), (16, 4), (17, 9), (33, 7)]
    return {
        "uniform": [_geo("uniform", big, (dw, _dh(dw))) for dw in range(1, 81)],
        # (up to 48 columns every plan of open_h still has a box level, and from 64, where it has none, up to 79 the window of a shrink by
        #  4 .. 3.24 is wider than the single-axis build takes: 80 and 81 are the first tiles that build gets.  The same for open_v: 36 rows is
        #  a shrink by 4 without a level, 45 and 46 the first the build gets, on the transposed node.)
        "open_h": [_geo("open_h", big, (dw, 144)) for dw in list(range(1, 49)) + [80, 81]],
        "open_v": [_geo("open_v", big, (256, dh)) for dh in list(range(1, 37)) + [45, 46]],
        # (3 x 2, reduced 9 x 5, is already the path's third tile; 1 x 17, reduced 3 x 37, is not on it)
        "ragged": [_geo("ragged", ragged, (dw, _dh(dw))) for dw in range(1, 41)] + [_geo("ragged", ragged, (1, 17))],
        # (40 columns leave a context at 66 bands, two over what it keeps: four tiles more for a margin)
        "crop": [_geo("crop", (200, 120), (dw, _dh(dw)), crop=(10.5, 20.25, 96, 60)) for dw in range(1, 45)],
        "tiny_src": [_geo("tiny_src", s, d) for s in [(8, 2), (8, 4), (12, 6), (6, 4), (4, 2), (2, 2), (1, 1)] for d in tiny_dst if s != d],
    }


PATHS = _paths()
# One tile of a shape the kernel has a build for that the emulator cannot run; tests/test_gpu_small_tiles.py holds wave_cases (below), this
# tile included, to the routes the device takes.  It is a height-only shrink by 4 without a box level: its windows are too wide for a column
# pair, and the host runs the single-axis build one tile per wave on the transposed node (make_wave_job_rgba_transposed allows that; the
# width-only twin of it goes to the pass kernels).  The emulator's entry point has no single-axis mode with one tile per wave.
EMU_NO_MODE = {"open_v_256x144_256x36"}


def takes(geo, kind):
    """Whether a source kind exists at this source size: planar 4:2:0 frames have even sizes, from 2 x 2."""
    return kind != "yuv420" or (geo.src[0] % 2 == 0 and geo.src[1] % 2 == 0)


def cases(path, kind):
    return [g for g in PATHS[path] if takes(g, kind)]


def node_of(geo, kind, name):
    """-> (the oracle's RGBA8 node texture, the (y, u, v) planes it was converted from or None)"""
    if kind == "yuv420":
        y, u, v = zoo.yuv_planes(geo, name)
        return orc.planar_yuv_to_rgba(y, u, v, geo.src[0], geo.src[1]), (y, u, v)
    return (zoo.opaque_node(geo, name) if kind == "opaque" else zoo.alpha_node(geo, name)), None


def plan_text(plan):
    """One cell of the route table: kind, first axis, box levels, reduced size, scales."""
    first = "hv"[plan.axis[0]] + ("hv"[plan.axis[1]] if plan.kind == 2 else "")
    scales = " x ".join(f"{plan.scale[i]:.3f}" for i in range(plan.kind))
    return f"{first:<2} levels {tuple(plan.levels)} reduced {plan.reduced[0]}x{plan.reduced[1]} scale {scales}"


def wave_shape(plan):
    """What a plan is to the matrix-core kernel, judged as the host judges it before it looks at window widths:
    None — not the kernel's (a single-axis plan behind a box level, which the host sends to the pass kernels; a reduced source under the
    kernel's minimum, transposed for a vertical first pass); else "two" | "single"."""
    boxed = tuple(plan.levels) != (0, 0)
    if plan.kind == 1 and boxed:
        return None
    w, h = plan.reduced
    if plan.axis[0] == 1:
        w, h = h, w
    if w < WAVE_MIN[0] or h < WAVE_MIN[1]:
        return None
    return "two" if plan.kind == 2 else "single"


def wave_cases(path, kind):
    """The tiles of a path the host sends to k_ingest_wave (whichever build), known without a device."""
    return [g for g in cases(path, kind) if wave_shape(g.plan()) is not None]


class Pool(zoo.Pool):
    """resample_zoo.Pool over thousands of tiles: an item keeps its Geo in place of the node texture, and the node is made again for the few
    tiles the witness is asked about."""

    def __init__(self, key, channels, kind):
        super().__init__(key, channels)
        self.kind = kind

    def _witness(self, item):
        g, _, geo, crop = item
        node, _ = node_of(geo, self.kind, self.key[1])
        return zoo.witness(node, crop, g.shape[1], g.shape[0])[..., :self.channels]
