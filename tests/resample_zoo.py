"""The resampler's zoo, shared by tests/test_emu_resample_zoo.py (k_ingest_wave on the lane emulator) and tests/test_gpu_resample_zoo.py (on
the device): the content real video holds and smooth sinusoids do not — constants, impulses, period-2 patterns, bi-level edges, near-black and
near-white ranges, hard alpha edges —, the smallest geometry at which each build of the kernel exists, an f64 witness that rounds where the
reference rounds, and the pools the two modules judge.  Pure numpy, seeded; nothing here touches a device.

The bars (the same in both modules):
  A      every byte within 1 LSB of orc.resample of the oracle's node texture;
  exact  a constant node gives that constant, an opaque source alpha 255, alpha 0 all zero, a second run the same bytes;
  B1     pooled per (build class, content class) over >= POOL_MIN bytes: the share of bytes equal to the oracle's >= FLOOR (the floor
         tests/test_emu_wave.py asks of the same source);
  B2     only where B1 misses: of the bytes where kernel and oracle differ, the kernel equals the witness in >= DISPUTE_SHARE.  Oracle and
         kernel both round the value the witness computes; where the oracle flips a share e of the bytes off the witness and the kernel a
         share k, they dispute about e + k of the bytes and the kernel is right in the e the oracle flipped: e / (e + k).  A kernel as
         accurate as the oracle (k = e) wins half, one with three times the oracle's error a quarter — the bar —, one that lost an operand's
         low half (k of the order of 100 e) a hundredth.
Colour bytes are pooled for opaque sources (their alpha is 255 by the exact property and would only dilute the share), all four bytes for
sources with an alpha channel."""
import zlib

import numpy as np

from oracle import oracle as orc
from tests.test_witness import lanczos_matrix, linear_to_srgb, srgb_to_linear, to_byte

TOL = 1
FLOOR = 0.9995
DISPUTE_SHARE = 0.25
POOL_MIN = 200_000
WITNESS_MAX_DIFF = 2e-4  # share of bytes in which the oracle may differ from the witness, per pool (a condition on the reference alone)
# Classes whose pool the witness cannot be held on (tests/test_emu_resample_zoo.py measures it): periodic content repeats ONE value over a
# whole tile, and where that value sits on a rounding boundary the f32 reference and the f64 witness part on every copy of it.  These are
# judged by B1 alone — no B2 for them.
WITNESS_NOT_HELD = {
    "checker_1": "one-tile geometry: the filtered checkerboard is one value near 0.5 on a boundary (code 187 | 188) — 1152 copies, 5.6e-3 of the pool",
    "alpha_blocks": "fractional crop: the top offset of 10.5 makes the vertical weights symmetric, alpha 0 | 255 meets at exactly 127.5 (2.0e-4)",
}


# ------------------------------------------------------------------------------------------------------------------ geometries
class Geo:
    """source -> tile, crop = (top, left, width, height) or None for the whole source; `check(plan)` says what the plan must be for the
    case to reach the build it is named after; `ks` = the (NKS, K, KV) k-step counts the emulator's band builder reports, where pinned."""

    def __init__(self, name, src, dst, check, crop=None, ks=None):
        self.name, self.src, self.dst, self.ks = name, src, dst, ks
        self.crop = tuple(float(c) for c in crop) if crop else (0.0, 0.0, float(src[0]), float(src[1]))
        self._check = check

    def plan(self):
        p = orc.resample_plan(self.src[0], self.src[1], self.crop, self.dst[0], self.dst[1])
        assert self._check(p), (self.name, p)
        return p

    @property
    def pixels(self):
        return self.dst[0] * self.dst[1]


def _two(first, levels=(0, 0)):
    return lambda p: p.kind == 2 and tuple(p.levels) == levels and tuple(p.axis[:2]) == (first, 1 - first)


GEOMETRIES = [
    Geo("4x2", (96, 60), (64, 40), _two(0), ks=(4, 4, 2)),
    Geo("ragged", (130, 74), (86, 49), _two(0)),                        # generic build: a last pair with one tile, partial tiles
    Geo("upscale", (64, 36), (96, 54), _two(0)),
    Geo("8x2", (256, 144), (128, 72), _two(0), ks=(5, 5, 2)),
    Geo("8x3", (384, 216), (128, 72), _two(0), ks=(7, 7, 3)),
    Geo("one_tile", (500, 96), (128, 48), lambda p: _two(0)(p) and p.scale[0] > 3.8),   # windows wider than 8 k-steps: one tile per wave
    Geo("v_first", (96, 60), (65, 40), _two(1)),
    Geo("width_only", (130, 74), (90, 74), lambda p: p.kind == 1 and p.axis[0] == 0 and tuple(p.levels) == (0, 0)),
    Geo("height_only", (130, 74), (130, 50), lambda p: p.kind == 1 and p.axis[0] == 1 and tuple(p.levels) == (0, 0)),
    Geo("crop_whole", (200, 120), (64, 40), _two(0), crop=(10, 20, 96, 60), ks=(4, 4, 2)),
    Geo("crop_fraction", (200, 120), (64, 40), _two(0), crop=(10.5, 20.25, 96, 60)),
    Geo("box_v_first", (640, 360), (100, 56), _two(1, (1, 1))),           # 2 x 2 box mean, residual 3.2 x 3.214
    Geo("box_h_first", (640, 360), (100, 57), _two(0, (1, 1))),           # ... residual 3.2 x 3.158
]
GEO = {g.name: g for g in GEOMETRIES}
NV12_GEOMETRIES = ("4x2", "8x2")


# ------------------------------------------------------------------------------------------------------------------ contents
CONSTANTS = [(0, 0, 0), (1, 2, 3), (5, 16, 64), (127, 128, 129), (200, 254, 255), (255, 255, 255)]
PATTERNS = ["white_impulses", "black_impulses", "impulses_on_grey", "checker_1", "stripes_3", "bilevel_blocks", "noise_0_8", "noise_247_255",
            "white_noise"]
OPAQUE_CLASSES = [f"const_{r}_{g}_{b}" for r, g, b in CONSTANTS] + PATTERNS
YUV_CLASSES = OPAQUE_CLASSES + ["white_noise_chroma"]
ALPHA_CLASSES = ["alpha_0", "const_alpha_128", "alpha_blocks", "white_ramp", "alpha_0_5", "noise_under_noise"]


def _blocks(w, h, rng):
    return np.kron(rng.integers(0, 2, ((h + 3) // 4, (w + 3) // 4)), np.ones((4, 4), np.int64))[:h, :w]


def _pattern(name, w, h, rng, k):
    """One plane of codes 0..255.  `k` turns the periodic patterns (0 vertical, 1 horizontal, 2 diagonal) so that the three channels of an
    RGB node differ; the phase comes from `rng`."""
    yy, xx = np.mgrid[0:h, 0:w]
    px, py = int(rng.integers(0, 7)), int(rng.integers(0, 5))
    if name in ("white_impulses", "black_impulses", "impulses_on_grey"):   # single texels on a 7 x 5 grid: what shows single weights
        base, on = {"white_impulses": (0, 255), "black_impulses": (255, 0), "impulses_on_grey": (118, 255)}[name]
        p = np.full((h, w), base, np.int64)
        p[py::5, px::7] = on
        if name == "impulses_on_grey":   # every other impulse black
            sub = p[py::5, px::7]
            sub[(np.add.outer(np.arange(sub.shape[0]), np.arange(sub.shape[1])) & 1) == 1] = 0
    elif name == "checker_1":
        p = ((xx + yy + px) & 1) * 255
    elif name == "stripes_3":
        p = (((xx, yy, xx + yy)[k % 3] + px) // 3 & 1) * 255
    elif name == "bilevel_blocks":
        p = _blocks(w, h, rng) * 255
    elif name == "noise_0_8":
        p = rng.integers(0, 9, (h, w))
    elif name == "noise_247_255":
        p = rng.integers(247, 256, (h, w))
    else:
        p = rng.integers(0, 256, (h, w))
    return p.astype(np.uint8)


def _seed(geo, name, salt):
    """The zoo's own geometries keep the seed they always had; any other (tests/small_tiles.py) is seeded by its name, sizes and crop — one
    entry more, so that it can never be one of the former."""
    cls = (OPAQUE_CLASSES + ["white_noise_chroma"] + ALPHA_CLASSES).index(name)
    if any(g is geo for g in GEOMETRIES):
        return [salt, GEOMETRIES.index(geo), cls]
    return [salt, zlib.crc32(repr((geo.name, tuple(geo.src), tuple(geo.dst), geo.crop)).encode()), cls, 1]


def opaque_node(geo, name):
    """RGBA8 node texture (alpha 255) of an opaque class."""
    w, h = geo.src
    node = np.full((h, w, 4), 255, np.uint8)
    if name.startswith("const_"):
        node[..., :3] = CONSTANTS[OPAQUE_CLASSES.index(name)]
    else:
        rng = np.random.default_rng(_seed(geo, name, 1))
        for k in range(3):
            node[..., k] = _pattern(name, w, h, rng, k)
    return node


def _y_of_code(c):
    """The limited-range luma of an sRGB code (16 + 219 c / 255): the same picture as Y."""
    return np.rint(16.0 + np.asarray(c, np.float64) * (219.0 / 255.0)).astype(np.uint8)


def yuv_planes(geo, name):
    """(y, u, v) of a 4:2:0 frame: the class as a luma pattern (constants: the triple's green code) under U = V = 128, and white noise under
    noise chroma."""
    w, h = geo.src
    rng = np.random.default_rng(_seed(geo, name, 2))
    u = np.full((h // 2, w // 2), 128, np.uint8)
    v = u.copy()
    if name.startswith("const_"):
        y = np.full((h, w), _y_of_code(CONSTANTS[OPAQUE_CLASSES.index(name)][1]), np.uint8)
    elif name == "white_noise_chroma":
        y = rng.integers(0, 256, (h, w), dtype=np.uint8)
        u, v = rng.integers(0, 256, u.shape, dtype=np.uint8), rng.integers(0, 256, u.shape, dtype=np.uint8)
    else:
        y = _y_of_code(_pattern(name, w, h, rng, 2))
    return y, u, v


def alpha_node(geo, name):
    """Premultiplied RGBA8 node texture (colour <= alpha on every texel) of an alpha class."""
    w, h = geo.src
    rng = np.random.default_rng(_seed(geo, name, 3))
    node = np.zeros((h, w, 4), np.uint8)
    colour = rng.integers(0, 256, (h, w, 3))
    if name == "alpha_0":
        return node
    if name == "const_alpha_128":
        node[...] = (100, 64, 20, 128)
        return node
    if name == "alpha_blocks":      # hard 0 / 255 edges over noise colour
        a = _blocks(w, h, rng) * 255
    elif name == "white_ramp":      # white under an alpha that climbs from 0 to 255 across the width
        a = np.broadcast_to(np.rint(np.arange(w) * 255.0 / (w - 1)).astype(np.int64), (h, w))
        colour = np.full((h, w, 3), 255)
    elif name == "alpha_0_5":
        a = rng.integers(0, 6, (h, w))
    else:
        a = rng.integers(0, 256, (h, w))
    node[..., :3] = colour * a[..., None] // 255
    node[..., 3] = a
    return node


def is_constant(name):
    return name.startswith("const_") or name == "alpha_0"


# ------------------------------------------------------------------------------------------------------------------ the witness
def f16(x):
    """Round to nearest even onto binary16 and back (the RGBA16F textures between the reference's passes)."""
    return np.asarray(x, np.float64).astype(np.float16).astype(np.float64)


def witness(node, crop, dw, dh):
    """RGBA8 node (sRGB colour, linear unorm8 alpha) -> dw x dh bytes by the plan the reference makes, in f64, rounding where the reference
    stores: the box mean (downsample.wgsl: clamp to edge, / fx fy) and pass 1 into RGBA16F, the last pass into sRGB bytes (alpha: unorm8).
    What it does not restate: the reference's f32 sums, its weights by rotation, its order of additions."""
    node = np.asarray(node)
    sh, sw = node.shape[:2]
    plan = orc.resample_plan(sw, sh, crop, dw, dh)
    assert plan.kind > 0
    cur = np.concatenate([srgb_to_linear(node[..., :3] / 255.0), node[..., 3:] / 255.0], -1)
    fx, fy = 1 << plan.levels[0], 1 << plan.levels[1]
    if fx * fy > 1:
        rw, rh = plan.reduced
        ix, iy = np.minimum(np.arange(rw * fx), sw - 1), np.minimum(np.arange(rh * fy), sh - 1)
        cur = f16(cur[iy][:, ix].reshape(rh, fy, rw, fx, 4).mean(axis=(1, 3)))
    for i in range(plan.kind):
        last = i == plan.kind - 1
        tw, th = (dw, dh) if last else plan.mid
        axis, scale, offset, perp = plan.axis[i], float(plan.scale[i]), float(plan.offset[i]), int(plan.perp_offset[i])
        if axis == 0:
            m = lanczos_matrix(cur.shape[1], tw, scale, offset)
            cur = np.einsum("xs,ysc->yxc", m, cur[np.clip(np.arange(th) + perp, 0, cur.shape[0] - 1)])
        else:
            m = lanczos_matrix(cur.shape[0], th, scale, offset)
            cur = np.einsum("ys,sxc->yxc", m, cur[:, np.clip(np.arange(tw) + perp, 0, cur.shape[1] - 1)])
        if not last:
            cur = f16(cur)
    return np.concatenate([to_byte(linear_to_srgb(cur[..., :3])), to_byte(cur[..., 3:])], -1)


# ------------------------------------------------------------------------------------------------------------------ judging
def check_case(got, want, node, name, opaque, again=None):
    """Bar A and the exact properties of one tile -> list of what failed (empty: nothing)."""
    bad = []
    d = np.abs(got.astype(np.int16) - want.astype(np.int16))
    if d.max() > TOL:
        bad.append(f"{name}: {(d > TOL).sum()} bytes off by more than {TOL} (max {d.max()}, first at {np.argwhere(d > TOL)[0].tolist()})")
    if opaque and not (got[..., 3] == 255).all():
        bad.append(f"{name}: {(got[..., 3] != 255).sum()} alpha bytes of an opaque source are not 255")
    if is_constant(name):
        c = node[0, 0]
        assert (node == c).all()
        if not (got == c).all():
            bad.append(f"{name}: constant {c.tolist()} came out as {np.unique(got.reshape(-1, 4), axis=0)[:4].tolist()}")
    if again is not None and not np.array_equal(got, again):
        bad.append(f"{name}: {(got != again).sum()} bytes differ on a second run")
    return bad


class Pool:
    """The tiles of one (build class, content class): what B1 and B2 are decided on."""

    def __init__(self, key, channels):
        self.key, self.channels, self.items = key, channels, []

    def add(self, got, want, node, crop):
        self.items.append((got[..., :self.channels], want[..., :self.channels], node, crop))

    @property
    def total(self):
        return sum(g.size for g, _, _, _ in self.items)

    @property
    def differing(self):
        return sum(int((g != w).sum()) for g, w, _, _ in self.items)

    @property
    def share(self):
        return 1.0 - self.differing / self.total

    def _witness(self, item):
        g, _, node, crop = item
        return witness(node, crop, g.shape[1], g.shape[0])[..., :self.channels]

    def disputes(self):
        """-> (bytes where kernel and oracle differ, how many of them the kernel has as the witness has them)"""
        n = won = 0
        for item in self.items:
            g, w = item[:2]
            m = g != w
            if m.any():
                n += int(m.sum())
                won += int((g[m] == self._witness(item)[m]).sum())
        return n, won

    def oracle_against_witness(self):
        """-> share of the pool's bytes in which the oracle differs from the witness"""
        return sum(int((w != self._witness(item)).sum()) for item in self.items for w in [item[1]]) / self.total

    def verdict(self):
        """-> (passes, one line for the record).  B1, else B2; never a number read off the kernel under test."""
        line = f"{self.key[0]:>6} {self.key[1]:<20} {self.total:>8} bytes, {self.differing:>5} differ, share {self.share:.6f}"
        if self.total < POOL_MIN:
            return False, line + f": pool below {POOL_MIN} bytes"
        if self.share >= FLOOR:
            return True, line
        n, won = self.disputes()
        if self.key[1] in WITNESS_NOT_HELD:
            return False, line + f" < {FLOOR}: no B2 for this class, the witness is not held on it (for the record: it has {won} of {n} disputes as the kernel)"
        return won >= DISPUTE_SHARE * n, line + f" < {FLOOR}: B2, {won} of {n} disputes go to the kernel"
