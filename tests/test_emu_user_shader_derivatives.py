"""Screen-space derivatives of user shaders (SMR_DERIVATIVES: smr_dpdx, smr_dpdy, smr_fwidth and their _fine / _coarse forms on 2 x 2 pixel
quads with helper invocations) on the lane emulator: smr_user_shader_prelude.h compiled for the CPU by tests/emu/emu_user_shader_quad.cpp —
one host thread per lane, quad exchanges at a barrier per quad — with a fixture of tests/user_shader_sources_derivatives.py in the user's
place.  The expected pictures come from the numpy model below, written from the rules of include/smr.h: the fragment's inputs in f64 at EVERY
pixel centre of the target padded to even width and height, no coverage applied (a helper's inputs are the same formulas at its own centre);
the quad differences; then coverage, blend and store.  Its geometry is that of the sibling models (tests/test_emu_user_shader_affine.py,
_clip.py, _varyings.py; held equal to them by a test here) — never the code under test.  Decode, encode, caps and the comparison are those
files'.  tests/test_gpu_user_shader_derivatives.py holds the compiled programs to the same model."""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import emu_build
from tests import test_emu_user_shader_affine as A
from tests import test_emu_user_shader_clip as M
from tests import test_emu_user_shader_varyings as V
from tests import user_shader_sources_derivatives as SD
from tests import user_shader_sources_varyings as SV
from tests.test_emu_user_shader_affine import CAP, EDGE, TEXEL, ROTATION, SPAN_EDGE, decode, encode, pack, run, sources
from tests.test_emu_user_shader_clip import f32
from tests.test_gpu_shaders import _textures

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
P8 = C.POINTER(C.c_uint8)
PI = C.POINTER(C.c_int)

W, H = A.W, A.H  # 70 x 9: two workgroup columns, three rows of workgroups, the last column and row of quads half outside


# ------------------------------------------------------------------------------------------------------------------ the model
class Grid:
    """the pixel centres of a Wt x Ht target padded to even width and height (the quads of the contract), normalised by the true size"""

    def __init__(self, Wt, Ht):
        self.W, self.H, self.We, self.He = Wt, Ht, Wt + (Wt & 1), Ht + (Ht & 1)
        ys, xs = np.mgrid[0:self.He, 0:self.We]
        self.px, self.py = xs + 0.5, ys + 0.5
        self.X, self.Y = self.px / Wt * 2.0 - 1.0, 1.0 - self.py / Ht * 2.0
        self.inside = (xs < Wt) & (ys < Ht)

    def _q(self, a):
        return np.asarray(a, np.float64).reshape(self.He // 2, 2, self.We // 2, 2)

    def _back(self, d):
        return np.broadcast_to(d, (self.He // 2, 2, self.We // 2, 2)).reshape(self.He, self.We)

    # quad a = (x0, y0), b = (x0 + 1, y0), c = (x0, y0 + 1), d = (x0 + 1, y0 + 1); window y grows downwards
    def dpdx_coarse(self, a):
        q = self._q(a)
        return self._back(q[:, 0:1, :, 1:2] - q[:, 0:1, :, 0:1])  # b - a for all four

    def dpdy_coarse(self, a):
        q = self._q(a)
        return self._back(q[:, 1:2, :, 0:1] - q[:, 0:1, :, 0:1])  # c - a for all four

    def dpdx_fine(self, a):
        q = self._q(a)
        return self._back(q[:, :, :, 1:2] - q[:, :, :, 0:1])  # the pixel's own row: right - left

    def dpdy_fine(self, a):
        q = self._q(a)
        return self._back(q[:, 1:2, :, :] - q[:, 0:1, :, :])  # the pixel's own column: lower - upper

    dpdx, dpdy = dpdx_coarse, dpdy_coarse  # the plain forms are the coarse ones: a definition (include/smr.h)

    def fwidth(self, a, flavour=""):
        return np.abs(getattr(self, "dpdx" + flavour)(a)) + np.abs(getattr(self, "dpdy" + flavour)(a))

    def quad_all(self, mask):
        return self._back(self._q(mask).astype(bool).all(axis=(1, 3), keepdims=True))


def affine_layers(g, planes, first=0):
    """one layer per drawn plane {xx, xy, yx, yy, cx, cy}: the rules of A.quad_coordinates and A.model on the padded grid.  A layer is a dict:
    plane_id, cover and near (the doubt rule's "an edge passes too close"), and the fragment's inputs u, v at every centre of the grid"""
    out = []
    for n, m in enumerate(planes):
        xx, xy, yx, yy, cx, cy = [float(v) for v in m]
        if xy == 0.0 and yx == 0.0:
            if not (xx > 0.0) or not (yy > 0.0):
                continue
            qx, qy = (g.X - cx) / xx, (g.Y - cy) / yy
        else:
            det = xx * yy - xy * yx
            if not math.isfinite(det) or not det > 0.0 or not math.isfinite(f32(det)):
                continue
            dx, dy = g.X - cx, g.Y - cy
            qx, qy = (dx * yy - dy * xy) / det, (dy * xx - dx * yx) / det
        near_x, near_y = np.abs(np.abs(qx) - 1.0) < EDGE, np.abs(np.abs(qy) - 1.0) < EDGE
        near = (near_x & (np.abs(qy) < 1.0 + EDGE)) | (near_y & (np.abs(qx) < 1.0 + EDGE))
        cover = (qx >= -1.0) & (qx < 1.0) & (qy > -1.0) & (qy <= 1.0) & g.inside
        out.append(dict(plane_id=first + n, cover=cover, near=near & g.inside, u=(qx + 1.0) / 2.0, v=(1.0 - qy) / 2.0, S=None))
    return out


def plane_layers(g, planes, first=0):
    """smr_plane {sx, sy, cx, cy}"""
    return affine_layers(g, [[p[0], 0.0, 0.0, p[1], p[2], p[3]] for p in planes], first)


def whole_target_layers(g, n_src):
    """no vertex stage: every plane covers the target; plane_id -1 alone when there is no source"""
    return affine_layers(g, [[1.0, 0.0, 0.0, 1.0, 0.0, 0.0]] * max(n_src, 1), first=0 if n_src else -1)


def clip_layers(g, planes, modes="", first=0):
    """one layer per drawn TRIANGLE of planes of four vertices [x, y, z, w, u, v, t_0 ..]: the rules of M.model and V.model, line for line,
    on the padded grid.  Every interpolated input is the triangle's own plane over the whole grid: what a helper of that triangle gets.
    S = sum E_i is kept: where it is <= 0 at a pixel of a quad the extrapolated quotients mean nothing (a vertex behind the eye)"""
    out = []
    N = len(modes)
    for n, verts in enumerate(planes):
        vs = np.array([[V.value(c) for c in v] for v in verts], np.float64)
        smooth = [6 + j for j in range(N) if modes[j] != "F"]
        with np.errstate(all="ignore"):
            for ti, tri in enumerate(M.TRIANGLES):
                p = [np.array([vs[k, 0], vs[k, 1], vs[k, 3]]) for k in tri]
                coef = [np.cross(p[(i + 1) % 3], p[(i + 2) % 3]) for i in range(3)]
                D = float(np.dot(p[0], coef[0]))
                if not math.isfinite(D) or not D > 0.0 or not math.isfinite(f32(D)):
                    continue
                attrs = vs[list(tri)]
                if not np.isfinite(attrs[:, :6]).all() or not np.isfinite(attrs[:, smooth]).all():
                    continue
                E = [c[0] * g.X + c[1] * g.Y + c[2] for c in coef]
                mag = [abs(c[0] * g.X) + abs(c[1] * g.Y) + abs(c[2]) for c in coef]
                incl = [c[0] > 0.0 or (c[0] == 0.0 and c[1] < 0.0) for c in coef]
                z, q, w = attrs[:, 2], attrs[:, 3] - attrs[:, 2], attrs[:, 3]
                E += [sum(E[i] * z[i] for i in range(3)), sum(E[i] * q[i] for i in range(3))]
                mag += [sum(np.abs(E[i] * z[i]) for i in range(3)), sum(np.abs(E[i] * q[i]) for i in range(3))]
                incl += [True, True]
                cover = g.inside.copy()
                near = np.zeros(cover.shape, bool)
                outside = np.zeros(cover.shape, bool)
                for e, m, inc in zip(E, mag, incl):
                    cover &= (e > 0.0) | ((e == 0.0) & inc)
                    near |= np.abs(e) < EDGE * m
                    outside |= e < -EDGE * m
                S = E[0] + E[1] + E[2]
                Wn = sum(E[i] * w[i] for i in range(3))
                vary = []
                for j in range(N):
                    t = attrs[:, 6 + j]
                    if modes[j] == "P":
                        vary.append(sum(E[i] * t[i] for i in range(3)) / S)
                    elif modes[j] == "L":
                        vary.append(sum(E[i] * (t[i] * w[i]) for i in range(3)) / Wn)
                    else:
                        vary.append(np.full(S.shape, t[0]))
                out.append(dict(plane_id=first + n, triangle=ti, cover=cover, near=near & ~outside & g.inside,
                                u=sum(E[i] * attrs[i, 4] for i in range(3)) / S, v=sum(E[i] * attrs[i, 5] for i in range(3)) / S, vary=vary,
                                S=S, Smag=np.abs(E[0]) + np.abs(E[1]) + np.abs(E[2])))
    return out


# u = N / S in f32 carries a relative error of about 2^-22 * sum |E_i| / S: with S at least this share of sum |E_i| at all four pixels of a
# quad the error of a difference, times the fixtures' k <= 1, stays under 1e-4.  Below it (a plane that passes behind the eye) the
# derivative channels are not compared: only coverage
WELL_CONDITIONED = 0.05


def model(g, layers, textures, srgb, fragment):
    """-> (RGBA8 picture, doubt mask, smallest texel-boundary distance of a compared pixel, mask of pixels whose colour is not compared: a
    quad-mate has S <= 0 or nearly, list of the layers' cover masks).  `fragment(g, layer, dec)` -> (premultiplied colours (He, We, 4) at EVERY
    centre of the grid — quad differences included — and texel margins or None); coverage is applied here, after the differences:
    premultiplied OVER per layer in order, stored to the RGBA8 target and read back before the next."""
    dec = [None if t is None else decode(t, srgb) for t in textures]
    out = np.zeros((g.H, g.W, 4), np.uint8)
    doubt = np.zeros((g.H, g.W), bool)
    loose = np.zeros((g.H, g.W), bool)
    margin = np.inf
    covers = []
    for L in layers:
        doubt |= L["near"][:g.H, :g.W]
        cover = L["cover"][:g.H, :g.W]
        covers.append(cover)
        with np.errstate(all="ignore"):
            f, mg = fragment(g, L, dec)
        if L["S"] is not None:
            loose |= (cover & ~g.quad_all(L["S"] >= WELL_CONDITIONED * L["Smag"])[:g.H, :g.W])
        if mg is not None:
            margin = min(margin, float(mg[:g.H, :g.W][cover & ~doubt].min(initial=np.inf)))
        fc = np.nan_to_num(f[:g.H, :g.W][cover], nan=0.0, posinf=2.0, neginf=-1.0)
        acc = decode(out[cover], srgb)
        out[cover] = encode(fc + acc * (1.0 - fc[:, 3:4]), srgb)
    return out, doubt, margin, loose, covers


def check(got, m, what):
    """the project's comparison (A.compare): <= 1 LSB outside the doubtful pixels, those few, no compared pixel on a texel boundary.  Where a
    quad-mate lies behind the eye only alpha (coverage) is compared"""
    want, doubt, margin, loose, _ = m
    g = got.copy()
    g[loose, :3] = want[loose, :3]
    A.compare(g, want, doubt, margin if np.isfinite(margin) else 1.0, what)
    assert np.array_equal(got.any(axis=-1)[~doubt], want.any(axis=-1)[~doubt]), f"{what}: coverage differs from the model's"


def nearest(L, dec, g):
    """A.nearest_fragment at every centre of the grid (a helper's extrapolated uv may leave the source: its texel is dropped with it)"""
    t = dec[L["plane_id"]]
    h, w = t.shape[:2]
    fu, fv = L["u"] * w, L["v"] * h
    tx = np.clip(np.nan_to_num(np.floor(fu)), 0, w - 1).astype(int)
    ty = np.clip(np.nan_to_num(np.floor(fv)), 0, h - 1).astype(int)
    return t[ty, tx], np.minimum(np.abs(fu - np.round(fu)), np.abs(fv - np.round(fv)))


def position_fragment(flavour):
    def fragment(g, L, dec):
        dx, dy = getattr(g, "dpdx" + flavour), getattr(g, "dpdy" + flavour)
        return np.stack([dx(g.px), dy(g.py), dx(g.py), dy(g.px)], axis=-1), None
    return fragment


def edge_fragment(flavour):
    def fragment(g, L, dec):
        dx, dy = getattr(g, "dpdx" + flavour), getattr(g, "dpdy" + flavour)
        return np.stack([0.5 + SD.EDGE_KX * dx(L["u"]), 0.5 + SD.EDGE_KY * dy(L["v"]), 0.5 + dy(L["u"]) + dx(L["v"]), np.ones(g.X.shape)], axis=-1), None
    return fragment


def product_fragment(axis):
    def fragment(g, L, dec):
        t = g.px * g.py
        return np.stack([getattr(g, f"dpd{axis}_fine")(t) / 8.0, getattr(g, f"dpd{axis}_coarse")(t) / 8.0, getattr(g, f"dpd{axis}")(t) / 8.0,
                         np.ones(g.X.shape)], axis=-1), None
    return fragment


def disc_fragment(g, L, dec):
    """SD.DISC"""
    dx, dy = g.px - (0.5 * g.W + f32(0.3)), g.py - (0.5 * g.H + f32(0.1))
    d = np.sqrt(dx * dx + dy * dy)
    cover = np.clip(0.5 - (d - f32(0.4) * min(g.W, g.H)) / g.fwidth(d), 0.0, 1.0)
    t, mg = nearest(L, dec, g)
    return t * cover[..., None], mg


def overlap_fragment(g, L, dec):
    """SD.OVERLAP"""
    t, mg = nearest(L, dec, g)
    if L["plane_id"] < 1:
        return t, mg
    return np.stack([0.5 * (0.25 + g.fwidth(L["u"])), 0.5 * (0.25 + g.fwidth(L["v"])), 0.5 * t[..., 2], np.full(g.X.shape, 0.5)], axis=-1), mg


def perspective_fragment(g, L, dec):
    """SD.PERSPECTIVE"""
    k = SD.PERSPECTIVE_K
    return np.stack([0.5 * (0.5 + k * g.dpdx(L["u"])), 0.5 * (0.5 + k * g.dpdy(L["v"])), 0.5 * (0.5 + k * g.dpdx_fine(L["vary"][0])),
                     np.full(g.X.shape, 0.5)], axis=-1), None


# ---- the cases' constants
SIZES_1 = [(70, 6), (67, 5)]  # two workgroup columns, two rows, both partial; odd: the last column and row of quads have helpers outside
# case 2: an smr_plane of 32 x 4 pixels on 64 x 8 whose left / top edges fall on odd pixels (columns 17 .. 48, rows 3 .. 6: every edge quad is
# half helpers), and the same shifted by one pixel (M.TIE_PLANE: columns 16 .. 47, rows 2 .. 5)
EDGE_PLANES = {"odd": ([0.5, 0.5, 0.046875, -0.375], (17, 49, 3, 7)), "even": (M.TIE_PLANE, (16, 48, 2, 6))}
# case 5: A.SPAN_EDGE moved 32 pixels to the left: its corners lie around x = 32, where two waves of a quad-mode workgroup meet
SPAN_32 = [p[:4] + [f32(p[4] - 64.0 / W), p[5]] for p in SPAN_EDGE]
OVERLAP_CASES = {"rotation": ROTATION, "span_64": SPAN_EDGE, "span_32": SPAN_32}
PERSPECTIVE_CASES = {"flip": (V.FLIP_V, sources, (W, H)), "flip_65x5": (V.FLIP_V, sources, (65, 5)), "span": (V.SPAN_V, sources, (W, H)),
                     "behind": (V.BEHIND_V, lambda: sources()[:1], (W, H))}
DISC_SIZES = [(W, H), (34, 31)]  # (a disc of 7 pixels in one wave's rows; one of 25 across x = 32 and eight rows of quads, both sides odd)


def position_model(flavour, size, srgb):
    g = Grid(*size)
    return model(g, whole_target_layers(g, 0), [], srgb, position_fragment(flavour))


def edge_model(flavour, which, srgb):
    g = Grid(64, 8)
    return model(g, plane_layers(g, [EDGE_PLANES[which][0]]), sources()[:1], srgb, edge_fragment(flavour))


def product_model(axis, srgb):
    g = Grid(8, 8)
    return model(g, whole_target_layers(g, 0), [], srgb, product_fragment(axis))


def disc_model(textures, size, srgb):
    g = Grid(*size)
    return model(g, whole_target_layers(g, len(textures)), textures, srgb, disc_fragment)


def overlap_model(case, srgb):
    g = Grid(W, H)
    return model(g, affine_layers(g, OVERLAP_CASES[case]), sources(), srgb, overlap_fragment)


def perspective_model(case, srgb):
    planes, tex, size = PERSPECTIVE_CASES[case]
    g = Grid(*size)
    return model(g, clip_layers(g, planes, SV.PERSP_MODES), tex(), srgb, perspective_fragment)


def test_the_model_is_its_siblings_and_its_constants_stay_under_the_caps():
    """What the other tests assume, checked with the models alone: without a derivative this file's geometry draws the sibling models'
    pictures; every (case, size) used stays under CAP and TEXEL; the differenced values times k leave room in [0, 1]; the cases hold what
    they are for (helpers outside an odd target, edge quads half helpers, a quad cut by the diagonal, an edge at x = 32, S <= 0 in a quad)."""
    def plain_nearest(g, L, dec):
        return nearest(L, dec, g)
    for srgb in (True, False):
        for planes in (ROTATION, SPAN_EDGE):
            g = Grid(W, H)
            mine, theirs = model(g, affine_layers(g, planes), sources(), srgb, plain_nearest), A.model(planes, sources(), W, H, srgb)
            assert np.array_equal(mine[0], theirs[0]) and np.array_equal(mine[1], theirs[1]) and mine[2] == theirs[2]
        for planes, size in ((M.FLIP, (W, H)), (M.FLIP, (65, 5)), (M.SPAN, (W, H)), (M.BEHIND, (W, H))):
            g = Grid(*size)
            tex = sources()[:len(planes)]
            mine, theirs = model(g, clip_layers(g, planes), tex, srgb, plain_nearest), M.model(planes, tex, *size, srgb)
            assert np.array_equal(mine[0], theirs[0]) and np.array_equal(mine[1], theirs[1]) and mine[2] == theirs[2]
        for case in OVERLAP_CASES:
            want, doubt, margin, loose, covers = overlap_model(case, srgb)
            assert doubt.mean() <= CAP and margin > TEXEL and not loose.any() and all(c.any() for c in covers), (case, doubt.mean(), margin)
            assert (covers[0] & covers[1]).any() or case != "rotation"  # (the planes overlap: the blend order and the read-back show)
        for case in PERSPECTIVE_CASES:
            want, doubt, margin, loose, covers = perspective_model(case, srgb)
            assert doubt.mean() <= CAP and (case == "behind" or not loose.any()), (case, doubt.mean(), loose.sum())
            keep = want.any(axis=-1) & ~loose
            assert want[keep][:, :3].min() > 5 and want[keep][:, :3].max() < 250, case  # (no compared channel is clamped)
        for size in DISC_SIZES:
            want, doubt, margin, loose, covers = disc_model(sources(), size, srgb)
            assert not doubt.any() and margin > TEXEL, (size, margin)
            a = want[..., 3]
            assert (a == 0).any() and (a > 200).any() and ((a > 20) & (a < 200)).sum() >= 6, size  # outside, inside, and an edge in between
    # the renderer case of tests/test_gpu_user_shader_derivatives.py: the disc over one 16 x 8 input stream, a 48 x 24 target
    want, doubt, margin, loose, covers = disc_model(_textures(1, M.IW, M.IH), (48, 24), True)
    assert not doubt.any() and margin > TEXEL and want[:, 32:, 3].any() and not want[0].any()
    # case 1: the padded grid has a column and a row outside 67 x 5
    g = Grid(67, 5)
    assert (g.We, g.He) == (68, 6) and not g.inside[:, 67].any() and not g.inside[5].any()
    # case 2: the covered rectangles; with odd edges every edge quad holds helpers
    for which, (plane, (x0, x1, y0, y1)) in EDGE_PLANES.items():
        g = Grid(64, 8)
        cover = plane_layers(g, [plane])[0]["cover"]
        want = np.zeros((8, 64), bool)
        want[y0:y1, x0:x1] = True
        assert np.array_equal(cover, want), which
        assert (g.quad_all(cover) != cover).any() == (which == "odd")
    # case 5: corners either side of x = 32 and (the sibling's constants) of x = 64
    g = Grid(W, H)
    for planes, x in ((SPAN_32, 32), (SPAN_EDGE, 64)):
        first, second = [L["cover"] for L in affine_layers(g, planes)]
        assert first[:, x].any() and not first[:, x + 1:].any() and first[:, :x].any(), x
        assert second[:, x - 1].any() and not second[:, :x - 1].any() and second[:, x:].any(), x
    assert any(L["cover"][:, 32].any() and not L["cover"][:, 31].all() for L in affine_layers(g, ROTATION))
    # case 6: a quad holds pixels of both triangles of one plane; one plane set has vertices behind the eye
    tris = clip_layers(g, V.FLIP_V, SV.PERSP_MODES)
    assert len(tris) == 4 and [t["triangle"] for t in tris] == [0, 1, 0, 1]
    a, b = tris[0]["cover"], tris[1]["cover"]
    qa, qb = ~g.quad_all(~a), ~g.quad_all(~b)  # quads with a pixel of the triangle
    assert (qa & qb).sum() >= 8 and not (a & b).any()
    assert min(v[3] for v in V.BEHIND_V[0]) < 0.0 and any(L["cover"].any() for L in clip_layers(g, V.BEHIND_V, SV.PERSP_MODES))


# ------------------------------------------------------------------------------------------------------------------ the emulator
def build(name):
    """tests/emu/_build/libsmr_emu_user_quad_<name>.so: emu_user_shader_quad.cpp (one host thread per lane, a barrier per quad) with the
    fixture as the user's translation unit"""
    out_dir = os.path.join(emu_build.EMU, "_build")
    os.makedirs(out_dir, exist_ok=True)
    user = os.path.join(out_dir, f"user_shader_quad_{name}.inc")
    text = "// generated from tests/user_shader_sources_derivatives.py\n" + SD.ALL[name]
    if not os.path.exists(user) or open(user).read() != text:
        with open(user, "w") as f:
            f.write(text)
    lib = os.path.join(out_dir, f"libsmr_emu_user_quad_{name}.so")
    deps = [user, os.path.join(emu_build.EMU, "emu_user_shader_quad.cpp"), os.path.join(emu_build.EMU, "emu_device.h"), os.path.join(emu_build.EMU, "emu_guard.h"),
            os.path.join(emu_build.EMU, "shim/hip/hip_runtime.h")] + [os.path.join(emu_build.CSRC, h) for h in
                                                                       ("smr_internal.h", "smr_shader_dev.h", "smr_user_shader_prelude.h", "smr_tables.h")]
    if not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(d) for d in deps):
        cmd = [emu_build.CLANG, "-std=c++17", "-fPIC", "-shared", "-DSMR_EMU=1", "-ffp-contract=off", "-Wno-unused-function", "-O2",
               f'-DSMR_EMU_USER_SOURCE="{user}"', "-I", os.path.join(emu_build.EMU, "shim"), "-I", emu_build.EMU, "-I", emu_build.CSRC,
               "-I", os.path.join(ROOT, "include"), "-o", lib, deps[1], "-lpthread"]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    h = C.CDLL(lib)
    h.emu_user_shader.argtypes = [C.c_int, C.POINTER(P8), PI, PI, C.c_int, C.c_int, C.c_int, C.c_float, P8, C.c_uint32, P8]
    h.emu_user_shader.restype = C.c_int
    return h


_EMUS = {}


def emu(name, guard=0):
    if not os.path.exists(emu_build.CLANG):
        pytest.skip("no clang++ to build the emulator with")
    if name not in _EMUS:
        _EMUS[name] = build(name)
    _EMUS[name].emu_set_guard(guard, 1 if guard else 0)
    return _EMUS[name]


def check_position(got, flavour, size, srgb):
    """case 1: (1, 1, 0, 0) on every pixel, byte for byte — and the model says the same"""
    want = encode(np.array([1.0, 1.0, 0.0, 0.0]), srgb)
    assert got.shape == (size[1], size[0], 4) and (got == want).all(), f"{flavour} {size}: {(got != want).any(axis=-1).sum()} pixels are not {want}"
    assert np.array_equal(position_model(flavour, size, srgb)[0], got)


def check_edge(got, flavour, which, srgb):
    """case 2: dpdx(uv.x) = 1 / 32 and dpdy(uv.y) = 1 / 4 exactly on every covered pixel, the edge columns and rows included; nothing elsewhere.
    (Every centre on the left and top edges is "doubtful" to the model's rule; the arithmetic is exact here, so all are compared.)"""
    x0, x1, y0, y1 = EDGE_PLANES[which][1]
    want = np.zeros((8, 64, 4), np.uint8)
    want[y0:y1, x0:x1] = encode(np.array([0.5 + SD.EDGE_KX / 32.0, 0.5 + SD.EDGE_KY / 4.0, 0.5, 1.0]), srgb)
    assert np.array_equal(got, want), f"{flavour} {which}: {(got != want).any(axis=-1).sum()} pixels differ"
    assert np.array_equal(edge_model(flavour, which, srgb)[0], got)


def check_product(got, axis, srgb):
    """case 3: t = position.x * position.y on 8 x 8.  Along x: fine is y + 0.5 of the pixel's own row, coarse y0 + 0.5 for both rows of the quad;
    along y the mirror image; plain equals coarse.  Exact in f32 (half-integers below 8 and their products), so byte for byte"""
    ys, xs = np.mgrid[0:8, 0:8]
    own, first = (ys, ys & ~1) if axis == "x" else (xs, xs & ~1)
    want = encode(np.stack([(own + 0.5) / 8.0, (first + 0.5) / 8.0, (first + 0.5) / 8.0, np.ones((8, 8))], axis=-1), srgb)
    assert np.array_equal(got, want), f"{axis}: {(got != want).any(axis=-1).sum()} pixels differ"
    assert np.array_equal(got[..., 1], got[..., 2]) and not np.array_equal(got[..., 0], got[..., 1])
    assert np.array_equal(product_model(axis, srgb)[0], got)


@pytest.mark.parametrize("srgb", [True, False])
@pytest.mark.parametrize("size", SIZES_1)
@pytest.mark.parametrize("flavour", sorted(SD.FLAVOURS))
def test_the_derivatives_of_position_are_exact(flavour, size, srgb):
    check_position(run(emu(f"position_{flavour}"), [], *size, srgb=srgb), SD.FLAVOURS[flavour], size, srgb)


@pytest.mark.parametrize("srgb", [True, False])
@pytest.mark.parametrize("which", sorted(EDGE_PLANES))
@pytest.mark.parametrize("flavour", sorted(SD.FLAVOURS))
def test_helpers_on_a_plane_edge_give_the_edge_pixels_their_derivatives(flavour, which, srgb):
    got = run(emu(f"edge_{flavour}"), sources()[:1], 64, 8, pack([EDGE_PLANES[which][0]]), srgb=srgb)
    check_edge(got, SD.FLAVOURS[flavour], which, srgb)


@pytest.mark.parametrize("srgb", [True, False])
@pytest.mark.parametrize("axis", ["x", "y"])
def test_fine_takes_the_pixels_own_row_and_coarse_the_quads_first(axis, srgb):
    check_product(run(emu(f"product_{axis}"), [], 8, 8, srgb=srgb), axis, srgb)


@pytest.mark.parametrize("srgb", [True, False])
@pytest.mark.parametrize("size", DISC_SIZES)
def test_an_anti_aliased_disc_by_fwidth_matches_the_model(size, srgb):
    got = run(emu("disc"), sources(), *size, srgb=srgb)
    check(got, disc_model(sources(), size, srgb), f"disc {size}")


@pytest.mark.parametrize("srgb", [True, False])
@pytest.mark.parametrize("case", sorted(OVERLAP_CASES))
def test_overlapping_rotated_planes_with_fwidth_match_the_model(case, srgb):
    """per-plane helpers, the blend order and the read-back between planes; plane corners either side of x = 64 and of x = 32"""
    got = run(emu("overlap"), sources(), W, H, pack(OVERLAP_CASES[case]), srgb=srgb)
    check(got, overlap_model(case, srgb), case)


@pytest.mark.parametrize("srgb", [True, False])
@pytest.mark.parametrize("case", sorted(PERSPECTIVE_CASES))
def test_derivatives_in_perspective_match_the_model(case, srgb):
    """dpdx(uv), dpdy(uv) and the fine dpdx of a perspective varying; a quad cut by the shared diagonal runs once per triangle, each time with
    that triangle's extrapolation; behind the eye (S <= 0 in the quad) only coverage is held"""
    planes, tex, size = PERSPECTIVE_CASES[case]
    got = run(emu("perspective"), tex(), *size, V.pack_planes(planes), srgb=srgb)
    check(got, perspective_model(case, srgb), case)


def remap_cases():
    """case 7: (fixture, the emulator of the original, sources, size, parameter bytes) over the stage's existing plane sets and sizes"""
    out = {}
    for name, (plane, size) in {"inset": ([0.5, 0.25, 0.1, -0.2], (W, H)), "tie": (M.TIE_PLANE, (64, 8))}.items():
        out[f"plane_param-{name}"] = ("plane_param", A.emu, lambda: sources()[:1], size, pack([plane]))
    for name, planes in {"axis_aligned": [[0.5, 0.0, 0.0, 0.25, 0.1, -0.2]], "rotation": ROTATION, "span_edge": SPAN_EDGE}.items():
        out[f"affine_param-{name}"] = ("affine_param", A.emu, sources, (W, H), pack(planes))
    for name, (planes, tex, size) in dict(V.UNUSED_CASES, flip_65x5=(M.FLIP, sources, (65, 5)), flip_1x1=(M.FLIP, sources, (1, 1))).items():
        out[f"clip_param-{name}"] = ("clip_param", M.emu, tex, size, M.pack_planes(planes))
    for name, (fixture, planes, modes, tex, size, params) in V.SMOOTH_CASES.items():
        if fixture == "vary_param":
            out[f"vary_param-{name}"] = ("vary_param", V.emu, tex, size, params)
    return out


REMAP = remap_cases()


@pytest.mark.parametrize("srgb", [True, False])
@pytest.mark.parametrize("case", sorted(REMAP))
def test_the_quad_lane_map_draws_the_same_picture(case, srgb):
    fixture, original, tex, size, params = REMAP[case]
    before = run(original(fixture), tex(), *size, params, srgb=srgb)
    after = run(emu(f"remap_{fixture}"), tex(), *size, params, srgb=srgb)
    assert before.any() and np.array_equal(before, after), f"{(before != after).sum()} bytes differ"


@pytest.mark.parametrize("name", sorted(SD.MISUSE))
def test_a_derivative_without_the_macro_is_a_compile_error_that_names_it(name):
    import __graft_entry__ as ge
    ge.build()
    from smelter_amd import _ffi, hip
    hip.ShaderProgram(SD.ALL[name]).close()  # (the same source with the define compiles: the error below is the missing define's)
    with pytest.raises(hip.ShaderCompileError) as e:
        hip.ShaderProgram(SD.MISUSE[name])
    assert e.value.code == -1  # SMR_ERR_INVALID
    assert SD.MISUSE_ERROR in e.value.log and "at the top of the shader source" in e.value.log, e.value.log
    # through the C ABI: a program object with the log and no code object — nothing to register or launch
    lib = _ffi.load()
    h = C.c_void_p()
    assert lib.smr_shader_program_create(SD.MISUSE[name].encode(), C.byref(h)) == _ffi.SMR_ERR_INVALID and h.value
    p, n = C.c_void_p(), C.c_size_t()
    assert lib.smr_shader_program_code(h, C.byref(p), C.byref(n)) == _ffi.SMR_ERR_INVALID
    lib.smr_shader_program_destroy(h)


def test_the_fixtures_use_no_scratch_and_the_clip_ones_the_lds_their_n_needs():
    """0 scratch bytes is a condition; the quad exchanges use no LDS: none without the clip stage, with it the table's 64 vertices of 6 + N
    words and 32 records (V's formula; 5 632 B without varyings).  The registers are printed (DESIGN.md section 3e quotes them), not asserted."""
    import __graft_entry__ as ge
    ge.build()
    from smelter_amd import hip
    from tools import kernel_resources as kr
    print()
    for name, src in SD.ALL.items():
        p = hip.ShaderProgram(src)
        r = kr.code_object_resources(p.code)["smr_user_shader_kernel"]
        p.close()
        print(f"{name:24} VGPR {r['vgpr']:3} SGPR {r['sgpr']:3} LDS {r['lds']:5} scratch {r['scratch']}")
        assert r["scratch"] == 0, f"{name}: {r['scratch']} scratch bytes per lane"
        n = re.search(r"#define SMR_VARYINGS (\d+)", src)
        if n:
            lds = 64 * (6 + int(n.group(1))) * 4 + 32 * 16 * ((29 + 3 * int(n.group(1)) + 3) // 4)
        else:
            lds = 5632 if "SMR_HAS_VERTEX_CLIP" in src else 0
        assert r["lds"] == lds, (name, r["lds"], lds)


@pytest.mark.parametrize("guard", [1, 2])
def test_on_guard_paged_buffers_no_access_falls_outside(guard):
    """Run in a child process per guard mode: a load or store that leaves its surface — a helper's outside an odd target, say — is a
    segmentation fault there, not here."""
    if not os.path.exists(emu_build.CLANG):
        pytest.skip("no clang++ to build the emulator with")
    env = dict(os.environ, SMR_EMU_USER_SHADER_GUARD=str(guard))
    r = subprocess.run([sys.executable, "-m", "tests.test_emu_user_shader_derivatives"], capture_output=True, text=True, env=env, cwd=ROOT, timeout=600)
    assert r.returncode == 0, f"guard mode {guard}: rc {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    assert "no access fell outside" in r.stdout, r.stdout[-2000:]


def test_the_example_carries_the_disc_shader():
    """examples/user_shader.c's fifth shader is SD.DISC, the text the renderer case runs"""
    text = open(os.path.join(ROOT, "examples", "user_shader.c")).read()
    body = text[text.index("static const char *DISC ="):]
    body = body[:body.index('";') + 1]
    got = "".join(re.findall(r'^\s*"(.*)"$', body, flags=re.M)).replace("\\n", "\n")
    assert got.strip() == SD.DISC.strip()


# ---- what the child processes run (python -m tests.test_emu_user_shader_derivatives, SMR_EMU_USER_SHADER_GUARD = the guard mode): cases 1, 2, 6
def inner(guard):
    for srgb in (False, True):
        for flavour, suffix in SD.FLAVOURS.items():
            for size in SIZES_1:
                check_position(run(emu(f"position_{flavour}", guard), [], *size, srgb=srgb), suffix, size, srgb)
            for which in EDGE_PLANES:
                check_edge(run(emu(f"edge_{flavour}", guard), sources()[:1], 64, 8, pack([EDGE_PLANES[which][0]]), srgb=srgb), suffix, which, srgb)
        for case, (planes, tex, size) in PERSPECTIVE_CASES.items():
            check(run(emu("perspective", guard), tex(), *size, V.pack_planes(planes), srgb=srgb), perspective_model(case, srgb), case)


if __name__ == "__main__":
    inner(int(os.environ["SMR_EMU_USER_SHADER_GUARD"]))
    print("no access fell outside")
