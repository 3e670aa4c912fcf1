"""Varyings of user shaders (SMR_VARYINGS beside SMR_HAS_VERTEX_CLIP: up to eight f32 per vertex, each interpolated perspective-correct,
linear in screen space or flat, and the whole @builtin(position)) on the lane emulator: smr_user_shader_prelude.h compiled for the CPU by
tests/emu/emu_user_shader_clip.cpp with a fixture of tests/user_shader_sources_varyings.py in the user's place.  The expected pictures come
from the numpy model below: the geometry of tests/test_emu_user_shader_clip.py's model (held equal to it by a test here) with the three
interpolation rules of include/smr.h in f64 — never from the code under test.  The plane sets, sizes, caps and the comparison are that
file's.  tests/test_gpu_user_shader_varyings.py holds the compiled programs to the same model."""
import ctypes as C
import math
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

from tests import emu_build
from tests import test_emu_user_shader_clip as M
from tests import user_shader_sources_varyings as SV
from tests.test_emu_user_shader_clip import BEHIND, DEPTH, DEPTH_FREE, FLIP, GRID, IDENTITY, SPAN, TIE, H, W, f32, grid_sources
from tests.test_emu_user_shader_affine import CAP, EDGE, TEXEL, compare, decode, encode, run, sources
from tests.test_gpu_shaders import _textures

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
P8 = C.POINTER(C.c_uint8)
PI = C.POINTER(C.c_int)


# ------------------------------------------------------------------------------------------------------------------ the model
def word(v):
    """the 32-bit word of a vertex value: an int is the word itself, a float its f32"""
    return v if isinstance(v, int) else struct.unpack("<I", struct.pack("<f", v))[0]


def value(v):
    return struct.unpack("<f", struct.pack("<I", v))[0] if isinstance(v, int) else float(v)


def model(planes, modes, textures, Wt, Ht, srgb, fragment, first=0):
    """-> (RGBA8 picture, doubt mask, smallest texel-boundary distance, per plane the number of blends of each pixel, per plane and triangle
    the coverage).  `planes`: four vertices [x, y, z, w, u, v, t_0 .. t_N-1] each (a flat t may be an int: the word); `modes`: one of "P"
    (perspective), "L" (linear), "F" (flat) per varying.  Coverage, depth clip, uv, blend and the doubt rule are those of M.model, line for
    line.  With E_i the edge functions: S = sum E_i, Wn = sum E_i w_i; a perspective varying is sum E_i t_i / S, a linear one
    sum E_i (t_i w_i) / Wn, a flat one the word of the triangle's first vertex; position.z = sum E_i z_i / Wn, position.w = S / Wn.
    `fragment(plane_id, u, v, z_over_w, one_over_w, values, words, dec)` -> (premultiplied colours, texel margins)."""
    dec = [None if t is None else decode(t, srgb) for t in textures]
    out = np.zeros((Ht, Wt, 4), np.uint8)
    doubt = np.zeros((Ht, Wt), bool)
    margin = np.inf
    counts, tri_cover = [], []
    ys, xs = np.mgrid[0:Ht, 0:Wt]
    X = (xs + 0.5) / Wt * 2.0 - 1.0
    Y = 1.0 - (ys + 0.5) / Ht * 2.0
    N = len(modes)
    for n, verts in enumerate(planes):
        count = np.zeros((Ht, Wt), int)
        counts.append(count)
        tri_cover.append([np.zeros((Ht, Wt), bool), np.zeros((Ht, Wt), bool)])
        assert all(len(v) == 6 + N for v in verts)
        vs = np.array([[value(c) for c in v] for v in verts], np.float64)
        ws = np.array([[word(c) for c in v[6:]] for v in verts], np.uint32).reshape(4, N)
        smooth = [6 + j for j in range(N) if modes[j] != "F"]
        with np.errstate(all="ignore"):
            for ti, tri in enumerate(M.TRIANGLES):
                p = [np.array([vs[k, 0], vs[k, 1], vs[k, 3]]) for k in tri]
                coef = [np.cross(p[(i + 1) % 3], p[(i + 2) % 3]) for i in range(3)]
                D = float(np.dot(p[0], coef[0]))
                if not math.isfinite(D) or not D > 0.0 or not math.isfinite(f32(D)):
                    continue
                attrs = vs[list(tri)]
                if not np.isfinite(attrs[:, :6]).all() or not np.isfinite(attrs[:, smooth]).all():  # (a flat varying is data: any word)
                    continue
                E = [c[0] * X + c[1] * Y + c[2] for c in coef]
                mag = [abs(c[0] * X) + abs(c[1] * Y) + abs(c[2]) for c in coef]
                incl = [c[0] > 0.0 or (c[0] == 0.0 and c[1] < 0.0) for c in coef]
                z, q, w = attrs[:, 2], attrs[:, 3] - attrs[:, 2], attrs[:, 3]
                E += [sum(E[i] * z[i] for i in range(3)), sum(E[i] * q[i] for i in range(3))]
                mag += [sum(np.abs(E[i] * z[i]) for i in range(3)), sum(np.abs(E[i] * q[i]) for i in range(3))]
                incl += [True, True]
                cover = np.ones((Ht, Wt), bool)
                near = np.zeros((Ht, Wt), bool)
                outside = np.zeros((Ht, Wt), bool)
                for e, m, inc in zip(E, mag, incl):
                    cover &= (e > 0.0) | ((e == 0.0) & inc)
                    near |= np.abs(e) < EDGE * m
                    outside |= e < -EDGE * m
                doubt |= near & ~outside
                count += cover
                tri_cover[n][ti] = cover
                S = E[0] + E[1] + E[2]
                Wn = sum(E[i] * w[i] for i in range(3))
                u = (sum(E[i] * attrs[i, 4] for i in range(3)) / S)[cover]
                v = (sum(E[i] * attrs[i, 5] for i in range(3)) / S)[cover]
                values = np.zeros((int(cover.sum()), N))
                for j in range(N):
                    t = attrs[:, 6 + j]
                    if modes[j] == "P":
                        values[:, j] = (sum(E[i] * t[i] for i in range(3)) / S)[cover]
                    elif modes[j] == "L":
                        values[:, j] = (sum(E[i] * (t[i] * w[i]) for i in range(3)) / Wn)[cover]
                    else:
                        values[:, j] = t[0]  # the provoking vertex: the triangle's first
                words = np.broadcast_to(ws[tri[0]], (values.shape[0], N))
                f, mg = fragment(first + n, u, v, (E[3] / Wn)[cover], (S / Wn)[cover], values, words, dec)
                if mg.size:
                    margin = min(margin, float(mg[~doubt[cover]].min(initial=np.inf)))
                acc = decode(out[cover], srgb)
                out[cover] = encode(f + acc * (1.0 - f[:, 3:4]), srgb)
    return out, doubt, margin, counts, tri_cover


def check(got, m, what):
    compare(got, m[0], m[1], m[2], what)


def _no_margin(u):
    return np.full(u.shape, np.inf)


def encode_fragment(plane, u, v, zw, ow, values, words, dec):
    """SV._ENCODE_FRAGMENT"""
    pick = np.where(words[:, 4] & 1, 0.75, 0.5)
    return np.stack([0.5 * values[:, 0] * values[:, 3], 0.5 * values[:, 1] * pick, 0.5 * values[:, 2], np.full(u.shape, 0.5)], axis=-1), _no_margin(u)


def position_fragment(plane, u, v, zw, ow, values, words, dec):
    """SV.VARY_POSITION's"""
    return np.stack([zw, ow * SV.POSITION_K, values[:, 0], np.ones(u.shape)], axis=-1), _no_margin(u)


def flat_bits_fragment(plane, u, v, zw, ow, values, words, dec):
    """SV.VARY_FLAT_BITS's"""
    f = np.tile(np.array(SV.WRONG), (u.size, 1))
    f[words[:, 0] == SV.WORD_NAN] = SV.RED
    f[words[:, 0] == SV.WORD_DENORMAL] = SV.GREEN
    return f, _no_margin(u)


def nearest_fragment(plane, u, v, zw, ow, values, words, dec):
    """SV.VARY_UNUSED's: CLIP_PARAM's"""
    return M.nearest_fragment(plane, u, v, dec)


LIGHT = (f32(-0.48), f32(0.6), f32(-0.64))


def lit_fragment(plane, u, v, zw, ow, values, words, dec):
    """SV.LIT's, for its last source (the tests give it no other)"""
    texel, mg = M.nearest_fragment(plane, u, v, dec)
    n = values[:, :3]
    diffuse = np.maximum((n * np.array(LIGHT)).sum(axis=-1) / np.sqrt((n * n).sum(axis=-1)), 0.0)
    k = (0.25 + 0.75 * diffuse) * values[:, 3]
    return np.concatenate([texel[:, :3] * k[:, None], texel[:, 3:4]], axis=-1), mg


def lit_planes(t, n_src, sizes, Wt, Ht):
    """smr_vertex_clip of SV.LIT in f64: M.flip_planes with the turned normal and the tint of each vertex"""
    planes = M.flip_planes(t, n_src, sizes, Wt, Ht)
    c, s = math.cos(t), math.sin(t)
    out = [[list(vtx) + [0.0, 0.0, -1.0, 1.0] for vtx in p] for p in planes[:-1]]
    card = []
    for k, (vtx, ((px, py), _)) in enumerate(zip(planes[-1], M.CORNERS)):
        nx, ny, nz = 0.5 * px, 0.25 * py, -1.0
        card.append(list(vtx) + [f32(nx * c - nz * s), f32(ny), f32(nx * s + nz * c), 1.0 if k == 0 else 0.875])
    return out + [card]


LIT_MODES = "PPPF"


# ---- the varyings the cases give the plane sets of tests/test_emu_user_shader_clip.py
def _lsb(x, bit):
    """the f32 nearest x with the lowest bit of its word set to `bit`"""
    return value((word(f32(x)) & ~1) | bit)


def smooth_values(n_planes, N, seed):
    """[plane][vertex][varying]: non-dyadic f32 in 0.1 .. 0.95.  Varying 4 (where there is one) selects by its word's lowest bit: set at
    vertex 0 and clear at vertex 2, the two provoking vertices, so both constants show"""
    rng = np.random.default_rng(seed)
    vals = [[[f32(x) for x in rng.uniform(0.1, 0.95, N)] for _ in range(4)] for _ in range(n_planes)]
    if N > 4:
        for p in vals:
            p[0][4], p[2][4] = _lsb(p[0][4], 1), _lsb(p[2][4], 0)
    return vals


def with_varyings(planes, vals):
    return [[list(vtx) + list(vals[n][k]) for k, vtx in enumerate(p)] for n, p in enumerate(planes)]


def pack_planes(planes):
    return b"".join(struct.pack("<I", word(c)) for p in planes for vtx in p for c in vtx)


FLIP_V = with_varyings(FLIP, smooth_values(2, 5, 5))
SPAN_V = with_varyings(SPAN, smooth_values(2, 5, 6))
BEHIND_V = with_varyings(BEHIND, smooth_values(1, 5, 7))
# equal at the four vertices (flat ones included: either provoking vertex gives the same word)
IDENTITY_V = with_varyings(IDENTITY, [[[f32(0.3), f32(0.7), f32(0.45), f32(0.6), f32(0.9)]] * 4])
# dyadic: multiples of 1 / 8.  Varying 0 is 1 everywhere, so r = 0.5 * varying 3 exactly; varying 2 is what the linear / perspective pair
# interpolates
TIE_V = with_varyings(TIE, [[[1.0, 0.25, 0.125, 0.75, 0.5], [1.0, 0.875, 0.625, 0.5, 0.5], [1.0, 0.5, 1.0, 0.25, 0.5], [1.0, 0.125, 0.375, 0.5, 0.5]]])


def grid_tables():
    """per plane of GRID the eight f32 of SV.VARY_GRID: varying j of vertex k is word j + k.  Words 4 and 6 are varying 4 at the two provoking
    vertices: lowest bit set and clear"""
    rng = np.random.default_rng(8)
    tabs = [[f32(x) for x in rng.uniform(0.1, 0.95, 8)] for _ in range(16)]
    for t in tabs:
        t[4], t[6] = _lsb(t[4], 1), _lsb(t[6], 0)
    return tabs


GRID_V = with_varyings(GRID, [[[t[j + k] for j in range(5)] for k in range(4)] for t in grid_tables()])


def pack_grid():
    return M.pack_planes(GRID) + b"".join(struct.pack("<8f", *t) for t in grid_tables())


FLIP_BITS = with_varyings(FLIP, [[[SV.WORD_NAN], [SV.WORD_OTHER], [SV.WORD_DENORMAL], [SV.WORD_OTHER]]] * 2)
FLIP_P = with_varyings(FLIP, smooth_values(2, 1, 9))
DEPTH_FREE_P = with_varyings(DEPTH_FREE, smooth_values(1, 1, 10))
DEPTH_P = with_varyings(DEPTH, smooth_values(1, 1, 10))  # (not among the issue's cases: here position.z runs over the depth range)

# (fixture, planes, modes, sources, size, parameter bytes, fragment): what the emulator and the device tests both run, cases 1 - 4
SMOOTH_CASES = {
    "flip": ("vary_param", FLIP_V, SV.VARY_MODES, sources, (W, H), pack_planes(FLIP_V)),
    "flip_65x5": ("vary_param", FLIP_V, SV.VARY_MODES, sources, (65, 5), pack_planes(FLIP_V)),
    "flip_1x1": ("vary_param", FLIP_V, SV.VARY_MODES, sources, (1, 1), pack_planes(FLIP_V)),
    "grid": ("vary_grid", GRID_V, SV.VARY_MODES, grid_sources, (W, H), pack_grid()),
    "span": ("vary_param", SPAN_V, SV.VARY_MODES, sources, (W, H), pack_planes(SPAN_V)),
    "behind": ("vary_persp", BEHIND_V, SV.PERSP_MODES, lambda: sources()[:1], (W, H), pack_planes(BEHIND_V)),
}
POSITION_CASES = {"flip": (FLIP_P, sources), "depth_free": (DEPTH_FREE_P, lambda: sources()[:1]), "depth": (DEPTH_P, lambda: sources()[:1])}
# case 9: (planes of CLIP_PARAM's layout, sources, size)
UNUSED_CASES = {"flip": (FLIP, sources, (W, H)), "behind": (BEHIND, lambda: sources()[:1], (W, H)), "depth": (DEPTH, lambda: sources()[:1], (W, H)),
                "span": (SPAN, sources, (W, H)), "grid": (GRID, grid_sources, (W, H)), "tie": (TIE, lambda: sources()[:1], (64, 8))}
UNUSED_MODES = "PLP"


def unused_planes(planes):
    """what SV.VARY_UNUSED's vertex stage adds to CLIP_PARAM's vertices"""
    return [[list(vtx) + [vtx[4], f32(f32(vtx[5]) + f32(vtx[3])), float(k)] for k, vtx in enumerate(p)] for p in planes]


def test_the_model_is_the_clip_stages_and_its_constants_stay_under_the_cap():
    """What the other tests assume, checked with the models alone: this file's model draws M.model's picture (same coverage, same doubt) for
    every plane set used; every (plane set, size) pair stays under the cap; the case with a vertex behind the eye carries no linear varying."""
    for planes, tex, size in UNUSED_CASES.values():
        for srgb in (True, False):
            mine = model(unused_planes(planes), UNUSED_MODES, tex(), *size, srgb, nearest_fragment)
            theirs = M.model(planes, tex(), *size, srgb)
            assert np.array_equal(mine[0], theirs[0]) and np.array_equal(mine[1], theirs[1]) and mine[2] == theirs[2]
            assert all(np.array_equal(a, b) for a, b in zip(mine[3], theirs[3]))
    for name, (fixture, planes, modes, tex, size, params) in SMOOTH_CASES.items():
        m = model(planes, modes, tex(), *size, True, encode_fragment)
        assert m[1].mean() <= CAP and m[2] > TEXEL, (name, m[1].mean())
        assert len(params) <= 2048 and m[0].any(), name
        picks = {word(p[k][10]) & 1 for p in planes for k in (0, 2)}
        assert picks == {0, 1}, name  # both of the fragment's constants show
    assert "L" not in SMOOTH_CASES["behind"][2] and min(v[3] for v in BEHIND_V[0]) < 0.0
    assert "L" in SV.VARY_MODES and all(v[3] > 0.0 for p in FLIP_V + GRID_V + SPAN_V for v in p)
    for planes, tex in POSITION_CASES.values():
        m = model(planes, "P", tex(), W, H, True, position_fragment)
        assert m[1].mean() <= CAP and all(0.6 < 1.0 / v[3] < 1.7 for p in planes for v in p)
    for planes, size in ((IDENTITY_V, (8, 8)), (TIE_V, (64, 8))):
        m = model(planes, SV.VARY_MODES, sources()[:1], *size, True, encode_fragment)
        assert (np.array(m[3][0]) == 1).sum() == (64 if size == (8, 8) else 32 * 4)
    m = model(FLIP_BITS, "F", sources(), W, H, True, flat_bits_fragment)
    assert not m[1].any() and all(c.any() for p in m[4] for c in p)  # (every triangle of both planes covers something)
    for t in M.PTS:
        m = model(lit_planes(f32(t), 1, [(M.IW, M.IH)], M.OW, M.OH), LIT_MODES, _textures(1, M.IW, M.IH), M.OW, M.OH, True, lit_fragment)
        assert not m[1].any() and m[0].any() == (t < 1.5) and (m[2] > TEXEL or t > 1.5)


# ------------------------------------------------------------------------------------------------------------------ the emulator
def build(name):
    """tests/emu/_build/libsmr_emu_user_vary_<name>.so: the build of tests.test_emu_user_shader_clip.build for a fixture of this file's
    sources — emu_user_shader_clip.cpp takes the fixture through SMR_EMU_USER_SOURCE, unchanged"""
    out_dir = os.path.join(emu_build.EMU, "_build")
    os.makedirs(out_dir, exist_ok=True)
    user = os.path.join(out_dir, f"user_shader_vary_{name}.inc")
    text = "// generated from tests/user_shader_sources_varyings.py\n" + SV.ALL[name]
    if not os.path.exists(user) or open(user).read() != text:
        with open(user, "w") as f:
            f.write(text)
    lib = os.path.join(out_dir, f"libsmr_emu_user_vary_{name}.so")
    deps = [user, os.path.join(emu_build.EMU, "emu_user_shader_clip.cpp"), os.path.join(emu_build.EMU, "emu_device.h"), os.path.join(emu_build.EMU, "emu_guard.h"),
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


def same_coverage(got, m):
    assert np.array_equal(got.any(axis=-1), m[0].any(axis=-1))  # (no pixel is doubtful: coverage is exactly the model's)


@pytest.mark.parametrize("srgb", [True, False])
@pytest.mark.parametrize("case", sorted(SMOOTH_CASES))
def test_interpolated_varyings_match_the_model(case, srgb):
    """cases 1 - 4: two cards in perspective at three sizes, sixteen planes each with its own values (the last record's last word is
    varying 4 of plane 15), planes ending either side of x = 64, a vertex behind the eye (perspective and flat only)"""
    fixture, planes, modes, tex, size, params = SMOOTH_CASES[case]
    got = run(emu(fixture), tex(), *size, params, srgb=srgb)
    m = model(planes, modes, tex(), *size, srgb, encode_fragment)
    check(got, m, case)
    if not m[1].any():
        same_coverage(got, m)


@pytest.mark.parametrize("srgb", [True, False])
def test_equal_varyings_on_the_identity_quad_give_one_colour_drawn_once(srgb):
    got = run(emu("vary_param"), sources()[:1], 8, 8, pack_planes(IDENTITY_V), srgb=srgb)
    want = model(IDENTITY_V, SV.VARY_MODES, sources()[:1], 8, 8, srgb, encode_fragment)[0]
    assert (got == got[0, 0]).all(axis=-1).all(), "the 64 pixels are not all equal"
    assert np.abs(got[0, 0].astype(int) - want[0, 0].astype(int)).max() <= 1 and got[0, 0, 3] == 128, (got[0, 0], want[0, 0])


@pytest.mark.parametrize("srgb", [True, False])
def test_dyadic_varyings_are_exact_and_linear_equals_perspective_where_w_is_one(srgb):
    """every product and sum is exact and Wn == S, so the linear varying 2 of vary_param and the perspective varying 2 of vary_persp are the
    same quotient: byte-equal pictures; r is 0.5 * the flat varying 3 exactly: 0.375 in the first triangle, 0.125 in the second"""
    tex = sources()[:1]
    linear = run(emu("vary_param"), tex, 64, 8, pack_planes(TIE_V), srgb=srgb)
    persp = run(emu("vary_persp"), tex, 64, 8, pack_planes(TIE_V), srgb=srgb)
    assert np.array_equal(linear, persp), f"{(linear != persp).sum()} bytes differ"
    m = model(TIE_V, SV.VARY_MODES, tex, 64, 8, srgb, encode_fragment)
    assert linear.any(axis=-1).sum() == 32 * 4 and np.abs(linear.astype(int) - m[0].astype(int)).max() <= 1
    for cover, r in zip(m[4][0], (0.375, 0.125)):
        assert cover.any() and (linear[cover][:, 0] == encode(np.array([r, 0.0, 0.0, 0.5]), srgb)[0]).all()


def check_flat_bits(got, srgb):
    """case 7: no pixel shows the third colour, each triangle shows its own, as many pixels of each as the model's coverage leaves visible"""
    m = model(FLIP_BITS, "F", sources(), *got.shape[1::-1], srgb, flat_bits_fragment)
    assert not m[1].any()
    colours = {name: encode(np.array(c), srgb) for name, c in (("red", SV.RED), ("green", SV.GREEN), ("wrong", SV.WRONG))}
    seen = {name: (got == c).all(axis=-1) for name, c in colours.items()}
    assert not seen["wrong"].any(), f"{seen['wrong'].sum()} pixels got another word than the provoking vertex's"
    first = (m[4][1][0] | (m[4][0][0] & ~m[4][1][1]))  # the first triangles': the upper plane's, and the lower plane's where the upper is absent
    second = (m[4][1][1] | (m[4][0][1] & ~m[4][1][0]))
    assert first.any() and second.any() and not (first & second).any()
    assert np.array_equal(seen["red"], first) and np.array_equal(seen["green"], second), (seen["red"].sum(), first.sum(), seen["green"].sum(), second.sum())
    assert np.array_equal(got, m[0])


@pytest.mark.parametrize("srgb", [True, False])
def test_a_flat_varying_is_the_provoking_vertex_word_bit_for_bit(srgb):
    check_flat_bits(run(emu("vary_flat_bits"), sources(), W, H, pack_planes(FLIP_BITS), srgb=srgb), srgb)


@pytest.mark.parametrize("srgb", [True, False])
@pytest.mark.parametrize("case", sorted(POSITION_CASES))
def test_position_z_and_w_match_the_model(case, srgb):
    planes, tex = POSITION_CASES[case]
    got = run(emu("vary_position"), tex(), W, H, pack_planes(planes), srgb=srgb)
    check(got, model(planes, "P", tex(), W, H, srgb, position_fragment), f"position {case}")


@pytest.mark.parametrize("srgb", [True, False])
@pytest.mark.parametrize("case", sorted(UNUSED_CASES))
def test_declaring_varyings_changes_neither_coverage_nor_uv(case, srgb):
    planes, tex, size = UNUSED_CASES[case]
    without = run(M.emu("clip_param"), tex(), *size, M.pack_planes(planes), srgb=srgb)
    with_them = run(emu("vary_unused"), tex(), *size, M.pack_planes(planes), srgb=srgb)
    assert without.any() and np.array_equal(without, with_them), f"{(without != with_them).sum()} bytes differ"


@pytest.mark.parametrize("name", sorted(SV.BROKEN))
def test_a_misdeclared_varying_is_a_compile_error(name):
    import __graft_entry__ as ge
    ge.build()
    from smelter_amd import hip
    hip.ShaderProgram(SV.VARY_POSITION).close()  # (a well-formed declaration compiles: the errors below are the declarations')
    src, message = SV.BROKEN[name]
    with pytest.raises(hip.ShaderCompileError) as e:
        hip.ShaderProgram(src)
    assert e.value.code == -1  # SMR_ERR_INVALID
    assert message in e.value.log, e.value.log


def test_the_fixtures_use_no_scratch_and_the_lds_their_n_needs():
    """0 scratch bytes is a condition; LDS is 64 vertices of 6 + N words and 32 records of 29 + 3 N words rounded up to 16 bytes: a shader with
    two varyings does not pay for eight.  The registers are printed (DESIGN.md section 3e quotes them), not asserted."""
    import __graft_entry__ as ge
    ge.build()
    from smelter_amd import hip
    from tools import kernel_resources as kr
    print()
    for name, src in SV.ALL.items():
        p = hip.ShaderProgram(src)
        r = kr.code_object_resources(p.code)["smr_user_shader_kernel"]
        p.close()
        n = int(re.search(r"#define SMR_VARYINGS (\d+)", src).group(1))
        print(f"{name:16} N {n} VGPR {r['vgpr']:3} SGPR {r['sgpr']:3} LDS {r['lds']:5} scratch {r['scratch']}")
        assert r["scratch"] == 0, f"{name}: {r['scratch']} scratch bytes per lane"
        assert r["lds"] == 64 * (6 + n) * 4 + 32 * 16 * ((29 + 3 * n + 3) // 4) < 12 * 1024, (name, r["lds"])


@pytest.mark.parametrize("guard", [1, 2])
def test_on_guard_paged_buffers_no_access_falls_outside(guard):
    """Run in a child process per guard mode: a load or store that leaves its surface is a segmentation fault there, not here."""
    if not os.path.exists(emu_build.CLANG):
        pytest.skip("no clang++ to build the emulator with")
    env = dict(os.environ, SMR_EMU_USER_SHADER_GUARD=str(guard))
    r = subprocess.run([sys.executable, "-m", "tests.test_emu_user_shader_varyings"], capture_output=True, text=True, env=env, cwd=ROOT, timeout=600)
    assert r.returncode == 0, f"guard mode {guard}: rc {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    assert "no access fell outside" in r.stdout, r.stdout[-2000:]


@pytest.mark.parametrize("t", M.PTS)
def test_the_lit_card_matches_the_model(t):
    """the renderer case's shader without the renderer"""
    tex = _textures(1, M.IW, M.IH)
    got = run(emu("lit"), tex, M.OW, M.OH, time_s=t)
    m = model(lit_planes(f32(t), 1, [(M.IW, M.IH)], M.OW, M.OH), LIT_MODES, tex, M.OW, M.OH, True, lit_fragment)
    compare(got, m[0], m[1], m[2] if t < 1.5 else 1.0, f"lit t={t}")
    same_coverage(got, m)
    assert got.any() == (t < 1.5)
    if t < 1.5:  # (the light does something: the picture is not the unlit card's)
        assert not np.array_equal(got, run(M.emu("flip"), tex, M.OW, M.OH, time_s=t))


def test_the_example_carries_the_lit_card():
    """examples/user_shader.c's fourth shader is SV.LIT, the text the renderer case runs"""
    text = open(os.path.join(ROOT, "examples", "user_shader.c")).read()
    body = text[text.index("static const char *LIT ="):]
    body = body[:body.index('";') + 1]
    got = "".join(re.findall(r'^\s*"(.*)"$', body, flags=re.M)).replace("\\n", "\n")
    assert got.strip() == SV.LIT.strip()


# ---- what the child processes run (python -m tests.test_emu_user_shader_varyings, SMR_EMU_USER_SHADER_GUARD = the guard mode)
def inner(guard):
    for srgb in (False, True):
        for case in ("flip", "flip_65x5", "flip_1x1", "grid"):
            fixture, planes, modes, tex, size, params = SMOOTH_CASES[case]
            check(run(emu(fixture, guard), tex(), *size, params, srgb=srgb), model(planes, modes, tex(), *size, srgb, encode_fragment), case)


if __name__ == "__main__":
    inner(int(os.environ["SMR_EMU_USER_SHADER_GUARD"]))
    print("no access fell outside")
