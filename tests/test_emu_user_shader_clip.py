"""The clip vertex stage of user shaders (SMR_HAS_VERTEX_CLIP: a homogeneous clip position and tex_coords per vertex of the quad, drawn as two
triangles) on the lane emulator: smr_user_shader_prelude.h compiled for the CPU by tests/emu/emu_user_shader_clip.cpp — one host thread per
lane, a real barrier, LDS as statics — with a fixture of tests/user_shader_sources_clip.py in the user's place.  The expected pictures come
from the numpy model below, the coverage contract of include/smr.h in f64 — never from the code under test; decode, encode, the nearest-texel
fragment and the comparison are those of tests/test_emu_user_shader_affine.py.  tests/test_gpu_user_shader_clip.py holds the compiled
programs to the same model."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import emu_build
from tests import user_shader_sources_clip as SC
from tests.test_emu_user_shader_affine import CAP, EDGE, TEXEL, compare, decode, encode, nearest_fragment, pack, run, sources
from tests.test_gpu_shaders import _textures

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
P8 = C.POINTER(C.c_uint8)
PI = C.POINTER(C.c_int)

W, H = 70, 9  # the target: a multiple of neither 64 nor 4 (the sources are 5 x 3: sources())
# plane.rs:11-28: position.xy and tex_coords of the quad's four vertices; triangles (0, 1, 2) and (2, 3, 0)
CORNERS = [((1.0, -1.0), (1.0, 1.0)), ((1.0, 1.0), (1.0, 0.0)), ((-1.0, 1.0), (0.0, 0.0)), ((-1.0, -1.0), (0.0, 1.0))]
TRIANGLES = [(0, 1, 2), (2, 3, 0)]
NAN = float("nan")


# ------------------------------------------------------------------------------------------------------------------ the model
def f32(v):
    return float(np.float32(v))


def card(deg, d, sx, sy, cx, cy, z=(0.5, 0.0), mirror=False, radians=None):
    """a sx x sy card turned by `deg` degrees about its vertical axis, seen from distance d, then moved to (cx, cy): four vertices
    [x, y, z, w, u, v], the position as the f32 the shader reads.  z = z[0] * w + z[1] * zr (0.5 w: the middle of the depth range)"""
    th = math.radians(deg) if radians is None else radians
    out = []
    for (px, py), (u, v) in CORNERS:
        if mirror:
            px = -px
        xr, zr = px * sx * math.cos(th), px * sx * math.sin(th)
        w = 1.0 + zr / d
        out.append([f32(xr + cx * w), f32(py * sy + cy * w), f32(z[0] * w + z[1] * zr), f32(w), u, v])
    return out


def constant_fragment(plane, u, v, dec):
    """SC.CLIP_HALF's fragment"""
    return np.broadcast_to(np.array([0.25, 0.5, 0.125, 0.5]), (u.size, 4)), np.full(u.shape, np.inf)


def model(planes, textures, Wt, Ht, srgb, fragment=nearest_fragment, first=0):
    """-> (RGBA8 picture, mask of pixels an edge or a depth bound passes too close to, smallest texel-boundary distance of a compared pixel,
    per plane the number of times each pixel was blended).  `planes`: four vertices [x, y, z, w, u, v] each; plane i has plane_id first + i.
    The contract of include/smr.h in f64: per triangle (i, j, k), (a, b, c)_i = p_j x p_k with p = (x, y, w); D = p_i . (a, b, c)_i; drawn
    if D > 0 and finite; E_i = a_i X + b_i Y + c_i; covered if every E_i > 0, or == 0 on an inclusive edge (a > 0, or a == 0 and b < 0);
    kept if sum E_i z_i >= 0 and sum E_i (w_i - z_i) >= 0; uv = sum E_i t_i / sum E_i; premultiplied OVER per triangle in index order,
    stored to the RGBA8 target and read back before the next."""
    dec = [None if t is None else decode(t, srgb) for t in textures]
    out = np.zeros((Ht, Wt, 4), np.uint8)
    doubt = np.zeros((Ht, Wt), bool)
    margin = np.inf
    counts = []
    ys, xs = np.mgrid[0:Ht, 0:Wt]
    X = (xs + 0.5) / Wt * 2.0 - 1.0
    Y = 1.0 - (ys + 0.5) / Ht * 2.0
    for n, verts in enumerate(planes):
        count = np.zeros((Ht, Wt), int)
        counts.append(count)
        vs = np.array(verts, np.float64)
        with np.errstate(all="ignore"):
            for tri in TRIANGLES:
                p = [np.array([vs[k, 0], vs[k, 1], vs[k, 3]]) for k in tri]
                coef = [np.cross(p[(i + 1) % 3], p[(i + 2) % 3]) for i in range(3)]
                D = float(np.dot(p[0], coef[0]))
                if not math.isfinite(D) or not D > 0.0 or not math.isfinite(f32(D)):
                    continue
                attrs = vs[list(tri)]
                if not np.isfinite(attrs).all():  # (a NaN or an infinity in z, u or v: nothing is drawn either)
                    continue
                E = [c[0] * X + c[1] * Y + c[2] for c in coef]
                mag = [abs(c[0] * X) + abs(c[1] * Y) + abs(c[2]) for c in coef]
                incl = [c[0] > 0.0 or (c[0] == 0.0 and c[1] < 0.0) for c in coef]
                z, q = attrs[:, 2], attrs[:, 3] - attrs[:, 2]
                # the two depth sums, held to the same rule as the edges (they have no inclusive side to lose: >= 0 keeps the pixel)
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
                S = E[0] + E[1] + E[2]
                u = (sum(E[i] * attrs[i, 4] for i in range(3)) / S)[cover]
                v = (sum(E[i] * attrs[i, 5] for i in range(3)) / S)[cover]
                f, mg = fragment(first + n, u, v, dec)
                if mg.size:
                    margin = min(margin, float(mg[~doubt[cover]].min(initial=np.inf)))
                acc = decode(out[cover], srgb)
                out[cover] = encode(f + acc * (1.0 - f[:, 3:4]), srgb)
    return out, doubt, margin, counts


def check(got, m, what):
    compare(got, m[0], m[1], m[2], what)


# case 1: two cards in perspective, the second over the first
FLIP = [card(37, 2.5, 0.8, 0.7, -0.1, 0.05), card(-55, 2.0, 0.6, 0.8, 0.3, -0.1)]
# case 2: a card whose right side passes behind the eye (its vertices' w: 2.299 and -0.299)
BEHIND = [card(60, 0.6, 0.9, 0.8, 0.0, 0.0)]
# case 3: the far side leaves the depth range (z > w there); the same card within it
DEPTH = [card(40, 2.5, 0.8, 0.7, 0.0, 0.0, z=(0.5, 2.0))]
DEPTH_FREE = [card(40, 2.5, 0.8, 0.7, 0.0, 0.0)]


def _with(plane, vertex, component, value):
    out = [list(v) for v in plane]
    out[vertex][component] = value
    return out


# case 4: planes that draw nothing
NOTHING = {
    "back_facing": card(120, 2.5, 0.8, 0.7, 0.0, 0.0),
    "edge_on": card(90, 2.5, 0.8, 0.7, 0.0, 0.0),  # (cos 90 degrees is 6e-17 in f64: a sliver no centre lies in)
    "edge_on_exact": [[0.0, py * 0.7, 0.5, 1.0 + px * 0.32, u, v] for (px, py), (u, v) in CORNERS],  # (the same with an exact zero: D == 0)
    "mirrored": card(37, 2.5, 0.8, 0.7, -0.1, 0.05, mirror=True),
    "w_zero": [[px * 0.5, py * 0.5, 0.0, 0.0, u, v] for (px, py), (u, v) in CORNERS],
    "w_negative": [[px * 0.5, py * 0.5, -0.5, -1.0, u, v] for (px, py), (u, v) in CORNERS],
    "nan_x": _with(FLIP[0], 0, 0, NAN),
    "nan_y": _with(FLIP[0], 2, 1, NAN),
    "nan_z": _with(FLIP[0], 0, 2, NAN),  # (vertices 0 and 2 are in both triangles; a NaN in z, u or v of vertex 1 or 3 leaves the other one)
    "nan_w": _with(FLIP[0], 2, 3, NAN),
    "nan_u": _with(FLIP[0], 0, 4, NAN),
    "nan_v": _with(FLIP[0], 2, 5, NAN),
    "inf_x": _with(FLIP[0], 0, 0, float("inf")),
    "inf_w": _with(FLIP[0], 2, 3, float("inf")),
}
# case 5 (a): 64 x 8, the left and top edges exactly through pixel centres — the smr_plane {0.5, 0.5, 0.015625, -0.125}
TIE = [[[0.5 * px + 0.015625, 0.5 * py - 0.125, 0.0, 1.0, u, v] for (px, py), (u, v) in CORNERS]]
TIE_PLANE = [0.5, 0.5, 0.015625, -0.125]
# case 5 (b): 8 x 8, the identity quad: the diagonal passes through eight centres
IDENTITY = [[[px, py, 0.0, 1.0, u, v] for (px, py), (u, v) in CORNERS]]
# case 6: planes that end one pixel either side of x = 64, where the spans of two waves (and two workgroups) meet
SPAN = [card(34, 2.5, 0.35, 0.22, 0.59, 0.22), card(-25, 2.5, 0.12, 0.21, 0.9, -0.23)]
# case 7: all sixteen planes
GRID = [card(25 if i % 2 else -25, 2.5, 0.1, 0.4, -0.875 + 0.25 * (i % 8), 0.5 - (i // 8)) for i in range(16)]

# the renderer case of tests/test_gpu_user_shader_clip.py: the card shader over one 16 x 8 input stream, a 32 x 16 target
IW, IH, OW, OH = 16, 8, 32, 16
PTS = [0.0, 0.9, 2.0]


def flip_planes(t, n_src, sizes, Wt, Ht):
    """smr_vertex_clip of SC.FLIP in f64: the last source a card turned by t radians, every source before it over the whole target"""
    w, h = sizes[-1]
    fit = min(Wt / w, Ht / h) * f32(0.6)
    return [IDENTITY[0]] * (n_src - 1) + [card(0.0, 2.5, fit * w / Wt, fit * h / Ht, 0.0, 0.0, radians=t)]


def grid_sources():
    """sixteen 2 x 2 sources of distinct texels"""
    return _textures(16, 2, 2, seed=23)


def covered(counts):
    return [int((c > 0).sum()) for c in counts]


def test_the_models_constants_stay_under_the_cap():
    """What the other tests assume about the constants above, checked with the model alone."""
    for srgb in (True, False):
        want, doubt, margin, counts = model(FLIP, sources(), W, H, srgb)
        assert covered(counts) == [300, 188] and int(((counts[0] > 0) & (counts[1] > 0)).sum()) == 72, covered(counts)
        assert not doubt.any() and 1.2e-3 < margin < 1.4e-3, (doubt.mean(), margin)
        assert max(c.max() for c in counts) == 1  # (no pixel in both triangles of a plane)
        first = model(FLIP[:1], sources()[:1], W, H, srgb)[0]
        both = (counts[0] > 0) & (counts[1] > 0)
        assert (want[both] != first[both]).any(axis=-1).sum() >= 10  # the second plane shows over the first
    _, doubt, _, counts = model(FLIP, sources(), 65, 5, True)
    assert covered(counts) == [149, 101] and not doubt.any()
    _, doubt, _, counts = model(FLIP, sources(), 1, 1, True)
    assert covered(counts) == [1, 0] and not doubt.any()

    want, doubt, margin, counts = model(BEHIND, sources()[:1], W, H, True)
    assert [f"{v[3]:.3f}" for v in BEHIND[0]] == ["2.299", "2.299", "-0.299", "-0.299"]
    assert covered(counts) == [348] and doubt.sum() == 1 and 9.0e-5 < margin < 1.0e-4, (covered(counts), doubt.sum(), margin)
    assert (counts[0] > 0)[:, 41].any() and not (counts[0] > 0)[:, 42:].any() and (counts[0] > 0)[:, 0].any()

    clipped, free = model(DEPTH, sources()[:1], W, H, True), model(DEPTH_FREE, sources()[:1], W, H, True)
    assert round(float((clipped[3][0] > 0).mean()), 3) == 0.206 and round(float((free[3][0] > 0).mean()), 3) == 0.459
    assert doubt_ok(clipped) and doubt_ok(free)
    assert not ((clipped[3][0] > 0) & ~(free[3][0] > 0)).any()  # (the clip only takes pixels away)

    for name, plane in NOTHING.items():
        assert not model([plane], sources()[:1], W, H, True)[0].any(), name
    # (and the card the NaN cases spoil does draw)
    assert model([FLIP[0]], sources()[:1], W, H, True)[0].any()

    want, doubt, margin, counts = model(TIE, sources()[:1], 64, 8, True)
    assert counts[0].max() == 1 and np.array_equal(np.argwhere(counts[0] > 0).min(axis=0), [2, 16]) and np.array_equal(np.argwhere(counts[0] > 0).max(axis=0), [5, 47])
    assert int((counts[0] > 0).sum()) == 32 * 4
    _, _, _, counts = model(IDENTITY, [], 8, 8, True, fragment=constant_fragment, first=-1)
    assert (counts[0] == 1).all()  # multiplicity exactly 1 everywhere, the eight centres on the diagonal included

    want, doubt, margin, counts = model(SPAN, sources(), W, H, True)
    a, b = counts[0] > 0, counts[1] > 0
    assert not doubt.any() and margin > TEXEL
    assert a.sum() == 39 and a[:, 45].any() and not a[:, :45].any() and a[:, 64].sum() == 1 and not a[:, 65:].any()
    assert b.sum() == 7 and b[:, 63].sum() == 1 and not b[:, :63].any() and b[:, 69].any()

    want, doubt, margin, counts = model(GRID, grid_sources(), W, H, True)
    assert not doubt.any() and 1.2e-2 < margin < 1.4e-2, (doubt.sum(), margin)
    assert all(c in (24, 28) for c in covered(counts)), covered(counts)

    for t, cov, mg in ((0.0, 0.391, 0.083), (0.9, 0.230, 0.011), (2.0, 0.0, None)):
        picture, doubt, margin, counts = model(flip_planes(f32(t), 1, [(IW, IH)], OW, OH), _textures(1, IW, IH), OW, OH, True)
        assert not doubt.any() and round(float((counts[0] > 0).mean()), 3) == cov, (t, doubt.sum(), (counts[0] > 0).mean())
        if mg is not None:
            assert abs(margin - mg) < 0.05 * mg, (t, margin)


def doubt_ok(m):
    return m[1].mean() <= CAP and m[2] > TEXEL


# ------------------------------------------------------------------------------------------------------------------ the emulator
def build(name):
    """tests/emu/_build/libsmr_emu_user_clip_<name>.so: emu_user_shader_clip.cpp (one host thread per lane) with the fixture as the user's
    translation unit; plane_param, which has no clip stage, runs through the same file: its kernel meets no barrier"""
    out_dir = os.path.join(emu_build.EMU, "_build")
    os.makedirs(out_dir, exist_ok=True)
    user = os.path.join(out_dir, f"user_shader_clip_{name}.inc")
    text = "// generated from tests/user_shader_sources_clip.py\n" + SC.ALL[name]
    if not os.path.exists(user) or open(user).read() != text:
        with open(user, "w") as f:
            f.write(text)
    lib = os.path.join(out_dir, f"libsmr_emu_user_clip_{name}.so")
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


def pack_planes(planes):
    return pack([v for plane in planes for v in plane])


@pytest.mark.parametrize("srgb", [True, False])
@pytest.mark.parametrize("size", [(W, H), (65, 5), (1, 1)])
def test_overlapping_planes_in_perspective_match_the_model(srgb, size):
    got = run(emu("clip_param"), sources(), *size, pack_planes(FLIP), srgb=srgb)
    m = model(FLIP, sources(), *size, srgb)
    check(got, m, f"flip {size}")
    assert np.array_equal(got.any(axis=-1), m[0].any(axis=-1))  # (no pixel is doubtful: coverage is exactly the model's)


@pytest.mark.parametrize("srgb", [True, False])
def test_a_plane_that_passes_behind_the_eye_matches_the_model(srgb):
    """two vertices have w < 0: homogeneous edge functions draw exactly the part in front of the eye, without a clipping step"""
    got = run(emu("clip_param"), sources()[:1], W, H, pack_planes(BEHIND), srgb=srgb)
    check(got, model(BEHIND, sources()[:1], W, H, srgb), "behind the eye")
    assert got[:, :42].any() and not got[:, 42:].any()


@pytest.mark.parametrize("srgb", [True, False])
def test_the_depth_range_clips_per_pixel(srgb):
    tex = sources()[:1]
    clipped, free = run(emu("clip_param"), tex, W, H, pack_planes(DEPTH), srgb=srgb), run(emu("clip_param"), tex, W, H, pack_planes(DEPTH_FREE), srgb=srgb)
    mc, mf = model(DEPTH, tex, W, H, srgb), model(DEPTH_FREE, tex, W, H, srgb)
    check(clipped, mc, "depth clipped")
    check(free, mf, "within the depth range")
    sure = ~(mc[1] | mf[1])
    assert np.array_equal((clipped != free).any(axis=-1)[sure], (mc[0] != mf[0]).any(axis=-1)[sure]) and (mc[0] != mf[0]).any()


@pytest.mark.parametrize("name", sorted(NOTHING))
def test_back_facing_degenerate_and_nan_planes_cover_nothing(name):
    got = run(emu("clip_param"), sources()[:1], W, H, pack_planes([NOTHING[name]]))
    assert not got.any(), f"{name}: {np.count_nonzero(got.any(axis=-1))} pixels drawn"


@pytest.mark.parametrize("srgb", [True, False])
def test_edges_through_pixel_centres_follow_the_top_left_rule_byte_for_byte(srgb):
    """dyadic vertices: every product and sum of the rasteriser is exact, so the picture IS the smr_plane one"""
    tex = sources()[:1]
    as_plane = run(emu("plane_param"), tex, 64, 8, pack([TIE_PLANE]), srgb=srgb)
    as_clip = run(emu("clip_param"), tex, 64, 8, pack_planes(TIE), srgb=srgb)
    cover = as_plane.any(axis=-1)
    assert cover[2:6, 16:48].all() and cover.sum() == 32 * 4
    assert np.array_equal(as_plane, as_clip), f"{(as_plane != as_clip).sum()} bytes differ"
    # (every centre on the left and top edges is "doubtful" to the model's rule; the arithmetic is exact here, so all are compared)
    want = model(TIE, tex, 64, 8, srgb)[0]
    assert np.abs(as_clip.astype(int) - want.astype(int)).max() <= 1


@pytest.mark.parametrize("srgb", [True, False])
def test_the_shared_diagonal_is_drawn_once(srgb):
    """the identity quad on 8 x 8: eight centres lie on the diagonal; each belongs to exactly one triangle — no crack, no double blend"""
    got = run(emu("clip_half"), [], 8, 8, pack_planes(IDENTITY), srgb=srgb)
    want = model(IDENTITY, [], 8, 8, srgb, fragment=constant_fragment, first=-1)[0]
    assert (got == got[0, 0]).all(axis=-1).all(), "the 64 pixels are not all equal"
    assert np.abs(got[0, 0].astype(int) - want[0, 0].astype(int)).max() <= 1 and got[0, 0, 3] == 128, (got[0, 0], want[0, 0])


@pytest.mark.parametrize("srgb", [True, False])
def test_planes_that_end_a_pixel_past_a_wave_span_boundary_match_the_model(srgb):
    """the wave early-out must not drop a triangle for a span that holds one pixel of it"""
    got = run(emu("clip_param"), sources(), W, H, pack_planes(SPAN), srgb=srgb)
    m = model(SPAN, sources(), W, H, srgb)
    check(got, m, "span")
    assert np.array_equal(got.any(axis=-1), m[0].any(axis=-1))


@pytest.mark.parametrize("srgb", [True, False])
def test_sixteen_planes_each_from_its_own_slot_of_the_table(srgb):
    tex = grid_sources()
    got = run(emu("clip_param"), tex, W, H, pack_planes(GRID), srgb=srgb)
    m = model(GRID, tex, W, H, srgb)
    check(got, m, "grid")
    assert np.array_equal(got.any(axis=-1), m[0].any(axis=-1))


def test_no_sources_is_one_plane_with_plane_id_minus_one():
    got = run(emu("clip_half"), [], W, H, pack_planes(FLIP[:1]))
    m = model(FLIP[:1], [], W, H, True, fragment=constant_fragment, first=-1)
    check(got, m, "no sources")
    assert np.array_equal(got.any(axis=-1), m[0].any(axis=-1)) and got.any()


def test_an_absent_source_in_the_middle_keeps_the_others_in_their_slots():
    tex = grid_sources()[:3]
    tex[1] = None
    got = run(emu("clip_param"), tex, W, H, pack_planes(GRID[:3]))
    # (smr_dimensions and smr_load of an absent source answer 0: its plane blends transparent black over nothing)
    m = model([GRID[0], GRID[2]], [tex[0], tex[2]], W, H, True)
    check(got, m, "absent source")
    assert np.array_equal(got.any(axis=-1), m[0].any(axis=-1))


@pytest.mark.parametrize("guard", [1, 2])
def test_on_guard_paged_buffers_no_access_falls_outside(guard):
    """Run in a child process per guard mode: a load or store that leaves its surface is a segmentation fault there, not here."""
    if not os.path.exists(emu_build.CLANG):
        pytest.skip("no clang++ to build the emulator with")
    env = dict(os.environ, SMR_EMU_USER_SHADER_GUARD=str(guard))
    r = subprocess.run([sys.executable, "-m", "tests.test_emu_user_shader_clip"], capture_output=True, text=True, env=env, cwd=ROOT, timeout=600)
    assert r.returncode == 0, f"guard mode {guard}: rc {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    assert "no access fell outside" in r.stdout, r.stdout[-2000:]


@pytest.mark.parametrize("source", ["WITH_PLANE", "WITH_AFFINE"])
def test_a_second_vertex_stage_beside_the_clip_stage_is_a_compile_error(source):
    import __graft_entry__ as ge
    ge.build()
    from smelter_amd import hip
    hip.ShaderProgram(SC.CLIP_PARAM).close()  # (the same source with the one define compiles: the error below is the two defines')
    with pytest.raises(hip.ShaderCompileError) as e:
        hip.ShaderProgram(getattr(SC, source))
    assert e.value.code == -1  # SMR_ERR_INVALID
    assert SC.CLIP_ERROR in e.value.log and SC.ONE_STAGE_ERROR in e.value.log, e.value.log


@pytest.mark.parametrize("t", PTS)
def test_the_card_shader_matches_the_model(t):
    """the renderer case's shader (sinf / cosf of in.time and smr_dimensions in the vertex stage) without the renderer"""
    tex = _textures(1, IW, IH)
    got = run(emu("flip"), tex, OW, OH, time_s=t)
    m = model(flip_planes(f32(t), 1, [(IW, IH)], OW, OH), tex, OW, OH, True)
    check(got, m, f"flip t={t}")
    assert np.array_equal(got.any(axis=-1), m[0].any(axis=-1)) and got.any() == (t < 1.5)


def test_the_example_carries_the_card_shader():
    """examples/user_shader.c's third shader is SC.FLIP, the text the renderer case runs"""
    import re
    text = open(os.path.join(ROOT, "examples", "user_shader.c")).read()
    body = text[text.index("static const char *FLIP ="):]
    body = body[:body.index('";') + 1]
    got = "".join(re.findall(r'^\s*"(.*)"$', body, flags=re.M)).replace("\\n", "\n")
    assert got.strip() == SC.FLIP.strip()


# ---- what the child processes run (python -m tests.test_emu_user_shader_clip, SMR_EMU_USER_SHADER_GUARD = the guard mode)
def inner(guard):
    tex = sources()
    for srgb in (False, True):
        check(run(emu("clip_param", guard), tex, W, H, pack_planes(FLIP), srgb=srgb), model(FLIP, tex, W, H, srgb), "flip")
        check(run(emu("clip_param", guard), tex[:1], W, H, pack_planes(BEHIND), srgb=srgb), model(BEHIND, tex[:1], W, H, srgb), "behind the eye")
        check(run(emu("clip_param", guard), grid_sources(), W, H, pack_planes(GRID), srgb=srgb), model(GRID, grid_sources(), W, H, srgb), "grid")
    for name, plane in NOTHING.items():
        assert not run(emu("clip_param", guard), tex[:1], W, H, pack_planes([plane])).any(), name


if __name__ == "__main__":
    inner(int(os.environ["SMR_EMU_USER_SHADER_GUARD"]))
    print("no access fell outside")
