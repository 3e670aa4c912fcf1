"""The affine vertex stage, smr_load and smr_dimensions of user shaders on the lane emulator: smr_user_shader_prelude.h compiled for
the CPU by tests/emu/emu_user_shader.cpp (the build of tests/test_emu_user_shader.py, with a fixture of tests/user_shader_sources_affine.py
in the user's place).  The expected pictures come from the numpy model below — geometry in f64, decode and encode through the oracle's
sRGB tables — never from the code under test.  tests/test_gpu_user_shader_affine.py holds the compiled programs to the same model."""
import ctypes as C
import math
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as orc
from tests import emu_build
from tests import user_shader_sources_affine as SA
from tests.test_gpu_shaders import _textures

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
P8 = C.POINTER(C.c_uint8)
PI = C.POINTER(C.c_int)

W, H, SW, SH = 70, 9, 5, 3  # the target: a multiple of neither 64 nor 4; the sources
EDGE = 1e-4                 # a pixel whose f64 qx or qy lies this close to +-1 may fall on either side of the edge
CAP = 0.02                  # of the target's pixels may be left out for that reason
TEXEL = 1e-5                # the constants below keep every compared pixel's uv * size this far from a texel boundary (f32 against f64)


# ------------------------------------------------------------------------------------------------------------------ the model
def decode(tex, srgb):
    """RGBA8 -> f64 in the blending space, as load_texel: the decode table for colour in sRGB mode, /255 otherwise; alpha /255."""
    t = np.asarray(tex, np.uint8)
    out = t.astype(np.float64) / 255.0
    if srgb:
        out[..., :3] = orc.srgb_decode_table().astype(np.float64)[t[..., :3]]
    return out


def encode(rgba, srgb):
    """f64 blending space -> RGBA8, as store_texel: colour code = #{i in 1..255 : thr[i] <= x} in sRGB mode, round(clamp(x) * 255) otherwise."""
    x = np.asarray(rgba, np.float64).astype(np.float32)
    unorm = np.floor(np.clip(x, 0.0, 1.0) * np.float32(255.0) + np.float32(0.5)).astype(np.uint8)
    if srgb:
        thr = orc.srgb_threshold_table()[1:256]
        unorm[..., :3] = np.searchsorted(thr, x[..., :3], side="right").astype(np.uint8)
    return unorm


def quad_coordinates(m, Wt, Ht):
    """(qx, qy, drawn) of every pixel centre for the plane {xx, xy, yx, yy, cx, cy}; drawn is False for a plane that covers nothing:
    axis-aligned with xx <= 0 or yy <= 0, det zero / NaN / infinite, or mirrored (det < 0: the reference culls back faces)."""
    xx, xy, yx, yy, cx, cy = [float(v) for v in m]
    ys, xs = np.mgrid[0:Ht, 0:Wt]
    X = (xs + 0.5) / Wt * 2.0 - 1.0
    Y = 1.0 - (ys + 0.5) / Ht * 2.0
    if xy == 0.0 and yx == 0.0:
        if not (xx > 0.0) or not (yy > 0.0):
            return None, None, False
        return (X - cx) / xx, (Y - cy) / yy, True
    det = xx * yy - xy * yx
    if not math.isfinite(det) or not det > 0.0 or not math.isfinite(float(np.float32(det))):
        return None, None, False
    dx, dy = X - cx, Y - cy
    return (dx * yy - dy * xy) / det, (dy * xx - dx * yx) / det, True


def nearest_fragment(plane, u, v, dec):
    """the fixtures' fragment: the texel of source `plane` nearest uv -> (colours, distance of uv * size to the nearest texel boundary)"""
    t = dec[plane]
    h, w = t.shape[:2]
    fu, fv = u * w, v * h
    tx, ty = np.minimum(np.floor(fu).astype(int), w - 1), np.minimum(np.floor(fv).astype(int), h - 1)
    margin = np.minimum(np.abs(fu - np.round(fu)), np.abs(fv - np.round(fv)))
    return t[ty, tx], margin


def model(planes, textures, Wt, Ht, srgb, fragment=nearest_fragment):
    """-> (RGBA8 picture, mask of pixels an edge passes too close to, smallest texel-boundary distance of a drawn pixel).  One plane per
    source in order, premultiplied-alpha OVER, stored to the RGBA8 target and read back before the next, as the kernel does."""
    dec = [decode(t, srgb) for t in textures]
    out = np.zeros((Ht, Wt, 4), np.uint8)
    doubt = np.zeros((Ht, Wt), bool)
    margin = np.inf
    for plane, m in enumerate(planes):
        qx, qy, drawn = quad_coordinates(m, Wt, Ht)
        if not drawn:
            continue
        near_x, near_y = np.abs(np.abs(qx) - 1.0) < EDGE, np.abs(np.abs(qy) - 1.0) < EDGE
        doubt |= (near_x & (np.abs(qy) < 1.0 + EDGE)) | (near_y & (np.abs(qx) < 1.0 + EDGE))
        cover = (qx >= -1.0) & (qx < 1.0) & (qy > -1.0) & (qy <= 1.0)
        u, v = (qx[cover] + 1.0) / 2.0, (1.0 - qy[cover]) / 2.0
        f, mg = fragment(plane, u, v, dec)
        if mg.size:
            margin = min(margin, float(mg[~doubt[cover]].min(initial=np.inf)))
        acc = decode(out[cover], srgb)
        out[cover] = encode(f + acc * (1.0 - f[:, 3:4]), srgb)
    return out, doubt, margin


def rotated(deg, sx, sy, cx, cy):
    """scale (sx, sy), then a turn by `deg` in clip space, then a move to (cx, cy) — the entries as the f32 the shader reads"""
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    return [float(np.float32(v)) for v in (c * sx, -s * sy, s * sx, c * sy, cx, cy)]


def pack(planes):
    return b"".join(struct.pack(f"<{len(p)}f", *p) for p in planes)


def sources():
    """two 5 x 3 sources of distinct texels; the second has noise alpha, so the order of the blend shows"""
    return _textures(2, SW, SH, seed=11)


# the planes of case 2: 30 degrees and -75 degrees, different scales, the second over the first
ROTATION = [rotated(30.0, 0.7, 0.6, -0.2, 0.1), rotated(-75.0, 0.5, 0.8, 0.25, -0.1)]
# planes whose corners lie one pixel either side of x = 64, where the spans of two waves meet: the first reaches column 64 in one row
# and no further (the second block draws that one pixel of it), the second starts at column 63 in one row (the first block draws that one)
SPAN_EDGE = [rotated(45.0, 0.25, 0.325, 0.5, 0.45), rotated(-30.0, 0.07, 0.28, 0.9, -0.4)]
# case 3: (a) - (c) mirrored, det < 0 — culled like the reference's back faces; (d) det == 0; (e) - (g) a NaN entry
NAN = float("nan")
NOTHING = {
    "mirrored_x": [-v if i in (0, 2) else v for i, v in enumerate(rotated(30.0, 0.7, 0.6, -0.2, 0.1))],
    "mirrored_y": [-v if i in (1, 3) else v for i, v in enumerate(rotated(-75.0, 0.5, 0.8, 0.25, -0.1))],
    "mirrored_axis_aligned": [-0.5, 0.0, 0.0, 0.25, 0.1, -0.2],
    "det_zero": [0.5, 0.25, 0.5, 0.25, 0.0, 0.0],
    "nan_scale": [NAN, 0.0, 0.0, 0.5, 0.0, 0.0],
    "nan_shear": [0.5, NAN, 0.1, 0.5, 0.0, 0.0],
    "nan_centre": [0.5, 0.1, 0.1, 0.5, NAN, 0.0],
}
# case 4: {i, x, y} of each smr_load in row 0 of the probe picture, for sources [5 x 3, absent]; only the first and the last hit a texel
PROBES = [(0, 0, 0), (-1, 0, 0), (2, 0, 0), (16, 0, 0), (0, -1, 0), (0, 0, -1), (0, SW, 0), (0, 0, SH), (1, 0, 0), (0, -2 ** 31, 2 ** 31 - 1),
          (0, SW - 1, SH - 1)]


# the renderer case of tests/test_gpu_user_shader_affine.py: the rotating shader over one 16 x 8 input stream, a 32 x 16 target
IW, IH, OW, OH = 16, 8, 32, 16
PTS = [0.0, 0.7]  # (at 0 the plane is axis-aligned: the fast path; at 0.7 s it has turned by 0.7 rad)


def rotate_planes(t, n_src, sizes, Wt, Ht):
    """smr_vertex_affine of SA.ROTATE in f64: the last source turned by t radians, every source before it over the whole target"""
    w, h = sizes[-1]
    fit = min(Wt / w, Ht / h) * float(np.float32(0.6))
    hw, hh = 0.5 * fit * w, 0.5 * fit * h
    c, s = math.cos(t), math.sin(t)
    return [[1.0, 0.0, 0.0, 1.0, 0.0, 0.0]] * (n_src - 1) + [[2 * hw * c / Wt, -2 * hh * s / Wt, 2 * hw * s / Ht, 2 * hh * c / Ht, 0.0, 0.0]]


def compare(got, want, doubt, margin, what):
    """within 1 LSB per channel outside the doubtful pixels; those are few, and no compared pixel sits on a texel boundary"""
    assert doubt.mean() <= CAP, f"{what}: {doubt.mean():.4f} of the pixels lie within {EDGE} of an edge"
    assert margin > TEXEL, f"{what}: a compared pixel lies {margin:.2e} from a texel boundary"
    d = np.abs(got.astype(np.int16) - want.astype(np.int16)).max(axis=-1)
    d[doubt] = 0
    assert d.max() <= 1, f"{what}: max diff {d.max()} at {np.unravel_index(d.argmax(), d.shape)}: got {got[np.unravel_index(d.argmax(), d.shape)]}, " \
                         f"want {want[np.unravel_index(d.argmax(), d.shape)]}"


def probe_expected(tex, n_cols):
    want = np.zeros((2, n_cols, 4), np.uint8)
    want[0, 0], want[0, len(PROBES) - 1] = tex[0, 0], tex[SH - 1, SW - 1]
    want[1, :, 3] = 255
    want[1, 1, :2] = [SW, SH]  # column k holds smr_dimensions(in, k - 1): -1, the 5 x 3 source, the absent one, out of range
    return want


def test_the_models_constants_stay_under_the_cap():
    """What the other tests assume about ROTATION, checked with the model alone."""
    for srgb in (True, False):
        want, doubt, margin = model(ROTATION, sources(), W, H, srgb)
        assert doubt.mean() <= CAP and margin > TEXEL, (doubt.mean(), margin)
        first = model(ROTATION[:1], sources()[:1], W, H, srgb)[0]
        both = want.any(axis=-1) & first.any(axis=-1)
        assert both.sum() >= 20 and (want[both] != first[both]).any(axis=-1).sum() >= 10  # the planes overlap and the second shows
        assert 0.2 < want.any(axis=-1).mean() < 0.9  # and neither hides the target
    for name, m in NOTHING.items():
        assert not model([m], sources()[:1], W, H, True)[0].any(), name
    want, doubt, margin = model(SPAN_EDGE, sources(), W, H, True)
    assert not doubt.any() and margin > TEXEL, (doubt.mean(), margin)
    first = model(SPAN_EDGE[:1], sources()[:1], W, H, True)[0].any(axis=-1)
    second = want.any(axis=-1) & ~first
    assert first[:, 64].sum() == 1 and not first[:, 65:].any() and first[:, :64].any()  # one pixel of the first plane in the second span
    assert second[:, 63].sum() == 2 and not second[:, :63].any() and second[:, 64:].any()  # two of the second plane in the first span,
    assert (second[:, 63] & ~second[:, 64]).sum() == 1                                     # one of them alone in its row
    for t in PTS:
        picture, doubt, margin = model(rotate_planes(float(np.float32(t)), 1, [(IW, IH)], OW, OH), _textures(1, IW, IH), OW, OH, True)
        assert doubt.mean() <= CAP and margin > TEXEL and picture.any(axis=-1).mean() > 0.1, (t, doubt.mean(), margin)


# ------------------------------------------------------------------------------------------------------------------ the emulator
def build(name):
    """tests/emu/_build/libsmr_emu_user_affine_<name>.so: the build of tests.test_emu_user_shader.build for a fixture of this file's sources"""
    out_dir = os.path.join(emu_build.EMU, "_build")
    os.makedirs(out_dir, exist_ok=True)
    user = os.path.join(out_dir, f"user_shader_affine_{name}.inc")
    text = "// generated from tests/user_shader_sources_affine.py\n" + SA.ALL[name]
    if not os.path.exists(user) or open(user).read() != text:
        with open(user, "w") as f:
            f.write(text)
    lib = os.path.join(out_dir, f"libsmr_emu_user_affine_{name}.so")
    deps = [user, os.path.join(emu_build.EMU, "emu_user_shader.cpp"), os.path.join(emu_build.EMU, "emu_device.h"), os.path.join(emu_build.EMU, "emu_guard.h"),
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


def run(emu, textures, Wt, Ht, params=b"", time_s=0.0, srgb=True):
    """tests.test_emu_user_shader.run with absent sources: a None in `textures` is a NULL entry"""
    n = len(textures)
    tex = [None if t is None else np.ascontiguousarray(t, np.uint8) for t in textures]
    px = (P8 * max(n, 1))(*[None if t is None else t.ctypes.data_as(P8) for t in tex])
    ws = (C.c_int * max(n, 1))(*[0 if t is None else t.shape[1] for t in tex])
    hs = (C.c_int * max(n, 1))(*[0 if t is None else t.shape[0] for t in tex])
    pbuf = np.frombuffer(bytes(params) or b"\0", np.uint8).copy()
    out = np.zeros((Ht, Wt, 4), np.uint8)
    rc = emu.emu_user_shader(n, px, ws, hs, Wt, Ht, 1 if srgb else 0, float(time_s), pbuf.ctypes.data_as(P8), len(params), out.ctypes.data_as(P8))
    assert rc == 0, rc
    return out


_EMUS = {}


def emu(name, guard=0):
    if not os.path.exists(emu_build.CLANG):
        pytest.skip("no clang++ to build the emulator with")
    if name not in _EMUS:
        _EMUS[name] = build(name)
    _EMUS[name].emu_set_guard(guard, 1 if guard else 0)
    return _EMUS[name]


@pytest.mark.parametrize("srgb", [True, False])
def test_an_axis_aligned_affine_plane_is_the_smr_plane_one_byte_for_byte(srgb):
    tex = sources()[:1]
    as_plane = run(emu("plane_param"), tex, W, H, pack([[0.5, 0.25, 0.1, -0.2]]), srgb=srgb)
    as_affine = run(emu("affine_param"), tex, W, H, pack([[0.5, 0.0, 0.0, 0.25, 0.1, -0.2]]), srgb=srgb)
    assert as_plane.any() and not as_plane.all(axis=-1).all()  # (the plane covers part of the target, not all of it)
    assert np.array_equal(as_plane, as_affine), f"{(as_plane != as_affine).sum()} bytes differ"
    want, doubt, margin = model([[0.5, 0.0, 0.0, 0.25, 0.1, -0.2]], tex, W, H, srgb)
    compare(as_affine, want, doubt, margin, "axis-aligned")


@pytest.mark.parametrize("srgb", [True, False])
def test_rotated_planes_match_the_model(srgb):
    got = run(emu("affine_param"), sources(), W, H, pack(ROTATION), srgb=srgb)
    want, doubt, margin = model(ROTATION, sources(), W, H, srgb)
    compare(got, want, doubt, margin, "rotation")


@pytest.mark.parametrize("srgb", [True, False])
def test_planes_that_end_a_pixel_past_a_wave_span_boundary_match_the_model(srgb):
    """the wave early-out must not drop a plane for a span that holds one pixel of it"""
    got = run(emu("affine_param"), sources(), W, H, pack(SPAN_EDGE), srgb=srgb)
    want, doubt, margin = model(SPAN_EDGE, sources(), W, H, srgb)
    compare(got, want, doubt, margin, "span edge")
    assert np.array_equal(got.any(axis=-1), want.any(axis=-1))  # (no pixel is doubtful: coverage is exactly the model's)


@pytest.mark.parametrize("name", sorted(NOTHING))
def test_mirrored_singular_and_nan_planes_cover_nothing(name):
    """det < 0: the reference's pipeline culls back faces (wgpu/common_pipeline.rs:104-107), so a mirrored plane is not drawn"""
    got = run(emu("affine_param"), sources()[:1], W, H, pack([NOTHING[name]]))
    assert not got.any(), f"{name}: {np.count_nonzero(got.any(axis=-1))} pixels drawn"


@pytest.mark.parametrize("srgb", [False, True])
def test_smr_load_reproduces_the_source_tiled(srgb):
    tex = sources()[1]  # (the one with noise alpha)
    got = run(emu("tile"), [tex], W, H, srgb=srgb)
    want = np.tile(tex, (H // SH + 1, W // SW + 1, 1))[:H, :W]
    assert np.array_equal(got, want), f"{(got != want).sum()} bytes differ"


def test_smr_load_and_smr_dimensions_out_of_range_and_absent():
    tex = sources()[0]
    n = len(PROBES) + 1
    got = run(emu("probe"), [tex, None], n, 2, b"".join(struct.pack("<3i", *p) for p in PROBES), srgb=False)
    assert np.array_equal(got, probe_expected(tex, n)), got.tolist()
    assert not run(emu("tile"), [None], 8, 2, srgb=False).any()


@pytest.mark.parametrize("guard", [1, 2])
def test_on_guard_paged_buffers_no_access_falls_outside(guard):
    """Run in a child process per guard mode: a load or store that leaves its surface is a segmentation fault there, not here."""
    if not os.path.exists(emu_build.CLANG):
        pytest.skip("no clang++ to build the emulator with")
    env = dict(os.environ, SMR_EMU_USER_SHADER_GUARD=str(guard))
    r = subprocess.run([sys.executable, "-m", "tests.test_emu_user_shader_affine"], capture_output=True, text=True, env=env, cwd=ROOT, timeout=600)
    assert r.returncode == 0, f"guard mode {guard}: rc {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    assert "no access fell outside" in r.stdout, r.stdout[-2000:]


def test_both_vertex_stages_in_one_source_is_a_compile_error():
    import __graft_entry__ as ge
    ge.build()
    from smelter_amd import hip
    hip.ShaderProgram(SA.AFFINE_PARAM).close()  # (the same source with the one define compiles: the error below is the two defines')
    with pytest.raises(hip.ShaderCompileError) as e:
        hip.ShaderProgram(SA.BOTH_DEFINES)
    assert e.value.code == -1  # SMR_ERR_INVALID
    assert SA.BOTH_DEFINES_ERROR in e.value.log, e.value.log


@pytest.mark.parametrize("t", PTS)
def test_the_rotating_shader_matches_the_model(t):
    """the renderer case's shader (sinf / cosf of in.time in the vertex stage, smr_dimensions for the aspect ratio) without the renderer"""
    tex = _textures(1, IW, IH)
    got = run(emu("rotate"), tex, OW, OH, time_s=t)
    compare(got, *model(rotate_planes(float(np.float32(t)), 1, [(IW, IH)], OW, OH), tex, OW, OH, True), f"rotate t={t}")


def test_the_example_carries_the_rotating_shader():
    """examples/user_shader.c's second shader is SA.ROTATE, the text the renderer case runs"""
    import re
    text = open(os.path.join(ROOT, "examples", "user_shader.c")).read()
    body = text[text.index("static const char *ROTATE ="):]
    body = body[:body.index('";') + 1]
    got = "".join(re.findall(r'^\s*"(.*)"$', body, flags=re.M)).replace("\\n", "\n")
    assert got.strip() == SA.ROTATE.strip()


# ---- what the child processes run (python -m tests.test_emu_user_shader_affine, SMR_EMU_USER_SHADER_GUARD = the guard mode)
def inner(guard):
    tex = sources()
    n = len(PROBES) + 1
    got = run(emu("probe", guard), [tex[0], None], n, 2, b"".join(struct.pack("<3i", *p) for p in PROBES), srgb=False)
    assert np.array_equal(got, probe_expected(tex[0], n))
    for srgb in (False, True):
        got = run(emu("tile", guard), [tex[1]], W, H, srgb=srgb)
        assert np.array_equal(got, np.tile(tex[1], (H // SH + 1, W // SW + 1, 1))[:H, :W])
        got = run(emu("affine_param", guard), tex, W, H, pack(ROTATION), srgb=srgb)
        compare(got, *model(ROTATION, tex, W, H, srgb), "rotation")
    for name, m in NOTHING.items():
        assert not run(emu("affine_param", guard), tex[:1], W, H, pack([m])).any(), name


if __name__ == "__main__":
    inner(int(os.environ["SMR_EMU_USER_SHADER_GUARD"]))
    print("no access fell outside")
