"""The compositor's copy workgroups walking RUNS of tiles, its paired stores and its one cold guard repair per block, on the lane emulator
(tests/emu/emu_compose_walk.cpp: k_classify_tiles + k_compose_output of smelter_amd/csrc/smr_fused_compose.h compiled for the CPU, launched with
a caller-chosen number of copy workgroups and with the per-wave lane exchange set up): EVERY BYTE EQUAL to the oracle's apply_layouts +
rgba_to_yuv / rgba_to_nv12, whatever the run length, and equal to the launch with a workgroup per tile.  Test infrastructure only;
tests/test_gpu_compose_walk.py holds the gfx950 binary to the oracle on the same scenes."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import oracle as orc
from tests.compose_walk import FLAGGED_TEXTURE, OUTS, SIZES, flagged_scene, tiles_of, walk_scene

HERE = os.path.dirname(os.path.abspath(__file__))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
P8 = C.POINTER(C.c_uint8)
CLASSES = ["clear", "colour", "texture", "full", "skip", "sampled", "select"]


@pytest.fixture(scope="module")
def emu():
    if not os.path.exists(CLANG):
        pytest.skip("no clang++ to build the emulator with")
    from tests import emu_build
    lib = emu_build.build("smr_emu_compose_walk", "emu_compose_walk.cpp", ("smr_fused_compose.h", "smr_layout_dev.h", "smr_convert_dev.h", "smr_yuv_fast.h", "smr_tables.h"))
    h = C.CDLL(lib)
    h.emu_compose_walk.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(P8), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                   C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, P8, P8, P8, C.POINTER(C.c_int)]
    h.emu_yuv_flagged.argtypes = [C.c_int, C.POINTER(C.c_int), C.c_int]
    h.emu_yuv_block_flags.argtypes = [P8, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    orc.build()
    return h


def _p(a):
    return a.ctypes.data_as(P8)


def compose(emu, scene, W, H, out, groups, srgb=True):
    layouts, sources, kinds, shifts = scene
    arr = orc.pack_layouts(layouts)
    n = len(sources)
    keep = [np.ascontiguousarray(s, np.uint8) for s in sources]
    px = (P8 * n)(*[_p(s) for s in keep])
    ws = (C.c_int * n)(*[s.shape[1] for s in keep])
    hs = (C.c_int * n)(*[s.shape[0] for s in keep])
    ks = (C.c_int * n)(*kinds)
    sh = (C.c_int * n)(*shifts)
    info = (C.c_int * 10)()
    nv = {"planar": 0, "nv12": 1, "rgba": 2}[out]
    if nv == 2:
        o0, o1, o2 = np.zeros((H, W, 4), np.uint8), np.zeros(1, np.uint8), np.zeros(1, np.uint8)
    elif nv == 1:
        o0, o1, o2 = np.zeros((H, W), np.uint8), np.zeros((H // 2, W // 2, 2), np.uint8), np.zeros(1, np.uint8)
    else:
        o0, o1, o2 = np.zeros((H, W), np.uint8), np.zeros((H // 2, W // 2), np.uint8), np.zeros((H // 2, W // 2), np.uint8)
    rc = emu.emu_compose_walk(C.addressof(arr), len(layouts), n, px, ws, hs, ks, sh, W, H, nv, int(srgb), groups, _p(o0), _p(o1), _p(o2), info)
    assert rc == 0, rc
    return (o0, o1, o2)[:{0: 3, 1: 2, 2: 1}[nv]], dict(zip(CLASSES + ["listed", "workgroups", "pairs"], list(info)))


_ORACLE = {}


def oracle_output(scene, W, H, out, srgb=True, key=None):
    """(computed once per scene and format, shared, never written to)"""
    if key is not None and (key, out) in _ORACLE:
        return _ORACLE[(key, out)]
    layouts, sources = scene[0], scene[1]
    rgba = orc.apply_layouts(W, H, layouts, sources, srgb=srgb)
    got = (rgba,) if out == "rgba" else orc.rgba_to_nv12(rgba) if out == "nv12" else orc.rgba_to_planar_yuv(rgba, orc.YUV420)
    got = tuple(np.asarray(g) for g in got)
    if key is not None:
        _ORACLE[(key, out)] = got
    return got


def assert_same(got, want, what):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        w = np.asarray(w).reshape(g.shape)
        assert np.array_equal(g, w), (what, "plane", k, int((g != w).sum()), np.argwhere(g != w)[:5].tolist())


def group_counts(W, H):
    t = tiles_of(W, H)
    return sorted({1, 2, 3, t - 1, t, t + 3})


@pytest.mark.parametrize("out", OUTS)
@pytest.mark.parametrize("W,H", SIZES)
def test_runs_of_every_length_are_the_oracle_and_the_launch_with_a_workgroup_per_tile(emu, W, H, out):
    scene = walk_scene(W, H)
    want = oracle_output(scene, W, H, out, key=(W, H))
    tiles = tiles_of(W, H)
    per_tile, classes = compose(emu, scene, W, H, out, tiles)
    assert_same(per_tile, want, (W, H, out, "a workgroup per tile", classes))
    assert classes["pairs"] == (0 if out == "rgba" else 1)   # (the allocator's 256-byte pitches admit the paired stores)
    for groups in group_counts(W, H):
        if groups == tiles:
            continue
        got, classes = compose(emu, scene, W, H, out, groups)
        assert classes["workgroups"] == classes["listed"] + groups
        assert_same(got, want, (W, H, out, groups, classes))
        assert_same(got, per_tile, (W, H, out, groups, "against a workgroup per tile"))


def test_every_tile_class_occurs_in_the_scenes(emu):
    seen = dict.fromkeys(CLASSES, 0)
    for W, H in SIZES:
        _got, classes = compose(emu, walk_scene(W, H), W, H, "planar", 3)
        for c in CLASSES:
            seen[c] += classes[c]
    for c in ("clear", "colour", "texture", "sampled", "select", "full"):
        assert seen[c] > 0, seen


@pytest.mark.parametrize("out", OUTS)
def test_paired_and_per_lane_stores_write_no_padding_byte(emu, out):
    """Guard mode 3 of the harness (tests/emu/emu_guard.h): sources on their smallest pitch, every output plane on its smallest pitch + 32,
    pre-filled from a seeded pattern whose row padding is compared after the launch.  Width 384: the planes' pitches (416, 224) keep the
    paired stores; widths 386 and 1282 (420 / 226, 1316 / 674): per-lane stores."""
    emu.emu_set_guard(3, 1)
    try:
        took = set()
        for W, H in SIZES:
            scene = walk_scene(W, H)
            want = oracle_output(scene, W, H, out, key=(W, H))
            for groups in (2, tiles_of(W, H)):
                got, classes = compose(emu, scene, W, H, out, groups)   # (rc -77: a padding byte was written)
                assert_same(got, want, (W, H, out, groups, "guard mode", classes))
            took.add(classes["pairs"])
        assert took == ({0} if out == "rgba" else {0, 1}), took
    finally:
        emu.emu_set_guard(0, 0)


# ---- guard coverage: blocks whose fast-path values raise the guard flag (smr_yuv_fast.h)

def flagged_inputs(emu):
    buf = (C.c_int * (3 * 256))()
    n = emu.emu_yuv_flagged(0, buf, 256)
    luma = np.array(buf[:3 * n], np.int64).reshape(n, 3)
    sums = []
    for plane in (1, 2):
        m = emu.emu_yuv_flagged(plane, buf, 64)
        sums.append(np.array(buf[:3 * m], np.int64).reshape(m, 3))
    return luma, np.concatenate(sums)


def flagged_texture(emu):
    """128 x 16 opaque texels = 32 x 8 blocks of 4 x 2, by block column: 0 mod 4 — random pixels; 1 — one flagged luma triple among random
    pixels; 2 — a 2x2 half whose byte sums are a flagged chroma input; 3 — eight flagged luma triples.  -> (texture, luma flags per
    block, chroma flags per block, triples found, sums found)"""
    luma, sums = flagged_inputs(emu)
    rng = np.random.default_rng(7)
    t = rng.integers(0, 256, (16, 128, 4), dtype=np.uint8)
    t[..., 3] = 255
    k = 0
    for by in range(8):
        for bx in range(32):
            blk = t[2 * by:2 * by + 2, 4 * bx:4 * bx + 4]
            kind = bx % 4
            if kind == 1:
                blk[rng.integers(0, 2), rng.integers(0, 4), :3] = luma[k % len(luma)]
            elif kind == 2:
                s = sums[k % len(sums)]
                for ch in range(3):   # four bytes with that sum
                    q, r = divmod(int(s[ch]), 4)
                    blk[:, 0:2, ch] = np.array([[q + (r > 0), q + (r > 1)], [q + (r > 2), q]], np.uint8)
            elif kind == 3:
                for j in range(8):
                    blk[j // 4, j % 4, :3] = luma[(k + j) % len(luma)]
            k += 8
    nl, nc = (C.c_int * 256)(), (C.c_int * 256)()
    tt = np.ascontiguousarray(t)
    emu.emu_yuv_block_flags(_p(tt), 128, 16, nl, nc)
    return tt, np.array(nl[:]), np.array(nc[:]), len(luma), len(sums)


def test_blocks_with_no_one_and_only_flagged_values_are_the_oracle(emu):
    t, nl, nc, n_luma, n_sums = flagged_texture(emu)
    assert n_luma >= 64 and n_sums >= 16, (n_luma, n_sums)
    assert ((nl == 0) & (nc == 0)).any() and ((nl == 1) & (nc == 0)).any() and ((nl == 0) & (nc == 1)).any() and (nl == 8).any(), (nl.tolist(), nc.tolist())
    assert np.array_equal(np.load(FLAGGED_TEXTURE), t), "tests/golden/compose_walk_flagged.npy (what the device test reads) is not this texture"
    W, H = 128, 16
    scene = flagged_scene(t)
    for out in OUTS:
        want = oracle_output(scene, W, H, out)
        got, classes = compose(emu, scene, W, H, out, 1)
        assert classes["texture"] == 1, classes
        assert_same(got, want, ("flagged texture", out))
