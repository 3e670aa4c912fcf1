"""k_ingest_wave's tile stores at the edges of a destination, on the CPU (the lane emulator of tests/emu, through the entry points of
tests/test_emu_wave.py).  A tile that lies wholly inside the destination is stored by a straight-line path — one 16-byte store per lane, chosen
once for the wave — and a tile the destination's right or bottom edge cuts by the per-lane path with its ragged tail.  The sizes below put both
kinds side by side: widths with a tail of 1 .. 3 texels behind one or three whole tile columns, a width of exactly two tile columns, one texel
more, one whole lane group less; heights of exactly one tile row, one row more, one row less than two.

Every case runs in guard mode 3 (tests/emu/emu_guard.h): the tile sits on the smallest admitted pitch + 32 bytes of seeded padding that is
compared after the launch, so a store that reaches past a row's last texel fails the case.  Three properties per case:
  * within 1 LSB of the oracle's resample of the same node texture;
  * the RGB12-node build's tile is the RGBA8-node build's tile bit for bit (same codes in, same arithmetic);
  * the d_w x d_h tile is byte-equal to the top-left d_w x d_h texels of the same job (same source, scales and offsets) rendered 32 columns wider
    and 16 rows taller: there the narrow job's edge tiles are interior tiles, so the two store paths must write the same bytes.  (A texel's weights
    depend on the scale, the offset and the source size alone; a column pair's window starts where its first tile's does and a chunk's ring slot is
    absolute, so the larger job sums the same products in the same order plus exact zeros.)
Every case and node kind meets the exact-fraction floor tests/test_emu_wave.py asks of a node-texture case (0.9995) on its own; the fraction
pooled over all cases is asserted once more on top."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import oracle as orc

CLANG = "/opt/rocm/lib/llvm/bin/clang++"
P8 = C.POINTER(C.c_uint8)

WIDTHS = (29, 31, 32, 33, 35, 48, 61)
HEIGHTS = (16, 17, 31)
GROW = (32, 16)  # the larger job of the crop identity: one column pair wider, one tile row taller
FLOOR = 0.9995   # (tests/test_emu_wave.py: test_emulated_kernel_on_an_rgba_node_texture)

# scale -> source size: holds the crop of the largest grown job (61 + 32 columns, 31 + 16 rows; the 3x case 33 + 32, 31 + 16), width a multiple of 4
# (RGB12 rows hold whole groups of four texels)
SOURCES = {1.5: (144, 72), 3.0: (196, 144)}
CASES_3X = [(33, 31)]  # the <8, 3> class: a tail of one texel behind two tile columns, one row less than two tile rows


@pytest.fixture(scope="module")
def emu():
    if not os.path.exists(CLANG):
        pytest.skip("no clang++ to build the emulator with")
    from tests import emu_build
    h = C.CDLL(emu_build.build("smr_emu"))
    h.emu_ingest_wave.argtypes = [P8, P8, P8, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, P8, C.c_int, C.c_int,
                                  C.c_int, C.c_int, C.POINTER(C.c_int)]
    orc.build()
    h.emu_set_guard(3, 1)
    yield h
    h.emu_set_guard(int(os.environ.get("SMR_EMU_GUARD", "0")), 1 if os.environ.get("SMR_EMU_GUARD") else 0)  # (the library is shared with test_emu_wave.py)


def _p(a):
    return a.ctypes.data_as(P8)


_nodes, _results = {}, {}


def _node(scale):
    """white noise, opaque: the RGBA8 node texture and the same codes as RGB12 rows [R0 R1 R2 R3 G0 .. G3 B0 .. B3] per four pixels"""
    if scale not in _nodes:
        sw, sh = SOURCES[scale]
        node = np.random.default_rng(int(scale * 1000) + sw).integers(0, 256, (sh, sw, 4), dtype=np.uint8)
        node[..., 3] = 255
        packed = np.ascontiguousarray(node[..., :3].reshape(sh, sw // 4, 4, 3).transpose(0, 1, 3, 2)).reshape(sh, 3 * sw)
        _nodes[scale] = (np.ascontiguousarray(node), packed)
    return _nodes[scale]


def _render(emu, scale, kind, dw, dh):
    """-> (tile, plan tail, (NKS, K, KV)) on the node texture (kind 2: RGBA8, 6: RGB12): by the class build of the job's k-step counts where there
    is one, else (-2: heights of 16 and 17 at scale 1.5 have pass-2 windows of one k-step, no class's) by the generic build — the same store code,
    there without the deferral"""
    sw, sh = SOURCES[scale]
    node, packed = _node(scale)
    crop = (0.0, 0.0, scale * dw, scale * dh)
    assert crop[2] <= sw and crop[3] <= sh
    plan = orc.resample_plan(sw, sh, crop, dw, dh)
    assert plan.kind == 2 and plan.levels == (0, 0) and tuple(plan.axis[:2]) == (0, 1), plan
    tail = (plan.scale[0], plan.offset[0], plan.scale[1], plan.offset[1])
    src = packed if kind == 6 else node
    got = np.zeros((dh, dw, 4), np.uint8)
    info = (C.c_int * 4)()
    rc = emu.emu_ingest_wave(_p(src), _p(src), _p(src), sw, sh, 0, kind, *tail, _p(got), dw, dh, 2, 1, info)
    if rc == -2:
        rc = emu.emu_ingest_wave(_p(src), _p(src), _p(src), sw, sh, 0, kind, *tail, _p(got), dw, dh, 2, 0, info)
    assert rc == 0, f"{dw}x{dh} kind {kind}: rc {rc} (-77: row padding was written) {list(info)}"
    return got, tail, tuple(info[:3])


def _case(emu, scale, dw, dh):
    """One destination size, computed once: the tile from either node, the oracle's tile and the exact-byte count."""
    key = (scale, dw, dh)
    if key in _results:
        return _results[key]
    sw, sh = SOURCES[scale]
    node, _ = _node(scale)
    _, want = orc.resample(node, (0.0, 0.0, scale * dw, scale * dh), dw, dh)
    out = {"want": want}
    for kind in (2, 6):
        got, tail, ks = _render(emu, scale, kind, dw, dh)
        big, tail_big, _ = _render(emu, scale, kind, dw + GROW[0], dh + GROW[1])
        assert tail_big == tail, (tail, tail_big)  # the same job: same scales and offsets
        out[kind] = (got, big[:dh, :dw], ks)
    _results[key] = out
    return out


def _check(out, dw, dh, kv, nks_max):
    want = out["want"]
    for kind in (2, 6):
        got, cropped, ks = out[kind]
        assert ks[1] <= nks_max and ks[2] == kv, (kind, ks)
        d = np.abs(got.astype(np.int16) - want.astype(np.int16))
        print(f"{dw}x{dh} kind {kind}: max |diff| {d.max()}, exact {(d == 0).mean():.5f} of {d.size}")
        assert d.max() <= 1, f"kind {kind}: {(d > 1).sum()} bytes off by more than 1 (max {d.max()})"
        assert (d == 0).mean() >= FLOOR, f"kind {kind}: exact fraction {(d == 0).mean():.5f} of {d.size} bytes (< {FLOOR})"
        assert (got[..., 3] == 255).all()
        bad = np.argwhere((got != cropped).any(axis=-1))
        assert bad.size == 0, f"kind {kind}: {len(bad)} texels differ from the grown job's, the first at (row, column) {tuple(bad[0])}"
    assert np.array_equal(out[2][0], out[6][0]), int((out[2][0] != out[6][0]).sum())


@pytest.mark.parametrize("dh", HEIGHTS)
@pytest.mark.parametrize("dw", WIDTHS)
def test_edge_tiles_at_scale_1_5(emu, dw, dh):
    """the benchmark's class (<4, 2>): windows of at most 4 k-steps, pass-2 windows of 2 (of 1 below 18 rows: the generic build)"""
    _check(_case(emu, 1.5, dw, dh), dw, dh, 2 if dh > 17 else 1, 4)


@pytest.mark.parametrize("dw,dh", CASES_3X)
def test_edge_tiles_at_scale_3(emu, dw, dh):
    """the <8, 3> class: windows of at most 8 k-steps, pass-2 windows of 3"""
    _check(_case(emu, 3.0, dw, dh), dw, dh, 3, 8)


def test_pooled_exact_fraction(emu):
    """over every case above, on top of each case's own floor (cases another test has computed are not computed again)"""
    eq = n = 0
    for scale, cases in ((1.5, [(w, h) for w in WIDTHS for h in HEIGHTS]), (3.0, CASES_3X)):
        for dw, dh in cases:
            out = _case(emu, scale, dw, dh)
            for kind in (2, 6):
                eq += int((out[kind][0] == out["want"]).sum())
                n += out["want"].size
    print(f"pooled exact fraction {eq / n:.5f} over {n} bytes (floor {FLOOR})")
    assert eq / n >= FLOOR, f"pooled exact fraction {eq / n:.5f} over {n} bytes (< {FLOOR})"
