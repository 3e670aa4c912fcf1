"""The 10-bit 4:2:2 input converter (smelter_amd/csrc/smr_convert_hi422.h, k_yuv422_hi_to_rgba's per-thread runs of 4 x 4 blocks: planar
10-bit, P210, v210) compiled for the CPU by tests/emu/emu_convert_hi422.cpp.  EVERY BYTE EQUAL, twice:

  * content whose 10-bit codes are 4 b against the ORACLE — planar_yuv_to_rgba(YUV422) of the bytes b for planar and P210,
    interleaved422_to_rgba of the UYVY frame with bytes b for v210 (the value rule of include/smr.h makes the 8-bit reference apply);
  * true 10-bit content against the witnesses: tests/hi_depth_model.py::node_rgba with (h, w / 2) chroma planes, and
    tests/hi422_model.py::node_rgba_v210 — itself held to the oracle on 4 b content here before it is used.

Test infrastructure only: the product has no CPU path; tests/test_gpu_hi422.py holds the kernels themselves on the device."""
import ctypes as C
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

from oracle import oracle as orc
from tests import hi422_model as h422
from tests import hi_depth_model as hdm

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
P8 = C.POINTER(C.c_uint8)
# (12, 2): all three g % 3 cases | (260, 10): a second 64-lane column group, and a partly filled last v210 group
SIZES = [(8, 2), (12, 2), (16, 6), (20, 4), (24, 2), (28, 6), (132, 74), (260, 10), (1920, 8)]
GUARD_SIZES = [(8, 2), (12, 2), (260, 10)]
EXTREMES = np.array([0, 1, 63, 64, 65, 66, 67, 68, 511, 512, 513, 939, 940, 941, 959, 960, 961, 1022, 1023], np.uint16)  # (test_emu_convert_hi.py's)
LAYOUTS = ["planar", "p210", "v210"]
LAYOUT_ID = {"planar": 0, "p210": 1, "v210": 2}
_HANDLE = None


def _emu():
    global _HANDLE
    if _HANDLE is None:
        from tests import emu_build
        lib = emu_build.build("smr_emu_convert_hi422", "emu_convert_hi422.cpp",
                              ("smr_convert_hi422.h", "smr_convert_hi.h", "smr_convert_420.h", "smr_convert_batch.h", "smr_convert_dev.h", "smr_yuv_fast.h"))
        h = C.CDLL(lib)
        h.emu_convert_hi422_run.argtypes = [P8, P8, P8, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, P8]
        PP8, PI = C.POINTER(P8), C.POINTER(C.c_int)
        h.emu_convert_hi422_shares.argtypes = [C.c_int, PP8, PP8, PP8, PI, PI, C.c_int, PI, C.c_int, PP8]
        h.emu_v210_pixel_codes.argtypes = [P8, C.c_int, C.c_int, C.POINTER(C.c_uint16)]
        orc.build()
        if os.environ.get("SMR_EMU_GUARD"):  # the child of test_converter_never_leaves_its_planes: planes of exactly pitch * h bytes against an unmapped page
            h.emu_set_guard(int(os.environ["SMR_EMU_GUARD"]), 1 if os.environ.get("SMR_EMU_PITCH", "tight") == "tight" else 0)
        _HANDLE = h
    return _HANDLE


@pytest.fixture(scope="module")
def emu():
    if not os.path.exists(CLANG):
        pytest.skip("no clang++ to build the emulator with")
    return _emu()


def _p(a):
    return a.ctypes.data_as(P8)


def _content8(kind, w, h, rng):
    """tests/test_emu_convert_hi.py's contents in 4:2:2 geometry: (y bytes (h, w), chroma byte pairs (h, w / 2, 2))."""
    cw = w // 2
    if kind == "noise":
        return rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h, cw, 2), dtype=np.uint8)
    if kind == "extremes":  # the range clamps' corners and their neighbours
        return (rng.choice(np.array([0, 1, 15, 16, 17, 234, 235, 236, 254, 255], np.uint8), (h, w)),
                rng.choice(np.array([0, 15, 16, 17, 127, 128, 129, 239, 240, 241, 255], np.uint8), (h, cw, 2)))
    xx, yy = np.meshgrid(np.arange(w), np.arange(h))  # camera-like: smooth luma, slow chroma
    y = (16 + (xx * 3 + yy * 2) % 200 + rng.integers(0, 8, (h, w))).astype(np.uint8)
    c = np.stack([(100 + (np.arange(cw)[None, :] + np.arange(h)[:, None]) % 60), (140 - (np.arange(cw)[None, :] * 2 + np.arange(h)[:, None]) % 70)], -1).astype(np.uint8)
    return y, c


def _content10(kind, w, h, rng):
    """True 10-bit codes: (y (h, w), chroma pairs (h, w / 2, 2)), uint16."""
    cw = w // 2
    if kind == "noise":
        return rng.integers(0, 1024, (h, w)).astype(np.uint16), rng.integers(0, 1024, (h, cw, 2)).astype(np.uint16)
    return rng.choice(EXTREMES, (h, w)), rng.choice(EXTREMES, (h, cw, 2))


def _planes(layout, y, c, junk=None):
    """Codes y (h, w), chroma pairs c (h, w / 2, 2) -> the layout's three byte views (unused ones repeat the first).  junk: random generator
    for the ignored bits — the six other bits of a word, or bits 30 - 31 of a v210 dword and the components beyond w."""
    y, c = np.asarray(y, np.uint16), np.asarray(c, np.uint16)
    h, w = y.shape
    if layout == "v210":
        n = h422.groups(w)
        plane = h422.v210_pack(y, c[..., 0], c[..., 1], junk=None if junk is None else junk.integers(0, 4, (h, 4 * n)),
                               beyond=None if junk is None else junk.integers(0, 1024, (h, 6 * n)))
        b = plane.view(np.uint8)
        return b, b, b
    jy = np.zeros_like(y) if junk is None else junk.integers(0, 64, y.shape).astype(np.uint16)
    jc = np.zeros_like(c) if junk is None else junk.integers(0, 64, c.shape).astype(np.uint16)
    if layout == "p210":
        yw, cw_ = np.ascontiguousarray((y << 6) | jy), np.ascontiguousarray((c << 6) | jc)
        return yw.view(np.uint8), cw_.view(np.uint8), cw_.view(np.uint8)
    yw, cw_ = np.ascontiguousarray(y | (jy << 10)), c | (jc << 10)
    return yw.view(np.uint8), np.ascontiguousarray(cw_[..., 0]).view(np.uint8), np.ascontiguousarray(cw_[..., 1]).view(np.uint8)


def _run(emu, layout, y, c, rgb12, nb=1, junk=None):
    """The emulated converter on codes y, c (chroma pairs) -> (h, w, 4) RGBA8 (an RGB12 node unpacked, alpha 255)."""
    h, w = y.shape
    py, pu, pv = _planes(layout, y, c, junk)
    out = np.zeros((h, 3 * w), np.uint8) if rgb12 else np.zeros((h, w, 4), np.uint8)
    rc = emu.emu_convert_hi422_run(_p(py), _p(pu), _p(pv), w, h, LAYOUT_ID[layout], 1 if rgb12 else 0, nb, _p(out))
    assert rc == 0, rc
    return hdm.rgb12_rows_to_rgba(out, w, h) if rgb12 else out


def _oracle8(layout, y, c):
    h, w = y.shape
    if layout == "v210":
        return orc.interleaved422_to_rgba(h422.uyvy_of(y, c[..., 0], c[..., 1]), w, h, 0)
    return orc.planar_yuv_to_rgba(y, np.ascontiguousarray(c[..., 0]), np.ascontiguousarray(c[..., 1]), w, h, orc.YUV422)


def _witness(layout, y, c):
    if layout == "v210":
        return h422.node_rgba_v210(y, c[..., 0], c[..., 1])
    return hdm.node_rgba(y, c[..., 0], c[..., 1])


def _diff(got, want):
    return int((got != want).sum()), np.argwhere(got != want)[:4].tolist()


def _seed(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kind", ["noise", "extremes", "camera"])
def test_codes_4b_give_the_oracles_bytes_of_b(emu, w, h, layout, kind):
    """A 10-bit 4:2:2 frame whose codes are 4 b has the node texture, byte for byte, of the 8-bit frame with bytes b — RGBA8 and RGB12 — and
    the witness agrees with the oracle there (asserted before the witness is used anywhere)."""
    rng = _seed(w, h, layout, kind)
    y, c = _content8(kind, w, h, rng)
    want = _oracle8(layout, y, c)
    y10, c10 = y.astype(np.uint16) * 4, c.astype(np.uint16) * 4
    assert np.array_equal(_witness(layout, y10, c10), want), "the witness is not the oracle on 4 b content"
    for rgb12 in (0, 1):
        got = _run(emu, layout, y10, c10, rgb12)
        assert np.array_equal(got, want), (layout, kind, w, h, rgb12, _diff(got, want))


@pytest.mark.parametrize("w", list(range(8, 262, 2)))
def test_the_v210_witness_is_the_oracle_on_4b_content_at_every_even_width_from_8(w):
    """node_rgba_v210 against orc.interleaved422_to_rgba at every even width from 8 to 260 (below 8 the oracle's own x_pos formula leaves the
    rule: those widths are held to the model only)."""
    orc.build()
    rng = _seed(w, "witness")
    y, c = _content8("noise", w, 3, rng)
    want = orc.interleaved422_to_rgba(h422.uyvy_of(y, c[..., 0], c[..., 1]), w, 3, 0)
    assert np.array_equal(h422.node_rgba_v210(y.astype(np.uint16) * 4, c[..., 0].astype(np.uint16) * 4, c[..., 1].astype(np.uint16) * 4), want)


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kind", ["noise", "extremes"])
def test_true_10_bit_content_is_the_witness_byte_for_byte(emu, w, h, layout, kind):
    rng = _seed(w, h, layout, kind, 10)
    y, c = _content10(kind, w, h, rng)
    want = _witness(layout, y, c)
    for rgb12 in (0, 1):
        for nb in (1, 2):  # (runs of one block and runs that prefetch the next)
            got = _run(emu, layout, y, c, rgb12, nb=nb)
            assert np.array_equal(got, want), (layout, kind, w, h, rgb12, nb, _diff(got, want))


@pytest.mark.parametrize("w,h", [(1, 1), (2, 2), (5, 3), (6, 1), (7, 5), (12, 2), (13, 2), (37, 21), (260, 3)])
def test_v210_pack_and_unpack_are_inverses(w, h):
    rng = _seed(w, h, "pack")
    y = rng.integers(0, 1024, (h, w)).astype(np.uint16)
    cb, cr = rng.integers(0, 1024, (h, (w + 1) // 2)).astype(np.uint16), rng.integers(0, 1024, (h, (w + 1) // 2)).astype(np.uint16)
    n = h422.groups(w)
    for plane in (h422.v210_pack(y, cb, cr), h422.v210_pack(y, cb, cr, junk=rng.integers(0, 4, (h, 4 * n)), beyond=rng.integers(0, 1024, (h, 6 * n)))):
        assert plane.shape == (h, 4 * n) and plane.dtype == np.uint32
        y2, cb2, cr2 = h422.v210_unpack(plane, w)
        assert np.array_equal(y2, y) and np.array_equal(cb2, cb) and np.array_equal(cr2, cr)
    # the layout itself, spelled out for one group: d0 = Cb0 Y0 Cr0 | d1 = Y1 Cb1 Y2 | d2 = Cr1 Y3 Cb2 | d3 = Y4 Cr2 Y5
    yy, cbb, crr = np.array([[1, 2, 3, 4, 5, 6]]), np.array([[11, 12, 13]]), np.array([[21, 22, 23]])
    d = h422.v210_pack(yy, cbb, crr)[0]
    assert [int(x) for x in d] == [11 | 1 << 10 | 21 << 20, 2 | 12 << 10 | 3 << 20, 22 | 4 << 10 | 13 << 20, 5 | 23 << 10 | 6 << 20]


@pytest.mark.parametrize("w,h", [(1, 1), (2, 2), (6, 1), (7, 5), (37, 21), (260, 3)])
def test_the_general_v210_fetch_finds_every_pixels_codes(emu, w, h):
    """cv210_pixel_codes (k_yuv422_hi_to_rgba_any's fetch) at any width: pixel x gets Y[x] and the chroma of pair x / 2, whatever bits 30 - 31 and
    the components beyond w hold."""
    rng = _seed(w, h, "fetch")
    y = rng.integers(0, 1024, (h, w)).astype(np.uint16)
    cb, cr = rng.integers(0, 1024, (h, (w + 1) // 2)).astype(np.uint16), rng.integers(0, 1024, (h, (w + 1) // 2)).astype(np.uint16)
    n = h422.groups(w)
    plane = h422.v210_pack(y, cb, cr, junk=rng.integers(0, 4, (h, 4 * n)), beyond=rng.integers(0, 1024, (h, 6 * n)))
    out = np.zeros((h, w, 3), np.uint16)
    assert emu.emu_v210_pixel_codes(_p(plane.view(np.uint8)), w, h, out.ctypes.data_as(C.POINTER(C.c_uint16))) == 0
    pair = np.arange(w) // 2
    assert np.array_equal(out[..., 0], y) and np.array_equal(out[..., 1], cb[:, pair]) and np.array_equal(out[..., 2], cr[:, pair])


@pytest.mark.parametrize("w,h", [(8, 2), (12, 2), (20, 4), (132, 74), (260, 10)])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_ignored_bits_change_nothing(emu, w, h, layout):
    """v210 bits 30 - 31 and the components beyond w in the last group, the six other bits of P210 and planar words, all random: the bytes of
    the frame with those bits clear (the mask or shift comes before any table lookup: no word indexes outside a table)."""
    rng = _seed(w, h, layout, "junk")
    y, c = _content10("noise", w, h, rng)
    for rgb12 in (0, 1):
        clean = _run(emu, layout, y, c, rgb12)
        got = _run(emu, layout, y, c, rgb12, junk=np.random.default_rng(w + h))
        assert np.array_equal(got, clean), (layout, w, h, rgb12, _diff(got, clean))
    assert np.array_equal(clean, _witness(layout, y, c))
    if layout == "v210":  # every ignored bit set
        n = h422.groups(w)
        plane = h422.v210_pack(y, c[..., 0], c[..., 1], junk=np.full((h, 4 * n), 3), beyond=np.full((h, 6 * n), 1023))
        out = np.zeros((h, w, 4), np.uint8)
        b = plane.view(np.uint8)
        assert emu.emu_convert_hi422_run(_p(b), _p(b), _p(b), w, h, 2, 0, 1, _p(out)) == 0
        assert np.array_equal(out, clean)


SHARE_SIZES = [(264, 38), (8, 2), (516, 26), (64, 130), (20, 6)]
SHARE_RGB12 = [1, 0, 0, 1, 0]


def _shares(emu, layout, waves, sizes, rgb12, contents):
    keep, ys, us, vs, outs = [], [], [], [], []
    for (w, h), r12, (y, c) in zip(sizes, rgb12, contents):
        py, pu, pv = _planes(layout, y, c)
        keep.append((py, pu, pv))
        ys.append(py); us.append(pu); vs.append(pv)
        outs.append(np.zeros((h, 3 * w), np.uint8) if r12 else np.zeros((h, w, 4), np.uint8))
    n = len(sizes)
    arr = lambda xs: (P8 * n)(*[_p(x) for x in xs])
    ints = lambda xs: (C.c_int * n)(*xs)
    assert emu.emu_convert_hi422_shares(n, arr(ys), arr(us), arr(vs), ints([s[0] for s in sizes]), ints([s[1] for s in sizes]), LAYOUT_ID[layout],
                                        ints(rgb12), waves, arr(outs)) == 0
    return [hdm.rgb12_rows_to_rgba(o, w, h) if r12 else o for (w, h), r12, o in zip(sizes, rgb12, outs)]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("waves", [1, 3, 8])
def test_a_launch_cut_into_equal_shares_writes_each_jobs_own_bytes(emu, layout, waves):
    """k_yuv422_hi_to_rgba's partition (cv_plan + cv422_share): five frames of different sizes and node formats in one launch of `waves`
    workgroups — every byte of every frame what the job gives alone, and the witness's (a unit missed or doubled would show)."""
    rng = np.random.default_rng(17 * waves + LAYOUT_ID[layout])
    contents = [_content10("noise", w, h, rng) for w, h in SHARE_SIZES]
    together = _shares(emu, layout, waves, SHARE_SIZES, SHARE_RGB12, contents)
    for (w, h), r12, (y, c), got in zip(SHARE_SIZES, SHARE_RGB12, contents, together):
        alone = _run(emu, layout, y, c, r12)
        assert np.array_equal(got, alone), (layout, w, h, waves, _diff(got, alone))
        assert np.array_equal(got, _witness(layout, y, c)), (layout, w, h, waves)


def guard_run():
    """The child of test_converter_never_leaves_its_planes (SMR_EMU_GUARD, SMR_EMU_PITCH set): every layout and node format at GUARD_SIZES, runs of
    one and two blocks, junk bits included, and one launch cut into shares — against the witness, with every plane exactly pitch * h bytes."""
    emu = _emu()
    for layout in LAYOUTS:
        for w, h in GUARD_SIZES:
            rng = _seed(w, h, layout, "guard")
            y, c = _content10("noise", w, h, rng)
            want = _witness(layout, y, c)
            for rgb12 in (0, 1):
                for nb in (1, 2):
                    assert np.array_equal(_run(emu, layout, y, c, rgb12, nb=nb), want), (layout, w, h, rgb12, nb)
                assert np.array_equal(_run(emu, layout, y, c, rgb12, junk=np.random.default_rng(1)), want), (layout, w, h, rgb12, "junk")
        sizes, rgb12 = GUARD_SIZES + [(20, 6)], [1, 0, 1, 0]
        contents = [_content10("noise", w, h, np.random.default_rng(w)) for w, h in sizes]
        for got, (y, c) in zip(_shares(emu, layout, 3, sizes, rgb12, contents), contents):
            assert np.array_equal(got, _witness(layout, y, c)), (layout, "shares")
    print("guard run passed")


@pytest.mark.parametrize("pitch", ["tight", "wide"])
@pytest.mark.parametrize("mode", [1, 2, 3])
def test_converter_never_leaves_its_planes(emu, mode, pitch):
    """ONE memory contract (include/smr.h, smr_surface_wrap): guard_run in a child process with every plane and node texture exactly pitch * h
    bytes — on the SMALLEST pitch conv_route lets through, the row's own bytes (tight), and on wide ones (256-byte rows; v210: a capture
    card's stride) — ending at (mode 1) or starting behind (mode 2) an unmapped page: a load or store outside a plane kills the child,
    prefetches included.  Mode 3 is the WRITE half (tests/emu/emu_guard.h): node textures on the smallest pitch + 32, pre-filled from a seeded
    pattern, the row padding compared after."""
    env = dict(os.environ, SMR_EMU_GUARD=str(mode), SMR_EMU_PITCH=pitch)
    r = subprocess.run([sys.executable, "-c", "from tests import test_emu_convert_hi422 as t; t.guard_run()"], capture_output=True, text=True, env=env,
                       cwd=ROOT, timeout=600)
    assert r.returncode == 0, f"guard mode {mode}, {pitch}: rc {r.returncode} (-11 = a kernel left its planes; 'write footprint' = it wrote row padding)\n{r.stdout[-3000:]}\n{r.stderr[-2000:]}"
    assert "guard run passed" in r.stdout
