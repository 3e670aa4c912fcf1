"""The 10-bit 4:2:0 input converter (smelter_amd/csrc/smr_convert_hi.h, k_yuv420_hi_to_rgba's per-thread runs of 4 x 4 blocks) compiled for
the CPU by tests/emu/emu_convert_hi.cpp.  EVERY BYTE EQUAL, twice:

  * content whose 10-bit codes are 4 b against the ORACLE's planar_yuv_to_rgba / nv12_to_rgba of the bytes b (the value rule of
    include/smr.h makes the 8-bit reference apply unchanged);
  * true 10-bit content against tests/hi_depth_model.py, the numpy restatement of the oracle's sequence — itself held to the oracle on
    4 b content here.

Test infrastructure only: the product has no CPU path; tests/test_gpu_hi_depth.py holds the kernels themselves on the device."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as orc
from tests import hi_depth_model as hdm

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
P8 = C.POINTER(C.c_uint8)
SIZES = [(8, 2), (8, 6), (12, 4), (64, 36), (132, 74), (256, 18), (1920, 16)]
EXTREMES = np.array([0, 1, 63, 64, 65, 66, 67, 68, 511, 512, 513, 939, 940, 941, 959, 960, 961, 1022, 1023], np.uint16)


@pytest.fixture(scope="module")
def emu():
    if not os.path.exists(CLANG):
        pytest.skip("no clang++ to build the emulator with")
    from tests import emu_build
    lib = emu_build.build("smr_emu_convert_hi", "emu_convert_hi.cpp", ("smr_convert_hi.h", "smr_convert_420.h", "smr_convert_batch.h", "smr_convert_dev.h", "smr_yuv_fast.h"))
    h = C.CDLL(lib)
    h.emu_convert_hi_run.argtypes = [P8, P8, P8, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, P8]
    PP8, PI = C.POINTER(P8), C.POINTER(C.c_int)
    h.emu_convert_hi_shares.argtypes = [C.c_int, PP8, PP8, PP8, PI, PI, C.c_int, PI, C.c_int, PP8]
    PF = C.POINTER(C.c_float)
    h.emu_convert_hi_tables.argtypes = [PF, PF]
    h.emu_convert_hi_tables.restype = None
    orc.build()
    if os.environ.get("SMR_EMU_GUARD"):  # the inner run of test_converter_never_leaves_its_planes: planes of exactly pitch * h bytes against an unmapped page
        h.emu_set_guard(int(os.environ["SMR_EMU_GUARD"]), 1)
    return h


def _p(a):
    return a.ctypes.data_as(P8)


def _content8(kind, w, h, rng):
    """tests/test_emu_convert.py's contents: (y bytes (h, w), chroma byte pairs (h/2, w/2, 2))."""
    cw, ch = w // 2, h // 2
    if kind == "noise":
        return rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (ch, cw, 2), dtype=np.uint8)
    if kind == "extremes":  # the range clamps' corners and their neighbours
        return (rng.choice(np.array([0, 1, 15, 16, 17, 234, 235, 236, 254, 255], np.uint8), (h, w)),
                rng.choice(np.array([0, 15, 16, 17, 127, 128, 129, 239, 240, 241, 255], np.uint8), (ch, cw, 2)))
    xx, yy = np.meshgrid(np.arange(w), np.arange(h))  # camera-like: smooth luma, slow chroma
    y = (16 + (xx * 3 + yy * 2) % 200 + rng.integers(0, 8, (h, w))).astype(np.uint8)
    c = np.stack([(100 + (np.arange(cw)[None, :] + np.arange(ch)[:, None]) % 60), (140 - (np.arange(cw)[None, :] * 2 + np.arange(ch)[:, None]) % 70)], -1).astype(np.uint8)
    return y, c


def _content10(kind, w, h, rng):
    """True 10-bit codes: (y (h, w), chroma pairs (h/2, w/2, 2)), uint16."""
    cw, ch = w // 2, h // 2
    if kind == "noise":
        return rng.integers(0, 1024, (h, w)).astype(np.uint16), rng.integers(0, 1024, (ch, cw, 2)).astype(np.uint16)
    return rng.choice(EXTREMES, (h, w)), rng.choice(EXTREMES, (ch, cw, 2))


def _words(codes, p010, junk=None):
    """Codes -> the format's 16-bit words; junk: the six ignored bits (low ones for P010, high ones for planar), zero by default."""
    codes = np.asarray(codes, np.uint16)
    j = np.zeros_like(codes) if junk is None else np.asarray(junk, np.uint16) & 0x3F
    return np.ascontiguousarray((codes << 6) | j if p010 else codes | (j << 10))


def _run(emu, y, c, w, h, p010, rgb12, nb=1, junk=None):
    """The emulated converter on codes y, c (chroma pairs) -> (h, w, 4) RGBA8 (an RGB12 node unpacked, alpha 255)."""
    jy, jc = (None, None) if junk is None else junk
    yw, cwords = _words(y, p010, jy), _words(c, p010, jc)
    if p010:
        u = v = cwords
    else:
        u, v = np.ascontiguousarray(cwords[..., 0]), np.ascontiguousarray(cwords[..., 1])
    out = np.zeros((h, 3 * w), np.uint8) if rgb12 else np.zeros((h, w, 4), np.uint8)
    rc = emu.emu_convert_hi_run(_p(yw.view(np.uint8)), _p(u.view(np.uint8)), _p(v.view(np.uint8)), w, h, 1 if p010 else 0, 1 if rgb12 else 0, nb, _p(out))
    assert rc == 0, rc
    return hdm.rgb12_rows_to_rgba(out, w, h) if rgb12 else out


def _oracle8(y, c, w, h, p010):
    if p010:
        return orc.nv12_to_rgba(y, np.ascontiguousarray(c), w, h)
    return orc.planar_yuv_to_rgba(y, np.ascontiguousarray(c[..., 0]), np.ascontiguousarray(c[..., 1]), w, h, orc.YUV420)


def _diff(got, want):
    return int((got != want).sum()), np.argwhere(got != want)[:4].tolist()


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("fmt", ["p010", "planar"])
@pytest.mark.parametrize("kind", ["noise", "extremes", "camera"])
def test_codes_4b_give_the_oracles_bytes_of_b(emu, w, h, fmt, kind):
    """A 10-bit frame whose codes are 4 b has the node texture, byte for byte, of the 8-bit frame with bytes b — RGBA8 and RGB12 — and the
    witness agrees with the oracle there too."""
    rng = np.random.default_rng(hash((w, h, fmt, kind)) % 2**32)
    p010 = fmt == "p010"
    y, c = _content8(kind, w, h, rng)
    want = _oracle8(y, c, w, h, p010)
    y10, c10 = y.astype(np.uint16) * 4, c.astype(np.uint16) * 4
    assert np.array_equal(hdm.node_rgba(y10, c10[..., 0], c10[..., 1]), want), "the witness is not the oracle on 4 b content"
    for rgb12 in (0, 1):
        got = _run(emu, y10, c10, w, h, p010, rgb12)
        assert np.array_equal(got, want), (fmt, kind, w, h, rgb12, _diff(got, want))


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("fmt", ["p010", "planar"])
@pytest.mark.parametrize("kind", ["noise", "extremes"])
def test_true_10_bit_content_is_the_witness_byte_for_byte(emu, w, h, fmt, kind):
    rng = np.random.default_rng(hash((w, h, fmt, kind, 10)) % 2**32)
    p010 = fmt == "p010"
    y, c = _content10(kind, w, h, rng)
    want = hdm.node_rgba(y, c[..., 0], c[..., 1])
    for rgb12 in (0, 1):
        got = _run(emu, y, c, w, h, p010, rgb12)
        assert np.array_equal(got, want), (fmt, kind, w, h, rgb12, _diff(got, want))


def test_the_tables_are_the_operations_themselves(emu):
    """The two 1024-entry tables the kernel builds: the code's unorm value is the IEEE quotient (c / 4) / 255, its luma range expansion
    (Markstein's corrected quotient) is the IEEE division of the oracle, clamped — for every code."""
    ylut, ulut = np.zeros(1024, np.float32), np.zeros(1024, np.float32)
    PF = C.POINTER(C.c_float)
    emu.emu_convert_hi_tables(ylut.ctypes.data_as(PF), ulut.ctypes.data_as(PF))
    codes = np.arange(1024)
    u = hdm.unorm_of_code(codes)
    assert np.array_equal(ulut.view(np.uint32), u.view(np.uint32))
    want = hdm._clamp01((u - np.float32(16.0) / np.float32(255.0)) / np.float32(0.85882352941))
    assert np.array_equal(ylut, want)  # (values: a clamp may give +0 where the kernel's median keeps -0; the sums that follow absorb it)


@pytest.mark.parametrize("fmt", ["p010", "planar"])
def test_every_luma_code_against_a_sweep_of_flat_chroma(emu, fmt):
    """All 1024 luma codes against flat chroma patches (dense in Cb, the clamps' corners in Cr): every byte the witness's."""
    w, h = 1024, 2
    p010 = fmt == "p010"
    y = np.tile(np.arange(1024, dtype=np.uint16), (h, 1))
    for cu in list(range(0, 1024, 41)) + [63, 64, 65, 959, 960, 961, 1023]:
        for cv in (0, 64, 67, 309, 512, 515, 805, 960, 1023):
            c = np.empty((h // 2, w // 2, 2), np.uint16)
            c[..., 0], c[..., 1] = cu, cv
            want = hdm.node_rgba(y, c[..., 0], c[..., 1])
            got = _run(emu, y, c, w, h, p010, 0)
            assert np.array_equal(got, want), (fmt, cu, cv, _diff(got, want))


@pytest.mark.parametrize("w,h", [(8, 2), (12, 4), (132, 74), (256, 18)])
@pytest.mark.parametrize("fmt", ["p010", "planar"])
def test_the_six_other_bits_of_a_word_are_ignored(emu, w, h, fmt):
    """P010 with random low six bits, planar with random high six bits: the bytes of the frame with those bits clear (the mask or shift comes
    before any table lookup: no word indexes outside a table)."""
    rng = np.random.default_rng(hash((w, h, fmt, "junk")) % 2**32)
    p010 = fmt == "p010"
    y, c = _content10("noise", w, h, rng)
    junk = (rng.integers(0, 64, y.shape), rng.integers(0, 64, c.shape))
    junk[0][0, 0] = 63; junk[1][0, 0] = 63
    for rgb12 in (0, 1):
        clean = _run(emu, y, c, w, h, p010, rgb12)
        got = _run(emu, y, c, w, h, p010, rgb12, junk=junk)
        assert np.array_equal(got, clean), (fmt, w, h, rgb12, _diff(got, clean))
    assert np.array_equal(clean, hdm.node_rgba(y, c[..., 0], c[..., 1]))


@pytest.mark.parametrize("w,h", [(8, 2), (8, 6), (12, 4), (64, 36), (132, 74), (256, 130), (1920, 22)])
@pytest.mark.parametrize("fmt", ["p010", "planar"])
@pytest.mark.parametrize("nb", [1, 2, 3, 4, 7])
def test_runs_of_blocks_equal_the_witness_byte_for_byte(emu, w, h, fmt, nb):
    """cvhi_run — what a wave of k_yuv420_hi_to_rgba executes — writes the witness's bytes whatever the run length, at every frame height (runs
    that end inside a block, heights of 2 mod 4), RGBA8 and RGB12."""
    rng = np.random.default_rng(hash((w, h, fmt, nb)) % 2**32)
    p010 = fmt == "p010"
    y, c = _content10("noise", w, h, rng)
    want = hdm.node_rgba(y, c[..., 0], c[..., 1])
    for rgb12 in (0, 1):
        got = _run(emu, y, c, w, h, p010, rgb12, nb=nb)
        assert np.array_equal(got, want), (fmt, nb, w, h, rgb12, _diff(got, want))


@pytest.mark.parametrize("fmt", ["p010", "planar"])
@pytest.mark.parametrize("waves", [1, 3, 8, 9, 13, 64, 1000])
def test_a_launch_cut_into_equal_shares_writes_the_witnesss_bytes(emu, fmt, waves):
    """k_yuv420_hi_to_rgba's partition (cv_plan + cvhi_share): five frames of different sizes and node formats in one launch of `waves`
    workgroups — every byte of every frame the witness's (a unit missed or doubled would show)."""
    p010 = fmt == "p010"
    rng = np.random.default_rng(17 * waves + p010)
    sizes = [(264, 38), (8, 2), (516, 26), (64, 130), (20, 6)]
    rgb12 = [1, 0, 0, 1, 0]
    ys, us, vs, outs, wants = [], [], [], [], []
    for (w, h), r12 in zip(sizes, rgb12):
        y, c = _content10("noise", w, h, rng)
        wants.append(hdm.node_rgba(y, c[..., 0], c[..., 1]))
        cwords = _words(c, p010)
        ys.append(_words(y, p010).view(np.uint8))
        us.append((cwords if p010 else np.ascontiguousarray(cwords[..., 0])).view(np.uint8))
        vs.append((cwords if p010 else np.ascontiguousarray(cwords[..., 1])).view(np.uint8))
        outs.append(np.zeros((h, 3 * w), np.uint8) if r12 else np.zeros((h, w, 4), np.uint8))
    n = len(sizes)
    arr = lambda xs: (P8 * n)(*[_p(x) for x in xs])
    ints = lambda xs: (C.c_int * n)(*xs)
    assert emu.emu_convert_hi_shares(n, arr(ys), arr(us), arr(vs), ints([s[0] for s in sizes]), ints([s[1] for s in sizes]), 1 if p010 else 0,
                                     ints(rgb12), waves, arr(outs)) == 0
    for (w, h), r12, got, want in zip(sizes, rgb12, outs, wants):
        if r12:
            got = hdm.rgb12_rows_to_rgba(got, w, h)
        assert np.array_equal(got, want), (w, h, waves, _diff(got, want))


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_converter_never_leaves_its_planes(emu, mode):
    """ONE memory contract (include/smr.h, smr_surface_wrap): the tests above once more in a child process with every plane and node texture
    exactly pitch * h bytes on the SMALLEST pitch conv_route lets through — the row's own bytes — ending at (mode 1) or starting behind
    (mode 2) an unmapped page: a load or store outside a plane kills the child, prefetches included.  Mode 3 is the WRITE half
    (tests/emu/emu_guard.h): node textures on the smallest pitch + 32, pre-filled from a seeded pattern, the row padding compared after."""
    if os.environ.get("SMR_EMU_GUARD"):
        pytest.skip("this is the inner run")
    env = dict(os.environ, SMR_EMU_GUARD=str(mode))
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-p", "no:cacheprovider", "-k",
                        "codes_4b or true_10_bit or other_bits or runs_of_blocks or equal_shares"], capture_output=True, text=True, env=env, cwd=ROOT, timeout=1200)
    assert r.returncode == 0, f"guard mode {mode}: rc {r.returncode} (-11 = a kernel left its planes; 'write footprint' = it wrote row padding)\n{r.stdout[-3000:]}\n{r.stderr[-2000:]}"
    assert " passed" in r.stdout
