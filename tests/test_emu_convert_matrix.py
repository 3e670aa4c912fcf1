"""The block converters' own source per colour matrix (tests/emu/emu_convert_matrix.cpp: cv420_run / cv420_share with the matrix as a template
argument, the 10-bit converters with it in the job) against tests/color_matrix_model.py, byte for byte, without a GPU."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import color_matrix_model as cm
from tests.emu_build import CLANG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P8 = C.POINTER(C.c_uint8)
SIZES = [(8, 2), (12, 4), (64, 36), (132, 74), (260, 10)]
GUARD_SIZES = [(8, 2), (12, 4), (260, 10)]
MATRICES = [cm.BT601, cm.BT2020_NCL]
# variant -> (harness kind, base format, full range)
VARIANTS = {"420": (0, cm.PLANAR_YUV420, 0), "j420": (0, cm.PLANAR_YUVJ420, 1), "nv12": (1, cm.NV12, 0), "420p10": (2, cm.PLANAR_YUV420P10, 0),
            "p010": (3, cm.P010, 0), "422p10": (4, cm.PLANAR_YUV422P10, 0), "p210": (5, cm.P210, 0), "v210": (6, cm.V210, 0)}
Y8 = np.array([0, 1, 15, 16, 17, 234, 235, 236, 254, 255])  # tests/test_emu_convert.py's `extremes`
C8 = np.array([0, 15, 16, 17, 127, 128, 129, 239, 240, 241, 255])
X10 = np.array([0, 1, 63, 64, 65, 66, 67, 68, 511, 512, 513, 939, 940, 941, 959, 960, 961, 1022, 1023])  # tests/test_emu_convert_hi.py's
_HANDLE = None


def _emu():
    global _HANDLE
    if _HANDLE is None:
        from tests import emu_build
        lib = emu_build.build("smr_emu_convert_matrix", "emu_convert_matrix.cpp",
                              ("smr_convert_hi422.h", "smr_convert_hi.h", "smr_convert_420.h", "smr_convert_batch.h", "smr_convert_dev.h", "smr_yuv_fast.h", "smr_frame_formats.h"))
        h = C.CDLL(lib)
        i = C.c_int
        h.emu_cm_run.argtypes = [P8, P8, P8, i, i, i, i, i, i, i, i, P8]
        PP8, PI = C.POINTER(P8), C.POINTER(C.c_int)
        h.emu_cm_shares.argtypes = [i, PP8, PP8, PP8, PI, PI, i, PI, PI, i, i, i, PP8]
        h.emu_cm_coefficients.argtypes = [C.POINTER(C.c_float)]
        if os.environ.get("SMR_EMU_GUARD"):  # the child of test_converters_never_leave_their_planes
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


def _planes(variant, w, h, kind, seed):
    fmt = VARIANTS[variant][1]
    if kind == "noise":
        return cm.noise_planes(fmt, w, h, seed)
    rng = np.random.default_rng(seed)
    ch = cm.chroma_shape(fmt, w, h)
    if cm.is_hi(fmt):
        return cm.planes_of(fmt, rng.choice(X10, (h, w)), rng.choice(X10, ch), rng.choice(X10, ch))
    return cm.planes_of(fmt, rng.choice(Y8, (h, w)), rng.choice(C8, ch), rng.choice(C8, ch))


def _witness(variant, w, h, planes, matrix, rgb12):
    node = cm.node_rgba(VARIANTS[variant][1], w, h, planes, matrix)
    return cm.rgb12_rows(node) if rgb12 else node


def _three(planes):
    p = [np.ascontiguousarray(a) for a in planes]
    return p + [p[-1]] * (3 - len(p))  # (the harness ignores what a kind does not have)


def _run(emu, variant, w, h, planes, matrix, rgb12, nb=1, tight=0):
    kind, _, full = VARIANTS[variant]
    out = np.zeros((h, 3 * w) if rgb12 else (h, w, 4), np.uint8)
    p = _three(planes)
    rc = emu.emu_cm_run(_p(p[0]), _p(p[1]), _p(p[2]), w, h, kind, full, rgb12, nb, matrix, tight, _p(out))
    assert rc == 0, (variant, w, h, rc)
    return out


def _shares(emu, variant, sizes, contents, matrix, rgb12s, waves, tight=0, fulls=None):
    kind = VARIANTS[variant][0]
    n = len(sizes)
    keep = [_three(c) for c in contents]
    outs = [np.zeros((h, 3 * w) if r else (h, w, 4), np.uint8) for (w, h), r in zip(sizes, rgb12s)]
    arr = lambda k: (P8 * n)(*[_p(q[k]) for q in keep])  # noqa: E731
    ints = lambda v: (C.c_int * n)(*v)  # noqa: E731
    fulls = fulls or [VARIANTS[variant][2]] * n
    rc = emu.emu_cm_shares(n, arr(0), arr(1), arr(2), ints([s[0] for s in sizes]), ints([s[1] for s in sizes]), kind, ints(fulls), ints(rgb12s), waves, matrix,
                           tight, (P8 * n)(*[_p(o) for o in outs]))
    assert rc == 0, (variant, rc)
    return outs


def test_compiled_table_is_the_witness_table(emu):
    got = (C.c_float * 12)()
    emu.emu_cm_coefficients(got)
    want = np.array([cm.COEF[m] for m in (cm.BT709, cm.BT601, cm.BT2020_NCL)], np.float32).reshape(-1)
    assert np.array_equal(np.array(got[:], np.float32), want)


@pytest.mark.parametrize("kind", ["noise", "extremes"])
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("matrix", MATRICES)
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_block_converters_are_the_witness_byte_for_byte(emu, variant, matrix, w, h, kind):
    seed = ((list(VARIANTS).index(variant) * 1000 + w) * 1000 + h) * 2 + ["noise", "extremes"].index(kind)  # (integers only: the same content in every run)
    planes = _planes(variant, w, h, kind, seed)
    for rgb12 in (0, 1):
        want = _witness(variant, w, h, planes, matrix, rgb12)
        for nb in (1, 3):
            got = _run(emu, variant, w, h, planes, matrix, rgb12, nb=nb)
            assert np.array_equal(got, want), (variant, cm.NAMES[matrix], w, h, kind, rgb12, nb, int(np.abs(got.astype(int) - want.astype(int)).max()))
        if VARIANTS[variant][0] <= 1:  # the _tight build
            got = _run(emu, variant, w, h, planes, matrix, rgb12, nb=2, tight=1)
            assert np.array_equal(got, want), (variant, cm.NAMES[matrix], w, h, kind, rgb12, "tight")


def test_bt709_argument_is_the_default_instantiation(emu):
    """matrix 0 through the new harness = the witness at BT.709 (which is the oracle: tests/test_color_matrix_model.py)"""
    for variant in VARIANTS:
        planes = _planes(variant, 20, 6, "noise", 7)
        assert np.array_equal(_run(emu, variant, 20, 6, planes, cm.BT709, 0), _witness(variant, 20, 6, planes, cm.BT709, 0)), variant


MIXED = [(132, 74), (8, 2), (260, 10), (64, 36), (12, 4)]


@pytest.mark.parametrize("waves", [1, 3, 16])
@pytest.mark.parametrize("matrix", MATRICES)
@pytest.mark.parametrize("variant", [v for v in VARIANTS if v != "j420"])
def test_multi_job_launch_of_mixed_sizes(emu, variant, matrix, waves):
    """Five frames of mixed sizes and node formats in one launch, cut by the host's own cv_plan; planar 4:2:0 mixes both ranges."""
    contents = [_planes(variant, w, h, "noise", 100 + i) for i, (w, h) in enumerate(MIXED)]
    rgb12s = [1, 0, 1, 0, 1]
    fulls = [0, 1, 0, 1, 0] if variant == "420" else None
    outs = _shares(emu, variant, MIXED, contents, matrix, rgb12s, waves, fulls=fulls)
    for i, ((w, h), c, r, got) in enumerate(zip(MIXED, contents, rgb12s, outs)):
        fmt = cm.PLANAR_YUVJ420 if fulls and fulls[i] else VARIANTS[variant][1]
        node = cm.node_rgba(fmt, w, h, c, matrix)
        want = cm.rgb12_rows(node) if r else node
        assert np.array_equal(got, want), (variant, cm.NAMES[matrix], waves, i)


def guard_run():
    """The child of test_converters_never_leave_their_planes (SMR_EMU_GUARD, SMR_EMU_PITCH set): every variant, matrix and node format at
    GUARD_SIZES, and one launch cut into shares — against the witness, with every plane exactly pitch * h bytes."""
    emu = _emu()
    for variant in VARIANTS:
        for matrix in MATRICES:
            for w, h in GUARD_SIZES:
                planes = _planes(variant, w, h, "noise", w * 131 + h)
                for rgb12 in (0, 1):
                    want = _witness(variant, w, h, planes, matrix, rgb12)
                    assert np.array_equal(_run(emu, variant, w, h, planes, matrix, rgb12, nb=2), want), (variant, matrix, w, h, rgb12)
                    if VARIANTS[variant][0] <= 1:
                        assert np.array_equal(_run(emu, variant, w, h, planes, matrix, rgb12, nb=1, tight=1), want), (variant, matrix, w, h, rgb12, "tight")
            sizes, rgb12s = GUARD_SIZES + [(20, 6)], [1, 0, 1, 0]
            contents = [_planes(variant, w, h, "noise", w) for w, h in sizes]
            for got, (w, h), c, r in zip(_shares(emu, variant, sizes, contents, matrix, rgb12s, 3), sizes, contents, rgb12s):
                assert np.array_equal(got, _witness(variant, w, h, c, matrix, r)), (variant, matrix, "shares")
    print("guard run passed")


@pytest.mark.parametrize("pitch", ["tight", "wide"])
@pytest.mark.parametrize("mode", [1, 2, 3])
def test_converters_never_leave_their_planes(emu, mode, pitch):
    """The existing harnesses' guard modes (tests/emu/emu_guard.h) on the per-matrix builds: planes and node textures of exactly pitch * h bytes
    ending at (1) or starting behind (2) an unmapped page; 3 compares the node rows' padding after the run."""
    env = dict(os.environ, SMR_EMU_GUARD=str(mode), SMR_EMU_PITCH=pitch)
    r = subprocess.run([sys.executable, "-c", "from tests import test_emu_convert_matrix as t; t.guard_run()"], capture_output=True, text=True, env=env,
                       cwd=ROOT, timeout=600)
    assert r.returncode == 0, f"guard mode {mode}, {pitch}: rc {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-2000:]}"
    assert "guard run passed" in r.stdout
