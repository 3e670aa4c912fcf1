"""tests/color_matrix_model.py — the witness of the input colour matrices — held to the oracle at BT.709 byte for byte (everything the three
matrices share), anchored per matrix to the 100 % colour bars computed from (Kr, Kb) in float64, and the enum's values in include/smr.h,
smelter_amd/hip.py and the Rust patch held to each other.  No GPU."""
import os
import re

import numpy as np
import pytest

from oracle import oracle as orc
from tests import color_matrix_model as cm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(8, 2), (12, 4), (7, 5), (37, 21), (132, 74)]
MATRICES = [cm.BT709, cm.BT601, cm.BT2020_NCL]
Y_EXTREMES = np.array([0, 1, 15, 16, 17, 234, 235, 236, 254, 255], np.uint8)  # tests/test_emu_convert.py's `extremes`: the range clamps' corners
C_EXTREMES = np.array([0, 15, 16, 17, 127, 128, 129, 239, 240, 241, 255], np.uint8)


@pytest.fixture(scope="module", autouse=True)
def _oracle():
    orc.build()


def _bytes(kind, shape, rng, chroma):
    if kind == "extremes":
        return rng.choice(C_EXTREMES if chroma else Y_EXTREMES, shape)
    return rng.integers(0, 256, shape, dtype=np.uint8)


def _frame8(fmt, w, h, kind, seed):
    """Bytes of an 8-bit frame: y (h, w), chroma planes of the format's shape (the interleaved formats: the (h, w // 2, 4) plane itself)."""
    rng = np.random.default_rng(seed)
    if fmt in (cm.UYVY422, cm.YUYV422):
        plane = np.empty((h, max(w // 2, 1), 4), np.uint8)
        luma = (1, 3) if fmt == cm.UYVY422 else (0, 2)
        for k in range(4):
            plane[..., k] = _bytes(kind, plane.shape[:2], rng, k not in luma)
        return [plane]
    ch = cm.chroma_shape(fmt, w, h)
    return [_bytes(kind, (h, w), rng, False), _bytes(kind, ch, rng, True), _bytes(kind, ch, rng, True)]


def _oracle_node(fmt, w, h, p):
    """The oracle's node texture of the 8-bit frame whose bytes are p (the 10-bit formats: of their 8-bit twin)."""
    if fmt in (cm.UYVY422, cm.YUYV422, cm.V210):
        return orc.interleaved422_to_rgba(p[0], w, h, 1 if fmt == cm.YUYV422 else 0)
    if fmt in (cm.NV12, cm.P010):
        return orc.nv12_to_rgba(p[0], np.ascontiguousarray(np.stack([p[1], p[2]], -1)), w, h)
    variant = {cm.PLANAR_YUV420: orc.YUV420, cm.PLANAR_YUVJ420: orc.YUVJ420, cm.PLANAR_YUV422: orc.YUV422, cm.PLANAR_YUV444: orc.YUV444,
               cm.PLANAR_YUV420P10: orc.YUV420, cm.PLANAR_YUV422P10: orc.YUV422, cm.P210: orc.YUV422}[fmt]
    return orc.planar_yuv_to_rgba(p[0], p[1], p[2], w, h, variant)


@pytest.mark.parametrize("kind", ["noise", "extremes"])
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("fmt", cm.YCBCR_FORMATS)
def test_witness_at_bt709_is_the_oracle_byte_for_byte(fmt, w, h, kind):
    """Everything the three matrices share — fetch, chroma sample, code rule, range step, store — is the oracle's.  The 10-bit formats carry
    codes 4 b, as tests/test_emu_convert_hi.py's do: their node is the 8-bit twin's."""
    seed = ((fmt * 1000 + w) * 1000 + h) * 2 + ["noise", "extremes"].index(kind)  # (integers only: the same content in every run)
    if fmt == cm.V210 and (w % 2 or w < 8):
        # v210's rule is UYVY's for even widths from 8 up (include/smr.h); elsewhere UYVY has no such frame, and the BT.709 reference is the
        # v210 witness the 4:2:2 work is held to (tests/hi422_model.py)
        from tests import hi422_model as h422
        rng = np.random.default_rng(seed)
        y, cb, cr = (_bytes(kind, s_, rng, c).astype(np.uint16) * 4 for s_, c in (((h, w), False), ((h, (w + 1) // 2), True), ((h, (w + 1) // 2), True)))
        planes = cm.planes_of(cm.V210, y, cb, cr)
        want = h422.node_rgba_v210(y, cb, cr)
    elif fmt == cm.V210:  # the UYVY twin: pair chroma
        p8 = _frame8(cm.UYVY422, w, h, kind, seed)
        y = np.stack([p8[0][..., 1], p8[0][..., 3]], -1).reshape(h, w)
        planes = cm.planes_of(cm.V210, y.astype(np.uint16) * 4, p8[0][..., 0].astype(np.uint16) * 4, p8[0][..., 2].astype(np.uint16) * 4)
        want = _oracle_node(fmt, w, h, p8)
    else:
        p8 = _frame8(fmt, w, h, kind, seed)
        if fmt in (cm.UYVY422, cm.YUYV422):
            planes = p8
        else:
            s = 4 if cm.is_hi(fmt) else 1
            planes = cm.planes_of(fmt, p8[0].astype(np.uint16) * s, p8[1].astype(np.uint16) * s, p8[2].astype(np.uint16) * s)
        want = _oracle_node(fmt, w, h, p8)
    got = cm.node_rgba(fmt, w, h, planes, cm.BT709)
    assert np.array_equal(got, want), (fmt, w, h, kind, int(np.abs(got.astype(int) - want.astype(int)).max()))


@pytest.mark.parametrize("matrix", MATRICES)
@pytest.mark.parametrize("fmt", [f for f in cm.YCBCR_FORMATS if f != cm.PLANAR_YUVJ420])
def test_witness_reproduces_the_colour_bars(fmt, matrix):
    """The witness is right, not only self-consistent: the limited-range codes of the eight 100 % bars, computed from (Kr, Kb) in float64 and
    rounded to the format's codes, come back as the bar.  Bound for 8-bit codes: half a luma code x 255 / 219 = 0.58, plus half a chroma code
    x 255 / 224 x 1.8814 = 1.07, plus the store's 0.5 -> 2; with 10-bit codes the code errors are a quarter of that -> 1."""
    bits = 10 if cm.is_hi(fmt) else 8
    bound = 1 if bits == 10 else 2
    w, h = 8, 2
    for rgb in cm.BARS:
        yc, cb, cr = cm.bar_codes(matrix, rgb, bits)
        ch = cm.chroma_shape(fmt, w, h)
        planes = cm.planes_of(fmt, np.full((h, w), yc), np.full(ch, cb), np.full(ch, cr))
        got = cm.node_rgba(fmt, w, h, planes, matrix)[..., :3].astype(int)
        want = np.array(rgb) * 255
        d = np.abs(got - want[None, None, :]).max()
        print(cm.NAMES[matrix], fmt, rgb, (yc, cb, cr), "max channel error", d)
        assert d <= bound, (cm.NAMES[matrix], fmt, rgb, got[0, 0], d)


def test_matrices_differ_on_saturated_colour():
    """(a witness that ignored its matrix argument would pass the BT.709 test)"""
    planes = cm.planes_of(cm.PLANAR_YUV420, np.full((2, 8), 81), np.full((1, 4), 90), np.full((1, 4), 240))
    nodes = [cm.node_rgba(cm.PLANAR_YUV420, 8, 2, planes, m) for m in MATRICES]
    assert not np.array_equal(nodes[0], nodes[1]) and not np.array_equal(nodes[0], nodes[2]) and not np.array_equal(nodes[1], nodes[2])


# ---- header and bindings

def _header():
    with open(os.path.join(ROOT, "include", "smr.h")) as f:
        return f.read()


def test_enum_values_agree_in_header_binding_and_rust_patch():
    from smelter_amd import _ffi, hip
    m = re.search(r"typedef enum smr_color_matrix \{([^}]*)\}", _header())
    assert m, "include/smr.h lacks smr_color_matrix"
    header = {k: int(v) for k, v in re.findall(r"(SMR_MATRIX_\w+)\s*=\s*(\d+)", m.group(1))}
    assert header == {"SMR_MATRIX_BT709": 0, "SMR_MATRIX_BT601": 1, "SMR_MATRIX_BT2020_NCL": 2}
    assert (hip.MATRIX_BT709, hip.MATRIX_BT601, hip.MATRIX_BT2020_NCL) == (0, 1, 2)
    assert (_ffi.MATRIX_BT709, _ffi.MATRIX_BT601, _ffi.MATRIX_BT2020_NCL) == (0, 1, 2)
    with open(os.path.join(ROOT, "integration", "smelter-render-hip.patch")) as f:
        patch = f.read()
    for name, value in header.items():
        assert re.search(r"^\+.*\b%s\b.*=\s*%d\b" % (name, value), patch, re.M), f"{name} = {value} is not bound in the Rust patch"
    assert (cm.BT709, cm.BT601, cm.BT2020_NCL) == (0, 1, 2)


def test_format_split_macros_and_abi_version():
    from smelter_amd import hip
    h = _header()
    assert re.search(r"#define SMR_FRAME_WITH_MATRIX\(format, m\)\s+\(\(uint32_t\)\(format\) \| \(\(uint32_t\)\(m\) << 8\)\)", h)
    assert re.search(r"#define SMR_FRAME_BASE_FORMAT\(format\)\s+\(\(uint32_t\)\(format\) & 0xffu\)", h)
    assert re.search(r"#define SMR_FRAME_MATRIX\(format\)\s+\(\(\(uint32_t\)\(format\) >> 8\) & 0xfu\)", h)
    assert re.search(r"#define SMR_ABI_VERSION 2\b", h)
    for f in range(15):
        assert hip.frame_format(f, hip.MATRIX_BT709) == f  # SMR_FRAME_WITH_MATRIX(f, 0) == f
        for m in (1, 2):
            t = hip.frame_format(f, m)
            assert t != f and hip.frame_base_format(t) == f and hip.frame_matrix(t) == m and t < 0x1000


def test_the_library_compiles_the_table_the_witness_uses():
    """smr_frame_formats.h's literals are the witness's (the emulator test reads them back from compiled code; this reads the source)."""
    with open(os.path.join(ROOT, "smelter_amd", "csrc", "smr_frame_formats.h")) as f:
        src = f.read()
    for m in MATRICES:
        lit = ", ".join("%.4ff" % c for c in cm.COEF[m])
        assert "SmrMatrixCoef{%s}" % lit in src, (cm.NAMES[m], lit)
