"""The input converter's classifier (smelter_amd/csrc/smr_convert_route.h: conv_route, conv_rgb12_ok) compiled for the CPU by
tests/emu/emu_convert_route.cpp and pinned on frames described by numbers — a plane is an address, a pitch and who owns it; nothing is read.

The expected routes are written out by hand from the rules in the header's comments:
  * a node that does not take 16-byte stores: general;
  * SMR_CONVERT_AUTO, width a multiple of 4 from 8, even height from 2, both <= 16384: a block converter if the planes allow it —
    8-bit 4:2:0 / J420 / NV12: every plane dword-aligned with rows of at least their bytes; the tight kernel unless the library owns the chroma
    plane(s); the kernel per colour matrix.  10-bit: the first plane 8-byte aligned, chroma planes dword-aligned, rows of at least their bytes
    (v210: 16 bytes per six pixels);
  * otherwise the 4 x 2 batch kernel for planar 4:2:0 / 4:2:2 / 4:4:4 and NV12 whose subsampled axes are even, UYVY / YUYV of even width from 8
    (dword-aligned plane), BGRA / ARGB (16-byte aligned plane), sizes from 2 to 16384, unless SMR_CONVERT_GENERAL;
  * otherwise general."""
import ctypes as C

import pytest

F = dict(YUV420=0, YUV422=1, YUV444=2, YUVJ420=3, UYVY=4, YUYV=5, NV12=6, BGRA=7, ARGB=8, RGBA=9, P010=10, YUV420P10=11, YUV422P10=12, P210=13, V210=14)
ROUTES = ["GENERAL", "BATCH", "P", "NV", "P_TIGHT", "NV_TIGHT", "HI420_P", "HI420_P010", "HI422_P", "HI422_P210", "HI422_V210",
          "P_601", "NV_601", "P_TIGHT_601", "NV_TIGHT_601", "P_2020", "NV_2020", "P_TIGHT_2020", "NV_TIGHT_2020", "COUNT"]
AUTO, GENERAL, BLOCK_4X2 = 0, 1, 2


@pytest.fixture(scope="module")
def lib():
    from tests import emu_build
    h = C.CDLL(emu_build.build("smr_emu_convert_route", "emu_convert_route.cpp", ("smr_convert_route.h", "smr_frame_formats.h")))
    h.emu_conv_route.restype = C.c_int
    h.emu_conv_route_value.restype = C.c_int
    return h


def plane_rows(fmt, w):
    """bytes per row of each plane of a frame of width w (include/smr.h)"""
    c = (w + 1) // 2
    return {"YUV420": [w, c, c], "YUVJ420": [w, c, c], "YUV422": [w, c, c], "YUV444": [w, w, w], "NV12": [w, 2 * c], "UYVY": [4 * c], "YUYV": [4 * c],
            "BGRA": [4 * w], "ARGB": [4 * w], "RGBA": [4 * w], "P010": [2 * w, 4 * c], "P210": [2 * w, 4 * c], "YUV420P10": [2 * w, 2 * c, 2 * c],
            "YUV422P10": [2 * w, 2 * c, 2 * c], "V210": [16 * ((w + 5) // 6)]}[fmt]


def route(lib, fmt, w, h, owned=(True, True, True), impl=AUTO, matrix=0, node16=True, ptr_off=(0, 0, 0), pitch=None):
    """-> (route name, conv_rgb12_ok).  Planes at 256-byte aligned addresses (+ ptr_off) with rows padded to 256 bytes unless `pitch` says otherwise."""
    rows = plane_rows(fmt, w)
    n = len(rows)
    ptr = (C.c_ulonglong * 3)(*[0x100000 * (k + 1) + ptr_off[k] for k in range(3)])
    pit = (C.c_ulonglong * 3)(*[(pitch[k] if pitch and pitch[k] is not None else (rows[k] + 255) // 256 * 256) if k < n else 0 for k in range(3)])
    own = (C.c_int * 3)(*[1 if o else 0 for o in owned])
    ok = C.c_int(-1)
    r = lib.emu_conv_route(impl, F[fmt] | (matrix << 8), w, h, n, ptr, pit, own, 1 if node16 else 0, C.byref(ok))
    return ROUTES[r + 1], bool(ok.value)


def test_the_tests_route_names_are_the_headers(lib):
    assert [lib.emu_conv_route_value(i) for i in range(len(ROUTES))] == list(range(-1, len(ROUTES) - 1))


# the routes of a frame the block converters take (1920 x 1080, planes the library owns, BT.709), per base format
BASE = dict(YUV420="P", YUV422="BATCH", YUV444="BATCH", YUVJ420="P", UYVY="BATCH", YUYV="BATCH", NV12="NV", BGRA="BATCH", ARGB="BATCH", RGBA="GENERAL",
            P010="HI420_P010", YUV420P10="HI420_P", YUV422P10="HI422_P", P210="HI422_P210", V210="HI422_V210")
BLOCK_FORMATS = ("YUV420", "YUVJ420", "NV12", "P010", "YUV420P10", "YUV422P10", "P210", "V210")
HI = ("P010", "YUV420P10", "YUV422P10", "P210", "V210")
# ... and of one the 4 x 2 batch kernel takes where it applies
NO_BLOCK = dict(BASE, YUV420="BATCH", YUVJ420="BATCH", NV12="BATCH", P010="GENERAL", YUV420P10="GENERAL", YUV422P10="GENERAL", P210="GENERAL", V210="GENERAL")
ALL_GENERAL = {f: "GENERAL" for f in F}


def expect(lib, want, w, h, **kw):
    got = {f: route(lib, f, w, h, **kw)[0] for f in F}
    assert got == want, {f: (got[f], want[f]) for f in F if got[f] != want[f]}


def test_every_format_at_1920x1080_with_owned_planes(lib):
    expect(lib, BASE, 1920, 1080)
    # an RGB12 node: the block converters' frames, and only those
    assert {f: route(lib, f, 1920, 1080)[1] for f in F} == {f: f in BLOCK_FORMATS for f in F}


def test_planes_the_library_does_not_own_take_the_tight_kernel(lib):
    tight = dict(BASE, YUV420="P_TIGHT", YUVJ420="P_TIGHT", NV12="NV_TIGHT")  # (8-bit 4:2:0 only: the 10-bit kernels stay inside a row's bytes)
    expect(lib, tight, 1920, 1080, owned=(False, False, False))
    expect(lib, tight, 1920, 1080, owned=(True, False, False))
    expect(lib, dict(tight, NV12="NV"), 1920, 1080, owned=(True, True, False))  # (NV12 has no third plane; planar needs both chroma planes owned)
    expect(lib, BASE, 1920, 1080, owned=(False, True, True))  # (the luma plane is read inside its rows by either kernel)


@pytest.mark.parametrize("w", [8, 12])
def test_block_widths(lib, w):
    expect(lib, BASE, w, 16)


def test_widths_the_block_converters_decline(lib):
    expect(lib, NO_BLOCK, 10, 16)
    expect(lib, dict(NO_BLOCK, UYVY="GENERAL", YUYV="GENERAL"), 6, 16)  # (packed 4:2:2: from 8)
    # odd: nothing subsampled horizontally, so 4:4:4 and the byte permutes only
    expect(lib, dict(ALL_GENERAL, YUV444="BATCH", BGRA="BATCH", ARGB="BATCH"), 7, 16)


def test_heights(lib):
    expect(lib, BASE, 16, 2)
    expect(lib, BASE, 16, 16384)
    # odd: no block converter; the batch kernel where the chroma is not subsampled vertically
    expect(lib, dict(NO_BLOCK, YUV420="GENERAL", YUVJ420="GENERAL", NV12="GENERAL"), 16, 3)


def test_sizes_past_16384_are_general(lib):
    expect(lib, ALL_GENERAL, 16388, 2)
    expect(lib, ALL_GENERAL, 16, 16386)


def test_plane_alignment(lib):
    # first plane aligned to 4, not 8: no 10-bit block converter; no 16-byte permute kernel either
    expect(lib, dict(BASE, BGRA="GENERAL", ARGB="GENERAL", **{f: "GENERAL" for f in HI}), 1920, 1080, ptr_off=(4, 0, 0))
    # ... its pitch likewise
    for f in F:
        rows = plane_rows(f, 1920)
        want = "GENERAL" if f in HI + ("BGRA", "ARGB") else BASE[f]
        assert route(lib, f, 1920, 1080, pitch=[(rows[0] + 255) // 256 * 256 + 4, None, None])[0] == want, f
    # a chroma plane aligned to 2, not 4: no block converter (v210 has no chroma plane)
    for off in ((0, 2, 0), (0, 0, 2)):
        want = dict(NO_BLOCK, V210="HI422_V210")
        if off[2]:
            want.update(NV12="NV", P010="HI420_P010", P210="HI422_P210")  # (two planes: nothing moved)
        expect(lib, want, 1920, 1080, ptr_off=off)


def test_pitches(lib):
    # v210: 16 bytes per six pixels — 1920 / 6 = 320 groups; one short: general
    assert route(lib, "V210", 1920, 1080, pitch=[16 * 320])[0] == "HI422_V210"
    assert route(lib, "V210", 1920, 1080, pitch=[16 * 319])[0] == "GENERAL"
    assert route(lib, "V210", 1922, 1080, pitch=[16 * 320])[0] == "GENERAL"  # (not a multiple of 4)
    assert route(lib, "V210", 1924, 1080, pitch=[16 * 320])[0] == "GENERAL"  # (321 groups)
    # a first-plane pitch below the row's bytes (16 short: every alignment holds)
    for f in F:
        rows = plane_rows(f, 1920)
        assert route(lib, f, 1920, 1080, pitch=[rows[0] - 16, None, None])[0] == NO_BLOCK[f], f
    # ... and a chroma pitch: exactly the row's bytes is enough, 4 fewer is not
    for f in ("YUV420", "YUVJ420", "NV12", "P010", "YUV420P10", "YUV422P10", "P210"):
        rows = plane_rows(f, 1920)
        assert route(lib, f, 1920, 1080, pitch=[None, rows[1], None])[0] == BASE[f], f
        assert route(lib, f, 1920, 1080, pitch=[None, rows[1] - 4, None])[0] == NO_BLOCK[f], f


def test_a_node_that_takes_no_16_byte_stores_is_general_unless_rgb12(lib):
    expect(lib, ALL_GENERAL, 1920, 1080, node16=False)
    expect(lib, BASE, 1920, 1080, node16=True)  # (what smr_frames_to_rgba_batch passes for an RGB12 node, whatever its alignment)


def test_convert_impl(lib):
    expect(lib, ALL_GENERAL, 1920, 1080, impl=GENERAL)
    expect(lib, NO_BLOCK, 1920, 1080, impl=BLOCK_4X2)
    assert not any(route(lib, f, 1920, 1080, impl=i)[1] for f in F for i in (GENERAL, BLOCK_4X2))


@pytest.mark.parametrize("matrix,tag", [(1, "_601"), (2, "_2020")])
def test_the_matrix_moves_only_the_8_bit_block_kernels(lib, matrix, tag):
    ycbcr = [f for f in F if f not in ("BGRA", "ARGB", "RGBA")]
    for owned, t in ((True, ""), (False, "_TIGHT")):
        want = dict(BASE, YUV420="P" + t + tag, YUVJ420="P" + t + tag, NV12="NV" + t + tag)
        got = {f: route(lib, f, 1920, 1080, matrix=matrix, owned=(owned,) * 3)[0] for f in ycbcr}
        assert got == {f: want[f] for f in ycbcr}
    assert {f: route(lib, f, 10, 16, matrix=matrix)[0] for f in ycbcr} == {f: NO_BLOCK[f] for f in ycbcr}


def test_rgb12_width_cap(lib):
    for f in BLOCK_FORMATS:
        assert route(lib, f, 5120, 16) == (BASE[f], True), f   # 3 * 5120 = 15360 <= 15364
        assert route(lib, f, 5124, 16) == (BASE[f], False), f  # the route stays, an RGB12 node is declined
    assert route(lib, "YUV422", 1920, 1080)[1] is False
