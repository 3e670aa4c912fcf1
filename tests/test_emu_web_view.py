"""k_web_view (smelter_amd/csrc/smr_web_view.h: a WebView node's page and up to 16 children per launch) compiled for the CPU by
tests/emu/emu_web_view.cpp.  Every thread of every workgroup of a node's launches runs on buffers that are exactly as large as the surfaces
they hold, with the byte after them (guard mode 1) or before them (mode 2) on an unmapped page:

  * every byte of the destination buffer outside the w x h texels — the bytes before its base, its row padding — keeps its sentinel;
  * on INTEGER rectangles the texels are within 1 LSB of the committed oracle (oracle.apply_layouts over tests/web_view_model.oracle_layers):
    the project's compositor bar;
  * on FRACTIONAL rectangles (quarters, never .5) they are within 1 LSB of tests/web_view_model.model_node, the f32 model of
    render_website.wgsl and the rasteriser's coverage rule — which test_model_meets_the_oracle_on_integer_rectangles first holds to the
    oracle itself, on the CPU, within the same 1 LSB;

pages 5 x 3, 67 x 21 (width no multiple of 4), 130 x 33 (tile seams both ways) and 64 x 16 on a pitched, 4-byte-aligned destination (the
narrow store path); 0, 1, 3 and 17 children (two launches); over and under content; sRGB and UNORM.  Test infrastructure only:
tests/test_gpu_web_view.py holds the kernel itself on the device."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import emu_build
from tests import web_view_model as wm

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
P8 = C.POINTER(C.c_uint8)
PI = C.POINTER(C.c_int)
PU = C.POINTER(C.c_uint32)
PF = C.POINTER(C.c_float)
SENTINEL = 0xC3

# (page w, h, destination pitch or 0 = the allocator's (a multiple of 256), destination offset, page pitch or 0 = tight)
PAGES = [(5, 3, 0, 0, 0), (67, 21, 0, 0, 0), (130, 33, 0, 0, 768), (64, 16, 64 * 4 + 4, 4, 0)]
COUNTS = (0, 1, 3, 17)


def load_emu():
    h = C.CDLL(emu_build.build("smr_emu_web_view", "emu_web_view.cpp", ("smr_web_view.h", "smr_node_tiles.h", "../../tests/emu/emu_node_kernel.h", "smr_layout_dev.h", "smr_shader_dev.h", "smr_tables.h")))
    h.emu_web_view.argtypes = [P8, C.c_int, C.c_int, C.c_uint32, C.c_int, C.POINTER(P8), PI, PI, PF, C.c_int, C.c_int, C.c_uint32, C.c_uint32, P8, PU]
    h.emu_web_view.restype = C.c_int
    return h


def case(W, H, n, fractional, seed):
    """-> (page, children, rects): n children on rectangles taken round the list from a start that differs per case."""
    rng = np.random.default_rng(seed)
    page = wm.page_bitmap(rng, W, H)
    children = wm.make_children(rng, n)
    if n >= 2:
        children[1] = None  # a child without a texture: the 1 x 1 transparent one
    pool = wm.fractional_rects(W, H) if fractional else wm.integer_rects(W, H)
    rects = [pool[(seed * 5 + k) % len(pool)] for k in range(n)]
    return page, children, rects


def run(emu, page, children, rects, method, srgb, dst_pitch, dst_off, page_pitch):
    """One node through the emulator -> (texels h x w x 4, launches, wide, page_wide); asserts the write footprint."""
    H, W = page.shape[:2]
    n = len(children)
    pitch = dst_pitch or (W * 4 + 255) & ~255
    ppitch = page_pitch or W * 4
    size = dst_off + pitch * (H - 1) + W * 4
    out = np.zeros(size, np.uint8)
    info = np.zeros(3, np.uint32)
    one = np.zeros((1, 1, 4), np.uint8)
    px = [np.ascontiguousarray(c if c is not None else one) for c in children]
    sw = np.array([0 if c is None else c.shape[1] for c in children] + [0], np.int32)
    sh = np.array([0 if c is None else c.shape[0] for c in children] + [0], np.int32)
    rc = np.array([float(v) for q in rects for v in q] + [0.0], np.float32)
    srcs = (P8 * max(n, 1))(*[p.ctypes.data_as(P8) for p in px])
    pg = np.ascontiguousarray(page)
    blocks = emu.emu_web_view(pg.ctypes.data_as(P8), W, H, ppitch, n, srcs, sw.ctypes.data_as(PI), sh.ctypes.data_as(PI), rc.ctypes.data_as(PF),
                              1 if method == wm.UNDER else 0, 1 if srgb else 0, pitch, dst_off, out.ctypes.data_as(P8), info.ctypes.data_as(PU))
    assert blocks == ((W + 63) // 64) * ((H + 15) // 16), blocks
    inside = np.zeros(size, bool)
    for y in range(H):
        inside[dst_off + y * pitch: dst_off + y * pitch + W * 4] = True
    bad = np.flatnonzero(~inside & (out != SENTINEL))
    assert bad.size == 0, f"byte {bad[0]} outside the destination's texels was written ({out[bad[0]]:#x})"
    return out[inside].reshape(H, W, 4), int(info[0]), int(info[1]), int(info[2])


def lsb(a, b):
    return int(np.abs(a.astype(np.int32) - b.astype(np.int32)).max())


def test_model_meets_the_oracle_on_integer_rectangles():
    """The f32 model is trusted on fractional rectangles only because it is within 1 LSB of the oracle where the oracle applies."""
    worst = 0
    for W, H, *_ in PAGES:
        for n in COUNTS:
            for method in (wm.OVER, wm.UNDER, wm.CHROMIUM):
                for srgb in (True, False):
                    page, children, rects = case(W, H, n, False, seed=W + n)
                    d = lsb(wm.model_node(page, children, rects, method, srgb), wm.oracle_node(page, children, rects, method, srgb))
                    worst = max(worst, d)
                    assert d <= 1, f"{W}x{H}, {n} children, method {method}, srgb={srgb}: the model is {d} LSB from the oracle"
    print(f"model against the oracle on integer rectangles: at most {worst} LSB")


@pytest.mark.parametrize("guard", [0, 1, 2])
def test_web_view_node_in_one_launch_per_16_children(guard):
    """Run in a child process per guard mode: a store or load that leaves its buffer is a segmentation fault there, not here."""
    if not os.path.exists(emu_build.CLANG):
        pytest.skip("no clang++ to build the emulator with")
    env = dict(os.environ, SMR_EMU_WEB_GUARD=str(guard))
    r = subprocess.run([sys.executable, "-m", "tests.test_emu_web_view"], capture_output=True, text=True, env=env, cwd=ROOT, timeout=1200)
    assert r.returncode == 0, f"guard mode {guard}: rc {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-2000:]}"
    assert "all web views drawn" in r.stdout, r.stdout[-2000:]


# ---- what the child processes run (python -m tests.test_emu_web_view, SMR_EMU_WEB_GUARD = the guard mode)
def inner(emu, guard):
    worst = {"oracle": 0, "model": 0}
    for W, H, dpitch, doff, ppitch in PAGES:
        for n in COUNTS:
            for method in (wm.OVER, wm.UNDER):
                for srgb in (True, False):
                    for fractional in (False, True):
                        if fractional and n == 0:
                            continue
                        page, children, rects = case(W, H, n, fractional, seed=W + n)
                        what = f"{W}x{H} pitch {dpitch} off {doff}, {n} children, method {method}, srgb={srgb}, fractional={fractional}"
                        got, launches, wide, page_wide = run(emu, page, children, rects, method, srgb, dpitch, doff, ppitch)
                        assert launches == (2 if n == 17 else 1), (what, launches)
                        if guard != 1:  # (the buffers start on 16 bytes there: the paths follow from pitch and offset)
                            assert wide == (0 if dpitch else 1), (what, wide)
                            assert page_wide == (1 if (ppitch or W * 4) % 16 == 0 else 0), (what, page_wide)
                        model = wm.model_node(page, children, rects, method, srgb)
                        dm = lsb(got, model)
                        worst["model"] = max(worst["model"], dm)
                        if not fractional:
                            do = lsb(got, wm.oracle_node(page, children, rects, method, srgb))
                            worst["oracle"] = max(worst["oracle"], do)
                            print(f"{what}: {do} LSB from the oracle, {dm} from the model")
                            assert do <= 1, f"{what}: {do} LSB from the oracle"
                        else:
                            print(f"{what}: {dm} LSB from the model")
                        assert dm <= 1, f"{what}: {dm} LSB from the model"
    # the page alone, whatever the method says without children; and children only where rectangles say so
    page, children, rects = case(67, 21, 3, False, seed=5)
    alone, *_ = run(emu, page, [], [], wm.OVER, True, 0, 0, 0)
    assert (alone == wm.swizzle(page)).all(), "the page alone is not the swizzled bitmap, byte for byte"
    under, *_ = run(emu, page, [], [], wm.UNDER, True, 0, 0, 0)
    assert (under == alone).all()
    hostile = [(float("nan"), 0, 4, 4), (0, 0, float("inf"), 4), (1e30, 1e30, 1e30, 1e30), (-1e30, -1e30, 1e30, 1e30), (2, 2, -4, 4)]
    kids = wm.make_children(np.random.default_rng(3), len(hostile))
    same, *_ = run(emu, page, kids, hostile, wm.OVER, True, 0, 0, 0)
    assert (same == alone).all(), "a rectangle without pixels drew"
    print(f"worst: {worst}")


if __name__ == "__main__":
    g = int(os.environ["SMR_EMU_WEB_GUARD"])
    lib = load_emu()
    lib.emu_set_guard(g, 0)
    inner(lib, g)
    print("all web views drawn")
