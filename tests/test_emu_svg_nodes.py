"""k_svg_nodes (smelter_amd/csrc/smr_svg_nodes.h: the colour fix-up of up to 16 new SVG rasters, in place, in one launch) compiled for
the CPU by tests/emu/emu_svg_nodes.cpp.  Every thread of every workgroup of ONE launch runs on buffers that are exactly as large as the
surfaces they hold, behind an unmapped page, on a pitch larger than the row and filled from a seeded pattern (guard mode 3: the emulator
compares every byte outside a job's texels after the launch — the store mask is the job's texels), or ending on an unmapped page (mode 1):

  * the 256 x 256 image whose R channel enumerates every (c, alpha), G and B the same table under two fixed permutations of c;
  * random premultiplied images (c <= alpha) at widths 1, 3, 4, 5, 63, 64, 65, 67 x heights 1, 15, 16, 17;
  * a surface whose base is 4 bytes off a 16-byte boundary (the texel path), tight rows, the allocator's pitch;
  * batches of 1, 16 and 17 jobs of mixed sizes (sv_plan's prefix sums; 17 jobs are two launches)

all equal, BYTE FOR BYTE, to oracle.add_premultiplied_alpha(oracle.remove_premultiplied_alpha(x), True): the model and the emulator run the
same f32 operations on the same CPU, so nothing is left to tolerate.  Test infrastructure only: tests/test_gpu_svg_images.py holds the
kernel itself on the device."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as orc
from tests import emu_build

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
P8 = C.POINTER(C.c_uint8)
PI = C.POINTER(C.c_int)
PU = C.POINTER(C.c_uint32)
MAX_JOBS = 16
WIDTHS = (1, 3, 4, 5, 63, 64, 65, 67)
HEIGHTS = (1, 15, 16, 17)


def load_emu():
    h = C.CDLL(emu_build.build("smr_emu_svg_nodes", "emu_svg_nodes.cpp", ("smr_svg_nodes.h", "smr_node_tiles.h", "../../tests/emu/emu_node_kernel.h", "smr_shader_dev.h", "smr_tables.h")))
    h.emu_svg_nodes.argtypes = [C.c_int, C.POINTER(P8), PI, PI, PU, PU, C.POINTER(P8), PU]
    h.emu_svg_nodes.restype = C.c_int
    return h


def exhaustive():
    """256 x 256: alpha = the row, R = the column, G and B the column under two fixed permutations — every (c, alpha) in every channel."""
    c = np.arange(256, dtype=np.uint8)
    px = np.empty((256, 256, 4), np.uint8)
    px[..., 0] = c[None, :]
    px[..., 1] = np.random.default_rng(1).permutation(c)[None, :]
    px[..., 2] = np.random.default_rng(2).permutation(c)[None, :]
    px[..., 3] = c[:, None]
    return px


def premultiplied(rng, w, h):
    """Noise with varying alpha, premultiplied as tiny-skia's pixmap is (colour <= alpha)."""
    px = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    px[..., :3] = (px[..., :3].astype(np.uint32) * px[..., 3:4] // 255).astype(np.uint8)
    return px


def model(px):
    return orc.add_premultiplied_alpha(orc.remove_premultiplied_alpha(px), True)


def tiles(w, h):
    return ((w + 63) // 64) * ((h + 15) // 16)


def run(emu, jobs, guard):
    """jobs: (pixels[h, w, 4], pitch or 0 = tight, offset of the base).  One launch per 16 jobs, as smr_svg_nodes makes them.  In guard mode
    3 every job goes on its pitch + 32.  -> (workgroups per launch, wide flag per job)."""
    launches, wides = [], []
    for at in range(0, len(jobs), MAX_JOBS):
        batch = jobs[at:at + MAX_JOBS]
        n = len(batch)
        ins = [np.ascontiguousarray(px) for px, _, _ in batch]
        ws = np.array([px.shape[1] for px in ins], np.int32)
        hs = np.array([px.shape[0] for px in ins], np.int32)
        pitch = np.array([(p or int(w) * 4) + (32 if guard == 3 else 0) for (_, p, _), w in zip(batch, ws)], np.uint32)
        offs = np.array([off for _, _, off in batch], np.uint32)
        outs = [np.zeros_like(px) if px.size else np.zeros(4, np.uint8) for px in ins]
        wide = np.zeros(n, np.uint32)
        arr = lambda xs: (P8 * n)(*[x.ctypes.data_as(P8) for x in xs])
        blocks = emu.emu_svg_nodes(n, arr(ins), ws.ctypes.data_as(PI), hs.ctypes.data_as(PI), pitch.ctypes.data_as(PU), offs.ctypes.data_as(PU),
                                   arr(outs), wide.ctypes.data_as(PU))
        assert blocks != -77, "a byte outside a job's texels was written (see stderr)"
        assert blocks == sum(tiles(int(w), int(h)) if w and h else 0 for w, h in zip(ws, hs)), (blocks, list(zip(ws, hs)))
        for i, px in enumerate(ins):
            if not px.size:
                continue
            want = model(px)
            diff = np.argwhere(outs[i] != want)
            assert diff.size == 0, (f"job {at + i} ({ws[i]} x {hs[i]}, pitch {pitch[i]}, base + {offs[i]}): texel (x {diff[0][1]}, y {diff[0][0]}) "
                                    f"{px[diff[0][0], diff[0][1]]} became {outs[i][diff[0][0], diff[0][1]]}, the model gives {want[diff[0][0], diff[0][1]]}; "
                                    f"{len(diff)} bytes differ")
        launches.append(blocks)
        wides += [int(x) for x in wide]
    return launches, wides


@pytest.mark.parametrize("guard", [3, 1])
def test_svg_nodes_in_one_launch(guard):
    """Run in a child process per guard mode: a store or load that leaves its buffer is a segmentation fault there, not here."""
    if not os.path.exists(emu_build.CLANG):
        pytest.skip("no clang++ to build the emulator with")
    env = dict(os.environ, SMR_EMU_SVG_GUARD=str(guard))
    r = subprocess.run([sys.executable, "-m", "tests.test_emu_svg_nodes"], capture_output=True, text=True, env=env, cwd=ROOT, timeout=1200)
    assert r.returncode == 0, f"guard mode {guard}: rc {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    assert "all svg rasters fixed" in r.stdout, r.stdout[-2000:]


# ---- what the child processes run (python -m tests.test_emu_svg_nodes, SMR_EMU_SVG_GUARD = the guard mode)
def inner_exhaustive(emu, guard):
    launches, wide = run(emu, [(exhaustive(), 0, 0)], guard)
    assert launches == [tiles(256, 256)]
    if guard != 1:  # (mode 1: the buffer's start has the alignment of its size only)
        assert wide == [1]
    # the same through the texel path
    launches, wide = run(emu, [(exhaustive(), 0, 4)], guard)
    assert launches == [tiles(256, 256)] and (guard == 1 or wide == [0])


def inner_sizes(emu, guard):
    rng = np.random.default_rng(42)
    for w in WIDTHS:
        for h in HEIGHTS:
            px = premultiplied(rng, w, h)
            # tight rows, the allocator's pitch, a base 4 bytes off a 16-byte boundary, a pitch that is no multiple of 16
            for pitch, off in ((0, 0), ((w * 4 + 255) & ~255, 0), ((w * 4 + 255) & ~255, 4), (w * 4 + 36, 0)):
                launches, wide = run(emu, [(px, pitch, off)], guard)
                assert launches == [tiles(w, h)]
                if guard != 1:
                    assert wide == [1 if ((pitch or w * 4) % 16 == 0 and off % 16 == 0) else 0], (wide, w, h, pitch, off)


def inner_batches(emu, guard):
    rng = np.random.default_rng(7)
    for n in (1, 16, 17):
        jobs = []
        for i in range(n):
            w, h = WIDTHS[(3 * i) % len(WIDTHS)] + 2 * (i // 8), HEIGHTS[i % len(HEIGHTS)] + (i // 4)
            jobs.append((premultiplied(rng, w, h), (w * 4 + 255) & ~255, 4 if i % 5 == 3 else 0))
        if n > 2:  # a job without a texel in the middle: no tile, no access
            jobs[n // 2] = (np.zeros((0, 5, 4), np.uint8), 256, 0)
        launches, wide = run(emu, jobs, guard)
        assert len(launches) == (n + MAX_JOBS - 1) // MAX_JOBS
        if guard != 1:
            assert wide == [1 if (px.size and off == 0) else 0 for px, _, off in jobs], wide
    assert run(emu, [], guard) == ([], [])


if __name__ == "__main__":
    g = int(os.environ["SMR_EMU_SVG_GUARD"])
    lib = load_emu()
    lib.emu_set_guard(g, 0)
    inner_exhaustive(lib, g)
    inner_sizes(lib, g)
    inner_batches(lib, g)
    print("all svg rasters fixed")
