"""k_text_nodes (smelter_amd/csrc/smr_text_nodes.h: up to 16 Text rasters drawn in one launch, every workgroup walking the bin of its own
tile) compiled for the CPU by tests/emu/emu_text_nodes.cpp, with the bins tx_plan (host/text_bins.h) makes.  Every thread of every workgroup
of ONE launch runs on buffers that are exactly as large as what they hold: behind an unmapped page, the surface on a pitch larger than the
row and filled from a seeded pattern (guard mode 3: every byte outside a job's texels is compared after the launch — the store mask is the
job's texels), or surface, records, bin_first, bin_glyph and atlas each ENDING on an unmapped page (mode 1: a coverage load wider than a
byte, or one for a texel outside its glyph, faults on the atlas' last row).

The jobs are tests/text_zoo.py's, in sRGB and in unorm mode: widths 1, 3, 4, 5, 63, 64, 65, 67 x heights 1, 15, 16, 17; a job without glyphs;
a glyph in four bins; glyph starts at x mod 4 = 1, 2, 3; glyphs ending on the surface's last texel and on the atlas' last byte (atlas width
257); glyphs without an area, partly and wholly outside, at the ends of int32; an empty bin between full ones; painter's order; a base
4 bytes off a 16-byte boundary with tight rows; batches of 1, 16 and 17 jobs with a job without a texel in the middle.  The workgroup count of
every launch equals the tile sum.

All equal, BYTE FOR BYTE, to oracle.blit_glyphs: the model and the emulator run the same f32 operations in the same order on the same CPU
(the blend is k_blit_glyphs', which the oracle restates; the colour is prepared by the same f64 pow), so nothing is left to tolerate.  Test
infrastructure only: tests/test_gpu_text_nodes.py holds the kernel itself on the device."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as orc
from oracle.oracle import Glyph
from tests import emu_build, text_zoo as zoo

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
P8 = C.POINTER(C.c_uint8)
PI = C.POINTER(C.c_int)
PU = C.POINTER(C.c_uint32)
PF = C.POINTER(C.c_float)
PG = C.POINTER(zoo.CGlyph)
MAX_JOBS = 16
DEPS = ("smr_text_nodes.h", "host/text_bins.h", "smr_node_tiles.h", "../../tests/emu/emu_node_kernel.h", "smr_shader_dev.h", "smr_tables.h")


def load_emu():
    h = C.CDLL(emu_build.build("smr_emu_text_nodes", "emu_text_nodes.cpp", DEPS))
    h.emu_text_nodes.argtypes = [C.c_int, PI, PI, PU, PU, PF, C.POINTER(PG), PU, C.POINTER(P8), PU, PU, C.c_int, C.POINTER(P8), PU]
    h.emu_text_nodes.restype = C.c_int
    return h


def run(emu, jobs, guard, srgb, layout=(0, 0), want=None):
    """jobs: text_zoo jobs.  layout: (pitch rule, offset of the base): 0 = tight rows, 1 = the allocator's pitch, 2 = a pitch that is no
    multiple of 16.  One launch per 16 jobs, as smr_text_nodes makes them; in guard mode 3 every surface goes on its pitch + 32.  Every job's
    texels are held to oracle.blit_glyphs (or to want[i]).  -> (pictures, workgroups per launch, wide flag per job)"""
    pictures, launches, wides = [], [], []
    rule, off = layout
    for at in range(0, len(jobs), MAX_JOBS):
        part = jobs[at:at + MAX_JOBS]
        n = len(part)
        ws = np.array([j[0] for j in part], np.int32)
        hs = np.array([j[1] for j in part], np.int32)
        base = [int(w) * 4 if rule == 0 else ((int(w) * 4 + 255) & ~255) if rule == 1 else int(w) * 4 + 36 for w in ws]
        pitch = np.array([p + (32 if guard == 3 else 0) for p in base], np.uint32)
        offs = np.array([off] * n, np.uint32)
        bg = np.array([j[2] for j in part], np.float32).reshape(-1)
        garrs = [zoo.pack(j[3]) for j in part]
        ng = np.array([len(j[3]) for j in part], np.uint32)
        atlases = [np.ascontiguousarray(j[4], dtype=np.uint8) for j in part]
        aw = np.array([a.shape[1] for a in atlases], np.uint32)
        ah = np.array([a.shape[0] for a in atlases], np.uint32)
        outs = [np.zeros((max(int(h), 0), max(int(w), 0), 4), np.uint8) if w and h else np.zeros(4, np.uint8) for w, h in zip(ws, hs)]
        wide = np.zeros(n, np.uint32)
        arr8 = lambda xs: (P8 * n)(*[x.ctypes.data_as(P8) for x in xs])
        blocks = emu.emu_text_nodes(n, ws.ctypes.data_as(PI), hs.ctypes.data_as(PI), pitch.ctypes.data_as(PU), offs.ctypes.data_as(PU), bg.ctypes.data_as(PF),
                                    (PG * n)(*[C.cast(g, PG) for g in garrs]), ng.ctypes.data_as(PU), arr8(atlases), aw.ctypes.data_as(PU), ah.ctypes.data_as(PU),
                                    int(srgb), arr8(outs), wide.ctypes.data_as(PU))
        assert blocks != -77, "a byte outside a job's texels was written (see stderr)"
        assert blocks != -78, "tx_plan made a bin the kernel may not rely on (see stderr)"
        assert blocks == sum(zoo.tiles(int(w), int(h)) for w, h in zip(ws, hs)), (blocks, list(zip(ws, hs)))
        for i, (w, h, jbg, glyphs, atlas) in enumerate(part):
            if not (w and h):
                pictures.append(None)
                continue
            model = want[at + i] if want is not None else orc.blit_glyphs(w, h, jbg, glyphs, atlas, srgb=srgb)
            diff = np.argwhere(outs[i] != model)
            assert diff.size == 0, (f"job {at + i} ({w} x {h}, pitch {pitch[i]}, base + {off}, srgb {srgb}): texel (x {diff[0][1]}, y {diff[0][0]}) is "
                                    f"{outs[i][diff[0][0], diff[0][1]]}, the model gives {model[diff[0][0], diff[0][1]]}; {len(diff)} bytes differ")
            pictures.append(outs[i])
        launches.append(blocks)
        wides += [int(x) for x in wide]
    return pictures, launches, wides


@pytest.mark.parametrize("guard", [3, 1])
def test_text_nodes_in_one_launch(guard):
    """Run in a child process per guard mode: a store or load that leaves its buffer is a segmentation fault there, not here."""
    if not os.path.exists(emu_build.CLANG):
        pytest.skip("no clang++ to build the emulator with")
    env = dict(os.environ, SMR_EMU_TEXT_GUARD=str(guard))
    r = subprocess.run([sys.executable, "-m", "tests.test_emu_text_nodes"], capture_output=True, text=True, env=env, cwd=ROOT, timeout=1200)
    assert r.returncode == 0, f"guard mode {guard}: rc {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    assert "all text rasters drawn" in r.stdout, r.stdout[-2000:]


# ---- what the child processes run (python -m tests.test_emu_text_nodes, SMR_EMU_TEXT_GUARD = the guard mode)
LAYOUTS = ((0, 0), (1, 0), (1, 4), (0, 4), (2, 0))  # tight; the allocator's pitch; its base 4 bytes off; tight AND 4 bytes off; a pitch no multiple of 16


def expect_wide(w, layout, guard):
    rule, off = layout
    pitch = (w * 4 if rule == 0 else (w * 4 + 255) & ~255 if rule == 1 else w * 4 + 36) + (32 if guard == 3 else 0)
    return 1 if pitch % 16 == 0 and off % 16 == 0 else 0


def inner_sizes(emu, guard):
    jobs = zoo.sizes()
    for srgb in (True, False):
        for layout in LAYOUTS:
            for job in jobs:
                _, launches, wide = run(emu, [job], guard, srgb, layout)
                assert launches == [zoo.tiles(job[0], job[1])]
                if guard != 1:  # (mode 1: the buffer's start has the alignment of its size only)
                    assert wide == [expect_wide(job[0], layout, guard)], (wide, job[0], job[1], layout)


def inner_edges(emu, guard):
    cases = zoo.edge_cases()
    for srgb in (True, False):
        for layout in ((1, 0), (0, 4)):
            got = {}
            for name, job in cases.items():
                got[name] = run(emu, [job], guard, srgb, layout)[0][0]
            # (each already equals the oracle) the order of two overlapping glyphs shows
            assert (got["painter's order a, b"] != got["painter's order b, a"]).any()
            # a job without glyphs is its background on every texel
            assert len(np.unique(got["no glyphs"].reshape(-1, 4), axis=0)) == 1


def inner_extremes(emu, guard):
    """Glyphs at the ends of int32 lie wholly outside: the picture is the one without them (the oracle's own loop is not asked to walk
    2^31 rows; what is compared is its picture of the remaining glyphs)."""
    rng = np.random.default_rng(5)
    w, h, bg, glyphs, atlas = zoo.random_job(rng, 67, 17)
    big, small = 2**31 - 1, -2**31
    col = (0.9, 0.1, 0.5, 1.0)
    far = [Glyph(big, 3, 20, 10, 0, 0, col), Glyph(small, 3, 20, 10, 0, 0, col), Glyph(5, big, 20, 10, 0, 0, col), Glyph(5, small, 20, 10, 0, 0, col),
           Glyph(big - 5, big - 5, 24, 12, 1, 1, col), Glyph(small, small, 24, 12, 1, 1, col), Glyph(-20, big, 24, 12, 1, 1, col)]
    mixed = [far[0], glyphs[0], far[1], far[2]] + glyphs[1:3] + far[3:6] + glyphs[3:] + [far[6]]
    for srgb in (True, False):
        want = orc.blit_glyphs(w, h, bg, glyphs, atlas, srgb=srgb)
        run(emu, [(w, h, bg, mixed, atlas)], guard, srgb, (1, 0), want=[want])


def inner_batches(emu, guard):
    for n in (1, 16, 17):
        jobs = zoo.batch(n)
        for srgb in (True, False):
            pictures, launches, wide = run(emu, jobs, guard, srgb, (1, 0))
            assert len(launches) == (n + MAX_JOBS - 1) // MAX_JOBS
            assert sum(launches) == sum(zoo.tiles(j[0], j[1]) for j in jobs)
            if n > 2:
                assert pictures[n // 2] is None and wide[n // 2] == 0  # the job without a texel: no tile, no access
    assert run(emu, [], guard, True) == ([], [], [])


if __name__ == "__main__":
    g = int(os.environ["SMR_EMU_TEXT_GUARD"])
    lib = load_emu()
    lib.emu_set_guard(g, 0)
    inner_sizes(lib, g)
    inner_edges(lib, g)
    inner_extremes(lib, g)
    inner_batches(lib, g)
    print("all text rasters drawn")
