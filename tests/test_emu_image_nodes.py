"""k_image_nodes (smelter_amd/csrc/smr_image_nodes.h: the renderer's image pass, one launch for up to 16 Image nodes drawn into their own
resolution) compiled for the CPU by tests/emu/emu_image_nodes.cpp.  Every thread of every workgroup of ONE launch runs on buffers that are
exactly as large as the surfaces they hold, with the byte after them (guard mode 1) or before them (mode 2) on an unmapped page:

  * every byte of a destination buffer outside the dw x dh texels — the bytes before its base, its row padding — keeps its sentinel;
  * the texels are byte-equal to a texel-by-texel loop over sample_rgba_bilinear and store_texel in the same emulator: what
    k_rescale_bilinear does, so the batched kernel writes k_rescale_bilinear's bytes;
  * against the oracle's rescale_bilinear they meet the bar tests/test_gpu_parity.py::test_rescale_bilinear sets for this arithmetic:
    at most 1 LSB, at least 0.99 of the bytes identical;

in both pixel interpretations.  Test infrastructure only: tests/test_gpu_animated_images.py holds the kernel itself on the device."""
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
SENTINEL = 0xC3
MAX_JOBS = 16

# (source w, h, destination w, h): one job each, and the jobs of the mixed batches
SHAPES = [(160, 90, 1, 1), (160, 90, 65, 5), (3, 2, 67, 9), (5, 5, 5, 5), (7, 3, 3, 7), (64, 16, 128, 32)]


def load_emu():
    h = C.CDLL(emu_build.build("smr_emu_image_nodes", "emu_image_nodes.cpp", ("smr_image_nodes.h", "smr_node_tiles.h", "../../tests/emu/emu_node_kernel.h", "smr_shader_dev.h", "smr_tables.h")))
    h.emu_image_nodes.argtypes = [C.c_int, C.POINTER(P8), PI, PI, PI, PI, PU, PU, C.c_int, C.POINTER(P8), C.POINTER(P8), PU]
    h.emu_image_nodes.restype = C.c_int
    return h


def tiles(dw, dh):
    return ((dw + 63) // 64) * ((dh + 15) // 16)


def source(rng, w, h):
    """Noise with varying alpha, premultiplied the way the renderer's assets are (colour <= alpha)."""
    px = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    px[..., :3] = (px[..., :3].astype(np.uint32) * px[..., 3:4] // 255).astype(np.uint8)
    return px


def run(emu, jobs, srgb, seed):
    """jobs: (sw, sh, dw, dh, dst_pitch or 0 = tight, dst_off).  One launch per 16 jobs, as smr_image_nodes makes them.  -> (workgroups per
    launch, wide flag per job)."""
    rng = np.random.default_rng(seed)
    launches, wides = [], []
    for at in range(0, len(jobs), MAX_JOBS):
        batch = jobs[at:at + MAX_JOBS]
        n = len(batch)
        srcs = [source(rng, sw, sh) for sw, sh, *_ in batch]
        pitch = [p or dw * 4 for sw, sh, dw, dh, p, off in batch]
        sizes = [off + ((pitch[i] * (dh - 1) + dw * 4) if dw and dh else 0) for i, (sw, sh, dw, dh, p, off) in enumerate(batch)]
        outs = [np.zeros(max(s, 1), np.uint8) for s in sizes]
        refs = [np.zeros((max(dh, 1), max(dw, 1), 4), np.uint8) for sw, sh, dw, dh, p, off in batch]
        ints = [np.array([j[k] for j in batch], np.int32) for k in range(4)]
        pitches, offs = np.array(pitch, np.uint32), np.array([j[5] for j in batch], np.uint32)
        wide = np.zeros(n, np.uint32)
        arr = lambda xs: (P8 * n)(*[x.ctypes.data_as(P8) for x in xs])
        blocks = emu.emu_image_nodes(n, arr(srcs), *[a.ctypes.data_as(PI) for a in ints], pitches.ctypes.data_as(PU), offs.ctypes.data_as(PU),
                                     1 if srgb else 0, arr(outs), arr(refs), wide.ctypes.data_as(PU))
        assert blocks == sum(tiles(j[2], j[3]) for j in batch), (blocks, batch)
        for i, (sw, sh, dw, dh, p, off) in enumerate(batch):
            what = f"job {at + i} {batch[i]} srgb={srgb}"
            got = outs[i][:sizes[i]]
            if not (dw and dh):
                assert (got == SENTINEL).all(), what + ": a job without texels wrote"
                continue
            inside = np.zeros(sizes[i], bool)
            for y in range(dh):
                inside[off + y * pitch[i]: off + y * pitch[i] + dw * 4] = True
            bad = np.flatnonzero(~inside & (got != SENTINEL))
            assert bad.size == 0, f"{what}: byte {bad[0]} outside the destination's texels was written ({got[bad[0]]:#x})"
            texels = got[inside].reshape(dh, dw, 4)
            diff = np.argwhere(texels != refs[i])
            assert diff.size == 0, f"{what}: texel (x {diff[0][1]}, y {diff[0][0]}) is {texels[diff[0][0], diff[0][1]]}, the texel loop gives {refs[i][diff[0][0], diff[0][1]]}"
            want = orc.rescale_bilinear(srcs[i], dw, dh, orc.PX_RGBA8_SRGB if srgb else orc.PX_RGBA8_UNORM)
            d = np.abs(texels.astype(np.int32) - want.astype(np.int32))
            exact = float((d == 0).mean())
            print(f"{what}: max |diff| to the oracle {d.max()} LSB, {exact:.5f} of bytes identical")
            assert d.max() <= 1, f"{what}: {d.max()} LSB from the oracle"
            assert exact >= 0.99, f"{what}: only {exact:.5f} of bytes identical to the oracle"
        launches.append(blocks)
        wides += list(wide)
    return launches, wides


def mixed(n):
    """n jobs of mixed sizes on the allocator's pitch (a multiple of 256), a job without a tile in the middle."""
    jobs = []
    for i in range(n):
        sw, sh, dw, dh = SHAPES[i % len(SHAPES)]
        dw, dh = dw + 3 * (i // len(SHAPES)), dh + (i // len(SHAPES))
        jobs.append((sw, sh, dw, dh, (dw * 4 + 255) & ~255, 0))
    if n > 2:
        sw, sh, dw, dh, p, off = jobs[n // 2]
        jobs[n // 2] = (sw, sh, 0, dh, p, off)
    return jobs


@pytest.mark.parametrize("guard", [0, 1, 2])
def test_image_nodes_in_one_launch(guard):
    """Run in a child process per guard mode: a store or load that leaves its buffer is a segmentation fault there, not here."""
    if not os.path.exists(emu_build.CLANG):
        pytest.skip("no clang++ to build the emulator with")
    env = dict(os.environ, SMR_EMU_IMAGE_GUARD=str(guard))
    r = subprocess.run([sys.executable, "-m", "tests.test_emu_image_nodes"], capture_output=True, text=True, env=env, cwd=ROOT, timeout=1200)
    assert r.returncode == 0, f"guard mode {guard}: rc {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-2000:]}"
    assert "all image nodes drawn" in r.stdout, r.stdout[-2000:]


# ---- what the child processes run (python -m tests.test_emu_image_nodes, SMR_EMU_IMAGE_GUARD = the guard mode)
def inner_single_jobs(emu, guard):
    for srgb in (True, False):
        for k, (sw, sh, dw, dh) in enumerate(SHAPES):
            # tight rows (wide only where the row is a multiple of 16 bytes and the buffer starts on 16), the allocator's pitch, a pitch larger
            # than the row that is no multiple of 16, and a base that is not 16-aligned
            for pitch, off in ((0, 0), ((dw * 4 + 255) & ~255, 0), (dw * 4 + 36, 0), ((dw * 4 + 255) & ~255, 4), (dw * 4 + 48, 8)):
                launches, wide = run(emu, [(sw, sh, dw, dh, pitch, off)], srgb, seed=100 + k)
                assert launches == [tiles(dw, dh)]
                if guard != 1:  # (the buffer starts on 16 bytes there: the path follows from pitch and offset)
                    assert wide == [1 if ((pitch or dw * 4) % 16 == 0 and off % 16 == 0) else 0], (wide, pitch, off)


def inner_batches(emu, guard):
    for srgb in (True, False):
        for n in (1, 16, 17):
            jobs = mixed(n)
            launches, wide = run(emu, jobs, srgb, seed=7 + n)
            assert len(launches) == (n + MAX_JOBS - 1) // MAX_JOBS
            if guard != 1:
                assert all(w == (1 if j[2] else 0) for w, j in zip(wide, jobs)), wide
    assert run(emu, [], True, seed=1) == ([], [])


if __name__ == "__main__":
    g = int(os.environ["SMR_EMU_IMAGE_GUARD"])
    lib = load_emu()
    lib.emu_set_guard(g, 0)
    inner_single_jobs(lib, g)
    inner_batches(lib, g)
    print("all image nodes drawn")
