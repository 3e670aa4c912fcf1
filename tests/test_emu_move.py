"""k_move_rects (smelter_amd/csrc/smr_move_rects.h: the local gather's transport, one launch for up to 16 pitched rectangles) compiled for
the CPU by tests/emu/emu_move.cpp.  Every thread of every workgroup of ONE launch runs on buffers that are exactly as large as the rectangles
they hold, with the byte after them (guard mode 1) or before them (mode 2) on an unmapped page: the bytes arrive, the destination's row padding
keeps its sentinel, nothing outside [row, row + row_bytes) is read or written.  Once more under AddressSanitizer + UBSan.  Test
infrastructure only: tests/test_gpu_comm.py and tests/test_gpu_sharded_renderer.py hold the kernel itself on the device."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import emu_build

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
P8 = C.POINTER(C.c_uint8)
PU = C.POINTER(C.c_uint32)
SENTINEL = 0xC3


def load_emu():
    h = C.CDLL(emu_build.build("smr_emu_move", "emu_move.cpp", ("smr_move_rects.h",)))
    h.emu_move_rects.argtypes = [C.c_int, C.POINTER(P8)] + [PU] * 8 + [C.POINTER(P8), PU]
    h.emu_move_rects.restype = C.c_int
    return h


def pitch256(n):
    return (n + 255) & ~255


def the_sixteen():
    """(row_bytes, rows, src_pitch, dst_pitch, src_off, dst_off, src_align, dst_align) x 16: what one launch may be handed."""
    r = []
    r.append((1280 * 4, 37, 1280 * 4, pitch256(1280 * 4), 0, 0, 16, 16))      # an RGBA8 tile, tight rows into the library's pitch
    r.append((320 * 4, 180, pitch256(320 * 4), pitch256(320 * 4), 0, 0, 16, 16))  # ... pitch to pitch
    r.append((16, 700, 16, 32, 0, 0, 16, 16))                                   # one 16-byte group per row: 256 rows side by side
    r.append((960, 5, 1024, 960, 0, 0, 16, 16))                                 # a chroma plane of a 1080p frame
    r.append((4112, 9, 4352, 4112, 16, 32, 16, 16))                             # wider than 256 lanes x 16 bytes, aligned offsets
    r.append((1, 13, 1, 3, 0, 0, 1, 1))                                         # widths of 1 .. 67 bytes, odd pitches
    r.append((2, 7, 5, 2, 3, 1, 1, 1))
    r.append((15, 9, 17, 31, 1, 2, 1, 1))
    r.append((17, 6, 33, 19, 5, 5, 16, 16))                                     # same phase (5), odd pitches: the phase then changes per row
    r.append((33, 4, 48, 64, 7, 7, 16, 16))                                     # same phase in every row: head 9, body 16, tail 8
    r.append((67, 11, 80, 96, 3, 3, 16, 16))                                    # head 13, body 48, tail 6
    r.append((67, 3, 67, 67, 0, 9, 16, 16))                                     # phases differ: bytes throughout
    r.append((64, 1, 64, 64, 0, 0, 16, 16))                                     # one row, fast
    r.append((61, 1, 61, 61, 2, 11, 1, 1))                                      # one row, bytes
    r.append((128, 0, 128, 128, 0, 0, 16, 16))                                  # zero rows
    r.append((1921, 8, pitch256(1921), pitch256(1921), 0, 0, 16, 16))           # an odd-width luma plane on the library's pitch: body + tail
    return r


def run(emu, rects, seed=5):
    rng = np.random.default_rng(seed)
    n = len(rects)
    data = [rng.integers(0, 256, max(rb * rows, 1), dtype=np.uint8) for rb, rows, *_ in rects]
    data = [np.where(d == SENTINEL, 7, d).astype(np.uint8) for d in data]   # (no payload byte looks like untouched padding)
    sizes = [(do + dp * (rows - 1) + rb) if rows else do for rb, rows, sp, dp, so, do, sa, da in rects]
    outs = [np.zeros(max(s, 1), np.uint8) for s in sizes]
    cols = [np.array([r[k] for r in rects], np.uint32) for k in range(8)]
    fast = np.zeros(max(n, 1), np.uint32)
    dp_ = (P8 * max(n, 1))(*[d.ctypes.data_as(P8) for d in data])
    op_ = (P8 * max(n, 1))(*[o.ctypes.data_as(P8) for o in outs])
    blocks = emu.emu_move_rects(n, dp_, *[c.ctypes.data_as(PU) for c in cols], op_, fast.ctypes.data_as(PU))
    assert blocks >= 0
    for i, (rb, rows, sp, dp, so, do, sa, da) in enumerate(rects):
        if not sizes[i]:
            continue
        got = outs[i][:sizes[i]]
        want = np.full(sizes[i], SENTINEL, np.uint8)
        for y in range(rows):
            want[do + y * dp: do + y * dp + rb] = data[i][y * rb:(y + 1) * rb]
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, f"rectangle {i} {rects[i]}: first wrong byte at {bad[0]} (row {max(bad[0] - do, 0) // dp}), got {got[bad[0]]} want {want[bad[0]]}"
    return blocks, list(fast[:n])


@pytest.mark.parametrize("guard", [0, 1, 2])
def test_sixteen_rectangles_in_one_launch(guard):
    """Run in a child process per guard mode: a store or load that leaves its buffer is a segmentation fault there, not here."""
    if not os.path.exists(emu_build.CLANG):
        pytest.skip("no clang++ to build the emulator with")
    env = dict(os.environ, SMR_EMU_MOVE_GUARD=str(guard))
    r = subprocess.run([sys.executable, "-m", "tests.test_emu_move"], capture_output=True, text=True, env=env, cwd=ROOT, timeout=1200)
    assert r.returncode == 0, f"guard mode {guard}: rc {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-2000:]}"
    assert "all rectangles arrived" in r.stdout, r.stdout[-2000:]


# ---- what the child processes run (python -m tests.test_emu_move, SMR_EMU_MOVE_GUARD = the guard mode)
def inner_the_sixteen(emu):
    rects = the_sixteen()
    assert len(rects) == 16
    blocks, fast = run(emu, rects)
    assert blocks > 16
    # (paths by construction where the buffers' own alignment is given: mode 0 and 2 start every buffer on 256 bytes / a page)
    if os.environ["SMR_EMU_MOVE_GUARD"] != "1":
        assert fast[:5] == [1] * 5 and fast[12] == 1 and fast[14] == 0, fast
        assert fast[8:11] == [0, 0, 0] and fast[11] == 2 and fast[13] == 2 and fast[15] == 0, fast
    assert 1 in fast and 0 in fast and 2 in fast, fast


def inner_fewer_rectangles_and_none(emu):
    assert run(emu, [])[0] == 0
    assert run(emu, [(128, 0, 128, 128, 0, 0, 16, 16)])[0] == 0
    blocks, fast = run(emu, the_sixteen()[3:6], seed=9)
    assert blocks >= 3 and fast[0] == 1


def inner_random_rectangles(emu):
    rng = np.random.default_rng(int(os.environ["SMR_EMU_MOVE_GUARD"]) + 40)
    for _ in range(12):
        rects = []
        for _ in range(int(rng.integers(1, 17))):
            rb, rows = int(rng.integers(1, 300)), int(rng.integers(0, 40))
            if rng.random() < 0.4:   # aligned
                rb = (rb + 15) & ~15
                rects.append((rb, rows, rb + 16 * int(rng.integers(0, 4)), rb + 16 * int(rng.integers(0, 4)), 16 * int(rng.integers(0, 2)), 0, 16, 16))
            else:
                rects.append((rb, rows, rb + int(rng.integers(0, 20)), rb + int(rng.integers(0, 20)), int(rng.integers(0, 17)), int(rng.integers(0, 17)),
                              int(rng.choice([1, 16])), int(rng.choice([1, 16]))))
        run(emu, rects, seed=int(rng.integers(1 << 30)))


def test_move_rects_under_address_sanitizer():
    """The instrumented build, the way tests/test_emu_asan.py runs the other kernels: buffers at their exact sizes between red zones, misaligned
    vector accesses and overflowing index arithmetic abort."""
    rt = emu_build.asan_runtime()
    if rt is None:
        pytest.skip("the emulator's compiler has no shared AddressSanitizer runtime")
    preload = rt + (":" + os.environ["LD_PRELOAD"] if os.environ.get("LD_PRELOAD") else "")
    env = dict(os.environ, SMR_EMU_ASAN="1", SMR_EMU_MOVE_GUARD="0", LD_PRELOAD=preload, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0")
    r = subprocess.run([sys.executable, "-m", "tests.test_emu_move"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, cwd=ROOT, timeout=2400)
    out = r.stdout
    report = out[out.index("ERROR: AddressSanitizer"):][:4000] if "ERROR: AddressSanitizer" in out else out[-2500:]
    assert r.returncode == 0, f"rc {r.returncode}\n{report}"
    assert "all rectangles arrived" in out and "AddressSanitizer" not in out and "runtime error" not in out, report


if __name__ == "__main__":
    lib = load_emu()
    lib.emu_set_guard(int(os.environ["SMR_EMU_MOVE_GUARD"]), 0)
    inner_the_sixteen(lib)
    inner_fewer_rectangles_and_none(lib)
    inner_random_rectangles(lib)
    print("all rectangles arrived")
