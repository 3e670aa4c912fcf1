"""The frame clock of animated images (include/smr.h: smr_animated_frame_index; AnimatedAsset::render,
smelter-render/src/transformations/image/animated_image.rs:120-149) against a restatement in Python integers — CPU only.

With pts_0 = 0, pts_k = delays[0] + .. + delays[k - 1] and D = the sum of all delays (1 if that is 0): t = max(pts - start_pts, 0) mod D, and
the frame is the k that minimises |pts_k - t|, the first such k on a tie; no wrap-around near the end of the loop."""
import ctypes as C

import numpy as np
import pytest

import smelter_amd
from smelter_amd import _ffi
from smelter_amd.scene import SceneError, animated_frame_index

MS = 1_000_000
WORKED = [100 * MS, 200 * MS, 50 * MS, 150 * MS]   # frame starts at 0, 100, 300, 350 ms; D = 500 ms
I64_MAX, U64_MAX = 2**63 - 1, 2**64 - 1


def model(delays, pts, start):
    total = sum(delays) or 1
    t = max(pts - start, 0) % total
    best, best_diff, frame_pts = 0, None, 0
    for k, d in enumerate(delays):
        diff = abs(frame_pts - t)
        if best_diff is None or diff < best_diff:   # strictly closer: the first of equally close frames stays
            best, best_diff = k, diff
        frame_pts += d
    return best


@pytest.mark.parametrize("t_ms,frame", [(0, 0), (49, 0), (50, 0), (51, 1), (200, 1), (201, 2), (325, 2), (326, 3), (499, 3), (500, 0), (551, 1)])
def test_worked_example(t_ms, frame):
    assert model(WORKED, t_ms * MS, 0) == frame
    assert animated_frame_index(WORKED, t_ms * MS) == frame
    assert smelter_amd.animated_frame_index(WORKED, t_ms * MS + 7 * MS, 7 * MS) == frame   # the clock counts from start_pts
    assert animated_frame_index(WORKED, t_ms * MS + 3 * 500 * MS) == frame                 # ... and loops


def test_ties_to_the_nanosecond():
    assert animated_frame_index(WORKED, 50 * MS + 1) == 1 and animated_frame_index(WORKED, 50 * MS) == 0
    assert animated_frame_index(WORKED, 325 * MS + 1) == 3 and animated_frame_index(WORKED, 325 * MS) == 2
    assert animated_frame_index(WORKED, 500 * MS - 1) == 3   # no wrap-around: the last frame, not frame 0


def test_all_zero_delays_run_on_a_one_nanosecond_loop():
    for n in (1, 2, 5):
        for pts in (0, 1, 12345, I64_MAX):
            assert animated_frame_index([0] * n, pts) == 0 == model([0] * n, pts, 0)
    # zero delays inside an animation: frames 1 and 2 start together, the first of them is chosen
    d = [10, 0, 10]
    assert [animated_frame_index(d, t) for t in (0, 5, 6, 10, 14, 15, 16, 19, 20)] == [model(d, t, 0) for t in (0, 5, 6, 10, 14, 15, 16, 19, 20)]
    assert animated_frame_index(d, 6) == 1 and animated_frame_index(d, 19) == 1


def test_one_huge_delay():
    for d in ([I64_MAX], [U64_MAX], [1, U64_MAX], [U64_MAX, U64_MAX, 5], [I64_MAX, 1, I64_MAX]):
        for pts, start in ((0, 0), (I64_MAX, 0), (I64_MAX, -I64_MAX - 1), (I64_MAX - 1, -5), (2**62, 1)):
            assert animated_frame_index(d, pts, start) == model(d, pts, start), (d, pts, start)
    assert animated_frame_index([1, U64_MAX], I64_MAX) == 1


def test_pts_before_start_is_time_zero():
    for start in (1, 500 * MS, I64_MAX):
        for pts in (0, start - 1, -I64_MAX - 1, -1):
            assert animated_frame_index(WORKED, pts, start) == 0
    assert animated_frame_index(WORKED, -100 * MS, -151 * MS) == 1   # negative pts on a negative start: 51 ms in


def test_random_cases_against_the_model():
    rng = np.random.default_rng(20240611)
    for case in range(2000):
        n = int(rng.integers(1, 13))
        scale = [1, 10, MS, 40 * MS, 2**40][int(rng.integers(0, 5))]
        delays = [int(x) for x in rng.integers(0, 8, n) * scale + rng.integers(0, 2, n) * rng.integers(0, 1000, n)]
        start = int(rng.integers(-2**40, 2**40))
        total = sum(delays) or 1
        pick = int(rng.integers(0, 4))
        if pick == 0:      # on and around a midpoint between two frame starts (the ties)
            starts = np.cumsum([0] + delays[:-1])
            k = int(rng.integers(0, n))
            nxt = int(starts[k + 1]) if k + 1 < n else total
            t = (int(starts[k]) + nxt) // 2 + int(rng.integers(-1, 2))
        elif pick == 1:    # around the end of the loop
            t = total * int(rng.integers(1, 4)) + int(rng.integers(-2, 3))
        else:
            t = int(rng.integers(0, 4 * total + 1))
        pts = start + max(t, 0) if pick != 3 else start + int(rng.integers(-5, 6))
        assert animated_frame_index(delays, pts, start) == model(delays, pts, start), (case, delays, pts, start)


def test_no_frames_and_null():
    lib = _ffi.load()
    one = (C.c_uint64 * 1)(5)
    assert lib.smr_animated_frame_index(None, 3, 0, 0) < 0
    assert lib.smr_animated_frame_index(one, 0, 0, 0) < 0
    with pytest.raises(SceneError):
        animated_frame_index([], 0)


def test_registration_refusals_that_need_no_device():
    """Without a renderer every registration call is SMR_ERR_INVALID before anything is touched; the refusals that need one (no frames, more
    than 1000, an overflowing delay sum, a duplicate id) run against the stand-in device in tests/test_animated_host_sanitizers.py and on the
    GPU in tests/test_gpu_animated_images.py."""
    lib = _ffi.load()
    px = (C.c_uint8 * 16)()
    delays = (C.c_uint64 * 2)(1, 1)
    count = C.c_uint64(77)
    assert lib.smr_renderer_register_animated_image(None, b"gif", px, 1, 1, 2, delays) == _ffi.SMR_ERR_INVALID
    assert lib.smr_renderer_register_animated_image(None, b"gif", px, 1, 1, 0, delays) == _ffi.SMR_ERR_INVALID
    assert lib.smr_renderer_image_launches(None, C.byref(count)) == _ffi.SMR_ERR_INVALID and count.value == 77
    assert lib.smr_scene_node_start_pts(None, 0, None) == _ffi.SMR_ERR_INVALID
    for name in ("smr_renderer_register_animated_image", "smr_animated_frame_index", "smr_scene_node_start_pts", "smr_renderer_image_launches"):
        assert name in _ffi.EXPORTS
