"""The user-shader kernel on the lane emulator: smr_user_shader_prelude.h over smr_shader_dev.h — the two files the library embeds and hands
the runtime compiler — compiled for the CPU by tests/emu/emu_user_shader.cpp with one fixture of tests/user_shader_sources.py in the user's
place, run on guard-paged buffers against the oracle's forward rasterisation of the same shader (orc.builtin_shader) for the seven
restated built-ins.  Inputs and thresholds are those of tests/test_gpu_shaders.py for the same arithmetic; the oracle is the yardstick,
never the built-in kernel's output.  Test infrastructure only: tests/test_gpu_user_shaders.py holds the compiled programs on the device."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import emu_build
from tests import user_shader_sources as S

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
P8 = C.POINTER(C.c_uint8)
PI = C.POINTER(C.c_int)


def build(name):
    """tests/emu/_build/libsmr_emu_user_<name>.so: emu_user_shader.cpp with the fixture's text as the user's translation unit."""
    out_dir = os.path.join(emu_build.EMU, "_build")
    os.makedirs(out_dir, exist_ok=True)
    user = os.path.join(out_dir, f"user_shader_{name}.inc")
    text = "// generated from tests/user_shader_sources.py\n" + S.ALL[name]
    if not os.path.exists(user) or open(user).read() != text:
        with open(user, "w") as f:
            f.write(text)
    lib = os.path.join(out_dir, f"libsmr_emu_user_{name}.so")
    deps = [user, os.path.join(emu_build.EMU, "emu_user_shader.cpp"), os.path.join(emu_build.EMU, "emu_device.h"), os.path.join(emu_build.EMU, "emu_guard.h"),
            os.path.join(emu_build.EMU, "shim/hip/hip_runtime.h")] + [os.path.join(emu_build.CSRC, h) for h in
                                                                       ("smr_internal.h", "smr_shader_dev.h", "smr_user_shader_prelude.h", "smr_tables.h")]
    if not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(d) for d in deps):
        cmd = [emu_build.CLANG, "-std=c++17", "-fPIC", "-shared", "-DSMR_EMU=1", "-ffp-contract=off", "-Wno-unused-function", "-O2",
               f'-DSMR_EMU_USER_SOURCE="{user}"', "-I", os.path.join(emu_build.EMU, "shim"), "-I", emu_build.EMU, "-I", emu_build.CSRC,
               "-I", os.path.join(ROOT, "include"), "-o", lib, deps[1], "-lpthread"]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    h = C.CDLL(lib)
    h.emu_user_shader.argtypes = [C.c_int, C.POINTER(P8), PI, PI, C.c_int, C.c_int, C.c_int, C.c_float, P8, C.c_uint32, P8]
    h.emu_user_shader.restype = C.c_int
    return h


def run(emu, textures, W, H, params=b"", time_s=0.0, srgb=True):
    n = len(textures)
    tex = [np.ascontiguousarray(t, np.uint8) for t in textures]
    px = (P8 * max(n, 1))(*[t.ctypes.data_as(P8) for t in tex])
    ws = (C.c_int * max(n, 1))(*[t.shape[1] for t in tex])
    hs = (C.c_int * max(n, 1))(*[t.shape[0] for t in tex])
    pbuf = np.frombuffer(bytes(params) or b"\0", np.uint8).copy()
    out = np.zeros((H, W, 4), np.uint8)
    rc = emu.emu_user_shader(n, px, ws, hs, W, H, 1 if srgb else 0, float(time_s), pbuf.ctypes.data_as(P8), len(params), out.ctypes.data_as(P8))
    assert rc == 0, rc
    return out


@pytest.mark.parametrize("guard", [0, 1, 2])
def test_restated_builtins_match_the_oracle_on_guarded_buffers(guard):
    """Run in a child process per guard mode: a sample or store that leaves its surface is a segmentation fault there, not here."""
    if not os.path.exists(emu_build.CLANG):
        pytest.skip("no clang++ to build the emulator with")
    env = dict(os.environ, SMR_EMU_USER_SHADER_GUARD=str(guard))
    r = subprocess.run([sys.executable, "-m", "tests.test_emu_user_shader"], capture_output=True, text=True, env=env, cwd=ROOT, timeout=2400)
    assert r.returncode == 0, f"guard mode {guard}: rc {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    assert "seven shaders match the oracle" in r.stdout, r.stdout[-2000:]


# ---- what the child processes run (python -m tests.test_emu_user_shader, SMR_EMU_USER_SHADER_GUARD = the guard mode)
def inner(guard):
    from oracle import oracle as orc
    from tests.test_gpu_shaders import GRADIENT_RGB_EXPECTED, _check, _textures
    emus = {}
    for name in S.RESTATED:
        emus[name] = build(name)
        emus[name].emu_set_guard(guard, 1 if guard else 0)

    got = run(emus["gradient"], [], 8, 2)
    assert got.reshape(-1).tolist() == GRADIENT_RGB_EXPECTED
    _check(run(emus["gradient"], [], 640, 360), orc.builtin_shader(orc.SHADER_GRADIENT, [], 640, 360), "gradient")

    for n_src in (0, 1, 2, 3):
        tex = _textures(n_src, 32, 18)
        got = run(emus["color_by_texture_count"], tex, 64, 36)
        assert np.array_equal(got, orc.builtin_shader(orc.SHADER_COLOR_BY_TEXTURE_COUNT, tex, 64, 36)), f"color_by_texture_count n={n_src}"

    for W, H in ((640, 360), (333, 201)):
        tex = _textures(1, 160, 90)
        _check(run(emus["red_border"], tex, W, H), orc.builtin_shader(orc.SHADER_RED_BORDER, tex, W, H), f"red_border {W}x{H}")

    for n_src in (0, 1, 2, 4, 5):
        tex = _textures(n_src, 200, 120)
        _check(run(emus["layout_planes"], tex, 640, 360), orc.builtin_shader(orc.SHADER_LAYOUT_PLANES, tex, 640, 360), f"layout_planes n={n_src}")

    for t in (0.0, 0.7, 1.9, 4.0):
        tex = _textures(1, 320, 180)
        _check(run(emus["fade_to_ball"], tex, 640, 360, time_s=t), orc.builtin_shader(orc.SHADER_FADE_TO_BALL, tex, 640, 360, time=t),
               f"fade_to_ball t={t}", identical=0.98)

    for t in (0.0, 0.4, 1.3):
        tex = _textures(1, 320, 180)
        got = run(emus["silly"], tex, 640, 360, time_s=t)
        ref = orc.builtin_shader(orc.SHADER_SILLY, tex, 640, 360, time=t)
        d = np.abs(got.astype(np.int16) - ref.astype(np.int16))
        print(f"silly t={t}: within 1 {(d <= 1).mean():.5f}, identical {(d == 0).mean():.4f}")
        assert (d <= 1).mean() >= 0.999 and (d == 0).mean() >= 0.97, f"silly t={t}: {(d <= 1).mean():.5f} / {(d == 0).mean():.4f}"
    assert not run(emus["silly"], [], 64, 36).any()

    tex = _textures(3, 200, 200)
    circles = [(10, 20, 300, 300, (0.0, 0.0, 1.0, 1.0)), (200, 50, 250, 200, (0.0, 0.25, 0.0, 0.5)), (400, 100, 240, 260, (0.0, 0.0, 0.0, 0.0))]
    params = orc.circle_layout_params(circles)
    got = run(emus["circle_layout"], tex, 640, 360, params)
    _check(got, orc.builtin_shader(orc.SHADER_CIRCLE_LAYOUT, tex, 640, 360, params=params), "circle_layout", identical=0.99)
    assert not got[5, 5].any() and got[20, 10].tolist() == [0, 0, 255, 255]

    # the unorm render target (SMR_MODE_CPU_OPTIMIZED) through the same kernel
    tex = _textures(2, 200, 120)
    _check(run(emus["layout_planes"], tex, 640, 360, srgb=False), orc.builtin_shader(orc.SHADER_LAYOUT_PLANES, tex, 640, 360, srgb=False), "layout_planes unorm")


if __name__ == "__main__":
    inner(int(os.environ["SMR_EMU_USER_SHADER_GUARD"]))
    print("seven shaders match the oracle")
