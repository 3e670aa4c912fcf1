"""examples/web_view.c: the WebView entry points from plain C11.  It compiles with -Wall -Wextra -Werror against include/smr.h and links
against the library; without a GPU the program stops at smr_ctx_create — loudly, exit code 2 —, with one it renders three frames of a web
view with an embedded camera: one k_web_view launch each."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_example(tmp_path):
    exe = str(tmp_path / "web_view")
    libdir = os.path.join(ROOT, "smelter_amd")
    cmd = ["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "web_view.c"),
           "-o", exe, "-L", libdir, "-l:libsmr_hip.so", f"-Wl,-rpath,{libdir}", "-lm"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_example_compiles_and_stops_loudly_without_a_gpu(tmp_path):
    import torch
    exe = build_example(tmp_path)
    if torch.cuda.is_available():
        pytest.skip("GPU present: covered by the gpu test")
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 2 and "no HIP device" in p.stderr


@pytest.mark.gpu
def test_example_renders_three_frames(tmp_path):
    exe = build_example(tmp_path)
    out = tmp_path / "out.rgba"
    p = subprocess.run([exe, str(out)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    assert "3 k_web_view launches" in p.stdout, p.stdout
    assert out.stat().st_size == 640 * 360 * 4
