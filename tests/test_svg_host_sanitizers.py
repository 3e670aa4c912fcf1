"""SVG image assets in the host half of the library (smelter_amd/csrc/host/renderer.cpp: registration, the rasteriser's calls inside
update_scene, pinned staging, the raster cache and its release, unregistration) under AddressSanitizer + UBSan, the way
tests/test_web_view_host_sanitizers.py runs WebView nodes: tests/san/svg_driver.cpp — a stand-alone program with its own main — is compiled
by g++ together with the host sources and linked against tests/san/null_device.cpp, a stand-in for the GPU half that checks and
dereferences every surface it is handed, counts the ones it hands out and fails allocations on request.  The driver itself supplies the
entry points this feature reaches through weak references (staging of exactly the size asked for, an upload that reads every byte,
smr_svg_nodes).  The program is run directly: nothing is loaded into Python."""
import json
import os
import subprocess

import pytest

from tests import san_build


@pytest.fixture(scope="module")
def driver():
    return san_build.build("svg_driver", ("renderer.cpp", "null_device.cpp", "svg_driver.cpp"))


def test_svg_images_on_a_failing_host_and_a_failing_device(driver):
    """Register / update / unregister churn; a rasteriser that fails on its k-th call, for every k (the previous scene stays, no surface or
    staging buffer leaks); the same asset at 40 sizes over 40 updates (`resident` returns to what the last scene uses); unregister refused
    while in use; the renderer destroyed with rasters resident — then every device allocation and every staging allocation failing in turn:
    SMR_ERR_OOM or nothing, no leak, no freed surface handed to the device."""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([driver], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, f"rc {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-6000:]}"
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-6000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert got["lives"] == 54 and got["refused_with_oom"] > 20 and got["checks"] > 1500, got
    # two strict lives: five failing calls each, forty sizes each; the fix-up ran (in the GPU-optimized lives only)
    assert got["refused_callbacks"] == 10 and got["size_updates"] == 80 and got["uploads"] > 150 and got["fix_calls"] > 40, got
