"""Animated images in the host half of the library (smelter_amd/csrc/host/renderer.cpp: registration, the image pass, per-lane node surfaces)
under AddressSanitizer + UBSan, the way tests/test_host_sanitizers.py runs the renderer: tests/san/animated_driver.cpp — a stand-alone
program — is compiled by g++ together with the host sources and linked against tests/san/null_device.cpp, a stand-in for the GPU half that
checks and dereferences every surface it is handed, counts the ones it hands out and fails allocations on request.  It has no
smr_image_nodes, so the image pass takes its one-rescale-per-job route (the weak reference).  The program is run directly."""
import json
import os
import subprocess

import pytest

from tests import san_build


@pytest.fixture(scope="module")
def driver():
    return san_build.build("animated_driver", ("renderer.cpp", "null_device.cpp", "animated_driver.cpp"))


def test_animated_images_on_a_hostile_host_and_a_failing_device(driver):
    """Refused registrations (no frames, 1001 frames, delays beyond INT64_MAX, ids taken), animated nodes at their own size and scaled, alone
    and under Shader and View nodes, over two lanes with updates in between — the image pass's launch counts included —, then every device
    allocation failing in turn: SMR_ERR_OOM or nothing, no surface leaked, no freed surface handed to the device."""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([driver], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, f"rc {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-6000:]}"
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-6000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert got["lives"] == 92 and got["refused_with_oom"] > 60 and got["checks"] > 5000, got
