"""WebView nodes in the host half of the library (smelter_amd/csrc/host/renderer.cpp: registration, paints into the pinned staging ring,
rectangles, the per-lane page copies, exclusivity across outputs) under AddressSanitizer + UBSan, the way
tests/test_animated_host_sanitizers.py runs the image pass: tests/san/web_view_driver.cpp — a stand-alone program with its own main — is
compiled by g++ together with the host sources and linked against tests/san/null_device.cpp, a stand-in for the GPU half that checks and
dereferences every surface it is handed, counts the ones it hands out and fails allocations on request.  The driver itself supplies the
five entry points this feature reaches through weak references (staging of exactly the size asked for, an upload that reads every byte, a
stream that is busy on request, smr_web_view).  The program is run directly."""
import json
import os
import subprocess

import pytest

from tests import san_build


@pytest.fixture(scope="module")
def driver():
    return san_build.build("web_view_driver", ("renderer.cpp", "null_device.cpp", "web_view_driver.cpp"))


def test_web_views_on_a_hostile_host_and_a_failing_device(driver):
    """Register / paint / positions / unregister churn, hostile sizes and pitches, more and fewer rectangles than children, a repaint between
    updates, busy streams under the staging ring, the renderer destroyed with paints pending — then every device allocation failing in
    turn: SMR_ERR_OOM or nothing, no surface or staging buffer leaked, no freed surface handed to the device."""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([driver], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, f"rc {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-6000:]}"
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-6000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert got["lives"] == 42 and got["refused_with_oom"] > 20 and got["checks"] > 2000 and got["uploads"] > 100 and got["idle_queries"] > 100, got
