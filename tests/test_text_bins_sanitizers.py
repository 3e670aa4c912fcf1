"""The host pieces of the batched Text path under AddressSanitizer + UBSan: tx_plan (smelter_amd/csrc/host/text_bins.h — the tile bins
k_text_nodes walks) and the Text raster cache of smelter_amd/csrc/host/renderer.cpp.  tests/san/text_bins_driver.cpp — a stand-alone program
with its own main — is compiled by g++ together with the host sources and linked against tests/san/null_device.cpp, a stand-in for the GPU
half that checks and dereferences every surface it is handed and counts the ones it hands out (the renderer then draws a new raster with
one smr_blit_glyphs call: smr_text_nodes is a weak reference).  The program is run directly: nothing is loaded into Python."""
import json
import os
import subprocess

import pytest

from tests import san_build

FONTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fonts")


@pytest.fixture(scope="module")
def driver():
    return san_build.build("text_bins_driver", ("renderer.cpp", "null_device.cpp", "text_bins_driver.cpp"))


def test_text_bins_and_the_raster_cache(driver):
    """Glyphs with INT32_MAX / INT32_MIN coordinates and sizes, 10^5 glyphs in one tile, a run whose bins would not fit 32 bits, 300 random
    runs against a brute-force 64-bit intersection test: bin_first monotone, every index in range and ascending.  Then the cache, in both
    rendering modes: updates that add, drop and duplicate Text nodes over two outputs, set_text on a node whose raster is shared, a font-book
    swap, both outputs unregistered — the reference counts recounted at every step, `resident` 0 at the end, no surface left."""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([driver, FONTS], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, f"rc {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-6000:]}"
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-6000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert got["plans"] == 8 + 1 + 300 and got["entries"] > 100000 and got["cache_steps"] == 2 * 17 and got["checks"] > 100000, got
