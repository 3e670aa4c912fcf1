"""The pair chroma of the output conversion's fast path (smelter_amd/csrc/smr_yuv_fast.h: constants422 / convert422, what the compositor's packed
4:2:2 store computes Cb and Cr with): tools/check_yuv_fast_422.cpp — compiled against THE header the kernels include — proves that an
unflagged byte is the byte of the reference sequence (byte / 255, a * .5 + b * .5, rgba_to_yuv.wgsl's chroma formulas, the unorm8 store) over
the pair's byte sums times every value the f32 mean can take for a sum.  Here every 8th red sum (`quick`: well under a second); the whole
domain, 133 M sum triples per plane, is profiles/yuv_fast_422_check.txt.  Luma is convert<0>, unchanged: tests/test_yuv_fast.py."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pair_fast_path_never_disagrees_outside_its_guard_band(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path / "check_yuv_fast_422")
    r = subprocess.run([gxx, "-O2", "-fopenmp", "-ffp-contract=off", "-I", os.path.join(ROOT, "smelter_amd", "csrc"), "-o", exe,
                        os.path.join(ROOT, "tools", "check_yuv_fast_422.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, "quick"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "OK: the pair fast path never disagrees" in r.stdout, r.stdout[-2000:]
    planes = re.findall(r"^plane (\d) (\d+) sum triples, (\d+) combinations: flagged ([0-9.]+) %.*mismatches NOT flagged (\d+);", r.stdout, re.M)
    assert [p[0] for p in planes] == ["1", "2"], r.stdout[-2000:]
    for plane, sums, combos, flagged, unflagged_mismatches in planes:
        assert int(unflagged_mismatches) == 0, r.stdout[-2000:]
        assert int(combos) >= int(sums) >= 511 * 511 * 64, (plane, sums, combos)  # (every 8th of 511 red sums: 64 of them)
        # a cap, not a measurement: "flag everything" must not pass (the 2x2 fast path flags 0.024 %)
        assert 0.0 < float(flagged) < 0.1, (plane, flagged)
