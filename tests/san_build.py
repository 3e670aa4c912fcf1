"""Builds the stand-alone sanitizer programs of tests/san: a driver with its own main, compiled by g++ under AddressSanitizer + UBSan together
with the host sources of the library (smelter_amd/csrc/host: plain C++17, no HIP involved).  The programs are run directly by their tests:
nothing is loaded into Python."""
import os
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HOST = os.path.join(ROOT, "smelter_amd", "csrc", "host")
SAN = os.path.join(HERE, "san")
HOST_SOURCES = [os.path.join(HOST, f) for f in ("scene.cpp", "scene_build.cpp", "scene_capi.cpp", "text.cpp", "text_capi.cpp")]  # what every program links
SANITIZE = "-fsanitize=address,undefined,float-cast-overflow"
FLAGS = ["-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", SANITIZE, "-fno-sanitize-recover=undefined,float-cast-overflow",
         "-I", os.path.join(ROOT, "include"), "-I", HOST, "-I", SAN]


def _path(name):
    in_san = os.path.join(SAN, name)
    return in_san if os.path.exists(in_san) else os.path.join(HOST, name)


def build(name, driver_sources):
    """-> the path of the program tests/san/_build/<name>/<name>, linked from HOST_SOURCES and `driver_sources` (file names of tests/san or of
    the host directory: the driver, and what it needs beyond the scene engine and the text pipeline, such as renderer.cpp and null_device.cpp).
    Rebuilt when a source, a host header, a header of tests/san or smr.h is newer.  Skips the calling test without g++ or its sanitizer
    runtimes."""
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    out = os.path.join(SAN, "_build", name)
    os.makedirs(out, exist_ok=True)
    probe = os.path.join(out, "probe.cpp")
    with open(probe, "w") as f:
        f.write("int main() { return 0; }\n")
    if subprocess.run([gxx, SANITIZE, probe, "-o", os.path.join(out, "probe")], capture_output=True).returncode != 0:
        pytest.skip("this g++ has no sanitizer runtimes")
    exe = os.path.join(out, name)
    sources = HOST_SOURCES + [_path(f) for f in driver_sources]
    deps = sources + [os.path.join(d, f) for d in (HOST, SAN) for f in os.listdir(d) if f.endswith(".h")] + [os.path.join(ROOT, "include", "smr.h")]
    if os.path.exists(exe) and os.path.getmtime(exe) >= max(os.path.getmtime(p) for p in deps):
        return exe

    def compile_one(src):
        obj = os.path.join(out, os.path.basename(src) + ".o")
        r = subprocess.run([gxx] + FLAGS + ["-c", src, "-o", obj], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        return obj
    with ThreadPoolExecutor(max_workers=8) as ex:
        objs = list(ex.map(compile_one, sources))
    r = subprocess.run([gxx, SANITIZE] + objs + ["-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe
