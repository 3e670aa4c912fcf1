"""User shaders without a GPU (include/smr.h "user shaders"): a fragment function written in HIP C++ is compiled to a gfx950 code object by
the ROCm runtime compiler at registration — compilation, its error reporting and the kernel's resource footprint need no device.  The
registry path (register source -> compile error -> registry unchanged; a program destroyed while registered elsewhere) runs on the null
device of tests/san under AddressSanitizer + UBSan (tests/san/shader_registry_driver.cpp)."""
import json
import os
import shutil
import subprocess

import pytest

from tests import user_shader_sources as S

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
KERNEL = "smr_user_shader_kernel"


@pytest.fixture(scope="module")
def hip():
    import __graft_entry__ as ge
    ge.build()
    from smelter_amd import hip as h
    return h


@pytest.fixture(scope="module")
def programs(hip):
    out = {}
    for name, src in S.ALL.items():
        out[name] = hip.ShaderProgram(src)
    yield out
    for p in out.values():
        p.close()


def test_every_fixture_compiles_to_a_gfx950_code_object(programs):
    for name, p in programs.items():
        code = p.code
        assert code[:4] == b"\x7fELF", name
        assert KERNEL.encode() in code, f"{name}: no {KERNEL} symbol"
        assert int.from_bytes(code[48:52], "little") & 0xff == 0x4f, f"{name}: e_flags {code[48:52].hex()} is not gfx950"  # EF_AMDGPU_MACH_AMDGCN_GFX950
        assert p.log == "", f"{name}: {p.log}"
        assert p.launches == 0


def test_fixtures_use_no_scratch_and_their_registers_are_on_record(programs, hip):
    """0 scratch bytes is a condition (these fragments are a few dozen operations).  The VGPR counts are printed beside k_shader_planes' —
    the built-in kernel that carries all seven fragments behind a switch — and quoted in DESIGN.md section 3e; they are not asserted."""
    from smelter_amd import build
    from tools import kernel_resources as kr
    builtin = {k: v for k, v in kr.library_resources(build.LIB).items() if "k_shader_planes" in k}
    assert len(builtin) == 1
    b = next(iter(builtin.values()))
    print(f"\n{'k_shader_planes (built-in, seven fragments)':46} VGPR {b['vgpr']:3} SGPR {b['sgpr']:3} scratch {b['scratch']} kernarg {b['kernarg']}")
    for name, p in programs.items():
        res = kr.code_object_resources(p.code)
        assert list(res) == [KERNEL], res
        r = res[KERNEL]
        print(f"{name:46} VGPR {r['vgpr']:3} SGPR {r['sgpr']:3} scratch {r['scratch']} kernarg {r['kernarg']}")
        assert r["scratch"] == 0, f"{name}: {r['scratch']} scratch bytes per lane"
        assert r["lds"] == 0 and r["kernarg"] <= 4096, r


@pytest.mark.parametrize("name", sorted(S.BROKEN))
def test_a_source_that_does_not_compile_is_refused_with_the_compilers_log(hip, name):
    src, mentions = S.BROKEN[name]
    with pytest.raises(hip.ShaderCompileError) as e:
        hip.ShaderProgram(src)
    assert e.value.code == -1  # SMR_ERR_INVALID
    assert e.value.log.strip(), "empty log"
    for m in mentions:
        assert m in e.value.log, f"{name}: the log does not mention {m!r}:\n{e.value.log}"


def test_the_c_abi_hands_out_a_program_with_the_log_when_the_source_is_refused(hip):
    import ctypes as C
    from smelter_amd import _ffi
    lib = _ffi.load()
    h = C.c_void_p()
    assert lib.smr_shader_program_create(S.BROKEN["unknown_identifier"][0].encode(), C.byref(h)) == _ffi.SMR_ERR_INVALID
    assert h.value, "no program object to read the log from"
    assert b"smr_sample_nearest" in lib.smr_shader_program_log(h)
    p, n = C.c_void_p(), C.c_size_t()
    assert lib.smr_shader_program_code(h, C.byref(p), C.byref(n)) == _ffi.SMR_ERR_INVALID
    lib.smr_shader_program_destroy(h)
    assert lib.smr_shader_program_create(None, C.byref(h)) == _ffi.SMR_ERR_INVALID and not h.value


def test_the_library_gained_no_link_dependency(hip):
    """libhiprtc.so is loaded with dlopen when the first program is created (as librccl is): not a DT_NEEDED entry."""
    from smelter_amd import build
    out = subprocess.run(["readelf", "-d", build.LIB], capture_output=True, text=True, check=True).stdout
    needed = [line for line in out.splitlines() if "NEEDED" in line]
    assert needed and not any("hiprtc" in line for line in needed), needed


def test_kernel_resources_tool_reads_a_user_shaders_code_object(programs, tmp_path):
    path = tmp_path / "silly.co"
    path.write_bytes(programs["silly"].code)
    r = subprocess.run([os.sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), str(path)], capture_output=True, text=True, check=True)
    assert KERNEL in r.stdout and "VGPR" in r.stdout, r.stdout


def test_registry_on_the_null_device_under_the_host_sanitizers(hip, tmp_path):
    """register source -> compile error -> registry unchanged; programs replaced and destroyed while registered elsewhere."""
    from smelter_amd import build
    from tests import san_build as ths
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    out_dir = os.path.join(HERE, "san", "_build", "shader_registry")
    os.makedirs(out_dir, exist_ok=True)
    probe = os.path.join(out_dir, "probe.cpp")
    with open(probe, "w") as f:
        f.write("int main() { return 0; }\n")
    if subprocess.run([gxx, ths.SANITIZE, probe, "-o", os.path.join(out_dir, "probe")], capture_output=True).returncode != 0:
        pytest.skip("this g++ has no sanitizer runtimes")
    build.write_prelude_inc(out_dir)
    srcs = ths.HOST_SOURCES + [os.path.join(ths.HOST, "renderer.cpp"), os.path.join(ths.HOST, "shader_program.cpp"),
                               os.path.join(HERE, "san", "null_device.cpp"), os.path.join(HERE, "san", "shader_registry_driver.cpp")]
    exe = os.path.join(out_dir, "shader_registry_driver")
    r = subprocess.run([gxx] + ths.FLAGS + ["-I", out_dir] + srcs + ["-o", exe, "-ldl"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    # (leak detection off: the runtime compiler keeps process-lifetime caches that are not this library's to free)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, f"rc {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-6000:]}"
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-6000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert got["compiler"] is True, "the runtime compiler (libhiprtc.so) did not load"
    assert got == {"compiler": True, "user_launches": 6, "failures": 0}, got
