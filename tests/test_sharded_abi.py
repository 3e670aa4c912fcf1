"""The sharded renderer's entry points (smr_renderer_add_shard, smr_renderer_input_ctx) and the mover's launch counter at the drop-in
boundary, without a GPU: exported, bound by the generated Rust binding with the header's arity, the ABI version unchanged (additions only),
null arguments refused with a message.  tests/test_gpu_sharded_renderer.py holds what they do."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"smr_renderer_add_shard": 2, "smr_renderer_input_ctx": 3}


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from smelter_amd import _ffi
    return _ffi.load()


def test_new_symbols_are_declared_exported_and_listed(lib):
    from smelter_amd import _ffi
    hdr = open(os.path.join(ROOT, "include", "smr.h")).read()
    for name, arity in NEW.items():
        m = re.search(r"SMR_API\s+int\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, flags=re.S)
        assert m, f"include/smr.h does not declare {name}"
        assert len(m.group(1).split(",")) == arity
        assert name in _ffi.EXPORTS and hasattr(lib, name)
        assert len(getattr(lib, name).argtypes) == arity


def test_generated_rust_binding_binds_them():
    patch = open(os.path.join(ROOT, "integration", "smelter-render-hip.patch")).read()
    for name, arity in NEW.items():
        m = re.search(r"^\+\s*pub fn " + name + r"\(([^)]*)\) -> c_int;", patch, flags=re.M)
        assert m, f"hip/sys.rs does not bind {name}"
        assert len(m.group(1).split(",")) == arity
    assert "+pub const SMR_KERNEL_MOVE_RECTS: u32 = 8;" in patch and "+pub const SMR_KERNEL_COUNT_: u32 = 10;" in patch


def test_abi_version_is_still_two_and_the_counter_has_its_slot(lib):
    from smelter_amd import hip
    hdr = open(os.path.join(ROOT, "include", "smr.h")).read()
    assert lib.smr_abi_version() == 2 and "#define SMR_ABI_VERSION 2" in hdr
    assert re.search(r"SMR_KERNEL_MOVE_RECTS\s*=\s*8\b", hdr) and re.search(r"SMR_KERNEL_COUNT_\s*=\s*10\b", hdr)
    assert hip.KERNEL_NAMES[8] == "move_rects" and len(hip.KERNEL_NAMES) == 10  # (slot 9: SMR_KERNEL_INGEST_WAVE_DIRECT, an addition behind it)
    assert "smr_renderer_add_shard" in hdr[hdr.index("#define SMR_ABI_VERSION") - 2500:hdr.index("#define SMR_ABI_VERSION")], "the header's history names the additions"


def test_null_arguments_fail_with_a_message(lib):
    """No device is needed to be refused: a null renderer, and — on a renderer over a context handle that is never dereferenced before the
    argument check — a null shard / id / out."""
    out = C.c_void_p()
    assert lib.smr_renderer_add_shard(None, None) < 0
    assert lib.smr_renderer_input_ctx(None, b"in0", C.byref(out)) < 0
    assert lib.smr_renderer_last_error(None) == b"null renderer"
    import torch
    if not torch.cuda.is_available():
        return  # (a renderer needs a context, a context needs a device: the rest runs in tests/test_gpu_sharded_renderer.py)
    from smelter_amd import hip
    from smelter_amd.renderer import Renderer
    ctx = hip.Context(0)
    r = Renderer(ctx)
    assert lib.smr_renderer_add_shard(r._h, None) < 0 and b"null argument" in lib.smr_renderer_last_error(r._h)
    assert lib.smr_renderer_input_ctx(r._h, None, C.byref(out)) < 0 and b"null argument" in lib.smr_renderer_last_error(r._h)
    assert lib.smr_renderer_input_ctx(r._h, b"in0", None) < 0 and b"null argument" in lib.smr_renderer_last_error(r._h)
    assert lib.smr_renderer_input_ctx(r._h, b"nobody", C.byref(out)) < 0 and b"not registered" in lib.smr_renderer_last_error(r._h)
    r.close()
    ctx.close()
