"""One resample plan through k_ingest_wave on the lane emulator, by the build the host would launch — shared by tests/test_emu_resample_zoo.py
and tests/test_emu_small_tiles.py.  Test infrastructure only."""
import ctypes as C
import os

import numpy as np

from oracle import oracle as orc

CLANG = "/opt/rocm/lib/llvm/bin/clang++"
P8 = C.POINTER(C.c_uint8)


def load():
    """-> the emulator library with emu_ingest_wave bound (and the oracle built), or None where there is no compiler to build it with"""
    if not os.path.exists(CLANG):
        return None
    from tests import emu_build
    h = C.CDLL(emu_build.build("smr_emu"))
    h.emu_ingest_wave.argtypes = [P8, P8, P8, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, P8, C.c_int, C.c_int,
                                  C.c_int, C.c_int, C.POINTER(C.c_int)]
    orc.build()
    return h


def _p(a):
    return a.ctypes.data_as(P8)


def _rgb12(node):
    h, w = node.shape[:2]
    return np.ascontiguousarray(node[..., :3].reshape(h, w // 4, 4, 3).transpose(0, 1, 3, 2)).reshape(h, 3 * w)


def emulate(emu, geo, plan, node, alpha, rgb12=False, refusal=False):
    """The tile k_ingest_wave makes of `node` by `plan`, through the build the host would launch: the class build where the k-step counts
    have one (`ks`), one tile per wave where a pair's window is too wide, the single-axis build for one pass, the RGBA16F build behind the
    oracle's box mean; a plan whose first pass is vertical on the transposed node.  `refusal`: where the windows are too wide for the
    kernel either way (can_fuse_wave_rgba says no and the host takes the pass kernels), return None instead of failing."""
    (sw, sh), (dw, dh) = geo.src, geo.dst
    boxed = tuple(plan.levels) != (0, 0)
    if boxed:
        tex = orc.downsample(node, orc.PX_RGBA8_SRGB, 1 << plan.levels[0], 1 << plan.levels[1])   # (h, w, 4) f16 patterns
        sw, sh = plan.reduced
        mode = 5 if alpha else 3
    else:
        tex = _rgb12(node) if rgb12 else node
        mode = 4 if alpha else 6 if rgb12 else 2
    transposed = plan.axis[0] == 1
    if transposed:
        assert not rgb12
        tex, sw, sh, dw, dh = tex.transpose(1, 0, 2), sh, sw, dh, dw
    flat = np.ascontiguousarray(tex).view(np.uint8)
    if plan.kind == 1:
        tail, spec = (plan.scale[0], plan.offset[0], 1.0, float(plan.perp_offset[0])), 2
    else:
        tail, spec = (plan.scale[0], plan.offset[0], plan.scale[1], plan.offset[1]), (1 if geo.ks else 0)
    got = np.zeros((dh, dw, 4), np.uint8)
    info = (C.c_int * 4)()
    rc = emu.emu_ingest_wave(_p(flat), _p(flat), _p(flat), sw, sh, 0, mode, *tail, _p(got), dw, dh, 2, spec, info)
    if rc == -1 and spec == 0:   # more k-steps than a column pair holds: one tile per unit, as the host builds the band then
        rc = emu.emu_ingest_wave(_p(flat), _p(flat), _p(flat), sw, sh, 0, mode, *tail, _p(got), dw, dh, 2, 3, info)
    if rc == -1 and refusal:
        return None
    assert rc == 0, (geo.name, rc, list(info))
    if geo.ks:
        assert tuple(info[:3]) == geo.ks, (geo.name, list(info))
    return got.transpose(1, 0, 2) if transposed else got
