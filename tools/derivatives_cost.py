#!/usr/bin/env python3
"""What quad mode costs a shader that calls no derivative ("Derivatives"): `#define SMR_DERIVATIVES` deals the 64 x 4
pixels of a workgroup out as 32 x 2 blocks of 2 x 2 quads per wave — a wave's contiguous store run is 128 bytes in each of two rows instead of 256
in one — and keeps the lanes outside a plane alive as helpers.  Two fragments that call no derivative, each compiled without and with the
macro: the rotating example (tests/user_shader_sources_affine.py ROTATE: an affine plane with edges, the parent's 21.1 us) and a filtered copy
of source 0 over the whole target (no vertex stage, one smr_sample).  1920x1080 target, one 1080p source, one process, alternating rounds — the
method of tools/user_shader_cost.py and tools/clip_vertex_cost.py: per round and path, host microseconds per call (the time to enqueue CALLS
launches, nothing waited for) and microseconds per call with the device drained (enqueue + smr_sync over CALLS back-to-back launches).  The
pictures of a pair are compared first: they must be byte-equal.
usage: python tools/derivatives_cost.py [--rounds 5] [--calls 2000]"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY = r"""
__device__ float4 smr_fragment(const smr_shader_in &in, int plane_id, float2 uv, float2 position) {
    return smr_sample(in, plane_id, uv.x, uv.y);
}
"""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=2000)
    a = ap.parse_args()
    import numpy as np
    from smelter_amd import hip
    from tests import user_shader_sources_affine as SA
    from tools.kernel_resources import code_object_resources

    define = "#define SMR_DERIVATIVES\n"
    progs = {"rotate": hip.ShaderProgram(SA.ROTATE), "rotate, quad mode": hip.ShaderProgram(define + SA.ROTATE),
             "copy": hip.ShaderProgram(COPY), "copy, quad mode": hip.ShaderProgram(define + COPY)}
    for name, p in progs.items():
        r = code_object_resources(bytes(p.code))["smr_user_shader_kernel"]
        print(f"{name:18} {r['vgpr']} VGPRs, {r['sgpr']} SGPRs, {r['lds']} B LDS, {r['scratch']} B scratch")

    ctx = hip.Context(0)
    lib = ctx.lib
    W, H = 1920, 1080
    rng = np.random.default_rng(1)
    src = ctx.surface_from(rng.integers(0, 256, (H, W, 4), dtype=np.uint8))
    dst = ctx.surface(W, H)
    ptrs = (C.c_void_p * 1)(src.handle)
    t = C.c_float(0.7)

    def call(name):
        handle = progs[name].handle
        return lambda: lib.smr_user_shader(ctx.handle, handle, None, 0, ptrs, 1, dst.handle, t)

    pictures = {}
    for name in progs:
        assert call(name)() == 0
        ctx.sync()
        pictures[name] = dst.download()
    for name in ("rotate", "copy"):
        differ = int((pictures[name] != pictures[name + ", quad mode"]).sum())
        print(f"{name}: {int(pictures[name].any(axis=-1).sum())} of {W * H} pixels drawn, {differ} bytes differ in quad mode")
        assert differ == 0, "quad mode does not draw the same picture"

    paths = [(n, call(n)) for n in progs]

    def one_round(fn):
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(a.calls):
            fn()
        t1 = time.perf_counter()
        ctx.sync()
        t2 = time.perf_counter()
        return (t1 - t0) / a.calls * 1e6, (t2 - t0) / a.calls * 1e6

    for _, fn in paths:  # warm-up: module load, clocks
        for _ in range(200):
            assert fn() == 0
    ctx.sync()
    rows = {n: [] for n, _ in paths}
    for r in range(a.rounds):
        for name, fn in paths if r % 2 == 0 else paths[::-1]:
            rows[name].append(one_round(fn))
    print(f"{a.rounds} alternating rounds x {a.calls} calls, {W}x{H} target, one {W}x{H} source, t = 0.7")
    print(f"{'path':36} {'host us/call (enqueue)':>34} {'us/call, device drained':>34}")
    med = {}
    for name, _ in paths:
        host = [x[0] for x in rows[name]]
        full = [x[1] for x in rows[name]]
        med[name] = (statistics.median(host), statistics.median(full))
        print(f"{'smr_user_shader(' + name + ')':36} {f'median {med[name][0]:.2f} (range {min(host):.2f} - {max(host):.2f})':>34} "
              f"{f'median {med[name][1]:.2f} (range {min(full):.2f} - {max(full):.2f})':>34}")
    for name in ("rotate", "copy"):
        print(f"{name}: quad mode / default, device drained: {med[name + ', quad mode'][1] / med[name][1]:.3f}")
    for p in progs.values():
        p.close()
    ctx.close()


if __name__ == "__main__":
    main()
