#!/usr/bin/env python3
"""What a user shader costs against the built-in kernel that carries the same fragment: `silly` restated as a user
shader (tests/user_shader_sources.py) against smr_builtin_shader(SMR_SHADER_SILLY), 1920x1080 target, one 1080p source, one process,
alternating rounds.  Per round and path: host microseconds per call (the time to enqueue CALLS launches, nothing waited for) and
microseconds per call with the device drained (enqueue + smr_sync over CALLS back-to-back launches: the kernel's time when the GPU is the
bottleneck).  Device time per kernel comes from a run of its own under the profiler:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o s -- python tools/user_shader_cost.py --rounds 1 --calls 500
Also: compile time of a registration, cold (the first program of the process: the runtime compiler loads) and of the same text again.
usage: python tools/user_shader_cost.py [--rounds 5] [--calls 2000]"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=2000)
    a = ap.parse_args()
    import numpy as np
    from smelter_amd import hip
    from tests import user_shader_sources as S

    t0 = time.perf_counter()
    prog = hip.ShaderProgram(S.SILLY)
    cold = time.perf_counter() - t0
    again = []
    for _ in range(3):
        t0 = time.perf_counter()
        hip.ShaderProgram(S.SILLY).close()
        again.append(time.perf_counter() - t0)
    print(f"compile: cold {cold * 1e3:.0f} ms (loads the runtime compiler), the same text again {statistics.median(again) * 1e3:.0f} ms "
          f"(min {min(again) * 1e3:.0f}, max {max(again) * 1e3:.0f})")

    ctx = hip.Context(0)
    lib = ctx.lib
    W, H = 1920, 1080
    rng = np.random.default_rng(1)
    src = ctx.surface_from(rng.integers(0, 256, (H, W, 4), dtype=np.uint8))
    dst = ctx.surface(W, H)
    ptrs = (C.c_void_p * 1)(src.handle)
    t = C.c_float(0.4)

    def builtin():
        return lib.smr_builtin_shader(ctx.handle, hip.SHADER_SILLY, None, 0, ptrs, 1, dst.handle, t)

    def user():
        return lib.smr_user_shader(ctx.handle, prog.handle, None, 0, ptrs, 1, dst.handle, t)

    def one_round(fn):
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(a.calls):
            fn()
        t1 = time.perf_counter()
        ctx.sync()
        t2 = time.perf_counter()
        return (t1 - t0) / a.calls * 1e6, (t2 - t0) / a.calls * 1e6

    for fn in (builtin, user):  # warm-up: module load, clocks
        for _ in range(200):
            assert fn() == 0
    ctx.sync()
    rows = {"builtin": [], "user": []}
    for r in range(a.rounds):
        for name, fn in (("builtin", builtin), ("user", user)) if r % 2 == 0 else (("user", user), ("builtin", builtin)):
            rows[name].append(one_round(fn))
    print(f"{a.rounds} alternating rounds x {a.calls} calls, {W}x{H} target, one {W}x{H} source, silly at t = 0.4")
    print(f"{'path':28} {'host us/call (enqueue)':>34} {'us/call, device drained':>34}")
    med = {}
    for name, label in (("builtin", "smr_builtin_shader(SILLY)"), ("user", "smr_user_shader(silly)")):
        host = [x[0] for x in rows[name]]
        full = [x[1] for x in rows[name]]
        med[name] = (statistics.median(host), statistics.median(full))
        print(f"{label:28} {f'median {med[name][0]:.2f} (range {min(host):.2f} - {max(host):.2f})':>34} "
              f"{f'median {med[name][1]:.2f} (range {min(full):.2f} - {max(full):.2f})':>34}")
    print(f"user / builtin: host {med['user'][0] / med['builtin'][0]:.3f}, drained {med['user'][1] / med['builtin'][1]:.3f}")
    assert prog.launches == 200 + a.rounds * a.calls
    prog.close()
    ctx.close()


if __name__ == "__main__":
    main()
