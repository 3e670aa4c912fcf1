#!/usr/bin/env python3
"""What varyings cost on the clip vertex stage ("Varyings"): the `w = 1` rotation of tools/clip_vertex_cost.py (its clip
twin, N = 0) against the same shader with four perspective varyings and with eight of mixed modes (three perspective, three linear, two
flat), all consumed by the fragment as a factor on the texel.  1920x1080 target, one 1080p source, one process, alternating rounds — the
method of tools/clip_vertex_cost.py.  Per round and build: host microseconds per call (the time to enqueue CALLS launches, nothing waited
for) and microseconds per call with the device drained (enqueue + smr_sync over CALLS back-to-back launches).  Device time per kernel comes
from a run of its own under the profiler, one build per run, since all kernels carry the same name:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o s -- python tools/varyings_cost.py --rounds 1 --calls 500 --only n4
usage: python tools/varyings_cost.py [--rounds 5] [--calls 2000] [--only n0|n4|n8]"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# ROTATE's fragment with the varyings' mean as a factor on the colour (every varying is 0.5 .. 1 at the vertices)
FRAGMENT_V = r"""
__device__ float4 smr_fragment(const smr_shader_in &in, int plane_id, float2 uv, float4 position, const smr_varyings<SMR_VARYINGS> &v) {
    const uint2 d = smr_dimensions(in, plane_id);
    if (plane_id != in.texture_count - 1) {
        int band = (int)(uv.x * 8.0f);
        if (band > (int)d.x - 1) band = (int)d.x - 1;
        return smr_load(in, plane_id, band, 0);
    }
    int tx = (int)floorf(uv.x * (float)d.x), ty = (int)floorf(uv.y * (float)d.y);
    if (tx > (int)d.x - 1) tx = (int)d.x - 1;
    if (ty > (int)d.y - 1) ty = (int)d.y - 1;
    const float4 texel = smr_load(in, plane_id, tx, ty);
    float k = 0.0f;
    for (int j = 0; j < SMR_VARYINGS; j++) k += v.v[j];
    k = k / (float)SMR_VARYINGS;
    return make_float4(texel.x * k, texel.y * k, texel.z * k, texel.w);
}
"""


def with_varyings(twin, n, flat, linear):
    """tools/clip_vertex_cost.py's CLIP_TWIN returning n varyings: varying j of vertex k is 0.5 + (j + k) / 32"""
    head = f"#define SMR_VARYINGS {n}\n#define SMR_VARYINGS_FLAT {flat:#x}\n#define SMR_VARYINGS_LINEAR {linear:#x}\n"
    body = twin.replace("smr_clip_vertex ", "smr_clip_vertex_v<SMR_VARYINGS> ")
    fill = "    for (int j = 0; j < SMR_VARYINGS; j++) o.varyings[j] = 0.5f + 0.03125f * (float)(j + vertex_index);\n"
    assert body.count("    o.tex_coords = tex_coords;\n") == 1
    return head + body.replace("    o.tex_coords = tex_coords;\n", "    o.tex_coords = tex_coords;\n" + fill) + FRAGMENT_V


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--only", choices=["n0", "n4", "n8"])
    a = ap.parse_args()
    import numpy as np
    from smelter_amd import hip
    from tests import user_shader_sources_affine as SA
    from tools.clip_vertex_cost import CLIP_TWIN
    from tools.kernel_resources import code_object_resources

    fragment = SA.ROTATE[SA.ROTATE.index("__device__ float4 smr_fragment"):]
    progs = {"n0": hip.ShaderProgram(CLIP_TWIN + fragment), "n4": hip.ShaderProgram(with_varyings(CLIP_TWIN, 4, 0x0, 0x0)),
             "n8": hip.ShaderProgram(with_varyings(CLIP_TWIN, 8, 0xC0, 0x38))}
    for name, p in progs.items():
        r = code_object_resources(bytes(p.code))["smr_user_shader_kernel"]
        print(f"{name:4} {r['vgpr']} VGPRs, {r['sgpr']} SGPRs, {r['lds']} B LDS, {r['scratch']} B scratch")

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

    covered = {}
    for name in progs:
        assert call(name)() == 0
        ctx.sync()
        covered[name] = dst.download().any(axis=-1)
    print(f"pictures: {int(covered['n0'].sum())} of {W * H} pixels drawn")
    assert np.array_equal(covered["n0"], covered["n4"]) and np.array_equal(covered["n0"], covered["n8"]), "varyings changed the coverage"

    paths = [(n, call(n)) for n in progs if a.only in (None, n)]

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
    print(f"{'build':28} {'host us/call (enqueue)':>34} {'us/call, device drained':>34}")
    for name, _ in paths:
        host = [x[0] for x in rows[name]]
        full = [x[1] for x in rows[name]]
        print(f"{'smr_user_shader(' + name + ')':28} {f'median {statistics.median(host):.2f} (range {min(host):.2f} - {max(host):.2f})':>34} "
              f"{f'median {statistics.median(full):.2f} (range {min(full):.2f} - {max(full):.2f})':>34}")
    for p in progs.values():
        p.close()
    ctx.close()


if __name__ == "__main__":
    main()
