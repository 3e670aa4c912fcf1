#!/usr/bin/env python3
"""What the clip vertex stage costs against the affine one for the same picture ("Clip vertex stage"): the rotating
example (tests/user_shader_sources_affine.py ROTATE: coverage decided in quad space, the vertex stage evaluated by every lane) against the
same rotation written as a clip stage with w = 1 (below: four vertex calls per plane per workgroup, a table in LDS, two triangles of edge
functions), 1920x1080 target, one 1080p source, one process, alternating rounds — the method of tools/user_shader_cost.py.  Per round and
path: host microseconds per call (the time to enqueue CALLS launches, nothing waited for) and microseconds per call with the device drained
(enqueue + smr_sync over CALLS back-to-back launches).  Device time per kernel comes from a run of its own under the profiler, one path per
run, since both kernels carry the same name:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o s -- python tools/clip_vertex_cost.py --rounds 1 --calls 500 --only clip
The two pictures are compared first: they must agree except on pixels an edge passes through.
usage: python tools/clip_vertex_cost.py [--rounds 5] [--calls 2000] [--only affine|clip]"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# ROTATE's plane as a clip stage: corner (px, py) -> (xx px + xy py, yx px + yy py, 0, 1), tex_coords passed through; ROTATE's fragment
CLIP_TWIN = r"""
#define SMR_HAS_VERTEX_CLIP
__device__ smr_clip_vertex smr_vertex_clip(const smr_shader_in &in, int plane_id, int vertex_index, float3 position, float2 tex_coords) {
    smr_clip_vertex o;
    o.position = make_float4(position.x, position.y, 0.0f, 1.0f);
    o.tex_coords = tex_coords;
    if (plane_id != in.texture_count - 1) return o;
    const uint2 d = smr_dimensions(in, plane_id);
    const float W = (float)in.output_resolution.x, H = (float)in.output_resolution.y;
    const float fit = fminf(W / (float)d.x, H / (float)d.y) * 0.6f;
    const float hw = 0.5f * fit * (float)d.x, hh = 0.5f * fit * (float)d.y;
    const float c = cosf(in.time), s = sinf(in.time);
    o.position.x = 2.0f * hw * c / W * position.x + -2.0f * hh * s / W * position.y;
    o.position.y = 2.0f * hw * s / H * position.x + 2.0f * hh * c / H * position.y;
    return o;
}
"""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--only", choices=["affine", "clip"])
    a = ap.parse_args()
    import numpy as np
    from smelter_amd import hip
    from tests import user_shader_sources_affine as SA
    from tools.kernel_resources import code_object_resources

    fragment = SA.ROTATE[SA.ROTATE.index("__device__ float4 smr_fragment"):]
    progs = {"affine": hip.ShaderProgram(SA.ROTATE), "clip": hip.ShaderProgram(CLIP_TWIN + fragment)}
    for name, p in progs.items():
        r = code_object_resources(bytes(p.code))["smr_user_shader_kernel"]
        print(f"{name:7} {r['vgpr']} VGPRs, {r['sgpr']} SGPRs, {r['lds']} B LDS, {r['scratch']} B scratch")

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
    differ = (pictures["affine"] != pictures["clip"]).any(axis=-1)
    drawn = pictures["affine"].any(axis=-1)
    print(f"pictures: {int(drawn.sum())} of {W * H} pixels drawn, {int(differ.sum())} differ between the two stages")
    assert differ.sum() <= 0.001 * drawn.sum(), "the twin does not draw the affine shader's picture"

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
    print(f"{'path':28} {'host us/call (enqueue)':>34} {'us/call, device drained':>34}")
    med = {}
    for name, _ in paths:
        host = [x[0] for x in rows[name]]
        full = [x[1] for x in rows[name]]
        med[name] = (statistics.median(host), statistics.median(full))
        print(f"{'smr_user_shader(' + name + ')':28} {f'median {med[name][0]:.2f} (range {min(host):.2f} - {max(host):.2f})':>34} "
              f"{f'median {med[name][1]:.2f} (range {min(full):.2f} - {max(full):.2f})':>34}")
    if len(med) == 2:
        print(f"clip / affine: host {med['clip'][0] / med['affine'][0]:.3f}, drained {med['clip'][1] / med['affine'][1]:.3f}")
    for p in progs.values():
        p.close()
    ctx.close()


if __name__ == "__main__":
    main()
