#!/usr/bin/env python3
"""Frames per second of the headline scene (bench.py's: 8 x 1080p -> 4K, at rest) through the Renderer for a chosen OUTPUT format, and the
stand-alone output converter at 4K — the A/B behind DESIGN.md section 3m (packed 4:2:2 outputs against planar 4:2:2).  One context, one
frame in flight; every timed window ends in a device synchronise.  Prints one JSON line.

usage: python tools/bench_output_format.py --format uyvy [--frames 300] [--runs 5] [--warmup 30]
       SMR_LIB=other/libsmr_hip.so python tools/bench_output_format.py --format planar422      (another build of the library, same script)
A kernel trace of the same loop: rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_output_format.py --format uyvy --runs 1"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--format", choices=["planar420", "planar422", "nv12", "uyvy", "yuyv"], required=True)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--ring", type=int, default=3, help="distinct input frame sets cycled through")
    args = ap.parse_args()
    import numpy as np
    import bench
    from smelter_amd import hip
    from smelter_amd.renderer import Renderer
    fmt = {"planar420": hip.FRAME_PLANAR_YUV420, "planar422": hip.FRAME_PLANAR_YUV422, "nv12": hip.FRAME_NV12, "uyvy": hip.FRAME_UYVY422,
           "yuyv": hip.FRAME_YUYV422}[args.format]
    ctx = hip.Context(0)
    r = Renderer(ctx, stream_fallback_timeout_s=3600.0)
    ids = [f"input_{i}" for i in range(bench.N_IN)]
    for i in ids:
        r.register_input(i)
    book = bench.font_book()
    if book is not None:
        r.set_fontbook(book)
    nodes = r.update_scene("out", bench.OUT_W, bench.OUT_H, bench.scene_json(), output_format=fmt)
    if book is None:
        from smelter_amd import _ffi
        atlas, glyphs = bench.label_run()
        for n in nodes:
            if n.kind == _ffi.NODE_TEXT:
                r.set_text("out", n.index, glyphs, atlas)
    ring = [{ids[i]: f for i, f in row.items()} for row in bench.make_inputs(ctx, hip, args.ring, list(range(bench.N_IN)))]
    sets = [r.make_frame_set(row) for row in ring]
    frame_ns, tick = 1_000_000_000 // 60, 0  # (presentation timestamps never go backwards)
    for k in range(args.warmup):
        r.render_packed(tick * frame_ns, sets[k % len(sets)])
        tick += 1
    r.sync()
    fps = []
    for _ in range(args.runs):
        t0 = time.perf_counter()
        for k in range(args.frames):
            r.render_packed(tick * frame_ns, sets[k % len(sets)])
            tick += 1
        r.sync()
        fps.append(args.frames / (time.perf_counter() - t0))
    # the stand-alone converter at the output's size: device events around 100 calls
    node = ctx.surface_from(np.random.default_rng(1).integers(0, 256, (bench.OUT_H, bench.OUT_W, 4), dtype=np.uint8))
    out = ctx.frame(fmt, bench.OUT_W, bench.OUT_H)
    conv = []
    for _ in range(args.runs):
        for _ in range(10):
            ctx.rgba_to_frame(node, fmt, out)
        ctx.timer_start()
        for _ in range(100):
            ctx.rgba_to_frame(node, fmt, out)
        conv.append(ctx.timer_stop() * 10.0)  # us per call
    print(json.dumps({"format": args.format, "lib": os.environ.get("SMR_LIB", "this tree's"), "frames": args.frames, "fps": [round(f, 1) for f in fps],
                      "us_per_frame": [round(1e6 / f, 1) for f in fps], "rgba_to_frame_us_4k": [round(c, 2) for c in conv]}))
    r.close()
    ctx.close()


if __name__ == "__main__":
    main()
