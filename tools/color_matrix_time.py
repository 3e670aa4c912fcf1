#!/usr/bin/env python3
"""k_yuv420_to_rgba on tagged frames beside untagged ones: one conversion launch of eight 1920 x 1080 NV12 frames into RGB12
node textures, the same frames tagged BT.601 (k_yuv420_to_rgba<true, 1>) against untagged (k_yuv420_to_rgba<true, 0>) — tools/hi_depth_time.py's
workload and method (a `rocprofv3 --kernel-trace` run, the converter's rows of the trace), in ONE process, alternating:

   python tools/color_matrix_time.py run N           blocks of N calls of smr_ingest_resample_batch with eight 1080p inputs into 1280 x 720 tiles,
                                                     in the order  untagged, tagged, untagged, tagged  (the two untagged blocks are identical
                                                     runs: their difference is the spread the tagged figure is read against)
   python tools/color_matrix_time.py report DIR N    the converter launches of the kernel trace under DIR (the -d of the run) in time order, cut
                                                     into the four blocks of N: average, minimum, maximum in microseconds per block

Uses the smelter_amd package of the directory it is started in."""
import csv
import glob
import json
import os
import sys

sys.path.insert(0, os.getcwd())


def run(n):
    import numpy as np
    from smelter_amd import hip
    from smelter_amd.synth import test_input
    ctx = hip.Context(0)
    iw, ih, dw, dh, inputs = 1920, 1080, 1280, 720, 8
    sets = {}
    for tag, matrix in (("untagged", hip.MATRIX_BT709), ("bt601", hip.MATRIX_BT601)):
        frames = []
        for i in range(inputs):
            y, u, v = test_input(i, iw, ih, noise_seed=900 + i)
            frames.append(ctx.frame(hip.frame_format(hip.FRAME_NV12, matrix), iw, ih, [y, np.ascontiguousarray(np.stack([u, v], -1))]))
        sets[tag] = frames
    dsts = [ctx.surface(dw, dh) for _ in range(inputs)]
    crops = [(0.0, 0.0, float(iw), float(ih))] * inputs
    for tag in ("untagged", "bt601"):  # warm-up: tables, node surfaces, both code objects
        ctx.ingest_resample_batch(sets[tag], crops, dsts)
    ctx.sync()
    means = {}
    before = ctx.kernel_launches()
    for tag in ("untagged", "bt601", "untagged", "bt601"):
        for _ in range(n):
            ctx.ingest_resample_batch(sets[tag], crops, dsts)
        ctx.sync()
        means[tag] = round(float(np.mean([d.download().mean() for d in dsts])), 4)
    ran = {k: v - before[k] for k, v in ctx.kernel_launches().items() if v != before[k]}
    print(json.dumps({"calls_per_block": n, "blocks": ["untagged", "bt601", "untagged", "bt601"], "launches": ran, "mean_byte": means}))
    ctx.close()


def report(d, n):
    rows = []
    for f in sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)):
        for row in csv.DictReader(open(f)):
            key = {k.lower(): k for k in row}
            name = row[key["kernel_name"]]
            if "k_yuv420_to_rgba" in name:
                rows.append((int(row[key["start_timestamp"]]), int(row[key["end_timestamp"]]), name.split("::")[-1].split("(")[0]))
    rows.sort()
    rows = rows[2:]  # the two warm-up launches
    for b, label in enumerate(("untagged", "bt601", "untagged", "bt601")):
        part = rows[b * n:(b + 1) * n]
        if not part:
            continue
        us = [(e - s) / 1e3 for s, e, _ in part]
        names = sorted({nm for _, _, nm in part})
        print(f"block {b} {label:9s} {','.join(names):40s} calls {len(us):5d}  avg {sum(us) / len(us):7.2f} us  min {min(us):7.2f}  max {max(us):7.2f}")


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "run":
        run(int(sys.argv[2]))
    elif len(sys.argv) >= 4 and sys.argv[1] == "report":
        report(sys.argv[2], int(sys.argv[3]))
    else:
        sys.exit(__doc__)
