#!/usr/bin/env python3
"""The 10-bit block converter beside the 8-bit one: one conversion launch of eight 1920 x 1080 frames into RGB12 node textures,
P010 (k_yuv420_hi_to_rgba<true>, 6.0 bytes moved per pixel: 3 in, 3 out) against NV12 (k_yuv420_to_rgba<true>, 4.5: 1.5 in, 3 out); and the
10-bit 4:2:2 block converter: planar 10-bit and P210 (k_yuv422_hi_to_rgba<0>, <1>: 4 in, 3 out), v210 (<2>: 2.67 in, 3 out)
beside P010 and beside UYVY through k_yuv_to_rgba_batch (2 in, 4 out: that kernel writes RGBA8 nodes).

   python tools/hi_depth_time.py run FORMAT N        FORMAT: p010 | nv12 | planar422 | p210 | v210 | uyvy.  The workload, for one `rocprofv3 --kernel-trace --stats` run: N calls of
                                                     smr_ingest_resample_batch with eight 1080p inputs into 1280 x 720 tiles (the default
                                                     route: ONE converter launch per call into RGB12 nodes, then the matrix-core resampler)
   python tools/hi_depth_time.py report DIR [DIR...] the converter kernels' rows of the kernel stats under each DIR (the -d of a run), one
                                                     line per directory: calls, average, minimum, maximum in microseconds

Uses the smelter_amd package of the directory it is started in.  The two formats are measured on the same commit and the same device,
alternating, three runs each; the frames hold the same picture (the P010 codes are 4 x the NV12 bytes), so the tiles' mean byte agrees.
The 4:2:2 frames repeat every chroma row of that picture (v210 and UYVY take the pair's own chroma instead of interpolating)."""
import csv
import glob
import json
import os
import sys

sys.path.insert(0, os.getcwd())


def v210_pack(y, cb, cr):
    """Codes y (h, w), cb, cr (h, w / 2), w a multiple of 6 -> the (h, 4 w / 6) dwords: Cb0 Y0 Cr0 | Y1 Cb1 Y2 | Cr1 Y3 Cb2 | Y4 Cr2 Y5 (lo mid hi)."""
    import numpy as np
    h, w = y.shape
    y, cb, cr = y.reshape(h, w // 6, 6), cb.reshape(h, w // 6, 3), cr.reshape(h, w // 6, 3)
    d = np.stack([cb[..., 0] | y[..., 0] << 10 | cr[..., 0] << 20, y[..., 1] | cb[..., 1] << 10 | y[..., 2] << 20,
                  cr[..., 1] | y[..., 3] << 10 | cb[..., 2] << 20, y[..., 4] | cr[..., 2] << 10 | y[..., 5] << 20], -1)
    return np.ascontiguousarray(d.reshape(h, 4 * (w // 6)).astype(np.uint32))


def run(fmt_name, n):
    import numpy as np
    from smelter_amd import hip
    from smelter_amd.synth import test_input
    ctx = hip.Context(0)
    iw, ih, dw, dh, inputs = 1920, 1080, 1280, 720, 8
    frames = []
    for i in range(inputs):
        y, u, v = test_input(i, iw, ih, noise_seed=900 + i)
        c = np.ascontiguousarray(np.stack([u, v], -1))
        c2 = np.ascontiguousarray(np.repeat(c, 2, axis=0))  # 4:2:2: a chroma row per luma row
        if fmt_name == "planar422":
            frames.append(ctx.frame(hip.FRAME_PLANAR_YUV422P10, iw, ih, [y.astype(np.uint16) << 2, c2[..., 0].astype(np.uint16) << 2, c2[..., 1].astype(np.uint16) << 2]))
        elif fmt_name == "p210":
            frames.append(ctx.frame(hip.FRAME_P210, iw, ih, [y.astype(np.uint16) << 8, c2.astype(np.uint16) << 8]))
        elif fmt_name == "v210":
            frames.append(ctx.frame(hip.FRAME_V210, iw, ih, [v210_pack(y.astype(np.uint32) << 2, c2[..., 0].astype(np.uint32) << 2, c2[..., 1].astype(np.uint32) << 2)]))
        elif fmt_name == "uyvy":
            frames.append(ctx.frame(hip.FRAME_UYVY422, iw, ih, [np.ascontiguousarray(np.stack([c2[..., 0], y[:, 0::2], c2[..., 1], y[:, 1::2]], -1))]))
        elif fmt_name == "p010":
            frames.append(ctx.frame(hip.FRAME_P010, iw, ih, [y.astype(np.uint16) << 8, c.astype(np.uint16) << 8]))  # code 4 b in the high ten bits
        else:
            frames.append(ctx.frame(hip.FRAME_NV12, iw, ih, [y, c]))
    dsts = [ctx.surface(dw, dh) for _ in frames]
    crops = [(0.0, 0.0, float(iw), float(ih))] * inputs
    before = ctx.kernel_launches()
    for _ in range(n):
        ctx.ingest_resample_batch(frames, crops, dsts)
    ctx.sync()
    ran = {k: v - before[k] for k, v in ctx.kernel_launches().items() if v != before[k]}
    print(json.dumps({"tree": os.path.basename(os.getcwd()), "format": fmt_name, "calls": n, "launches": ran,
                      "mean_byte": round(float(np.mean([d.download().mean() for d in dsts])), 4)}))
    ctx.close()


def report(dirs):
    for d in dirs:
        for f in sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)):
            for row in csv.DictReader(open(f)):
                if any(k in row["Name"] for k in ("k_yuv420_to_rgba", "k_yuv420_hi_to_rgba", "k_yuv422_hi_to_rgba", "k_yuv_to_rgba_batch")):
                    name = row["Name"].split("::")[-1].split("(")[0]
                    print(f"{d}: {name:36s} calls {int(row['Calls']):5d}  avg {float(row['AverageNs']) / 1e3:7.2f} us  min {int(row['MinNs']) / 1e3:7.2f}  max {int(row['MaxNs']) / 1e3:7.2f}")


if __name__ == "__main__":
    if len(sys.argv) >= 4 and sys.argv[1] == "run" and sys.argv[2] in ("p010", "nv12", "planar422", "p210", "v210", "uyvy"):
        run(sys.argv[2], int(sys.argv[3]))
    elif len(sys.argv) >= 3 and sys.argv[1] == "report":
        report(sys.argv[2:])
    else:
        sys.exit(__doc__)
