"""What the sharded renderer's transport and driver cost on ONE device (contexts of one device share its CUs and HBM: these are code-path and
host-cost numbers, NOT a scaling point), configs[3] geometry — 8 x 4K YUV420 inputs, 1280 x 720 tiles, a 4K output:

  (a) smr_gather_tiles, world 2 (4 remote tiles) and world 8 (7): host time per call (the enqueue) and time per call with the device drained.
      With a laboratory build (tools/variant.sh lab; SMR_LIB=smelter_amd/variants/libsmr_hip.lab.so) the per-tile hipMemcpy2DAsync transport
      this replaced (SMR_GATHER_COPIES=1, read when a communicator is created) runs in the same process, rounds alternating with k_move_rects.
  (b) frames/s of Renderer(ctx, shards=[...]) at world 2 and 8 beside the single-context Renderer on the same frames (host enqueue per frame,
      and frames/s with the device drained at the end).

python tools/shard_rate.py [--rounds 5] [--calls 2000] [--frames 300]"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from smelter_amd import hip, synth  # noqa: E402
from smelter_amd.renderer import Renderer  # noqa: E402

IW, IH, W, H, N = 3840, 2160, 3840, 2160, 8
TW, TH = 1280, 720


def gather_rate(world, calls, rounds):
    ctxs = [hip.Context(0) for _ in range(world)]
    owners = [i % world for i in range(N)]
    src = [ctxs[owners[i]].surface(TW, TH) for i in range(N)]
    dst = [src[i] if owners[i] == 0 else ctxs[0].surface(TW, TH) for i in range(N)]
    modes = ["mover"]
    if hip.lab_build():
        modes = ["copies", "mover"]
    comms = {}
    for m in modes:
        os.environ["SMR_GATHER_COPIES"] = "1" if m == "copies" else "0"
        comms[m] = hip.Comm.local(ctxs)
    os.environ.pop("SMR_GATHER_COPIES", None)
    res = {m: {"host_us": [], "drained_us": []} for m in modes}
    for rnd in range(rounds + 1):      # (round 0 warms up: code objects, first launches)
        for m in modes:
            comm = comms[m]
            for c in ctxs:
                c.sync()
            t0 = time.perf_counter()
            for _ in range(calls):
                comm.gather(0, owners, src, dst)
            t1 = time.perf_counter()
            for c in ctxs:
                c.sync()
            t2 = time.perf_counter()
            if rnd:
                res[m]["host_us"].append(1e6 * (t1 - t0) / calls)
                res[m]["drained_us"].append(1e6 * (t2 - t0) / calls)
    remote = sum(1 for o in owners if o)
    for m in modes:
        h, d = res[m]["host_us"], res[m]["drained_us"]
        print(f"gather world {world} ({remote} remote tiles) {m:6s}: host {statistics.median(h):7.1f} us/call (min {min(h):.1f} max {max(h):.1f}), "
              f"drained {statistics.median(d):7.1f} us/call (min {min(d):.1f} max {max(d):.1f}) over {rounds} rounds of {calls} calls")
    for comm in comms.values():
        comm.close()
    for c in ctxs:
        c.close()


def renderer_rate(world, frames_n):
    ctxs = [hip.Context(0) for _ in range(world)]
    r = Renderer(ctxs[0], stream_fallback_timeout_s=3600.0, shards=ctxs[1:])
    frames = {}
    for i in range(N):
        r.register_input(f"in{i}")
        frames[f"in{i}"] = r.input_context(f"in{i}").frame(hip.FRAME_PLANAR_YUV420, IW, IH, list(synth.test_input(i, IW, IH, noise_seed=900 + i)))
    r.update_scene("out", W, H, {"type": "tiles", "background_color": "#000000FF",
                                 "children": [{"type": "input_stream", "input_id": f"in{i}"} for i in range(N)]})
    packed = r.make_frame_set(frames)
    ns = 1_000_000_000 // 60
    for s in range(30):
        r.render_packed(s * ns, packed)
    r.sync()
    t0 = time.perf_counter()
    for s in range(frames_n):
        r.render_packed((30 + s) * ns, packed)
    t1 = time.perf_counter()
    r.sync()
    t2 = time.perf_counter()
    moves = sum(c.kernel_launches()["move_rects"] for c in ctxs)
    print(f"renderer world {world}: host enqueue {1e6 * (t1 - t0) / frames_n:.1f} us/frame, {frames_n / (t2 - t0):.1f} frames/s with the device drained "
          f"({moves / (30 + frames_n):.2f} move_rects launches per frame)")
    r.close()
    for f in frames.values():
        f.destroy()
    for c in ctxs:
        c.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--frames", type=int, default=300)
    a = ap.parse_args()
    print(f"library: {'laboratory' if hip.lab_build() else 'product'} build; one device, {N} x {IW}x{IH} inputs, tiles {TW}x{TH}, output {W}x{H}")
    for world in (2, 8):
        gather_rate(world, a.calls, a.rounds)
    for world in (1, 2, 8):
        renderer_rate(world, a.frames)


if __name__ == "__main__":
    main()
