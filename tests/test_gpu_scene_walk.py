"""Random walks of scene updates (tests/scene_walk.py) through the long-lived Renderer on the device, frame by frame: the state the renderer
keeps between frames — tile-class cache, parameter-pack ring, resample targets, per-node surfaces and their opaque claims, the alternating
output frames, direct-output jobs, lanes, shards, static Image nodes, the scene's transition state — driven together, in orders nobody planned.

Per seed one op list drives four renderers, each with its own context(s) and its own uploads of the same planes:
  (a) the default renderer                      (b) one with two extra lanes (frames in flight; read back two render calls later)
  (c) direct_output on, compose_select off, compact_nodes off (include/smr.h: "same output bytes either way" for each)
  (d) one with a shard on a second context of the same device
and three comparisons are made:
  * (a) against the ORACLE at every rendered frame of every live output: the oracle's own scene state (oracle/transition.py over
    tests/scene_json.py — never the product's engine) laid out at that pts, rendered by tests/refpipe.py over the oracle's node textures of
    that frame's planes (None for an absent, stale or unregistered input).  <= 1 LSB on every byte of every plane; the share of identical
    bytes, pooled per seed and plane, >= 0.99 (the floor tests/test_gpu_reference_scenes.py holds frames behind the resampler to).
    It cannot see an error below 1 LSB, nor one on fewer than 1 % of a walk's bytes that stays within 1 LSB.
  * (b), (c), (d) against (a), byte for byte, at every rendered frame.  This cannot see an error every configuration shares.
  * (a) against a brand-new renderer on a brand-new context at every frame the walk marks `settled` (given only that output's last update
    and the current frames): byte for byte.  This sees state that survives in the long-lived renderer; it cannot see an error a renderer
    makes from its first frame on (the oracle comparison does).
The second walk (no transitions; scenes also hold a blur Shader node over a nested View, a static Image in a Rescaler of another size and a
Text label) has no oracle picture — the oracle's scene chain does not restate those node kinds — and makes the two renderer comparisons.

A failing assertion names seed, op index, output, plane, the largest difference and the number of differing bytes, and leaves the op list
up to that op as JSON under tmp_path.

Identical-byte pools of (a) against the oracle, measured on an MI355X (Y / U / V per seed; NV12's UV plane counts into U and V):
  seed 11: 0.999996 / 0.999989 / 1.000000  (4080384 luma bytes, worst 1 LSB)
  seed 12: 1.000000 / 1.000000 / 1.000000  (1677464 luma bytes, worst 0 LSB)
  seed 13: 0.999999 / 0.999998 / 1.000000  (3211776 luma bytes, worst 1 LSB)
  seed 14: 0.999999 / 1.000000 / 1.000000  (4045824 luma bytes, worst 1 LSB)
  seed 15: 1.000000 / 1.000000 / 1.000000  (4584796 luma bytes, worst 1 LSB)
  seed 16: 0.999997 / 1.000000 / 0.999998  (2567856 luma bytes, worst 1 LSB)
  seed 17: 0.999996 / 0.999995 / 0.999997  (1517036 luma bytes, worst 1 LSB)
  seed 18: 0.999999 / 0.999987 / 0.999998  (2103552 luma bytes, worst 1 LSB)
  seed 19: 0.999999 / 0.999999 / 0.999999  (3555912 luma bytes, worst 1 LSB)
  seed 20: 0.999998 / 0.999999 / 0.999999  (3311372 luma bytes, worst 1 LSB)
  seed 21: 1.000000 / 0.999991 / 1.000000  (4325492 luma bytes, worst 1 LSB)
  seed 22: 1.000000 / 1.000000 / 1.000000  (2352384 luma bytes, worst 1 LSB)
  all 12: 0.999999 / 0.999996 / 0.999999  (37333848 luma bytes); the floor is 0.99
Kernels the twelve walks reached on that run (smr_debug_kernel_launches, the default renderer): k_compose_output 1070 launches, the matrix-core
resampler 1083, the 4:2:0 block converter 1334; with direct_output on 49 resampler launches carried direct-output jobs; the shard moved
489 gathers.  The general resampling passes, the f32 ingest kernel and the general compositor were not reached by these seeds: they stay with
their own zoos (tests/test_gpu_parity.py, tests/test_gpu_fused.py, tests/test_gpu_compose_zoo.py).

The third walk (tests/scene_walk.walk_formats: all fifteen base formats, the three matrices, odd and ragged sizes, BGRA / ARGB / RGBA frames with alpha over
other inputs, an input id changing format, depth, matrix, alpha or size between two renders, a sixth of the frame specs in caller memory over torch
buffers of the tightest pitch; odd seeds in MODE_CPU_OPTIMIZED with the oracle at srgb=False) makes all three comparisons with the same bars.  The node of a
frame with a matrix tag or of 10 bits is tests/color_matrix_model.node_rgba (the oracle has no such converter; tests/test_color_matrix_model.py holds the
model to the oracle at BT.709, the device converters are held to it byte for byte by tests/test_gpu_color_matrix.py and the 10-bit modules).  Its pools on
an MI355X:
  seed 201 (cpu): 1.000000 / 1.000000 / 1.000000  (2724780 luma bytes, worst 0 LSB; 12 frames in caller memory; converter launches 136, of them the 4:2:0 block converter 60)
  seed 202 (gpu): 0.999997 / 0.999996 / 1.000000  (1908672 luma bytes, worst 1 LSB; 11 frames in caller memory; converter launches 112, of them the 4:2:0 block converter 31)
  seed 203 (cpu): 1.000000 / 1.000000 / 1.000000  (5700740 luma bytes, worst 0 LSB; 8 frames in caller memory; converter launches 159, of them the 4:2:0 block converter 57)
  seed 204 (gpu): 0.999994 / 0.999997 / 0.999992  (3667716 luma bytes, worst 1 LSB; 13 frames in caller memory; converter launches 326, of them the 4:2:0 block converter 126)
  seed 205 (cpu): 1.000000 / 1.000000 / 1.000000  (3732480 luma bytes, worst 0 LSB; 8 frames in caller memory; converter launches 88, of them the 4:2:0 block converter 25)
  seed 206 (gpu): 0.999994 / 0.999993 / 0.999995  (3526648 luma bytes, worst 1 LSB; 9 frames in caller memory; converter launches 260, of them the 4:2:0 block converter 88)
  seed 207 (cpu): 1.000000 / 1.000000 / 1.000000  (5305260 luma bytes, worst 0 LSB; 8 frames in caller memory; converter launches 227, of them the 4:2:0 block converter 53)
  seed 208 (gpu): 0.999981 / 0.999998 / 0.999984  (2270924 luma bytes, worst 1 LSB; 11 frames in caller memory; converter launches 111, of them the 4:2:0 block converter 73)
Launches of the default renderer over the eight seeds: compose_output 690, frame_to_rgba 1419, frame_to_rgba_420 513, ingest_wave_rgba 533, resample_general 20: converters other than the 4:2:0 block
converter ran 906 times, and seed 204 reached the general resampling passes (20 launches).  A MODE_CPU_OPTIMIZED walk has no resampler (every byte was the
oracle's).  A traced build of the same walks showed the RGB12 node and the RGBA8 node alternating on one source index at one size in seeds
202, 204 and 206, for 8-bit 4:2:0 and 10-bit 4:2:2 frames.  These walks, and 51 further seeds run once, found no difference.
"""
import ctypes as C
import json

import numpy as np
import pytest

from oracle import oracle as orc
from tests import color_matrix_model as cmm, refpipe, scene_walk as SW, scenes

# (an absent input has size 0 x 0: the reference's layout arithmetic divides by it, and so does the oracle's)
pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:invalid value encountered:RuntimeWarning"),
              pytest.mark.filterwarnings("ignore:divide by zero encountered:RuntimeWarning")]

KINDS = ("plain", "lanes", "options", "shard")


@pytest.fixture(scope="module")
def hip():
    from smelter_amd import hip as h
    orc.build()
    return h


_planes_cache, _node_cache = {}, {}


def _planes(spec):
    key = tuple(spec)
    if key not in _planes_cache:
        if len(_planes_cache) > 256:
            _planes_cache.clear()
        _planes_cache[key] = SW.frame_planes(spec)
    return _planes_cache[key]


_ORACLE_PLANAR = {"yuv420": orc.YUV420, "yuv422": orc.YUV422, "yuv444": orc.YUV444, "yuvj420": orc.YUVJ420}
_MATRIX = {None: cmm.BT709, "bt601": cmm.BT601, "bt2020": cmm.BT2020_NCL}


def _node(spec, srgb=True):
    """The oracle's node texture of a frame: its own converters for the untagged 8-bit formats; for a frame with a matrix tag or of 10 bits, where the
    oracle has no converter, tests/color_matrix_model.py (held to the oracle at BT.709 by tests/test_color_matrix_model.py)."""
    key = tuple(spec) + (srgb,)
    if key not in _node_cache:
        if len(_node_cache) > 256:
            _node_cache.clear()
        fmt, w, h, _ = spec
        base, matrix = SW.split_format(fmt)
        p = _planes(spec)
        if matrix is not None or base in SW.HI_FORMATS:
            node = cmm.node_rgba(SW.BASE_FORMATS.index(base), w, h, p, _MATRIX[matrix])
        elif base == "nv12":
            node = orc.nv12_to_rgba(p[0], p[1], w, h)
        elif base in _ORACLE_PLANAR:
            node = orc.planar_yuv_to_rgba(p[0], p[1], p[2], w, h, _ORACLE_PLANAR[base])
        elif base in SW.PACKED_8BIT_FORMATS:
            node = orc.interleaved422_to_rgba(p[0], w, h, 0 if base == "uyvy422" else 1)
        elif base in ("bgra", "argb"):
            node = orc.swizzle_to_rgba(p[0], w, h, 0 if base == "bgra" else 1)
        else:
            assert base == "rgba", base
            node = orc.add_premultiplied_alpha(p[0], srgb)
        _node_cache[key] = node
    return _node_cache[key]


def _frame_format(hip, fmt):
    """The smr_frame.format of a spec's format string: the base format and, behind an "@", its matrix (SMR_FRAME_WITH_MATRIX)."""
    base, matrix = SW.split_format(fmt)
    tag = {None: hip.MATRIX_BT709, "bt601": hip.MATRIX_BT601, "bt2020": hip.MATRIX_BT2020_NCL}[matrix]
    return hip.frame_format(SW.BASE_FORMATS.index(base), tag)


def _torch():
    try:
        import torch
        return torch if torch.cuda.is_available() else None
    except ImportError:
        return None


def _wrapped_frame(torch, ctx, fmt, w, h, planes):
    """The frame over torch buffers with the tightest pitch a wrapped plane may have (its rows' bytes rounded up to 4), each exactly pitch * rows
    long: -> (frame, buffers to keep alive)."""
    bufs, pairs = [], []
    for p in planes:
        rows = np.ascontiguousarray(p).view(np.uint8).reshape(p.shape[0], -1)
        pitch = (rows.shape[1] + 3) // 4 * 4
        buf = torch.zeros((pitch * rows.shape[0],), dtype=torch.uint8, device="cuda")
        buf.view(rows.shape[0], pitch)[:, :rows.shape[1]] = torch.from_numpy(rows).cuda()
        bufs.append(buf)
        pairs.append((buf.data_ptr(), pitch))
    torch.cuda.synchronize()
    return ctx.wrapped_frame(fmt, w, h, pairs), bufs


def _logo():
    rng = np.random.default_rng(5)
    w, h = SW.IMAGE_SIZE
    img = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    img[: h // 2, :, 3] = 255
    return img


class Rig:
    """One renderer configuration with its own contexts and its own uploads."""

    def __init__(self, hip, kind, nodes=False, mode=None, wrap=False):
        from smelter_amd.renderer import Renderer
        self.hip, self.kind, self.nodes, self.wrap = hip, kind, nodes, wrap
        self.mode = hip.MODE_GPU_OPTIMIZED if mode is None else mode
        self.ctx = hip.Context(0, self.mode)
        self.more = []
        if kind == "options":
            self.ctx.set_direct_output(True)
            self.ctx.set_compose_select(False)
            self.ctx.set_compact_nodes(False)
        if kind == "lanes":
            self.more = [hip.Context(0, self.mode), hip.Context(0, self.mode)]
            self.r = Renderer(self.ctx, lanes=self.more)
        elif kind == "shard":
            self.more = [hip.Context(0, self.mode)]
            self.r = Renderer(self.ctx, shards=self.more)
        else:
            self.r = Renderer(self.ctx)
        if nodes:
            self.r.register_image(SW.IMAGE_ID, _logo())
            self.r.register_shader(SW.SHADER_ID)
        self.registered, self.frames, self.made, self.held, self.caller_memory = [], {}, {}, [], []

    def close(self):
        self.r.sync()
        self.r.close()
        for f in self.made.values():
            f.destroy()
        for c in self.more + [self.ctx]:
            c.close()

    def apply(self, op):
        """Every op but render."""
        from smelter_amd import _ffi
        k = op["op"]
        if k == "register_input":
            self.r.register_input(op["input_id"])
            self.registered.append(op["input_id"])
        elif k == "unregister_input":
            self.r.unregister_input(op["input_id"])
            self.registered.remove(op["input_id"])
        elif k == "frames":
            self.frames = op["frames"]
        elif k == "unregister_output":
            self.r.unregister_output(op["output_id"])
        elif k == "update":
            fmt = self.hip.FRAME_NV12 if op["format"] == "nv12" else self.hip.FRAME_PLANAR_YUV420
            nodes = self.r.update_scene(op["output_id"], op["width"], op["height"], op["scene"], output_format=fmt)
            if self.nodes:
                atlas, glyphs = scenes.label_glyphs(*SW.LABEL)
                for n in nodes:
                    if n.kind == _ffi.NODE_TEXT:
                        self.r.set_text(op["output_id"], n.index, glyphs, atlas)

    def _frame(self, iid, spec):
        ctx = self.r.input_context(iid) if self.kind == "shard" and iid in self.registered else self.ctx
        key = (ctx.handle.value, tuple(spec))
        if key not in self.made:   # (never destroyed before close: frames in flight may still read them)
            torch = _torch() if self.wrap and spec[3] % 6 == 0 else None
            if torch is not None:  # a sixth of the format walk's frames live in caller memory (owned frames where there is no torch)
                self.made[key], bufs = _wrapped_frame(torch, ctx, _frame_format(self.hip, spec[0]), spec[1], spec[2], _planes(spec))
                self.caller_memory.append(bufs)
            else:
                self.made[key] = ctx.frame(_frame_format(self.hip, spec[0]), spec[1], spec[2], _planes(spec))
        return self.made[key]

    def render(self, op):
        """-> {output id: BorrowedFrame}"""
        from smelter_amd import _ffi
        live = [(k, f) for k, f in sorted(self.frames.items()) if f is not None]
        arr = (_ffi.InputFrame * max(len(live), 1))()
        keep = []
        for i, (k, spec) in enumerate(live):
            f = self._frame(k, spec)
            key = k.encode()
            keep.append((key, f))
            arr[i].input_id, arr[i].frame, arr[i].pts_ns = key, C.pointer(f.c), op["frame_pts"].get(k, op["pts_ns"])
        n = self.r.render_packed(op["pts_ns"], (arr, len(live), keep))
        return {self.r._outs[i].output_id.decode(): self.r.output(i) for i in range(n)}


def _fresh_render(hip, update_op, registered, frames, render_op, nodes=False, mode=None, wrap=False):
    """A brand-new renderer on a brand-new context: that output's last update, the current frames, one render."""
    rig = Rig(hip, "plain", nodes, mode, wrap)
    try:
        for iid in registered:
            rig.apply({"op": "register_input", "input_id": iid})
        rig.apply(update_op)
        rig.frames = frames
        return [np.array(p) for p in rig.render(render_op)[update_op["output_id"]].download()]
    finally:
        rig.close()


class Fail(AssertionError):
    pass


def _plane_names(fmt):
    return ["Y", "UV"] if fmt == "nv12" else ["Y", "U", "V"]


def _run_walk(hip, seed, ops, tmp_path, oracle_on, nodes, kinds=KINDS, mode=None, wrap=False, stats=None):
    """mode: the rendering mode of every context (the four rigs', the fresh renderers') and of the oracle; wrap: frame specs whose content seed is a
    multiple of 6 live in caller memory; stats: a dict that receives the default rig's kernel launch counts."""
    srgb = mode is None or mode == hip.MODE_GPU_OPTIMIZED
    rigs = {k: Rig(hip, k, nodes, mode, wrap) for k in kinds}
    witness = SW.OracleOutputs() if oracle_on else None
    last_update, registered, frames = {}, [], {}
    pools = {p: [0, 0] for p in "YUV"}   # identical bytes, bytes
    worst = 0
    fresh_checks, after_sibling_checks = 0, 0
    k = -1

    def fail(what, oid, fmt, got, want, at=None):
        at = k if at is None else at
        for name, g, w_ in zip(_plane_names(fmt), got, want):
            if g.shape != w_.shape or not np.array_equal(g, w_):
                d = np.abs(g.astype(np.int32) - w_.astype(np.int32)) if g.shape == w_.shape else None
                path = tmp_path / f"walk_{seed}_op{at}.json"
                path.write_text(json.dumps(ops[:at + 1]))
                raise Fail(f"seed {seed} op {at} output {oid!r} plane {name}: {what}: max difference "
                           f"{int(d.max()) if d is not None else 'shape'}, {int((d != 0).sum()) if d is not None else -1} bytes differ; ops in {path}")

    def equal(what, oid, fmt, got, want):
        if any(g.shape != w_.shape or not np.array_equal(g, w_) for g, w_ in zip(got, want)):
            fail(what, oid, fmt, got, want)

    def flush(n_keep):
        if "lanes" not in rigs:
            return
        held = rigs["lanes"].held
        while len(held) > n_keep:
            hk, outs, wants = held.pop(0)
            for oid, (fmt, want) in wants.items():
                got = outs[oid].download()
                if any(not np.array_equal(g, w_) for g, w_ in zip(got, want)):
                    fail("two extra lanes against the default renderer", oid, fmt, got, want, at=hk)

    try:
        for k, op in enumerate(ops):
            if op["op"] != "render":
                if op["op"] in ("update", "unregister_output"):
                    flush(0)   # the update frees an output's frames: whatever is still held is read first
                for r in rigs.values():
                    r.apply(op)
                if op["op"] == "register_input":
                    registered.append(op["input_id"])
                elif op["op"] == "unregister_input":
                    registered.remove(op["input_id"])
                elif op["op"] == "frames":
                    frames = op["frames"]
                elif op["op"] == "update":
                    last_update[op["output_id"]] = op
                    if witness:
                        witness.update(op)
                elif op["op"] == "unregister_output":
                    del last_update[op["output_id"]]
                    if witness:
                        witness.unregister(op["output_id"])
                continue
            outs = {name: r.render(op) for name, r in rigs.items()}
            assert all(set(o) == set(last_update) for o in outs.values()), (seed, k, [sorted(o) for o in outs.values()])
            vis = SW.visible_frames(op, frames, set(registered))
            mine = {}
            for oid in sorted(last_update):
                fmt = last_update[oid]["format"]
                a = [np.array(p) for p in outs["plain"][oid].download()]
                mine[oid] = (fmt, a)
                if witness:
                    W, H = last_update[oid]["width"], last_update[oid]["height"]
                    layouts = witness.layouts(oid, op["pts_ns"], vis, srgb=srgb)
                    textures = [_node(vis[i], srgb) if i in vis else None for i in witness.inputs[oid]]
                    rgba = refpipe.layout_node_render(layouts, textures, W, H, srgb=srgb, omp=True)
                    want = list(orc.rgba_to_nv12(rgba)) if fmt == "nv12" else list(orc.rgba_to_planar_yuv(rgba, orc.YUV420, omp=True))
                    for name, g, w_ in zip(_plane_names(fmt), a, want):
                        d = np.abs(g.astype(np.int32) - w_.astype(np.int32))
                        worst = max(worst, int(d.max()))
                        if d.max() > 1:
                            fail("the default renderer against the oracle, more than 1 LSB", oid, fmt, a, want)
                        for ch, dd in (("U", d[..., 0]), ("V", d[..., 1])) if name == "UV" else ((name, d),):
                            pools[ch][0] += int((dd == 0).sum())
                            pools[ch][1] += dd.size
                for name in [n for n in ("options", "shard") if n in rigs]:
                    equal(f"{name} against the default renderer", oid, fmt, outs[name][oid].download(), a)
                if oid in op["settled"]:
                    got = _fresh_render(hip, last_update[oid], registered, frames, op, nodes, mode, wrap)
                    equal("the long-lived default renderer against a brand-new one", oid, fmt, a, got)
                    fresh_checks += 1
                    after_sibling_checks += bool(ops[k - 1].get("only_moves_a_sibling"))
            if "lanes" in rigs:
                rigs["lanes"].held.append((k, outs["lanes"], mine))
            flush(2)   # a lane's frame is read back two render calls later
        if "lanes" in rigs:
            rigs["lanes"].r.sync()
        flush(0)
        if stats is not None and "plain" in rigs:
            stats["launches"] = rigs["plain"].ctx.kernel_launches()
            stats["caller_memory"] = len(rigs["plain"].caller_memory)
    finally:
        for r in rigs.values():
            r.close()
    return pools, worst, fresh_checks, after_sibling_checks


@pytest.mark.parametrize("seed", SW.SEEDS)
def test_a_walk_of_scene_updates_renders_the_oracle_picture_in_every_configuration(hip, seed, tmp_path):
    ops = SW.walk(seed)
    pools, worst, fresh, _ = _run_walk(hip, seed, ops, tmp_path, oracle_on=True, nodes=False)
    shares = {p: same / max(total, 1) for p, (same, total) in pools.items()}
    print(f"walk {seed}: identical to the oracle Y {shares['Y']:.6f} U {shares['U']:.6f} V {shares['V']:.6f} "
          f"({pools['Y'][1]} / {pools['U'][1]} / {pools['V'][1]} bytes), worst {worst} LSB, {fresh} frames against a new renderer")
    assert worst <= 1
    assert fresh >= 2
    for p, s in shares.items():
        assert s >= 0.99, f"seed {seed} plane {p}: only {s:.5f} of the bytes identical to the oracle's"


@pytest.mark.parametrize("seed", SW.FORMAT_SEEDS)
def test_a_walk_of_input_formats_matrices_and_alpha_renders_the_oracle_picture_in_every_configuration(hip, seed, tmp_path):
    """tests/scene_walk.walk_formats: every base format, the three matrices, odd sizes, alpha over other inputs, a sixth of the frames in caller
    memory; odd seeds in MODE_CPU_OPTIMIZED.  The same four rigs, three comparisons and bars as the first walk."""
    mode = hip.MODE_CPU_OPTIMIZED if SW.format_mode(seed) == "cpu_optimized" else hip.MODE_GPU_OPTIMIZED
    stats = {}
    pools, worst, fresh, _ = _run_walk(hip, seed, SW.walk_formats(seed), tmp_path, oracle_on=True, nodes=False, mode=mode, wrap=True, stats=stats)
    shares = {p: same / max(total, 1) for p, (same, total) in pools.items()}
    ran = {k: n for k, n in stats["launches"].items() if n}
    print(f"format walk {seed} ({SW.format_mode(seed)}): identical to the oracle Y {shares['Y']:.6f} U {shares['U']:.6f} V {shares['V']:.6f} "
          f"({pools['Y'][1]} / {pools['U'][1]} / {pools['V'][1]} bytes), worst {worst} LSB, {fresh} frames against a new renderer, "
          f"{stats['caller_memory']} frames in caller memory, launches {ran}")
    assert worst <= 1
    assert fresh >= 2
    for p, s in shares.items():
        assert s >= 0.99, f"seed {seed} plane {p}: only {s:.5f} of the bytes identical to the oracle's"
    # what follows from the walk alone (tests/test_scene_walk.py: every seed shows a frame the 4:2:0 block converter does not take)
    assert stats["launches"]["frame_to_rgba"] - stats["launches"]["frame_to_rgba_420"] > 0, ran
    if mode == hip.MODE_GPU_OPTIMIZED:
        assert stats["launches"]["compose_output"] > 0, ran
    if _torch() is not None:
        assert stats["caller_memory"] > 0


@pytest.mark.parametrize("seed", SW.NODE_SEEDS)
def test_a_walk_with_shader_image_and_text_nodes_renders_the_same_in_every_configuration(hip, seed, tmp_path):
    ops = SW.walk_nodes(seed)
    _, _, fresh, after_sibling = _run_walk(hip, seed, ops, tmp_path, oracle_on=False, nodes=True)
    assert fresh >= 8, fresh
    assert after_sibling >= 1   # a static Image node beside a sibling that moved: neither redrawn wrongly nor left stale


def test_a_remote_input_resampled_along_one_axis_mid_transition_renders_the_default_renderers_bytes(hip, tmp_path):
    """What an earlier walk 19 found at its op 23: a 96 x 54 input that lives on the shard, shown at 95.13 x 53.51 (-> 95 x 54: a one-axis plan) while three
    transitions run.  The owner resampled it with the general passes, the default renderer with the matrix-core kernel's one-axis route: one byte
    of U differed by one code (the shard's was the oracle's).  Such an input now travels as its raw planes
    (csrc/host/renderer.cpp: owner_takes_the_roots_route; tests/test_gpu_sharded_renderer.py pins the rule plan by plan)."""
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scene_walk_one_axis_on_a_shard.json")
    ops = json.load(open(path))["ops"]   # (recorded: the walks may change, what this replays may not)
    assert ops[-1]["op"] == "render" and ops[-1]["pts_ns"] == 894000000
    _run_walk(hip, 19, ops, tmp_path, oracle_on=False, nodes=False, kinds=("plain", "shard"))
