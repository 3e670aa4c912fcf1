"""The sharded renderer (smr_renderer_add_shard: inputs dealt to several contexts, tiles resampled on their owners, gathered by ONE
k_move_rects launch per owner and node, composed on the root) against the single-context renderer of the same library on the same frames and
pts: EVERY BYTE of every output plane equal (np.array_equal).  The single-context renderer's own parity with the oracle is pinned by
tests/test_gpu_renderer.py and tests/test_gpu_reference_scenes.py.  One device serves: two or three hip.Context(0); the cross-device stores of
the mover run only in the last test, where two GPUs are visible."""
import json
import os

import numpy as np
import pytest

from tests import scenes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = json.load(open(os.path.join(ROOT, "tests", "golden", "render_test_scenes.json")))["tests"]


@pytest.fixture(scope="module")
def hip():
    from smelter_amd import hip as h
    return h


class Pair:
    """The same renderer twice: `one` on a single context, `many` on a root context with shards.  Frames are uploaded where each wants them."""

    def __init__(self, hip, shards=1, mode=None, devices=None):
        from smelter_amd.renderer import Renderer
        mode = hip.MODE_GPU_OPTIMIZED if mode is None else mode
        devices = devices or [0] * shards
        self.hip = hip
        self.one_ctx, self.root = hip.Context(0, mode=mode), hip.Context(0, mode=mode)
        self.shards = [hip.Context(d, mode=mode) for d in devices]
        self.one, self.many = Renderer(self.one_ctx), Renderer(self.root, shards=self.shards)
        self.f_one, self.f_many, self.owner = {}, {}, {}

    def register_input(self, iid, fmt, w, h, planes):
        self.one.register_input(iid)
        self.many.register_input(iid)
        c = self.many.input_context(iid)
        self.owner[iid] = c
        self.f_one[iid] = self.one_ctx.frame(fmt, w, h, list(planes))
        self.f_many[iid] = c.frame(fmt, w, h, list(planes))

    def both(self, fn):
        """fn(renderer): the same call on both; both succeed or both raise the same message."""
        from smelter_amd.scene import SceneError
        res = []
        for r in (self.one, self.many):
            try:
                res.append(("ok", fn(r)))
            except SceneError as e:
                res.append(("error", str(e)))
        assert res[0][0] == res[1][0], res
        if res[0][0] == "error":
            assert res[0][1] == res[1][1]
        return res[0][0] == "ok"

    def update(self, output, W, H, scene, **kw):
        return self.both(lambda r: r.update_scene(output, W, H, scene, **kw))

    def render_equal(self, pts_s, what, ids=None, frame_pts_s=None):
        sel = (lambda d: d) if ids is None else (lambda d: {k: d[k] for k in ids})
        a = self.one.render(pts_s, sel(self.f_one), frame_pts_s)
        b = self.many.render(pts_s, sel(self.f_many), frame_pts_s)
        assert sorted(a) == sorted(b)
        got = {}
        for oid in a:
            assert b[oid].ctx is self.root, "outputs are composed on the root context"
            pa, pb = a[oid].download(), b[oid].download()
            assert len(pa) == len(pb)
            for k, (x, y) in enumerate(zip(pa, pb)):
                assert np.array_equal(x, y), f"{what}: output {oid} plane {k} differs in {int((x != y).sum())} bytes"
            got[oid] = pa
        return got

    def close(self):
        self.one.close()
        self.many.close()
        for d in (self.f_one, self.f_many):
            for f in d.values():
                f.destroy()
        for c in [self.one_ctx, self.root] + self.shards:
            c.close()


def _tiles(order, margin, transition_ms=None):
    s = {"type": "tiles", "id": "grid", "background_color": "#101820FF", "margin": margin,
         "children": [{"type": "input_stream", "id": f"c{i}", "input_id": f"in{i}"} for i in order]}
    if transition_ms:
        s["transition"] = {"duration_ms": transition_ms}
    return s


def _configs3_run(hip, pair, iw, ih, W, H):
    """36 frames of configs[3]'s geometry (8 inputs in a Tiles scene) with a transition running almost throughout: an update that changes the
    tile size, one halfway that reorders the children, one that changes the tile size again."""
    n, frames_n = 8, 36
    rng = np.random.default_rng(91)
    for i in range(n):
        planes = scenes.random_yuv420(iw, ih, rng) if i % 2 else scenes.test_input(i, iw, ih, noise_seed=700 + i)
        pair.register_input(f"in{i}", hip.FRAME_PLANAR_YUV420, iw, ih, planes)
    assert [pair.owner[f"in{i}"] is pair.shards[0] for i in range(n)] == [False, True] * 4   # k-th registered input -> context k mod 2
    order = list(range(n))
    assert pair.update("out", W, H, _tiles(order, 0))
    shard = pair.shards[0]
    for k in range(frames_n):
        if k == 3:
            assert pair.update("out", W, H, _tiles(order, 24, 400))                      # the tiles shrink: their sizes change every frame
        if k == 18:
            assert pair.update("out", W, H, _tiles(order[::-1], 24, 400))                # halfway: the children change places
        if k == 27:
            assert pair.update("out", W, H, _tiles(order[::-1][2:] + order[::-1][:2], 8, 300))   # ... and the tile size changes again
        before_s, before_r = shard.kernel_launches(), pair.root.kernel_launches()
        pair.render_equal(0.020 * k, f"frame {k}")
        ran_s = {key: v - before_s[key] for key, v in shard.kernel_launches().items()}
        ran_r = {key: v - before_r[key] for key, v in pair.root.kernel_launches().items()}
        # the four remote tiles of the frame travel in ONE launch on their owner's stream, none by a copy of its own
        assert ran_s["move_rects"] == 1 and ran_r["move_rects"] == 0, (k, ran_s, ran_r)
        resampled = sum(ran_s[key] for key in ("ingest_wave", "ingest_wave_rgba", "ingest_valu", "resample_general"))
        assert resampled >= 1 and ran_s["compose_output"] == 0, (k, ran_s)               # the shard resamples its inputs, the root composes
        assert ran_r["compose_output"] == 1, (k, ran_r)
    pair.many.sync()


def test_configs3_geometry_with_a_transition_running_is_byte_equal_and_moves_in_one_launch(hip):
    pair = Pair(hip, shards=1)
    try:
        _configs3_run(hip, pair, 3840, 2160, 3840, 2160)
    finally:
        pair.close()


def test_the_shard_on_a_second_device(hip):
    """The mover's stores into PEER memory: the same run at 1080p with the shard on device 1."""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs (one renderer thread driving both)")
    pair = Pair(hip, devices=[1])
    try:
        _configs3_run(hip, pair, 1920, 1080, 1920, 1080)
    finally:
        pair.close()


IW, IH, W, H = 320, 180, 640, 360


def _small_inputs(hip, pair, n=4, fmt=None):
    for i in range(n):
        if fmt is None:
            pair.register_input(f"in{i}", hip.FRAME_PLANAR_YUV420, IW, IH, scenes.test_input(i, IW, IH, noise_seed=40 + i))
        else:
            rng = np.random.default_rng(60 + i)
            px = rng.integers(0, 256, (IH, IW, 4), dtype=np.uint8)
            pair.register_input(f"in{i}", fmt, IW, IH, [px])


def _inp(i, **kw):
    return dict({"type": "input_stream", "input_id": f"in{i}"}, **kw)


FALLBACK_SCENES = {
    # in1 and in3 live on the shard
    "one_to_one": {"type": "view", "background_color": "#203040FF", "children": [
        {"type": "view", "top": 11, "left": 17, "width": IW, "height": IH, "children": [_inp(1)]},
        {"type": "rescaler", "top": 200, "left": 300, "width": 200, "height": 120, "child": _inp(3)}]},
    "the_same_input_under_two_layouts": {"type": "view", "background_color": "#203040FF", "children": [
        {"type": "rescaler", "top": 0, "left": 0, "width": 400, "height": 225, "child": _inp(1)},
        {"type": "rescaler", "top": 150, "left": 350, "width": 250, "height": 200, "border_radius": 16, "child": _inp(1)},
        {"type": "view", "top": 230, "left": 5, "width": IW, "height": IH, "children": [_inp(1)]}]},
    "under_a_blur_shader": {"type": "view", "children": [
        {"type": "shader", "shader_id": "soften", "resolution": {"width": IW, "height": IH}, "shader_param": {"type": "f32", "value": 2.0}, "children": [_inp(3)]},
        {"type": "rescaler", "top": 180, "left": 320, "width": 320, "height": 180, "child": _inp(0)}]},
    "blur_of_another_size": {"type": "shader", "shader_id": "soften", "resolution": {"width": 500, "height": 300}, "shader_param": {"type": "f32", "value": 1.5},
                             "children": [_inp(1)]},
    "input_as_the_root": _inp(1),
    "nested_layout_node": {"type": "view", "background_color": "#204060FF", "children": [
        {"type": "shader", "shader_id": "soften", "resolution": {"width": 480, "height": 270}, "shader_param": {"type": "f32", "value": 2.5},
         "children": [{"type": "view", "width": 480, "height": 270, "background_color": "#FF0000FF", "children": [
             {"type": "rescaler", "width": 300, "height": 200, "border_radius": 20, "child": _inp(1)},
             {"type": "rescaler", "width": 180, "height": 100, "child": _inp(2)},
             {"type": "view", "top": 60, "left": 150, "width": IW, "height": IH, "children": [_inp(3)]}]}]},
        {"type": "rescaler", "top": 250, "left": 400, "width": 200, "height": 100, "child": _inp(3)}]},
    "tiles_of_four": scenes.cfg2_scene_json(4),
}


@pytest.mark.parametrize("name", sorted(FALLBACK_SCENES))
def test_what_cannot_travel_as_a_tile_falls_back_to_the_same_bytes(hip, name):
    pair = Pair(hip, shards=1)
    try:
        _small_inputs(hip, pair)
        for r in (pair.one, pair.many):
            r.register_shader("soften")
        assert pair.update("out", W, H, FALLBACK_SCENES[name])
        for k in range(3):   # (both alternating sets, and the first again)
            got = pair.render_equal(0.04 * k, f"{name} frame {k}")
        assert got["out"][0].std() > 3, "not a blank frame"
    finally:
        pair.close()


def test_a_non_opaque_remote_input_travels_as_its_raw_frame(hip):
    """(A frame with an alpha channel is never tiled on its owner: the root's smr_render_layouts has the matrix-core kernel's alpha builds for it,
    smr_ingest_resample_batch has not.)"""
    pair = Pair(hip, shards=1)
    try:
        _small_inputs(hip, pair, fmt=hip.FRAME_BGRA)
        for name in ("tiles_of_four", "one_to_one", "input_as_the_root"):
            assert pair.update("out", W, H, FALLBACK_SCENES[name])
            for k in range(2):
                pair.render_equal(0.04 * k, f"bgra {name} frame {k}")
    finally:
        pair.close()


def test_cpu_optimized_mode_moves_the_raw_frames(hip):
    pair = Pair(hip, shards=1, mode=hip.MODE_CPU_OPTIMIZED)
    try:
        _small_inputs(hip, pair)
        assert pair.update("out", W, H, scenes.cfg2_scene_json(4))
        before = pair.shards[0].kernel_launches()
        for k in range(3):
            pair.render_equal(0.04 * k, f"cpu optimized frame {k}")
        ran = {key: v - before[key] for key, v in pair.shards[0].kernel_launches().items()}
        assert ran["move_rects"] == 3 and ran["frame_to_rgba"] == 0, ran   # one launch per frame for the six planes; nothing is resampled on the shard
    finally:
        pair.close()


def test_stale_missing_and_unregistered_remote_inputs(hip):
    pair = Pair(hip, shards=1)
    try:
        _small_inputs(hip, pair)
        assert pair.update("out", W, H, scenes.cfg2_scene_json(4))
        fresh = {f"in{i}": 10.0 for i in range(4)}
        full = pair.render_equal(10.0, "all fresh", frame_pts_s=fresh)["out"]
        stale = pair.render_equal(10.0, "in1 stale", frame_pts_s=dict(fresh, in1=9.4))["out"]
        missing = pair.render_equal(10.0, "in1 missing", ids=["in0", "in2", "in3"], frame_pts_s=fresh)["out"]
        assert np.array_equal(stale[0], missing[0]) and not np.array_equal(stale[0], full[0])
        pair.both(lambda r: r.unregister_input("in3"))
        unreg = pair.render_equal(10.0, "in3 unregistered", frame_pts_s=fresh)["out"]
        assert not np.array_equal(unreg[0], full[0])
        # registered again it is the fifth registration: context 4 mod 2 = the root's
        pair.one.register_input("in3")
        pair.many.register_input("in3")
        assert pair.many.input_context("in3") is pair.root
        pair.f_many["in3"].destroy()
        pair.f_many["in3"] = pair.root.frame(hip.FRAME_PLANAR_YUV420, IW, IH, pair.f_one["in3"].download())
        again = pair.render_equal(10.0, "in3 back, on the root", frame_pts_s=fresh)["out"]
        assert np.array_equal(again[0], full[0])
    finally:
        pair.close()


def test_two_outputs(hip):
    pair = Pair(hip, shards=1)
    try:
        _small_inputs(hip, pair)
        assert pair.update("a", W, H, scenes.cfg2_scene_json(4))
        assert pair.update("b", 480, 270, FALLBACK_SCENES["one_to_one"], output_format=hip.FRAME_NV12)
        for k in range(3):
            got = pair.render_equal(0.04 * k, f"two outputs frame {k}")
        assert sorted(got) == ["a", "b"]
        pair.both(lambda r: r.unregister_output("a"))
        pair.render_equal(0.2, "one output left")
    finally:
        pair.close()


def _box(i, w, h, **kw):
    return {"type": "view", "background_color": "#203040FF", "children": [dict({"type": "rescaler", "top": 7.25, "left": 9.5, "width": w, "height": h, "child": _inp(i)}, **kw)]}


# in1 (160 x 90) and in3 (36 x 64) live on the shard.  The plan of each scene's one remote input -> does it travel as a tile the owner resamples?
ROUTE_SCENES = {
    "one_axis_horizontal": (_box(1, 159.25, 89.6), False),    # 160 x 90 -> 159 x 90
    "one_axis_vertical": (_box(3, 40, 63.25), False),         # 36 x 64 -> 36 x 63
    "box_pre_reduced": (_box(1, 32, 18), False),              # a fifth: a box pre-reduction, then the residual
    "vertical_first": (_box(1, 54, 40), True),                # 160 x 90 -> 54 x 30: the vertical scale is the larger one (both transpose)
    "two_passes_horizontal_first": (_box(1, 80, 45), True),   # a half
}


@pytest.mark.parametrize("name", sorted(ROUTE_SCENES))
def test_a_plan_the_owner_would_resample_on_another_route_travels_as_a_raw_frame(hip, name):
    """smr_render_layouts on the root and smr_ingest_resample_batch on an owner choose a resampling route each.  They choose alike for a
    two-pass plan without box pre-reduction of a Y'CbCr frame; for a one-axis plan and a pre-reduced one the root has matrix-core routes the
    batch entry point has not (it runs the general passes: the oracle's bytes, where the matrix-core kernel is within 1 LSB of them), so a
    tile made on the owner could differ from the single-context renderer's by one code.  Found by
    tests/test_gpu_scene_walk.py (recorded in tests/golden/scene_walk_one_axis_on_a_shard.json: a 96 x 54 input at 95 x 54 mid-transition, one byte
    of U); such an input travels as its raw
    planes and the root resamples it as the single-context renderer does."""
    from tests import scene_walk as SW
    scene, tiled = ROUTE_SCENES[name]
    pair = Pair(hip, shards=1)
    try:
        for i, (w, h) in enumerate([(160, 90), (160, 90), (128, 72), (36, 64)]):
            pair.register_input(f"in{i}", hip.FRAME_PLANAR_YUVJ420, w, h, SW.frame_planes(["yuvj420", w, h, 1061427712 + i]))
        assert pair.owner["in1"] is pair.shards[0] and pair.owner["in3"] is pair.shards[0]
        assert pair.update("out", 384, 216, scene)
        before = pair.shards[0].kernel_launches()
        for k in range(2):
            pair.render_equal(0.04 * k, f"{name} frame {k}")
        ran = {key: v - before[key] for key, v in pair.shards[0].kernel_launches().items()}
        resampled = sum(ran[key] for key in ("ingest_wave", "ingest_wave_rgba", "ingest_valu", "resample_general"))
        assert ran["move_rects"] == 2, ran
        assert (resampled >= 2) if tiled else (resampled == 0 and ran["frame_to_rgba"] == 0), (name, ran)
    finally:
        pair.close()


def _font_books():
    from tests import text_twin as TT
    try:
        return TT.NativeFontBook.system(), TT.NativeFontBook.system()
    except FileNotFoundError:
        return None


SHADER_OF = {"layout_planes.wgsl": "SHADER_LAYOUT_PLANES", "fade_to_ball.wgsl": "SHADER_FADE_TO_BALL", "color_output_with_texture_count.wgsl": "SHADER_COLOR_BY_TEXTURE_COUNT",
             "red_border.wgsl": "SHADER_RED_BORDER", "circle_layout.wgsl": "SHADER_CIRCLE_LAYOUT"}


def _has_text(component):
    if isinstance(component, dict):
        return component.get("type") == "text" or any(_has_text(v) for v in component.values())
    if isinstance(component, list):
        return any(_has_text(v) for v in component)
    return False


@pytest.mark.parametrize("case", ALL, ids=[f'{t["module"]}.{t["name"]}' for t in ALL])
def test_every_reference_scene_on_three_contexts(hip, case):
    """Every scene tests/test_gpu_reference_scenes.py renders — the 110 layout scenes and the 33 with Text / Image / Shader nodes — at every
    rendered pts (snapshots and the renders between them).  What the single-context renderer refuses, the sharded one refuses with the same
    words; nothing else is left out (odd output sizes included: both renderers take them or neither)."""
    from smelter_amd import _ffi
    from tests.test_gpu_reference_scenes import _bitmap, _input_planes
    mode = hip.MODE_GPU_OPTIMIZED if case["mode"] == "gpu_optimized" else hip.MODE_CPU_OPTIMIZED
    Wc, Hc = case["resolution"]
    books = None
    if any(_has_text(s["update"]) for s in case["steps"] if "update" in s):
        books = _font_books()
        if books is None:
            pytest.skip("no TrueType fonts on this machine (the single-context test skips too)")
    pair = Pair(hip, shards=2, mode=mode)
    try:
        if books:
            pair.one.set_fontbook(books[0])
            pair.many.set_fontbook(books[1])
        for inp in case["inputs"]:
            pair.register_input(inp["id"], hip.FRAME_PLANAR_YUV420, inp["width"], inp["height"], _input_planes(inp))
        for spec in case.get("renderers", []):
            for r in (pair.one, pair.many):
                if spec["kind"] == "image":
                    r.register_image(spec["id"], _bitmap(spec))
                else:
                    r.register_shader(spec["id"], getattr(_ffi, SHADER_OF[spec["wgsl"]]))
        rendered, active = 0, False
        for step in case["steps"]:
            if "update" in step:
                active = pair.update("output_1", Wc, Hc, step["update"]) or active
                continue
            if not active:
                continue
            pts_ms = step.get("snapshot_ms", step.get("render_ms"))
            pair.render_equal(pts_ms / 1e3, f'{case["name"]} @ {pts_ms} ms')
            rendered += 1
        assert rendered >= 1 or not active
    finally:
        pair.close()
        for b in books or ():
            b.close()


def test_refusals_leave_the_renderer_usable(hip):
    from smelter_amd.renderer import Renderer
    from smelter_amd.scene import SceneError
    a, b, c = hip.Context(0), hip.Context(0), hip.Context(0)
    cpu = hip.Context(0, mode=hip.MODE_CPU_OPTIMIZED)
    r = Renderer(a)
    try:
        with pytest.raises(SceneError, match="another rendering mode"):
            r.add_shard(cpu)
        with pytest.raises(SceneError, match="the renderer's own"):
            r.add_shard(a)
        r.add_shard(b)
        with pytest.raises(SceneError, match="a shard already"):
            r.add_shard(b)
        with pytest.raises(SceneError, match="lanes and shards do not combine"):
            r.add_lane(c)
        r.register_input("in0")
        r.register_input("in1")
        with pytest.raises(SceneError, match="before the first smr_renderer_register_input"):
            r.add_shard(c)
        with pytest.raises(SceneError, match="not registered"):
            r.input_context("nobody")
        assert r.input_context("in0") is a and r.input_context("in1") is b
        frames = {"in0": a.frame(hip.FRAME_PLANAR_YUV420, IW, IH, list(scenes.test_input(0, IW, IH))),
                  "in1": b.frame(hip.FRAME_PLANAR_YUV420, IW, IH, list(scenes.test_input(1, IW, IH)))}
        r.update_scene("out", W, H, scenes.cfg2_scene_json(2))
        assert r.render(0.0, frames)["out"].download()[0].std() > 3     # still renders
        d = hip.Context(0)
        lanes = Renderer(c, lanes=[d])
        with pytest.raises(SceneError, match="lanes and shards do not combine"):
            lanes.add_shard(b)
        lanes.register_input("in0")
        lanes.update_scene("out", W, H, scenes.cfg2_scene_json(1))
        f = c.frame(hip.FRAME_PLANAR_YUV420, IW, IH, list(scenes.test_input(0, IW, IH)))
        for k in range(2):
            assert lanes.render(0.04 * k, {"in0": f})["out"].download()[0].std() > 3
        lanes.close()
        d.close()
    finally:
        r.close()
        for x in (a, b, c, cpu):
            x.close()
