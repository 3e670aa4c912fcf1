"""User shaders on the device (include/smr.h "user shaders"): HIP C++ fragment functions compiled at registration, launched through
smr_user_shader and through Shader nodes of the renderer.  The seven built-in plane shaders restated in the user-shader language
(tests/user_shader_sources.py) are held (a) to the oracle's forward rasterisation with the thresholds tests/test_gpu_shaders.py uses for
the same arithmetic and (b), where no transcendental function is involved, to the built-in kernel byte for byte — same helper text,
same compiler flags: any difference is a defect of the new path.  Original shaders are held to bytes that follow from the contract."""
import json
import struct

import numpy as np
import pytest

from oracle import oracle as orc
from tests import refpipe, scenes
from tests import user_shader_sources as S
from tests.test_gpu_shaders import GRADIENT_RGB_EXPECTED, _check, _textures

pytestmark = pytest.mark.gpu

CIRCLES = [(10, 20, 300, 300, (0.0, 0.0, 1.0, 1.0)), (200, 50, 250, 200, (0.0, 0.25, 0.0, 0.5)), (400, 100, 240, 260, (0.0, 0.0, 0.0, 0.0))]


@pytest.fixture(scope="module")
def hip():
    from smelter_amd import hip as h
    return h


@pytest.fixture(scope="module")
def ctx(hip):
    c = hip.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def programs(hip):
    out = {name: hip.ShaderProgram(src) for name, src in S.ALL.items()}
    yield out
    for p in out.values():
        p.close()


def _run_user(ctx, program, textures, W, H, params=b"", time_s=0.0):
    srcs = [ctx.surface_from(t) for t in textures]
    dst = ctx.surface(W, H)
    dst.upload(np.full((H, W, 4), 77, np.uint8))  # stale contents must not show through the clear
    before = program.launches
    ctx.user_shader(program, srcs, dst, params, time_s)
    assert program.launches == before + 1
    return dst.download()


def _run_builtin(ctx, sid, textures, W, H, params=b"", time_s=0.0):
    srcs = [ctx.surface_from(t) for t in textures]
    dst = ctx.surface(W, H)
    dst.upload(np.full((H, W, 4), 77, np.uint8))
    ctx.builtin_shader(sid, srcs, dst, params, time_s)
    return dst.download()


# ---- 5: the seven restated built-ins
def test_gradient_reproduces_the_reference_golden_bytes_and_the_builtin(ctx, programs):
    got = _run_user(ctx, programs["gradient"], [], 8, 2)
    assert got.reshape(-1).tolist() == GRADIENT_RGB_EXPECTED
    big = _run_user(ctx, programs["gradient"], [], 640, 360)
    _check(big, orc.builtin_shader(orc.SHADER_GRADIENT, [], 640, 360), "gradient")
    assert np.array_equal(big, _run_builtin(ctx, orc.SHADER_GRADIENT, [], 640, 360))


@pytest.mark.parametrize("n_src", [0, 1, 2, 3])
def test_color_by_texture_count(ctx, programs, n_src):
    tex = _textures(n_src, 32, 18)
    got = _run_user(ctx, programs["color_by_texture_count"], tex, 64, 36)
    assert np.array_equal(got, orc.builtin_shader(orc.SHADER_COLOR_BY_TEXTURE_COUNT, tex, 64, 36))
    assert np.array_equal(got, _run_builtin(ctx, orc.SHADER_COLOR_BY_TEXTURE_COUNT, tex, 64, 36))


@pytest.mark.parametrize("size", [(640, 360), (333, 201)])
def test_red_border(ctx, programs, size):
    W, H = size
    tex = _textures(1, 160, 90)
    got = _run_user(ctx, programs["red_border"], tex, W, H)
    _check(got, orc.builtin_shader(orc.SHADER_RED_BORDER, tex, W, H), "red_border")
    builtin = _run_builtin(ctx, orc.SHADER_RED_BORDER, tex, W, H)
    assert np.array_equal(got, builtin), f"red_border: {(got != builtin).sum()} bytes differ from the built-in kernel"


@pytest.mark.parametrize("n_src", [0, 1, 2, 4, 5])
def test_layout_planes(ctx, programs, n_src):
    tex = _textures(n_src, 200, 120)
    got = _run_user(ctx, programs["layout_planes"], tex, 640, 360)
    _check(got, orc.builtin_shader(orc.SHADER_LAYOUT_PLANES, tex, 640, 360), f"layout_planes n={n_src}")
    builtin = _run_builtin(ctx, orc.SHADER_LAYOUT_PLANES, tex, 640, 360)
    assert np.array_equal(got, builtin), f"layout_planes n={n_src}: {(got != builtin).sum()} bytes differ from the built-in kernel"


@pytest.mark.parametrize("t", [0.0, 0.7, 1.9, 4.0])
def test_fade_to_ball(ctx, programs, t):
    tex = _textures(1, 320, 180)
    got = _run_user(ctx, programs["fade_to_ball"], tex, 640, 360, time_s=t)
    builtin = _run_builtin(ctx, orc.SHADER_FADE_TO_BALL, tex, 640, 360, time_s=t)
    print(f"fade_to_ball t={t}: {(got != builtin).sum()} bytes differ from the built-in kernel")
    _check(got, orc.builtin_shader(orc.SHADER_FADE_TO_BALL, tex, 640, 360, time=t),
           f"fade_to_ball t={t} ({(got != builtin).sum()} bytes differ from the built-in kernel)", identical=0.98)


@pytest.mark.parametrize("t", [0.0, 0.4, 1.3])
def test_silly(ctx, programs, t):
    tex = _textures(1, 320, 180)
    got = _run_user(ctx, programs["silly"], tex, 640, 360, time_s=t)
    builtin = _run_builtin(ctx, orc.SHADER_SILLY, tex, 640, 360, time_s=t)
    ref = orc.builtin_shader(orc.SHADER_SILLY, tex, 640, 360, time=t)
    d = np.abs(got.astype(np.int16) - ref.astype(np.int16))
    print(f"silly t={t}: within 1 {(d <= 1).mean():.5f}, identical {(d == 0).mean():.4f}; {(got != builtin).sum()} bytes differ from the built-in kernel")
    assert (d <= 1).mean() >= 0.999 and (d == 0).mean() >= 0.97, \
        f"silly t={t}: {(d <= 1).mean():.5f} / {(d == 0).mean():.4f} ({(got != builtin).sum()} bytes differ from the built-in kernel)"
    assert not _run_user(ctx, programs["silly"], [], 64, 36).any()


def test_circle_layout(ctx, programs):
    tex = _textures(3, 200, 200)
    params = orc.circle_layout_params(CIRCLES)
    got = _run_user(ctx, programs["circle_layout"], tex, 640, 360, params)
    builtin = _run_builtin(ctx, orc.SHADER_CIRCLE_LAYOUT, tex, 640, 360, params)
    print(f"circle_layout: {(got != builtin).sum()} bytes differ from the built-in kernel")
    _check(got, orc.builtin_shader(orc.SHADER_CIRCLE_LAYOUT, tex, 640, 360, params=params),
           f"circle_layout ({(got != builtin).sum()} bytes differ from the built-in kernel)", identical=0.99)
    assert not got[5, 5].any() and got[20, 10].tolist() == [0, 0, 255, 255]


# ---- 6: original shaders, expected bytes from the contract
@pytest.mark.parametrize("mode", ["gpu_optimized", "cpu_optimized"])
def test_swap_rb_is_exact_in_both_rendering_modes(hip, programs, mode):
    c = hip.Context(0, mode=hip.MODE_GPU_OPTIMIZED if mode == "gpu_optimized" else hip.MODE_CPU_OPTIMIZED)
    try:
        tex = _textures(2, 333, 201)[1]  # (the one with noise alpha)
        got = _run_user(c, programs["swap_rb"], [tex], 333, 201)
        want = tex[..., [2, 1, 0, 3]].copy()
        assert np.array_equal(got, want), f"{(got != want).sum()} bytes differ"
    finally:
        c.close()


@pytest.mark.parametrize("mode", ["gpu_optimized", "cpu_optimized"])
def test_param_fill_returns_its_parameter(hip, programs, mode):
    srgb = mode == "gpu_optimized"
    c = hip.Context(0, mode=hip.MODE_GPU_OPTIMIZED if srgb else hip.MODE_CPU_OPTIMIZED)
    try:
        rgba = (0.2, 0.45, 0.7, 0.8)
        got = _run_user(c, programs["param_fill"], [], 97, 41, struct.pack("<4f", *rgba))
        f32 = [float(np.float32(x)) for x in rgba]
        unorm = lambda x: int(np.float32(np.float32(x) * np.float32(255.0)) + np.float32(0.5))  # noqa: E731
        want = [orc.srgb_encode8(x) if srgb else unorm(x) for x in f32[:3]] + [unorm(f32[3])]
        assert (got.reshape(-1, 4) == np.array(want, np.uint8)).all(), (got[0, 0].tolist(), want)
    finally:
        c.close()


def test_vertex_stage_places_planes_in_quadrants(ctx, programs):
    tex = _textures(5, 16, 16)  # (the fifth plane is degenerate: it covers nothing)
    got = _run_user(ctx, programs["quadrant_colors"], tex, 64, 36)
    want = np.zeros((36, 64, 4), np.uint8)
    want[:18, :32] = [255, 0, 0, 255]
    want[:18, 32:] = [0, 255, 0, 255]
    want[18:, :32] = [0, 0, 255, 255]
    want[18:, 32:] = [0, 0, 0, 255]
    assert np.array_equal(got, want)
    two = _run_user(ctx, programs["quadrant_colors"], tex[:2], 64, 36)
    assert np.array_equal(two[:18], want[:18]) and not two[18:].any()  # the lower half was only cleared


def test_struct_list_parameter(ctx, programs):
    bands = [(2, 5, (1.0, 0.0, 0.0, 1.0)), (4, 10, (0.0, 1.0, 0.0, 1.0)), (30, 100, (0.0, 0.0, 1.0, 1.0))]
    params = b"".join(struct.pack("<2I4f", a, n, *c) for a, n, c in bands)
    got = _run_user(ctx, programs["bands"], [], 40, 36, params)
    want = np.zeros((36, 40, 4), np.uint8)
    want[2:4] = [255, 0, 0, 255]
    want[4:14] = [0, 255, 0, 255]
    want[30:] = [0, 0, 255, 255]
    assert np.array_equal(got, want)
    assert not _run_user(ctx, programs["bands"], [], 40, 36, b"").any()


# ---- 7: through the renderer
def _scene_and_params(W, H):
    lists = [[(20, 30, 280, 280, (0.0, 0.0, 1.0, 1.0)), (330, 40, 300, 300, (0.0, 0.0, 0.0, 0.0))],
             [(100, 10, 200, 320, (0.0, 0.5, 0.0, 0.5)), (300, 60, 320, 240, (0.25, 0.0, 0.0, 1.0))]]

    def entry(c):
        l, t, w, h, bg = c
        color = {"type": "list", "value": [{"type": "f32", "value": x} for x in bg]}
        return {"type": "struct", "value": [
            {"field_name": "left_px", "type": "u32", "value": l}, {"field_name": "top_px", "type": "u32", "value": t},
            {"field_name": "width_px", "type": "u32", "value": w}, {"field_name": "height_px", "type": "u32", "value": h},
            dict(field_name="background_color", **color)]}
    scene = {"type": "view", "background_color": "#102030FF", "children": [
        {"type": "shader", "shader_id": "circles_by_time", "resolution": {"width": W, "height": H},
         "shader_param": {"type": "list", "value": [entry(c) for cs in lists for c in cs]},
         "children": [{"type": "input_stream", "input_id": "in0"}, {"type": "input_stream", "input_id": "in1"}]},
        {"type": "rescaler", "width": 200, "height": 120, "top": 20, "left": 400, "child": {"type": "input_stream", "input_id": "in2"}},
    ]}
    return scene, lists


PTS = [0.0, 0.5, 1.0, 2.5]


def _render_scene(hip, program, fmt, lanes=0, shards=0):
    """-> (frames per pts, launches of `program`)"""
    from smelter_amd.renderer import Renderer
    iw, ih, W, H = 320, 180, 640, 360
    root = hip.Context(0)
    extra = [hip.Context(0) for _ in range(lanes + shards)]
    r = Renderer(root, lanes=extra[:lanes], shards=extra[lanes:])
    try:
        planes = [scenes.test_input(i, iw, ih, noise_seed=21 + i) for i in range(3)]
        frames = {}
        for i, p in enumerate(planes):
            r.register_input(f"in{i}")
            frames[f"in{i}"] = r.input_context(f"in{i}").frame(hip.FRAME_PLANAR_YUV420, iw, ih, list(p))
        r.register_shader_program("circles_by_time", program)
        scene, _ = _scene_and_params(W, H)
        r.update_scene("out", W, H, json.dumps(scene), output_format=fmt)
        before = program.launches
        out = []
        for t in PTS:
            out.append([np.asarray(p).copy() for p in r.render(t, frames, {k: t for k in frames})["out"].download()])
        r.sync()
        return out, program.launches - before, planes
    finally:
        r.close()
        for c in extra:
            c.close()
        root.close()


@pytest.mark.parametrize("fmt", ["rgba", "yuv420"])
def test_user_shader_scene_through_the_renderer_matches_the_oracle(hip, programs, fmt):
    """view -> [shader(user, two input streams), rescaler -> input stream]; shader_param a list of structs; the shader reads in.time."""
    from smelter_amd.scene import Scene
    iw, ih, W, H = 320, 180, 640, 360
    program = programs["circles_by_time"]
    got, launches, planes = _render_scene(hip, program, hip.FRAME_RGBA if fmt == "rgba" else hip.FRAME_PLANAR_YUV420)
    assert launches == len(PTS)  # one per frame and Shader node
    scene, lists = _scene_and_params(W, H)
    tex = [orc.planar_yuv_to_rgba(*p, iw, ih) for p in planes]
    sc = Scene()
    sc.update(scene, W, H)
    for t, frame in zip(PTS, got):
        layer = orc.builtin_shader(orc.SHADER_CIRCLE_LAYOUT, tex[:2], W, H, params=orc.circle_layout_params(lists[1 if t >= 1.0 else 0]))
        layouts = sc.layouts(0, int(t * 1e9), [(W, H), (iw, ih)])
        if fmt == "rgba":
            want = refpipe.layout_node_render(layouts, [layer, tex[2]], W, H)
            _check(frame[0].reshape(H, W, 4), want, f"scene t={t}", identical=0.99)
        else:
            want, _ = refpipe.render_yuv420(layouts, [layer, tex[2]], W, H)
            for g, w_ in zip(frame, want):
                assert refpipe.max_diff(g, w_) <= 1 and refpipe.exact_fraction(g, w_) >= 0.99, (t, refpipe.max_diff(g, w_), refpipe.exact_fraction(g, w_))
    assert not np.array_equal(got[0][0], got[2][0])  # in.time reached the shader


@pytest.mark.parametrize("extra", ["lane", "shard"])
def test_lanes_and_shards_render_the_user_shader_scene_to_the_same_bytes(hip, programs, extra):
    program = programs["circles_by_time"]
    single, n1, _ = _render_scene(hip, program, hip.FRAME_PLANAR_YUV420)
    many, n2, _ = _render_scene(hip, program, hip.FRAME_PLANAR_YUV420, lanes=1 if extra == "lane" else 0, shards=1 if extra == "shard" else 0)
    assert n1 == n2 == len(PTS)
    for a, b in zip(single, many):
        for pa, pb in zip(a, b):
            assert np.array_equal(pa, pb)


def test_register_shader_source_and_its_compile_error_through_the_renderer(ctx, hip):
    from smelter_amd.renderer import Renderer
    from smelter_amd.scene import SceneError
    r = Renderer(ctx)
    try:
        r.register_shader_source("fx", S.GRADIENT)
        scene = {"type": "shader", "shader_id": "fx", "resolution": {"width": 8, "height": 2}}
        r.update_scene("out", 8, 2, json.dumps(scene), output_format=hip.FRAME_RGBA)
        assert np.asarray(r.render(0.0, {})["out"].download()[0]).reshape(-1).tolist() == GRADIENT_RGB_EXPECTED
        with pytest.raises(SceneError) as e:
            r.register_shader_source("fx", S.BROKEN["unknown_identifier"][0])
        assert "smr_sample_nearest" in str(e.value)
        assert np.asarray(r.render(0.0, {})["out"].download()[0]).reshape(-1).tolist() == GRADIENT_RGB_EXPECTED  # the registry kept what it had
        r.register_shader_source("fx", S.COLOR_BY_TEXTURE_COUNT)  # re-registering replaces
        assert np.asarray(r.render(0.0, {})["out"].download()[0]).reshape(-1, 4)[0].tolist() == [255, 0, 0, 255]
        with pytest.raises(SceneError) as e:
            r.register_shader("fx", 99)
        assert "user WGSL is not supported" in str(e.value)
    finally:
        r.close()


# ---- 8: error paths
def test_invalid_arguments_launch_nothing(ctx, hip, programs):
    p = programs["param_fill"]
    before = p.launches
    dst = ctx.surface(32, 32)
    tex = _textures(1, 8, 8)[0]
    with pytest.raises(hip.SmrError) as e:
        ctx.user_shader(p, [], dst, b"\0" * (2048 + 4))
    assert e.value.code == -1 and "parameter bytes" in str(e.value)
    ctx.user_shader(p, [], dst, b"\0" * 2048)  # the cap itself is fine
    with pytest.raises(hip.SmrError) as e:
        ctx.user_shader(p, [], ctx.surface(32, 32, hip.PX_R8))
    assert e.value.code == -1 and "RGBA8" in str(e.value)
    with pytest.raises(hip.SmrError) as e:
        ctx.user_shader(p, [ctx.surface_from(tex)] * 17, dst)
    assert e.value.code == -1 and "16 sources" in str(e.value)
    with pytest.raises(hip.SmrError) as e:
        ctx.user_shader(p, [ctx.surface(8, 8, hip.PX_R8)], dst)
    assert e.value.code == -1 and "source 0" in str(e.value)
    assert p.launches == before + 1
    ctx.sync()


def test_a_program_outlives_the_context_that_loaded_it_and_loads_again(hip):
    """The module is unloaded with the last context of its device, or with the program, whichever goes first."""
    p = hip.ShaderProgram(S.GRADIENT)
    try:
        for _ in range(2):
            c = hip.Context(0)
            got = _run_user(c, p, [], 8, 2)
            c.close()
            assert got.reshape(-1).tolist() == GRADIENT_RGB_EXPECTED
        assert p.launches == 2
    finally:
        p.close()
    c = hip.Context(0)
    q = hip.ShaderProgram(S.GRADIENT)
    _run_user(c, q, [], 8, 2)
    q.close()  # the program first, then the context
    c.close()
