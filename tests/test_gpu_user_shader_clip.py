"""The clip vertex stage of user shaders on the device: the fixtures of tests/user_shader_sources_clip.py compiled by
smr_shader_program_create and launched through smr_user_shader, through a Shader node of the renderer and into wrapped targets, held to the
numpy model of tests/test_emu_user_shader_clip.py (same sizes, same planes, same cap on the pixels an edge passes too close to)."""
import json
import types

import numpy as np
import pytest

from oracle import oracle as orc
from tests import refpipe, scenes
from tests import test_emu_user_shader_clip as M
from tests import user_shader_sources_clip as SC

pytestmark = pytest.mark.gpu

W, H = M.W, M.H


@pytest.fixture(scope="module")
def hip():
    from smelter_amd import hip as h
    return h


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


@pytest.fixture(scope="module")
def programs(hip):
    out = {name: hip.ShaderProgram(src) for name, src in SC.ALL.items()}
    yield out
    for p in out.values():
        p.close()


@pytest.fixture(scope="module")
def contexts(hip):
    out = {True: hip.Context(0, mode=hip.MODE_GPU_OPTIMIZED), False: hip.Context(0, mode=hip.MODE_CPU_OPTIMIZED)}
    yield out
    for c in out.values():
        c.close()


ABSENT = types.SimpleNamespace(handle=None)  # a NULL entry in smr_user_shader's `src`


def _run(ctx, program, textures, Wt, Ht, params=b"", time_s=0.0):
    srcs = [ABSENT if t is None else ctx.surface_from(t) for t in textures]
    dst = ctx.surface(Wt, Ht)
    dst.upload(np.full((Ht, Wt, 4), 77, np.uint8))  # stale contents must not show through the clear
    ctx.user_shader(program, srcs, dst, params, time_s)
    return dst.download()


def _same_coverage(got, m):
    assert np.array_equal(got.any(axis=-1), m[0].any(axis=-1))  # (no pixel is doubtful: coverage is exactly the model's)


@pytest.mark.parametrize("srgb", [True, False])
@pytest.mark.parametrize("size", [(W, H), (65, 5), (1, 1)])
def test_overlapping_planes_in_perspective_match_the_model(contexts, programs, srgb, size):
    got = _run(contexts[srgb], programs["clip_param"], M.sources(), *size, M.pack_planes(M.FLIP))
    m = M.model(M.FLIP, M.sources(), *size, srgb)
    M.check(got, m, f"flip {size}")
    _same_coverage(got, m)


@pytest.mark.parametrize("srgb", [True, False])
def test_a_plane_that_passes_behind_the_eye_matches_the_model(contexts, programs, srgb):
    got = _run(contexts[srgb], programs["clip_param"], M.sources()[:1], W, H, M.pack_planes(M.BEHIND))
    M.check(got, M.model(M.BEHIND, M.sources()[:1], W, H, srgb), "behind the eye")
    assert got[:, :42].any() and not got[:, 42:].any()


@pytest.mark.parametrize("srgb", [True, False])
def test_the_depth_range_clips_per_pixel(contexts, programs, srgb):
    tex = M.sources()[:1]
    clipped = _run(contexts[srgb], programs["clip_param"], tex, W, H, M.pack_planes(M.DEPTH))
    free = _run(contexts[srgb], programs["clip_param"], tex, W, H, M.pack_planes(M.DEPTH_FREE))
    mc, mf = M.model(M.DEPTH, tex, W, H, srgb), M.model(M.DEPTH_FREE, tex, W, H, srgb)
    M.check(clipped, mc, "depth clipped")
    M.check(free, mf, "within the depth range")
    sure = ~(mc[1] | mf[1])
    assert np.array_equal((clipped != free).any(axis=-1)[sure], (mc[0] != mf[0]).any(axis=-1)[sure]) and (mc[0] != mf[0]).any()


@pytest.mark.parametrize("name", sorted(M.NOTHING))
def test_back_facing_degenerate_and_nan_planes_cover_nothing(contexts, programs, name):
    got = _run(contexts[True], programs["clip_param"], M.sources()[:1], W, H, M.pack_planes([M.NOTHING[name]]))
    assert not got.any(), f"{name}: {np.count_nonzero(got.any(axis=-1))} pixels drawn"


@pytest.mark.parametrize("srgb", [True, False])
def test_edges_through_pixel_centres_follow_the_top_left_rule_byte_for_byte(contexts, programs, srgb):
    tex = M.sources()[:1]
    as_plane = _run(contexts[srgb], programs["plane_param"], tex, 64, 8, M.pack([M.TIE_PLANE]))
    as_clip = _run(contexts[srgb], programs["clip_param"], tex, 64, 8, M.pack_planes(M.TIE))
    cover = as_plane.any(axis=-1)
    assert cover[2:6, 16:48].all() and cover.sum() == 32 * 4
    assert np.array_equal(as_plane, as_clip), f"{(as_plane != as_clip).sum()} bytes differ"
    want = M.model(M.TIE, tex, 64, 8, srgb)[0]
    assert np.abs(as_clip.astype(int) - want.astype(int)).max() <= 1


@pytest.mark.parametrize("srgb", [True, False])
def test_the_shared_diagonal_is_drawn_once(contexts, programs, srgb):
    got = _run(contexts[srgb], programs["clip_half"], [], 8, 8, M.pack_planes(M.IDENTITY))
    want = M.model(M.IDENTITY, [], 8, 8, srgb, fragment=M.constant_fragment, first=-1)[0]
    assert (got == got[0, 0]).all(axis=-1).all(), "the 64 pixels are not all equal"
    assert np.abs(got[0, 0].astype(int) - want[0, 0].astype(int)).max() <= 1 and got[0, 0, 3] == 128, (got[0, 0], want[0, 0])


@pytest.mark.parametrize("srgb", [True, False])
def test_planes_that_end_a_pixel_past_a_wave_span_boundary_match_the_model(contexts, programs, srgb):
    got = _run(contexts[srgb], programs["clip_param"], M.sources(), W, H, M.pack_planes(M.SPAN))
    m = M.model(M.SPAN, M.sources(), W, H, srgb)
    M.check(got, m, "span")
    _same_coverage(got, m)


@pytest.mark.parametrize("srgb", [True, False])
def test_sixteen_planes_each_from_its_own_slot_of_the_table(contexts, programs, srgb):
    tex = M.grid_sources()
    got = _run(contexts[srgb], programs["clip_param"], tex, W, H, M.pack_planes(M.GRID))
    m = M.model(M.GRID, tex, W, H, srgb)
    M.check(got, m, "grid")
    _same_coverage(got, m)


def test_no_sources_is_one_plane_with_plane_id_minus_one(contexts, programs):
    got = _run(contexts[True], programs["clip_half"], [], W, H, M.pack_planes(M.FLIP[:1]))
    m = M.model(M.FLIP[:1], [], W, H, True, fragment=M.constant_fragment, first=-1)
    M.check(got, m, "no sources")
    _same_coverage(got, m)
    assert got.any()


def test_an_absent_source_in_the_middle_keeps_the_others_in_their_slots(contexts, programs):
    tex = M.grid_sources()[:3]
    tex[1] = None
    got = _run(contexts[True], programs["clip_param"], tex, W, H, M.pack_planes(M.GRID[:3]))
    m = M.model([M.GRID[0], M.GRID[2]], [tex[0], tex[2]], W, H, True)
    M.check(got, m, "absent source")
    _same_coverage(got, m)


# ---- through the renderer: the card shader over one input stream
IW, IH, OW, OH, PTS = M.IW, M.IH, M.OW, M.OH, M.PTS


def test_the_card_shader_through_the_renderer_matches_the_model(hip, programs):
    """view -> shader(flip, one 16 x 8 input stream) at three pts values, composed like the scene of tests/test_gpu_user_shader_affine.py"""
    from smelter_amd.renderer import Renderer
    from smelter_amd.scene import Scene
    scene = {"type": "view", "background_color": "#102030FF", "children": [
        {"type": "shader", "shader_id": "flip", "resolution": {"width": OW, "height": OH},
         "children": [{"type": "input_stream", "input_id": "in0"}]}]}
    program = programs["flip"]
    root = hip.Context(0)
    r = Renderer(root)
    try:
        planes = scenes.test_input(0, IW, IH, noise_seed=21)
        r.register_input("in0")
        frames = {"in0": r.input_context("in0").frame(hip.FRAME_PLANAR_YUV420, IW, IH, list(planes))}
        r.register_shader_program("flip", program)
        r.update_scene("out", OW, OH, json.dumps(scene), output_format=hip.FRAME_RGBA)
        before = program.launches
        got = [np.asarray(r.render(t, frames, {"in0": t})["out"].download()[0]).reshape(OH, OW, 4).copy() for t in PTS]
        r.sync()
        assert program.launches == before + len(PTS)
    finally:
        r.close()
        root.close()
    tex = orc.planar_yuv_to_rgba(*planes, IW, IH)
    sc = Scene()
    sc.update(scene, OW, OH)
    for t, frame in zip(PTS, got):
        layer, doubt, margin, counts = M.model(M.flip_planes(M.f32(t), 1, [(IW, IH)], OW, OH), [tex], OW, OH, True)
        assert layer.any() == (t < 1.5)  # (at 2.0 rad the card shows its back: the frame is the view's background alone)
        want = refpipe.layout_node_render(sc.layouts(0, int(t * 1e9), [(OW, OH)]), [layer], OW, OH)
        M.compare(frame, want, doubt, margin if t < 1.5 else 1.0, f"renderer t={t}")
    assert not np.array_equal(got[0], got[1]) and not np.array_equal(got[1], got[2])  # in.time reached the vertex stage
    assert (got[2] == got[2][0, 0]).all()


# ---- into a surface the library does not own
@pytest.mark.parametrize("srgb", [True, False])
def test_the_clip_stage_into_a_wrapped_target(torch, hip, contexts, programs, srgb):
    """nothing outside the texels is written, the texels equal those of a library-owned surface (tests/test_gpu_write_footprint.py's helper
    asserts both over the three geometries of tests/wrapped.py) and satisfy the model"""
    from tests.test_gpu_write_footprint import _into_surface
    c = contexts[srgb]
    srcs = [c.surface_from(t) for t in M.sources()]
    for Wt, Ht in [(65, 5), (1, 1)]:
        got = _into_surface(torch, c, Wt, Ht, lambda d: c.user_shader(programs["clip_param"], srcs, d, M.pack_planes(M.FLIP)), "user_shader clip")
        m = M.model(M.FLIP, M.sources(), Wt, Ht, srgb)
        M.check(got, m, f"wrapped {Wt}x{Ht}")
        _same_coverage(got, m)
    for t in srcs:
        t.destroy()
