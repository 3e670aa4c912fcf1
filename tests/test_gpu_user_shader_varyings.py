"""Varyings of user shaders on the device: the fixtures of tests/user_shader_sources_varyings.py compiled by smr_shader_program_create and
launched through smr_user_shader, through a Shader node of the renderer and into wrapped targets, held to the numpy model of
tests/test_emu_user_shader_varyings.py (same cases, same planes, same caps).  Nothing here loops, retries or is meant to fault: the NaN of
the flat-varying case is a word in a register."""
import json
import types

import numpy as np
import pytest

from oracle import oracle as orc
from tests import refpipe, scenes
from tests import test_emu_user_shader_clip as M
from tests import test_emu_user_shader_varyings as V
from tests import user_shader_sources_clip as SC
from tests import user_shader_sources_varyings as SV
from tests.test_emu_user_shader_affine import compare, encode, sources

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
    out = {name: hip.ShaderProgram(src) for name, src in SV.ALL.items()}
    out["clip_param"] = hip.ShaderProgram(SC.CLIP_PARAM)
    yield out
    for p in out.values():
        p.close()


@pytest.fixture(scope="module")
def contexts(hip):
    out = {True: hip.Context(0, mode=hip.MODE_GPU_OPTIMIZED), False: hip.Context(0, mode=hip.MODE_CPU_OPTIMIZED)}
    yield out
    for c in out.values():
        c.close()


ABSENT = types.SimpleNamespace(handle=None)


def _run(ctx, program, textures, Wt, Ht, params=b"", time_s=0.0):
    srcs = [ABSENT if t is None else ctx.surface_from(t) for t in textures]
    dst = ctx.surface(Wt, Ht)
    dst.upload(np.full((Ht, Wt, 4), 77, np.uint8))  # stale contents must not show through the clear
    ctx.user_shader(program, srcs, dst, params, time_s)
    return dst.download()


@pytest.mark.parametrize("srgb", [True, False])
@pytest.mark.parametrize("case", sorted(V.SMOOTH_CASES))
def test_interpolated_varyings_match_the_model(contexts, programs, case, srgb):
    fixture, planes, modes, tex, size, params = V.SMOOTH_CASES[case]
    got = _run(contexts[srgb], programs[fixture], tex(), *size, params)
    m = V.model(planes, modes, tex(), *size, srgb, V.encode_fragment)
    V.check(got, m, case)
    if not m[1].any():
        V.same_coverage(got, m)


@pytest.mark.parametrize("srgb", [True, False])
def test_equal_varyings_on_the_identity_quad_give_one_colour_drawn_once(contexts, programs, srgb):
    got = _run(contexts[srgb], programs["vary_param"], sources()[:1], 8, 8, V.pack_planes(V.IDENTITY_V))
    want = V.model(V.IDENTITY_V, SV.VARY_MODES, sources()[:1], 8, 8, srgb, V.encode_fragment)[0]
    assert (got == got[0, 0]).all(axis=-1).all(), "the 64 pixels are not all equal"
    assert np.abs(got[0, 0].astype(int) - want[0, 0].astype(int)).max() <= 1 and got[0, 0, 3] == 128, (got[0, 0], want[0, 0])


@pytest.mark.parametrize("srgb", [True, False])
def test_dyadic_varyings_are_exact_and_linear_equals_perspective_where_w_is_one(contexts, programs, srgb):
    tex = sources()[:1]
    linear = _run(contexts[srgb], programs["vary_param"], tex, 64, 8, V.pack_planes(V.TIE_V))
    persp = _run(contexts[srgb], programs["vary_persp"], tex, 64, 8, V.pack_planes(V.TIE_V))
    assert np.array_equal(linear, persp), f"{(linear != persp).sum()} bytes differ"
    m = V.model(V.TIE_V, SV.VARY_MODES, tex, 64, 8, srgb, V.encode_fragment)
    assert linear.any(axis=-1).sum() == 32 * 4 and np.abs(linear.astype(int) - m[0].astype(int)).max() <= 1
    for cover, r in zip(m[4][0], (0.375, 0.125)):
        assert cover.any() and (linear[cover][:, 0] == encode(np.array([r, 0.0, 0.0, 0.5]), srgb)[0]).all()


@pytest.mark.parametrize("srgb", [True, False])
def test_a_flat_varying_is_the_provoking_vertex_word_bit_for_bit(contexts, programs, srgb):
    V.check_flat_bits(_run(contexts[srgb], programs["vary_flat_bits"], sources(), W, H, V.pack_planes(V.FLIP_BITS)), srgb)


@pytest.mark.parametrize("srgb", [True, False])
@pytest.mark.parametrize("case", sorted(V.POSITION_CASES))
def test_position_z_and_w_match_the_model(contexts, programs, case, srgb):
    planes, tex = V.POSITION_CASES[case]
    got = _run(contexts[srgb], programs["vary_position"], tex(), W, H, V.pack_planes(planes))
    V.check(got, V.model(planes, "P", tex(), W, H, srgb, V.position_fragment), f"position {case}")


@pytest.mark.parametrize("srgb", [True, False])
@pytest.mark.parametrize("case", sorted(V.UNUSED_CASES))
def test_declaring_varyings_changes_neither_coverage_nor_uv(contexts, programs, case, srgb):
    planes, tex, size = V.UNUSED_CASES[case]
    without = _run(contexts[srgb], programs["clip_param"], tex(), *size, M.pack_planes(planes))
    with_them = _run(contexts[srgb], programs["vary_unused"], tex(), *size, M.pack_planes(planes))
    assert without.any() and np.array_equal(without, with_them), f"{(without != with_them).sum()} bytes differ"


# ---- through the renderer: the lit card over one input stream
IW, IH, OW, OH, PTS = M.IW, M.IH, M.OW, M.OH, M.PTS


def test_the_lit_card_through_the_renderer_matches_the_model(hip, programs):
    """view -> shader(lit, one 16 x 8 input stream) at the three pts values of the card test, composed like its scene"""
    from smelter_amd.renderer import Renderer
    from smelter_amd.scene import Scene
    scene = {"type": "view", "background_color": "#102030FF", "children": [
        {"type": "shader", "shader_id": "lit", "resolution": {"width": OW, "height": OH},
         "children": [{"type": "input_stream", "input_id": "in0"}]}]}
    program = programs["lit"]
    root = hip.Context(0)
    r = Renderer(root)
    try:
        planes = scenes.test_input(0, IW, IH, noise_seed=21)
        r.register_input("in0")
        frames = {"in0": r.input_context("in0").frame(hip.FRAME_PLANAR_YUV420, IW, IH, list(planes))}
        r.register_shader_program("lit", program)
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
        layer, doubt, margin, counts, _ = V.model(V.lit_planes(M.f32(t), 1, [(IW, IH)], OW, OH), V.LIT_MODES, [tex], OW, OH, True, V.lit_fragment)
        assert layer.any() == (t < 1.5)  # (at 2.0 rad the card shows its back: the frame is the view's background alone)
        want = refpipe.layout_node_render(sc.layouts(0, int(t * 1e9), [(OW, OH)]), [layer], OW, OH)
        compare(frame, want, doubt, margin if t < 1.5 else 1.0, f"renderer t={t}")
    assert not np.array_equal(got[0], got[1]) and not np.array_equal(got[1], got[2])  # in.time reached the vertex stage
    assert (got[2] == got[2][0, 0]).all()


# ---- into a surface the library does not own
@pytest.mark.parametrize("srgb", [True, False])
def test_varyings_into_a_wrapped_target(torch, hip, contexts, programs, srgb):
    """nothing outside the texels is written, the texels equal those of a library-owned surface (tests/test_gpu_write_footprint.py's helper
    asserts both over the three geometries of tests/wrapped.py) and satisfy the model"""
    from tests.test_gpu_write_footprint import _into_surface
    c = contexts[srgb]
    srcs = [c.surface_from(t) for t in sources()]
    for Wt, Ht in [(65, 5), (1, 1)]:
        got = _into_surface(torch, c, Wt, Ht, lambda d: c.user_shader(programs["vary_param"], srcs, d, V.pack_planes(V.FLIP_V)), "user_shader varyings")
        m = V.model(V.FLIP_V, SV.VARY_MODES, sources(), Wt, Ht, srgb, V.encode_fragment)
        V.check(got, m, f"wrapped {Wt}x{Ht}")
        V.same_coverage(got, m)
    for t in srcs:
        t.destroy()
