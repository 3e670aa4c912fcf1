"""Screen-space derivatives of user shaders on the device: the fixtures of tests/user_shader_sources_derivatives.py compiled by
smr_shader_program_create and launched through smr_user_shader, through a Shader node of the renderer and into wrapped targets, held to the
numpy model of tests/test_emu_user_shader_derivatives.py (same cases, same planes, same caps).  Programs are compiled once per module.
Nothing here loops, retries or is meant to fault: a helper's extrapolated value is a word in a register."""
import json
import types

import numpy as np
import pytest

from oracle import oracle as orc
from tests import refpipe, scenes
from tests import test_emu_user_shader_clip as M
from tests import test_emu_user_shader_derivatives as D
from tests import test_emu_user_shader_varyings as V
from tests import user_shader_sources_derivatives as SD
from tests.test_emu_user_shader_affine import compare, pack, sources

pytestmark = pytest.mark.gpu

W, H = D.W, D.H


@pytest.fixture(scope="module")
def hip():
    from smelter_amd import hip as h
    return h


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


@pytest.fixture(scope="module")
def programs(hip):
    out = {name: hip.ShaderProgram(src) for name, src in SD.ALL.items()}
    out.update({name: hip.ShaderProgram(src) for name, src in SD.ORIGINALS.items()})
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
@pytest.mark.parametrize("size", D.SIZES_1)
@pytest.mark.parametrize("flavour", sorted(SD.FLAVOURS))
def test_the_derivatives_of_position_are_exact(contexts, programs, flavour, size, srgb):
    D.check_position(_run(contexts[srgb], programs[f"position_{flavour}"], [], *size), SD.FLAVOURS[flavour], size, srgb)


@pytest.mark.parametrize("srgb", [True, False])
@pytest.mark.parametrize("which", sorted(D.EDGE_PLANES))
@pytest.mark.parametrize("flavour", sorted(SD.FLAVOURS))
def test_helpers_on_a_plane_edge_give_the_edge_pixels_their_derivatives(contexts, programs, flavour, which, srgb):
    got = _run(contexts[srgb], programs[f"edge_{flavour}"], sources()[:1], 64, 8, pack([D.EDGE_PLANES[which][0]]))
    D.check_edge(got, SD.FLAVOURS[flavour], which, srgb)


@pytest.mark.parametrize("srgb", [True, False])
@pytest.mark.parametrize("axis", ["x", "y"])
def test_fine_takes_the_pixels_own_row_and_coarse_the_quads_first(contexts, programs, axis, srgb):
    D.check_product(_run(contexts[srgb], programs[f"product_{axis}"], [], 8, 8), axis, srgb)


@pytest.mark.parametrize("srgb", [True, False])
@pytest.mark.parametrize("size", D.DISC_SIZES)
def test_an_anti_aliased_disc_by_fwidth_matches_the_model(contexts, programs, size, srgb):
    got = _run(contexts[srgb], programs["disc"], sources(), *size)
    D.check(got, D.disc_model(sources(), size, srgb), f"disc {size}")


@pytest.mark.parametrize("srgb", [True, False])
@pytest.mark.parametrize("case", sorted(D.OVERLAP_CASES))
def test_overlapping_rotated_planes_with_fwidth_match_the_model(contexts, programs, case, srgb):
    got = _run(contexts[srgb], programs["overlap"], sources(), W, H, pack(D.OVERLAP_CASES[case]))
    D.check(got, D.overlap_model(case, srgb), case)


@pytest.mark.parametrize("srgb", [True, False])
@pytest.mark.parametrize("case", sorted(D.PERSPECTIVE_CASES))
def test_derivatives_in_perspective_match_the_model(contexts, programs, case, srgb):
    planes, tex, size = D.PERSPECTIVE_CASES[case]
    got = _run(contexts[srgb], programs["perspective"], tex(), *size, V.pack_planes(planes))
    D.check(got, D.perspective_model(case, srgb), case)


@pytest.mark.parametrize("srgb", [True, False])
@pytest.mark.parametrize("case", sorted(D.REMAP))
def test_the_quad_lane_map_draws_the_same_picture(contexts, programs, case, srgb):
    fixture, _, tex, size, params = D.REMAP[case]
    before = _run(contexts[srgb], programs[fixture], tex(), *size, params)
    after = _run(contexts[srgb], programs[f"remap_{fixture}"], tex(), *size, params)
    assert before.any() and np.array_equal(before, after), f"{(before != after).sum()} bytes differ"


# ---- through the renderer: the disc shader over one input stream
IW, IH, OW, OH = M.IW, M.IH, 48, 24  # (three target pixels per texel: no centre on a texel boundary; the disc of 19 pixels crosses x = 32)
PTS = [0.0, 0.9]


def test_the_disc_shader_through_the_renderer_matches_the_model(hip, programs):
    """view -> shader(disc, one 16 x 8 input stream), composed like its scene"""
    from smelter_amd.renderer import Renderer
    from smelter_amd.scene import Scene
    scene = {"type": "view", "background_color": "#102030FF", "children": [
        {"type": "shader", "shader_id": "disc", "resolution": {"width": OW, "height": OH},
         "children": [{"type": "input_stream", "input_id": "in0"}]}]}
    program = programs["disc"]
    root = hip.Context(0)
    r = Renderer(root)
    try:
        planes = scenes.test_input(0, IW, IH, noise_seed=21)
        r.register_input("in0")
        frames = {"in0": r.input_context("in0").frame(hip.FRAME_PLANAR_YUV420, IW, IH, list(planes))}
        r.register_shader_program("disc", program)
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
    layer, doubt, margin, loose, _ = D.disc_model([tex], (OW, OH), True)
    assert not doubt.any() and not loose.any() and (layer[..., 3] == 0).any() and (layer[..., 3] == 255).any()
    for t, frame in zip(PTS, got):
        want = refpipe.layout_node_render(sc.layouts(0, int(t * 1e9), [(OW, OH)]), [layer], OW, OH)
        compare(frame, want, doubt, margin, f"renderer t={t}")
    assert np.array_equal(got[0], got[1])  # (the disc does not move)


# ---- into a surface the library does not own
@pytest.mark.parametrize("srgb", [True, False])
def test_derivatives_into_a_wrapped_target(torch, hip, contexts, programs, srgb):
    """nothing outside the texels is written — the helpers outside an odd target store nothing — and the texels equal those of a
    library-owned surface (tests/test_gpu_write_footprint.py's helper asserts both over the three geometries of tests/wrapped.py)"""
    from tests.test_gpu_write_footprint import _into_surface
    c = contexts[srgb]
    got = _into_surface(torch, c, 67, 5, lambda d: c.user_shader(programs["position_fine"], [], d, b""), "user_shader derivatives of position")
    D.check_position(got, "_fine", (67, 5), srgb)
    srcs = [c.surface_from(t) for t in sources()[:1]]
    got = _into_surface(torch, c, 64, 8, lambda d: c.user_shader(programs["edge_plain"], srcs, d, pack([D.EDGE_PLANES["odd"][0]])), "user_shader helpers on an edge")
    D.check_edge(got, "", "odd", srgb)
    for t in srcs:
        t.destroy()
