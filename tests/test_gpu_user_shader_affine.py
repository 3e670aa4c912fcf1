"""The affine vertex stage, smr_load and smr_dimensions of user shaders on the device: the fixtures of tests/user_shader_sources_affine.py
compiled by smr_shader_program_create and launched through smr_user_shader and through a Shader node of the renderer, held to the numpy
model of tests/test_emu_user_shader_affine.py (same sizes, same planes, same cap on the pixels an edge passes too close to)."""
import json
import struct
import types

import numpy as np
import pytest

from oracle import oracle as orc
from tests import refpipe, scenes
from tests import test_emu_user_shader_affine as M
from tests import user_shader_sources_affine as SA

pytestmark = pytest.mark.gpu

W, H, SW, SH = M.W, M.H, M.SW, M.SH


@pytest.fixture(scope="module")
def hip():
    from smelter_amd import hip as h
    return h


@pytest.fixture(scope="module")
def programs(hip):
    out = {name: hip.ShaderProgram(src) for name, src in SA.ALL.items()}
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


@pytest.mark.parametrize("srgb", [True, False])
def test_an_axis_aligned_affine_plane_is_the_smr_plane_one_byte_for_byte(contexts, programs, srgb):
    tex = M.sources()[:1]
    as_plane = _run(contexts[srgb], programs["plane_param"], tex, W, H, M.pack([[0.5, 0.25, 0.1, -0.2]]))
    as_affine = _run(contexts[srgb], programs["affine_param"], tex, W, H, M.pack([[0.5, 0.0, 0.0, 0.25, 0.1, -0.2]]))
    assert as_plane.any() and not as_plane.all(axis=-1).all()
    assert np.array_equal(as_plane, as_affine), f"{(as_plane != as_affine).sum()} bytes differ"
    M.compare(as_affine, *M.model([[0.5, 0.0, 0.0, 0.25, 0.1, -0.2]], tex, W, H, srgb), "axis-aligned")


@pytest.mark.parametrize("srgb", [True, False])
def test_rotated_planes_match_the_model(contexts, programs, srgb):
    got = _run(contexts[srgb], programs["affine_param"], M.sources(), W, H, M.pack(M.ROTATION))
    M.compare(got, *M.model(M.ROTATION, M.sources(), W, H, srgb), "rotation")


@pytest.mark.parametrize("srgb", [True, False])
def test_planes_that_end_a_pixel_past_a_wave_span_boundary_match_the_model(contexts, programs, srgb):
    """the wave early-out must not drop a plane for a span that holds one pixel of it"""
    got = _run(contexts[srgb], programs["affine_param"], M.sources(), W, H, M.pack(M.SPAN_EDGE))
    want, doubt, margin = M.model(M.SPAN_EDGE, M.sources(), W, H, srgb)
    M.compare(got, want, doubt, margin, "span edge")
    assert np.array_equal(got.any(axis=-1), want.any(axis=-1))


@pytest.mark.parametrize("srgb", [False, True])
def test_smr_load_reproduces_the_source_tiled(contexts, programs, srgb):
    tex = M.sources()[1]
    got = _run(contexts[srgb], programs["tile"], [tex], W, H)
    want = np.tile(tex, (H // SH + 1, W // SW + 1, 1))[:H, :W]
    assert np.array_equal(got, want), f"{(got != want).sum()} bytes differ"


def test_smr_load_and_smr_dimensions_out_of_range_and_absent(contexts, programs):
    tex = M.sources()[0]
    n = len(M.PROBES) + 1
    got = _run(contexts[False], programs["probe"], [tex, None], n, 2, b"".join(struct.pack("<3i", *p) for p in M.PROBES))
    assert np.array_equal(got, M.probe_expected(tex, n)), got.tolist()
    assert not _run(contexts[False], programs["tile"], [None], 8, 2).any()


# ---- through the renderer: the rotating shader over one input stream
IW, IH, OW, OH, PTS = M.IW, M.IH, M.OW, M.OH, M.PTS


def test_the_rotating_shader_through_the_renderer_matches_the_model(hip, programs):
    """view -> shader(rotate, one 16 x 8 input stream) at two pts values, composed like the scenes of tests/test_gpu_user_shaders.py"""
    from smelter_amd.renderer import Renderer
    from smelter_amd.scene import Scene
    scene = {"type": "view", "background_color": "#102030FF", "children": [
        {"type": "shader", "shader_id": "rotate", "resolution": {"width": OW, "height": OH},
         "children": [{"type": "input_stream", "input_id": "in0"}]}]}
    program = programs["rotate"]
    root = hip.Context(0)
    r = Renderer(root)
    try:
        planes = scenes.test_input(0, IW, IH, noise_seed=21)
        r.register_input("in0")
        frames = {"in0": r.input_context("in0").frame(hip.FRAME_PLANAR_YUV420, IW, IH, list(planes))}
        r.register_shader_program("rotate", program)
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
        layer, doubt, margin = M.model(M.rotate_planes(float(np.float32(t)), 1, [(IW, IH)], OW, OH), [tex], OW, OH, True)
        assert layer.any(axis=-1).mean() > 0.1
        want = refpipe.layout_node_render(sc.layouts(0, int(t * 1e9), [(OW, OH)]), [layer], OW, OH)
        M.compare(frame, want, doubt, margin, f"renderer t={t}")
    assert not np.array_equal(got[0], got[1])  # in.time reached the vertex stage
