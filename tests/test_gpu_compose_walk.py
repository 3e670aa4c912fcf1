"""k_compose_output's copy workgroups on the device: runs of tiles with the next tile's texels requested ahead, paired stores on interior
tiles, one cold guard repair per block — the scenes of tests/test_emu_compose_walk.py (tests/compose_walk.py) through smr_render_layouts
into planar 4:2:0, NV12 and an RGBA8 node: EVERY BYTE EQUAL to the oracle's apply_layouts + output converters (no resampler runs: every
texture is drawn at its own size from whole-texel crops; the compositor adds no rounding of its own)."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests.compose_walk import FLAGGED_TEXTURE, OUTS, SIZES, flagged_scene, walk_scene

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from smelter_amd import hip as h
    orc.build()
    return h


@pytest.fixture(scope="module")
def ctx(hip):
    c = hip.Context(0)
    yield c
    c.close()


def oracle_planes(scene, W, H, out):
    rgba = orc.apply_layouts(W, H, scene[0], scene[1], srgb=True)
    planes = (rgba,) if out == "rgba" else orc.rgba_to_nv12(rgba) if out == "nv12" else orc.rgba_to_planar_yuv(rgba, orc.YUV420)
    return [np.asarray(p) for p in planes]


def device_sources(c, scene):
    srcs = []
    for s in scene[1]:
        t = c.surface_from(s)
        t.opaque = True   # (a resampled video tile: known to be opaque)
        srcs.append(t)
    return srcs


def render(c, hip, scene, W, H, out, target=None):
    """One smr_render_layouts call (the fused compositor, asserted) onto a poisoned output of the library's, or into `target`."""
    srcs = device_sources(c, scene)
    own = target is None
    if out == "rgba":
        target = c.surface(W, H)
        target.upload(np.full((H, W, 4), 0x5A, np.uint8))
        kw = {"out_rgba": target}
    else:
        if own:
            target = c.frame(hip.FRAME_NV12 if out == "nv12" else hip.FRAME_PLANAR_YUV420, W, H)
            target.upload([np.full(s, 0x5A, np.uint8) for s in target.plane_shapes()])
        kw = {"out": target}
    c.profile_reset()
    c.profile_enable(True)
    c.render_layouts(scene[0], srcs, W, H, **kw)
    c.sync()
    prof = c.profile_read()
    c.profile_enable(False)
    assert prof["fused_compose_output"][1] == 1 and prof["layouts"][1] == 0, f"left the fused compositor: {prof}"
    if not own:
        return None
    got = target.download()
    target.destroy()
    return [got] if out == "rgba" else list(got)


def assert_same(got, want, what):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        w = np.asarray(w).reshape(g.shape)
        assert np.array_equal(g, w), (what, "plane", k, int((g != w).sum()), np.argwhere(g != w)[:5].tolist())


@pytest.mark.parametrize("out", OUTS)
@pytest.mark.parametrize("W,H", SIZES)
def test_runs_and_paired_stores_are_the_oracle_byte_for_byte(ctx, hip, W, H, out):
    scene = walk_scene(W, H)
    assert_same(render(ctx, hip, scene, W, H, out), oracle_planes(scene, W, H, out), (W, H, out))


@pytest.mark.parametrize("out", OUTS)
def test_blocks_with_flagged_values_are_the_oracle_byte_for_byte(ctx, hip, out):
    """(the texture: tests/compose_walk.py; the CPU test asserts the file is what the fast path's own enumeration gives)"""
    scene = flagged_scene(np.load(FLAGGED_TEXTURE))
    assert_same(render(ctx, hip, scene, 128, 16, out), oracle_planes(scene, 128, 16, out), ("flagged texture", out))


def test_a_wrapped_frame_with_tight_rows_of_odd_pitch_takes_the_per_lane_stores(ctx, hip):
    """Planar output in the caller's memory, rows of 386 and 193 bytes on pitches 388 and 196: not the multiples of 8 and 4 the paired stores
    need — the per-lane stores, the oracle's bytes, and no byte outside the texels written (tests/wrapped.py)."""
    import torch
    from tests.wrapped import WrappedFrame
    W, H = 386, 50
    wf = WrappedFrame(torch, ctx, hip.FRAME_PLANAR_YUV420, W, H, "tight", 5)
    assert wf.dests[0].pitch % 8 != 0 and wf.dests[1].pitch % 4 == 0
    scene = walk_scene(W, H)
    render(ctx, hip, scene, W, H, "planar", target=wf.frame)
    assert_same(wf.planes("compose walk"), oracle_planes(scene, W, H, "planar"), "wrapped tight planar 386 x 50")
    for sfc in wf.frame.surfaces:
        sfc.destroy()
