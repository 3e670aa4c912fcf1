"""SVG image assets end to end on the GPU (include/smr.h: smr_renderer_register_svg_image / _unregister_image / _svg_stats; SvgAsset,
smelter-render/src/transformations/image/svg_image.rs): the host's rasteriser is asked, inside update_scene, for the asset at every NODE size
the scene shows it at; the pixmaps are fixed up in place by k_svg_nodes (one launch per 16 new rasters) and the nodes sample the rasters.

The bytes are held against existing, independent code: the device's own smr_remove_premultiplied_alpha -> smr_add_premultiplied_alpha chain
on the same pixmap (byte for byte; both entry points are held to the oracle by tests/test_gpu_parity.py::test_premultiply), and the oracle's
chain under that test's own rule (<= 1 LSB, >= 0.999 of the bytes identical) on the texels whose stage-one bytes the device and the oracle
agree on — at most 0.1 % of the texels may be left out, the complement of the 0.999 that test grants stage one."""
import numpy as np
import pytest

from oracle import oracle as orc
from smelter_amd.scene import SceneError

pytestmark = pytest.mark.gpu

TOL = 1  # tests/test_gpu_parity.py


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
def ctx_cpu(hip):
    c = hip.Context(0, mode=hip.MODE_CPU_OPTIMIZED)
    yield c
    c.close()


def exhaustive():
    """256 x 256: alpha = the row, R = the column, G and B the column under two fixed permutations — every (c, alpha) in every channel."""
    c = np.arange(256, dtype=np.uint8)
    px = np.empty((256, 256, 4), np.uint8)
    px[..., 0] = c[None, :]
    px[..., 1] = np.random.default_rng(1).permutation(c)[None, :]
    px[..., 2] = np.random.default_rng(2).permutation(c)[None, :]
    px[..., 3] = c[:, None]
    return px


def noise(w, h, seed=0, opaque=False):
    """Seeded random valid premultiplied bytes (c <= alpha) at w x h."""
    rng = np.random.default_rng((seed, w, h))
    px = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    if opaque:
        px[..., 3] = 255
    px[..., :3] = (px[..., :3].astype(np.uint32) * px[..., 3:4] // 255).astype(np.uint8)
    return px


def disc(w, h):
    """A premultiplied anti-aliased disc that fills the box, drawn analytically at w x h: what a vector rasteriser does and a rescale does not."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    d = np.hypot((x + 0.5 - w / 2) / (w / 2), (y + 0.5 - h / 2) / (h / 2))
    cover = np.clip((1.0 - d) * min(w, h) / 2 + 0.5, 0.0, 1.0)
    a = np.rint(cover * 255).astype(np.uint32)
    px = np.empty((h, w, 4), np.uint8)
    for k, c in enumerate((230, 120, 40)):
        px[..., k] = (c * a + 127) // 255
    px[..., 3] = a
    return px


class Rasteriser:
    """The fixture's host side: `draw(w, h)` makes the pixmap, every call is recorded, `fail` lists sizes it raises for."""

    def __init__(self, draw, fail=()):
        self.draw, self.fail, self.calls = draw, set(fail), []

    def __call__(self, w, h):
        self.calls.append((w, h))
        if (w, h) in self.fail:
            raise RuntimeError(f"no raster at {w}x{h}")
        return self.draw(w, h)


def device_chain(c, px):
    """What the two existing passes make of a pixmap on context c: (stage one, both stages)."""
    one = c.remove_premultiplied_alpha(c.surface_from(px))
    return one.download(), c.add_premultiplied_alpha(one).download()


def frame(r, w, h, pts_ns=0):
    r.render_packed(pts_ns, r.make_frame_set({}))
    return np.array(r.output(0).download()[0]).reshape(h, w, 4)


def column(sizes, image_id="logo"):
    """Image nodes of the given sizes stacked from the top left corner of a transparent view: node i covers rows sum(h[:i]) .. of the frame."""
    return {"type": "view", "direction": "column", "children": [{"type": "image", "image_id": image_id, "width": w, "height": h} for w, h in sizes]}


def node_rows(got, sizes):
    y = 0
    for w, h in sizes:
        yield got[y:y + h, :w]
        y += h


def renderer(c, **kw):
    from smelter_amd.renderer import Renderer
    return Renderer(c, **kw)


@pytest.mark.parametrize("name", ["exhaustive_256x256", "noise_67x17"])
def test_bytes(ctx, ctx_cpu, hip, name):
    px = exhaustive() if name.startswith("exhaustive") else noise(67, 17, seed=5)
    h, w = px.shape[:2]
    r = renderer(ctx)
    try:
        ras = Rasteriser(lambda w_, h_: px)
        r.register_svg_image("logo", w, h, ras)
        assert r.svg_stats() == (0, 0, 0) and ras.calls == []          # nothing is rasterised at registration
        r.update_scene("out", w, h, {"type": "image", "image_id": "logo"}, hip.FRAME_RGBA)
        assert ras.calls == [(w, h)] and r.svg_stats() == (1, 1, 1)
        got = frame(r, w, h)
        assert r.image_launches() == 0
    finally:
        r.close()
    one, both = device_chain(ctx, px)
    diff = np.argwhere(got != both)
    assert diff.size == 0, f"texel (x {diff[0][1]}, y {diff[0][0]}) {px[diff[0][0], diff[0][1]]}: {got[diff[0][0], diff[0][1]]}, the two passes give {both[diff[0][0], diff[0][1]]}"
    # the oracle's chain, on the texels whose stage one the device and the oracle agree on
    one_orc = orc.remove_premultiplied_alpha(px)
    keep = (one == one_orc).all(axis=2)
    left_out = 1.0 - float(keep.mean())
    want = orc.add_premultiplied_alpha(one_orc, True)
    d = np.abs(got[keep].astype(np.int32) - want[keep].astype(np.int32))
    exact = float((d == 0).mean())
    print(f"{name}: {left_out:.5%} of texels left out (stage one differs); max |diff| {d.max()} LSB, {exact:.5f} of bytes identical to the oracle")
    assert left_out <= 0.001, f"{left_out:.5%} of the texels differ from the oracle after stage one (> 0.1 %)"
    assert d.max() <= TOL, f"{d.max()} LSB from the oracle"
    assert exact >= 0.999, f"only {exact:.5f} of bytes identical to the oracle"
    # CPU-optimized: the pixmap's bytes are the node's, and nothing is launched
    r = renderer(ctx_cpu)
    try:
        r.register_svg_image("logo", w, h, Rasteriser(lambda w_, h_: px))
        r.update_scene("out", w, h, {"type": "image", "image_id": "logo"}, hip.FRAME_RGBA)
        assert (frame(r, w, h) == px).all()
        assert r.svg_stats() == (1, 0, 1)
    finally:
        r.close()


def test_rasterised_at_the_node_size(ctx, hip):
    sizes = [(64, 64), (160, 100)]
    r = renderer(ctx)
    try:
        ras = Rasteriser(disc)
        r.register_svg_image("logo", 64, 64, ras)
        r.update_scene("out", 160, 164, column(sizes), hip.FRAME_RGBA)
        assert sorted(ras.calls) == sizes                               # exactly those two sizes, once each
        assert r.svg_stats() == (2, 1, 2)
        got = frame(r, 160, 164)
        small, large = node_rows(got, sizes)
        fixed_small, fixed_large = device_chain(ctx, disc(64, 64))[1], device_chain(ctx, disc(160, 100))[1]
        assert (small == fixed_small).all()
        assert (large == fixed_large).all(), "the 160 x 100 node is not the fix-up of what the rasteriser returned for 160 x 100"
        rescaled = orc.rescale_bilinear(fixed_small, 160, 100)
        assert np.abs(large.astype(np.int32) - rescaled.astype(np.int32)).max() > 8, "the large node looks like a rescale of the small raster"
        assert r.image_launches() == 0
        # the same scene again: nothing to rasterise; dropping the large node releases its raster
        r.update_scene("out", 160, 164, column(sizes), hip.FRAME_RGBA)
        assert len(ras.calls) == 2 and r.svg_stats() == (2, 1, 2)
        assert (frame(r, 160, 164) == got).all()
        r.update_scene("out", 160, 164, column(sizes[:1]), hip.FRAME_RGBA)
        assert len(ras.calls) == 2 and r.svg_stats() == (2, 1, 1)
        assert (frame(r, 160, 164)[:64, :64] == fixed_small).all()
    finally:
        r.close()


def test_seventeen_sizes_are_two_launches(ctx, hip):
    sizes = [(3 + 4 * i, 2 + i) for i in range(17)]                     # 3 x 2 .. 67 x 18: below, at and above one 64-wide tile
    W, H = max(w for w, _ in sizes), sum(h for _, h in sizes)
    r = renderer(ctx)
    try:
        ras = Rasteriser(lambda w, h: noise(w, h, seed=17))
        r.register_svg_image("logo", 40, 40, ras)
        r.update_scene("out", W, H, column(sizes), hip.FRAME_RGBA)
        assert r.svg_stats() == (17, 2, 17) and sorted(ras.calls) == sorted(sizes)
        got = frame(r, W, H)
        for (w, h), node in zip(sizes, node_rows(got, sizes)):
            assert (node == device_chain(ctx, noise(w, h, seed=17))[1]).all(), f"the {w} x {h} node"
        assert r.image_launches() == 0
    finally:
        r.close()


def test_a_failing_rasteriser_refuses_the_update(ctx, hip):
    sizes = [(20, 10), (30, 12)]
    r = renderer(ctx)
    try:
        ras = Rasteriser(lambda w, h: noise(w, h, seed=3), fail=[(31, 9)])
        r.register_svg_image("logo", 20, 10, ras)
        r.update_scene("out", 32, 24, column(sizes), hip.FRAME_RGBA)
        before = frame(r, 32, 24)
        stats = r.svg_stats()
        with pytest.raises(SceneError) as e:
            r.update_scene("out", 32, 24, column([(8, 8), (31, 9), (9, 9)]), hip.FRAME_RGBA)
        assert '"logo"' in str(e.value) and "31x9" in str(e.value) and "no raster at 31x9" in str(e.value)
        assert ras.calls[-1] == (31, 9) and r.svg_stats() == (stats[0] + 2, stats[1], stats[2])   # (8 x 8 was made, and released again)
        assert [(n.width, n.height) for n in r.nodes("out")][1:] == sizes                             # the previous scene is the active one
        assert (frame(r, 32, 24, pts_ns=40_000_000) == before).all()
    finally:
        r.close()


def test_opaque_under_a_rescaler_on_two_lanes_and_unregistration(ctx, hip):
    scene = {"type": "view", "background_color": "#204060FF", "children": [
        {"type": "rescaler", "child": {"type": "image", "image_id": "logo", "width": 50, "height": 30}}]}
    frames = []
    for lanes in (0, 1):
        extra = [hip.Context(0) for _ in range(lanes)]
        r = renderer(ctx, lanes=extra)
        try:
            ras = Rasteriser(lambda w, h: noise(w, h, seed=9, opaque=True))
            r.register_svg_image("logo", 25, 15, ras)
            r.update_scene("out", 96, 54, scene, hip.FRAME_RGBA)
            assert ras.calls == [(50, 30)]                              # the node's size, not the rescaler's: once, whatever the lanes
            frames.append([frame(r, 96, 54, pts_ns=k * 40_000_000) for k in range(4)])
            with pytest.raises(SceneError, match="a scene uses"):
                r.unregister_image("logo")
            r.unregister_output("out")
            assert r.svg_stats()[2] == 0
            r.unregister_image("logo")
            with pytest.raises(SceneError, match="does not exist"):
                r.update_scene("out", 96, 54, scene, hip.FRAME_RGBA)
            r.register_svg_image("logo", 25, 15, ras)                   # the id is free again
            r.update_scene("out", 96, 54, scene, hip.FRAME_RGBA)
            assert ras.calls == [(50, 30), (50, 30)]
            assert (frame(r, 96, 54) == frames[-1][0]).all()
        finally:
            r.close()
            for c in extra:
                c.close()
    assert frames[0][0][27, 48, 3] == 255 and len(np.unique(frames[0][0][..., :3])) > 50   # (the asset is on screen)
    for k in range(4):
        assert (frames[0][k] == frames[1][k]).all(), f"frame {k}: two lanes differ from one"
