"""Animated image assets end to end on the GPU (include/smr.h: smr_renderer_register_animated_image; AnimatedAsset,
smelter-render/src/transformations/image/animated_image.rs:41-149): an Image node of an animated asset shows, at every render, the frame of
that pts on the node's own clock — so a renderer with the animated asset and one with the chosen frame registered as a STATIC image must
produce the same bytes, at the node's own size and scaled, in both rendering modes.  Also: the clock across scene updates (the reference's
gif_progress_between_updates), per-frame opacity, the image pass's launch counts (one k_image_nodes launch per 16 scaled nodes), lanes, and
k_image_nodes itself through the library against smr_rescale_bilinear (byte for byte) and the oracle (the bar of
tests/test_gpu_parity.py::test_rescale_bilinear: <= 1 LSB, >= 0.99 of the bytes identical)."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as orc

pytestmark = pytest.mark.gpu

MS = 1_000_000
DELAYS = [100 * MS, 200 * MS, 50 * MS, 150 * MS]     # frame starts at 0, 100, 300, 350 ms; the loop is 500 ms
WORKED = [(49, 0), (50, 0), (51, 1), (200, 1), (201, 2), (325, 2), (326, 3), (499, 3), (500, 0)]   # (t in ms, frame)
SHAPES = [(160, 90, 1, 1), (160, 90, 65, 5), (3, 2, 67, 9), (5, 5, 5, 5), (7, 3, 3, 7), (64, 16, 128, 32)]   # tests/test_emu_image_nodes.py's


@pytest.fixture(scope="module")
def hip():
    from smelter_amd import hip as h
    return h


@pytest.fixture(scope="module", params=[True, False], ids=["gpu_optimized", "cpu_optimized"])
def ctx(hip, request):
    c = hip.Context(0, mode=hip.MODE_GPU_OPTIMIZED if request.param else hip.MODE_CPU_OPTIMIZED)
    c.srgb = request.param
    yield c
    c.close()


def noise_asset(seed, n=4, w=12, h=10):
    """n frames of noise with varying alpha, [n, h, w, 4] straight RGBA8."""
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 4), dtype=np.uint8)


ASSETS = {"gif": noise_asset(1), "gif2": noise_asset(2)}


def make_renderer(ctx, animated, lanes=()):
    """A renderer with ASSETS registered as animated images (`animated`) or with every frame of them as a static image "<asset>_<k>"."""
    from smelter_amd.renderer import Renderer
    r = Renderer(ctx, lanes=lanes)
    for name, frames in ASSETS.items():
        if animated:
            r.register_animated_image(name, frames, DELAYS)
        else:
            for k in range(frames.shape[0]):
                r.register_image(f"{name}_{k}", frames[k])
    return r


def render(r, pts_ns):
    r.render_packed(pts_ns, r.make_frame_set({}))
    return [np.array(p) for p in r.output(0).download()]


def same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and (x == y).all() for x, y in zip(a, b))


def two_nodes(image_id):
    """The asset at its own size and scaled to 37 x 21, over a background both blend with."""
    return {"type": "view", "background_color": "#204060FF", "children": [
        {"type": "image", "id": "own", "image_id": image_id},
        {"type": "image", "id": "scaled", "image_id": image_id, "width": 37, "height": 21}]}


@pytest.fixture(scope="module", params=["rgba_64x36", "yuv420_128x72"])
def output(hip, request):
    return {"rgba_64x36": (64, 36, hip.FRAME_RGBA), "yuv420_128x72": (128, 72, hip.FRAME_PLANAR_YUV420)}[request.param]


def test_animated_equals_static_at_every_worked_time(ctx, output):
    W, H, fmt = output
    still, anim = make_renderer(ctx, False), make_renderer(ctx, True)
    try:
        want = []
        for k in range(4):
            still.update_scene("out", W, H, two_nodes(f"gif_{k}"), fmt)
            want.append(render(still, 0))
        assert not same(want[0], want[1]) and not same(want[2], want[3])   # (the frames differ: equality below means something)
        anim.update_scene("out", W, H, two_nodes("gif"), fmt)
        for t_ms, k in WORKED + [(0, 0), (1551, 1)]:
            assert same(render(anim, t_ms * MS), want[k]), f"t = {t_ms} ms: not the bytes of frame {k} as a static image"
        # to the nanosecond around the first tie
        assert same(render(anim, 50 * MS + 1), want[1]) and same(render(anim, 50 * MS), want[0])
    finally:
        still.close()
        anim.close()


def test_progress_across_updates(ctx, hip):
    """gif_progress_between_updates (integration-tests/src/render_tests/image.rs:184) and what follows from image_component.rs:91-120."""
    W, H, fmt = 64, 36, hip.FRAME_RGBA
    still, anim = make_renderer(ctx, False), make_renderer(ctx, True)
    try:
        def want(image):
            still.update_scene("out", W, H, two_nodes(image), fmt)
            return render(still, 0)
        anim.update_scene("out", W, H, two_nodes("gif"), fmt)
        assert same(render(anim, 0), want("gif_0"))
        assert same(render(anim, 260 * MS), want("gif_2"))
        anim.update_scene("out", W, H, two_nodes("gif"), fmt)             # the identical component: the clock runs on
        assert same(render(anim, 360 * MS), want("gif_3"))                # t = 360 ms, not 360 - 260 = 100 ms (frame 1)
        anim.update_scene("out", W, H, two_nodes("gif2"), fmt)            # another asset under the same ids: its clock starts at the last render
        assert same(render(anim, 360 * MS), want("gif2_0"))
        assert same(render(anim, (360 + 51) * MS), want("gif2_1"))
        assert same(render(anim, (360 + 326) * MS), want("gif2_3"))
        # a component without an id restarts on every update
        anon = {"type": "view", "background_color": "#204060FF", "children": [{"type": "image", "image_id": "gif", "width": 37, "height": 21}]}

        def want_anon(k):
            still.update_scene("out", W, H, {**anon, "children": [{**anon["children"][0], "image_id": f"gif_{k}"}]}, fmt)
            return render(still, 0)
        P = (360 + 326) * MS
        anim.update_scene("out", W, H, anon, fmt)
        assert same(render(anim, P + 201 * MS), want_anon(2))
        anim.update_scene("out", W, H, anon, fmt)
        assert same(render(anim, P + 252 * MS), want_anon(1))             # 51 ms after the restart (a clock kept would say 252 ms: frame 2)
    finally:
        still.close()
        anim.close()


def test_opaque_and_translucent_frames_alternate(ctx, hip):
    """Frames 0 and 2 are opaque, 1 and 3 are not: the opaque-layer hand-off (SMR_SOURCE_OPAQUE_SURFACE) is decided per frame, and either way
    the bytes are those of the static twin."""
    from smelter_amd.renderer import Renderer
    W, H, fmt = 128, 72, hip.FRAME_PLANAR_YUV420
    frames = np.random.default_rng(5).integers(0, 256, (4, 32, 64, 4), dtype=np.uint8)
    frames[0, ..., 3] = 255
    frames[2, ..., 3] = 255
    frames[3, 7, 9, 3] = 254

    def scene(image_id):
        return {"type": "view", "background_color": "#203040FF", "children": [
            {"type": "view", "top": 8, "left": 16, "width": 64, "height": 32, "children": [{"type": "image", "image_id": image_id}]},
            {"type": "view", "top": 20, "left": 40, "width": 60, "height": 30, "background_color": "#FFFFFF60", "border_radius": 6}]}
    still, anim = Renderer(ctx), Renderer(ctx)
    try:
        anim.register_animated_image("flip", frames, DELAYS)
        anim.update_scene("out", W, H, scene("flip"), fmt)
        for k in range(4):
            still.register_image(f"flip_{k}", frames[k])
        for t_ms, k in [(0, 0), (51, 1), (201, 2), (326, 3), (500, 0)]:
            still.update_scene("out", W, H, scene(f"flip_{k}"), fmt)
            assert same(render(anim, t_ms * MS), render(still, 0)), f"frame {k} ({'opaque' if k % 2 == 0 else 'translucent'})"
    finally:
        still.close()
        anim.close()


def row_of(ids, sizes):
    return {"type": "view", "background_color": "#102030FF", "children": [
        {"type": "image", "image_id": i, "width": w, "height": h} for i, (w, h) in zip(ids, sizes)]}


def test_the_image_pass_is_one_launch_per_sixteen_scaled_nodes(ctx, hip):
    W, H, fmt = 128, 72, hip.FRAME_RGBA
    still, anim = make_renderer(ctx, False), make_renderer(ctx, True)
    try:
        for r in (still, anim):
            r.register_image("logo", ASSETS["gif2"][3])
        sizes8 = [(9 + i, 9 + (i % 3)) for i in range(8)]
        ids8 = ["gif", "logo", "gif2", "gif", "logo", "gif2", "logo", "gif"]          # 5 animated, 3 static, all scaled
        anim.update_scene("out", W, H, row_of(ids8, sizes8), fmt)
        n0 = anim.image_launches()
        got = [render(anim, 0), render(anim, 51 * MS), render(anim, 326 * MS)]
        assert anim.image_launches() - n0 == 3                                         # one launch per render, eight jobs at first, then five
        for (t_ms, k), g in zip([(0, 0), (51, 1), (326, 3)], got):
            still.update_scene("out", W, H, row_of([i if i == "logo" else f"{i}_{k}" for i in ids8], sizes8), fmt)
            assert same(g, render(still, 0)), f"t = {t_ms} ms"
        # only static nodes remain: drawn once into the new graph's surfaces, then never again
        anim.update_scene("out", W, H, row_of(["logo"] * 3, sizes8[:3]), fmt)
        n0 = anim.image_launches()
        first = render(anim, 400 * MS)
        assert anim.image_launches() - n0 == 1
        assert same(render(anim, 440 * MS), first) and same(render(anim, 480 * MS), first)
        assert anim.image_launches() - n0 == 1
        still.update_scene("out", W, H, row_of(["logo"] * 3, sizes8[:3]), fmt)
        assert same(first, render(still, 0))
        assert still.image_launches() == 4                                             # (its static nodes: drawn once per update above)
        # 17 scaled animated nodes: two launches per render
        sizes17 = [(6 + (i % 2), 5 + (i % 4)) for i in range(17)]
        ids17 = ["gif" if i % 3 else "gif2" for i in range(17)]
        anim.update_scene("out", W, H, row_of(ids17, sizes17), fmt)
        n0 = anim.image_launches()
        a, b = render(anim, 500 * MS), render(anim, 700 * MS)                            # clocks started at 480 ms: t = 20 ms, 220 ms
        assert anim.image_launches() - n0 == 4
        for g, k in ((a, 0), (b, 2)):
            still.update_scene("out", W, H, row_of([f"{i}_{k}" for i in ids17], sizes17), fmt)
            assert same(g, render(still, 0)), f"frame {k}"
    finally:
        still.close()
        anim.close()


def test_lanes_render_the_single_lane_frames(ctx, hip):
    W, H, fmt = 128, 72, hip.FRAME_PLANAR_YUV420
    lane = hip.Context(0, mode=hip.MODE_GPU_OPTIMIZED if ctx.srgb else hip.MODE_CPU_OPTIMIZED)
    one, two = make_renderer(ctx, True), make_renderer(ctx, True, lanes=[lane])
    try:
        scene = {"type": "view", "background_color": "#204060FF", "children": [
            {"type": "image", "image_id": "gif", "width": 37, "height": 21}, {"type": "image", "image_id": "gif2"},
            {"type": "image", "image_id": "gif2", "width": 50, "height": 44}]}
        for r in (one, two):
            r.update_scene("out", W, H, scene, fmt)
        for t_ms in (0, 51, 120, 201, 326, 499):
            assert same(render(two, t_ms * MS), render(one, t_ms * MS)), f"t = {t_ms} ms"
        assert two.image_launches() == one.image_launches() == 6
    finally:
        one.close()
        two.close()
        lane.close()


def test_a_single_frame_is_a_static_image(ctx, hip):
    from smelter_amd.renderer import Renderer
    from smelter_amd.scene import SceneError
    W, H, fmt = 64, 36, hip.FRAME_RGBA
    a, b = Renderer(ctx), Renderer(ctx)
    try:
        a.register_animated_image("pic", ASSETS["gif"][2:3], [123])
        b.register_image("pic", ASSETS["gif"][2])
        for r in (a, b):
            r.update_scene("out", W, H, two_nodes("pic"), fmt)
        for pts in (0, 77 * MS, 10**12):
            assert same(render(a, pts), render(b, pts))
        assert a.image_launches() == b.image_launches() == 1                            # a static node: drawn once
        # what registration refuses (the messages of AnimatedAsset::new, the static call's for the rest)
        with pytest.raises(SceneError, match="does not contain any frames"):
            a.register_animated_image("none", ASSETS["gif"][:0], [])
        with pytest.raises(SceneError, match="over 1000 frames"):
            a.register_animated_image("many", np.zeros((1001, 1, 1, 4), np.uint8), [1] * 1001)
        with pytest.raises(SceneError, match="INT64_MAX"):
            a.register_animated_image("long", ASSETS["gif"][:2], [2**63 - 1, 1])
        with pytest.raises(SceneError, match="already registered"):
            a.register_animated_image("pic", ASSETS["gif"], DELAYS)
        a.register_animated_image("thousand", np.full((1000, 1, 2, 4), 200, np.uint8), [MS] * 1000)   # the most the reference takes
        a.update_scene("out", W, H, two_nodes("thousand"), fmt)
        render(a, 999 * MS + 400_000)
    finally:
        a.close()
        b.close()


def _image_nodes(ctx):
    fn = ctx.lib.smr_image_nodes   # the internal export the renderer's image pass calls (not part of smr.h)
    fn.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_uint32]
    fn.restype = C.c_int
    return fn


def premultiplied(rng, w, h):
    px = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    px[..., :3] = (px[..., :3].astype(np.uint32) * px[..., 3:4] // 255).astype(np.uint8)
    return px


@pytest.mark.parametrize("n_jobs", [1, 6, 17])
def test_k_image_nodes_writes_the_bytes_of_rescale_bilinear(ctx, n_jobs):
    rng = np.random.default_rng(40 + n_jobs)
    shapes = [SHAPES[i % len(SHAPES)] for i in range(n_jobs)] if n_jobs > 1 else [SHAPES[1]]
    shapes = [(sw, sh, dw + 3 * (i // len(SHAPES)), dh + i // len(SHAPES)) for i, (sw, sh, dw, dh) in enumerate(shapes)]
    px = [premultiplied(rng, sw, sh) for sw, sh, _, _ in shapes]
    srcs = [ctx.surface_from(p) for p in px]
    dsts = [ctx.surface(dw, dh) for _, _, dw, dh in shapes]
    refs = [ctx.surface(dw, dh) for _, _, dw, dh in shapes]
    try:
        arr = lambda ss: (C.c_void_p * len(ss))(*[s.handle for s in ss])
        ctx._check(_image_nodes(ctx)(ctx.handle, arr(srcs), arr(dsts), len(srcs)))
        for s, d in zip(srcs, refs):
            ctx.rescale_bilinear(s, d)
        for i, (sw, sh, dw, dh) in enumerate(shapes):
            got, ref = dsts[i].download(), refs[i].download()
            assert (got == ref).all(), f"job {i} {shapes[i]}: differs from smr_rescale_bilinear"
            want = orc.rescale_bilinear(px[i], dw, dh, orc.PX_RGBA8_SRGB if ctx.srgb else orc.PX_RGBA8_UNORM)
            d = np.abs(got.astype(np.int32) - want.astype(np.int32))
            print(f"job {i} {shapes[i]}: max |diff| to the oracle {d.max()} LSB, {(d == 0).mean():.5f} of bytes identical")
            assert d.max() <= 1 and (d == 0).mean() >= 0.99, f"job {i} {shapes[i]}: {d.max()} LSB, {(d == 0).mean():.5f} identical"
    finally:
        for s in srcs + dsts + refs:
            s.destroy()


def test_k_image_nodes_writes_only_the_texels_of_a_window(ctx):
    """A destination that is a window inside a larger allocation, on a pitch that is no multiple of 16 (smr_surface_wrap asks for a 16-byte
    base and a 4-byte pitch): texel by texel, and not a byte of the surrounding allocation changes."""
    rng = np.random.default_rng(9)
    px = premultiplied(rng, 3, 2)
    parent_px = rng.integers(0, 256, (12, 128, 4), dtype=np.uint8)   # rows of 512 bytes: the pitch, so a download shows every byte
    src, parent, ref = ctx.surface_from(px), ctx.surface_from(parent_px), ctx.surface(67, 9)
    info = parent.info()
    assert info.pitch == 512
    base, pitch = 16, 324
    window = ctx.wrap(info.dptr + base, pitch, 67, 9)
    try:
        ctx._check(_image_nodes(ctx)(ctx.handle, (C.c_void_p * 1)(src.handle), (C.c_void_p * 1)(window.handle), 1))
        ctx.rescale_bilinear(src, ref)
        want = parent_px.reshape(-1).copy()
        rows = ref.download().reshape(9, 67 * 4)
        for y in range(9):
            want[base + y * pitch: base + y * pitch + 67 * 4] = rows[y]
        got = parent.download().reshape(-1)
        inside = want != parent_px.reshape(-1)
        assert (got[inside] == want[inside]).all()
        assert (got == want).all(), "a byte outside the window was written"
    finally:
        for s in (window, src, parent, ref):
            s.destroy()
