"""WebView nodes end to end on the GPU (include/smr.h "WebView nodes"; transformations/web_renderer/renderer.rs:78-134, shader.rs:53-114,
render_website.wgsl): a host-painted BGRA page and the node's children on the rectangles the page reported, drawn by ONE k_web_view launch
per node and 16 children.

The yardstick is tests/web_view_model.py: on integer rectangles the committed oracle (oracle.apply_layouts over the node's layer list), on
fractional ones (quarters, never .5) the f32 model that tests/test_emu_web_view.py holds to the oracle first.  The bar is the compositor's:
within 1 LSB per channel.  An RGBA output is a clone of the root node's texture (render_loop.rs:81-103), so a WebView as the root of an
output of the page's size shows the node's bytes themselves.

Through the renderer: nothing before a paint, the three embedding methods, a repaint, fewer rectangles than children, a stale and a fresh
input stream as children, the node inside a rescaler, two lanes, exclusivity across two outputs, the launch counts.  Through the internal
export smr_web_view: the emulator's shapes (tests/test_emu_web_view.py) and the write footprint on destinations in caller memory
(tests/wrapped.py).  Without the feature every test fails at registration."""
import ctypes as C

import numpy as np
import pytest

from smelter_amd import _ffi
from tests import web_view_model as wm
from tests import wrapped
from tests.test_emu_web_view import COUNTS, PAGES, case, lsb

pytestmark = pytest.mark.gpu

W, H = 67, 21   # the page of the renderer tests: a width that is no multiple of 4, two tile rows


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


@pytest.fixture(scope="module")
def material():
    """One page, a repaint, three child textures (two opaque images — premultiplication leaves their bytes — and a translucent BGRA frame
    whose node texture is its swizzle) and their rectangles, shared by the renderer tests and left unchanged."""
    rng = np.random.default_rng(11)
    page, page2 = wm.page_bitmap(rng, W, H), wm.page_bitmap(rng, W, H)
    img0, img2 = wm.premultiplied(rng, 17, 9, opaque=True), wm.premultiplied(rng, 5, 11, opaque=True)
    cam_bgra = wm.premultiplied(rng, 40, 30)
    rects = [(3.25, 1.75, 30.0, 12.5), (-4.25, 8.25, 40.0, 30.0), (50.25, 1.75, 20.25, 14.5)]
    return dict(page=page, page2=page2, img0=img0, img2=img2, cam_bgra=cam_bgra, cam=wm.swizzle(cam_bgra), rects=rects,
                int_rects=[(3.0, 2.0, 30.0, 12.0), (-4.0, 8.0, 40.0, 30.0), (50.0, 2.0, 20.0, 15.0)])


def web_scene(children=3, instance="page"):
    kids = [{"type": "image", "id": "c0", "image_id": "i0"}, {"type": "input_stream", "id": "c1", "input_id": "cam"},
            {"type": "image", "id": "c2", "image_id": "i2"}][:children]
    return {"type": "web_view", "id": "web", "instance_id": instance, "children": kids}


def make_renderer(ctx, material, embedding, lanes=()):
    from smelter_amd.renderer import Renderer
    r = Renderer(ctx, lanes=lanes)
    r.register_web_renderer("page", W, H, embedding)
    r.register_image("i0", material["img0"])
    r.register_image("i2", material["img2"])
    r.register_input("cam")
    return r


def render(r, hip, pts_s=1.0, cam=None, cam_pts_s=None, output="out"):
    frames = {"cam": cam} if cam is not None else {}
    out = r.render(pts_s, frames, {"cam": cam_pts_s} if cam_pts_s is not None else None)
    return np.array(out[output].download()[0])


def yardstick(material, children, rects, method, srgb, page="page"):
    """The oracle where every rectangle is on whole pixels, the f32 model otherwise (tests/web_view_model.py)."""
    whole = all(float(v) == int(v) for q in rects[:len(children)] for v in q)
    return (wm.oracle_node if whole else wm.model_node)(material[page], children, rects, method, srgb)


def test_before_a_paint_the_node_has_no_texture(ctx, hip, material):
    r = make_renderer(ctx, material, _ffi.WEB_NATIVE_OVER_CONTENT)
    try:
        r.update_scene("out", W, H, web_scene(), hip.FRAME_RGBA)
        r.web_positions("page", material["rects"])
        before = r.web_launches()
        assert not render(r, hip).any(), "a WebView root without a paint is not the empty output"
        # under a parent: the parent samples transparent — the bytes of the same view without the child
        box = {"type": "view", "background_color": "#20406080", "children": [web_scene()]}
        r.update_scene("out", W + 13, H + 7, box, hip.FRAME_RGBA)
        with_child = render(r, hip)
        r.update_scene("out", W + 13, H + 7, {**box, "children": []}, hip.FRAME_RGBA)
        assert (with_child == render(r, hip)).all()
        assert r.web_launches() == before
    finally:
        r.close()


@pytest.mark.parametrize("embedding", [_ffi.WEB_CHROMIUM_EMBEDDING, _ffi.WEB_NATIVE_OVER_CONTENT, _ffi.WEB_NATIVE_UNDER_CONTENT], ids=["chromium", "over", "under"])
@pytest.mark.parametrize("whole", [True, False], ids=["integer", "fractional"])
def test_three_methods_and_a_repaint(ctx, hip, material, embedding, whole):
    r = make_renderer(ctx, material, embedding)
    cam = ctx.frame(hip.FRAME_BGRA, 40, 30, [material["cam_bgra"]])
    rects = material["int_rects"] if whole else material["rects"]
    children = [material["img0"], material["cam"], material["img2"]]
    try:
        r.update_scene("out", W, H, web_scene(), hip.FRAME_RGBA)
        r.web_paint("page", material["page"])
        # before the first positions call: the page alone, byte for byte
        assert (render(r, hip, cam=cam) == wm.swizzle(material["page"])).all()
        r.web_positions("page", rects)
        before = r.web_launches()
        got = render(r, hip, cam=cam)
        assert r.web_launches() - before == 1
        d = lsb(got, yardstick(material, children, rects, embedding, ctx.srgb))
        print(f"method {embedding}, whole={whole}, srgb={ctx.srgb}: {d} LSB")
        assert d <= 1
        if embedding != _ffi.WEB_CHROMIUM_EMBEDDING:
            assert lsb(got, wm.swizzle(material["page"])) > 1, "the children left no trace"
        # a repaint replaces the page (here from a view with padded rows); rendering again without one keeps it
        padded = np.zeros((H, W + 5, 4), np.uint8)
        padded[:, :W] = material["page2"]
        r.web_paint("page", padded[:, :W])
        for _ in range(2):
            assert lsb(render(r, hip, cam=cam), yardstick(material, children, rects, embedding, ctx.srgb, page="page2")) <= 1
        # fewer rectangles than children: the children beyond them are not drawn; more: the extra ones are ignored
        r.web_positions("page", rects[:1])
        assert lsb(render(r, hip, cam=cam), yardstick(material, children[:1], rects[:1], embedding, ctx.srgb, page="page2")) <= 1
        r.web_positions("page", rects + [(0.0, 0.0, 5.0, 5.0)] * 3)
        assert lsb(render(r, hip, cam=cam), yardstick(material, children, rects, embedding, ctx.srgb, page="page2")) <= 1
    finally:
        r.close()
        cam.destroy()


def test_stale_and_fresh_input_stream_children(ctx, hip, material):
    r = make_renderer(ctx, material, _ffi.WEB_NATIVE_OVER_CONTENT)
    cam = ctx.frame(hip.FRAME_BGRA, 40, 30, [material["cam_bgra"]])
    rects, children = material["int_rects"], [material["img0"], material["cam"], material["img2"]]
    try:
        r.update_scene("out", W, H, web_scene(), hip.FRAME_RGBA)
        r.web_paint("page", material["page"])
        r.web_positions("page", rects)
        fresh = render(r, hip, pts_s=10.0, cam=cam, cam_pts_s=9.8)
        assert lsb(fresh, yardstick(material, children, rects, wm.OVER, ctx.srgb)) <= 1
        # 0.6 s old > the 0.5 s fallback timeout, and no frame at all: the child has no texture and draws nothing
        without = yardstick(material, [material["img0"], None, material["img2"]], rects, wm.OVER, ctx.srgb)
        assert lsb(without, yardstick(material, children, rects, wm.OVER, ctx.srgb)) > 1
        assert lsb(render(r, hip, pts_s=10.0, cam=cam, cam_pts_s=9.4), without) <= 1
        assert lsb(render(r, hip, pts_s=10.0), without) <= 1
    finally:
        r.close()
        cam.destroy()


def test_inside_a_rescaler(ctx, hip, material):
    """The parent samples the node's texture like any other child texture: the bytes of the same scene with the node's own texels registered
    as an image in its place (opaque throughout, so that registering them premultiplies nothing)."""
    rng = np.random.default_rng(5)
    page = wm.premultiplied(rng, W, H, opaque=True)
    r = make_renderer(ctx, material, _ffi.WEB_NATIVE_OVER_CONTENT)
    try:
        r.update_scene("out", W, H, web_scene(1), hip.FRAME_RGBA)
        r.web_paint("page", page)
        r.web_positions("page", material["int_rects"][:1])
        node = render(r, hip)
        assert lsb(node, wm.oracle_node(page, [material["img0"]], material["int_rects"][:1], wm.OVER, ctx.srgb)) <= 1 and (node[..., 3] == 255).all()
        r.register_image("node", node)
        box = lambda child: {"type": "view", "background_color": "#102030FF", "children": [{"type": "rescaler", "child": child}]}
        r.update_scene("out", 160, 90, box(web_scene(1)), hip.FRAME_RGBA)
        through_web = render(r, hip)
        r.update_scene("out", 160, 90, box({"type": "image", "image_id": "node"}), hip.FRAME_RGBA)
        through_image = render(r, hip)
        assert (through_web == through_image).all()
        assert len(np.unique(through_web.reshape(-1, 4), axis=0)) > 100, "the rescaled node left no trace"
    finally:
        r.close()


def test_two_lanes_keep_a_page_copy_each(ctx, hip, material):
    lane = hip.Context(0, mode=hip.MODE_GPU_OPTIMIZED if ctx.srgb else hip.MODE_CPU_OPTIMIZED)
    r = make_renderer(ctx, material, _ffi.WEB_NATIVE_UNDER_CONTENT, lanes=[lane])
    cam = ctx.frame(hip.FRAME_BGRA, 40, 30, [material["cam_bgra"]])
    rects, children = material["rects"], [material["img0"], material["cam"], material["img2"]]
    try:
        r.update_scene("out", W, H, web_scene(), hip.FRAME_RGBA)
        r.web_positions("page", rects)
        first = yardstick(material, children, rects, wm.UNDER, ctx.srgb)
        second = yardstick(material, children, rects, wm.UNDER, ctx.srgb, page="page2")
        assert lsb(first, second) > 1
        r.web_paint("page", material["page"])
        a, b = render(r, hip, cam=cam), render(r, hip, cam=cam)      # lane 0, lane 1
        assert lsb(a, first) <= 1 and (a == b).all()
        r.web_paint("page", material["page2"])
        c = render(r, hip, cam=cam)                                   # lane 0 has the new paint ...
        r.web_paint("page", material["page"])
        d, e = render(r, hip, cam=cam), render(r, hip, cam=cam)      # ... lane 1 skips it: the latest paint wins
        assert lsb(c, second) <= 1 and (d == a).all() and (e == a).all()
        before = r.web_launches()
        render(r, hip, cam=cam), render(r, hip, cam=cam)
        assert r.web_launches() - before == 2
    finally:
        r.close()
        cam.destroy()
        lane.close()


def test_exclusive_across_outputs_and_refused_unregistration(ctx, hip, material):
    from smelter_amd.scene import SceneError
    r = make_renderer(ctx, material, _ffi.WEB_NATIVE_OVER_CONTENT)
    try:
        r.update_scene("a", W, H, web_scene(0), hip.FRAME_RGBA)
        r.web_paint("page", material["page"])
        with pytest.raises(SceneError) as e:
            r.update_scene("b", W, H, {"type": "view", "children": [web_scene(0)]}, hip.FRAME_RGBA)
        assert str(e.value) == 'Instance of web renderer "page" was used more than once. Only one component can use specific web renderer at the time.'
        with pytest.raises(SceneError):
            r.unregister_web_renderer("page")
        out = r.render(1.0, {})
        assert list(out) == ["a"] and (np.array(out["a"].download()[0]) == wm.swizzle(material["page"])).all()
        r.update_scene("a", W, H, {"type": "view"}, hip.FRAME_RGBA)      # "a" lets go of it: "b" may have it, then nobody
        r.update_scene("b", W, H, web_scene(0), hip.FRAME_RGBA)
        assert (render(r, hip, output="b") == wm.swizzle(material["page"])).all()
        r.unregister_output("b")
        r.unregister_web_renderer("page")
        with pytest.raises(SceneError):
            r.update_scene("b", W, H, web_scene(0), hip.FRAME_RGBA)
    finally:
        r.close()


def test_seventeen_children_take_two_launches(ctx, hip, material):
    r = make_renderer(ctx, material, _ffi.WEB_NATIVE_UNDER_CONTENT)
    rng = np.random.default_rng(17)
    try:
        kids, children = [], []
        for k in range(17):
            w, h = wm.child_sizes(k)
            px = wm.premultiplied(rng, w, h, opaque=True)
            r.register_image(f"k{k}", px)
            children.append(px)
            kids.append({"type": "image", "id": f"k{k}", "image_id": f"k{k}"})
        rects = wm.integer_rects(W, H)[:17]
        r.update_scene("out", W, H, {"type": "web_view", "instance_id": "page", "children": kids}, hip.FRAME_RGBA)
        r.web_paint("page", material["page"])
        r.web_positions("page", rects)
        before = r.web_launches()
        got = render(r, hip)
        assert r.web_launches() - before == 2
        assert lsb(got, wm.oracle_node(material["page"], children, rects, wm.UNDER, ctx.srgb)) <= 1
        r.web_positions("page", rects[:16])
        before = r.web_launches()
        got = render(r, hip)
        assert r.web_launches() - before == 1
        assert lsb(got, wm.oracle_node(material["page"], children[:16], rects[:16], wm.UNDER, ctx.srgb)) <= 1
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------ the internal export
def _web_view(ctx):
    fn = ctx.lib.smr_web_view   # the internal export the renderer's WebView nodes call (not part of smr.h)
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(_ffi.WebRect), C.c_uint32, C.c_int]
    fn.restype = C.c_int
    return fn


def _call(ctx, fn, page_ptr, page_pitch, dst, srcs, rects, under):
    n = len(srcs)
    hs = (C.c_void_p * max(n, 1))(*[None if s is None else s.handle for s in srcs])
    rc = (_ffi.WebRect * max(n, 1))(*[_ffi.WebRect(*[float(v) for v in q]) for q in rects])
    ctx._check(fn(ctx.handle, C.c_void_p(page_ptr), page_pitch, dst.handle, hs, rc, n, 1 if under else 0))
    ctx.sync()


def test_export_meets_the_yardstick_on_the_emulators_shapes(ctx):
    fn = _web_view(ctx)
    worst = 0
    for Wp, Hp, *_ in PAGES:
        for n in COUNTS:
            for fractional in (False, True):
                if fractional and n == 0:
                    continue
                page, children, rects = case(Wp, Hp, n, fractional, seed=Wp + n)
                pg = ctx.surface_from(page)
                srcs = [None if c is None else ctx.surface_from(c) for c in children]
                dst = ctx.surface(Wp, Hp)
                dst.upload(np.full((Hp, Wp, 4), 77, np.uint8))  # stale contents must not show through
                try:
                    for method in (wm.OVER, wm.UNDER):
                        _call(ctx, fn, pg.info().dptr, pg.info().pitch, dst, srcs, rects, method == wm.UNDER)
                        want = (wm.model_node if fractional else wm.oracle_node)(page, children, rects, method, ctx.srgb)
                        d = lsb(dst.download(), want)
                        worst = max(worst, d)
                        assert d <= 1, f"{Wp}x{Hp}, {n} children, method {method}, fractional={fractional}, srgb={ctx.srgb}: {d} LSB"
                finally:
                    for s in [pg, dst] + [s for s in srcs if s is not None]:
                        s.destroy()
    print(f"srgb={ctx.srgb}: at most {worst} LSB from the yardstick")


@pytest.mark.parametrize("geometry", wrapped.GEOMETRIES)
def test_export_writes_the_texels_and_no_other_byte(ctx, geometry):
    """Destinations in caller memory (tests/wrapped.py): tight rows force the texel-by-texel stores, a window's neighbours are live data.
    The page sits in caller memory too, on rows that are no multiple of 16 bytes apart."""
    import torch
    fn = _web_view(ctx)
    for i, (Wp, Hp, n) in enumerate([(67, 21, 3), (130, 33, 17), (5, 3, 1), (64, 16, 0)]):
        page, children, rects = case(Wp, Hp, n, False, seed=Wp + n)
        src = wrapped.Dest(torch, Wp, Hp, 4, "slack" if i % 2 else "tight", seed=90 + i)
        host = src.before.copy()
        body = host[wrapped.HEAD:wrapped.HEAD + src.pitch * Hp].reshape(Hp, src.pitch)
        body[:, :Wp * 4] = page.reshape(Hp, Wp * 4)
        src.buf.copy_(torch.from_numpy(host))
        torch.cuda.synchronize()
        srcs = [None if c is None else ctx.surface_from(c) for c in children]
        ws = wrapped.WrappedSurface(torch, ctx, Wp, Hp, 0, geometry, seed=40 + i)
        try:
            for method in (wm.UNDER, wm.OVER):
                _call(ctx, fn, src.ptr, src.pitch, ws.surface, srcs, rects, method == wm.UNDER)
            got = ws.texels(f"smr_web_view {Wp}x{Hp}, {n} children")
            assert lsb(got, wm.oracle_node(page, children, rects, wm.OVER, ctx.srgb)) <= 1
        finally:
            ws.surface.destroy()
            for s in srcs:
                if s is not None:
                    s.destroy()


def test_export_refuses_what_it_cannot_draw(ctx, hip):
    fn = _web_view(ctx)
    dst, page = ctx.surface(16, 8), ctx.surface(16, 8)
    try:
        ptr, pitch = page.info().dptr, page.info().pitch
        with pytest.raises(hip.SmrError):
            _call(ctx, fn, ptr, 16 * 4 - 4, dst, [], [], False)          # rows closer than the texels need
        with pytest.raises(hip.SmrError):
            _call(ctx, fn, ptr + 2, pitch, dst, [], [], False)           # a page that is not dword aligned
        with pytest.raises(hip.SmrError):
            _call(ctx, fn, ptr, pitch, dst, [dst], [(0, 0, 4, 4)], False)  # the target as its own child
    finally:
        dst.destroy()
        page.destroy()
