"""Packed 4:2:2 output frames (SMR_FRAME_UYVY422 / SMR_FRAME_YUYV422 where a frame is an output, include/smr.h) on the device.

Every expected picture is tests/packed422_model.py's interleave: of the oracle's rgba_to_planar_yuv(px, YUV422) — byte for byte —, or of the
library's own FRAME_PLANAR_YUV422 output of the same call on the same context (that route is held to the oracle by the existing tests).

  1  smr_rgba_to_frame: k_rgba_to_packed422 at 2 x 1 ... 1026 x 2 — a ragged w % 4 == 2 group, either side of a 256-pixel workgroup edge —,
     opaque and translucent nodes, SMR_CONVERT_GENERAL, a node whose rows are dword- but not 16-byte aligned;
  2  smr_render_layouts: the fused store (k_compose_output<3 | 4>) on the compositor zoo's lists, in both rendering modes; the route is
     proven by the profile (no output-conversion launch, one k_compose_output), the unfused routes (odd height, under-aligned plane,
     SMR_OPT_FUSED_KERNELS = 0) by one output-conversion launch and the same bytes; SMR_OPT_DIRECT_OUTPUT declines packed outputs;
  3  the pixel pairs whose chroma lies nearest a code boundary through copy tiles: the repair branch, against the oracle;
  4  black; 5  the write footprint in caller memory; 6  the renderer (lanes, a shard, the other root paths); 7  the refusals.

(smr_surface_wrap takes 16-byte aligned bases only, so "under-aligned" is always a pitch: 4 mod 8 for a plane, 4 mod 16 for a node.)"""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import compose_zoo as zoo
from tests import packed422_model as pk
from tests import refpipe, scenes
from tests.wrapped import GEOMETRIES, WrappedFrame

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from smelter_amd import hip as h
    orc.build()
    return h


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


@pytest.fixture(scope="module")
def ctxs(hip):
    """srgb -> context: True SMR_MODE_GPU_OPTIMIZED, False SMR_MODE_CPU_OPTIMIZED"""
    out = {True: hip.Context(0), False: hip.Context(0, mode=hip.MODE_CPU_OPTIMIZED)}
    yield out
    for c in out.values():
        c.close()


@pytest.fixture(scope="module")
def ctx(ctxs):
    return ctxs[True]


def _rgba(seed, w, h, opaque):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    if opaque:
        a[..., 3] = 255
    else:  # premultiplied, as a node texture is
        a[..., :3] = (a[..., :3].astype(np.uint16) * a[..., 3:4] // 255).astype(np.uint8)
    return a


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got, want), f"{what}: {int((got != want).sum())} of {got.size} bytes differ, first at {np.argwhere(got != want)[:5].tolist()}"


def _profiled(c, call):
    """-> (launches of the output-conversion stage, k_compose_output launches, every kernel-counter delta summed) of call()"""
    before = c.kernel_launches()
    c.profile_reset()
    c.profile_enable(True)
    try:
        call()
        c.sync()
        prof = c.profile_read()
    finally:
        c.profile_enable(False)
    after = c.kernel_launches()
    return prof["output"][1], after["compose_output"] - before["compose_output"], sum(after[k] - before[k] for k in after), prof


# ------------------------------------------------------------------------------------------------------------------ 1. smr_rgba_to_frame
RGBA_SIZES = [(2, 1), (2, 2), (4, 3), (6, 3), (10, 5), (254, 3), (258, 9), (1026, 2)]


@pytest.mark.parametrize("w,h", RGBA_SIZES)
def test_rgba_to_frame_is_the_interleaved_planar_422_of_the_oracle(ctx, hip, torch, w, h):
    for opaque in (True, False):
        px = _rgba(w * 7 + h + opaque, w, h, opaque)
        node = ctx.surface_from(px)
        # the same bytes in caller memory on rows that are dword- but not 16-byte aligned: the kernel's 4-byte loads
        pitch = w * 4 + 4 if (w * 4 + 4) % 16 else w * 4 + 8
        host = np.zeros((h, pitch), np.uint8)
        host[:, :w * 4] = px.reshape(h, w * 4)
        buf = torch.from_numpy(host).cuda()
        loose = ctx.wrap(buf.data_ptr(), pitch, w, h)
        planar = ctx.rgba_to_frame(node, hip.FRAME_PLANAR_YUV422)
        own = planar.download()
        for order in pk.ORDERS:
            fmt, what = pk.frame_format(hip, order), f"{pk.NAMES[order]} {w}x{h} opaque {opaque}"
            want = pk.expected(orc, px, order)
            launches, _, _, _ = _profiled(ctx, lambda: ctx.rgba_to_frame(node, fmt).destroy())
            assert launches == 1, (what, launches)
            _same(ctx.rgba_to_frame(node, fmt).download()[0], want, what)
            _same(pk.interleave(*own, order), want, what + " (the library's planar 4:2:2 output)")
            _same(ctx.rgba_to_frame(loose, fmt).download()[0], want, what + f" (node pitch {pitch})")
            ctx.set_convert_impl(hip.CONVERT_GENERAL)
            try:
                launches, _, _, _ = _profiled(ctx, lambda: ctx.rgba_to_frame(node, fmt).destroy())
                assert launches == 1, (what, "SMR_CONVERT_GENERAL", launches)
                _same(ctx.rgba_to_frame(node, fmt).download()[0], want, what + " (SMR_CONVERT_GENERAL)")
            finally:
                ctx.set_convert_impl(hip.CONVERT_AUTO)
        planar.destroy(); loose.destroy(); node.destroy()
        del buf


# ------------------------------------------------------------------------------------------------------------------ 2. the fused route
FUSED_SIZES = [(2, 2), (130, 34), (258, 50), (642, 50), (1026, 18)]
LISTS = ("grid", "zoo3", "zoo7", "zoo11")


def _list(which, W, H, srgb):
    """(layouts, sources as host arrays | None, opaque flags): tests/compose_zoo.py's grid scene / zoo list `seed` with whole-texel crops
    (nothing is resampled: the compositor and its store alone)"""
    if which == "grid":
        layouts, sources, kinds = zoo.grid_scene(W, H, 2, 2, 0, srgb=srgb)
        return layouts, sources, [k == 2 for k in kinds]
    rng = np.random.default_rng(100 + int(which[3:]))
    sources = [zoo.video(96, 54, 7, alpha=True), zoo.video(64, 40, 8), None]
    layouts = zoo.zoo(max(W, 130), max(H, 34), rng, int(rng.integers(3, 14)), len(sources), srgb)  # (boxes of at least 8 x 6: the 2 x 2 output takes the 130 x 34 list)
    zoo.direct_crops(layouts)
    return layouts, sources, [False, True, False]


def _device_sources(c, sources, opaque):
    out = []
    for s, o in zip(sources, opaque):
        if s is None:
            out.append(None)
        else:
            t = c.surface_from(s)
            t.opaque = o
            out.append(t)
    return out


def _render(c, fmt, layouts, srcs, W, H, frame=None, poison=0x5A):
    out = frame or c.frame(fmt, W, H)
    if frame is None:
        out.upload([np.full(s, poison, np.uint8) for s in out.plane_shapes()])
    stats = _profiled(c, lambda: c.render_layouts(layouts, srcs, W, H, out=out))
    got = out.download() if frame is None else None
    if frame is None:
        out.destroy()
    return got, stats


@pytest.mark.parametrize("srgb", [True, False], ids=["gpu_optimized", "cpu_optimized"])
@pytest.mark.parametrize("W,H", FUSED_SIZES)
@pytest.mark.parametrize("which", LISTS)
def test_render_layouts_stores_the_packed_frame_from_the_compositor(ctxs, hip, which, W, H, srgb):
    c = ctxs[srgb]
    layouts, sources, opaque = _list(which, W, H, srgb)
    srcs = _device_sources(c, sources, opaque)
    planar, _ = _render(c, hip.FRAME_PLANAR_YUV422, layouts, srcs, W, H)
    for order in pk.ORDERS:
        what = f"{which} {W}x{H} {pk.NAMES[order]} srgb {srgb}"
        got, (conversions, composes, _, prof) = _render(c, pk.frame_format(hip, order), layouts, srcs, W, H, poison=0x5A + order)
        assert conversions == 0 and composes == 1 and prof["layouts"][1] == 0, f"{what}: not the fused store: {prof}"
        _same(got[0], pk.interleave(*planar, order), what + " against the same context's planar 4:2:2 output")
    if which == "grid":  # opaque sources, nothing resampled: the oracle's composited picture, the compositor's stated 1 LSB
        rgba = orc.apply_layouts(W, H, layouts, sources, srgb=srgb)
        for order in pk.ORDERS:
            got, _ = _render(c, pk.frame_format(hip, order), layouts, srcs, W, H)
            want = pk.expected(orc, rgba, order)
            print(f"grid {W}x{H} {pk.NAMES[order]} srgb {srgb}: max |diff| {refpipe.max_diff(got[0], want)}, exact {refpipe.exact_fraction(got[0], want):.5f}")
            assert refpipe.max_diff(got[0], want) <= 1
    for s in srcs:
        if s is not None:
            s.destroy()


@pytest.mark.parametrize("srgb", [True, False], ids=["gpu_optimized", "cpu_optimized"])
def test_what_the_fused_store_declines_is_converted_in_one_more_launch_to_the_same_bytes(ctxs, hip, torch, srgb):
    """An odd height, a wrapped plane whose rows are 4 mod 8 bytes apart, SMR_OPT_FUSED_KERNELS = 0: composed into RGBA8, then
    k_rgba_to_packed422 — one launch of the output-conversion stage."""
    c = ctxs[srgb]
    for which in ("grid", "zoo7"):
        for W, H, how in ((130, 33, "odd height"), (130, 34, "pitch"), (130, 34, "unfused")):
            layouts, sources, opaque = _list(which, W, H, srgb)
            srcs = _device_sources(c, sources, opaque)
            planar, _ = _render(c, hip.FRAME_PLANAR_YUV422, layouts, srcs, W, H)
            for order in pk.ORDERS:
                fmt, what = pk.frame_format(hip, order), f"{which} {W}x{H} {how} {pk.NAMES[order]} srgb {srgb}"
                if how == "pitch":
                    wf = WrappedFrame(torch, c, fmt, W, H, "tight", 5 + order)
                    assert wf.dests[0].pitch % 8 == 4
                    _, (conversions, composes, _, prof) = _render(c, fmt, layouts, srcs, W, H, frame=wf.frame)
                    got = [wf.planes(what)[0]]
                    for s in wf.frame.surfaces:
                        s.destroy()
                else:
                    if how == "unfused":
                        c.set_fused_kernels(False)
                    try:
                        got, (conversions, composes, _, prof) = _render(c, fmt, layouts, srcs, W, H)
                    finally:
                        c.set_fused_kernels(True)
                # (an odd height does not fit wave B at all: the general compositor; an under-aligned plane keeps wave B, on an RGBA8 target)
                assert conversions == 1 and composes == (1 if how == "pitch" else 0), f"{what}: {prof}"
                _same(got[0], pk.interleave(*planar, order), what)
            for s in srcs:
                if s is not None:
                    s.destroy()


def test_direct_output_declines_packed_frames(hip):
    """SMR_OPT_DIRECT_OUTPUT with a scene at rest: from the second frame on a 4:2:0 output's copy tiles are written by the resampler; a packed
    output keeps them in the compositor — the same bytes frame after frame, k_ingest_wave's direct build never launched."""
    iw, ih, W, H = 320, 180, 640, 360
    layouts, res = scenes.cfg2_scene(iw, ih, W, H, 4)
    c_on, c_off = hip.Context(0), hip.Context(0)
    try:
        c_on.set_direct_output(True)

        def sources(c):
            out = []
            for k, r in enumerate(res):
                if r == (iw, ih):
                    out.append(c.frame(hip.FRAME_PLANAR_YUV420, iw, ih, list(scenes.test_input(k, iw, ih, noise_seed=40 + k))))
                else:
                    out.append(c.surface_from(_rgba(k, r[0], r[1], False)))
            return out
        s_on, s_off = sources(c_on), sources(c_off)
        for order in pk.ORDERS:
            fmt = pk.frame_format(hip, order)
            ref, _ = _render(c_off, fmt, layouts, s_off, W, H)
            planar, _ = _render(c_off, hip.FRAME_PLANAR_YUV422, layouts, s_off, W, H)
            _same(ref[0], pk.interleave(*planar, order), f"{pk.NAMES[order]} cfg2")
            before = c_on.kernel_launches()["ingest_wave_direct"]
            for i in range(3):
                got, (conversions, composes, _, prof) = _render(c_on, fmt, layouts, s_on, W, H, poison=0x31 + i)
                assert conversions == 0 and composes == 1, prof
                _same(got[0], ref[0], f"{pk.NAMES[order]} frame {i} with direct output on")
            assert c_on.kernel_launches()["ingest_wave_direct"] == before
    finally:
        c_on.close()
        c_off.close()


# ------------------------------------------------------------------------------------------------------------------ 3. boundary content
def test_pairs_on_code_boundaries_convert_like_the_reference_sequence(ctx, hip):
    W, H = 512, 2
    px = pk.near_boundary_picture(W, H)
    src = ctx.surface_from(px)
    src.opaque = True
    layouts = [zoo.tex(0, 0.0, 0.0, float(W), float(H))]
    for order in pk.ORDERS:
        got, (conversions, composes, _, prof) = _render(ctx, pk.frame_format(hip, order), layouts, [src], W, H)
        assert conversions == 0 and composes == 1, prof
        _same(got[0], pk.expected(orc, px, order), f"{pk.NAMES[order]} near-boundary pairs through copy tiles")
        _same(ctx.rgba_to_frame(src, pk.frame_format(hip, order)).download()[0], pk.expected(orc, px, order), f"{pk.NAMES[order]} near-boundary pairs, smr_rgba_to_frame")
    src.destroy()


# ------------------------------------------------------------------------------------------------------------------ 4. black
@pytest.mark.parametrize("w,h", [(2, 1), (66, 5)])
def test_black_is_y16_u128_v128_in_the_frames_order(ctx, hip, w, h):
    from smelter_amd.renderer import Renderer
    for order in pk.ORDERS:
        fmt = pk.frame_format(hip, order)
        f = ctx.frame(fmt, w, h)
        f.upload([np.full(s, 0x5A, np.uint8) for s in f.plane_shapes()])
        ctx.fill_black(f)
        _same(f.download()[0], pk.black(w, h, order), f"fill_black {pk.NAMES[order]} {w}x{h}")
        f.destroy()
        r = Renderer(ctx)
        try:
            r.register_input("nobody")
            r.update_scene("out", w, h, {"type": "input_stream", "input_id": "nobody"}, output_format=fmt)
            _same(r.render(0.0, {})["out"].download()[0], pk.black(w, h, order), f"empty output {pk.NAMES[order]} {w}x{h}")
        finally:
            r.close()


# ------------------------------------------------------------------------------------------------------------------ 5. write footprint
@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_a_packed_plane_in_caller_memory_gets_its_w_times_2_bytes_per_row_and_no_other(ctx, hip, torch, geometry):
    for W, H in ((130, 34), (256, 32), (6, 2)):
        layouts, sources, opaque = _list("grid", W, H, True)
        srcs = _device_sources(ctx, sources, opaque)
        node = ctx.surface_from(_rgba(W + H, W, H, False))
        for order in pk.ORDERS:
            fmt = pk.frame_format(hip, order)
            want_render, _ = _render(ctx, fmt, layouts, srcs, W, H)
            want_convert = ctx.rgba_to_frame(node, fmt).download()
            for how in ("fused", "unfused", "rgba_to_frame", "fill_black"):
                what = f"{how} {pk.NAMES[order]} {W}x{H}"
                wf = WrappedFrame(torch, ctx, fmt, W, H, geometry, 11 + order, align=16 if how == "fused" else 4)
                if how == "unfused":
                    ctx.set_fused_kernels(False)
                try:
                    if how in ("fused", "unfused"):
                        ctx.render_layouts(layouts, srcs, W, H, out=wf.frame)
                    elif how == "rgba_to_frame":
                        ctx.rgba_to_frame(node, fmt, wf.frame)
                    else:
                        ctx.fill_black(wf.frame)
                finally:
                    ctx.set_fused_kernels(True)
                ctx.sync()
                got = wf.planes(what)[0]  # (asserts that no byte outside the texels changed)
                _same(got, want_render[0] if how in ("fused", "unfused") else want_convert[0] if how == "rgba_to_frame" else pk.black(W, H, order), what)
                for s in wf.frame.surfaces:
                    s.destroy()
        node.destroy()
        for s in srcs:
            if s is not None:
                s.destroy()


# ------------------------------------------------------------------------------------------------------------------ 6. the renderer
def _scene(W, H, wide, transition_ms=None):
    a = {"type": "rescaler", "id": "a", "top": 2, "left": 2, "width": wide, "height": H - 4, "child": {"type": "input_stream", "input_id": "in0"}}
    b = {"type": "rescaler", "id": "b", "top": 4, "left": W - 30, "width": 28, "height": H // 2, "child": {"type": "input_stream", "input_id": "in1"}}
    if transition_ms:
        a["transition"] = {"duration_ms": transition_ms}
    label = {"type": "view", "top": H - 14, "left": 6, "width": 40, "height": 10, "background_color": "#00000096"}
    return {"type": "view", "background_color": "#203040FF", "children": [a, b, label]}


def _five_frames(hip, r, W, H, frames_for):
    """Two outputs of one scene, packed and planar 4:2:2: at rest, then five frames of a transition -> every packed frame is its twin interleaved."""
    for order in pk.ORDERS:
        r.update_scene("pk", W, H, _scene(W, H, W // 2), output_format=pk.frame_format(hip, order))
        r.update_scene("pl", W, H, _scene(W, H, W // 2), output_format=hip.FRAME_PLANAR_YUV422)
        frames = frames_for()
        pts = 10.0 * order
        for step in range(7):
            if step == 2:
                for o, fmt in (("pk", pk.frame_format(hip, order)), ("pl", hip.FRAME_PLANAR_YUV422)):
                    r.update_scene(o, W, H, _scene(W, H, W // 2 + 20, 100), output_format=fmt)
            t = pts + step * 0.02
            outs = r.render(t, frames, {k: t for k in frames})
            got, planar = outs["pk"].download(), outs["pl"].download()
            _same(got[0], pk.interleave(*planar, order), f"{W}x{H} {pk.NAMES[order]} frame {step}")
            if step == 0:
                first = got[0]
        assert not np.array_equal(first, got[0]), "the transition moved nothing"


@pytest.mark.parametrize("W,H", [(64, 36), (130, 34)])
@pytest.mark.parametrize("how", ["plain", "two_lanes", "a_shard"])
def test_a_renderer_output_is_the_planar_422_output_interleaved(hip, W, H, how):
    from smelter_amd.renderer import Renderer
    root = hip.Context(0)
    extra = [hip.Context(0)] if how != "plain" else []
    r = Renderer(root, lanes=extra if how == "two_lanes" else (), shards=extra if how == "a_shard" else ())
    try:
        for k in range(2):
            r.register_input(f"in{k}")
        frames_for = lambda: {f"in{k}": (r.input_context(f"in{k}") if how == "a_shard" else root).frame(
            hip.FRAME_PLANAR_YUV420, 96, 54, list(scenes.test_input(k, 96, 54, noise_seed=60 + k))) for k in range(2)}
        _five_frames(hip, r, W, H, frames_for)
        r.sync()
    finally:
        r.close()
        for c in extra:
            c.close()
        root.close()


def test_the_other_root_paths_of_a_renderer_output(ctx, hip):
    """A root input_stream of another size (rescale, then smr_rgba_to_frame), a root Image, an unregistered input (black)."""
    from smelter_amd.renderer import Renderer
    W, H = 64, 36
    r = Renderer(ctx)
    try:
        r.register_input("in0")
        r.register_image("logo", _rgba(3, 40, 20, False))
        frames = {"in0": ctx.frame(hip.FRAME_PLANAR_YUV420, 96, 54, list(scenes.test_input(0, 96, 54, noise_seed=9)))}
        for name, scene, fs in (("input of another size", {"type": "input_stream", "input_id": "in0"}, frames),
                                ("image", {"type": "image", "image_id": "logo"}, {})):
            for order in pk.ORDERS:
                r.update_scene("pk", W, H, scene, output_format=pk.frame_format(hip, order))
                r.update_scene("pl", W, H, scene, output_format=hip.FRAME_PLANAR_YUV422)
                outs = r.render(0.0, fs, {k: 0.0 for k in fs})
                got, planar = outs["pk"].download(), outs["pl"].download()
                assert len(np.unique(planar[0])) > 4, f"{name}: an empty picture proves nothing"
                _same(got[0], pk.interleave(*planar, order), f"{name} {pk.NAMES[order]}")
        for order in pk.ORDERS:
            r.update_scene("pk", W, H, {"type": "input_stream", "input_id": "in0"}, output_format=pk.frame_format(hip, order))
            _same(r.render(1.0, {})["pk"].download()[0], pk.black(W, H, order), f"no frame for the root input, {pk.NAMES[order]}")
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------------------------ 7. refusals
def _hand_made_frame(ctx, hip, fmt, w, h, surfaces):
    from smelter_amd import _ffi
    f = hip.DeviceFrame.__new__(hip.DeviceFrame)
    f.ctx, f.fmt, f.w, f.h = ctx, fmt, w, h
    f.c = _ffi.Frame()
    f.c.format, f.c.width, f.c.height = fmt, w, h
    for i, s in enumerate(surfaces):
        f.c.planes[i] = s.handle.value
    return f


def test_odd_widths_wrong_planes_and_tagged_formats_are_refused_before_anything_is_launched(ctx, hip):
    from smelter_amd.renderer import Renderer
    from smelter_amd.scene import SceneError
    w, h = 17, 4
    node, plane = ctx.surface(w, h), ctx.surface(w // 2, h)
    wide = ctx.surface(16, h)  # w texels instead of w / 2 for a 16-wide frame
    node16 = ctx.surface(16, h)

    def refusals():
        for order in pk.ORDERS:
            fmt = pk.frame_format(hip, order)
            odd = _hand_made_frame(ctx, hip, fmt, w, h, [plane])
            for call in (lambda: ctx.rgba_to_frame(node, fmt, odd), lambda: ctx.fill_black(odd),
                         lambda: ctx.render_layouts([zoo.tex(0, 0.0, 0.0, 8.0, 4.0)], [node], w, h, out=odd)):
                with pytest.raises(hip.SmrError) as e:
                    call()
                assert e.value.code == -1 and "even width" in str(e.value), str(e.value)
            for bad, word in ((_hand_made_frame(ctx, hip, fmt, 16, h, [wide]), "plane 0"), (_hand_made_frame(ctx, hip, fmt, 16, h, []), "plane 0"),
                              (_hand_made_frame(ctx, hip, hip.frame_format(fmt, hip.MATRIX_BT601), 16, h, [ctx_plane16]), "colour matrix")):
                for call in (lambda: ctx.rgba_to_frame(node16, bad.fmt, bad), lambda: ctx.fill_black(bad)):
                    with pytest.raises(hip.SmrError) as e:
                        call()
                    assert e.value.code == -1 and word in str(e.value), str(e.value)

    ctx_plane16 = ctx.surface(8, h)
    conversions, composes, launched, prof = _profiled(ctx, refusals)
    assert launched == 0 and all(n == 0 for _, n in prof.values()), prof
    r = Renderer(ctx)
    try:
        for order in pk.ORDERS:
            fmt = pk.frame_format(hip, order)
            r.update_scene("out", 64, 36, {"type": "view", "background_color": "#FF0000FF"}, output_format=fmt)
            first = r.render(0.0, {})["out"].download()
            for bad_w, bad_fmt, word in ((63, fmt, "even width"), (64, hip.frame_format(fmt, hip.MATRIX_BT601), "colour matrix"), (64, hip.FRAME_V210, "input only")):
                with pytest.raises(SceneError) as e:
                    r.update_scene("out", bad_w, 36, {"type": "view", "background_color": "#00FF00FF"}, output_format=bad_fmt)
                assert word in str(e.value), str(e.value)
            again = r.render(0.02, {})["out"].download()  # the previous scene stays active
            _same(again[0], first[0], f"{pk.NAMES[order]}: the scene after refused updates")
            assert len(np.unique(first[0])) > 1
    finally:
        r.close()
    for s in (node, plane, wide, node16, ctx_plane16):
        s.destroy()
