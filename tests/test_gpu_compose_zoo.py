"""The fused compositor (k_classify_tiles + k_compose_output, smelter_amd/csrc/smr_fused_compose.h, driven by smr_render_layouts) on the
device, on the lists tests/test_emu_compose.py runs through the lane emulator (tests/compose_zoo.py: same generators, same seeds): rotations,
four radii, thin and thick borders, shadows, parent masks, translucent colours, textures with alpha at fractional crops, missing and
out-of-range sources, boxes that leave the frame, lists beyond the LDS copy by layouts and by masks — on RGBA8, planar 4:2:0 and NV12 outputs,
at the output sizes where the device code takes another path.  Every call goes through Context.render_layouts.

Bars (BASELINE.json's north star; the floors of test_gpu_parity.py::test_apply_layouts_zoo and test_gpu_fused.py::_oracle_floor): every byte
within 1 LSB of the oracle; >= 0.999 of the RGBA bytes of the pure-compositor groups identical, >= 0.995 of every Y'CbCr plane and of the
group with resampled children.  The fused kernels against the pass-per-launch kernels on the same device: no tolerance at all.
Every fused render is checked to have run k_compose_output once and the general compositor not at all.

Measured on an MI355X (gfx950), all 53 cases of this module, 262 planes compared with the oracle:
  pure compositor (CpuOptimized zoo, GpuOptimized zoo on whole-texel crops, the long lists, max_layouts, predicted / measured grid): share of
    identical bytes 1.00000 and max diff 0 on every plane of every output — the device agrees with the oracle (and so with the lane emulator)
    byte for byte;
  scaled children: Y, U, V and UV planes 1.00000; RGBA 1.00000 on four lists and 0.99998 on list 1 (258 x 50): one alpha byte of 51600 off by 1,
    behind the general resampler's tile;
  fused against pass-per-launch kernels on the same device: 0 differing bytes in every case, RGBA8, Y, U, V and NV12's UV alike.
A share below these on a later run is a drift worth reading, even where the floors still hold."""
import functools

import numpy as np
import pytest

from oracle import oracle as orc
from tests import compose_zoo as zoo
from tests import refpipe

pytestmark = pytest.mark.gpu

TOL = 1            # LSB, every byte (BASELINE.json north star)
FLOOR_RGBA = 0.999  # share of identical bytes, RGBA8 of the pure compositor (test_gpu_parity.py::test_apply_layouts_zoo)
FLOOR_YUV = 0.995   # ... of a Y'CbCr plane, and of everything behind a resampler (test_gpu_fused.py::_oracle_floor)
OUTS = ("rgba", "planar", "nv12")
# the smallest outputs at which the device code differs: baseline; width 2 mod 4 and a partial last tile row; a two-pixel last column block;
# 6 x 4 = 24 tiles (two k_classify_tiles workgroups of 16, the last partial); 9 x 2 tiles, the last two pixels wide
SIZES = [(256, 64), (258, 50), (130, 34), (642, 50), (1026, 18)]
FRAME_W, FRAME_H = 136, 20  # the 4:2:0 frame drawn 1:1 at the origin: it covers tile (0, 0) of 128 x 16 whole


@pytest.fixture(scope="module")
def hip():
    from smelter_amd import hip as h
    orc.build()
    return h


@pytest.fixture(scope="module")
def ctxs(hip):
    """(mode, fused) -> context."""
    out = {}
    for mode, m in (("cpu", hip.MODE_CPU_OPTIMIZED), ("gpu", hip.MODE_GPU_OPTIMIZED)):
        for fused in (True, False):
            c = hip.Context(0, mode=m)
            c.set_fused_kernels(fused)
            out[mode, fused] = c
    yield out
    for c in out.values():
        c.close()


# ------------------------------------------------------------------------------------------------------------------ lists and sources
class Case:
    """A layout list, its sources as host arrays (RGBA8 node, (y, u, v) planes of a 4:2:0 frame, or None) and which surfaces are opaque."""

    def __init__(self, what, W, H, layouts, sources, opaque, srgb):
        self.what, self.W, self.H, self.layouts, self.sources, self.opaque, self.srgb = what, W, H, layouts, sources, opaque, srgb

    @functools.cached_property
    def nodes(self):
        """The sources as the RGBA8 node textures the compositor reads (a frame: the exact converter's = the oracle's)."""
        return [orc.planar_yuv_to_rgba(*s, s[0].shape[1], s[0].shape[0]) if isinstance(s, tuple) else s for s in self.sources]


def _sources():
    a, o = zoo.video(96, 54, 7, alpha=True), zoo.video(64, 40, 8)   # (the emulator zoo's own two: premultiplied with alpha; opaque)
    assert (o[..., 3] == 255).all()
    return [a, o, None], [False, True, False]


def _with_frame(layouts, sources, opaque, on_top, seed):
    """Adds a 4:2:0 frame drawn 1:1 at the origin, under the list or over it; index 3 of the zoo (out of range) stays out of range."""
    for L in layouts:
        if L.type == 0 and L.source_index >= len(sources):
            L.source_index += 1
    L = zoo.tex(len(sources), 0.0, 0.0, float(FRAME_W), float(FRAME_H))
    return (layouts + [L]) if on_top else ([L] + layouts), sources + [zoo.frame_planes(FRAME_W, FRAME_H, seed)], opaque + [False]


@functools.lru_cache(maxsize=None)
def zoo_case(seed, mode, direct, n=None, size=None, frame=None):
    """List `seed` of the zoo: 3 to 14 layouts (or `n`) on SIZES[seed % 5]; `direct`: texture crops no resampler touches; `frame`: a 4:2:0
    frame "under" or "over" the list (by default: under, over or none by seed % 3)."""
    rng = np.random.default_rng(100 + seed)
    W, H = size or SIZES[seed % len(SIZES)]
    srgb = mode == "gpu"
    sources, opaque = _sources()
    layouts = zoo.zoo(W, H, rng, n or int(rng.integers(3, 14)), len(sources), srgb)
    if direct:
        zoo.direct_crops(layouts)
    frame = frame or (None, "under", "over")[seed % 3]
    if frame:
        layouts, sources, opaque = _with_frame(layouts, sources, opaque, frame == "over", seed)
    return Case(("zoo", seed, (W, H), mode), W, H, layouts, sources, opaque, srgb)


def _plan_kinds(case):
    """The resampling plan's kind (0: none) of every texture layout with a source behind it, as GpuOptimized decides it (layout.rs:238-278)."""
    kinds = []
    for L in case.layouts:
        if L.type == 0 and L.source_index < len(case.nodes) and case.nodes[L.source_index] is not None:
            node = case.nodes[L.source_index]
            dw, dh = max(refpipe._rust_round(L.width), 1), max(refpipe._rust_round(L.height), 1)
            kinds.append(orc.resample_plan(node.shape[1], node.shape[0], L.crop, dw, dh).kind)
            assert orc.resample(node, L.crop, dw, dh)[0] == kinds[-1]
    return kinds


def _assert_no_resampler(case):
    """The pure-compositor groups must not turn into resampler tests."""
    assert all(k == 0 for k in _plan_kinds(case)), (case.what, _plan_kinds(case))


def oracle_rgba(case, pure):
    if pure:
        return orc.apply_layouts(case.W, case.H, case.layouts, case.nodes, srgb=case.srgb)
    return refpipe.layout_node_render(case.layouts, case.nodes, case.W, case.H, srgb=case.srgb)


def planes_of(rgba, out):
    if out == "rgba":
        return [np.asarray(rgba)]
    if out == "nv12":
        return [np.asarray(p) for p in orc.rgba_to_nv12(rgba)]
    return [np.asarray(p) for p in orc.rgba_to_planar_yuv(rgba, orc.YUV420)]


# ------------------------------------------------------------------------------------------------------------------ rendering
def device_sources(c, hip, case):
    out = []
    for s, opaque in zip(case.sources, case.opaque):
        if s is None:
            out.append(None)
        elif isinstance(s, tuple):
            out.append(c.frame(hip.FRAME_PLANAR_YUV420, s[0].shape[1], s[0].shape[0], list(s)))
        else:
            t = c.surface_from(s)
            t.opaque = opaque   # -> SMR_SOURCE_OPAQUE_SURFACE (Context.render_layouts)
            out.append(t)
    return out


def render(c, hip, case, out, srcs=None, fused=True, poison=0x5A, layouts=None):
    """One smr_render_layouts call onto a poisoned output; a fused context must have run k_compose_output once and no general compositor."""
    srcs = srcs if srcs is not None else device_sources(c, hip, case)
    layouts = case.layouts if layouts is None else layouts
    W, H = case.W, case.H
    if out == "rgba":
        target = c.surface(W, H)
        target.upload(np.full((H, W, 4), poison, np.uint8))
        kw = {"out_rgba": target}
    else:
        target = c.frame(hip.FRAME_NV12 if out == "nv12" else hip.FRAME_PLANAR_YUV420, W, H)
        target.upload([np.full(s, poison, np.uint8) for s in target.plane_shapes()])
        kw = {"out": target}
    if fused:
        c.profile_reset()
        c.profile_enable(True)
    c.render_layouts(layouts, srcs, W, H, **kw)
    if fused:
        c.sync()
        prof = c.profile_read()
        c.profile_enable(False)
        assert prof["fused_compose_output"][1] == 1 and prof["layouts"][1] == 0, f"{case.what} {out}: left the fused compositor: {prof}"
    got = target.download()
    got = [got] if out == "rgba" else list(got)
    target.destroy()
    return got


def describe(g, w):
    d = np.abs(g.astype(np.int16) - w.astype(np.int16))
    return f"max diff {int(d.max())}, {float((d == 0).mean()):.5f} identical, {int((d != 0).sum())} of {d.size} bytes differ, first at {np.argwhere(d != 0)[:5].tolist()}"


def check_oracle(got, want, case, out, floor_rgba=FLOOR_RGBA):
    """<= 1 LSB on every byte, and the floor of identical bytes, per plane; -> the smallest share of identical bytes."""
    shares = []
    for k, (g, w) in enumerate(zip(got, want)):
        w = np.asarray(w).reshape(g.shape)
        floor = floor_rgba if out == "rgba" else FLOOR_YUV
        what = f"{case.what} {out} plane {k}: {describe(g, w)}"
        print(what)
        assert refpipe.max_diff(g, w) <= TOL, what
        assert refpipe.exact_fraction(g, w) >= floor, f"{what} (< {floor})"
        shares.append(refpipe.exact_fraction(g, w))
    return min(shares)


def check_same(got, ref, case, out, what="fused and pass-per-launch kernels differ on the same device"):
    for k, (g, r) in enumerate(zip(got, ref)):
        assert np.array_equal(g, r), f"{case.what} {out} plane {k}: {what}: {describe(g, r)}"


def run_case(ctxs, hip, case, mode, pure, unfused=True, floor_rgba=FLOOR_RGBA):
    cf, cu = ctxs[mode, True], ctxs[mode, False]
    sf = device_sources(cf, hip, case)
    su = device_sources(cu, hip, case) if unfused else None
    rgba = oracle_rgba(case, pure)
    for out in OUTS:
        got = render(cf, hip, case, out, sf)
        check_oracle(got, planes_of(rgba, out), case, out, floor_rgba)
        if unfused:
            check_same(got, render(cu, hip, case, out, su, fused=False), case, out)


# ------------------------------------------------------------------------------------------------------------------ groups 1 - 3
@pytest.mark.parametrize("seed", range(15))
def test_zoo_cpu_optimized_pure_compositor(ctxs, hip, seed):
    """CpuOptimized has no resampler in front of the compositor: textures at arbitrary fractional crops are sampled by the compositor itself."""
    run_case(ctxs, hip, zoo_case(seed, "cpu", False), "cpu", pure=True)


@pytest.mark.parametrize("seed", range(15))
def test_zoo_gpu_optimized_pure_compositor(ctxs, hip, seed):
    """GpuOptimized with every texture crop on whole texels at the layout's rounded size: nothing is resampled (asserted), the compositor alone."""
    case = zoo_case(seed, "gpu", True)
    _assert_no_resampler(case)
    run_case(ctxs, hip, case, "gpu", pure=True)


@pytest.mark.parametrize("seed", [1, 3, 4, 7, 11])   # (the lists of the zoo that hold a texture layout with a source behind it)
def test_zoo_gpu_optimized_scaled_children(ctxs, hip, seed):
    """The unrestricted zoo in GpuOptimized: resample_scaled_children in front of the compositor in the same call, the general resampler's
    tiles as its sources — against the oracle's resample-then-compose."""
    case = zoo_case(seed, "gpu", False)
    assert any(k > 0 for k in _plan_kinds(case)), "no layout with a scaled child in this list"
    run_case(ctxs, hip, case, "gpu", pure=False, unfused=False, floor_rgba=FLOOR_YUV)


# ------------------------------------------------------------------------------------------------------------------ group 5
@functools.lru_cache(maxsize=None)
def long_case(kind, mode):
    W, H = 258, 50
    if kind == "60_layouts":
        case = zoo_case(5, mode, True, n=60, size=(W, H), frame="over")
        assert len(case.layouts) == 61
    else:
        case = zoo_case(6, mode, True, n=10, size=(W, H), frame="under")
        zoo.many_masks(W, H, np.random.default_rng(66), case.layouts, 10)
        assert len(case.layouts) <= 48 and sum(len(L.masks) for L in case.layouts) > 96
    assert any(L.rotation_degrees != 0.0 for L in case.layouts) and any(L.masks for L in case.layouts)
    case.what = (kind, (W, H), mode)
    return case


@pytest.mark.parametrize("mode", ["cpu", "gpu"])
@pytest.mark.parametrize("kind", ["60_layouts", "100_masks"])
def test_lists_beyond_the_lds_copy(ctxs, hip, kind, mode):
    """More than 48 layouts, or no more than 48 layouts with more than 96 masks between them: k_compose_output's build that reads the list
    where it lies in memory — still one fused launch, on all three outputs."""
    case = long_case(kind, mode)
    if mode == "gpu":
        _assert_no_resampler(case)
    run_case(ctxs, hip, case, mode, pure=True)


# ------------------------------------------------------------------------------------------------------------------ group 6
def test_max_layouts_on_the_fused_path(hip):
    """A context of max_layouts = 3 handed five layouts draws the first three (params.rs:176-182), fused and pass-per-launch alike."""
    case = zoo_case(2, "gpu", True, n=4, size=(256, 64), frame="under")
    assert len(case.layouts) == 5
    _assert_no_resampler(case)
    first3 = Case(("max_layouts", 3), case.W, case.H, case.layouts[:3], case.sources, case.opaque, case.srgb)
    rgba3, rgba5 = oracle_rgba(first3, True), oracle_rgba(case, True)
    assert not np.array_equal(rgba3, rgba5), "the dropped layouts draw nothing: the case is vacuous"
    cf, cu = hip.Context(0, max_layouts=3), hip.Context(0, max_layouts=3)
    try:
        cu.set_fused_kernels(False)
        for out in ("rgba", "planar"):
            got = render(cf, hip, first3, out, layouts=case.layouts)
            check_oracle(got, planes_of(rgba3, out), first3, out)
            check_same(got, render(cu, hip, first3, out, fused=False, layouts=case.layouts), first3, out)
    finally:
        cf.close()
        cu.close()


# ------------------------------------------------------------------------------------------------------------------ group 7
@functools.lru_cache(maxsize=None)
def grid_case():
    """A 2 x 2 grid of 128 x 32 video tiles with labels, every tile a 4:2:0 frame: texture and select tiles read converted nodes."""
    W, H = 256, 64
    layouts, sources, _ = zoo.grid_scene(W, H, 2, 2, 0)
    frames = [zoo.frame_planes(s.shape[1], s.shape[0], 20 + i) for i, s in enumerate(sources)]
    return Case(("grid", (W, H), "gpu"), W, H, layouts, frames, [False] * len(frames), True)


@pytest.mark.parametrize("out", OUTS)
@pytest.mark.parametrize("which", ["zoo3", "zoo7", "zoo11", "grid"])
def test_predicted_grid_then_measured_grid(hip, which, out):
    """The first render of a list sizes the band part of k_compose_output's grid from the host's prediction (compose_predict), later ones from
    the count the classifier left: the same list three times on one context and once on a fresh one — four identical downloads, at the
    oracle's bar.  A tile composed in one regime and not in the other shows here."""
    case = grid_case() if which == "grid" else zoo_case(int(which[3:]), "gpu", True)
    _assert_no_resampler(case)
    a, b = hip.Context(0), hip.Context(0)
    try:
        sa = device_sources(a, hip, case)
        shots = [render(a, hip, case, out, sa, poison=0x30 + k) for k in range(3)]
        shots.append(render(b, hip, case, out, poison=0x77))
    finally:
        a.close()
        b.close()
    for k, s in enumerate(shots[1:], 1):
        check_same(s, shots[0], case, out, what=f"render {k} differs from the first ({'fresh context' if k == 3 else 'same context'})")
    check_oracle(shots[0], planes_of(oracle_rgba(case, True), out), case, out)


# ------------------------------------------------------------------------------------------------------------------ the renderer's opaque claim
def test_a_cover_beyond_max_layouts_does_not_make_the_node_opaque(hip):
    """Root view (opaque background) > gaussian blur at the node's own size, sigma 0 > nested view of four boxes: three small translucent
    ones, then an opaque full cover.  On a context of max_layouts = 3 the cover is never drawn, so the nested node is NOT opaque: the root
    must blend it over its background, not copy it (host/renderer.cpp, layouts_leave_an_opaque_surface looks at the drawn layouts only)."""
    from smelter_amd.renderer import Renderer
    from smelter_amd.scene import Scene
    W, H = 160, 48
    boxes = [(4, 8, 40, 20, "#FF000080"), (10, 60, 50, 30, "#00FF0060"), (20, 100, 44, 24, "#0000FFA0")]
    kids = [{"type": "view", "top": t, "left": l, "width": w, "height": h, "background_color": c} for t, l, w, h, c in boxes]
    kids.append({"type": "view", "top": 0, "left": 0, "width": W, "height": H, "background_color": "#C08040FF"})
    scene = {"type": "view", "background_color": "#2060A0FF", "children": [
        {"type": "shader", "shader_id": "soften", "resolution": {"width": W, "height": H}, "shader_param": {"type": "f32", "value": 0.0},
         "children": [{"type": "view", "width": W, "height": H, "children": kids}]}]}
    sc = Scene()
    sc.update(scene, W, H)
    inner, root = sc.layouts(2, 0, []), sc.layouts(0, 0, [(W, H)])
    assert len(inner) == 4 and all(L.type == 1 and L.color[3] < 1.0 and L.width < W for L in inner[:3])
    assert inner[3].color[3] == 1.0 and (inner[3].left, inner[3].top, inner[3].width, inner[3].height) == (0.0, 0.0, float(W), float(H))
    assert len(root) == 2 and root[0].type == 1 and root[0].color[3] == 1.0 and root[1].type == 0
    # the oracle: the first three layouts of the nested node, the blur, the root over its background
    node = orc.gaussian_blur(orc.apply_layouts(W, H, inner[:3], [], srgb=True), 0.0)
    want = orc.rgba_to_planar_yuv(orc.apply_layouts(W, H, root, [node], srgb=True), orc.YUV420)
    background = orc.rgba_to_planar_yuv(orc.apply_layouts(W, H, root[:1], [], srgb=True), orc.YUV420)
    empty = np.asarray(node)[..., 3] == 0
    assert empty.any() and not empty.all()
    c = hip.Context(0, max_layouts=3)
    r = Renderer(c)
    try:
        r.register_shader("soften")
        r.update_scene("out", W, H, scene)
        got = r.render(0.0, {})["out"].download()
    finally:
        r.close()
        c.close()
    empty_c = empty.reshape(H // 2, 2, W // 2, 2).all(axis=(1, 3))   # chroma samples whose four pixels are all undrawn
    for g, w, b, e, pl in zip(got, want, background, (empty, empty_c, empty_c), "YUV"):
        w, b = np.asarray(w).reshape(g.shape), np.asarray(b).reshape(g.shape)
        assert refpipe.max_diff(g, w) <= TOL, f"plane {pl}: {describe(g, w)}"
        assert refpipe.max_diff(g[e], b[e]) <= TOL, f"plane {pl}: the root's background does not show where the node drew nothing: {describe(g[e], b[e])}"
