"""Input colour matrices (SMR_MATRIX_BT601, SMR_MATRIX_BT2020_NCL in bits 8 - 11 of smr_frame.format) on the device: every kernel that turns an
input frame into a node texture against the witness (tests/color_matrix_model.py), the routes that carry a tagged frame — smr_ingest_resample
[_batch], smr_frame_preprocess, the renderer on one context, two lanes and a shard — and the refusals.  Shapes and helpers follow
tests/test_gpu_hi422.py."""
import numpy as np
import pytest

from oracle import oracle as orc
from oracle import scene as S
from tests import color_matrix_model as cm
from tests import refpipe

pytestmark = pytest.mark.gpu

BLOCK_SIZES = [(8, 2), (12, 2), (20, 4), (132, 74), (260, 10)]
ODD_SIZES = [(37, 21), (7, 5), (6, 1), (2, 2), (1, 1)]
BLOCK_FORMATS = {"420": cm.PLANAR_YUV420, "j420": cm.PLANAR_YUVJ420, "nv12": cm.NV12, "p010": cm.P010, "420p10": cm.PLANAR_YUV420P10,
                 "422p10": cm.PLANAR_YUV422P10, "p210": cm.P210, "v210": cm.V210}
GENERAL_FORMATS = {"422": cm.PLANAR_YUV422, "444": cm.PLANAR_YUV444, "uyvy": cm.UYVY422, "yuyv": cm.YUYV422}
MATRICES = [cm.BT601, cm.BT2020_NCL]


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
def ctx_general(hip):
    c = hip.Context(0)
    c.set_convert_impl(hip.CONVERT_GENERAL)
    yield c
    c.close()


def _ran(ctx, before):
    return {k: n - before[k] for k, n in ctx.kernel_launches().items()}


def _diff(got, want):
    return int((got != want).sum()), np.argwhere(got != want)[:4].tolist()


def _frame(ctx, hip, base, matrix, w, h, planes):
    """-> (the tagged device frame, the planes the witness sees): planes that are empty at this size are 1 x 1 placeholders on the device,
    zeroed here so that the witness knows their texel."""
    f = ctx.frame(hip.frame_format(base, matrix), w, h)
    up, wit = [], []
    for i, (p, s) in enumerate(zip(planes, f.plane_shapes())):
        if 0 in s:
            up.append(np.zeros(s, p.dtype))
            wit.append(np.zeros((1, 1) + tuple(s[2:]), p.dtype))
            ctx._check(ctx.lib.smr_surface_clear(ctx.handle, f.c.planes[i]))
        else:
            up.append(p)
            wit.append(p)
    f.upload(up)
    return f, wit


def _close(got, want, what):
    """The rule tests/test_gpu_parity.py and tests/test_gpu_hi422.py apply to the general kernels against the oracle / the witness at BT.709"""
    d, ex = refpipe.max_diff(got, want), refpipe.exact_fraction(got, want)
    print(what, "max_diff", d, "exact_fraction", ex)
    assert d <= 1 and ex >= 0.999, (what, d, ex)


# ------------------------------------------------------------------------------------------------ 6: the block converters

@pytest.mark.parametrize("w,h", BLOCK_SIZES)
@pytest.mark.parametrize("matrix", MATRICES)
@pytest.mark.parametrize("name", list(BLOCK_FORMATS))
def test_block_converter_writes_the_witnesss_bytes(ctx, hip, name, matrix, w, h):
    base = BLOCK_FORMATS[name]
    planes = cm.noise_planes(base, w, h, w * 31 + h + base)
    untagged, _ = _frame(ctx, hip, base, cm.BT709, w, h, planes)
    before = ctx.kernel_launches()
    ctx.frame_to_rgba(untagged)
    plain = _ran(ctx, before)
    tagged, wit = _frame(ctx, hip, base, matrix, w, h, planes)
    before = ctx.kernel_launches()
    got = ctx.frame_to_rgba(tagged).download()
    ran = _ran(ctx, before)
    want = cm.node_rgba(base, w, h, wit, matrix)
    assert np.array_equal(got, want), (name, cm.NAMES[matrix], w, h, _diff(got, want))
    assert ran["frame_to_rgba_420"] == 1 and ran["frame_to_rgba"] == 1 and ran == plain, (ran, plain)  # (the untagged frame's route)


def _device_plane(torch, arr2d, pitch):
    h, row = arr2d.shape
    buf = torch.zeros((pitch * h,), dtype=torch.uint8, device="cuda")
    buf.view(h, pitch)[:, :row] = torch.from_numpy(np.ascontiguousarray(arr2d)).cuda()
    return buf


@pytest.mark.parametrize("matrix", MATRICES)
@pytest.mark.parametrize("name", ["420", "j420", "nv12"])
def test_a_wrapped_frame_with_tight_rows_gives_the_witnesss_bytes(ctx, hip, name, matrix):
    """A frame over caller memory on the tightest pitch smr_surface_wrap admits: conv_route sends it to k_yuv420_to_rgba_tight.  What is checked
    is the bytes and that ONE block-converter launch made them; the counter is shared with the plain kernel, so which instantiation ran is not
    observable here (tests/test_emu_convert_matrix.py runs the tight build of each matrix by name, guard pages behind its planes)."""
    torch = pytest.importorskip("torch")
    w, h = 132, 74
    base = BLOCK_FORMATS[name]
    planes = cm.noise_planes(base, w, h, 77 + base)
    rows = [np.ascontiguousarray(p).view(np.uint8).reshape(p.shape[0], -1) for p in planes]
    pitches = [(r.shape[1] + 3) & ~3 for r in rows]  # the row's bytes, rounded up to the dword smr_surface_wrap asks for (66 -> 68 for planar chroma)
    bufs = [_device_plane(torch, r, p) for r, p in zip(rows, pitches)]
    frame = ctx.wrapped_frame(hip.frame_format(base, matrix), w, h, [(b.data_ptr(), p) for b, p in zip(bufs, pitches)])
    before = ctx.kernel_launches()
    got = ctx.frame_to_rgba(frame).download()
    assert _ran(ctx, before)["frame_to_rgba_420"] == 1
    want = cm.node_rgba(base, w, h, planes, matrix)
    assert np.array_equal(got, want), (name, cm.NAMES[matrix], _diff(got, want))


# ------------------------------------------------------------------------------------------------ 7: the general kernels

@pytest.mark.parametrize("w,h", [(8, 2), (132, 74), (37, 21)])
@pytest.mark.parametrize("matrix", MATRICES)
@pytest.mark.parametrize("name", list(GENERAL_FORMATS))
def test_422_444_and_packed_frames(ctx, ctx_general, hip, name, matrix, w, h):
    """k_yuv_to_rgba_batch (even sizes) and k_yuv_to_rgba / k_interleaved422_to_rgba: each other's bytes, as tests/test_gpu_parity.py demands
    at BT.709, and the witness by its rule for these kernels against the oracle."""
    base = GENERAL_FORMATS[name]
    if base in (cm.UYVY422, cm.YUYV422):
        planes = [np.random.default_rng(w + h + base).integers(0, 256, (h, w // 2, 4), dtype=np.uint8)]
    else:
        planes = cm.noise_planes(base, w, h, w * 7 + h + base)
    f, wit = _frame(ctx, hip, base, matrix, w, h, planes)
    got = ctx.frame_to_rgba(f).download()
    fg, _ = _frame(ctx_general, hip, base, matrix, w, h, planes)
    before = ctx_general.kernel_launches()
    general = ctx_general.frame_to_rgba(fg).download()
    ran = _ran(ctx_general, before)
    assert ran["frame_to_rgba_420"] == 0 and ran["frame_to_rgba"] == 1, ran
    assert np.array_equal(got, general), (name, cm.NAMES[matrix], w, h, _diff(got, general))
    _close(got, cm.node_rgba(base, w, h, wit, matrix), (name, cm.NAMES[matrix], w, h))


@pytest.mark.parametrize("matrix", MATRICES)
@pytest.mark.parametrize("name", list(BLOCK_FORMATS))
def test_general_kernels_of_the_block_formats(ctx, ctx_general, hip, name, matrix):
    """The block converter's formats through the general kernels.  From a CONVERT_GENERAL context at a block geometry: the witness's bytes and
    the default context's block-converter bytes, as tests/test_gpu_parity.py (k_yuv_to_rgba: 4:2:0, J420, NV12) and tests/test_gpu_hi_depth.py /
    tests/test_gpu_hi422.py (k_yuv_hi_to_rgba: the four word formats) demand at BT.709 — nothing before the three matrix statements changed;
    v210's general kernel has the 1 LSB / 0.999 rule there and keeps it here.  Then the geometries the block converter does not take, by that
    rule too.  Seeds: tests/test_gpu_hi422.py's for the same shapes."""
    base = BLOCK_FORMATS[name]
    w, h = 132, 74
    planes = cm.noise_planes(base, w, h, 5 + base)
    f, wit = _frame(ctx_general, hip, base, matrix, w, h, planes)
    before = ctx_general.kernel_launches()
    got = ctx_general.frame_to_rgba(f).download()
    ran = _ran(ctx_general, before)
    assert ran["frame_to_rgba_420"] == 0 and ran["frame_to_rgba"] == 1, ran
    want = cm.node_rgba(base, w, h, wit, matrix)
    fb, _ = _frame(ctx, hip, base, matrix, w, h, planes)
    before = ctx.kernel_launches()
    block = ctx.frame_to_rgba(fb).download()
    assert _ran(ctx, before)["frame_to_rgba_420"] == 1
    print(name, cm.NAMES[matrix], "general context: bytes off the witness", int((got != want).sum()), "off the block converter", int((got != block).sum()))
    if base == cm.V210:
        _close(got, want, (name, cm.NAMES[matrix], w, h, "general context"))
    else:
        assert np.array_equal(got, want), (name, cm.NAMES[matrix], w, h, _diff(got, want))
        assert np.array_equal(got, block), (name, cm.NAMES[matrix], w, h, _diff(got, block))
    for w, h in ODD_SIZES:
        planes = cm.noise_planes(base, w, h, w * 131 + h + base)
        f, wit = _frame(ctx, hip, base, matrix, w, h, planes)
        before = ctx.kernel_launches()
        got = ctx.frame_to_rgba(f).download()
        assert _ran(ctx, before)["frame_to_rgba_420"] == 0
        _close(got, cm.node_rgba(base, w, h, wit, matrix), (name, cm.NAMES[matrix], w, h))


# ------------------------------------------------------------------------------------------------ 8, 9: the resampling routes

def _camera(base, w, h, seed):
    """Camera-like content (smooth luma, slow chroma: 1 LSB end to end holds on such content) as planes of `base`; 10-bit formats get live low bits."""
    rng = np.random.default_rng(seed)
    xx, yy = np.meshgrid(np.arange(w), np.arange(h))
    y8 = 16 + (xx * 3 + yy * 2) % 200 + rng.integers(0, 8, (h, w))
    ch, cw = cm.chroma_shape(base, w, h)
    cx, cy = np.meshgrid(np.arange(cw), np.arange(ch))
    u8, v8 = 100 + (cx + cy) % 60, 140 - (2 * cx + cy) % 70
    if cm.is_hi(base):
        return cm.planes_of(base, y8 * 4 + rng.integers(0, 4, y8.shape), u8 * 4 + rng.integers(0, 4, u8.shape), v8 * 4 + rng.integers(0, 4, v8.shape))
    return cm.planes_of(base, y8, u8, v8)


def test_a_batch_that_mixes_matrices(ctx, hip):
    """Five NV12 frames of the same content tagged 709, 601, 2020, 601, 709 at 384 x 216 -> 256 x 144 (the RGB12 class route): every tile is
    the single-frame call's with that tag, the matrices' tiles differ, and the block converter is launched once per matrix present."""
    iw, ih, dw, dh = 384, 216, 256, 144
    tags = [cm.BT709, cm.BT601, cm.BT2020_NCL, cm.BT601, cm.BT709]
    planes = _camera(cm.NV12, iw, ih, 11)
    crop = (0.0, 0.0, float(iw), float(ih))
    single = {}
    for m in set(tags):
        f, _ = _frame(ctx, hip, cm.NV12, m, iw, ih, planes)
        dst = ctx.surface(dw, dh)
        assert ctx.ingest_resample(f, crop, dst) > 0
        single[m] = dst.download()
    frames = [_frame(ctx, hip, cm.NV12, m, iw, ih, planes)[0] for m in tags]
    dsts = [ctx.surface(dw, dh) for _ in tags]
    before = ctx.kernel_launches()
    kinds = ctx.ingest_resample_batch(frames, [crop] * 5, dsts)
    ran = _ran(ctx, before)
    assert all(k > 0 for k in kinds)
    assert 1 <= ran["frame_to_rgba_420"] <= 3 and ran["resample_general"] == 0 and ran["ingest_valu"] == 0, ran
    for m, d in zip(tags, dsts):
        assert np.array_equal(d.download(), single[m]), cm.NAMES[m]
    assert not np.array_equal(single[cm.BT709], single[cm.BT601]) and not np.array_equal(single[cm.BT709], single[cm.BT2020_NCL])
    assert not np.array_equal(single[cm.BT601], single[cm.BT2020_NCL])


# what the commit before the converter's routes became one classifier and one kernel table launched for test_a_batch_that_takes_every_route's
# batch (measured there, on the device): the refactor changes no launch
PARENT_LAUNCHES_OF_THE_EVERY_ROUTE_BATCH = {"frame_to_rgba": 13, "frame_to_rgba_420": 11}


def test_a_batch_that_takes_every_route(ctx, hip):
    """One ingest_resample_batch call whose frames take every converter route at once: a 16 x 4 frame of each block-kernel format (J420 and NV12
    tagged BT.601), a wrapped NV12 frame with tight rows (BT.2020: the tight kernel), a 10 x 4 planar 4:2:0 frame (the 4 x 2 batch kernel), a
    7 x 3 one (general) and seventeen 8 x 4 NV12 frames — one queue fills and is launched mid-batch (8 x 2 has no two-pass plan: 8 x 4 is the
    smallest frame the resampler's node route takes).  Every destination is byte-equal to the same frame through ingest_resample alone, and the
    two converter counters move as they did before the refactor."""
    torch = pytest.importorskip("torch")
    specs = [(BLOCK_FORMATS[n], m, 16, 4) for n, m in (("420", cm.BT709), ("j420", cm.BT601), ("nv12", cm.BT601), ("p010", cm.BT709), ("420p10", cm.BT709),
                                                      ("422p10", cm.BT709), ("p210", cm.BT709), ("v210", cm.BT709))]
    specs += [(cm.PLANAR_YUV420, cm.BT709, 10, 4), (cm.PLANAR_YUV420, cm.BT709, 7, 3)] + [(cm.NV12, cm.BT709, 8, 4)] * 17
    keep, frames = [], []
    for i, (base, m, w, h) in enumerate(specs):
        frames.append(_frame(ctx, hip, base, m, w, h, cm.noise_planes(base, w, h, 500 + i))[0])
    planes = cm.noise_planes(cm.NV12, 16, 4, 499)  # the wrapped frame: rows that fill their pitch
    rows = [np.ascontiguousarray(p).view(np.uint8).reshape(p.shape[0], -1) for p in planes]
    keep = [_device_plane(torch, r, r.shape[1]) for r in rows]
    frames.append(ctx.wrapped_frame(hip.frame_format(cm.NV12, cm.BT2020_NCL), 16, 4, [(b.data_ptr(), r.shape[1]) for b, r in zip(keep, rows)]))
    sizes = [(f.w, f.h, f.w * 3 // 4, f.h * 3 // 4) for f in frames]
    crops = [(0.0, 0.0, float(w), float(h)) for w, h, _, _ in sizes]
    single, kinds1 = [], []
    for f, c, (_, _, dw, dh) in zip(frames, crops, sizes):
        dst = ctx.surface(dw, dh)
        kinds1.append(ctx.ingest_resample(f, c, dst))
        single.append(dst.download())
    dsts = [ctx.surface(dw, dh) for _, _, dw, dh in sizes]
    before = ctx.kernel_launches()
    kinds = ctx.ingest_resample_batch(frames, crops, dsts)
    ran = _ran(ctx, before)
    print("every-route batch:", {k: ran[k] for k in PARENT_LAUNCHES_OF_THE_EVERY_ROUTE_BATCH}, "kinds", kinds)
    assert kinds == kinds1 and all(k > 0 for k in kinds), (kinds, kinds1)
    for i, (d, s) in enumerate(zip(dsts, single)):
        assert np.array_equal(d.download(), s), (i, specs[i] if i < len(specs) else "wrapped nv12", _diff(d.download(), s))
    assert {k: ran[k] for k in PARENT_LAUNCHES_OF_THE_EVERY_ROUTE_BATCH} == PARENT_LAUNCHES_OF_THE_EVERY_ROUTE_BATCH, ran


@pytest.mark.parametrize("iw,ih,dw,dh", [(64, 36, 40, 22), (256, 144, 96, 54), (384, 216, 256, 144)])
@pytest.mark.parametrize("name", ["nv12", "p010"])
def test_ingest_resample_of_a_bt601_frame_on_every_route(hip, ctx, name, iw, ih, dw, dh):
    """Against the oracle's resample of the witness node, within the 1 LSB tests/test_gpu_hi_depth.py's ingest tests allow — by default, with
    SMR_OPT_PLANE_SOURCE (which declines tagged frames: the default route's bytes), with SMR_OPT_FUSED_KERNELS 0 and with SMR_INGEST_VALU_F32."""
    base = BLOCK_FORMATS[name]
    planes = _camera(base, iw, ih, iw + dw)
    crop = (0.0, 0.0, float(iw), float(ih))
    kind, want = orc.resample(cm.node_rgba(base, iw, ih, planes, cm.BT601), crop, dw, dh)
    _, want709 = orc.resample(cm.node_rgba(base, iw, ih, planes, cm.BT709), crop, dw, dh)
    assert refpipe.max_diff(want, want709) > 2  # (the content tells the matrices apart)

    def run(c):
        f, _ = _frame(c, hip, base, cm.BT601, iw, ih, planes)
        dst = c.surface(dw, dh)
        assert c.ingest_resample(f, crop, dst) == kind
        out = dst.download()
        print(name, (iw, ih, dw, dh), "max_diff", refpipe.max_diff(out, want))
        assert refpipe.max_diff(out, want) <= 1, refpipe.max_diff(out, want)
        return out

    default = run(ctx)
    for setup in ("plane_source", "unfused", "valu_f32"):
        c = hip.Context(0)
        try:
            if setup == "plane_source":
                c.set_plane_source(True)
            elif setup == "unfused":
                c.set_fused_kernels(False)
            else:
                c.set_ingest_impl(hip.INGEST_VALU_F32)
            out = run(c)
            if setup == "plane_source":
                assert np.array_equal(out, default)
        finally:
            c.close()


def test_preprocess_of_a_tagged_frame(ctx, hip):
    w, h = 132, 74
    planes = _camera(cm.PLANAR_YUV420, w, h, 3)
    node = cm.node_rgba(cm.PLANAR_YUV420, w, h, planes, cm.BT2020_NCL)
    f, _ = _frame(ctx, hip, cm.PLANAR_YUV420, cm.BT2020_NCL, w, h, planes)
    got = ctx.frame_preprocess(f, (66, 38))
    want = orc.rescale_bilinear(node, 66, 38, orc.PX_RGBA8_SRGB)
    assert got.shape == want.shape and refpipe.max_diff(got, want) <= 1 and got.std() > 10
    assert np.array_equal(ctx.frame_preprocess(f), node)


# ------------------------------------------------------------------------------------------------ 10: the renderer

IW, IH, W, H = 128, 72, 256, 144
TAGS = [cm.BT709, cm.BT601, cm.BT2020_NCL]
SCENE = {"type": "view", "background_color": "#203040FF",
         "children": [{"type": "rescaler", "child": {"type": "input_stream", "input_id": f"in{i}"}} for i in range(3)]}


def _content():
    from tests import scenes
    return list(scenes.test_input(0, IW, IH, noise_seed=40))


def _oracle_picture(tags):
    root = S.View(children=[S.Rescaler(child=S.InputStream(i)) for i in range(3)], background_color=(0x20, 0x30, 0x40, 255))
    layouts = S.scene_layouts(root, W, H, [(IW, IH)] * 3)
    nodes = [cm.node_rgba(cm.PLANAR_YUV420, IW, IH, _content(), m) for m in tags]
    return refpipe.render_yuv420(layouts, nodes, W, H)[0]


def _render(hip, tag_sets, lanes=0, shard=False):
    """The scene rendered once per entry of tag_sets (the three inputs' matrices for that frame) -> the downloaded outputs."""
    from smelter_amd.renderer import Renderer
    root = hip.Context(0)
    extra = [hip.Context(0) for _ in range(lanes + (1 if shard else 0))]
    r = Renderer(root, lanes=extra if lanes else (), shards=extra if shard else ())
    made = []
    try:
        for i in range(3):
            r.register_input(f"in{i}")
        r.update_scene("out", W, H, SCENE)
        outs = []
        for k, tags in enumerate(tag_sets):
            frames = {}
            for i, m in enumerate(tags):
                c = r.input_context(f"in{i}") if shard else root
                frames[f"in{i}"] = c.frame(hip.frame_format(hip.FRAME_PLANAR_YUV420, m), IW, IH, _content())
            made += list(frames.values())
            outs.append(r.render(0.02 * k, frames)["out"].download())
        r.sync()
        return outs
    finally:
        r.close()
        for f in made:
            f.destroy()
        for c in [root] + extra:
            c.close()


def _within_1_lsb(got, want):
    for g, w_ in zip(got, want):
        assert refpipe.max_diff(g, w_) <= 1, refpipe.max_diff(g, w_)


@pytest.fixture(scope="module")
def single_picture(hip):
    return _render(hip, [TAGS])[0]


def test_renderer_draws_each_input_with_its_matrix(single_picture):
    want = _oracle_picture(TAGS)
    _within_1_lsb(single_picture, want)
    assert refpipe.max_diff(want[1], _oracle_picture([cm.BT709] * 3)[1]) > 2  # (the picture tells the matrices apart)


def test_renderer_on_two_lanes_and_with_a_shard_is_the_same_picture(hip, single_picture):
    for out in _render(hip, [TAGS, TAGS], lanes=1):  # (consecutive frames rotate through the lanes)
        for a, b in zip(out, single_picture):
            assert np.array_equal(a, b)
    (sharded,) = _render(hip, [TAGS], shard=True)
    for a, b in zip(sharded, single_picture):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("shard", [False, True])
def test_an_input_may_change_its_matrix_between_frames(hip, single_picture, shard):
    swapped = [cm.BT601, cm.BT2020_NCL, cm.BT709]
    first, second, third = _render(hip, [TAGS, swapped, TAGS], shard=shard)
    for a, b in zip(first, single_picture):
        assert np.array_equal(a, b)
    _within_1_lsb(second, _oracle_picture(swapped))
    assert not np.array_equal(second[1], first[1])
    for a, b in zip(third, first):
        assert np.array_equal(a, b)


# ------------------------------------------------------------------------------------------------ 11: refusals

def _hand_made_frame(ctx, hip, fmt, w, h, surfaces):
    from smelter_amd import _ffi
    f = hip.DeviceFrame.__new__(hip.DeviceFrame)
    f.ctx, f.fmt, f.w, f.h = ctx, fmt, w, h
    f.c = _ffi.Frame()
    f.c.format, f.c.width, f.c.height = fmt, w, h
    for i, s in enumerate(surfaces):
        f.c.planes[i] = s.handle.value
    return f


def test_bad_tags_are_refused_before_anything_is_launched(ctx, hip):
    w, h = 16, 8
    before = ctx.kernel_launches()
    planes = [ctx.surface(w, h, hip.PX_R8), ctx.surface(w // 2, h // 2, hip.PX_RG8)]
    rgba = ctx.surface(w, h, hip.PX_RGBA8)
    node = ctx.surface(w, h)
    for fmt, word in ((hip.frame_format(hip.FRAME_NV12, 3), "matrix"), (hip.frame_format(hip.FRAME_NV12, 15), "matrix"),
                      (hip.FRAME_NV12 | 0x1000, "bit 11"), (hip.frame_format(hip.FRAME_NV12, 1) | 0x80000000, "bit 11")):
        with pytest.raises(hip.SmrError) as e:
            ctx.frame(fmt, w, h)
        assert e.value.code == -1 and word in str(e.value), str(e.value)
        with pytest.raises(hip.SmrError) as e:
            ctx.frame_to_rgba(_hand_made_frame(ctx, hip, fmt, w, h, planes), node)
        assert e.value.code == -1 and word in str(e.value), str(e.value)
    for base in (hip.FRAME_BGRA, hip.FRAME_ARGB, hip.FRAME_RGBA):
        for m in (hip.MATRIX_BT601, hip.MATRIX_BT2020_NCL):
            with pytest.raises(hip.SmrError) as e:
                ctx.frame(hip.frame_format(base, m), w, h)
            assert e.value.code == -1 and "Y'CbCr formats only" in str(e.value), str(e.value)
            with pytest.raises(hip.SmrError) as e:
                ctx.frame_to_rgba(_hand_made_frame(ctx, hip, hip.frame_format(base, m), w, h, [rgba]), node)
            assert e.value.code == -1 and "Y'CbCr formats only" in str(e.value), str(e.value)
    assert sum(_ran(ctx, before).values()) == 0


def test_a_tagged_format_is_refused_wherever_a_frame_is_an_output(ctx, hip):
    from smelter_amd.renderer import Renderer
    from smelter_amd.scene import SceneError
    node = ctx.surface(16, 8)
    before = ctx.kernel_launches()
    for base in (hip.FRAME_PLANAR_YUV420, hip.FRAME_NV12):
        fmt = hip.frame_format(base, hip.MATRIX_BT601)
        out = ctx.frame(fmt, 16, 8)
        with pytest.raises(hip.SmrError) as e:
            ctx.rgba_to_frame(node, fmt, out)
        assert e.value.code == -1 and "colour matrix" in str(e.value)
        with pytest.raises(hip.SmrError) as e:
            ctx.fill_black(out)
        assert e.value.code == -1 and "colour matrix" in str(e.value)
    assert sum(_ran(ctx, before).values()) == 0
    r = Renderer(ctx)
    try:
        r.update_scene("out", 64, 36, {"type": "view", "background_color": "#FF0000FF"})
        first = r.render(0.0, {})["out"].download()
        with pytest.raises(SceneError) as e:
            r.update_scene("out", 64, 36, {"type": "view", "background_color": "#00FF00FF"}, output_format=hip.frame_format(hip.FRAME_PLANAR_YUV420, hip.MATRIX_BT601))
        assert "colour matrix" in str(e.value)
        again = r.render(0.02, {})["out"].download()  # the previous scene stays active
        for a, b in zip(first, again):
            assert np.array_equal(a, b)
    finally:
        r.close()
