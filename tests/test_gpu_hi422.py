"""10-bit 4:2:2 input frames (SMR_FRAME_PLANAR_YUV422P10, SMR_FRAME_P210, SMR_FRAME_V210) on the device: k_yuv422_hi_to_rgba (the block
converter), k_yuv_hi_to_rgba with 4:2:2 planes and k_yuv422_hi_to_rgba_any (v210, any geometry) against the oracle — content whose codes are
4 b has, byte for byte, the node texture of the 8-bit PLANAR_YUV422 / UYVY frame with bytes b — and against the witnesses
(tests/hi_depth_model.py, tests/hi422_model.py) on true 10-bit content; then the routes that carry such a frame: smr_ingest_resample[_batch],
smr_frame_preprocess, the renderer (one context, two lanes, a shard), and the refusals wherever a frame is an output.  Shapes and helpers
follow tests/test_gpu_hi_depth.py."""
import numpy as np
import pytest

from oracle import oracle as orc
from oracle import scene as S
from tests import hi422_model as h422
from tests import hi_depth_model as hdm
from tests import refpipe, wrapped

pytestmark = pytest.mark.gpu

BLOCK_SIZES = [(8, 2), (12, 2), (20, 4), (132, 74), (260, 10), (1024, 6)]
GENERAL_SIZES = [(37, 21), (7, 5), (6, 1), (2, 2), (1, 1)]
LAYOUTS = ["planar", "p210", "v210"]


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


def _fmt(hip, name):
    return {"planar": hip.FRAME_PLANAR_YUV422P10, "p210": hip.FRAME_P210, "v210": hip.FRAME_V210}[name]


def _cw(name, w):
    """Chroma columns the layout holds: v210 carries the pair of an odd width's last pixel, the planes are w / 2 wide."""
    return (w + 1) // 2 if name == "v210" else w // 2


def _planes10(name, y, c, junk=None):
    """10-bit codes y (h, w), chroma pairs c (h, _cw, 2) -> the format's planes.  junk: a generator for the ignored bits."""
    y, c = np.asarray(y, np.uint16), np.asarray(c, np.uint16)
    h, w = y.shape
    if name == "v210":
        n = h422.groups(w)
        return [h422.v210_pack(y, c[..., 0], c[..., 1], junk=None if junk is None else junk.integers(0, 4, (h, 4 * n)),
                               beyond=None if junk is None else junk.integers(0, 1024, (h, 6 * n)))]
    jy = np.zeros_like(y) if junk is None else junk.integers(0, 64, y.shape).astype(np.uint16)
    jc = np.zeros_like(c) if junk is None else junk.integers(0, 64, c.shape).astype(np.uint16)
    if name == "p210":
        return [np.ascontiguousarray((y << 6) | jy), np.ascontiguousarray((c << 6) | jc)]
    return [np.ascontiguousarray(y | (jy << 10)), np.ascontiguousarray(c[..., 0] | (jc[..., 0] << 10)), np.ascontiguousarray(c[..., 1] | (jc[..., 1] << 10))]


def _frame10(ctx, hip, name, y, c, junk=None):
    h, w = y.shape
    return ctx.frame(_fmt(hip, name), w, h, _planes10(name, y, c, junk))


def _clear_placeholders(ctx, frame):
    """Chroma planes of a 1-pixel-wide frame are 1 x 1 placeholders nothing uploads into: zero them so that the test knows their texel."""
    for i, shape in enumerate(frame.plane_shapes()):
        if 0 in shape:
            ctx._check(ctx.lib.smr_surface_clear(ctx.handle, frame.c.planes[i]))


def _ran(ctx, before):
    return {k: n - before[k] for k, n in ctx.kernel_launches().items()}


def _noise8(name, w, h, rng):
    return rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h, _cw(name, w), 2), dtype=np.uint8)


def _noise10(name, w, h, rng):
    return rng.integers(0, 1024, (h, w)).astype(np.uint16), rng.integers(0, 1024, (h, _cw(name, w), 2)).astype(np.uint16)


def _camera8(w, h, rng):
    """Camera-like content in 4:2:2 geometry: smooth luma, slow chroma (1 LSB end to end holds on such content)."""
    xx, yy = np.meshgrid(np.arange(w), np.arange(h))
    y8 = (16 + (xx * 3 + yy * 2) % 200 + rng.integers(0, 8, (h, w))).astype(np.uint8)
    cx, cy = xx[:, :w // 2], yy[:, :w // 2]
    c8 = np.stack([100 + (cx + cy // 2) % 60, 140 - (2 * cx + cy // 2) % 70], -1).astype(np.uint8)
    return y8, c8


def _oracle8(name, y, c):
    h, w = y.shape
    if name == "v210":
        return orc.interleaved422_to_rgba(h422.uyvy_of(y, c[..., 0], c[..., 1]), w, h, 0)
    return orc.planar_yuv_to_rgba(y, np.ascontiguousarray(c[..., 0]), np.ascontiguousarray(c[..., 1]), w, h, orc.YUV422)


def _witness(name, y, c):
    if name == "v210":
        return h422.node_rgba_v210(y, c[..., 0], c[..., 1])
    cu = c[..., 0] if c.size else np.zeros((1, 1), np.uint16)  # (an empty chroma plane: the zeroed 1 x 1 placeholder)
    cv = c[..., 1] if c.size else np.zeros((1, 1), np.uint16)
    return hdm.node_rgba(y, cu, cv)


def _x4(a):
    return a.astype(np.uint16) * 4


def _diff(got, want):
    return int((got != want).sum()), np.argwhere(got != want)[:4].tolist()


# ------------------------------------------------------------------------------------------------ the block converter

@pytest.mark.parametrize("w,h", BLOCK_SIZES)
@pytest.mark.parametrize("name", LAYOUTS)
def test_block_converter_writes_the_oracles_and_the_witnesss_bytes(ctx, ctx_general, hip, name, w, h):
    rng = np.random.default_rng(w * 31 + h + LAYOUTS.index(name))
    # codes 4 b: the oracle's bytes of b
    y8, c8 = _noise8(name, w, h, rng)
    before = ctx.kernel_launches()
    got = ctx.frame_to_rgba(_frame10(ctx, hip, name, _x4(y8), _x4(c8))).download()
    ran = _ran(ctx, before)
    want = _oracle8(name, y8, c8)
    assert np.array_equal(got, want), (name, w, h, _diff(got, want))
    assert ran["frame_to_rgba_420"] == 1 and ran["frame_to_rgba"] == 1, ran  # (the block converter's slot: one launch)
    # true 10-bit codes: the witness's bytes
    y, c = _noise10(name, w, h, rng)
    got = ctx.frame_to_rgba(_frame10(ctx, hip, name, y, c)).download()
    want = _witness(name, y, c)
    assert np.array_equal(got, want), (name, w, h, _diff(got, want))
    # the general kernel from a CONVERT_GENERAL context: no block launch; planar and P210 give the block converter's bytes
    before = ctx_general.kernel_launches()
    general = ctx_general.frame_to_rgba(_frame10(ctx_general, hip, name, y, c)).download()
    ran = _ran(ctx_general, before)
    assert ran["frame_to_rgba_420"] == 0 and ran["frame_to_rgba"] == 1, ran
    if name != "v210":
        assert np.array_equal(got, general), (name, w, h, _diff(got, general))
    else:
        assert refpipe.max_diff(general, want) <= 1 and refpipe.exact_fraction(general, want) >= 0.999


def test_ignored_bits_are_ignored_on_the_device(ctx, hip):
    """v210 bits 30 - 31 and the components beyond w, the six other bits of P210 and planar words, all random: the clean frame's bytes (block and
    general geometry)."""
    for w, h in ((132, 74), (260, 10), (37, 21)):
        for name in LAYOUTS:
            rng = np.random.default_rng(5 + w)
            y, c = _noise10(name, w, h, rng)
            clean = ctx.frame_to_rgba(_frame10(ctx, hip, name, y, c)).download()
            got = ctx.frame_to_rgba(_frame10(ctx, hip, name, y, c, junk=np.random.default_rng(w))).download()
            assert np.array_equal(got, clean), (name, w, h, _diff(got, clean))
            want = _witness(name, y, c)
            if w % 4 == 0:
                assert np.array_equal(got, want)
            else:
                assert refpipe.max_diff(got, want) <= 1 and refpipe.exact_fraction(got, want) >= 0.999


# ------------------------------------------------------------------------------------------------ any geometry

@pytest.mark.parametrize("w,h", GENERAL_SIZES)
@pytest.mark.parametrize("name", LAYOUTS)
def test_general_kernel_is_the_8_bit_general_kernel_on_4b_and_the_witness_within_1_lsb(ctx, ctx_general, hip, name, w, h):
    rng = np.random.default_rng(w * 131 + h + LAYOUTS.index(name))
    y8, c8 = _noise8(name, w, h, rng)
    f10 = _frame10(ctx, hip, name, _x4(y8), _x4(c8))
    _clear_placeholders(ctx, f10)
    before = ctx.kernel_launches()
    got = ctx.frame_to_rgba(f10).download()
    ran = _ran(ctx, before)
    assert ran["frame_to_rgba_420"] == 0 and ran["frame_to_rgba"] == 1, ran
    if name != "v210":  # k_yuv_to_rgba on the PLANAR_YUV422 frame: the same statements, so no tolerance
        f8 = ctx_general.frame(hip.FRAME_PLANAR_YUV422, w, h, [y8, np.ascontiguousarray(c8[..., 0]), np.ascontiguousarray(c8[..., 1])])
        _clear_placeholders(ctx_general, f8)
        want = ctx_general.frame_to_rgba(f8).download()
        assert np.array_equal(got, want), (name, w, h, _diff(got, want))
    # true 10-bit content: tests/test_gpu_parity.py's rule for the 8-bit general kernels against the oracle
    y, c = _noise10(name, w, h, rng)
    f10 = _frame10(ctx, hip, name, y, c)
    _clear_placeholders(ctx, f10)
    got = ctx.frame_to_rgba(f10).download()
    want = _witness(name, y, c)
    assert refpipe.max_diff(got, want) <= 1 and refpipe.exact_fraction(got, want) >= 0.999, (name, w, h, refpipe.max_diff(got, want), refpipe.exact_fraction(got, want))


@pytest.mark.parametrize("w,h", [(8, 1), (10, 3), (22, 5), (132, 74)])
def test_v210_with_codes_4b_is_the_devices_own_uyvy_node(ctx, ctx_general, hip, w, h):
    """Even widths from 8: a v210 frame with codes 4 b has the node texture of the UYVY frame with bytes b — k_yuv422_hi_to_rgba_any against
    k_interleaved422_to_rgba (a CONVERT_GENERAL context), and whichever kernels the default context picks for the two."""
    rng = np.random.default_rng(w + h)
    y8, c8 = _noise8("v210", w, h, rng)
    for c in (ctx_general, ctx):
        got = c.frame_to_rgba(_frame10(c, hip, "v210", _x4(y8), _x4(c8))).download()
        want = c.frame_to_rgba(c.frame(hip.FRAME_UYVY422, w, h, [h422.uyvy_of(y8, c8[..., 0], c8[..., 1])])).download()
        assert np.array_equal(got, want), (w, h, _diff(got, want))


# ------------------------------------------------------------------------------------------------ memory the caller owns

def _device_plane(torch, arr2d, pitch):
    """rows of `arr2d` (h x row bytes) at `pitch` in a device buffer of EXACTLY pitch * h bytes (torch rounds its own allocation up)."""
    h, row = arr2d.shape
    buf = torch.zeros((pitch * h,), dtype=torch.uint8, device="cuda")
    buf.view(h, pitch)[:, :row] = torch.from_numpy(np.ascontiguousarray(arr2d)).cuda()
    return buf


@pytest.mark.parametrize("name,pitch_kind", [("v210", "capture"), ("v210", "tight"), ("p210", "tight")])
def test_a_wrapped_frame_gives_the_owned_frames_bytes(ctx, hip, name, pitch_kind):
    """A v210 plane on a capture card's row stride ((w + 47) / 48) * 128 and one with tight rows, a P210 frame with tight rows: the block
    converter takes them as they are and writes the owned frame's bytes."""
    torch = pytest.importorskip("torch")
    w, h = 256, 18
    y, c = _noise10(name, w, h, np.random.default_rng(77))
    planes = _planes10(name, y, c)
    owned = ctx.frame_to_rgba(ctx.frame(_fmt(hip, name), w, h, planes)).download()
    rows = [p.view(np.uint8).reshape(h, -1) for p in planes]
    pitches = [((w + 47) // 48) * 128 if pitch_kind == "capture" else r.shape[1] for r in rows]  # tight: pitch = the row's bytes
    assert all(p >= r.shape[1] for p, r in zip(pitches, rows))
    bufs = [_device_plane(torch, r, p) for r, p in zip(rows, pitches)]
    frame = ctx.wrapped_frame(_fmt(hip, name), w, h, [(b.data_ptr(), p) for b, p in zip(bufs, pitches)])
    before = ctx.kernel_launches()
    got = ctx.frame_to_rgba(frame).download()
    assert _ran(ctx, before)["frame_to_rgba_420"] == 1
    assert np.array_equal(got, owned) and np.array_equal(got, _witness(name, y, c))


@pytest.mark.parametrize("geometry", wrapped.GEOMETRIES)
@pytest.mark.parametrize("name,w,h", [("planar", 132, 74), ("p210", 132, 74), ("v210", 132, 74), ("v210", 37, 21)])
def test_a_destination_in_caller_memory_keeps_every_byte_outside_its_texels(ctx, hip, geometry, name, w, h):
    torch = pytest.importorskip("torch")
    y, c = _noise10(name, w, h, np.random.default_rng(w + h))
    dst = wrapped.WrappedSurface(torch, ctx, w, h, hip.PX_RGBA8, geometry, seed=w * h + len(geometry), align=16 if w % 4 == 0 else 4)
    before = ctx.kernel_launches()
    ctx.frame_to_rgba(_frame10(ctx, hip, name, y, c), dst.surface)
    ctx.sync()
    got = dst.texels(f"frame_to_rgba {name}")
    if w % 4 == 0:
        assert _ran(ctx, before)["frame_to_rgba_420"] == 1
        assert np.array_equal(got, _witness(name, y, c))
    else:
        assert refpipe.max_diff(got, _witness(name, y, c)) <= 1


# ------------------------------------------------------------------------------------------------ the resampling routes

@pytest.mark.parametrize("iw,ih,dw,dh", [(64, 36, 40, 22), (256, 144, 96, 54), (384, 216, 256, 144)])  # (the last: scale 1.5, a class build — the RGB12 node route)
def test_ingest_resample_of_the_three_layouts(ctx, hip, iw, ih, dw, dh):
    """A planar 10-bit 4:2:2, a P210 and a v210 input of the same camera-like picture through smr_ingest_resample and through ONE
    smr_ingest_resample_batch call: the planar and P210 tiles byte-equal, every tile within 1 LSB of the oracle's resample of the witness node.
    Each layout's frame goes through the block converter (one launch per layout in the batch) and the matrix-core resampler on its node —
    at the last size the class build that reads RGB12 nodes (smr_conv_rgb12_ok answers for these frames; the route has no counter of its own:
    the block-converter and k_ingest_wave counters and the absence of general resampler launches are what is asserted)."""
    rng = np.random.default_rng(iw + dw)
    y8, c8 = _camera8(iw, ih, rng)
    y10, c10 = _x4(y8) + rng.integers(0, 4, y8.shape).astype(np.uint16), _x4(c8) + rng.integers(0, 4, c8.shape).astype(np.uint16)  # true 10-bit: the two fractional bits are live
    frames = [_frame10(ctx, hip, name, y10, c10) for name in LAYOUTS]
    crop = (0.0, 0.0, float(iw), float(ih))
    wants = []
    for name in LAYOUTS:
        kind, want = orc.resample(_witness(name, y10, c10), crop, dw, dh)
        assert kind > 0
        wants.append(want)
    singles = []
    for f in frames:
        dst = ctx.surface(dw, dh)
        assert ctx.ingest_resample(f, crop, dst) == kind
        singles.append(dst.download())
    dsts = [ctx.surface(dw, dh) for _ in frames]
    before = ctx.kernel_launches()
    assert ctx.ingest_resample_batch(frames, [crop] * 3, dsts) == [kind] * 3
    ran = _ran(ctx, before)
    assert ran["frame_to_rgba_420"] == 3 and ran["frame_to_rgba"] == 3, ran  # (one block-converter launch per layout)
    if (iw, dw) == (384, 256):
        assert ran["ingest_wave_rgba"] >= 1 and ran["resample_general"] == 0 and ran["ingest_valu"] == 0, ran
    batch = [d.download() for d in dsts]
    for tiles in (singles, batch):
        assert np.array_equal(tiles[0], tiles[1])
        for t, want in zip(tiles, wants):
            assert refpipe.max_diff(t, want) <= 1, refpipe.max_diff(t, want)
    for a, b in zip(singles, batch):
        assert np.array_equal(a, b)


def test_preprocess_of_a_v210_frame(ctx, hip):
    w, h = 132, 74
    y8, c8 = _camera8(w, h, np.random.default_rng(3))
    node = orc.interleaved422_to_rgba(h422.uyvy_of(y8, c8[..., 0], c8[..., 1]), w, h, 0)
    got = ctx.frame_preprocess(_frame10(ctx, hip, "v210", _x4(y8), _x4(c8)), (66, 38))
    want = orc.rescale_bilinear(node, 66, 38, orc.PX_RGBA8_SRGB)
    assert got.shape == want.shape and refpipe.max_diff(got, want) <= 1 and got.std() > 10
    got = ctx.frame_preprocess(_frame10(ctx, hip, "v210", _x4(y8), _x4(c8)))
    assert np.array_equal(got, node)


# ------------------------------------------------------------------------------------------------ the renderer

IW, IH, W, H = 320, 180, 256, 144
SCENE = {"type": "view", "background_color": "#203040FF",
         "children": [{"type": "rescaler", "child": {"type": "input_stream", "input_id": f"in{i}"}} for i in range(2)]}


def _inputs8():
    """The existing oracle_picture tests' inputs in 4:2:2 geometry: every chroma row twice."""
    from tests import scenes
    out = []
    for i in range(2):
        y, u, v = scenes.test_input(i, IW, IH, noise_seed=40 + i)
        out.append((y, np.ascontiguousarray(np.repeat(np.stack([u, v], -1), 2, axis=0))))
    return out


@pytest.fixture(scope="module")
def oracle_pictures():
    root = S.View(children=[S.Rescaler(child=S.InputStream(i)) for i in range(2)], background_color=(0x20, 0x30, 0x40, 255))
    layouts = S.scene_layouts(root, W, H, [(IW, IH)] * 2)
    out = {}
    for name in ("p210", "v210"):
        nodes = [_oracle8(name, y, c) for y, c in _inputs8()]
        out[name], _ = refpipe.render_yuv420(layouts, nodes, W, H)
    return out


def _render(hip, name, lanes=0, shard=False, frames_n=1):
    """The scene rendered `frames_n` times with inputs of layout `name` -> the downloaded outputs."""
    from smelter_amd.renderer import Renderer
    root = hip.Context(0)
    extra = [hip.Context(0) for _ in range(lanes + (1 if shard else 0))]
    r = Renderer(root, lanes=extra if lanes else (), shards=extra if shard else ())
    frames = {}
    try:
        for i, (y8, c8) in enumerate(_inputs8()):
            r.register_input(f"in{i}")
            c = r.input_context(f"in{i}") if shard else root
            frames[f"in{i}"] = _frame10(c, hip, name, _x4(y8), _x4(c8))
        r.update_scene("out", W, H, SCENE)
        outs = [r.render(0.02 * k, frames)["out"].download() for k in range(frames_n)]
        r.sync()
        return outs
    finally:
        r.close()
        for f in frames.values():
            f.destroy()
        for c in [root] + extra:
            c.close()


def _within_1_lsb(got, want):
    for g, w_ in zip(got, want):
        assert refpipe.max_diff(g, w_) <= 1, refpipe.max_diff(g, w_)


@pytest.fixture(scope="module")
def single_pictures(hip):
    return {name: _render(hip, name)[0] for name in ("p210", "v210")}


@pytest.mark.parametrize("name", ["p210", "v210"])
def test_renderer_draws_the_oracle_picture(single_pictures, oracle_pictures, name):
    _within_1_lsb(single_pictures[name], oracle_pictures[name])
    assert single_pictures[name][0].std() > 10


@pytest.mark.parametrize("name", ["p210", "v210"])
def test_renderer_on_two_lanes_is_the_single_lane_frame(hip, single_pictures, oracle_pictures, name):
    for out in _render(hip, name, lanes=1, frames_n=2):  # (consecutive frames rotate through the lanes)
        _within_1_lsb(out, oracle_pictures[name])
        for a, b in zip(out, single_pictures[name]):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("name", ["p210", "v210"])
def test_renderer_with_a_shard_is_the_single_context_frame(hip, single_pictures, oracle_pictures, name):
    (sharded,) = _render(hip, name, shard=True)
    _within_1_lsb(sharded, oracle_pictures[name])
    for a, b in zip(sharded, single_pictures[name]):
        assert np.array_equal(a, b)


# ------------------------------------------------------------------------------------------------ input only

def test_the_formats_are_refused_wherever_a_frame_is_an_output(ctx, hip):
    from smelter_amd.renderer import Renderer
    from smelter_amd.scene import SceneError
    node = ctx.surface(16, 8)
    for name in LAYOUTS:
        fmt = _fmt(hip, name)
        out = ctx.frame(fmt, 16, 8)
        with pytest.raises(hip.SmrError) as e:
            ctx.rgba_to_frame(node, fmt, out)
        assert e.value.code == -1 and "input only" in str(e.value)
        with pytest.raises(hip.SmrError) as e:
            ctx.fill_black(out)
        assert e.value.code == -1 and "input only" in str(e.value)
        r = Renderer(ctx)
        try:
            with pytest.raises(SceneError) as e:
                r.update_scene("out", 64, 36, {"type": "view"}, output_format=fmt)
            assert "input only" in str(e.value)
        finally:
            r.close()


def _hand_made_frame(ctx, hip, fmt, w, h, surfaces):
    from smelter_amd import _ffi
    f = hip.DeviceFrame.__new__(hip.DeviceFrame)
    f.ctx, f.fmt, f.w, f.h = ctx, fmt, w, h
    f.c = _ffi.Frame()
    f.c.format, f.c.width, f.c.height = fmt, w, h
    for i, s in enumerate(surfaces):
        f.c.planes[i] = s.handle.value
    return f


def test_a_v210_frame_whose_plane_is_half_the_width_in_texels_is_refused(ctx, hip):
    w, h = 48, 8  # (a v210 plane is 4 ceil(w / 6) = 32 texels wide, not UYVY's w / 2 = 24)
    plane = ctx.surface(w // 2, h, hip.PX_RGBA8)
    with pytest.raises(hip.SmrError) as e:
        ctx.frame_to_rgba(_hand_made_frame(ctx, hip, hip.FRAME_V210, w, h, [plane]))
    assert e.value.code == -1 and "plane 0" in str(e.value)
    plane.destroy()


def test_a_p210_frame_whose_uv_plane_is_r16_is_refused(ctx, hip):
    w, h = 16, 8
    ys, uv = ctx.surface(w, h, hip.PX_R16), ctx.surface(w // 2, h, hip.PX_R16)
    with pytest.raises(hip.SmrError) as e:
        ctx.frame_to_rgba(_hand_made_frame(ctx, hip, hip.FRAME_P210, w, h, [ys, uv]))
    assert e.value.code == -1 and "plane 1" in str(e.value)
    ys.destroy(); uv.destroy()
