"""10-bit 4:2:0 input frames (SMR_FRAME_P010, SMR_FRAME_PLANAR_YUV420P10) on the device: k_yuv420_hi_to_rgba (the block converter) and
k_yuv_hi_to_rgba (any geometry) against the oracle — content whose codes are 4 b has, byte for byte, the node texture of the 8-bit frame with
bytes b — and against tests/hi_depth_model.py, the numpy restatement of the oracle's sequence, on true 10-bit content; then the routes that
carry such a frame: smr_ingest_resample[_batch], the renderer (one context, two lanes, a shard), smr_frame_preprocess, and the refusals
wherever a frame is an output."""
import numpy as np
import pytest

from oracle import oracle as orc
from oracle import scene as S
from tests import hi_depth_model as hdm
from tests import refpipe, wrapped

pytestmark = pytest.mark.gpu

BLOCK_SIZES = [(8, 2), (8, 6), (12, 6), (132, 74), (260, 10), (1024, 6)]
GENERAL_SIZES = [(37, 21), (7, 5), (2, 2), (1, 1)]


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
    return hip.FRAME_P010 if name == "p010" else hip.FRAME_PLANAR_YUV420P10


def _planes10(y, c, p010):
    """10-bit codes y (h, w), chroma pairs c (h/2, w/2, 2) -> the format's planes of 16-bit words."""
    y, c = np.asarray(y, np.uint16), np.asarray(c, np.uint16)
    if p010:
        return [np.ascontiguousarray(y << 6), np.ascontiguousarray(c << 6)]
    return [np.ascontiguousarray(y), np.ascontiguousarray(c[..., 0]), np.ascontiguousarray(c[..., 1])]


def _planes8(y, c, nv12):
    return [y, np.ascontiguousarray(c)] if nv12 else [y, np.ascontiguousarray(c[..., 0]), np.ascontiguousarray(c[..., 1])]


def _frame10(ctx, hip, name, w, h, y, c):
    return ctx.frame(_fmt(hip, name), w, h, _planes10(y, c, name == "p010"))


def _clear_placeholders(ctx, frame):
    """Chroma planes of a 1-pixel-wide / -high frame are 1 x 1 placeholders nothing uploads into: zero them so that the test knows their texel."""
    for i, shape in enumerate(frame.plane_shapes()):
        if 0 in shape:
            ctx._check(ctx.lib.smr_surface_clear(ctx.handle, frame.c.planes[i]))


def _ran(ctx, before):
    return {k: n - before[k] for k, n in ctx.kernel_launches().items()}


def _noise8(w, h, rng):
    return rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h // 2, w // 2, 2), dtype=np.uint8)


def _noise10(w, h, rng):
    return rng.integers(0, 1024, (h, w)).astype(np.uint16), rng.integers(0, 1024, (h // 2, w // 2, 2)).astype(np.uint16)


def _oracle8(y, c, w, h, nv12):
    if nv12:
        return orc.nv12_to_rgba(y, np.ascontiguousarray(c), w, h)
    return orc.planar_yuv_to_rgba(y, np.ascontiguousarray(c[..., 0]), np.ascontiguousarray(c[..., 1]), w, h, orc.YUV420)


# ------------------------------------------------------------------------------------------------ the block converter

@pytest.mark.parametrize("w,h", BLOCK_SIZES)
@pytest.mark.parametrize("name", ["p010", "planar"])
def test_block_converter_writes_the_oracles_and_the_witnesss_bytes(ctx, ctx_general, hip, name, w, h):
    rng = np.random.default_rng(w * 31 + h + (name == "p010"))
    # codes 4 b: the oracle's bytes of b
    y8, c8 = _noise8(w, h, rng)
    before = ctx.kernel_launches()
    got = ctx.frame_to_rgba(_frame10(ctx, hip, name, w, h, y8.astype(np.uint16) * 4, c8.astype(np.uint16) * 4)).download()
    ran = _ran(ctx, before)
    want = _oracle8(y8, c8, w, h, name == "p010")
    assert np.array_equal(got, want), (name, w, h, int((got != want).sum()), np.argwhere(got != want)[:4].tolist())
    assert ran["frame_to_rgba_420"] == 1 and ran["frame_to_rgba"] == 1, ran  # (the block converter of 4:2:0 frames: one launch)
    # true 10-bit codes: the witness's bytes, and the general kernel's
    y, c = _noise10(w, h, rng)
    got = ctx.frame_to_rgba(_frame10(ctx, hip, name, w, h, y, c)).download()
    want = hdm.node_rgba(y, c[..., 0], c[..., 1])
    assert np.array_equal(got, want), (name, w, h, int((got != want).sum()), np.argwhere(got != want)[:4].tolist())
    before = ctx_general.kernel_launches()
    general = ctx_general.frame_to_rgba(_frame10(ctx_general, hip, name, w, h, y, c)).download()
    ran = _ran(ctx_general, before)
    assert ran["frame_to_rgba_420"] == 0 and ran["frame_to_rgba"] == 1, ran
    assert np.array_equal(got, general), (name, w, h, int((got != general).sum()))


def test_ignored_bits_of_the_words_are_ignored_on_the_device(ctx, hip):
    """P010 words with random low six bits, planar words with random high six bits: the clean frame's bytes (block and general geometry)."""
    rng = np.random.default_rng(5)
    for w, h in ((132, 74), (37, 21)):
        y, c = _noise10(w, h, rng)
        jy, jc = rng.integers(0, 64, y.shape).astype(np.uint16), rng.integers(0, 64, c.shape).astype(np.uint16)
        want = hdm.node_rgba(y, c[..., 0], c[..., 1])
        p = ctx.frame(hip.FRAME_P010, w, h, [(y << 6) | jy, (c << 6) | jc])
        q = ctx.frame(hip.FRAME_PLANAR_YUV420P10, w, h, [y | (jy << 10), c[..., 0] | (jc[..., 0] << 10), c[..., 1] | (jc[..., 1] << 10)])
        for f in (p, q):
            got = ctx.frame_to_rgba(f).download()
            if w % 4 == 0:
                assert np.array_equal(got, want)
            else:
                assert refpipe.max_diff(got, want) <= 1 and refpipe.exact_fraction(got, want) >= 0.999


# ------------------------------------------------------------------------------------------------ any geometry

@pytest.mark.parametrize("w,h", GENERAL_SIZES)
@pytest.mark.parametrize("name", ["p010", "planar"])
def test_general_kernel_is_the_8_bit_general_kernel_on_4b_and_the_witness_within_1_lsb(ctx, ctx_general, hip, name, w, h):
    rng = np.random.default_rng(w * 131 + h + (name == "p010"))
    nv = name == "p010"
    y8, c8 = _noise8(w, h, rng)
    f8 = ctx_general.frame(hip.FRAME_NV12 if nv else hip.FRAME_PLANAR_YUV420, w, h, _planes8(y8, c8, nv))
    _clear_placeholders(ctx_general, f8)
    want = ctx_general.frame_to_rgba(f8).download()  # k_yuv_to_rgba: the same statements, so no tolerance
    f10 = _frame10(ctx, hip, name, w, h, y8.astype(np.uint16) * 4, c8.astype(np.uint16) * 4)
    _clear_placeholders(ctx, f10)
    before = ctx.kernel_launches()
    got = ctx.frame_to_rgba(f10).download()
    ran = _ran(ctx, before)
    assert ran["frame_to_rgba_420"] == 0 and ran["frame_to_rgba"] == 1, ran
    assert np.array_equal(got, want), (name, w, h, int((got != want).sum()))
    # true 10-bit content: tests/test_gpu_parity.py's rule for the 8-bit general kernel against the oracle
    y, c = _noise10(w, h, rng)
    f10 = _frame10(ctx, hip, name, w, h, y, c)
    _clear_placeholders(ctx, f10)
    got = ctx.frame_to_rgba(f10).download()
    cu = c[..., 0] if c.size else np.zeros((1, 1), np.uint16)   # (an empty chroma plane: the zeroed 1 x 1 placeholder)
    cv = c[..., 1] if c.size else np.zeros((1, 1), np.uint16)
    want = hdm.node_rgba(y, cu, cv)
    assert refpipe.max_diff(got, want) <= 1 and refpipe.exact_fraction(got, want) >= 0.999, (name, w, h, refpipe.max_diff(got, want), refpipe.exact_fraction(got, want))


# ------------------------------------------------------------------------------------------------ memory the caller owns

def _device_plane(torch, arr2d, pitch):
    """rows of `arr2d` (h x row bytes) at `pitch` in a device buffer of EXACTLY pitch * h bytes (torch rounds its own allocation up)."""
    h, row = arr2d.shape
    buf = torch.zeros((pitch * h,), dtype=torch.uint8, device="cuda")
    buf.view(h, pitch)[:, :row] = torch.from_numpy(np.ascontiguousarray(arr2d)).cuda()
    return buf


def test_a_wrapped_p010_frame_with_tight_rows_gives_the_owned_frames_bytes(ctx, hip):
    torch = pytest.importorskip("torch")
    w, h = 256, 18
    y, c = _noise10(w, h, np.random.default_rng(77))
    planes = _planes10(y, c, True)
    owned = ctx.frame_to_rgba(ctx.frame(hip.FRAME_P010, w, h, planes)).download()
    rows = [planes[0].view(np.uint8).reshape(h, 2 * w), planes[1].view(np.uint8).reshape(h // 2, 2 * w)]  # pitch = the row's bytes
    bufs = [_device_plane(torch, r, r.shape[1]) for r in rows]
    frame = ctx.wrapped_frame(hip.FRAME_P010, w, h, [(b.data_ptr(), r.shape[1]) for b, r in zip(bufs, rows)])
    before = ctx.kernel_launches()
    got = ctx.frame_to_rgba(frame).download()
    assert _ran(ctx, before)["frame_to_rgba_420"] == 1
    assert np.array_equal(got, owned) and np.array_equal(got, hdm.node_rgba(y, c[..., 0], c[..., 1]))


@pytest.mark.parametrize("geometry", wrapped.GEOMETRIES)
@pytest.mark.parametrize("name,w,h", [("p010", 132, 74), ("planar", 132, 74), ("p010", 37, 21), ("planar", 7, 5)])
def test_a_destination_in_caller_memory_keeps_every_byte_outside_its_texels(ctx, hip, geometry, name, w, h):
    torch = pytest.importorskip("torch")
    y, c = _noise10(w, h, np.random.default_rng(w + h))
    dst = wrapped.WrappedSurface(torch, ctx, w, h, hip.PX_RGBA8, geometry, seed=w * h + len(geometry), align=16 if w % 4 == 0 else 4)
    before = ctx.kernel_launches()
    ctx.frame_to_rgba(_frame10(ctx, hip, name, w, h, y, c), dst.surface)
    ctx.sync()
    got = dst.texels(f"frame_to_rgba {name}")
    if w % 4 == 0:
        assert _ran(ctx, before)["frame_to_rgba_420"] == 1
        assert np.array_equal(got, hdm.node_rgba(y, c[..., 0], c[..., 1]))
    else:
        assert refpipe.max_diff(got, hdm.node_rgba(y, c[..., 0], c[..., 1])) <= 1


# ------------------------------------------------------------------------------------------------ the resampling routes

@pytest.mark.parametrize("iw,ih,dw,dh", [(64, 36, 40, 22), (256, 144, 96, 54), (384, 216, 256, 144)])  # (the last: scale 1.5, a class build — the RGB12 node route)
def test_ingest_resample_of_10_bit_inputs_equals_the_nv12_inputs_tile(ctx, hip, iw, ih, dw, dh):
    """An NV12, a P010 and a planar 10-bit input together — the 10-bit ones carry 4 b of the NV12 input's bytes — through smr_ingest_resample
    and through ONE smr_ingest_resample_batch call: the three tiles byte-equal, each within 1 LSB of the oracle's resample of the oracle node."""
    rng = np.random.default_rng(iw + dw)
    xx, yy = np.meshgrid(np.arange(iw), np.arange(ih))
    y8 = (16 + (xx * 3 + yy * 2) % 200 + rng.integers(0, 8, (ih, iw))).astype(np.uint8)  # camera-like: 1 LSB end to end holds on such content
    c8 = np.stack([100 + (xx[:ih // 2, :iw // 2] + yy[:ih // 2, :iw // 2]) % 60, 140 - (2 * xx[:ih // 2, :iw // 2] + yy[:ih // 2, :iw // 2]) % 70], -1).astype(np.uint8)
    y10, c10 = y8.astype(np.uint16) * 4, c8.astype(np.uint16) * 4
    frames = [ctx.frame(hip.FRAME_NV12, iw, ih, [y8, c8]), _frame10(ctx, hip, "p010", iw, ih, y10, c10), _frame10(ctx, hip, "planar", iw, ih, y10, c10)]
    crop = (0.0, 0.0, float(iw), float(ih))
    kind, want = orc.resample(orc.nv12_to_rgba(y8, c8, iw, ih), crop, dw, dh)
    assert kind > 0
    singles = []
    for f in frames:
        dst = ctx.surface(dw, dh)
        assert ctx.ingest_resample(f, crop, dst) == kind
        singles.append(dst.download())
    dsts = [ctx.surface(dw, dh) for _ in frames]
    assert ctx.ingest_resample_batch(frames, [crop] * 3, dsts) == [kind] * 3
    batch = [d.download() for d in dsts]
    for tiles in (singles, batch):
        assert np.array_equal(tiles[0], tiles[1]) and np.array_equal(tiles[0], tiles[2])
        for t in tiles:
            assert refpipe.max_diff(t, want) <= 1, refpipe.max_diff(t, want)


def test_preprocess_of_a_p010_frame_equals_that_of_the_nv12_frame(ctx, hip):
    w, h = 132, 74
    y8, c8 = _noise8(w, h, np.random.default_rng(3))
    a = ctx.frame_preprocess(ctx.frame(hip.FRAME_NV12, w, h, [y8, c8]), (66, 38))
    b = ctx.frame_preprocess(_frame10(ctx, hip, "p010", w, h, y8.astype(np.uint16) * 4, c8.astype(np.uint16) * 4), (66, 38))
    assert np.array_equal(a, b) and a.std() > 10
    a = ctx.frame_preprocess(ctx.frame(hip.FRAME_NV12, w, h, [y8, c8]))
    b = ctx.frame_preprocess(_frame10(ctx, hip, "p010", w, h, y8.astype(np.uint16) * 4, c8.astype(np.uint16) * 4))
    assert np.array_equal(a, b) and np.array_equal(a, orc.nv12_to_rgba(y8, c8, w, h))


# ------------------------------------------------------------------------------------------------ the renderer

IW, IH, W, H = 320, 180, 256, 144
SCENE = {"type": "view", "background_color": "#203040FF",
         "children": [{"type": "rescaler", "child": {"type": "input_stream", "input_id": f"in{i}"}} for i in range(2)]}
RESAMPLERS = ("ingest_wave", "ingest_wave_rgba", "ingest_valu", "resample_general", "ingest_wave_direct", "compose_output", "apply_layouts")


def _inputs8():
    from tests import scenes
    out = []
    for i in range(2):
        y, u, v = scenes.test_input(i, IW, IH, noise_seed=40 + i)
        out.append((y, np.ascontiguousarray(np.stack([u, v], -1))))
    return out


@pytest.fixture(scope="module")
def oracle_picture():
    root = S.View(children=[S.Rescaler(child=S.InputStream(i)) for i in range(2)], background_color=(0x20, 0x30, 0x40, 255))
    layouts = S.scene_layouts(root, W, H, [(IW, IH)] * 2)
    nodes = [orc.nv12_to_rgba(y, c, IW, IH) for y, c in _inputs8()]
    want, _ = refpipe.render_yuv420(layouts, nodes, W, H)
    return want


def _render(hip, fmt10, lanes=0, shard=False, frames_n=1):
    """The scene rendered `frames_n` times -> (list of downloaded outputs, kernel launches of the root context per kernel)."""
    from smelter_amd.renderer import Renderer
    root = hip.Context(0)
    extra = [hip.Context(0) for _ in range(lanes + (1 if shard else 0))]
    r = Renderer(root, lanes=extra if lanes else (), shards=extra if shard else ())
    frames = {}
    try:
        for i, (y8, c8) in enumerate(_inputs8()):
            r.register_input(f"in{i}")
            c = r.input_context(f"in{i}") if shard else root
            if fmt10:
                frames[f"in{i}"] = c.frame(hip.FRAME_P010, IW, IH, _planes10(y8.astype(np.uint16) * 4, c8.astype(np.uint16) * 4, True))
            else:
                frames[f"in{i}"] = c.frame(hip.FRAME_NV12, IW, IH, [y8, c8])
        r.update_scene("out", W, H, SCENE)
        before = root.kernel_launches()
        outs = [r.render(0.02 * k, frames)["out"].download() for k in range(frames_n)]
        r.sync()
        ran = {k: n - before[k] for k, n in root.kernel_launches().items()}
        return outs, ran
    finally:
        r.close()
        for f in frames.values():
            f.destroy()
        for c in [root] + extra:
            c.close()


def _within_1_lsb(got, want):
    for g, w_ in zip(got, want):
        assert refpipe.max_diff(g, w_) <= 1, refpipe.max_diff(g, w_)


def test_renderer_with_p010_inputs_draws_the_nv12_picture(hip, oracle_picture):
    (nv12,), ran8 = _render(hip, False)
    (p010,), ran10 = _render(hip, True)
    _within_1_lsb(p010, oracle_picture)
    _within_1_lsb(nv12, oracle_picture)
    assert ran10["frame_to_rgba_420"] >= 1, ran10  # (the 10-bit inputs went through the block converter)
    if all(ran8[k] == ran10[k] for k in RESAMPLERS):  # the same resampler and compositor kernels: the same node textures in, the same bytes out
        for a, b in zip(p010, nv12):
            assert np.array_equal(a, b)
    assert p010[0].std() > 10


def test_renderer_with_p010_inputs_on_two_lanes(hip, oracle_picture):
    outs, _ = _render(hip, True, lanes=1, frames_n=2)
    (single,), _ = _render(hip, True)
    for out in outs:  # (consecutive frames rotate through the lanes)
        _within_1_lsb(out, oracle_picture)
        for a, b in zip(out, single):
            assert np.array_equal(a, b)


def test_renderer_with_p010_inputs_and_a_shard_is_the_single_context_frame(hip, oracle_picture):
    (sharded,), _ = _render(hip, True, shard=True)
    (single,), _ = _render(hip, True)
    _within_1_lsb(sharded, oracle_picture)
    for a, b in zip(sharded, single):
        assert np.array_equal(a, b)


# ------------------------------------------------------------------------------------------------ input only

def test_10_bit_frames_are_refused_wherever_a_frame_is_an_output(ctx, hip):
    from smelter_amd.renderer import Renderer
    from smelter_amd.scene import SceneError
    node = ctx.surface(16, 8)
    for fmt in (hip.FRAME_P010, hip.FRAME_PLANAR_YUV420P10):
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
            r.update_scene("out", 64, 36, {"type": "view"}, output_format=hip.FRAME_P010)
        assert "input only" in str(e.value)
    finally:
        r.close()


def test_a_p010_frame_whose_uv_plane_is_r16_is_refused(ctx, hip):
    from smelter_amd import _ffi
    w, h = 16, 8
    ys, uv = ctx.surface(w, h, hip.PX_R16), ctx.surface(w // 2, h // 2, hip.PX_R16)
    f = hip.DeviceFrame.__new__(hip.DeviceFrame)
    f.ctx, f.fmt, f.w, f.h = ctx, hip.FRAME_P010, w, h
    f.c = _ffi.Frame()
    f.c.format, f.c.width, f.c.height = hip.FRAME_P010, w, h
    f.c.planes[0], f.c.planes[1] = ys.handle.value, uv.handle.value
    with pytest.raises(hip.SmrError) as e:
        ctx.frame_to_rgba(f)
    assert e.value.code == -1 and "plane 1" in str(e.value)
    ys.destroy(); uv.destroy()
