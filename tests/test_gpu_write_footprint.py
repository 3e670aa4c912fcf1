"""The WRITE half of smr_surface_wrap's contract (include/smr.h) on the device: of a surface it does not own the library writes the w x h
texels and no other byte.  The entry points that write a surface or a frame (all but smr_gather_tiles, which the sharded compositor
uses between tiles the library allocated, and the renderer, which owns its outputs) store into destinations in caller memory (tests/wrapped.py:
seeded random bytes all round, three geometries — tight, slack, a window inside a buffer three times as wide) at the smallest shapes that
put a grid's last group one texel past a block.  The block sizes are the sources' as they are now: 4 pixels per thread and 256 threads
per row block (smr_convert.hip), 4 x 2 blocks in 64 x 4 thread groups (k_yuv_to_rgba_batch, k_rgba_to_planes), 64 x 4 tiles
(smr_resample.hip, k_blit_glyphs, k_gauss_axis's row pass), 32 x 8 tiles (k_apply_layouts, k_shader_planes), 16-texel tile columns with
4-texel lane groups (k_ingest_wave's store_rows), 128 x 16 tiles of 4 x 2 blocks (k_compose_output).  Each case of a pass asserts

  1. nothing outside the texels was written (the helper names the first touched byte as row / byte in row, or head / tail);
  2. the texels equal, byte for byte, the same call into a surface the library allocated (the same kernel, or a fallback that is
     required to be bit-equal);
  3. the texels are within 1 LSB per channel of the oracle (integer paths: exact), and the share of exactly equal bytes, pooled over a
     pass's cases (a 1 x 1 picture cannot carry a floor of its own), meets the floor tests/test_gpu_parity.py uses for that pass.

Where a pass has no oracle of its own the third point is what the pass defines: zeros (smr_surface_clear), the uploaded bytes (the uploads),
the permuted source (swap_rb), the affine test's model, 1 LSB outside its doubtful pixels (user shaders: no parity floor exists for them, so
no exact fraction is pooled).  A size an entry point refuses is asserted as a refusal; nothing is skipped."""
import numpy as np
import pytest

from oracle import oracle as orc
from oracle.oracle import Glyph, Layout, Mask
from tests import refpipe, scenes
from tests.wrapped import GEOMETRIES, WrappedFrame, WrappedSurface

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from smelter_amd import hip as h
    return h


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


@pytest.fixture(scope="module")
def contexts(hip):
    """srgb -> context: True SMR_MODE_GPU_OPTIMIZED, False SMR_MODE_CPU_OPTIMIZED"""
    out = {True: hip.Context(0), False: hip.Context(0, mode=hip.MODE_CPU_OPTIMIZED)}
    yield out
    for c in out.values():
        c.close()


@pytest.fixture(scope="module")
def ctx(contexts):
    return contexts[True]


class Pool:
    """max |diff| per case, the exact fraction over all bytes of a pass's cases"""

    def __init__(self, name, floor, tol=1):
        self.name, self.floor, self.tol, self.eq, self.n = name, floor, tol, 0, 0

    def add(self, got, want, what, ulp16=False):
        got, want = np.asarray(got), np.asarray(want)
        assert got.shape == want.shape, (what, got.shape, want.shape)
        if ulp16:  # RGBA16F: distance of the bit patterns (the bar of test_single_passes_and_downsample)
            got, want = got.view(np.int16).astype(np.int32), want.view(np.int16).astype(np.int32)
        d = refpipe.max_diff(got, want)
        print(f"{self.name} {what}: max |diff| {d}, exact {(got == want).mean():.5f} of {got.size}")
        assert d <= self.tol, f"{self.name} {what}: max |diff| = {d} (> {self.tol}) against the oracle; exact fraction {(got == want).mean():.5f}"
        self.eq += int((got == want).sum())
        self.n += got.size

    def finish(self):
        assert self.n, f"{self.name}: no case ran"
        frac = self.eq / self.n
        print(f"{self.name}: pooled exact fraction {frac:.5f} over {self.n} bytes (floor {self.floor})")
        assert frac >= self.floor, f"{self.name}: pooled exact fraction {frac:.5f} over {self.n} bytes (< {self.floor})"


def _rgba(rng, w, h, premultiplied=True, opaque=False):
    """white noise; a forced share of alpha 0 and 255; RGB premultiplied where the pass expects it"""
    a = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    pick = rng.integers(0, 4, (h, w))
    a[..., 3][pick == 0] = 0
    a[..., 3][pick == 1] = 255
    if opaque:
        a[..., 3] = 255
    if premultiplied:
        a[..., :3] = (a[..., :3].astype(np.uint16) * a[..., 3:4] // 255).astype(np.uint8)
    return a


def _into_surface(torch, c, w, h, call, what, fmt=0, align=4, seed=1):
    """call(dst) into a surface of the library and into the three wrapped geometries -> the owned result, after asserting 1 and 2"""
    owned = c.surface(w, h, fmt)
    call(owned)
    ref = owned.download()
    owned.destroy()
    for g in GEOMETRIES:
        ws = WrappedSurface(torch, c, w, h, fmt, g, seed + w * 131 + h, align)
        call(ws.surface)
        c.sync()
        got = ws.texels(what)
        assert np.array_equal(got, ref), f"{what} [{g} {w}x{h}]: {int((got != ref).sum())} texel bytes differ from the result in a surface of the library"
        ws.surface.destroy()
    return ref


def _into_frame(torch, c, hip, fmt, w, h, call, what, align=4, seed=1):
    owned = c.frame(fmt, w, h)
    call(owned)
    ref = owned.download()
    owned.destroy()
    for g in GEOMETRIES:
        wf = WrappedFrame(torch, c, fmt, w, h, g, seed + w * 131 + h, align)
        call(wf.frame)
        c.sync()
        got = wf.planes(what)
        for i, (a, b) in enumerate(zip(got, ref)):
            assert np.array_equal(a, b), f"{what} [{g} {w}x{h}] plane {i}: {int((a != b).sum())} bytes differ from the result in a frame of the library"
        for sfc in wf.frame.surfaces:  # (the wrappers: the planes are the test's)
            sfc.destroy()
    return ref


# ------------------------------------------------------------------ smr_surface_clear, the uploads
@pytest.mark.parametrize("fmt_name", ["rgba8", "rgba16f", "r8"])
def test_surface_clear_of_a_wrapped_surface(torch, ctx, hip, fmt_name):
    """zeroes the texels — not the rows out to the pitch, which in a window are the neighbours' pixels"""
    fmt = {"rgba8": hip.PX_RGBA8, "rgba16f": hip.PX_RGBA16F, "r8": hip.PX_R8}[fmt_name]
    for w, h in [(1, 1), (5, 3), (65, 5)]:
        got = _into_surface(torch, ctx, w, h, lambda d: ctx._check(ctx.lib.smr_surface_clear(ctx.handle, d.handle)), f"surface_clear {fmt_name}", fmt=fmt)
        assert not got.any(), f"surface_clear {fmt_name} {w}x{h}: {int(np.count_nonzero(got))} texel values are not zero"  # exact: a fill


def test_uploads_into_wrapped_destinations(torch, ctx, hip):
    """smr_surface_upload, smr_frame_upload, smr_frame_upload_async: row-bounded copies, one size per plane layout"""
    rng = np.random.default_rng(3)
    for fmt, (w, h) in [(hip.PX_RGBA8, (5, 3)), (hip.PX_R8, (37, 5)), (hip.PX_RGBA16F, (3, 2))]:
        probe = hip.Surface(ctx, None, w, h, fmt)
        shape, dt = probe._shape_dtype()
        data = rng.integers(0, 256 if dt == np.uint8 else 65536, shape).astype(dt)
        got = _into_surface(torch, ctx, w, h, lambda d: d.upload(data), "surface_upload", fmt=fmt)
        assert np.array_equal(got, data), f"surface_upload fmt {fmt} {w}x{h}"

    def upload_async(f, planes):
        pinned = f.pinned_planes()
        for dst, src in zip(pinned, planes):
            dst[...] = src
        f.upload_async(pinned)
        ctx.sync()

    for fmt, (w, h) in [(hip.FRAME_PLANAR_YUV420, (6, 4)), (hip.FRAME_NV12, (6, 4)), (hip.FRAME_PLANAR_YUV444, (5, 3)), (hip.FRAME_BGRA, (5, 3))]:
        probe = hip.DeviceFrame.__new__(hip.DeviceFrame)
        probe.fmt, probe.w, probe.h = fmt, w, h
        planes = [rng.integers(0, 256, sh, dtype=np.uint8) for sh in probe.plane_shapes()]
        for what, call in [("frame_upload", lambda f: f.upload(planes)), ("frame_upload_async", lambda f: upload_async(f, planes))]:
            got = _into_frame(torch, ctx, hip, fmt, w, h, call, what)
            assert all(np.array_equal(g, p) for g, p in zip(got, planes)), f"{what} fmt {fmt} {w}x{h}"


# ------------------------------------------------------------------ smr_frame_to_rgba
def _frame_and_oracle(c, hip, rng, name, w, h):
    if name in ("420", "j420", "422", "444"):
        ov = {"420": orc.YUV420, "j420": orc.YUVJ420, "422": orc.YUV422, "444": orc.YUV444}[name]
        fmt = {"420": hip.FRAME_PLANAR_YUV420, "j420": hip.FRAME_PLANAR_YUVJ420, "422": hip.FRAME_PLANAR_YUV422, "444": hip.FRAME_PLANAR_YUV444}[name]
        ch, cw = orc.chroma_shape(w, h, ov)
        y, u, v = (rng.integers(0, 256, s, dtype=np.uint8) for s in ((h, w), (max(ch, 1), max(cw, 1)), (max(ch, 1), max(cw, 1))))
        return c.frame(fmt, w, h, [y, u, v]), orc.planar_yuv_to_rgba(y, u, v, w, h, ov)
    if name == "nv12":
        y, uv = rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h // 2, w // 2, 2), dtype=np.uint8)
        return c.frame(hip.FRAME_NV12, w, h, [y, uv]), orc.nv12_to_rgba(y, uv, w, h)
    if name in ("uyvy", "yuyv"):
        data = rng.integers(0, 256, (h, w // 2, 4), dtype=np.uint8)
        return c.frame(hip.FRAME_UYVY422 if name == "uyvy" else hip.FRAME_YUYV422, w, h, [data]), orc.interleaved422_to_rgba(data, w, h, 0 if name == "uyvy" else 1)
    data = _rgba(rng, w, h, premultiplied=False)
    return c.frame(hip.FRAME_BGRA if name == "bgra" else hip.FRAME_ARGB, w, h, [data]), orc.swizzle_to_rgba(data, w, h, 0 if name == "bgra" else 1)


TO_RGBA = {  # k_yuv420_to_rgba from 8 x 2 (4 x 4 blocks), k_yuv_to_rgba_batch / k_yuv_to_rgba / k_swizzle: four pixels per thread, 256 threads
    "420": [(2, 2), (6, 4), (8, 2), (12, 6), (260, 10)], "j420": [(2, 2), (6, 4), (8, 2), (12, 6), (260, 10)], "nv12": [(2, 2), (6, 4), (8, 2), (12, 6), (260, 10)],
    "422": [(2, 3), (10, 3)], "444": [(1, 1), (37, 5)], "uyvy": [(2, 1), (10, 3)], "yuyv": [(2, 1), (10, 3)],
    "bgra": [(1, 1), (5, 3), (257, 2)], "argb": [(1, 1), (5, 3), (257, 2)],
}


@pytest.mark.parametrize("impl", ["auto", "general"])
def test_frame_to_rgba_into_a_wrapped_node(torch, ctx, hip, impl):
    """every input format; the Y'CbCr formats' bytes pooled (floor 0.999: test_planar_yuv_to_rgba, test_interleaved422_to_rgba), the byte permutes exact"""
    pool, exact = Pool(f"frame_to_rgba {impl}", 0.999), Pool(f"frame_to_rgba swizzles {impl}", 1.0, 0)
    ctx.set_convert_impl(hip.CONVERT_GENERAL if impl == "general" else hip.CONVERT_AUTO)
    try:
        for name, sizes in TO_RGBA.items():
            for w, h in sizes:
                rng = np.random.default_rng(w * 977 + h)
                frame, want = _frame_and_oracle(ctx, hip, rng, name, w, h)
                # (tight = 4 w bytes: not a multiple of 16 for every width, where the block kernels' 16-byte stores leave the node to the pass kernels)
                got = _into_surface(torch, ctx, w, h, lambda d: ctx.frame_to_rgba(frame, d), f"frame_to_rgba {name} {impl}")
                (exact if name in ("bgra", "argb") else pool).add(got, want, f"{name} {w}x{h}")
                frame.destroy()
    finally:
        ctx.set_convert_impl(hip.CONVERT_AUTO)
    pool.finish()
    exact.finish()


@pytest.mark.parametrize("srgb", [True, False])
def test_premultiply_into_a_wrapped_surface(torch, contexts, srgb):
    c = contexts[srgb]
    add, rem = Pool(f"add premult srgb={srgb}", 0.999), Pool(f"remove premult srgb={srgb}", 0.999)  # (test_premultiply)
    for w, h in [(1, 1), (65, 5), (257, 3)]:  # k_premult: a pixel per thread, 256 per block
        data = _rgba(np.random.default_rng(w + h), w, h, premultiplied=False)
        src = c.surface_from(data)
        add.add(_into_surface(torch, c, w, h, lambda d: c.add_premultiplied_alpha(src, d), "add_premultiplied_alpha"), orc.add_premultiplied_alpha(data, srgb), f"{w}x{h}")
        rem.add(_into_surface(torch, c, w, h, lambda d: c.remove_premultiplied_alpha(src, d), "remove_premultiplied_alpha"), orc.remove_premultiplied_alpha(data), f"{w}x{h}")
        src.destroy()
    add.finish()
    rem.finish()


# ------------------------------------------------------------------ smr_rgba_to_frame, smr_frame_fill_black
TO_FRAME = {  # k_rgba_to_planes: 4 x 2 blocks, 64 x 4 of them per workgroup (even sizes); k_rgba_to_y + k_rgba_to_chroma (odd sizes, SMR_CONVERT_GENERAL)
    "420": [(2, 2), (6, 4), (258, 10), (37, 21), (5, 3)], "nv12": [(2, 2), (6, 4), (258, 10), (37, 21), (5, 3)],
    "422": [(2, 1), (6, 3), (37, 4)], "444": [(1, 1), (5, 3), (259, 2)],
}


@pytest.mark.parametrize("impl", ["auto", "general"])
def test_rgba_to_frame_into_a_wrapped_frame(torch, ctx, hip, impl):
    pool = Pool(f"rgba_to_frame {impl}", 0.999)  # (test_rgba_to_frame)
    ctx.set_convert_impl(hip.CONVERT_GENERAL if impl == "general" else hip.CONVERT_AUTO)
    try:
        for name, sizes in TO_FRAME.items():
            fmt = {"420": hip.FRAME_PLANAR_YUV420, "422": hip.FRAME_PLANAR_YUV422, "444": hip.FRAME_PLANAR_YUV444, "nv12": hip.FRAME_NV12}[name]
            for w, h in sizes:
                rgba = _rgba(np.random.default_rng(w * 31 + h), w, h)
                node = ctx.surface_from(rgba)
                got = _into_frame(torch, ctx, hip, fmt, w, h, lambda f: ctx.rgba_to_frame(node, fmt, f), f"rgba_to_frame {name} {impl}")
                want = orc.rgba_to_nv12(rgba) if name == "nv12" else orc.rgba_to_planar_yuv(rgba, {"420": orc.YUV420, "422": orc.YUV422, "444": orc.YUV444}[name])
                for i, (g, w_) in enumerate(zip(got, want)):  # every plane
                    if w_.size:
                        pool.add(g, w_, f"{name} {w}x{h} plane {i}")
                node.destroy()
    finally:
        ctx.set_convert_impl(hip.CONVERT_AUTO)
    pool.finish()


@pytest.mark.parametrize("name", ["420", "j420", "422", "444", "nv12", "rgba"])
def test_fill_black_into_a_wrapped_frame(torch, ctx, hip, name):
    fmt = {"420": hip.FRAME_PLANAR_YUV420, "j420": hip.FRAME_PLANAR_YUVJ420, "422": hip.FRAME_PLANAR_YUV422, "444": hip.FRAME_PLANAR_YUV444,
           "nv12": hip.FRAME_NV12, "rgba": hip.FRAME_RGBA}[name]
    for w, h in [(2, 2), (6, 4), (66, 34), (37, 21)]:  # k_fill_bytes: four bytes per thread
        got = _into_frame(torch, ctx, hip, fmt, w, h, lambda f: ctx.fill_black(f), f"fill_black {name}")
        if name == "rgba":
            assert not got[0].any()
        else:
            assert (got[0] == 16).all() and all((p == 128).all() for p in got[1:]), (name, w, h)  # exact: an integer path


# ------------------------------------------------------------------ resampler
def _launches(c, call):
    before = c.kernel_launches()
    out = call()
    return out, {k: n - before[k] for k, n in c.kernel_launches().items()}


# source 64 x 36, a crop that keeps both scales near 2 with the horizontal one the larger (a horizontal-first two-pass plan inside the
# matrix-core kernel's windows): tile widths 17, 18, 19 = store_rows' tail lengths 1, 2, 3 behind a 16-texel tile column, 33 = one texel
# past two of them; heights that end inside a 16-row tile row
WAVE_TILES = [(17, 15), (18, 17), (19, 16), (33, 9)]


def _wave_crop(dw, dh):
    return (0.0, 0.0, min(64.0, 2.0 * dw), min(36.0, 1.9 * dh)) if dw < 33 else (0.0, 0.0, 64.0, 1.9 * dh)


@pytest.mark.parametrize("name", ["444", "420"])
def test_the_matrix_core_resampler_into_a_wrapped_tile(torch, ctx, hip, name):
    """smr_ingest_resample (smr_resample itself always runs the pass kernels): an opaque frame through its node texture and k_ingest_wave —
    can_fuse_wave_rgba demands 16-byte pitches of the tile, so `tight` rounds the row up to 16 here — straight into the caller's tile.
    444: the RGBA8 node route; 420: the default route of 4:2:0 frames."""
    pool = Pool(f"ingest_resample {name}", 0.995)  # (test_resample_vs_oracle)
    sw, sh = 64, 36
    rng = np.random.default_rng(5)
    ov = orc.YUV444 if name == "444" else orc.YUV420
    ch, cw = orc.chroma_shape(sw, sh, ov)
    y, u, v = (rng.integers(0, 256, s, dtype=np.uint8) for s in ((sh, sw), (ch, cw), (ch, cw)))
    frame = ctx.frame(hip.FRAME_PLANAR_YUV444 if name == "444" else hip.FRAME_PLANAR_YUV420, sw, sh, [y, u, v])
    node = orc.planar_yuv_to_rgba(y, u, v, sw, sh, ov)
    for dw, dh in WAVE_TILES:
        crop = _wave_crop(dw, dh)
        plan = orc.resample_plan(sw, sh, crop, dw, dh)
        assert plan.kind == 2 and plan.axis[0] == 0 and plan.levels == (0, 0), plan
        got, ran = _launches(ctx, lambda: _into_surface(torch, ctx, dw, dh, lambda d: ctx.ingest_resample(frame, crop, d), f"ingest_resample {name}", align=16))
        assert ran["ingest_wave_rgba"] + ran["ingest_wave"] == 1 + len(GEOMETRIES) and ran["resample_general"] == 0 and ran["ingest_valu"] == 0, (dw, dh, ran)
        pool.add(got, orc.resample(node, crop, dw, dh)[1], f"-> {dw}x{dh}")
    pool.finish()


def test_the_batched_matrix_core_resampler_into_wrapped_tiles(torch, ctx, hip):
    """smr_ingest_resample_batch: two 4:2:0 inputs in one launch of k_ingest_wave, each into a caller's tile (16-byte pitches, as above)"""
    pool = Pool("ingest_resample_batch", 0.995)  # (test_resample_vs_oracle)
    sw, sh = 64, 36
    rng = np.random.default_rng(14)
    ch, cw = orc.chroma_shape(sw, sh, orc.YUV420)
    planes = [[rng.integers(0, 256, s, dtype=np.uint8) for s in ((sh, sw), (ch, cw), (ch, cw))] for _ in range(2)]
    frames = [ctx.frame(hip.FRAME_PLANAR_YUV420, sw, sh, p) for p in planes]
    sizes = [(17, 15), (33, 9)]
    crops = [_wave_crop(dw, dh) for dw, dh in sizes]
    owned = [ctx.surface(dw, dh) for dw, dh in sizes]
    assert ctx.ingest_resample_batch(frames, crops, owned) == [2, 2]
    refs = [o.download() for o in owned]
    for g in GEOMETRIES:
        ws = [WrappedSurface(torch, ctx, dw, dh, hip.PX_RGBA8, g, 77 + i, 16) for i, (dw, dh) in enumerate(sizes)]
        _, ran = _launches(ctx, lambda: ctx.ingest_resample_batch(frames, crops, [w.surface for w in ws]))
        ctx.sync()
        assert ran["ingest_wave_rgba"] + ran["ingest_wave"] in (1, 2) and ran["resample_general"] == 0 and ran["ingest_valu"] == 0, (g, ran)  # (a launch per class build)
        for w, ref, (dw, dh) in zip(ws, refs, sizes):
            got = w.texels("ingest_resample_batch")
            assert np.array_equal(got, ref), f"ingest_resample_batch [{g} {dw}x{dh}]: {int((got != ref).sum())} texel bytes differ from the result in a surface of the library"
            w.surface.destroy()
    for p, ref, crop, (dw, dh) in zip(planes, refs, crops, sizes):
        pool.add(ref, orc.resample(orc.planar_yuv_to_rgba(*p, sw, sh, orc.YUV420), crop, dw, dh)[1], f"-> {dw}x{dh}")
    for x in owned + frames:
        x.destroy()
    pool.finish()


def test_the_pass_kernels_resample_into_a_wrapped_destination(torch, ctx, hip):
    """smr_resample (k_downsample / k_downsample_wave, k_resample_pass: 64 x 4 tiles) from a translucent source: two-pass plans to the
    matrix-core cases' sizes, a single-pass plan, a box-pre-reduced plan."""
    pool = Pool("resample", 0.995)  # (test_resample_vs_oracle)
    rng = np.random.default_rng(6)
    src = _rgba(rng, 64, 36)
    s = ctx.surface_from(src)
    cases = [((0.0, 0.0, 64.0, 36.0), dw, dh) for dw, dh in WAVE_TILES] + [((0.0, 0.0, 64.0, 36.0), 33, 36), ((0.0, 0.0, 64.0, 36.0), 65, 5), ((0.0, 0.0, 64.0, 36.0), 1, 1)]
    for crop, dw, dh in cases:
        (kind, got), ran = _launches(ctx, lambda: _kind_and(ctx, torch, s, crop, dw, dh))
        okind, want = orc.resample(src, crop, dw, dh)
        assert kind == okind and kind > 0 and ran["ingest_wave_rgba"] == 0, (dw, dh, kind, okind, ran)
        pool.add(got, want, f"64x36 -> {dw}x{dh} kind {kind}")
    assert orc.resample_plan(64, 36, (0.0, 0.0, 64.0, 36.0), 33, 36).kind == 1  # (the single-pass plan above)
    big = _rgba(rng, 160, 90)
    b = ctx.surface_from(big)
    plan = orc.resample_plan(160, 90, (0.0, 0.0, 160.0, 90.0), 5, 3)
    assert plan.levels[0] > 0 and plan.levels[1] > 0, plan
    kind, got = _kind_and(ctx, torch, b, (0.0, 0.0, 160.0, 90.0), 5, 3)
    pool.add(got, orc.resample(big, (0.0, 0.0, 160.0, 90.0), 5, 3)[1], "160x90 -> 5x3 (box pre-reduced)")
    pool.finish()


def _kind_and(c, torch, s, crop, dw, dh):
    kinds = []
    got = _into_surface(torch, c, dw, dh, lambda d: kinds.append(c.resample(s, crop, d)), "resample")
    assert len(set(kinds)) == 1
    return kinds[0], got


def test_single_passes_and_box_means_into_wrapped_rgba16f(torch, ctx, hip):
    """smr_resample_pass / smr_downsample into RGBA16F destinations (8 bytes per texel): 1 x 1, 65 x 5 (one texel past a 64-wide tile, one row
    past a 4-row one), 3 x 9.  Compared as f16 bit patterns: within 1 — an f32 value on a rounding boundary — as test_single_passes_and_downsample."""
    F16 = hip.PX_RGBA16F
    rng = np.random.default_rng(7)
    src = _rgba(rng, 64, 32)
    s = ctx.surface_from(src)
    passes = Pool("resample_pass", 0.99)
    for dw, dh in [(1, 1), (65, 5), (3, 9)]:
        for axis in (0, 1):
            for scale in (2.3, 0.7):  # (the kernel clamps source coordinates: any destination size is a valid pass)
                got = _into_surface(torch, ctx, dw, dh, lambda d: ctx.resample_pass(s, axis, scale, 0.5, 1, d), "resample_pass", fmt=F16)
                passes.add(got, orc.resample_pass(src, orc.PX_RGBA8_SRGB, axis, scale, 0.5, 1, orc.PX_RGBA16F, dw, dh), f"-> {dw}x{dh} axis {axis} scale {scale}", ulp16=True)
    passes.finish()
    boxes = Pool("downsample", 0.99)
    for (sw, sh), (fx, fy) in [((3, 2), (4, 2)), ((258, 9), (4, 2)), ((10, 17), (4, 2)), ((64, 32), (4, 2)), ((64, 32), (32, 8)), ((33, 9), (32, 8)), ((64, 32), (2, 4))]:
        a = _rgba(rng, sw, sh)
        t = ctx.surface_from(a)
        dw, dh = -(-sw // fx), -(-sh // fy)
        got = _into_surface(torch, ctx, dw, dh, lambda d: ctx.downsample(t, fx, fy, d), "downsample", fmt=F16)
        boxes.add(got, orc.downsample(a, orc.PX_RGBA8_SRGB, fx, fy), f"{sw}x{sh} / {fx}x{fy} -> {dw}x{dh}", ulp16=True)
        t.destroy()
    boxes.finish()


@pytest.mark.parametrize("srgb", [True, False])
def test_rescale_bilinear_into_a_wrapped_surface(torch, contexts, srgb):
    c = contexts[srgb]
    pool = Pool(f"rescale_bilinear srgb={srgb}", 0.99)  # (test_rescale_bilinear)
    rng = np.random.default_rng(8)
    for (sw, sh), (dw, dh) in [((160, 90), (1, 1)), ((160, 90), (65, 5)), ((3, 2), (67, 9)), ((5, 5), (5, 5))]:  # k_rescale_bilinear: 64 x 4 tiles
        src = _rgba(rng, sw, sh)
        s = c.surface_from(src)
        got = _into_surface(torch, c, dw, dh, lambda d: c.rescale_bilinear(s, d), "rescale_bilinear")
        pool.add(got, orc.rescale_bilinear(src, dw, dh, orc.PX_RGBA8_SRGB if srgb else orc.PX_RGBA8_UNORM), f"{sw}x{sh} -> {dw}x{dh}")
        s.destroy()
    pool.finish()


# ------------------------------------------------------------------ compositor, text, shaders
def _small_zoo(W, H):
    """a cut-down _layout_zoo (test_gpu_parity.py): fill, rounded and bordered texture, rotated box with a mask, one layout hanging off every edge"""
    col = lambda c: orc.color_to_shader(c, True)
    m = Mask((2, 2, 2, 2), 1.0, 1.5, W - 3.0, H - 2.0)
    return [
        Layout(0, 0, W, H, type=1, color=col((32, 32, 48, 255))),
        Layout(1, 2, W * 0.6, H * 0.7, type=0, source_index=0, crop=(0, 0, 20, 12), border_radius=(3, 3, 3, 3), border_width=1.0, border_color=col((255, 128, 0, 255))),
        Layout(H * 0.2, W * 0.3, W * 0.5, H * 0.5, type=1, color=col((80, 80, 255, 128)), rotation_degrees=-33.0, masks=[m]),
        Layout(-H * 0.5, -W * 0.5, W * 2.0, H * 2.0, type=1, color=col((255, 255, 0, 60)), border_radius=(4, 4, 4, 4)),  # hangs off every edge
    ]


@pytest.mark.parametrize("srgb", [True, False])
def test_apply_layouts_into_a_wrapped_target(torch, contexts, srgb):
    c = contexts[srgb]
    pool = Pool(f"apply_layouts srgb={srgb}", 0.999)  # (test_apply_layouts_zoo)
    tex = _rgba(np.random.default_rng(9), 20, 12)
    src = c.surface_from(tex)
    for W, H in [(33, 9), (1, 1), (65, 17)]:  # k_apply_layouts: 32 x 8 tiles
        layouts = _small_zoo(W, H)
        got = _into_surface(torch, c, W, H, lambda d: c.apply_layouts(d, layouts, [src]), "apply_layouts")
        pool.add(got, orc.apply_layouts(W, H, layouts, [tex], srgb=srgb), f"{W}x{H}")
    pool.finish()


@pytest.mark.parametrize("srgb", [True, False])
def test_blit_glyphs_into_a_wrapped_target(torch, contexts, srgb):
    c = contexts[srgb]
    # test_blit_glyphs holds glyphs that do not overlap to 0.999 and overlapping ones on a coloured background to 0.995.  The pool mixes both:
    # in 3 x 3 every pixel lies under several clipped glyphs, in 65 x 5 the top- and bottom-clipped ones overlap — so the overlapping bar.
    pool = Pool(f"blit_glyphs srgb={srgb}", 0.995)
    atlas = np.random.default_rng(10).integers(0, 256, (8, 24), dtype=np.uint8)
    bg = orc.color_to_shader((20, 40, 90, 200), srgb)
    for W, H in [(65, 5), (3, 3)]:  # k_blit_glyphs: 64 x 4 tiles
        glyphs = [Glyph(-3, 1, 6, 3, 0, 0, (1.0, 0.2, 0.1, 0.7)), Glyph(W - 2, 0, 6, 4, 6, 0, (0.1, 0.9, 0.3, 1.0)),      # clipped left, right
                  Glyph(1, -2, 5, 4, 12, 0, (0.3, 0.3, 1.0, 0.9)), Glyph(0, H - 2, 6, 5, 18, 1, (1.0, 1.0, 0.2, 0.5)),    # clipped top, bottom
                  Glyph(W + 4, H + 4, 6, 5, 0, 2, (1.0, 0.0, 0.0, 1.0)), Glyph(-20, -20, 6, 5, 0, 2, (1.0, 0.0, 0.0, 1.0))]  # wholly outside
        got = _into_surface(torch, c, W, H, lambda d: c.blit_glyphs(d, bg, glyphs, atlas), "blit_glyphs")
        pool.add(got, orc.blit_glyphs(W, H, bg, glyphs, atlas, srgb=srgb), f"{W}x{H}")
    pool.finish()


def test_gaussian_blur_into_a_wrapped_destination(torch, ctx, hip):
    """row pass k_gauss_axis<64, 4, 0> into the context's scratch, column pass <32, 8, 1> (radius <= 28), <16, 16, 1> (<= 56), <8, 32, 1> into
    the caller's surface: every column-block shape, radii larger than the picture"""
    pool = Pool("gaussian_blur", 0.99)  # (test_gaussian_blur)
    rng = np.random.default_rng(11)
    for w, h in [(65, 5), (9, 33), (1, 1), (17, 17)]:
        src = _rgba(rng, w, h)
        s = ctx.surface_from(src)
        for sigma in (0.0, 1.5, 10.0, 20.0):
            got = _into_surface(torch, ctx, w, h, lambda d: ctx.gaussian_blur(s, sigma, d), f"gaussian_blur sigma {sigma}")
            pool.add(got, orc.gaussian_blur(src, sigma), f"{w}x{h} sigma {sigma}")
        s.destroy()
    pool.finish()


@pytest.mark.parametrize("srgb", [True, False])
def test_builtin_shaders_into_a_wrapped_target(torch, contexts, hip, srgb):
    c = contexts[srgb]
    pool = Pool(f"builtin_shader srgb={srgb}", 0.995)  # (tests/test_gpu_shaders.py: _check)
    rng = np.random.default_rng(12)
    tex = [_rgba(rng, 20, 12), _rgba(rng, 7, 9)]
    srcs = [c.surface_from(t) for t in tex]
    for W, H in [(65, 5), (1, 1)]:  # k_shader_planes
        for sid, n in [(hip.SHADER_LAYOUT_PLANES, 2), (hip.SHADER_GRADIENT, 0)]:
            got = _into_surface(torch, c, W, H, lambda d: c.builtin_shader(sid, srcs[:n], d), f"builtin_shader {sid}")
            pool.add(got, orc.builtin_shader(sid, tex[:n], W, H, srgb=srgb), f"shader {sid} {W}x{H}")
    pool.finish()


@pytest.mark.parametrize("srgb", [True, False])
def test_user_shaders_into_a_wrapped_target(torch, contexts, hip, srgb):
    from tests import test_emu_user_shader_affine as M
    from tests import user_shader_sources as S
    from tests import user_shader_sources_affine as SA
    c = contexts[srgb]
    swap, affine = hip.ShaderProgram(S.ALL["swap_rb"]), hip.ShaderProgram(SA.ALL["affine_param"])
    try:
        for W, H in [(65, 5), (1, 1)]:  # smr_user_shader_kernel
            tex = _rgba(np.random.default_rng(13), W, H)
            s = c.surface_from(tex)
            got = _into_surface(torch, c, W, H, lambda d: c.user_shader(swap, [s], d), "user_shader swap_rb")
            assert np.array_equal(got, tex[..., [2, 1, 0, 3]]), f"swap_rb {W}x{H}: {int((got != tex[..., [2, 1, 0, 3]]).sum())} bytes differ"  # exact: a source of the target's size
            s.destroy()
            srcs = [c.surface_from(t) for t in M.sources()]
            got = _into_surface(torch, c, W, H, lambda d: c.user_shader(affine, srcs, d, M.pack(M.ROTATION)), "user_shader affine")
            # (1 x 1 too: the model does not count its one pixel among those an edge passes close to, so it is compared)
            M.compare(got, *M.model(M.ROTATION, M.sources(), W, H, srgb), f"affine {W}x{H}")
            for t in srcs:
                t.destroy()
    finally:
        swap.close()
        affine.close()


# ------------------------------------------------------------------ smr_render_layouts
RENDER_SIZES = [(2, 2), (6, 4), (130, 18), (258, 34), (132, 16)]  # k_compose_output: 128 x 16 tiles of 4 x 2 blocks; W = 2 mod 4: the `half` stores


def _direct_layer(W, H):
    """-> (source size, crop, layer size) of the `direct` scene's video layer.  From 128 x 16 on the layer is the whole 128 x 16 compositor tiles
    of the output, at the origin, so every one of them is a copy tile of that layer (k_classify_tiles), and its source and crop give what
    smr_render_layouts marks for direct output: a two-pass, horizontal-first plan without box pre-reduction, inside the matrix-core kernel's
    windows (scales 2.25 / 2.19 onto 128 x 16, 1.125 / 1.09 onto 256 x 32).  The pictures below a tile hold no copy tile: the layer is
    resampled into its tile and composited."""
    if W < 128:
        return (64, 36), (0.0, 0.0, 64.0, 36.0), (max(W // 2 * 2 - 2, 2), max(H // 2 * 2 - 2, 2))
    return (288, 36), (0.0, 0.0, 288.0, 35.0), (W // 128 * 128, H // 16 * 16)


def _scene(c, hip, W, H, kind):
    """-> layouts, device sources, oracle nodes.  `scene`: cfg3_scene (tiles with rounded, bordered, shadowed rescalers) on two 16 x 8 inputs;
    `direct`: an aligned opaque layer over a fill — where the resampler's pixels are what the compositor would only copy"""
    (iw, ih), crop, (lw, lh) = ((16, 8), None, (0, 0)) if kind == "scene" else _direct_layer(W, H)
    planes = [scenes.test_input(i, iw, ih, noise_seed=40 + i) for i in range(2)]
    frames = [c.frame(hip.FRAME_PLANAR_YUV420, iw, ih, list(p)) for p in planes]
    nodes = refpipe.nodes_from_yuv420(planes)
    if kind == "scene":
        layouts, _ = scenes.cfg3_scene(iw, ih, W, H, 2, with_text=False)
    else:
        if W >= 128:
            plan = orc.resample_plan(iw, ih, crop, lw, lh)
            assert plan.kind == 2 and plan.axis[0] == 0 and plan.levels == (0, 0), plan
        layouts = [Layout(0, 0, W, H, type=1, color=orc.color_to_shader((20, 40, 60, 255), True)),
                   Layout(0.0, 0.0, float(lw), float(lh), type=0, source_index=0, crop=crop)]
    return layouts, frames, nodes


@pytest.mark.parametrize("kind", ["scene", "direct"])
@pytest.mark.parametrize("out", ["420", "nv12", "rgba"])
def test_render_layouts_into_wrapped_outputs(torch, hip, kind, out):
    """`direct` with a Y'CbCr output: SMR_OPT_DIRECT_OUTPUT is on and, from 128 x 16 on, every render must launch k_ingest_wave with the video
    layer's job marked for direct output (the SMR_KERNEL_INGEST_WAVE_DIRECT counter) — its copy tiles are then stored as Y'CbCr into the
    caller's planes by that kernel, not by the compositor.  RGBA targets, smaller pictures and the `scene` context never take that route."""
    c = hip.Context(0)
    pool = Pool(f"render_layouts {kind} {out}", 0.99)  # (the floor of white-noise content through the matrix-core resampler: test_fused_ingest_input_formats)
    try:
        if kind == "direct":
            c.set_direct_output(True)
        for W, H in RENDER_SIZES + ([(37, 21)] if out == "rgba" else []):
            layouts, frames, nodes = _scene(c, hip, W, H, kind)
            c.profile_reset()
            c.profile_enable(True)
            direct_before = c.kernel_launches()["ingest_wave_direct"]
            if out == "rgba":
                got = [_into_surface(torch, c, W, H, lambda d: c.render_layouts(layouts, frames, W, H, out_rgba=d), f"render_layouts {kind} rgba", align=16)]
            else:
                fmt = hip.FRAME_NV12 if out == "nv12" else hip.FRAME_PLANAR_YUV420
                # (rendered twice per destination: the second call sees the same layout list — a scene at rest, SMR_OPT_DIRECT_OUTPUT's case)
                got = _into_frame(torch, c, hip, fmt, W, H, lambda f: (c.render_layouts(layouts, frames, W, H, out=f), c.render_layouts(layouts, frames, W, H, out=f)),
                                  f"render_layouts {kind} {out}")
            c.sync()
            prof = c.profile_read()
            c.profile_enable(False)
            direct_launches = c.kernel_launches()["ingest_wave_direct"] - direct_before
            if kind == "direct" and out != "rgba" and W >= 128:  # (two renders into the library's frame and into each wrapped one)
                assert direct_launches == 2 * (1 + len(GEOMETRIES)), f"{W}x{H}: {direct_launches} launches with a direct-output job in {2 * (1 + len(GEOMETRIES))} renders"
            else:
                assert direct_launches == 0, (W, H, direct_launches)
            if W % 2 == 0 and H % 2 == 0:
                assert prof["fused_compose_output"][1] >= 1 + len(GEOMETRIES) and prof["layouts"][1] == 0, f"{W}x{H} left the fused compositor: {prof}"
            (wy, wu, wv), rgba = refpipe.render_yuv420(layouts, nodes, W - W % 2, H - H % 2) if out != "rgba" else ((None, None, None), refpipe.layout_node_render(layouts, nodes, W, H))
            want = [rgba] if out == "rgba" else [wy, np.stack([wu, wv], -1)] if out == "nv12" else [wy, wu, wv]
            for i, (g, w_) in enumerate(zip(got, want)):
                pool.add(g, w_, f"{W}x{H} plane {i}")
            for f in frames:
                f.destroy()
    finally:
        c.close()
    pool.finish()
