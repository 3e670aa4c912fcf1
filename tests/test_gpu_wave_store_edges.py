"""k_ingest_wave's tile stores at the edges of a destination, on the device: the shapes of tests/test_emu_wave_store_edges.py through
smr_ingest_resample into destinations in caller memory (tests/wrapped.py: tight, slack, a window inside a wider buffer — 16-byte pitches, which
the matrix-core route demands of a tile).  A tile that lies wholly inside the destination leaves by the straight-line path (one 16-byte store per
lane, chosen once for the wave), a tile the right or bottom edge cuts by the per-lane path with its ragged tail; per case and source format

  1. nothing outside the w x h texels was written, in any geometry, and the texels equal the same call into a surface of the library;
  2. the texels are within 1 LSB of the oracle's resample of the oracle's node texture;
  3. they are byte-equal to the top-left w x h texels of the same job (same frame, scales and offsets) rendered 32 columns wider and 16 rows
     taller, where the small job's edge tiles are interior tiles (why the sums are the same: tests/test_emu_wave_store_edges.py);
  4. every one of those calls launched k_ingest_wave (smr_debug_kernel_launches) and none the pass kernels or the f32 ingest kernel.

420: the default route of 4:2:0 frames (RGB12 node); 444: the RGBA8 node route.  The exact fraction is pooled over all cases of a format against
the floor tests/test_gpu_write_footprint.py asks of smr_ingest_resample (0.995: the smallest tile has 1 856 bytes)."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import refpipe
from tests.wrapped import GEOMETRIES, WrappedSurface

pytestmark = pytest.mark.gpu

WIDTHS = (29, 31, 32, 33, 35, 48, 61)
HEIGHTS = (16, 17, 31)
GROW = (32, 16)
FLOOR = 0.995
SOURCES = {1.5: (144, 72), 3.0: (196, 144)}  # holds the crop of the largest grown job; widths are multiples of 4 (RGB12 groups)
CASES_3X = [(33, 31)]                        # the <8, 3> class
FORMATS = ("420", "444")


@pytest.fixture(scope="module")
def hip():
    from smelter_amd import hip as h
    return h


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


@pytest.fixture(scope="module")
def ctx(hip):
    c = hip.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def sources(ctx, hip):
    """(format, scale) -> (frame on the device, the oracle's node texture): white noise, made once"""
    out = {}
    for name in FORMATS:
        ov = orc.YUV444 if name == "444" else orc.YUV420
        for scale, (sw, sh) in SOURCES.items():
            rng = np.random.default_rng(sw * 3 + sh + (444 if name == "444" else 420))
            ch, cw = orc.chroma_shape(sw, sh, ov)
            y, u, v = (rng.integers(0, 256, s, dtype=np.uint8) for s in ((sh, sw), (ch, cw), (ch, cw)))
            frame = ctx.frame(hip.FRAME_PLANAR_YUV444 if name == "444" else hip.FRAME_PLANAR_YUV420, sw, sh, [y, u, v])
            out[name, scale] = (frame, orc.planar_yuv_to_rgba(y, u, v, sw, sh, ov))
    yield out
    for frame, _ in out.values():
        frame.destroy()


_results = {}


def _case(torch, ctx, sources, name, scale, dw, dh):
    """One destination size of one format, computed once -> (texels, the oracle's tile) after asserting 1, 3 and 4."""
    key = (name, scale, dw, dh)
    if key in _results:
        return _results[key]
    frame, node = sources[name, scale]
    sw, sh = SOURCES[scale]
    what = f"ingest_resample {name} x{scale} -> {dw}x{dh}"

    def crop_of(w, h):
        return (0.0, 0.0, scale * w, scale * h)

    plan = orc.resample_plan(sw, sh, crop_of(dw, dh), dw, dh)
    big = orc.resample_plan(sw, sh, crop_of(dw + GROW[0], dh + GROW[1]), dw + GROW[0], dh + GROW[1])
    assert plan.kind == 2 and plan.axis[0] == 0 and plan.levels == (0, 0), plan
    assert (tuple(big.scale), tuple(big.offset)) == (tuple(plan.scale), tuple(plan.offset)), (plan, big)  # the same job, grown
    before = ctx.kernel_launches()
    owned = ctx.surface(dw, dh)
    ctx.ingest_resample(frame, crop_of(dw, dh), owned)
    ref = owned.download()
    owned.destroy()
    for g in GEOMETRIES:
        ws = WrappedSurface(torch, ctx, dw, dh, 0, g, 11 + dw * 131 + dh, 16)
        ctx.ingest_resample(frame, crop_of(dw, dh), ws.surface)
        ctx.sync()
        got = ws.texels(what)
        assert np.array_equal(got, ref), f"{what} [{g}]: {int((got != ref).sum())} texel bytes differ from the result in a surface of the library"
        ws.surface.destroy()
    grown = ctx.surface(dw + GROW[0], dh + GROW[1])
    ctx.ingest_resample(frame, crop_of(dw + GROW[0], dh + GROW[1]), grown)
    cropped = grown.download()[:dh, :dw]
    grown.destroy()
    ran = {k: n - before[k] for k, n in ctx.kernel_launches().items()}
    assert ran["ingest_wave_rgba"] + ran["ingest_wave"] == 2 + len(GEOMETRIES) and ran["resample_general"] == 0 and ran["ingest_valu"] == 0, (what, ran)
    bad = np.argwhere((ref != cropped).any(axis=-1))
    assert bad.size == 0, f"{what}: {len(bad)} texels differ from the grown job's, the first at (row, column) {tuple(bad[0])}"
    _results[key] = (ref, orc.resample(node, crop_of(dw, dh), dw, dh)[1])
    return _results[key]


def _check(got, want, what):
    d = refpipe.max_diff(got, want)
    print(f"{what}: max |diff| {d}, exact {(got == want).mean():.5f} of {got.size}")
    assert d <= 1, f"{what}: max |diff| = {d} (> 1) against the oracle; exact fraction {(got == want).mean():.5f}"
    assert (got[..., 3] == 255).all()


@pytest.mark.parametrize("dh", HEIGHTS)
@pytest.mark.parametrize("dw", WIDTHS)
@pytest.mark.parametrize("name", FORMATS)
def test_edge_tiles_at_scale_1_5(torch, ctx, sources, name, dw, dh):
    """the benchmark's class (<4, 2>); heights of 16 and 17 have pass-2 windows of one k-step and take the generic build (its stores are immediate)"""
    _check(*_case(torch, ctx, sources, name, 1.5, dw, dh), f"{name} x1.5 -> {dw}x{dh}")


@pytest.mark.parametrize("dw,dh", CASES_3X)
@pytest.mark.parametrize("name", FORMATS)
def test_edge_tiles_at_scale_3(torch, ctx, sources, name, dw, dh):
    """the <8, 3> class"""
    _check(*_case(torch, ctx, sources, name, 3.0, dw, dh), f"{name} x3 -> {dw}x{dh}")


@pytest.mark.parametrize("name", FORMATS)
def test_pooled_exact_fraction(torch, ctx, sources, name):
    """over every case of the format (cases another test has computed are not computed again)"""
    eq = n = 0
    for scale, cases in ((1.5, [(w, h) for w in WIDTHS for h in HEIGHTS]), (3.0, CASES_3X)):
        for dw, dh in cases:
            got, want = _case(torch, ctx, sources, name, scale, dw, dh)
            eq += int((got == want).sum())
            n += got.size
    print(f"ingest_resample {name}: pooled exact fraction {eq / n:.5f} over {n} bytes (floor {FLOOR})")
    assert eq / n >= FLOOR, f"ingest_resample {name}: pooled exact fraction {eq / n:.5f} over {n} bytes (< {FLOOR})"
