"""The matrix-core resampler (k_ingest_wave, smelter_amd/csrc/smr_ingest_wave.h) on the device, on the zoo of tests/resample_zoo.py — what
tests/test_emu_resample_zoo.py runs through the lane emulator, whose matrix instruction is a sequential f32 loop and not the hardware's:
constants, impulses, period-2 patterns, bi-level blocks, near-black and near-white noise, white noise, hard alpha edges, on the smallest
geometry of every build (class builds <4, 2>, <8, 2>, <8, 3>, the generic build on ragged tiles, upscale, one tile per wave, vertical-first,
width-only, height-only, crops at whole and fractional texels, box-pre-reduced plans in either pass order), from a 4:2:0 frame (RGB12 node),
an opaque RGBA8 surface, a premultiplied surface with alpha, and NV12 on two geometries.  Every case goes through Context.render_layouts with
one 1:1 layout into a poisoned RGBA8 output; the launch counters must show k_ingest_wave's node-texture route and neither the pass kernels
nor the f32 kernel.

Bars (tests/resample_zoo.py): A — every byte within 1 LSB of orc.resample of the oracle's node; exact — a constant node gives that constant,
opaque sources alpha 255, alpha 0 all zero, a second run into another poison the same bytes; B1 — per (build class, content class), pooled
over all geometries (>= 200 000 bytes), >= 0.9995 of the bytes equal to the oracle's; B2, only where B1 misses — of the disputed bytes the
device has at least a quarter as the f64 witness has them.

Measured on an MI355X (gfx950), 37 pools; A, the exact properties and the route hold on all 41 cases (every constant exact, alpha 0 all zero,
every second run identical), and no pool needs B2:
  rgb12 (4:2:0 frames and NV12, 241 470 colour bytes a pool): 1.000000 on the six constants, the three impulse classes, checker_1, stripes_3
    and bilevel_blocks; noise_0_8 0.999950 (12 bytes), noise_247_255 0.999988 (3), white_noise 0.999963 (9), white_noise_chroma 0.999992 (2);
  rgba8 (opaque surfaces, 206 142 colour bytes a pool): 1.000000 on the constants, the impulse classes, checker_1 and stripes_3; bilevel_blocks
    0.999985 (3), noise_0_8 0.999990 (2), noise_247_255 0.999976 (5), white_noise 0.999985 (3);
  alpha (274 856 bytes a pool): alpha_0, const_alpha_128, white_ramp 1.000000; alpha_blocks 0.999905 (26, 18 of them on the fractional crop
    whose alpha edges meet at exactly 127.5 — the emulator's 18), alpha_0_5 0.999989 (3), noise_under_noise 0.999982 (5).
A share below these on a later run is a drift worth reading, even where the floors still hold.

What this module found when it was written: checker_1 missed B1 on rgb12 and rgba8 (0.997615, 0.997206) — 576 bytes, all on the one-tile
geometry (500 x 96 -> 128 x 48), each off by one code and each as the f64 witness has it.  Pass 1 turns the checkerboard, in 8 of the 128
columns, into 0.5002433, 8.4e-7 from the boundary between two f16 values of the ring between the passes (the f32 oracle and the witness part
on it too: resample_zoo.WITNESS_NOT_HELD).  The lane emulator, which has the host's sinf / cosf as the oracle has, agreed with the oracle —
also with exact products and one rounding inside its matrix instruction — and gave exactly these 576 bytes once ONE sine of lanczos_weights
was moved by one ulp.  The cause was the device library's sinf / cosf in the weight builders; lanczos_weights (smr_resample_dev.h) now
evaluates them in f64 and rounds once, and the pool is at 1.000000 (alpha_blocks went from 52 differing bytes to 26 with it)."""
import numpy as np
import pytest

from oracle import oracle as orc
from oracle.oracle import Layout
from tests import resample_zoo as zoo

pytestmark = pytest.mark.gpu

KINDS = ("yuv420", "opaque", "alpha")
BUILD_CLASS = {"yuv420": "rgb12", "nv12": "rgb12", "opaque": "rgba8", "alpha": "alpha"}
CASES = [(g, k) for g in zoo.GEOMETRIES for k in KINDS] + [(zoo.GEO[n], "nv12") for n in zoo.NV12_GEOMETRIES]


@pytest.fixture(scope="module")
def hip():
    from smelter_amd import hip as h
    orc.build()
    return h


@pytest.fixture(scope="module")
def ctx(hip):
    c = hip.Context(0)
    yield c
    c.close()


def classes_of(kind):
    return {"yuv420": zoo.YUV_CLASSES, "nv12": zoo.YUV_CLASSES, "opaque": zoo.OPAQUE_CLASSES, "alpha": zoo.ALPHA_CLASSES}[kind]


def _source(ctx, hip, geo, kind, name):
    """-> (device source, the oracle's node texture of it)"""
    w, h = geo.src
    if kind in ("yuv420", "nv12"):
        y, u, v = zoo.yuv_planes(geo, name)
        if kind == "nv12":
            uv = np.ascontiguousarray(np.stack([u, v], axis=-1))
            return ctx.frame(hip.FRAME_NV12, w, h, [y, uv]), orc.nv12_to_rgba(y, uv, w, h)
        return ctx.frame(hip.FRAME_PLANAR_YUV420, w, h, [y, u, v]), orc.planar_yuv_to_rgba(y, u, v, w, h)
    node = zoo.opaque_node(geo, name) if kind == "opaque" else zoo.alpha_node(geo, name)
    surf = ctx.surface_from(node)
    surf.opaque = kind == "opaque"   # SMR_SOURCE_OPAQUE_SURFACE
    return surf, node


def _render(ctx, geo, src, poison):
    dw, dh = geo.dst
    out = ctx.surface(dw, dh).upload(np.full((dh, dw, 4), poison, np.uint8))
    before = ctx.kernel_launches()
    ctx.render_layouts([Layout(top=0, left=0, width=dw, height=dh, type=0, source_index=0, crop=geo.crop)], [src], dw, dh, out_rgba=out)
    got = out.download()
    ran = {k: v - before[k] for k, v in ctx.kernel_launches().items()}
    out.destroy()
    return got, ran


_RESULTS = {}


def run(ctx, hip, geo, kind):
    """-> (failures, [(class, got, want, node)]) of one geometry x source kind, rendered once."""
    if (geo.name, kind) not in _RESULTS:
        plan = geo.plan()
        bad, tiles = [], []
        for name in classes_of(kind):
            src, node = _source(ctx, hip, geo, kind, name)
            got, ran = _render(ctx, geo, src, 0xA5)
            again, _ = _render(ctx, geo, src, 0x3C)
            src.destroy()
            if ran["ingest_wave_rgba"] != 1 or ran["resample_general"] or ran["ingest_valu"] or ran["ingest_wave"]:
                bad.append(f"{name}: not the node-texture route of k_ingest_wave: {ran}")
            k, want = orc.resample(node, geo.crop, *geo.dst)
            assert k == plan.kind
            bad += zoo.check_case(got, want, node, name, kind != "alpha", again)
            tiles.append((name, got, want, node))
        _RESULTS[geo.name, kind] = (bad, tiles)
    return _RESULTS[geo.name, kind]


@pytest.mark.parametrize("geo,kind", CASES, ids=[f"{g.name}-{k}" for g, k in CASES])
def test_every_content_class_on_one_geometry_and_source(ctx, hip, geo, kind):
    """Bar A, the exact properties and the route, every content class of one geometry x source kind."""
    bad, tiles = run(ctx, hip, geo, kind)
    for name, got, want, _ in tiles:
        print(f"{geo.name:>14} {kind:>6} {name:<20} {(got != want).sum():>4} of {got.size} bytes differ")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("build", ["rgb12", "rgba8", "alpha"])
def test_pooled_shares(ctx, hip, build):
    """B1, else B2, per (build class, content class) over every geometry; every pool's share is printed."""
    kinds = [k for k in BUILD_CLASS if BUILD_CLASS[k] == build]
    pools = {name: zoo.Pool((build, name), 4 if build == "alpha" else 3) for name in classes_of(kinds[0])}
    for geo, kind in CASES:
        if kind in kinds:
            for name, got, want, node in run(ctx, hip, geo, kind)[1]:
                pools[name].add(got, want, node, geo.crop)
    bad = []
    for pool in pools.values():
        ok, line = pool.verdict()
        print(line)
        if not ok:
            bad.append(line)
    assert not bad, "\n".join(bad)
