"""Tiles that grow from nothing, on the device, through smr_render_layouts' per-layout route choice (smelter_amd/csrc/smr_fused.hip) — the
growth paths of tests/small_tiles.py, what tests/test_emu_small_tiles.py runs through the lane emulator for the kernel alone: 1 x 1, 2 x 1,
3 x 2 ... up to 80 x 45 of a 256 x 144 source, the same opening along one axis only, from a ragged 130 x 74 source, under a fractional crop,
and sources at and under the matrix-core kernel's minimum of 8 x 2; from a 4:2:0 frame, an opaque RGBA8 surface and a premultiplied surface.
Every case goes through Context.render_layouts with one 1:1 layout into a poisoned RGBA8 output, the route read from the launch counters.

Each (path, source kind) runs three times: growing on one long-lived context (pass 1), shrinking on the same context (pass 2), in a seeded
shuffled order on a new context (pass 3), each pass into another poison.  A growing tile asks its context for new weight bands on every
frame (get_wave_band keeps 64 and then evicts) and resizes the cached reduced / transposed surfaces of its layout from frame to frame; every
frame of a path holds other texels than its neighbours, so a stale table or texture is a wrong tile in one pass and not in another.

Bars:
  A       pass 1: every byte within 1 LSB of orc.resample of the oracle's node (orc.planar_yuv_to_rgba for frames);
  exact   a constant node gives the oracle's bytes, opaque kinds alpha 255, alpha_0 all zero; no poison left (the passes' poisons differ,
          their tiles must not);
  state   passes 2 and 3 byte-equal to pass 1 and by the same route, case by case; the contexts of uniform, ragged and crop build more than
          64 distinct bands in pass 1 alone (counted from the plans of the cases that took the wave route), so the eviction is reached;
  routes  each case launches exactly one of ingest_wave_rgba, ingest_wave, ingest_valu, resample_general; over the module ingest_wave_rgba
          is reached without box levels and behind a box reduction in either residual order, and so are the pass kernels;
  shares  pooled per (route family, source kind, content class): wave pools by the zoo's bar (B1 at 0.9995, else B2 against the f64
          witness), pools of the pass kernels — k_ingest_resample's tiles with them — at the 0.995 tests/test_gpu_parity.py asks of those
          kernels; every judged pool at least 200 000 bytes.

Measured on an MI355X (gfx950): 4 380 cases a pass (1 734 on 4:2:0 frames, 1 764 on opaque surfaces, 882 with alpha: 289 / 294 / 294
tiles by 6 / 6 / 3 content classes); every bar holds, all three passes agree byte for byte and route for route, no pool needs B2.
  routes (cases by the launch counter's own name, per source kind yuv420 | opaque | alpha):
    ingest_wave_rgba, no box level               348 | 348 | 174
    ingest_wave_rgba behind a box, horizontal    336 | 336 | 168
    ingest_wave_rgba behind a box, vertical      372 | 372 | 186
    ingest_wave                                    0 |   0 |   0
    resample_general                             660 | 708 | 354
    ingest_valu                                   18 |   0 |   0
  No case counts as ingest_wave: the plane-source builds and the fused conversion are opt-in, a 4:2:0 frame is converted exactly into a
  node texture (RGB12 where its width allows, else RGBA8) and resampled from that, which counts as ingest_wave_rgba.
  ingest_valu IS reached by default: a 4:2:0 frame under the wave kernel's 8 x 2 whose plan is two-pass, horizontal first, without a box
  level — 4 x 2 -> 1 x 1, 4 x 2 -> 5 x 3 and 2 x 2 -> 1 x 1 here — goes to k_ingest_resample (smr_render_layouts' can_fuse_ingest branch); its
  tiles hold bar A and the exact properties like every other, and are pooled with the pass kernels'.  The pass kernels take the rest of
  what the wave kernel refuses: reduced sources under 8 x 2 (transposed for a vertical first pass), every single-axis plan behind a box
  level (open_h up to 48 columns, open_v up to 35 rows), and 4 x 2 -> 17 x 9 of a frame (can_fuse_ingest refuses its vertical enlargement
  by 4.5).  open_v's 36 rows, a height-only shrink by 4 without a level, run the single-axis build one tile per wave.  The tiles on the wave
  route are exactly small_tiles.wave_cases (asserted): the pools tests/test_small_tiles_reference.py holds the witness on.
  distinct bands built on one context in pass 1: uniform 157, ragged 72, crop 72 (each above the 64 a context keeps: asserted); open_h 3,
  open_v 4, tiny_src 17 (few wave cases: these contexts never evict, their state bar rests on the resized surfaces alone).
  shares (bytes equal to the oracle's; differing bytes in brackets), wave pools of 549 822 colour bytes / 733 096 bytes with alpha:
    yuv420  constants 1.000000; white_impulses 0.999989 (6), bilevel_blocks 0.999984 (9), noise_0_8 0.999984 (9), white_noise 0.999984 (9);
    opaque  constants 1.000000; white_impulses 0.999989 (6), bilevel_blocks 0.999985 (8), noise_0_8 0.999984 (9), white_noise 0.999973 (15);
    alpha   alpha_0 1.000000; alpha_blocks 0.999929 (52), noise_under_noise 0.999975 (18);
  pools of the pass kernels (998 400 colour bytes of frames, 999 798 of opaque surfaces, 1 333 064 bytes with alpha):
    yuv420  constants, white_impulses, noise_0_8 1.000000; bilevel_blocks 0.999988 (12), white_noise 0.999994 (6);
    opaque  constants, white_impulses 1.000000; bilevel_blocks 0.999996 (4), noise_0_8 0.999999 (1), white_noise 0.999998 (2);
    alpha   alpha_0 1.000000; alpha_blocks 0.999998 (3), noise_under_noise 0.999997 (4).
A share below these on a later run is a drift worth reading, even where the floors still hold.  The slowest test takes 1.7 s."""
import numpy as np
import pytest

from oracle import oracle as orc
from oracle.oracle import Layout
from tests import resample_zoo as zoo
from tests import small_tiles as st

pytestmark = pytest.mark.gpu

ROUTES = ("ingest_wave_rgba", "ingest_wave", "ingest_valu", "resample_general")
POISON = {1: 0xA5, 2: 0x3C, 3: 0x5A}
GENERAL_FLOOR = 0.995   # tests/test_gpu_parity.py::test_resample_vs_oracle
EVICTING = ("uniform", "ragged", "crop")   # the paths whose wave cases alone need more than the 64 bands a context keeps
CASES = [(p, k) for p in st.PATHS for k in st.KINDS]


@pytest.fixture(scope="module")
def hip():
    from smelter_amd import hip as h
    orc.build()
    yield h
    for r in _RUNS.values():
        r.close()


class Run:
    """One (path, source kind): its cases in growing order, the oracle's tiles (computed once), the tiles and routes of each pass."""

    def __init__(self, hip, path, kind):
        self.hip, self.path, self.kind = hip, path, kind
        self.cases = [(g, n) for g in st.cases(path, kind) for n in st.CONTENTS[kind]]
        self.want = {}
        self.got = {1: {}, 2: {}, 3: {}}
        self.route = {1: {}, 2: {}, 3: {}}
        self.ctx = None

    def close(self):
        if self.ctx is not None:
            self.ctx.close()
            self.ctx = None

    def _source(self, ctx, geo, name):
        node, planes = st.node_of(geo, self.kind, name)
        if planes is not None:
            return ctx.frame(self.hip.FRAME_PLANAR_YUV420, geo.src[0], geo.src[1], list(planes)), node
        surf = ctx.surface_from(node)
        surf.opaque = self.kind == "opaque"   # SMR_SOURCE_OPAQUE_SURFACE
        return surf, node

    def _pass(self, ctx, n, order):
        for geo, name in order:
            dw, dh = geo.dst
            src, node = self._source(ctx, geo, name)
            out = ctx.surface(dw, dh).upload(np.full((dh, dw, 4), POISON[n], np.uint8))
            before = ctx.kernel_launches()
            ctx.render_layouts([Layout(top=0, left=0, width=dw, height=dh, type=0, source_index=0, crop=geo.crop)], [src], dw, dh, out_rgba=out)
            self.got[n][geo.name, name] = out.download()
            after = ctx.kernel_launches()
            self.route[n][geo.name, name] = tuple(after[k] - before[k] for k in ROUTES)
            out.destroy()
            src.destroy()
            if n == 1:
                k, want = orc.resample(node, geo.crop, dw, dh)
                assert k == geo.plan().kind
                self.want[geo.name, name] = want

    def growing(self):
        if not self.got[1]:
            self.ctx = self.hip.Context(0)
            self._pass(self.ctx, 1, self.cases)
        return self

    def again(self):
        self.growing()
        if not self.got[3]:
            self._pass(self.ctx, 2, self.cases[::-1])
            self.close()
            order = [self.cases[i] for i in np.random.default_rng([7, CASES.index((self.path, self.kind))]).permutation(len(self.cases))]
            fresh = self.hip.Context(0)
            try:
                self._pass(fresh, 3, order)
            finally:
                fresh.close()
        return self

    def route_name(self, geo, name):
        """The launch counter's own name — "ingest_wave_rgba" | "ingest_wave" (each plain, or "... box h" / "... box v" behind a box reduction,
        by the residual's first pass) | "ingest_valu" | "resample_general" —, None when the case launched none or several of the four."""
        ran = self.route[1][geo.name, name]
        if sum(ran) != 1 or max(ran) != 1:
            return None
        which = ROUTES[ran.index(1)]
        plan = geo.plan()
        if which.startswith("ingest_wave") and tuple(plan.levels) != (0, 0):
            which += " box " + "hv"[plan.axis[0]]
        return which


_RUNS = {}


def run(hip, path, kind):
    if (path, kind) not in _RUNS:
        _RUNS[path, kind] = Run(hip, path, kind)
    return _RUNS[path, kind]


def bands_of(geo):
    """The (scale, offset, n_dst, n_src, axis) bands a wave-route case asks its context for, as make_wave_job_rgba keys them (a plan whose
    first pass is vertical runs transposed; a single-axis plan brings a scale-1 band that carries the perpendicular offset)."""
    plan = geo.plan()
    (rw, rh), (dw, dh) = plan.reduced, geo.dst
    if plan.axis[0] == 1:
        rw, rh, dw, dh = rh, rw, dh, dw
    first = (plan.scale[0], plan.offset[0], dw, rw, "h")
    second = (1.0, float(plan.perp_offset[0]), dh, rh, "v") if plan.kind == 1 else (plan.scale[1], plan.offset[1], dh, rh, "v")
    return {first, second}


@pytest.mark.parametrize("path,kind", CASES, ids=[f"{p}-{k}" for p, k in CASES])
def test_growing_tile(hip, path, kind):
    """Pass 1: bar A, the exact properties and one route per case; prints the route table of this path and source kind."""
    r = run(hip, path, kind).growing()
    bad, bands, on_wave = [], set(), set()
    for geo in st.cases(path, kind):
        routes = {r.route_name(geo, n) for n in st.CONTENTS[kind]}
        print(f"{path:>8} {kind:>6} {geo.src[0]:>3}x{geo.src[1]:<3} -> {geo.dst[0]:>3}x{geo.dst[1]:<3} {st.plan_text(geo.plan()):<58} {sorted(map(str, routes))}")
        if len(routes) != 1 or None in routes:
            bad.append(f"{geo.name}: not one route for every content: {[r.route[1][geo.name, n] for n in st.CONTENTS[kind]]} of {ROUTES}")
        elif next(iter(routes)).startswith("ingest_wave"):
            bands |= bands_of(geo)
            on_wave.add(geo.name)
        for name in st.CONTENTS[kind]:
            node, _ = st.node_of(geo, kind, name)
            got, want = r.got[1][geo.name, name], r.want[geo.name, name]
            bad += [f"{geo.name} ({st.plan_text(geo.plan())}, {r.route_name(geo, name)}) {b}" for b in zoo.check_case(got, want, node, name, kind != "alpha")]
    print(f"{path} {kind}: {len(bands)} distinct bands on this context in pass 1")
    # (what tests/test_small_tiles_reference.py holds the witness on, without a device, are exactly the wave pools' tiles)
    assert on_wave == {g.name for g in st.wave_cases(path, kind)}, on_wave ^ {g.name for g in st.wave_cases(path, kind)}
    if path in EVICTING:
        assert len(bands) > 64, f"{path} {kind}: only {len(bands)} bands: the context never evicts one"
    assert not bad, "\n".join(bad[:40])


@pytest.mark.parametrize("path,kind", CASES, ids=[f"{p}-{k}" for p, k in CASES])
def test_shrinking_and_shuffled_passes_repeat_the_growing_one(hip, path, kind):
    """Passes 2 (same context, shrinking) and 3 (new context, shuffled) give pass 1's bytes by pass 1's route, case by case."""
    r = run(hip, path, kind).again()
    bad = []
    for geo, name in r.cases:
        key = geo.name, name
        for n in (2, 3):
            if r.route[n][key] != r.route[1][key]:
                bad.append(f"{geo.name} {name}: pass {n} ran {r.route[n][key]}, pass 1 {r.route[1][key]} of {ROUTES}")
            if not np.array_equal(r.got[n][key], r.got[1][key]):
                d = r.got[n][key] != r.got[1][key]
                left = int((r.got[n][key][d] == POISON[n]).sum())
                bad.append(f"{geo.name} {name} ({st.plan_text(geo.plan())}, {r.route_name(geo, name)}): pass {n} differs from pass 1 in {int(d.sum())} bytes ({left} of them its poison)")
    assert not bad, "\n".join(bad[:40])


def test_every_default_route_is_reached(hip):
    """Over the whole module: ingest_wave_rgba itself without box levels, behind a box reduction with the horizontal and with the vertical
    pass first, and the pass kernels; the count of cases per counter is printed."""
    count = {}
    for path, kind in CASES:
        r = run(hip, path, kind).growing()
        for geo, name in r.cases:
            key = (kind, r.route_name(geo, name))
            count[key] = count.get(key, 0) + 1
    for key in sorted(count, key=str):
        print(f"{key[0]:>6} {str(key[1]):<22} {count[key]:>5} cases")
    reached = {route for _, route in count}
    assert {"ingest_wave_rgba", "ingest_wave_rgba box h", "ingest_wave_rgba box v", "resample_general"} <= reached, reached


@pytest.mark.parametrize("kind", st.KINDS)
def test_pooled_shares(hip, kind):
    """Per (route family, content class) of one source kind, over every path: wave pools by the zoo's bar, pass-kernel pools at 0.995."""
    pools = {}
    for path in st.PATHS:
        r = run(hip, path, kind).growing()
        for geo, name in r.cases:
            route = r.route_name(geo, name)
            family = "wave" if str(route).startswith("ingest_wave") else "passes"
            pool = pools.setdefault((family, name), st.Pool((f"{family}/{kind}", name), 4 if kind == "alpha" else 3, kind))
            pool.add(r.got[1][geo.name, name], r.want[geo.name, name], geo, geo.crop)
    bad = []
    for (family, name), pool in sorted(pools.items()):
        if family == "wave":
            ok, line = pool.verdict()
        else:
            line = f"{pool.key[0]:>6} {pool.key[1]:<20} {pool.total:>8} bytes, {pool.differing:>5} differ, share {pool.share:.6f}"
            ok = pool.total >= zoo.POOL_MIN and pool.share >= GENERAL_FLOOR
            if pool.total < zoo.POOL_MIN:
                line += f": pool below {zoo.POOL_MIN} bytes — lengthen a path that takes this route"
        print(line)
        if not ok:
            bad.append(line)
    assert {f for f, _ in pools} == {"wave", "passes"}
    assert not bad, "\n".join(bad)
