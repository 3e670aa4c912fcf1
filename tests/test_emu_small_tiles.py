"""k_ingest_wave (smelter_amd/csrc/smr_ingest_wave.h) on the lane emulator along the growth paths of tests/small_tiles.py: a tile that opens
from 1 x 1, every plan the host sends to the kernel on the way — two-pass plans of either order, behind box levels (6, 6) .. (0, 0) (the
RGBA16F builds on the reduced texture orc.downsample leaves, transposed for a vertical first pass) or none, one tile per wave where a pair's
window is too wide, single-axis plans without a level.  Test infrastructure only; tests/test_gpu_small_tiles.py holds the device, and the
host's route choice around the kernel, to the same bars.

What is left out, and why:
  * single-axis plans behind a box level (all of open_h up to 48 columns, open_v up to 35 rows): the host sends them to the pass kernels
    (smr_render_layouts asks the single-axis builds for levels == (0, 0)), the kernel has no build for them and the emulator's tile of such
    a plan is garbage;
  * reduced sources under the kernel's minimum of 8 x 2 (4 x 3 of uniform's first tile, 3 x 3 / 5 x 3 / 9 x 5 transposed of ragged's, most of
    tiny_src): pass kernels too;
  * open_v at 36 rows, a height-only shrink by 4 without a level: the device runs the single-axis build one tile per wave, a combination
    emulate() has no mode for (small_tiles.EMU_NO_MODE; asserted to be the only such tile);
  * 4:2:0 frames: the default route resamples their node texture, RGB12 where the width allows, and emulate() runs RGB12 only for the zoo's
    class builds; the plane-source builds (opt-in on the device) it has no mode for at all.  The RGBA8 builds stand for them here.

The emulator costs a barrier per source chunk — 15 s and more for one content class over all paths —, so two classes run on every tile
(white_noise on opaque nodes, noise_under_noise on nodes with alpha: the pools), the exact classes (const_5_16_64, const_255_255_255,
alpha_0) on the tiles whose reduced source holds at most 64 x 36 texels, and every other class of small_tiles.CONTENTS (white_impulses,
bilevel_blocks, noise_0_8; alpha_blocks) on those with at most 32 x 18: tiles up to 15 x 8, the sizes no other module reaches.  Every
class pooled over all paths would take 140 s.  The device module runs every class on every tile.

Bars (tests/resample_zoo.py): A and the exact properties on every tile that is run; B1 on the two pools that reach POOL_MIN, and on those
the reference against the f64 witness: at most 2e-4 of the bytes.  The classes that run on small tiles only have a few thousand bytes
each, which cannot carry B1's floor: their counts are printed, not judged.  For every pool the DEVICE module judges by the zoo's bar the
witness condition is asserted in tests/test_small_tiles_reference.py, on the CPU, without the emulator.

Measured (emulator: a sequential f32 sum inside the matrix instruction): 175 tiles reach the kernel (uniform 79, open_h 2, open_v 2,
ragged 38, crop 44, tiny_src 10);
  opaque white_noise       522 174 colour bytes, 15 differ (share 0.999971), the oracle off the witness in 1.26e-4;
  alpha  noise_under_noise 696 232 bytes, 16 differ (share 0.999977), the oracle off the witness in 9.34e-5;
  constants on 65 tiles (22 908 colour bytes, alpha_0 30 544 bytes): exact; white_impulses, bilevel_blocks, noise_0_8 on 35 tiles (4 467
  colour bytes): 0 differ; alpha_blocks on 35 tiles (5 956 bytes): 7 differ; every byte within 1 LSB.
  The module takes 40 .. 66 s on eight cores (the emulator is bound by its barriers, and so by what else the machine does), 26 .. 39 s of
  them on uniform."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import resample_zoo as zoo
from tests import small_tiles as st
from tests.emu_wave_resample import emulate, load

KINDS = ("opaque", "alpha")
POOLED = {"opaque": "white_noise", "alpha": "noise_under_noise"}   # the classes that run on every tile
EXACT = ("const_5_16_64", "const_255_255_255", "alpha_0")
CHEAP = {True: 64 * 36, False: 32 * 18}   # reduced texels up to which the exact classes (True) and the other classes run


@pytest.fixture(scope="module")
def emu():
    h = load()
    if h is None:
        pytest.skip("no clang++ to build the emulator with")
    return h


_RESULTS = {}


def run(emu, path, kind):
    """-> (failures, [(geo, class, got, want, node)], [names of the tiles the kernel refused]) of one path x source kind, computed once."""
    if (path, kind) not in _RESULTS:
        bad, tiles, refused = [], [], []
        for geo in st.cases(path, kind):
            plan = geo.plan()
            if st.wave_shape(plan) is None:
                continue
            texels = plan.reduced[0] * plan.reduced[1]
            for name in [POOLED[kind]] + [n for n in st.CONTENTS[kind] if n != POOLED[kind] and texels <= CHEAP[n in EXACT]]:
                node, _ = st.node_of(geo, kind, name)
                got = emulate(emu, geo, plan, node, kind == "alpha", refusal=True)
                if got is None:   # windows too wide for the builds the emulator's entry point knows (small_tiles.EMU_NO_MODE)
                    refused.append(geo.name)
                    break
                k, want = orc.resample(node, geo.crop, *geo.dst)
                assert k == plan.kind
                bad += [f"{geo.name} ({st.plan_text(plan)}) {b}" for b in zoo.check_case(got, want, node, name, kind != "alpha")]
                tiles.append((geo, name, got, want, node))
        _RESULTS[path, kind] = (bad, tiles, refused)
    return _RESULTS[path, kind]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("path", list(st.PATHS))
def test_emulated_kernel_along_a_growth_path(emu, path, kind):
    """Bar A and the exact properties on every tile of one path x source kind that the host sends to the kernel; the one tile the
    emulator has no mode for is the one small_tiles.EMU_NO_MODE names."""
    bad, tiles, refused = run(emu, path, kind)
    for geo, name, got, want, _ in tiles:
        print(f"{geo.name:>28} {kind:>6} {name:<18} {(got != want).sum():>3} of {got.size} bytes differ   {st.plan_text(geo.plan())}")
    print(f"{path} {kind}: {len({g.name for g, *_ in tiles})} tiles through the kernel, refused by its window limits: {refused}")
    on_path = {g.name for g in st.PATHS[path]}
    assert set(refused) == on_path & st.EMU_NO_MODE
    assert {g.name for g, *_ in tiles} == {g.name for g in st.wave_cases(path, kind)} - st.EMU_NO_MODE
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("kind", KINDS)
def test_pooled_shares_and_the_witness(emu, kind):
    """B1 per content class, pooled over all paths, for the two classes that run on every tile — the zoo's verdict on a pool of at least
    POOL_MIN bytes — and the reference against the witness on those pools: at most 2e-4 of the bytes.  The other classes ran on the small
    tiles alone; their counts are printed and not judged: a share of a few thousand bytes cannot carry the floor (one boundary value copied
    seven times is 1.2e-3 of alpha_blocks' 5 956 bytes here and 1e-5 of its pool on the device, where every class has a full pool)."""
    pools = {name: zoo.Pool((kind, name), 4 if kind == "alpha" else 3) for name in st.CONTENTS[kind]}
    for path in st.PATHS:
        for geo, cls, got, want, node in run(emu, path, kind)[1]:
            pools[cls].add(got, want, node, geo.crop)
    for name, pool in pools.items():
        if name != POOLED[kind]:
            assert pool.items, name
            print(f"{kind:>6} {name:<20} {pool.total:>8} bytes on {len(pool.items)} small tiles, {pool.differing:>5} differ (bar A and the exact properties only)")
    pool = pools[POOLED[kind]]
    ok, line = pool.verdict()
    ow = pool.oracle_against_witness()
    print(line + f"; {len(pool.items)} tiles; oracle off the witness in {ow:.2e}")
    assert ok and pool.share >= zoo.FLOOR, line   # (B1 alone here: the emulator's matrix instruction adds in the oracle's order)
    assert ow <= zoo.WITNESS_MAX_DIFF or POOLED[kind] in zoo.WITNESS_NOT_HELD, f"{pool.key}: the oracle differs from the witness in {ow:.2e} of the bytes"


def test_the_paths_cross_what_they_are_for():
    """The sweep itself: every plan shape the kernel has a build for is on a path, at box levels from (6, 6) down, and the shapes it has none
    for are there too (so that the device module meets the host's other routes)."""
    orc.build()
    seen = set()
    for path, geos in st.PATHS.items():
        for geo in geos:
            plan = geo.plan()
            seen.add((st.wave_shape(plan), "hv"[plan.axis[0]], tuple(plan.levels) != (0, 0)))
    for want in [("two", "h", False), ("two", "v", False), ("two", "h", True), ("two", "v", True), ("single", "h", False), ("single", "v", False),
                 (None, "h", True), (None, "v", True), (None, "h", False), (None, "v", False)]:
        assert want in seen, want
    levels = {tuple(g.plan().levels) for g in st.PATHS["uniform"]}
    assert {(6, 6), (5, 5), (4, 4), (3, 3), (2, 2), (1, 1), (0, 0)} <= levels
