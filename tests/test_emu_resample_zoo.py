"""k_ingest_wave (smelter_amd/csrc/smr_ingest_wave.h) on the lane emulator, on the zoo of tests/resample_zoo.py: the content classes real
video holds (constants, impulses, period-2 patterns, bi-level blocks, near-black and near-white noise, hard alpha edges) on the smallest
geometry of every build emu_ingest_wave reaches — RGBA8 nodes (mode 2), RGB12 nodes (mode 6), nodes with alpha (mode 4) and, for the
box-pre-reduced plans, the RGBA16F texture orc.downsample leaves (modes 3 and 5).  Vertical-first and height-only plans run as the host
runs them: on the transposed node.  Test infrastructure only; tests/test_gpu_resample_zoo.py holds the device to the same bars.

Bars (tests/resample_zoo.py): A, the exact properties, and B1 per (build class, content class) pooled over all thirteen geometries
(206 142 colour bytes for opaque nodes, 274 856 bytes with alpha); an RGB12 tile must be the RGBA8 build's tile bit for bit, so it has
no pool of its own.  The witness itself is held too: per pool the oracle differs from it in at most 2e-4 of the bytes.

checker_1 and alpha_blocks cannot meet that (resample_zoo.WITNESS_NOT_HELD says why: one value on a rounding boundary, copied over a tile):
they are judged by B1 alone, here and on the device.

Measured (emulator: a sequential f32 sum inside the matrix instruction, the host's sinf / cosf): of 206 142 colour bytes a pool, 0 differ on the
constants, the impulses, checker_1 and stripes_3, 2 on bilevel_blocks and noise_0_8, 7 on noise_247_255, 3 on white_noise; of 274 856 bytes
with alpha 0 on alpha_0, const_alpha_128 and white_ramp, 24 on alpha_blocks (18 on the fractional crop), 3 on alpha_0_5 and noise_under_noise.
The oracle is off the witness in 0 .. 1.84e-4 of a pool (black_impulses: 38 copies of one value on the height-only plan), 5.6e-3 on
checker_1, 2.0e-4 on alpha_blocks.
What the pools are for: with pass 2's weights rounded to a single f16 (tried on a scratch copy, not kept) every tile is still within 1 LSB and
test_gpu_kernel_selection.py's smooth content keeps 0.987 .. 0.998 of its bytes — above that test's 0.985 —, while 12 of these 21 pools fall
to 0.686 .. 0.9975 and win 0 .. 9 of their 518 .. 14 263 disputes against the witness."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import resample_zoo as zoo
from tests.emu_wave_resample import emulate, load


@pytest.fixture(scope="module")
def emu():
    h = load()
    if h is None:
        pytest.skip("no clang++ to build the emulator with")
    return h


_RESULTS = {}
RGB12_TWINS = ("const_5_16_64", "impulses_on_grey", "noise_0_8", "white_noise")   # the classes also run through the RGB12 build (same codes, other loads)


def run(emu, geo, kind):
    """-> (failures, [(class, got, want, node)]) of one geometry x source kind, computed once."""
    if (geo.name, kind) not in _RESULTS:
        plan = geo.plan()
        alpha = kind == "alpha"
        bad, tiles = [], []
        for name in (zoo.ALPHA_CLASSES if alpha else zoo.OPAQUE_CLASSES):
            node = zoo.alpha_node(geo, name) if alpha else zoo.opaque_node(geo, name)
            k, want = orc.resample(node, geo.crop, *geo.dst)
            assert k == plan.kind
            got = emulate(emu, geo, plan, node, alpha)
            again = emulate(emu, geo, plan, node, alpha) if name in ("white_noise", "noise_under_noise") else None
            bad += zoo.check_case(got, want, node, name, not alpha, again)
            if name in RGB12_TWINS and not alpha and tuple(plan.levels) == (0, 0) and plan.axis[0] == 0 and geo.src[0] % 4 == 0 and geo.name != "one_tile":
                twin = emulate(emu, geo, plan, node, False, rgb12=True)
                if not np.array_equal(twin, got):
                    bad.append(f"{name}: the RGB12 build's tile differs from the RGBA8 build's in {(twin != got).sum()} bytes")
            tiles.append((name, got, want, node))
        _RESULTS[geo.name, kind] = (bad, tiles)
    return _RESULTS[geo.name, kind]


@pytest.mark.parametrize("kind", ["opaque", "alpha"])
@pytest.mark.parametrize("geo", zoo.GEOMETRIES, ids=lambda g: g.name)
def test_emulated_kernel_on_the_zoo(emu, geo, kind):
    """Bar A and the exact properties, every content class of one geometry x source kind."""
    bad, tiles = run(emu, geo, kind)
    for name, got, want, _ in tiles:
        print(f"{geo.name:>14} {kind:>6} {name:<20} {(got != want).sum():>4} of {got.size} bytes differ")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("kind", ["opaque", "alpha"])
def test_pooled_shares_and_the_witness(emu, kind):
    """B1 per (build class, content class) over all geometries, and the reference against the witness: at most 2e-4 of a pool's bytes."""
    alpha = kind == "alpha"
    pools = {name: zoo.Pool((kind, name), 4 if alpha else 3) for name in (zoo.ALPHA_CLASSES if alpha else zoo.OPAQUE_CLASSES)}
    for geo in zoo.GEOMETRIES:
        for name, got, want, node in run(emu, geo, kind)[1]:
            pools[name].add(got, want, node, geo.crop)
    bad = []
    for pool in pools.values():
        ok, line = pool.verdict()
        ow = pool.oracle_against_witness()
        print(line + f"; oracle off the witness in {ow:.2e}")
        if not ok or pool.share < zoo.FLOOR:   # (B1 alone here: the emulator's matrix instruction adds in the oracle's order)
            bad.append(line)
        if ow > zoo.WITNESS_MAX_DIFF and pool.key[1] not in zoo.WITNESS_NOT_HELD:
            bad.append(f"{pool.key}: the oracle differs from the witness in {ow:.2e} of the bytes")
    assert not bad, "\n".join(bad)
