"""The condition on the reference alone, for tests/test_gpu_small_tiles.py: B2 lets the f64 witness of tests/resample_zoo.py decide between the
device and the oracle, which is only sound where oracle and witness themselves agree — per pool the oracle differs from the witness in at
most resample_zoo.WITNESS_MAX_DIFF of the bytes.  Checked here, without a device and without the emulator, on every pool the device module
judges by the zoo's bar: per (source kind, content class) the tiles of all paths that take the wave route (small_tiles.wave_cases — held
to the device's own routes by that module, to the emulator's window limits by tests/test_emu_small_tiles.py).  The pools of the pass
kernels have a floor of their own and no B2.

Measured (549 822 colour bytes a pool, 733 096 with alpha; the oracle off the witness in):
  yuv420  constants 0; white_impulses 8.73e-5 (48 bytes), bilevel_blocks 1.25e-4 (69), noise_0_8 5.5e-6 (3), white_noise 1.20e-4 (66);
  opaque  constants 0; white_impulses 6.18e-5 (34), bilevel_blocks 1.44e-4 (79), noise_0_8 5.5e-6 (3), white_noise 1.20e-4 (66);
  alpha   alpha_0 0; noise_under_noise 8.87e-5 (65); alpha_blocks 1.06e-3 (778).
alpha_blocks cannot meet the constant at these sizes either: hard alpha edges put whole runs of texels on one rounding boundary (379 of its
bytes on open_v's 256 x 45 alone).  It is on resample_zoo.WITNESS_NOT_HELD already, for the same reason on the zoo's fractional crop, and is
judged by B1 alone in every module; no other class joins that list because of these sizes."""
import pytest

from oracle import oracle as orc
from tests import resample_zoo as zoo
from tests import small_tiles as st

POOLS = [(k, n) for k in st.KINDS for n in st.CONTENTS[k]]


@pytest.mark.parametrize("kind,name", POOLS, ids=[f"{k}-{n}" for k, n in POOLS])
def test_the_oracle_agrees_with_the_witness_on_a_wave_pool(kind, name):
    orc.build()
    channels = 4 if kind == "alpha" else 3
    total = differ = 0
    worst = (0, "-")
    for path in st.PATHS:
        for geo in st.wave_cases(path, kind):
            node, _ = st.node_of(geo, kind, name)
            _, want = orc.resample(node, geo.crop, *geo.dst)
            d = int((want[..., :channels] != zoo.witness(node, geo.crop, *geo.dst)[..., :channels]).sum())
            total, differ = total + want[..., :channels].size, differ + d
            worst = max(worst, (d, geo.name))
    print(f"{kind:>6} {name:<18} {total:>7} bytes, oracle off the witness in {differ:>4} = {differ / total:.2e} (most on {worst[1]}: {worst[0]})")
    assert total >= zoo.POOL_MIN
    if name in zoo.WITNESS_NOT_HELD:
        return   # (judged by B1 alone: Pool.verdict gives such a class no B2)
    assert differ <= zoo.WITNESS_MAX_DIFF * total, f"{kind} {name}: the oracle differs from the witness in {differ / total:.2e} of the bytes"
