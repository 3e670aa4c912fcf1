"""The packed 4:2:2 builds of wave B on the lane emulator: k_compose_output<3, *> (UYVY) and <4, *> (YUYV) of
smelter_amd/csrc/smr_fused_compose.h compiled for the CPU by tests/emu/emu_compose_packed.cpp and launched as smr_render_layouts launches them.

Expected, byte for byte: tests/packed422_model.py's interleave of the reference sequence (the oracle's rgba_to_planar_yuv(.., YUV422)) applied
to the emulator's own RGBA8 output (k_compose_output<2, *>) of the same list — the packed store adds nothing to the composited bytes but the
conversion, whatever class a tile falls into.  Lists: tests/compose_zoo.py's grid scene and zoo seeds 3, 7 and 11, in both rendering modes,
from the LDS copy of the list and read in place (BIG), at 2 x 2, 6 x 2 (a half block only / a full and a half block), 130 x 34 and 258 x 50
(a two-pixel last column block, partial tile rows), 256 x 64 (whole tiles: the paired stores).  Again under guard mode 3 (tests/emu/emu_guard.h)
with tight rows and with slack after each row: no byte outside a row's W * 2 is written.  And one picture made of the pixel pairs whose chroma
lies nearest a code boundary, so that the repair branch runs.  Test infrastructure only: tests/test_gpu_packed_outputs.py holds the gfx950
binary to the same model on the device."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import oracle as orc
from tests import compose_zoo as zoo
from tests import packed422_model as pk

CLANG = "/opt/rocm/lib/llvm/bin/clang++"
P8 = C.POINTER(C.c_uint8)
CLASSES = ["clear", "colour", "texture", "full", "skip", "sampled", "select"]
SIZES = [(2, 2), (6, 2), (130, 34), (258, 50), (256, 64)]


@pytest.fixture(scope="module")
def emu():
    if not os.path.exists(CLANG):
        pytest.skip("no clang++ to build the emulator with")
    from tests import emu_build
    lib = emu_build.build("smr_emu_compose_packed", "emu_compose_packed.cpp", ("smr_fused_compose.h", "smr_layout_dev.h", "smr_convert_dev.h", "smr_yuv_fast.h", "smr_tables.h"))
    h = C.CDLL(lib)
    h.emu_compose_packed.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(P8), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_int,
                                     C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, P8, C.POINTER(C.c_int)]
    h.emu_yuv422_block_flags.argtypes = [P8, C.c_int, C.c_int, C.POINTER(C.c_int)]
    orc.build()
    yield h
    h.emu_set_guard(0, 0)


def _p(a):
    return a.ctypes.data_as(P8)


def compose(emu, layouts, sources, kinds, W, H, nv, srgb=True, banded=-1, groups=0, pitch=0):
    """-> (the RGBA8 node (H, W, 4) for nv 2 / the packed plane's texels (H, W / 2, 4) for nv 3, 4; tile classes and launch facts)."""
    arr = orc.pack_layouts(layouts)
    n = len(sources)
    keep = [None if s is None else np.ascontiguousarray(s, np.uint8) for s in sources]
    px = (P8 * max(n, 1))(*[None if s is None else _p(s) for s in keep])
    ws = (C.c_int * max(n, 1))(*[1 if s is None else s.shape[1] for s in keep])
    hs = (C.c_int * max(n, 1))(*[1 if s is None else s.shape[0] for s in keep])
    ks = (C.c_int * max(n, 1))(*kinds)
    info = (C.c_int * 10)()
    out = np.zeros((H, W, 4) if nv == 2 else (H, W // 2, 4), np.uint8)
    rc = emu.emu_compose_packed(C.addressof(arr), len(layouts), n, px, ws, hs, ks, W, H, nv, int(srgb), banded, groups, pitch, _p(out), info)
    assert rc == 0, f"rc {rc} (-77: a byte outside the rows' texels was written, see stderr)"
    return out, dict(zip(CLASSES + ["listed", "workgroups", "pair"], list(info)))


def lists(W, H, srgb):
    """(name, layouts, sources, kinds): the grid scene and the zoo's lists 3, 7 and 11 on a W x H output."""
    out = [("grid",) + tuple(zoo.grid_scene(W, H, 2, 2, 0, srgb=srgb))]
    for seed in (3, 7, 11):
        rng = np.random.default_rng(100 + seed)
        sources = [zoo.video(96, 54, 7, alpha=True), zoo.video(64, 40, 8), None]
        # (the generator draws boxes of at least 8 x 6: the two smallest outputs take the 130 x 34 lists, whose boxes then leave the frame)
        out.append((f"zoo{seed}", zoo.zoo(max(W, 130), max(H, 34), rng, int(rng.integers(3, 14)), len(sources), srgb), sources, [1, 2, 0]))
    return out


def check(emu, name, layouts, sources, kinds, W, H, srgb, what="", **kw):
    rgba, _ = compose(emu, layouts, sources, kinds, W, H, 2, srgb)
    facts = None
    for order in pk.ORDERS:
        got, facts = compose(emu, layouts, sources, kinds, W, H, 3 + order, srgb, **kw)
        want = pk.expected(orc, rgba, order)
        assert np.array_equal(got, want), (name, (W, H), pk.NAMES[order], srgb, what, facts, int((got != want).sum()), np.argwhere(got != want)[:5].tolist())
    return facts


@pytest.mark.parametrize("srgb", [True, False])
@pytest.mark.parametrize("W,H", SIZES)
def test_packed_output_is_the_reference_sequence_of_the_composited_bytes(emu, W, H, srgb):
    emu.emu_set_guard(0, 0)
    for name, layouts, sources, kinds in lists(W, H, srgb):
        facts = check(emu, name, layouts, sources, kinds, W, H, srgb)
        assert facts["pair"] == 1  # (the allocator's pitch: whole tiles take the paired stores, every other block the per-lane ones)


@pytest.mark.parametrize("W,H", [(130, 34), (256, 64)])
def test_a_list_read_in_place_and_a_band_list_prediction_that_missed(emu, W, H):
    """BIG: more than 48 layouts; banded = 0: every composited tile is done, band after band, by the workgroup that owns it."""
    emu.emu_set_guard(0, 0)
    rng = np.random.default_rng(5)
    sources = [zoo.video(80, 40, 3)]
    layouts = zoo.zoo(W, H, rng, 60, 1)
    check(emu, "60 layouts", layouts, sources, [2], W, H, True)
    name, layouts, sources, kinds = lists(W, H, True)[0]
    check(emu, name, layouts, sources, kinds, W, H, True, what="banded 0, one copy workgroup", banded=0, groups=1)


@pytest.mark.parametrize("rows", ["tight", "slack"])
@pytest.mark.parametrize("W,H", SIZES)
def test_the_packed_stores_touch_only_the_rows_texels(emu, W, H, rows):
    """Guard mode 3: the plane starts behind an unmapped page, is filled from a seeded pattern, and every byte outside each row's first W * 2
    is compared after the launch.  tight: the smallest pitch the fused route admits (W * 2 rounded up to 8: a width of 2 mod 4 leaves four
    bytes of padding, the per-lane stores everywhere); slack: 32 bytes more, a multiple of 16 or not as the width has it."""
    tight = (W * 2 + 7) & ~7
    pitch = tight if rows == "tight" else tight + 32
    emu.emu_set_guard(3, 1)
    try:
        for name, layouts, sources, kinds in lists(W, H, True)[:2]:
            facts = check(emu, name, layouts, sources, kinds, W, H, True, what=f"{rows} rows, pitch {pitch}", pitch=pitch)
            assert facts["pair"] == int(pitch % 16 == 0)
        emu.emu_set_guard(1, 1)  # ... and the plane ENDS at an unmapped page: a store past the last row's last texel kills the run
        name, layouts, sources, kinds = lists(W, H, True)[0]
        check(emu, name, layouts, sources, kinds, W, H, True, what=f"{rows} rows, pitch {pitch}, guard page behind", pitch=pitch)
    finally:
        emu.emu_set_guard(0, 0)


def test_pairs_on_code_boundaries_take_the_repair_branch_to_the_reference_bytes(emu):
    """A 512 x 2 picture of the pixel pairs whose chroma lies nearest a code boundary (chosen in f64, tests/packed422_model.py), through copy
    tiles: the guard flags a chroma value in every block (counted with the header the kernel compiles), and the bytes are the oracle's."""
    emu.emu_set_guard(0, 0)
    px = pk.near_boundary_picture(512, 2)
    flags = (C.c_int * (128 * 1))()
    emu.emu_yuv422_block_flags(_p(px), 512, 2, flags)
    assert min(flags) >= 1 and sum(flags) >= 512, (min(flags), sum(flags))  # (the repair branch runs in every lane)
    layouts = [zoo.tex(0, 0.0, 0.0, 512.0, 2.0)]
    for pitch in (0, 1024 + 8):  # paired stores / per-lane stores
        rgba, classes = compose(emu, layouts, [px], [2], 512, 2, 2)
        assert np.array_equal(rgba, px) and classes["texture"] > 0, classes
        for order in pk.ORDERS:
            got, _ = compose(emu, layouts, [px], [2], 512, 2, 3 + order, pitch=pitch)
            want = pk.expected(orc, px, order)
            assert np.array_equal(got, want), (pk.NAMES[order], pitch, int((got != want).sum()), np.argwhere(got != want)[:5].tolist())
