"""Text nodes on the device: k_text_nodes (smelter_amd/csrc/smr_text_nodes.h — up to 16 rasters per launch, every workgroup walking the bin
of its own tile), its launcher smr_text_nodes (one pinned block, one copy, one synchronisation; not part of smr.h, reached through ctypes
here as the renderer reaches it) and the renderer's Text raster cache (include/smr.h, "Text nodes: cached rasters").

(a) The kernel, on the job zoo of the emulator test (tests/text_zoo.py, surfaces <= 131 x 34), in both context modes: BYTE FOR BYTE what
    smr_blit_glyphs leaves for the same inputs on the same context — the kernel every Text node was drawn by so far, unchanged in its
    interface and launch shape and held by tests/test_gpu_parity.py::test_blit_glyphs — and within test_blit_glyphs's rule of
    oracle.blit_glyphs: no byte more than TOL = 1 off, at least 0.995 of the bytes identical (the share is taken over the jobs of one
    call: a 1 x 1 job has four bytes).  One case draws into destinations wrapped in caller memory and asserts that only their texels change.
(b) The renderer, on a 256 x 144 output with tests/golden/fonts: rasterise calls = new keys, launches = ceil(new rasters / 16), rasters
    shared by nodes, outputs and lanes and released with the last scene that shows them; frames byte-equal to a brand-new renderer's.
(c) The fallback to smr_blit_glyphs of a job whose bins would push the call's block past the limit, forced by lowering the limit
    (smr_text_nodes_limit) under a small run of full-node quads on a large node."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from oracle import oracle as orc
from oracle.oracle import Glyph
from tests import refpipe, text_zoo as zoo

pytestmark = pytest.mark.gpu

TOL = 1  # LSB per channel: test_gpu_parity.test_blit_glyphs's rule
SHARE = 0.995
FONTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fonts")
P = C.c_void_p
U = C.c_uint32


@pytest.fixture(scope="module")
def hip():
    from smelter_amd import hip as h
    return h


@pytest.fixture(scope="module", params=["srgb", "unorm"])
def ctx(hip, request):
    c = hip.Context(0, mode=hip.MODE_GPU_OPTIMIZED if request.param == "srgb" else hip.MODE_CPU_OPTIMIZED)
    c.is_srgb = request.param == "srgb"
    yield c
    c.close()


@pytest.fixture(scope="module")
def gpu_ctx(hip):
    c = hip.Context(0)
    yield c
    c.close()


def entry(lib, limit=False):
    fn = lib.smr_text_nodes_limit if limit else lib.smr_text_nodes
    fn.argtypes = [P, C.POINTER(P), C.POINTER(C.c_float * 4), C.POINTER(C.POINTER(zoo.CGlyph)), C.POINTER(U), C.POINTER(P), C.POINTER(U), C.POINTER(U), U] + \
        ([C.c_size_t] if limit else [])
    fn.restype = C.c_int
    return fn


def text_nodes(ctx, surfaces, jobs, limit=None):
    """One smr_text_nodes call: jobs[i] drawn into surfaces[i].  -> the status"""
    n = len(jobs)
    garrs = [zoo.pack(j[3]) for j in jobs]
    atlases = [np.ascontiguousarray(j[4], dtype=np.uint8) for j in jobs]
    args = [ctx.handle, (P * n)(*[s.handle for s in surfaces]), ((C.c_float * 4) * n)(*[(C.c_float * 4)(*[float(x) for x in j[2]]) for j in jobs]),
            (C.POINTER(zoo.CGlyph) * n)(*[C.cast(g, C.POINTER(zoo.CGlyph)) for g in garrs]), (U * n)(*[len(j[3]) for j in jobs]),
            (P * n)(*[a.ctypes.data for a in atlases]), (U * n)(*[a.shape[1] for a in atlases]), (U * n)(*[a.shape[0] for a in atlases]), n]
    if limit is not None:
        return entry(ctx.lib, True)(*args, limit)
    return entry(ctx.lib)(*args)


def held(ctx, jobs, what):
    """The jobs through ONE smr_text_nodes call, each held byte for byte to smr_blit_glyphs on the same context, and the call to the oracle
    under test_blit_glyphs's rule.  -> the pictures"""
    live = [j for j in jobs if j[0] and j[1]]
    surfaces = [ctx.surface(j[0], j[1]) for j in live]
    assert text_nodes(ctx, surfaces, live) == 0, ctx.lib.smr_last_error(ctx.handle)
    got, want = [], []
    for k, (s, (w, h, bg, glyphs, atlas)) in enumerate(zip(surfaces, live)):
        px = s.download()
        witness = ctx.surface(w, h)
        ctx.blit_glyphs(witness, bg, glyphs, atlas)
        ref = witness.download()
        diff = np.argwhere(px != ref)
        assert diff.size == 0, (f"{what}, job {k} ({w} x {h}): texel (x {diff[0][1]}, y {diff[0][0]}) is {px[diff[0][0], diff[0][1]]}, smr_blit_glyphs gives "
                                f"{ref[diff[0][0], diff[0][1]]}; {len(diff)} bytes differ")
        model = orc.blit_glyphs(w, h, bg, glyphs, atlas, srgb=ctx.is_srgb)
        d = refpipe.max_diff(px, model)
        print(f"{what}, job {k} ({w} x {h}): max |diff| to the oracle {d} LSB, {refpipe.exact_fraction(px, model):.5f} identical")
        assert d <= TOL, f"{what}, job {k} ({w} x {h}): max |diff| to the oracle = {d} LSB (> {TOL})"
        got.append(px)
        want.append(model)
        witness.destroy()
        s.destroy()
    if got:
        a, b = np.concatenate([g.reshape(-1) for g in got]), np.concatenate([m.reshape(-1) for m in want])
        share = float((a == b).mean())
        print(f"{what}: {share:.5f} of {a.size} bytes identical to the oracle")
        assert share >= SHARE, f"{what}: only {share:.5f} of the bytes identical to the oracle (< {SHARE})"
    return got


# ------------------------------------------------------------------ (a) the kernel
def test_sizes(ctx):
    """Widths 1, 3, 4, 5, 63, 64, 65, 67 x heights 1, 15, 16, 17: 32 jobs, two launches of one call."""
    held(ctx, zoo.sizes(), "sizes")


def test_edge_cases(ctx):
    """No glyphs; a glyph in four bins; starts at x mod 4 = 1, 2, 3; ends on the last texel and on the atlas' last byte (width 257); glyphs
    without an area, partly and wholly outside; an empty bin between full ones; painter's order — 14 jobs in one launch."""
    cases = zoo.edge_cases()
    got = dict(zip(cases, held(ctx, list(cases.values()), "edge cases")))
    assert (got["painter's order a, b"] != got["painter's order b, a"]).any()
    assert len(np.unique(got["no glyphs"].reshape(-1, 4), axis=0)) == 1


@pytest.mark.parametrize("n", [1, 16, 17])
def test_batches(ctx, n):
    """1, 16 and 17 jobs of mixed sizes: one launch, one launch, two.  (The job without a texel in the middle of the zoo's batches is left out
    here, as the renderer leaves a zero-sized node out: smr_surface_create makes no such surface.  The emulator test hands k_text_nodes the
    empty job itself.)"""
    held(ctx, zoo.batch(n), f"batch of {n}")


@pytest.mark.parametrize("geometry", ["tight", "slack", "window"])
def test_wrapped_destinations_only_their_texels_change(ctx, hip, geometry):
    """Destinations in caller memory (tests/wrapped.py): 67 texels a row on a pitch of 268 (no 16-byte stores), 268 + 16, and as a window
    inside a buffer three times as wide (16-byte stores beside live data).  Every byte outside the texels keeps its value."""
    import torch

    from tests.wrapped import WrappedSurface
    cases = zoo.edge_cases()
    jobs = [cases["partly and wholly outside"], cases["ends on the last texel"], cases["ends on the last texel of a whole tile"], cases["no glyphs"]]
    wrapped = [WrappedSurface(torch, ctx, j[0], j[1], hip.PX_RGBA8, geometry, 500 + k) for k, j in enumerate(jobs)]
    assert text_nodes(ctx, [w.surface for w in wrapped], jobs) == 0, ctx.lib.smr_last_error(ctx.handle)
    ctx.sync()
    for k, (ws, (w, h, bg, glyphs, atlas)) in enumerate(zip(wrapped, jobs)):
        px = ws.texels(f"smr_text_nodes job {k}")
        witness = ctx.surface(w, h)
        ctx.blit_glyphs(witness, bg, glyphs, atlas)
        assert (px == witness.download()).all(), f"job {k} ({w} x {h}, {geometry})"
        witness.destroy()


def test_what_the_launcher_refuses(ctx, hip):
    """smr_blit_glyphs's validation — RGBA8 targets, glyphs inside their atlas —, and a repeated target."""
    job = zoo.edge_cases()["straddles four tiles"]
    w, h, bg, glyphs, atlas = job
    a, b = ctx.surface(w, h), ctx.surface(w, h)
    before = a.download()
    assert text_nodes(ctx, [a, a], [job, job]) < 0 and b"repeats" in ctx.lib.smr_last_error(ctx.handle)
    outside = (w, h, bg, [Glyph(0, 0, 5, 5, atlas.shape[1] - 4, 0, (1.0, 1.0, 1.0, 1.0))], atlas)
    assert text_nodes(ctx, [a, b], [job, outside]) < 0 and b"outside" in ctx.lib.smr_last_error(ctx.handle)
    r8 = ctx.surface(w, h, hip.PX_R8)
    assert text_nodes(ctx, [r8], [job]) < 0 and b"RGBA8" in ctx.lib.smr_last_error(ctx.handle)
    ctx.sync()
    assert (a.download() == before).all()  # a refused call draws nothing
    assert text_nodes(ctx, [], []) == 0
    for s in (a, b, r8):
        s.destroy()


# ------------------------------------------------------------------ (c) the fallback
def test_a_job_past_the_block_limit_is_drawn_by_blit_glyphs(ctx):
    """60 full-node quads on a 1024 x 512 node: 60 x 512 tiles of bin entries.  With the limit lowered to 600 KiB the job does not fit beside
    its 512 KiB atlas and goes through smr_blit_glyphs, while the small job of the same call stays batched; with the product's 64 MiB both
    are batched.  All three pictures of the large node are the same bytes."""
    rng = np.random.default_rng(31)
    W, H = 1024, 512
    atlas = zoo.atlas_of(rng, W, H)
    quads = [Glyph(0, 0, W, H, 0, 0, (float(rng.random()), float(rng.random()), float(rng.random()), 0.05)) for _ in range(60)]
    big = (W, H, (0.1, 0.3, 0.2, 0.5), quads, atlas)
    small = zoo.edge_cases()["straddles four tiles"]
    pictures = []
    for limit in (600 << 10, None):
        a, b = ctx.surface(W, H), ctx.surface(small[0], small[1])
        assert text_nodes(ctx, [a, b], [big, small], limit) == 0, ctx.lib.smr_last_error(ctx.handle)
        pictures.append((a.download(), b.download()))
        a.destroy()
        b.destroy()
    wa, wb = ctx.surface(W, H), ctx.surface(small[0], small[1])
    ctx.blit_glyphs(wa, big[2], big[3], big[4])
    ctx.blit_glyphs(wb, small[2], small[3], small[4])
    for big_px, small_px in pictures:
        assert (big_px == wa.download()).all() and (small_px == wb.download()).all()
    wa.destroy()
    wb.destroy()


# ------------------------------------------------------------------ (b) the renderer
W, H = 256, 144
LABELS = [f"cam {i}" for i in range(17)] + ["cam 0", "cam 5", "cam 5"]  # 20 nodes, 17 distinct keys


def scene(labels):
    """20 labels of 60 x 14 on a 4 x 5 grid, each in a view of its own that places it."""
    kids = []
    for i, t in enumerate(labels):
        kids.append({"type": "view", "left": 62 * (i % 4), "top": 16 * (i // 4), "width": 60, "height": 14,
                     "children": [{"type": "text", "text": t, "font_size": 11.0, "width": 60.0, "height": 14.0, "color": "#FFE080FF", "background_color": "#10305080"}]})
    return json.dumps({"type": "view", "background_color": "#00000000", "children": kids})


def cell(px, i):
    return px[16 * (i // 4):16 * (i // 4) + 14, 62 * (i % 4):62 * (i % 4) + 60]


@pytest.fixture(scope="module")
def book():
    from smelter_amd import fontbook
    b = fontbook.NativeFontBook()
    assert b.add_dir(FONTS) == 3
    yield b
    b.close()


def frame(r, hip, output="out", pts=0.0):
    return np.asarray(r.render(pts, {})[output].download()[0]).reshape(H, W, 4).copy()


def test_rasters_are_cached_and_shared(gpu_ctx, hip, book):
    from smelter_amd.renderer import Renderer
    ctx = gpu_ctx
    r, fresh = Renderer(ctx), Renderer(ctx)
    try:
        r.set_fontbook(book)
        assert r.text_stats() == (0, 0, 0)
        r.update_scene("out", W, H, scene(LABELS), hip.FRAME_RGBA)
        assert r.text_stats() == (17, 2, 17)          # rasterise calls = new keys; launches = ceil(17 / 16); resident
        first = frame(r, hip)
        assert (cell(first, 0) == cell(first, 17)).all() and (cell(first, 5) == cell(first, 19)).all()   # the nodes of one key show one raster
        assert (cell(first, 0) != cell(first, 1)).any() and cell(first, 3)[..., 3].max() > 200           # the text is really there (background alpha: 128)
        # one label changes: one rasterise call, one launch; the raster only the old scene showed is released
        changed = LABELS[:3] + ["LIVE"] + LABELS[4:]
        r.update_scene("out", W, H, scene(changed), hip.FRAME_RGBA)
        assert r.text_stats() == (18, 3, 17)
        # a second output with the same scene: nothing new
        r.update_scene("out2", W, H, scene(changed), hip.FRAME_RGBA)
        assert r.text_stats() == (18, 3, 17)
        # the same update again: nothing at all
        r.update_scene("out", W, H, scene(changed), hip.FRAME_RGBA)
        assert r.text_stats() == (18, 3, 17)
        outs = r.render(0.04, {})
        a = np.asarray(outs["out"].download()[0]).reshape(H, W, 4).copy()
        b = np.asarray(outs["out2"].download()[0]).reshape(H, W, 4).copy()
        # a brand-new renderer given only the final scene
        fresh.set_fontbook(book)
        fresh.update_scene("out", W, H, scene(changed), hip.FRAME_RGBA)
        assert fresh.text_stats() == (17, 2, 17)
        want = frame(fresh, hip)
        assert (a == want).all() and (b == want).all()
        for i in range(20):
            if i != 3:
                assert (cell(a, i) == cell(first, i)).all(), f"label {i} changed with label 3"
        assert (cell(a, 3) != cell(first, 3)).any()
        # released with the last scene that shows them
        r.unregister_output("out")
        assert r.text_stats() == (18, 3, 17)
        assert (frame(r, hip, "out2", 0.08) == want).all()
        r.unregister_output("out2")
        assert r.text_stats() == (18, 3, 0)
    finally:
        r.close()
        fresh.close()


def test_another_font_book_reuses_nothing(gpu_ctx, hip, book):
    from smelter_amd import fontbook
    from smelter_amd.renderer import Renderer
    bold = fontbook.NativeFontBook([os.path.join(FONTS, "Inter_18pt-Bold.ttf")])
    r = Renderer(gpu_ctx)
    try:
        r.set_fontbook(book)
        r.update_scene("out", W, H, scene(LABELS), hip.FRAME_RGBA)
        regular = frame(r, hip)
        r.set_fontbook(bold)
        assert r.text_stats() == (17, 2, 17)          # the active scene keeps its rasters until it is replaced
        r.update_scene("out", W, H, scene(LABELS), hip.FRAME_RGBA)
        assert r.text_stats() == (34, 4, 17)          # nothing was reused; the previous book's rasters went with their scene
        assert (frame(r, hip, pts=0.04) != regular).any()
        r.set_fontbook(book)                          # the first book again is a new generation too
        r.update_scene("out", W, H, scene(LABELS), hip.FRAME_RGBA)
        assert r.text_stats() == (51, 6, 17)
        assert (frame(r, hip, pts=0.08) == regular).all()
    finally:
        r.close()
        bold.close()


def test_set_text_on_a_shared_node_leaves_the_others_alone(gpu_ctx, hip, book):
    """Nodes 5, 18 and 19 show one raster.  smr_renderer_set_text on node 18 gives it a surface of its own, drawn by the same kernel."""
    from smelter_amd import _ffi
    from smelter_amd.renderer import Renderer
    r = Renderer(gpu_ctx)
    try:
        r.set_fontbook(book)
        nodes = r.update_scene("out", W, H, scene(LABELS), hip.FRAME_RGBA)
        before = frame(r, hip)
        text_nodes_ = [n for n in nodes if n.kind == _ffi.NODE_TEXT]
        assert len(text_nodes_) == 20 and [n.payload for n in text_nodes_] == LABELS
        glyphs, atlas = book.rasterise("own", 60, 14, 11.0, color=(0.2, 1.0, 0.4, 1.0))
        bg = orc.color_to_shader((0x80, 0x10, 0x10, 0xFF), True)
        r.set_text("out", text_nodes_[18].index, glyphs, atlas, bg)
        assert r.text_stats() == (17, 3, 17)          # one more launch, no rasterise call of the renderer's, nothing released
        after = frame(r, hip, pts=0.04)
        for i in range(20):
            if i != 18:
                assert (cell(after, i) == cell(before, i)).all(), f"label {i} changed with node 18's run"
        # the node's own surface: what smr_blit_glyphs draws of the run, composed 1:1 over the transparent view (the rule of
        # test_gpu_renderer's Text tests for that copy: <= 1 LSB, > 0.999 identical)
        witness = gpu_ctx.surface(60, 14)
        gpu_ctx.blit_glyphs(witness, bg, glyphs, atlas)
        want = witness.download()
        assert (cell(after, 18) != cell(before, 18)).any()
        assert np.abs(cell(after, 18).astype(int) - want.astype(int)).max() <= 1 and (cell(after, 18) == want).mean() > 0.999
        witness.destroy()
        # the next update draws the node from the book again, from the raster its key still has
        r.update_scene("out", W, H, scene(LABELS), hip.FRAME_RGBA)
        assert r.text_stats() == (17, 3, 17)
        assert (frame(r, hip, pts=0.08) == before).all()
    finally:
        r.close()


def test_two_lanes_give_the_one_lane_bytes(gpu_ctx, hip, book):
    from smelter_amd.renderer import Renderer
    lane = hip.Context(0)
    one, two = Renderer(gpu_ctx), Renderer(gpu_ctx, lanes=[lane])
    try:
        for r in (one, two):
            r.set_fontbook(book)
            r.update_scene("out", W, H, scene(LABELS), hip.FRAME_RGBA)
        assert two.text_stats() == (17, 2, 17)
        want = frame(one, hip)
        for k in range(4):  # both lanes, twice
            assert (frame(two, hip, pts=0.04 * k) == want).all(), f"frame {k}"
        changed = LABELS[:7] + ["on air"] + LABELS[8:]
        for r in (one, two):
            r.update_scene("out", W, H, scene(changed), hip.FRAME_RGBA)
        assert two.text_stats() == (18, 3, 17)
        want = frame(one, hip, pts=0.2)
        for k in range(4):
            assert (frame(two, hip, pts=0.2 + 0.04 * k) == want).all(), f"frame {k} after the update"
    finally:
        one.close()
        two.close()
        lane.close()


def test_cpu_optimized_mode(hip, book):
    """The batched path in the other context mode: the same counts, and the node is what smr_blit_glyphs draws there."""
    from smelter_amd.renderer import Renderer
    c = hip.Context(0, mode=hip.MODE_CPU_OPTIMIZED)
    r = Renderer(c)
    try:
        r.set_fontbook(book)
        r.update_scene("out", W, H, scene(LABELS), hip.FRAME_RGBA)
        assert r.text_stats() == (17, 2, 17)
        got = frame(r, hip)
        assert cell(got, 3)[..., 3].max() > 200 and (cell(got, 0) == cell(got, 17)).all() and (cell(got, 0) != cell(got, 1)).any()
    finally:
        r.close()
        c.close()
