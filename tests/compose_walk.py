"""Scenes of the compositor's tile-walk tests (test infrastructure): tests/test_emu_compose_walk.py runs them through the lane emulator,
tests/test_gpu_compose_walk.py through the gfx950 binary — the same lists, built from tests/compose_zoo.py's generators."""
import os

import numpy as np

from tests.compose_zoo import grid_scene, tex, video

SIZES = [(384, 48), (386, 50), (1282, 34)]   # all interior | a two-pixel last block and a 2-row last tile row | 11 tile columns: runs cross row ends
OUTS = ["planar", "nv12", "rgba"]
# A 128 x 16 opaque texture of blocks whose fast-path values raise the guard flag of smr_yuv_fast.h — none, exactly one, or all eight luma
# values of a 4 x 2 block.  Written by nobody at test time: tests/test_emu_compose_walk.py builds it from the header's own enumeration and
# asserts that this file holds exactly that; the device test reads it.
FLAGGED_TEXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "compose_walk_flagged.npy")


def tiles_of(W, H):
    return ((W + 127) // 128) * ((H + 15) // 16)


def walk_scene(W, H):
    """-> (layouts, sources, kinds, shifts).  compose_zoo's grid — 1:1 opaque textures over a colour background, translucent rounded labels with
    a border — with the background cut short of the right edge on the wide output (cleared tiles), a small 1:1 texture inside the background
    cell (tiles that select between two copies), and one texture at its own size and a fractional position (sampled tiles where it covers
    whole tiles — the wide output —, composited tiles along its edges).  shifts[i]: bytes by which the emulator moves source i's base off
    its 16-byte alignment."""
    cols = max(W // 256, 2) if W > 400 else 3
    layouts, sources, kinds = grid_scene(W, H, cols, 1, 0)
    tw = W // cols
    if W > 1024:
        layouts[0].width = float(W - 130)
    i = len(sources)
    sources.append(video(40, 20, 11)); kinds.append(2)
    layouts.append(tex(i, float((cols - 1) * tw + 44), 4.0, 40.0, 20.0))
    if W > 1024:
        sources.append(video(300, 40, 12)); kinds.append(2)
        layouts.append(tex(i + 1, 600.5, -3.25, 300.0, 40.0))   # covers tile columns 5 and 6 over the whole height
    else:
        sources.append(video(100, 20, 12)); kinds.append(2)
        layouts.append(tex(i + 1, 130.5, 20.25, 100.0, 20.0))
    shifts = [0] * len(sources)
    shifts[1] = 4   # the second grid texture's base is not 16-byte aligned: dword texel loads
    return layouts, sources, kinds, shifts


def flagged_scene(texture):
    return [tex(0, 0.0, 0.0, 128.0, 16.0)], [np.ascontiguousarray(texture, np.uint8)], [2], [0]
