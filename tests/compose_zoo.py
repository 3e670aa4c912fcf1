"""The layout lists of the compositor tests (test infrastructure): a small grid of video tiles with labels and a random "zoo" of layouts —
rotations, four radii, borders below and above one pixel, shadows, parent masks, translucent colours, textures with an alpha channel, crops,
source indices out of range, boxes that leave the frame.  tests/test_emu_compose.py (the kernel source on the lane emulator) and
tests/test_gpu_compose_zoo.py (the gfx950 binary) draw the same lists from the same seeds."""
import numpy as np

from oracle import oracle as orc


def video(w, h, seed, alpha=False):
    """An opaque 'resampled tile' (noise on a gradient: every texel differs from its neighbours), or with `alpha` a premultiplied one."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    t = np.stack([(xx * 3 + seed * 40) % 256, (yy * 5 + 90) % 256, (xx + yy * 2) % 256, np.full_like(xx, 255)], -1).astype(np.int64)
    t[..., :3] = np.clip(t[..., :3] + rng.integers(-20, 21, (h, w, 3)), 0, 255)
    if alpha:
        a = rng.integers(0, 256, (h, w))
        t = np.concatenate([t[..., :3] * a[..., None] // 255, a[..., None]], -1)
    return t.astype(np.uint8)


def tex(i, left, top, w, h, tw=None, th=None, **kw):
    tw, th = tw or int(w), th or int(h)
    return orc.Layout(top=top, left=left, width=w, height=h, type=0, source_index=i, crop=(0.0, 0.0, float(tw), float(th)), **kw)


def grid_scene(W, H, cols, rows, gap=0, srgb=True, labels=True):
    """BASELINE configs[2] in small: a background colour, a grid of opaque tiles blitted 1:1 (texture / select / colour / clear tiles), and
    translucent rounded labels with a border over the lower left corners of every other one (composited tiles)."""
    tw, th = (W - gap * (cols + 1)) // cols, (H - gap * (rows + 1)) // rows
    layouts = [orc.Layout(top=0.0, left=0.0, width=float(W), height=float(H), type=1, color=orc.color_to_shader((16, 24, 48, 255), srgb))]
    sources, kinds = [], []
    for r in range(rows):
        for c in range(cols):
            if r == rows - 1 and c == cols - 1:
                continue  # the last cell stays background
            i = len(sources)
            sources.append(video(tw, th, i))
            kinds.append(2)
            left, top = gap + c * (tw + gap), gap + r * (th + gap)
            layouts.append(tex(i, float(left), float(top), float(tw), float(th)))
            if labels and i % 2 == 0:
                layouts.append(orc.Layout(top=float(top + th - 22), left=float(left + 6), width=70.0, height=16.0, type=1, border_radius=(5.0,) * 4,
                                          color=orc.color_to_shader((0, 0, 0, 150), srgb), border_width=1.0, border_color=orc.color_to_shader((255, 255, 255, 200), srgb)))
    return layouts, sources, kinds


def zoo(W, H, rng, n, n_sources, srgb=True):
    layouts = []
    for _ in range(n):
        t = int(rng.integers(0, 3))
        w, h = float(rng.uniform(8, W * 0.7)), float(rng.uniform(6, H * 0.9))
        rmax = min(w, h) / 2
        L = orc.Layout(top=float(rng.uniform(-10, H - 4)), left=float(rng.uniform(-20, W - 8)), width=w, height=h, type=t,
                       rotation_degrees=float(rng.choice([0.0, 0.0, 0.0, 17.0, -33.5, 90.0])),
                       border_radius=tuple(float(rng.uniform(0, rmax)) if rng.random() < 0.5 else 0.0 for _ in range(4)),
                       color=orc.color_to_shader(tuple(int(v) for v in rng.integers(0, 256, 3)) + (int(rng.choice([255, 255, 140, 0])),), srgb),
                       border_color=orc.color_to_shader(tuple(int(v) for v in rng.integers(0, 256, 4)), srgb),
                       border_width=float(rng.choice([0.0, 0.0, 0.5, 1.0, 3.5])), blur_radius=float(rng.choice([0.0, 2.0, 9.0])) if t == 2 else 0.0)
        if t == 0:
            L.source_index = int(rng.integers(0, n_sources + 1))   # (n_sources: out of range = the empty texture)
            L.crop = (float(rng.uniform(0, 6)), float(rng.uniform(0, 9)), float(rng.uniform(20, 90)), float(rng.uniform(10, 50)))
        if rng.random() < 0.4:
            L.masks = [orc.Mask(radius=(float(rng.uniform(0, 12)),) * 4, top=float(rng.uniform(0, H / 2)), left=float(rng.uniform(0, W / 2)),
                                width=float(rng.uniform(W / 4, W)), height=float(rng.uniform(H / 4, H))) for _ in range(int(rng.integers(1, 4)))]
        layouts.append(L)
    return layouts


def frame_planes(w, h, seed):
    """A planar 4:2:0 frame (even w, h): luma noise on a gradient, chroma that changes from sample to sample."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    y = np.clip(16 + (xx * 2 + yy * 5 + seed * 30) % 200 + rng.integers(-6, 7, (h, w)), 0, 255).astype(np.uint8)
    cy, cx = np.mgrid[0:h // 2, 0:w // 2]
    u = ((cx * 7 + cy * 3 + seed * 11) % 256).astype(np.uint8)
    v = rng.integers(0, 256, (h // 2, w // 2), dtype=np.uint8)
    return y, u, v


def direct_crops(layouts):
    """The same list with every texture layout's crop on whole texels at the layout's own (rounded) size: ResampledChild::is_needed says no
    (resampler.rs:286-299), so GpuOptimized draws it without a resampling pass — the compositor samples the source itself."""
    for L in layouts:
        if L.type == 0:
            dw, dh = max(int(np.floor(np.float32(L.width) + np.float32(0.5))), 1), max(int(np.floor(np.float32(L.height) + np.float32(0.5))), 1)
            L.crop = (float(np.floor(L.crop[0])), float(np.floor(L.crop[1])), float(dw), float(dh))
    return layouts


def many_masks(W, H, rng, layouts, per_layout):
    """`per_layout` parent masks (zoo's own distribution) on every layout of the list."""
    for L in layouts:
        L.masks = [orc.Mask(radius=(float(rng.uniform(0, 12)),) * 4, top=float(rng.uniform(0, H / 2)), left=float(rng.uniform(0, W / 2)),
                            width=float(rng.uniform(W / 4, W)), height=float(rng.uniform(H / 4, H))) for _ in range(per_layout)]
    return layouts
