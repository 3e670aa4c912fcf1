"""What a WebView node must look like (test infrastructure): the yardsticks of tests/test_emu_web_view.py and tests/test_gpu_web_view.py.

The node is plain compositing (transformations/web_renderer/renderer.rs:78-134, shader.rs:53-114, render_website.wgsl): the page — the
browser's BGRA bitmap, B and R exchanged — and one axis-aligned rectangle per child, drawn one after the other onto a transparent RGBA8
target with premultiplied-alpha blending.

* `oracle_node`: a child on an INTEGER rectangle is a plain texture layout (no crop, radius, border, mask or rotation) and the page a 1:1
  texture layout of the swizzled bitmap, so the independent reference is the committed oracle.apply_layouts over the layer list
  `oracle_layers` builds.  The bar is the compositor's: within 1 LSB per channel.
* `model_node`: on a FRACTIONAL rectangle the oracle's layout has a smooth (anti-aliased) edge where a rasteriser has a hard one, so there the
  reference is a short numpy f32 model written from render_website.wgsl and the rasteriser's coverage rule — pixel (px, py) belongs to the
  rectangle iff x <= px + 0.5 < x + width and y <= py + 0.5 < y + height; its fragment is the child sampled bilinearly (clamp to edge) at
  ((px + 0.5 - x) / width, (py + 0.5 - y) / height).  tests/test_emu_web_view.py holds the model itself to the oracle within 1 LSB on the
  integer cases before anything is compared with it.  Fractional offsets are multiples of 1/4 and never .5: no pixel centre lies on an edge.
"""
import math

import numpy as np

from oracle import oracle as orc

CHROMIUM, OVER, UNDER = 0, 1, 2  # smr_web_embedding


def swizzle(page_bgra):
    return np.ascontiguousarray(np.asarray(page_bgra, np.uint8)[..., [2, 1, 0, 3]])


def premultiplied(rng, w, h, opaque=False):
    """Noise with varying alpha (or opaque), premultiplied: colour <= alpha, as a browser paints and as node textures are."""
    px = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    if opaque:
        px[..., 3] = 255
    px[..., :3] = (px[..., :3].astype(np.uint32) * px[..., 3:4] // 255).astype(np.uint8)
    return px


def page_bitmap(rng, w, h):
    """A premultiplied BGRA page with transparent, translucent and opaque regions."""
    px = premultiplied(rng, w, h)
    px[: max(h // 3, 1), : max(w // 2, 1), 3] = 255
    px[h - max(h // 4, 1):, :, :] = 0
    px[..., :3] = np.minimum(px[..., :3], px[..., 3:4])
    return px


def has_pixels(rect):
    x, y, w, h = (float(v) for v in rect)
    return all(math.isfinite(v) for v in (x, y, w, h)) and w > 0 and h > 0


def drawn(children, rects, method):
    """The (child, rectangle) pairs a node draws: zipped (renderer.rs:105-114), none with Chromium embedding (:128-130)."""
    return [] if method == CHROMIUM else list(zip(children, rects))


def oracle_layers(page_bgra, children, rects, method):
    """-> (layouts, sources) for oracle.apply_layouts.  Source 0 is the swizzled page."""
    H, W = page_bgra.shape[:2]
    page = orc.Layout(top=0.0, left=0.0, width=float(W), height=float(H), type=0, source_index=0, crop=(0.0, 0.0, float(W), float(H)))
    sources, kids = [swizzle(page_bgra)], []
    for child, rect in drawn(children, rects, method):
        sources.append(child)
        if not has_pixels(rect) or child is None:
            continue
        x, y, w, h = (float(v) for v in rect)
        ch, cw = child.shape[:2]
        kids.append(orc.Layout(top=y, left=x, width=w, height=h, type=0, source_index=len(sources) - 1, crop=(0.0, 0.0, float(cw), float(ch))))
    return (kids + [page] if method == UNDER else [page] + kids), sources


def oracle_node(page_bgra, children, rects, method, srgb):
    H, W = page_bgra.shape[:2]
    layouts, sources = oracle_layers(page_bgra, children, rects, method)
    return orc.apply_layouts(W, H, layouts, sources, srgb=srgb)


# ------------------------------------------------------------------------------------------------ the f32 model
F = np.float32


def _decode(px, srgb):
    """RGBA8 -> premultiplied f32 the way the texture unit does: sRGB texels through the decode table, alpha and UNORM texels / 255."""
    out = np.empty(px.shape, F)
    if srgb:
        out[..., :3] = orc.srgb_decode_table().astype(F)[px[..., :3]]
    else:
        out[..., :3] = px[..., :3].astype(F) / F(255)
    out[..., 3] = px[..., 3].astype(F) / F(255)
    return out


def _unorm8(v):
    v = np.where(v > F(0), v, F(0)).astype(F)  # (WGSL clamp; NaN -> 0)
    v = np.minimum(v, F(1))
    return np.floor(v * F(255) + F(0.5)).astype(np.uint8)


def _encode(v, srgb):
    """The render target's store: sRGB = the number of code thresholds at or below the value, UNORM = round to nearest."""
    out = np.empty(v.shape, np.uint8)
    if srgb:
        thr = orc.srgb_threshold_table().astype(F)[1:256]
        out[..., :3] = np.searchsorted(thr, np.nan_to_num(v[..., :3], nan=0.0), side="right").astype(np.uint8)
    else:
        out[..., :3] = _unorm8(v[..., :3])
    out[..., 3] = _unorm8(v[..., 3])
    return out


def _blend(acc8, frag, srgb):
    """PREMULTIPLIED_ALPHA_BLENDING onto the 8-bit target: src + dst * (1 - src.a), stored."""
    inv = (F(1) - frag[..., 3:4]).astype(F)
    return _encode((frag + (_decode(acc8, srgb) * inv).astype(F)).astype(F), srgb)


def _bilinear(src, u, v, srgb):
    """textureSample with a linear filter and clamp-to-edge at (u[x], v[y]) — 8 fractional bits of sub-texel weight, as the hardware has."""
    sh, sw = src.shape[:2]
    tex = _decode(src, srgb)

    def axis(t, n):
        s = (t * F(n) - F(0.5)).astype(F)
        f0 = np.floor(s)
        f = (np.floor(((s - f0).astype(F) * F(256) + F(0.5)).astype(F)) / F(256)).astype(F)
        i0 = f0.astype(np.int64)
        return np.clip(i0, 0, n - 1), np.clip(i0 + 1, 0, n - 1), f

    x0, x1, fx = axis(u, sw)
    y0, y1, fy = axis(v, sh)
    fx, fy = fx[None, :, None], fy[:, None, None]
    gx, gy = (F(1) - fx).astype(F), (F(1) - fy).astype(F)
    a, b = tex[y0][:, x0], tex[y0][:, x1]
    c, d = tex[y1][:, x0], tex[y1][:, x1]
    top = ((a * gx).astype(F) + (b * fx).astype(F)).astype(F)
    bot = ((c * gx).astype(F) + (d * fx).astype(F)).astype(F)
    return ((top * gy).astype(F) + (bot * fy).astype(F)).astype(F)


def model_node(page_bgra, children, rects, method, srgb):
    """The node's RGBA8 texels by the f32 model: every layer blended onto the 8-bit target and re-encoded, the first onto transparent."""
    H, W = page_bgra.shape[:2]
    acc = np.zeros((H, W, 4), np.uint8)
    layers = [("child", c, q) for c, q in drawn(children, rects, method)]
    layers = layers + [("page", None, None)] if method == UNDER else [("page", None, None)] + layers
    cx, cy = np.arange(W) + 0.5, np.arange(H) + 0.5  # pixel centres (float64: the rule itself, not the kernel's integer bounds)
    for kind, child, rect in layers:
        if kind == "page":
            acc = _blend(acc, _decode(swizzle(page_bgra), srgb), srgb)
            continue
        if child is None or not has_pixels(rect):
            continue
        x, y, w, h = (float(v) for v in rect)
        xs, ys = np.flatnonzero((cx >= x) & (cx < x + w)), np.flatnonzero((cy >= y) & (cy < y + h))
        if xs.size == 0 or ys.size == 0:
            continue
        u = ((xs.astype(F) + F(0.5) - F(x)).astype(F) / F(w)).astype(F)
        v = ((ys.astype(F) + F(0.5) - F(y)).astype(F) / F(h)).astype(F)
        frag = _bilinear(child, u, v, srgb)
        win = np.ix_(ys, xs)
        acc[win] = _blend(acc[win], frag, srgb)
    return acc


# ------------------------------------------------------------------------------------------------ the cases both test files draw
def integer_rects(W, H):
    """Rectangles on whole pixels: overlapping, partly outside on each side, fully outside, zero-sized, up- and downscaled."""
    return [(1, 1, max(W // 2, 1), max(H // 2, 1)), (W // 4, H // 4, max(W // 2, 2), max(H // 2, 2)), (-3, 2, 8, 5), (W - 4, 1, 9, 6),
            (2, -2, 7, 4), (3, H - 2, 6, 5), (W + 2, 1, 5, 5), (-20, -20, 10, 10), (4, 4, 0, 7), (5, 5, 6, -1), (0, 0, W, H), (W // 3, 0, 3, H),
            (0, H // 2, W, 2), (2, 2, 5, 5), (W // 2, H // 2, 40, 30), (1, 0, 2, 2), (W - 2, H - 2, 2, 2)]


def fractional_rects(W, H):
    """The same ground with edges between pixel centres: offsets and sizes in quarters, never .5."""
    return [(1.25, 0.75, W / 2 + 0.25, H / 2 - 0.25), (W / 4 + 0.75, H / 4 + 0.25, W / 2 - 0.75, H / 2 + 0.75), (-3.25, 2.25, 8.75, 5.25),
            (W - 4.25, 1.75, 9.25, 6.75), (2.75, -2.25, 7.25, 4.75), (3.25, H - 2.25, 6.75, 5.25), (W + 2.25, 1.25, 5.25, 5.75),
            (4.25, 4.75, 0.0, 7.25), (0.25, 0.25, 0.25, 0.25), (W / 3 + 0.25, 0.75, 3.75, H - 1.25), (2.25, 2.75, 5.25, 5.75),
            (W / 2 + 0.75, H / 2 + 0.25, 40.25, 30.75), (1.75, 0.25, 2.25, 2.75), (-0.25, -0.75, W + 0.75, H + 1.25), (5.75, 1.25, 1.25, 1.75),
            (0.75, H / 2 + 0.25, W - 1.25, 2.25), (W - 2.25, H - 2.75, 2.75, 3.25)]


def child_sizes(k):
    """Sizes of child k's texture: equal to, smaller and larger than typical rectangles (1:1, up- and downscaled), one a single texel."""
    return [(8, 5), (40, 30), (3, 2), (17, 9), (1, 1), (64, 16), (5, 11)][k % 7]


def make_children(rng, n):
    """n child textures; every third one opaque, the rest with translucent content."""
    out = []
    for k in range(n):
        w, h = child_sizes(k)
        out.append(premultiplied(rng, w, h, opaque=(k % 3 == 2)))
    return out
