"""A WebView node's picture — a 1920 x 1080 page with four 640 x 360 children over it — drawn N times two ways, for one
rocprofv3 --kernel-trace --stats run each.  Uses the smelter_amd package of the directory it is started in (so a checkout of another commit
can be measured beside this one):
   python tools/web_view_cost.py web N       smr_web_view: one k_web_view launch per picture (this library)
   python tools/web_view_cost.py layouts N   what every commit has: smr_frame_to_rgba of the BGRA page (k_swizzle), then smr_apply_layouts of
                                             five texture layouts (k_apply_layouts)
-> one JSON line: the route, N, and the mean of the picture's bytes (the two routes draw the same picture)."""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.getcwd())
import numpy as np

from smelter_amd import _ffi, hip
from smelter_amd.scene import Layout

route, n = sys.argv[1], int(sys.argv[2])
W, H, CW, CH = 1920, 1080, 640, 360
RECTS = [(64.0, 60.0), (1216.0, 60.0), (64.0, 660.0), (1216.0, 660.0)]
rng = np.random.default_rng(9)


def premultiplied(w, h):
    px = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    px[..., :3] = (px[..., :3].astype(np.uint32) * px[..., 3:4] // 255).astype(np.uint8)
    return px


ctx = hip.Context(0)
page_px = premultiplied(W, H)
kids = [ctx.surface_from(premultiplied(CW, CH)) for _ in RECTS]
dst = ctx.surface(W, H)
if route == "web":
    fn = ctx.lib.smr_web_view
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(_ffi.WebRect), C.c_uint32, C.c_int]
    fn.restype = C.c_int
    page = ctx.surface_from(page_px)
    info = page.info()
    srcs = (C.c_void_p * 4)(*[k.handle for k in kids])
    rects = (_ffi.WebRect * 4)(*[_ffi.WebRect(x, y, float(CW), float(CH)) for x, y in RECTS])
    for _ in range(n):
        ctx._check(fn(ctx.handle, info.dptr, info.pitch, dst.handle, srcs, rects, 4, 0))
else:
    frame = ctx.frame(hip.FRAME_BGRA, W, H, [page_px])
    node = ctx.surface(W, H)

    def tex(i, left, top, w, h):
        return Layout(top, left, float(w), float(h), 0.0, [0.0] * 4, 0, i, [0.0] * 4, [0.0] * 4, 0.0, [0.0, 0.0, float(w), float(h)], 0.0, [])
    layouts = [tex(0, 0.0, 0.0, W, H)] + [tex(1 + i, x, y, CW, CH) for i, (x, y) in enumerate(RECTS)]
    for _ in range(n):
        ctx.frame_to_rgba(frame, node)
        ctx.apply_layouts(dst, layouts, [node] + kids)
ctx.sync()
print(json.dumps({"tree": os.path.basename(os.getcwd()), "route": route, "pictures": n, "mean_byte": round(float(dst.download().mean()), 4)}))
ctx.close()
