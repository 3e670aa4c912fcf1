"""A 16-sticker overlay scene (profiles/r13_sticker_rate.txt): drained frames/s of the renderer loop and the image pass's launch
count.  Uses the smelter_amd package of the directory it is started in (so a checkout of another commit can be measured beside this one):
   python tools/sticker_rate.py animated|static LEGS FRAMES   -> one JSON line   (static: the stickers as static images, what every commit has)"""
import json
import os
import sys
import time

sys.path.insert(0, os.getcwd())
import numpy as np

from smelter_amd import hip
from smelter_amd.renderer import Renderer

mode, legs, frames = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
MS = 1_000_000
W, H = 1280, 720
ctx = hip.Context(0)
r = Renderer(ctx)
rng = np.random.default_rng(3)
kids = []
for i in range(16):
    asset = rng.integers(0, 256, (8, 64, 64, 4), dtype=np.uint8)
    if mode == "animated":
        r.register_animated_image(f"s{i}", asset, [40 * MS] * 8)
    else:
        r.register_image(f"s{i}", asset[0])
    kids.append({"type": "view", "top": 20 + 170 * (i // 4), "left": 40 + 300 * (i % 4), "width": 96, "height": 96,
                 "children": [{"type": "image", "image_id": f"s{i}", "width": 96, "height": 96}]})
r.update_scene("out", W, H, {"type": "view", "background_color": "#203040FF", "children": kids})
packed = r.make_frame_set({})
pts = 0
for _ in range(300):
    r.render_packed(pts, packed)
    pts += 33 * MS
r.sync()
rates = []
for _ in range(legs):
    t0 = time.perf_counter()
    for _ in range(frames):
        r.render_packed(pts, packed)
        pts += 33 * MS
    r.sync()
    rates.append(frames / (time.perf_counter() - t0))
launches = r.image_launches() if hasattr(r, "image_launches") else None
print(json.dumps({"tree": os.path.basename(os.getcwd()), "mode": mode, "frames_per_s": [round(x, 1) for x in rates], "image_launches": launches}))
r.close()
ctx.close()
