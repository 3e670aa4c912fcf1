"""Wall time of smr_renderer_update_scene + smr_renderer_sync for live text, in a fresh process, after warm-up, as the median of
50 updates.  Uses only calls every commit with a font book has, and the smelter_amd package of the directory it is started in (so a checkout
of another commit can be measured beside this one, on the same machine):
   python tools/text_update_time.py labels      32 one-line labels on a 1920 x 1080 output, ONE label changed per update (a scoreboard clock)
   python tools/text_update_time.py paragraph   one paragraph of about 1 500 glyphs in a 1280 x 720 node, changed every update (a ticker page)
-> one JSON line: the workload, the median / minimum / maximum in milliseconds, the glyph count of the paragraph, and the mean of the last
frame's bytes (two commits draw the same picture)."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.getcwd())
import numpy as np

from smelter_amd import fontbook, hip
from smelter_amd.renderer import Renderer

workload = sys.argv[1]
UPDATES, WARMUP = 50, 10
FONTS = os.path.join(os.getcwd(), "tests", "golden", "fonts")
WORDS = "live text clocks tickers subtitles scoreboards camera regie score goal half time break news weather sport".split()


def labels_scene(k):
    """4 columns x 8 rows of 400 x 40 labels; label k mod 32 shows the update's number."""
    kids = []
    for i in range(32):
        text = f"clock {k:05d}" if i == k % 32 else f"label {i} of the board"
        kids.append({"type": "view", "left": 40 + 460 * (i % 4), "top": 40 + 120 * (i // 4), "width": 400, "height": 40,
                     "children": [{"type": "text", "text": text, "font_size": 28.0, "width": 400.0, "height": 40.0, "color": "#FFFFFFFF", "background_color": "#00204080"}]})
    return 1920, 1080, json.dumps({"type": "view", "children": kids})


def paragraph_scene(k):
    rng = np.random.default_rng(k)
    text, glyphs = [], 0
    while glyphs < 1500:
        w = WORDS[int(rng.integers(0, len(WORDS)))]
        text.append(w)
        glyphs += len(w)
    body = " ".join(text)
    return 1280, 720, json.dumps({"type": "view", "children": [{"type": "text", "text": body, "font_size": 24.0, "line_height": 30.0, "wrap": "word", "width": 1280.0,
                                                                "height": 720.0, "color": "#FFFFFFFF", "background_color": "#101010FF"}]}), glyphs


ctx = hip.Context(0)
book = fontbook.NativeFontBook()
book.add_dir(FONTS)
r = Renderer(ctx)
r.set_fontbook(book)
make = labels_scene if workload == "labels" else paragraph_scene
times, n_glyphs = [], 0
for k in range(WARMUP + UPDATES):
    made = make(k)
    w, h, scene = made[:3]
    n_glyphs = made[3] if len(made) > 3 else 0
    r.sync()
    t0 = time.perf_counter()
    r.update_scene("out", w, h, scene, hip.FRAME_RGBA)
    r.sync()
    t1 = time.perf_counter()
    if k >= WARMUP:
        times.append((t1 - t0) * 1e3)
    r.render(0.04 * k, {})
picture = np.asarray(r.render(10.0, {})["out"].download()[0])
print(json.dumps({"tree": os.path.basename(os.getcwd()), "workload": workload, "updates": UPDATES, "median_ms": round(statistics.median(times), 3),
                  "min_ms": round(min(times), 3), "max_ms": round(max(times), 3), "paragraph_glyphs": n_glyphs, "mean_byte": round(float(picture.mean()), 4)}))
r.close()
book.close()
ctx.close()
