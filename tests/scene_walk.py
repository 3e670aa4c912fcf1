"""Seeded random walks of scene updates, frame changes and renders.  TEST INFRASTRUCTURE: a pure function of the seed, no GPU, no library.

`walk(seed)` is a list of ops (plain dicts, JSON-serialisable), generated up front, so a failure is reproduced by (seed, op index):
  {"op": "register_input" | "unregister_input", "input_id"}
  {"op": "update", "output_id", "width", "height", "format": "yuv420" | "nv12", "scene": smelter scene JSON}
  {"op": "unregister_output", "output_id"}
  {"op": "frames", "frames": {input_id: [format, w, h, content_seed] | None}}   the frames every following render is given (the whole set)
  {"op": "render", "pts_ns", "frame_pts": {input_id: pts_ns}, "settled": [output_id, ...]}
       frame_pts: the pts of the frames named (every other frame carries the render's pts): one older than the stream fallback timeout is
       dropped by populate_inputs.  settled: outputs the walk CLAIMS are settled at this pts (every transition over: a scene state that saw
       nothing but that output's last update lays out the same list, a new renderer renders the same frame) — claimed for the first frame
       past the last transition and for the last frame of such a run of frames at rest, not for every frame that is.
tests/test_scene_walk.py drives the C++ scene engine and the oracle's scene state through these and asserts what the walks cover;
tests/test_gpu_scene_walk.py drives renderers.  `walk_nodes(seed)` is the smaller walk without transitions whose scenes also hold a blur
Shader node, a static Image and a Text label (part 2 of the GPU module).  `walk_formats(seed)` is the walk of `walk`'s vocabulary over what a renderer
can be fed: a frame spec's format is any base format of smr_frame_format, a Y'CbCr one with its colour matrix behind an "@" ("p010@bt2020").

Scenes stay inside what tests/scene_json.to_oracle reads: View / Rescaler / Tiles over input streams, three layout levels deep at most.  A
scene is built from two generators, one for the STRUCTURE (kinds, child counts, which optional fields exist, component ids from a pool of
six shared by all kinds — so an id can come back as another kind) and one for the PARAMETERS (every number, colour, alignment, overflow mode,
the Tiles children): the same structure with new parameters is an update that matches by id, which is what transitions run on.  Numbers are
multiples of 1/4 (exact in f32), so nothing depends on how a parser rounds a decimal fraction.

Output resolution: smr_renderer_update_scene accepts a new resolution or format for a live output id (the output's frames are re-created:
csrc/host/renderer.cpp, "re-created at the new geometry when the lane next renders"), so the walk changes the resolution of "a" in place
and never unregisters it; "b" is unregistered and comes back, at another resolution and format.

Two things the walk does not emit because the reference rejects them: a component id used twice in one scene
(smelter-render/src/scene/validation.rs:48-72, validate_component_ids_uniqueness, per output) and an absolutely positioned component with both or neither of
top / bottom or left / right (smelter-api/src/video/component_into.rs:50-62, 161-173).  And one it leaves out on purpose: an output is
rendered at least once between its first update and its second (the reference keeps ONE last pts for all outputs, scene_state.rs:59-66; the
engine and the oracle keep one per output, so a transition started by the second update of an output that has never been rendered would
start at pts 0 here).  The root component carries no width / height: the root layout node's texture would take that size while the
layout keeps the output's (scene/layout.rs:245-262), and the output would be a rescaled copy of it, which oracle/transition.py does not restate.
"""
from __future__ import annotations

import copy

MS = 1_000_000
TIMEOUT_NS = 500 * MS          # the renderer's default stream_fallback_timeout (include/smr.h: smr_renderer_create)
SEEDS = [11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22]
NODE_SEEDS = [101, 102, 103, 104]
INPUT_IDS = ["in0", "in1", "in2", "in3"]
INPUT_SIZES = [(64, 36), (96, 54), (128, 72), (160, 90), (130, 74), (36, 64)]
INPUT_FORMATS = ["yuv420", "yuvj420", "nv12"]
OUTPUT_SIZES = [(192, 108), (256, 144), (130, 74), (384, 216)]
OUTPUT_FORMATS = ["yuv420", "nv12"]
EASINGS = ["linear", "bounce", "cubic_bezier"]
COMPONENT_IDS = ["c0", "c1", "c2", "c3", "c4", "c5"]
TILE_SLOTS = 8                 # the children of the k-th Tiles component of a scene take their ids from "s<k>_0" .. "s<k>_7"
OVERFLOWS = ["visible", "hidden", "fit", None]
H_ALIGNS = ["left", "center", "right", "justified", None]
V_ALIGNS = ["top", "center", "bottom", "justified", None]
ASPECTS = ["16:9", "4:3", "1:1", "9:16", None]
MAX_COMPONENTS = 22


class Rng:
    """splitmix64: the same numbers on every Python."""

    def __init__(self, seed):
        self.s = (int(seed) * 0xD1342543DE82EF95 + 1) & 0xFFFFFFFFFFFFFFFF
        self.s = self.u64()   # (the state is a hash of the seed: neighbouring seeds give unrelated streams, not shifted copies)

    def u64(self):
        self.s = (self.s + 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
        z = self.s
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
        return z ^ (z >> 31)

    def below(self, n):
        return self.u64() % n

    def between(self, a, b):
        """an integer in [a, b]"""
        return a + self.below(b - a + 1)

    def chance(self, p):
        return self.below(1000) < int(p * 1000)

    def pick(self, seq):
        return seq[self.below(len(seq))]

    def shuffled(self, seq):
        out = list(seq)
        for i in range(len(out) - 1, 0, -1):
            j = self.below(i + 1)
            out[i], out[j] = out[j], out[i]
        return out

    def quarter(self, lo, hi):
        """a multiple of 1/4 in [lo, hi]"""
        a, b = int(lo * 4), max(int(hi * 4), int(lo * 4))
        return self.between(a, b) / 4.0


def _colour(rp, alpha=None):
    a = rp.pick([255, 255, 128, 64]) if alpha is None else alpha
    return "#%02X%02X%02X%02X" % (rp.below(256), rp.below(256), rp.below(256), a)


def make_transition(r, long=False, interrupt=None):
    ms = r.between(150, 400) if long else r.between(40, 400)
    t = {"duration_ms": ms}
    kind = r.pick(EASINGS + [None])
    if kind == "cubic_bezier":
        t["easing_function"] = {"function_name": "cubic_bezier", "points": [r.below(17) / 16.0 for _ in range(4)]}
    elif kind is not None:
        t["easing_function"] = {"function_name": kind}
    si = r.pick([True, False, None]) if interrupt is None else interrupt
    if si is not None:
        t["should_interrupt"] = si
    return t


class _Builder:
    def __init__(self, struct_seed, param_seed, W, H):
        self.rs, self.rp, self.W, self.H = Rng(struct_seed), Rng(param_seed), W, H
        self.ids = self.rs.shuffled(COMPONENT_IDS)
        self.count = 0
        self.n_tiles = 0

    def _id(self, js):
        if self.ids and self.rs.chance(0.75):
            js["id"] = self.ids.pop()

    def _flip(self, v, a, b):
        return (b if v == a else a) if self.rp.chance(0.12) else v

    def _position(self, js, pw, ph, root):
        rs, rp = self.rs, self.rp
        if not root and rs.chance(0.3):
            vert, hor, rot = self._flip(rs.pick(["top", "bottom"]), "top", "bottom"), self._flip(rs.pick(["left", "right"]), "left", "right"), rs.chance(0.4)
            js[vert] = rp.quarter(-4, ph * 0.4)
            js[hor] = rp.quarter(-4, pw * 0.4)
            if rot:
                js["rotation"] = rp.quarter(-45, 45)
            if rs.chance(0.8):
                js["width"] = rp.quarter(pw * 0.2, pw * 0.8)
            if rs.chance(0.8):
                js["height"] = rp.quarter(ph * 0.2, ph * 0.8)
            return
        kind = 0 if root else rs.below(4)
        if kind == 1:
            js["width"] = rp.quarter(pw * 0.2, pw * 0.9)
        elif kind == 2:
            js["height"] = rp.quarter(ph * 0.2, ph * 0.9)
        elif kind == 3:
            js["width"], js["height"] = rp.quarter(pw * 0.2, pw * 0.9), rp.quarter(ph * 0.2, ph * 0.9)

    def _decor(self, js):
        rs, rp = self.rs, self.rp
        if rs.chance(0.4):
            js["border_radius"] = rp.quarter(0, 24)
        if rs.chance(0.35):
            js["border_width"] = rp.quarter(0, 6)
            js["border_color"] = _colour(rp)
        if rs.chance(0.25):
            js["box_shadow"] = [{"offset_x": rp.quarter(-8, 8), "offset_y": rp.quarter(-8, 8), "blur_radius": rp.quarter(0, 12), "color": _colour(rp)}
                                for _ in range(rp.between(1, 2))]

    def leaf(self):
        return {"type": "input_stream", "input_id": self.rp.pick(INPUT_IDS)}

    def child(self, depth, pw, ph):
        if depth >= 3 or self.count >= MAX_COMPONENTS:
            return self.leaf()
        k = self.rs.below(10)
        if k < 3:
            return self.leaf()
        if k < 6:
            return self.view(depth + 1, pw, ph)
        if k < 9:
            return self.rescaler(depth + 1, pw, ph)
        return self.tiles(depth + 1, pw, ph)

    def view(self, depth, pw, ph, root=False):
        rs, rp = self.rs, self.rp
        self.count += 1
        js = {"type": "view"}
        self._id(js)
        self._position(js, pw, ph, root)
        self._decor(js)
        d = rp.pick(["row", "column", None])
        if d:
            js["direction"] = d
        o = rp.pick(OVERFLOWS)
        if o:
            js["overflow"] = o
        bg = rp.between(1, 2) if root else rp.below(3)   # (a root is never invisible: a layout list is never empty)
        if bg:
            js["background_color"] = _colour(rp, 255 if bg == 1 else rp.pick([200, 128, 40]))
        pad = rs.below(5)
        if pad == 1:
            js["padding"] = rp.quarter(0, 10)
        elif pad == 2:
            js["padding_vertical"], js["padding_horizontal"] = rp.quarter(0, 10), rp.quarter(0, 10)
        elif pad == 3:
            js["padding"], js["padding_top"], js["padding_left"] = rp.quarter(0, 6), rp.quarter(0, 12), rp.quarter(0, 12)
        elif pad == 4:
            js["padding_horizontal"], js["padding_right"], js["padding_bottom"] = rp.quarter(0, 8), rp.quarter(0, 12), rp.quarter(0, 12)
        n = rs.between(1, 3) if root else rs.between(0, 3)
        cw, ch = (pw / max(n, 1), ph) if d != "column" else (pw, ph / max(n, 1))
        js["children"] = [self.child(depth, cw, ch) for _ in range(n)]
        return js

    def rescaler(self, depth, pw, ph, root=False):
        rs, rp = self.rs, self.rp
        self.count += 1
        js = {"type": "rescaler"}
        self._id(js)
        if not root and rs.chance(0.45):
            # a box that is an input size times 1, 1.5, 2 or 3: with that input inside, the resample plan sits at 1:1 or in a class window
            (iw, ih), f = rp.pick(INPUT_SIZES), rp.pick([1, 1.5, 2, 3])
            js["width"], js["height"] = iw * f, ih * f
            if rs.chance(0.4):
                js[self._flip(rs.pick(["top", "bottom"]), "top", "bottom")] = rp.quarter(0, 16)
                js[self._flip(rs.pick(["left", "right"]), "left", "right")] = rp.quarter(0, 16)
        else:
            self._position(js, pw, ph, root)
        self._decor(js)
        if root:
            js["border_width"], js["border_color"] = rp.quarter(1, 6), _colour(rp, 255)
        m = rp.pick(["fit", "fill", None])
        if m:
            js["mode"] = m
        ha, va = rp.pick(H_ALIGNS), rp.pick(V_ALIGNS)
        if ha:
            js["horizontal_align"] = ha
        if va:
            js["vertical_align"] = va
        js["child"] = self.leaf() if depth >= 3 or rs.chance(0.7) else self.view(depth + 1, pw, ph)
        return js

    def tiles(self, depth, pw, ph, root=False):
        rs, rp = self.rs, self.rp
        self.count += 1
        js = {"type": "tiles"}
        self._id(js)
        k = rs.below(4)
        if not root and k == 1:
            js["width"] = rp.quarter(pw * 0.4, pw)
        elif not root and k == 2:
            js["width"], js["height"] = rp.quarter(pw * 0.4, pw), rp.quarter(ph * 0.4, ph)
        if root or rp.chance(0.6):
            js["background_color"] = _colour(rp)
        a = rp.pick(ASPECTS)
        if a:
            js["tile_aspect_ratio"] = a
        if rp.chance(0.6):
            js["margin"] = rp.quarter(0, 8)
        if rp.chance(0.5):
            js["padding"] = rp.quarter(0, 6)
        ha, va = rp.pick(H_ALIGNS), rp.pick(V_ALIGNS)
        if ha:
            js["horizontal_align"] = ha
        if va:
            js["vertical_align"] = va
        kids = []
        nested = depth < 3 and rs.chance(0.25)
        pool = [f"s{self.n_tiles}_{j}" for j in range(TILE_SLOTS)]
        self.n_tiles += 1
        for i, tid in enumerate(rp.shuffled(pool)[:rp.between(1, 6)]):
            if nested and i == 0:
                c = self.rescaler(depth + 1, pw / 2, ph / 2) if rs.chance(0.5) else self.view(depth + 1, pw / 2, ph / 2)
                c.pop("id", None)
            else:
                c = {"type": "input_stream", "input_id": rp.pick(INPUT_IDS)}
            if rp.chance(0.85):
                c["id"] = tid
            kids.append(c)
        js["children"] = kids
        return js

    def grid(self):
        """A plain row or column of undecorated rescalers whose boxes are input sizes times 1, 1.5, 2 or 3, at whole-pixel offsets: with a 16:9
        input inside, a child is an aligned, unrotated, unmasked copy of a freshly resampled tile — what the compositor's copy tiles, the
        seam tiles between them and (SMR_OPT_DIRECT_OUTPUT) the resampler's direct-output jobs are for."""
        rs, rp = self.rs, self.rp
        self.count += 1
        js = {"type": "view", "direction": rp.pick(["row", "column"]), "background_color": _colour(rp, 255), "children": []}
        self._id(js)
        for _ in range(rs.between(2, 3)):
            self.count += 1
            (iw, ih), f = rp.pick(INPUT_SIZES[:4]), rp.pick([1, 1.5, 2, 3])
            c = {"type": "rescaler", "width": iw * f, "height": ih * f, "horizontal_align": "left", "vertical_align": "top",
                 "child": {"type": "input_stream", "input_id": rp.pick(INPUT_IDS)}}
            self._id(c)
            js["children"].append(c)
        return js

    def root(self):
        k = self.rs.below(10)
        if k < 5:
            return self.view(1, self.W, self.H, root=True)
        if k < 7:
            return self.tiles(1, self.W, self.H, root=True)
        if k < 8:
            return self.rescaler(1, self.W, self.H, root=True)
        return self.grid()


def build_scene(struct_seed, param_seed, W, H):
    return _Builder(struct_seed, param_seed, W, H).root()


def _layout_components(js, out=None):
    out = [] if out is None else out
    if js.get("type") in ("view", "rescaler", "tiles"):
        out.append(js)
        for c in js.get("children", []):
            _layout_components(c, out)
        if "child" in js:
            _layout_components(js["child"], out)
    elif js.get("type") == "shader":
        for c in js.get("children", []):
            _layout_components(c, out)
    return out


def add_transitions(scene, r, p=0.8, long=True, interrupt=None):
    """A `transition` on the components that carry an id (those a later update can continue)."""
    n = 0
    for c in _layout_components(scene):
        c.pop("transition", None)
        if "id" in c and r.chance(p):
            c["transition"] = make_transition(r, long, interrupt)
            n += 1
    return n


def max_transition_ms(scene):
    return max([c["transition"]["duration_ms"] for c in _layout_components(scene) if "transition" in c] or [0])


def _churn_tiles(scene, r):
    """Reorders, adds and removes children with ids of every Tiles component: -> number of Tiles changed."""
    n = 0
    for c in _layout_components(scene):
        if c["type"] != "tiles":
            continue
        kids = c["children"]
        used = {k.get("id") for k in kids}
        prefix = next((k["id"].split("_")[0] for k in kids if "_" in k.get("id", "")), None)
        how = r.below(3)
        if how == 0 and len(kids) > 1:
            kids[:] = r.shuffled(kids)
            if r.chance(0.5):
                kids.pop()
        elif how == 1 and len(kids) > 1:
            kids.pop(r.below(len(kids)))
        free = [f"{prefix}_{j}" for j in range(TILE_SLOTS) if f"{prefix}_{j}" not in used] if prefix else []
        if (how == 2 or len(kids) < 2) and len(kids) < 6 and free:
            kids.insert(r.below(len(kids) + 1), {"type": "input_stream", "input_id": r.pick(INPUT_IDS), "id": r.pick(free)})
        n += 1
    return n


def tiles_scene(r, W, H):
    """A Tiles root under a fixed id (what the Tiles churn phase starts from when the current scene has no Tiles)."""
    js = _Builder(r.u64(), r.u64(), W, H).tiles(1, W, H, root=True)
    if "id" not in js:
        used = {c.get("id") for c in _layout_components(js)}
        js["id"] = next(i for i in COMPONENT_IDS if i not in used)
    return js


# ----------------------------------------------------------------------------------------------------------------------------------- the walk
class _Walk:
    def __init__(self, seed, frames_target, transitions=True, scene_of=None):
        self.r = Rng(seed)
        self.ops = []
        self.pts = -1                 # the last rendered pts
        self.first = True
        self.registered = []
        self.frames = {}
        self.out = {}                 # output id -> {"W", "H", "format", "scene", "struct", "busy_until", "rendered"}
        self.renders = 0
        self.target = frames_target
        self.transitions = transitions
        self.scene_of = scene_of or build_scene

    # -- ops
    def register(self, iid):
        if iid not in self.registered:
            self.registered.append(iid)
            self.ops.append({"op": "register_input", "input_id": iid})

    def unregister(self, iid):
        if iid in self.registered:
            self.registered.remove(iid)
            self.ops.append({"op": "unregister_input", "input_id": iid})

    def new_frame(self, size=None, fmt=None):
        r = self.r
        w, h = size or r.pick(INPUT_SIZES)
        return [fmt or r.pick(INPUT_FORMATS), w, h, r.below(1 << 30)]

    def set_frames(self):
        self.ops.append({"op": "frames", "frames": copy.deepcopy(self.frames)})

    def update(self, oid, scene, W=None, H=None, fmt=None, struct=None):
        o = self.out.setdefault(oid, {"busy_until": 0, "rendered": False, "struct": None})
        if W is not None:
            o["W"], o["H"] = W, H
        if fmt is not None:
            o["format"] = fmt
        if struct is not None:
            o["struct"] = struct
        o["scene"] = copy.deepcopy(scene)
        # every transition this update can start or continue is over by then (a continued one ends when the one it continues would have)
        o["busy_until"] = max(o["busy_until"], max(self.pts, 0) + max_transition_ms(scene) * MS)
        self.ops.append({"op": "update", "output_id": oid, "width": o["W"], "height": o["H"], "format": o["format"], "scene": copy.deepcopy(scene)})

    def unregister_output(self, oid):
        if oid in self.out:
            del self.out[oid]
            self.ops.append({"op": "unregister_output", "output_id": oid})

    def render(self, step_ms=None, stale=None, past_transitions=False, mark=False):
        r = self.r
        if step_ms is None:
            step_ms = r.between(1, 200)
        pts = 0 if self.first and r.chance(0.5) else max(self.pts, 0) + step_ms * MS
        if past_transitions:
            pts = max([pts] + [o["busy_until"] + r.between(0, 40) * MS for o in self.out.values()])
        self.first = False
        self.pts = pts
        frame_pts = {}
        if stale is not None and pts > TIMEOUT_NS + 100 * MS:
            frame_pts[stale] = pts - TIMEOUT_NS - r.between(1, 100) * MS
        for o in self.out.values():
            o["rendered"] = True
        settled = sorted(k for k, o in self.out.items() if o["busy_until"] <= pts) if mark or past_transitions else []
        self.ops.append({"op": "render", "pts_ns": pts, "frame_pts": frame_pts, "settled": settled})
        self.renders += 1

    # -- scenes
    def fresh(self, oid, W=None, H=None, fmt=None):
        o = self.out.get(oid, {})
        W, H = (W, H) if W is not None else (o["W"], o["H"])
        for _ in range(8):   # (a structure with at least two components a later update can find again by id)
            struct = self.r.u64()
            scene = self.scene_of(struct, self.r.u64(), W, H)
            if sum(1 for c in _layout_components(scene) if "id" in c) >= 2:
                break
        if self.transitions and oid in self.out and self.r.chance(0.5):
            add_transitions(scene, self.r)
        self.update(oid, scene, W, H, fmt, struct)

    def moved(self, oid, with_transition=True, interrupt=None):
        """The current structure with new parameters: matches by id."""
        o = self.out[oid]
        scene = self.scene_of(o["struct"], self.r.u64(), o["W"], o["H"])
        if with_transition and self.transitions:
            add_transitions(scene, self.r, interrupt=interrupt)
        self.update(oid, scene)

    # -- phases
    def phase_transition(self, oid):
        """An update that starts transitions, a few frames into them, then a second update while they run."""
        r = self.r
        self.moved(oid)
        for _ in range(r.between(2, 3)):
            self.render(r.between(8, 45))
        o = self.out[oid]
        how = r.below(6)
        if how == 0:      # the same parameters again, with the id, without a transition object: the running one continues
            scene = copy.deepcopy(o["scene"])
            for c in _layout_components(scene):
                c.pop("transition", None)
            self.update(oid, scene)
        elif how == 1:    # the same parameters, a new transition object
            scene = copy.deepcopy(o["scene"])
            add_transitions(scene, r)
            self.update(oid, scene)
        elif how == 2:    # changed parameters, interrupting
            self.moved(oid, interrupt=True)
        elif how == 3:    # changed parameters, not interrupting: the running one goes on towards the new end
            self.moved(oid, interrupt=False)
        elif how == 4:    # changed parameters without a transition object
            self.moved(oid, with_transition=False)
        else:             # the id dropped: new components, no history
            scene = copy.deepcopy(o["scene"])
            for c in _layout_components(scene):
                if "transition" in c:
                    c.pop("id", None)
                    c.pop("transition", None)
            self.update(oid, scene)
        for _ in range(r.between(2, 4)):
            self.render(r.between(5, 50))

    def phase_tiles(self, oid):
        r = self.r
        o = self.out[oid]
        if not any(c["type"] == "tiles" and "id" in c for c in _layout_components(o["scene"])):
            scene = tiles_scene(r, o["W"], o["H"])
            self.update(oid, scene, struct=0)
            self.render(r.between(5, 40))
        for _ in range(r.between(1, 2)):
            scene = copy.deepcopy(self.out[oid]["scene"])
            _churn_tiles(scene, r)
            if self.transitions:
                add_transitions(scene, r, p=0.9)
            self.update(oid, scene)
            for _ in range(r.between(1, 2)):
                self.render(r.between(8, 70))

    def phase_rest(self, n=3, settled=False):
        self.render(past_transitions=settled)
        for i in range(n - 1):
            self.render(mark=settled and i == n - 2)

    def phase_content(self):
        for _ in range(3):
            for k, f in self.frames.items():
                if f is not None:
                    f[3] = self.r.below(1 << 30)
            self.set_frames()
            self.render()

    def phase_inputs(self, how=None):
        """An input changes size or format, is absent for a frame, or arrives stale."""
        r = self.r
        shown = [i for o in self.out.values() for i in input_ids_of(o["scene"]) if i in self.registered and self.frames.get(i) is not None]
        k = r.pick(shown) if shown else r.pick(self.registered) if self.registered else INPUT_IDS[0]
        how = r.below(4) if how is None else how
        if how == 2 and max(self.pts, 0) + 100 * MS <= TIMEOUT_NS + 100 * MS:
            how = 1   # (too early for a frame to be older than the timeout: absent instead)
        if how == 0:
            self.frames[k] = self.new_frame()
            self.set_frames()
            self.render()
        elif how == 1:
            keep = self.frames.get(k)
            self.frames[k] = None
            self.set_frames()
            self.render()
            self.frames[k] = keep if keep is not None else self.new_frame()
            self.set_frames()
            self.render()
        elif how == 2:
            self.render(r.between(100, 200), stale=k)
            self.render()
        else:
            f = self.frames.get(k) or self.new_frame()
            self.frames[k] = self.new_frame(size=(f[1], f[2]))   # the same size in another format (or the same)
            self.set_frames()
            self.render()

    def phase_registry(self, unregister=False):
        r = self.r
        if len(self.registered) > 1 and (unregister or (len(self.registered) > 2 and r.chance(0.6))):
            self.unregister(r.pick(self.registered))
        else:
            free = [i for i in INPUT_IDS if i not in self.registered]
            if free:
                k = r.pick(free)
                self.register(k)
                if self.frames.get(k) is None:
                    self.frames[k] = self.new_frame()
                    self.set_frames()
            elif self.registered:
                self.unregister(r.pick(self.registered))
        self.render()

    def phase_b(self):
        r = self.r
        if "b" in self.out:
            if r.chance(0.5):
                self.unregister_output("b")
                self.render()
            elif self.transitions:
                self.phase_transition("b")
            else:
                self.moved("b")
                self.render()
        else:
            W, H = r.pick(OUTPUT_SIZES)
            self.fresh("b", W, H, r.pick(OUTPUT_FORMATS))
            self.render()

    def phase_resolution(self):
        r = self.r
        o = self.out["a"]
        W, H = r.pick([s for s in OUTPUT_SIZES if s != (o["W"], o["H"])])
        if r.chance(0.5):
            self.fresh("a", W, H)
        else:
            o["W"], o["H"] = W, H
            self.moved("a")
        self.render()

    def run(self):
        r = self.r
        for k in INPUT_IDS[:3]:
            self.register(k)
        sizes = r.shuffled(INPUT_SIZES)
        for i, k in enumerate(INPUT_IDS):
            self.frames[k] = self.new_frame(size=sizes[i], fmt=INPUT_FORMATS[(i + r.below(3)) % 3]) if i < 3 else None
        self.set_frames()
        W, H = r.pick(OUTPUT_SIZES)
        self.fresh("a", W, H, "yuv420")
        self.render()
        # every walk: b alive then gone, a rest run, a content run, transitions with a second update, Tiles churn; the rest by lot
        must = ["b_on", "transition", "rest", "content", "tiles", "b_off", "inputs", "absent", "stale", "registry", "unregister", "settle", "transition", "resolution", "transition", "transition"]
        must = must[:2] + r.shuffled(must[2:])
        b_seen = False
        while must or self.renders < self.target - 3:
            ph = must.pop(0) if must else r.pick(["transition", "transition", "transition", "tiles", "inputs", "content", "registry", "b", "resolution", "rest", "fresh", "settle"])
            if ph == "b_on":
                if "b" not in self.out:
                    self.phase_b()
                b_seen = True
            elif ph == "b_off":
                if "b" not in self.out:
                    self.phase_b()
                self.render()
                self.unregister_output("b")
                self.render()
            elif ph == "b":
                self.phase_b()
            elif ph == "transition":
                if self.transitions:
                    self.phase_transition(r.pick(sorted(self.out)))
                else:
                    self.moved(r.pick(sorted(self.out)))
                    self.render()
            elif ph == "tiles":
                self.phase_tiles(r.pick(sorted(self.out)))
            elif ph == "rest":
                self.phase_rest(r.between(3, 4))
            elif ph == "settle":
                self.phase_rest(3, settled=True)
            elif ph == "content":
                self.phase_content()
            elif ph == "inputs":
                self.phase_inputs()
            elif ph == "absent":
                self.phase_inputs(1)
            elif ph == "stale":
                self.phase_inputs(2)
            elif ph == "registry":
                self.phase_registry()
            elif ph == "unregister":
                self.phase_registry(unregister=True)
            elif ph == "resolution":
                self.phase_resolution()
            elif ph == "fresh":
                self.fresh(r.pick(sorted(self.out)))
                self.render()
        assert b_seen
        if "b" in self.out:
            self.unregister_output("b")
        # the walk ends at rest: past every transition, nothing changing
        self.phase_rest(3, settled=True)
        return self.ops


def walk(seed, frames=40):
    return _Walk(seed, frames).run()


# ------------------------------------------------------------------------------------------------------- the walk with Shader / Image / Text nodes
IMAGE_ID, IMAGE_SIZE = "logo", (48, 40)       # the asset; the scenes show it in rescalers of other sizes
SHADER_ID = "soften"
LABEL = ("WALK", 2)                           # tests.scenes.label_glyphs arguments; the Text node is LABEL_W x LABEL_H


def _node_scene(struct_seed, param_seed, W, H):
    """View root: [a layout subtree, blur Shader over a nested View, the static Image inside a Rescaler, a Text label, a movable sibling]."""
    from tests import scenes
    rp = Rng(param_seed ^ 0x5555)
    sw, sh = rp.pick([(96, 54), (64, 48), (130, 74)])
    shader = {"type": "shader", "shader_id": SHADER_ID, "resolution": {"width": sw, "height": sh},
              "shader_param": {"type": "f32", "value": rp.pick([0.5, 1.0, 2.5, 4.0])},
              "children": [{"type": "view", "width": sw, "height": sh, "background_color": _colour(rp, 255),
                            "children": [{"type": "rescaler", "border_radius": rp.quarter(0, 12), "child": {"type": "input_stream", "input_id": rp.pick(INPUT_IDS)}}]}]}
    iw, ih = rp.pick([(24, 20), (72, 60), (96, 40), (50, 50)])
    image = {"type": "rescaler", "id": "img", "width": iw, "height": ih, "mode": rp.pick(["fit", "fill"]), "child": {"type": "image", "image_id": IMAGE_ID}}
    label = {"type": "view", "width": scenes.LABEL_W, "height": scenes.LABEL_H, "bottom": rp.quarter(0, 8), "left": rp.quarter(0, 8),
             "background_color": "#00000080", "children": [{"type": "text", "text": LABEL[0], "font_size": 16, "width": scenes.LABEL_W, "height": scenes.LABEL_H}]}
    sibling = {"type": "view", "id": "sib", "width": rp.quarter(10, 40), "height": rp.quarter(10, 40), "top": rp.quarter(0, H / 2), "right": rp.quarter(0, W / 2),
               "background_color": _colour(rp, 255)}
    b = _Builder(struct_seed, param_seed, W, H)
    sub = b.child(1, W / 2, H / 2)
    kids = [sub, shader, image, label, sibling]
    return {"type": "view", "direction": rp.pick(["row", "column"]), "overflow": rp.pick(["visible", "hidden"]), "background_color": _colour(rp, 255),
            "children": kids}


def move_sibling(scene, r):
    """The same scene with nothing but the `sib` view moved."""
    out = copy.deepcopy(scene)
    for c in out["children"]:
        if c.get("id") == "sib":
            c["top"], c["right"] = c["top"] + r.between(1, 12), c["right"] + r.between(1, 12)
    return out


class _NodeWalk(_Walk):
    def render(self, step_ms=None, stale=None, past_transitions=False, mark=False):
        # no transitions: every frame is settled; claimed for every third and for the one after an update that only moves a sibling
        after_sibling = bool(self.ops) and self.ops[-1].get("only_moves_a_sibling", False)
        super().render(step_ms, stale, past_transitions, mark or after_sibling or self.renders % 3 == 0)

    def run(self):
        r = self.r
        for k in INPUT_IDS[:3]:
            self.register(k)
        for i, k in enumerate(INPUT_IDS):
            self.frames[k] = self.new_frame() if i < 3 else None
        self.set_frames()
        W, H = r.pick([s for s in OUTPUT_SIZES if s != (130, 74)])
        self.fresh("a", W, H, "yuv420")
        self.render()
        must = r.shuffled(["sibling", "b_on", "content", "inputs", "b_off", "moved", "registry", "sibling", "rest", "fresh"])
        while self.renders < self.target - 2:
            ph = must.pop(0) if must else r.pick(["sibling", "moved", "content", "inputs", "fresh", "rest", "registry"])
            if ph == "sibling":
                self.update("a", move_sibling(self.out["a"]["scene"], r))
                self.ops[-1]["only_moves_a_sibling"] = True
                self.render()
            elif ph == "b_on" and "b" not in self.out:
                W, H = r.pick([s for s in OUTPUT_SIZES if s != (130, 74)])
                self.fresh("b", W, H, r.pick(OUTPUT_FORMATS))
                self.render()
            elif ph == "b_off" and "b" in self.out:
                self.unregister_output("b")
                self.render()
            elif ph == "moved":
                self.moved(r.pick(sorted(self.out)))
                self.render()
            elif ph == "content":
                self.phase_content()
            elif ph == "inputs":
                self.phase_inputs()
            elif ph == "registry":
                self.phase_registry()
            elif ph == "rest":
                self.phase_rest(3)
            elif ph == "fresh":
                self.fresh(r.pick(sorted(self.out)))
                self.render()
        self.phase_rest(2)
        return self.ops


def walk_nodes(seed, frames=25):
    """No transitions: a scene is a pure function of its last update, every frame is settled."""
    return _NodeWalk(seed, frames, transitions=False, scene_of=_node_scene).run()


# ------------------------------------------------------------------------------------------------- the walk of input formats, matrices and alpha
FORMAT_SEEDS = [201, 202, 203, 204, 205, 206, 207, 208]   # odd: MODE_CPU_OPTIMIZED contexts (the oracle at srgb=False), even: MODE_GPU_OPTIMIZED
# the base formats, by their smr_frame_format value (include/smr.h)
BASE_FORMATS = ["yuv420", "yuv422", "yuv444", "yuvj420", "uyvy422", "yuyv422", "nv12", "bgra", "argb", "rgba", "p010", "yuv420p10", "yuv422p10", "p210", "v210"]
MATRICES = [None, "bt601", "bt2020"]            # None: untagged (BT.709); carried in a spec's format string as "p010@bt2020"
ODD_SIZES = [(37, 21), (38, 21), (50, 22), (131, 75)]   # odd widths and heights; widths that fill neither a v210 group of 6 nor 48 pixels
FORMAT_SIZES = INPUT_SIZES + ODD_SIZES
ALPHA_FORMATS = ["bgra", "argb", "rgba"]
YCBCR_FORMATS = [f for f in BASE_FORMATS if f not in ALPHA_FORMATS]
RGB12_FORMATS = ["yuv420", "yuvj420", "nv12"]                 # 8-bit 4:2:0: what the block converter and the RGB12 node take
OTHER_8BIT_FORMATS = ["yuv422", "yuv444", "uyvy422", "yuyv422"]
PACKED_8BIT_FORMATS = ["uyvy422", "yuyv422"]                  # one texel per pixel pair: an even width
HI_FORMATS = ["p010", "yuv420p10", "yuv422p10", "p210", "v210"]
CONVERTER_FAMILIES = {"yuv420": "block420", "yuvj420": "block420", "nv12": "block420", "yuv422": "planar", "yuv444": "planar", "uyvy422": "packed",
                      "yuyv422": "packed", "bgra": "swizzle", "argb": "swizzle", "p010": "hi420", "yuv420p10": "hi420", "yuv422p10": "hi422",
                      "p210": "hi422", "v210": "v210"}   # (rgba: premultiplied on ingest, none of the seven)


def split_format(fmt):
    """"p010@bt2020" -> ("p010", "bt2020"); "nv12" -> ("nv12", None)"""
    base, _, matrix = fmt.partition("@")
    return base, matrix or None


def join_format(base, matrix):
    return base if matrix is None else f"{base}@{matrix}"


def format_mode(seed):
    return "cpu_optimized" if seed % 2 else "gpu_optimized"


def format_accepts(base, w, h):
    return w % 2 == 0 if base in PACKED_8BIT_FORMATS else True


def alpha_everywhere_255(spec):
    """One BGRA / ARGB / RGBA frame in four is opaque in every pixel."""
    return spec[3] % 4 == 0


def _format_scene(struct_seed, param_seed, W, H):
    """build_scene, and over a View root often one more child: an absolutely positioned Rescaler "ov" over its siblings, so that an input
    with alpha is composited over other inputs (a wrongly opaque hand-off shows in the picture)."""
    js = build_scene(struct_seed, param_seed, W, H)
    rs, rp = Rng(struct_seed ^ 0xF0F0), Rng(param_seed ^ 0x0F0F)
    if js["type"] == "view" and rs.chance(0.7):
        js["children"].append({"type": "rescaler", "id": "ov", "top": rp.quarter(0, H * 0.3), "left": rp.quarter(0, W * 0.3), "width": rp.quarter(W * 0.3, W * 0.7),
                               "height": rp.quarter(H * 0.3, H * 0.7), "mode": rp.pick(["fit", "fill"]), "child": {"type": "input_stream", "input_id": rp.pick(INPUT_IDS)}})
    return js


def overlay_input(scene):
    for c in scene.get("children", []):
        if c.get("id") == "ov" and c["type"] == "rescaler":
            return c["child"]["input_id"]
    return None


class _FormatWalk(_Walk):
    def __init__(self, seed, frames_target):
        super().__init__(seed, frames_target, scene_of=_format_scene)
        self.seed = seed

    def new_frame(self, size=None, fmt=None, among=None):
        r = self.r
        if fmt is None:
            pool = [b for b in (among or BASE_FORMATS) if size is None or format_accepts(b, *size)]
            base = r.pick(pool)
            fmt = join_format(base, r.pick(MATRICES) if base in YCBCR_FORMATS else None)
        if size is None:
            size = r.pick([s for s in FORMAT_SIZES if format_accepts(split_format(fmt)[0], *s)])
        return [fmt, size[0], size[1], r.below(1 << 30)]

    def seed_with_alpha(self):
        s = self.r.below(1 << 30)
        return s + 1 if s % 4 == 0 else s

    def shown(self):
        return [i for o in self.out.values() for i in input_ids_of(o["scene"]) if i in self.registered and self.frames.get(i) is not None]

    def phase_formats(self, how):
        """One input id changes between two consecutive renders: (a) opaque Y'CbCr <-> a format with alpha, (b) an RGB12-capable format <-> another
        8-bit Y'CbCr one, (c) 8 <-> 10 bits, all at the same size and back again; (d) nothing but the matrix, on new and on identical
        content; (e) the same format at a new size, an odd one first."""
        r = self.r
        shown = self.shown()
        k = r.pick(shown) if shown else self.registered[0]
        f = self.frames.get(k) or self.new_frame()
        size = (f[1], f[2])
        base, matrix = split_format(f[0])
        if how in "abc":
            pools = {"a": (YCBCR_FORMATS, ALPHA_FORMATS), "b": (RGB12_FORMATS, OTHER_8BIT_FORMATS), "c": (RGB12_FORMATS + OTHER_8BIT_FORMATS, HI_FORMATS)}[how]
            if base not in pools[0] and base not in pools[1]:
                f = self.new_frame(size, among=pools[0])
                self.frames[k] = f
                self.set_frames()
                self.render()
                base = split_format(f[0])[0]
            there = pools[1] if base in pools[0] else pools[0]
            g = self.new_frame(size, among=there)
            if how == "a":
                (g if there is ALPHA_FORMATS else f)[3] = self.seed_with_alpha()
                if there is not ALPHA_FORMATS:   # (the frame with alpha is the earlier one: shown once more with alpha for certain)
                    self.frames[k] = f
                    self.set_frames()
                    self.render()
            self.frames[k] = g
            self.set_frames()
            self.render()
            self.frames[k] = [f[0], f[1], f[2], self.seed_with_alpha() if how == "a" else r.below(1 << 30)]
            self.set_frames()
            self.render()
        elif how == "d":
            if base not in YCBCR_FORMATS:
                f = self.new_frame(size, among=YCBCR_FORMATS)
                self.frames[k] = f
                self.set_frames()
                self.render()
                base, matrix = split_format(f[0])
            others = [m for m in MATRICES if m != matrix]
            self.frames[k] = [join_format(base, others[0]), f[1], f[2], r.below(1 << 30)]   # new content under a new matrix
            self.set_frames()
            self.render()
            self.frames[k] = [join_format(base, others[1]), f[1], f[2], self.frames[k][3]]  # the same content under the third
            self.set_frames()
            self.render()
        else:
            sizes = [s for s in ODD_SIZES if s != size and format_accepts(base, *s)]
            self.frames[k] = [f[0], *r.pick(sizes), r.below(1 << 30)]
            self.set_frames()
            self.render()
            self.frames[k] = [f[0], *r.pick([s for s in FORMAT_SIZES if s != tuple(self.frames[k][1:3]) and format_accepts(base, *s)]), r.below(1 << 30)]
            self.set_frames()
            self.render()

    def phase_mix(self, how):
        """Every input gets a new frame: two of one base format under different matrices, or three converter families at once; then
        the tags move to other inputs."""
        r = self.r
        ids = r.shuffled(INPUT_IDS)
        if how == "pair":
            base = r.pick(YCBCR_FORMATS)
            tags = r.shuffled(MATRICES)
            bases = [base, base, r.pick([b for b in YCBCR_FORMATS if CONVERTER_FAMILIES[b] != CONVERTER_FAMILIES[base]]), r.pick(BASE_FORMATS)]
        else:
            fams = r.shuffled(sorted(set(CONVERTER_FAMILIES.values())))[:4]
            bases = [r.pick([b for b in BASE_FORMATS if CONVERTER_FAMILIES.get(b) == fam]) for fam in fams]
            tags = [r.pick(MATRICES) for _ in range(3)]
        for turn in range(3):
            for i, (k, b) in enumerate(zip(ids, bases)):
                tag = tags[(i + turn) % len(tags)] if b in YCBCR_FORMATS else None
                old = self.frames.get(k)
                if turn and old is not None:   # the same planes' geometry, the tag of its neighbour, new content on every second input
                    self.frames[k] = [join_format(b, tag), old[1], old[2], old[3] if i % 2 else r.below(1 << 30)]
                else:
                    self.frames[k] = self.new_frame(fmt=join_format(b, tag))
            self.set_frames()
            self.render()

    def class_boxes(self):
        """(input id, size) of every Rescaler of a live scene whose box is one of the first four INPUT_SIZES times 1.5, 2 or 3 and holds an input stream:
        with a frame of that size inside, the resample plan sits in a class window of the matrix-core resampler."""
        out = []
        for o in self.out.values():
            for c in _layout_components(o["scene"]):
                if c["type"] == "rescaler" and c["child"]["type"] == "input_stream" and "width" in c and "height" in c:
                    out += [(c["child"]["input_id"], s) for s in INPUT_SIZES[:4] for f in (1.5, 2, 3) if (c["width"], c["height"]) == (s[0] * f, s[1] * f)]
        return out

    def phase_node(self):
        """One source index between the node textures the resampler reads: an 8-bit 4:2:0 frame in a class window (the RGB12 node where the library
        chooses it), then at the same size another 8-bit format, 10 bits, alpha (the RGBA8 node), 4:2:0 under another matrix, and a new plan."""
        r = self.r
        for _ in range(12):
            boxes = self.class_boxes()
            if boxes:
                break
            self.fresh("a")
        if not boxes:
            return self.render()
        k, size = r.pick(boxes)
        self.register(k)
        tags = r.shuffled(MATRICES)
        for i, pool in enumerate([RGB12_FORMATS, OTHER_8BIT_FORMATS, RGB12_FORMATS, HI_FORMATS, RGB12_FORMATS, ALPHA_FORMATS, RGB12_FORMATS]):
            base = r.pick(pool)
            self.frames[k] = [join_format(base, tags[i % 3] if base in YCBCR_FORMATS else None), size[0], size[1], self.seed_with_alpha()]
            self.set_frames()
            self.render()
        self.moved(r.pick(sorted(self.out)), with_transition=False)
        self.render()

    def phase_overlay(self):
        """A scene with the overlay, its input in a format with alpha, the input below it changing."""
        r = self.r
        for _ in range(12):
            if overlay_input(self.out["a"]["scene"]) is not None:
                break
            self.fresh("a")
        k = overlay_input(self.out["a"]["scene"])
        if k is None:
            return self.render()
        self.register(k)
        size = r.pick(FORMAT_SIZES)
        for _ in range(3):
            self.frames[k] = [r.pick(ALPHA_FORMATS), size[0], size[1], self.seed_with_alpha()]
            for j in self.shown():
                if j != k and r.chance(0.5):
                    self.frames[j] = self.new_frame()
            self.set_frames()
            self.render()

    def run(self):
        r = self.r
        for k in INPUT_IDS[:3]:
            self.register(k)
        for i, k in enumerate(INPUT_IDS):   # (the first frames of consecutive seeds go through the base formats three at a time)
            self.frames[k] = self.new_frame(among=[BASE_FORMATS[(3 * self.seed + i) % len(BASE_FORMATS)]]) if i < 3 else None
        self.set_frames()
        W, H = r.pick(OUTPUT_SIZES)
        self.fresh("a", W, H, "yuv420")
        self.render()
        must = ["b_on", "transition", "a", "b", "c", "d", "e", "pair", "families", "overlay", "node", "content", "b_off", "absent", "stale", "registry", "settle", "tiles",
                "resolution", "inputs"]
        must = must[:2] + r.shuffled(must[2:])
        while must or self.renders < self.target - 3:
            ph = must.pop(0) if must else r.pick(["a", "b", "c", "d", "e", "pair", "families", "overlay", "node", "transition", "inputs"])
            if ph == "b_on":
                if "b" not in self.out:
                    self.phase_b()
            elif ph == "b_off":
                if "b" not in self.out:
                    self.phase_b()
                self.render()
                self.unregister_output("b")
                self.render()
            elif ph == "transition":
                self.phase_transition(r.pick(sorted(self.out)))
            elif ph in ("a", "b", "c", "d", "e"):
                self.phase_formats(ph)
            elif ph in ("pair", "families"):
                self.phase_mix(ph)
            elif ph == "overlay":
                self.phase_overlay()
            elif ph == "node":
                self.phase_node()
            elif ph == "tiles":
                self.phase_tiles(r.pick(sorted(self.out)))
            elif ph == "settle":
                self.phase_rest(3, settled=True)
            elif ph == "content":
                self.phase_content()
            elif ph == "inputs":
                self.phase_inputs()
            elif ph == "absent":
                self.phase_inputs(1)
            elif ph == "stale":
                self.phase_inputs(2)
            elif ph == "registry":
                self.phase_registry()
            elif ph == "resolution":
                self.phase_resolution()
        if "b" in self.out:
            self.unregister_output("b")
        self.phase_rest(3, settled=True)
        return self.ops


def walk_formats(seed, frames=30):
    """The walk over what a renderer can be fed: every base format, the three matrices, odd and ragged sizes, alpha over other inputs."""
    return _FormatWalk(seed, frames).run()


# ----------------------------------------------------------------------------------------------------------------------------------- helpers
def _alpha_field(w, h, seed):
    """Alpha 0 .. 255 with runs of 0 and of 255 (a dozen pixels along a row); 255 everywhere on one frame in four."""
    import numpy as np
    yy, xx = np.mgrid[0:h, 0:w]
    if seed % 4 == 0:
        return np.full((h, w), 255, np.int64)
    return np.clip((xx * 5 + yy * 3 + seed % 251) % 384 - 64, 0, 255)


def _format_planes(base, w, h, seed):
    """The planes of the formats the first walks do not use: the same gradients under noise; 10-bit codes with their low two bits in use and seeded
    junk in every bit the format ignores."""
    import numpy as np
    from tests import hi422_model
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    if base in ALPHA_FORMATS:
        a = _alpha_field(w, h, seed)
        c = [np.clip((xx * (3 + i) + yy * (2 + i) + seed % (89 + i)) % 256 + rng.integers(-24, 25, (h, w)), 0, 255) for i in range(3)]
        if base == "rgba":   # straight alpha
            return [np.ascontiguousarray(np.stack(c + [a], -1).astype(np.uint8))]
        r_, g_, b_ = [ci * a // 255 for ci in c]   # premultiplied: colour <= alpha
        order = [b_, g_, r_, a] if base == "bgra" else [a, r_, g_, b_]
        return [np.ascontiguousarray(np.stack(order, -1).astype(np.uint8))]
    y = np.clip(16 + (xx * 3 + yy * 2 + seed % 97) % 219 + rng.integers(-24, 25, (h, w)), 16, 235)
    if base in ("yuv444",):
        ch, cw = h, w
    elif base in ("yuv422", "yuv422p10", "p210"):
        ch, cw = h, w // 2
    elif base in PACKED_8BIT_FORMATS or base == "v210":
        ch, cw = h, (w + 1) // 2
    else:
        ch, cw = h // 2, w // 2
    cy, cx = np.mgrid[0:ch, 0:cw]
    u = np.clip(128 + 60 * np.sin(cx / 7.0 + seed % 13) + rng.integers(-12, 13, (ch, cw)), 16, 240).astype(np.int64)
    v = np.clip(128 + 60 * np.cos(cy / 5.0 + seed % 11) + rng.integers(-12, 13, (ch, cw)), 16, 240).astype(np.int64)
    if base in ("yuv422", "yuv444"):
        return [y.astype(np.uint8), u.astype(np.uint8), v.astype(np.uint8)]
    if base == "uyvy422":
        return [np.ascontiguousarray(np.stack([u, y[:, 0::2], v, y[:, 1::2]], -1).astype(np.uint8))]
    if base == "yuyv422":
        return [np.ascontiguousarray(np.stack([y[:, 0::2], u, y[:, 1::2], v], -1).astype(np.uint8))]
    # 10 bits: the byte's code times four plus two more bits
    y, u, v = (c * 4 + rng.integers(0, 4, c.shape) for c in (y, u, v))
    junk = lambda shape: rng.integers(0, 64, shape)   # noqa: E731
    if base in ("p010", "p210"):    # the code in the high ten bits, junk in the low six
        uv = np.stack([u, v], -1)
        return [((y << 6) | junk(y.shape)).astype(np.uint16), np.ascontiguousarray(((uv << 6) | junk(uv.shape)).astype(np.uint16))]
    if base in ("yuv420p10", "yuv422p10"):   # the code in the low ten bits, junk in the high six
        return [(c | (junk(c.shape) << 10)).astype(np.uint16) for c in (y, u, v)]
    assert base == "v210", base
    n = hi422_model.groups(w)
    return [hi422_model.v210_pack(y, u, v, junk=rng.integers(0, 4, (h, 4 * n)), beyond=rng.integers(0, 1024, (h, 6 * n)))]


def frame_planes(spec):
    """[format, w, h, content_seed] -> the planes of that frame (numpy, made on demand): gradients under noise of +-24 codes, so a stale or
    misplaced tile is many LSB wrong.  A matrix tag ("nv12@bt601") changes no plane."""
    import numpy as np
    fmt, w, h, seed = spec
    fmt = split_format(fmt)[0]
    if fmt not in INPUT_FORMATS:
        return _format_planes(fmt, w, h, seed)
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    lo, hi = (0, 255) if fmt == "yuvj420" else (16, 235)
    y = np.clip(lo + (xx * 3 + yy * 2 + seed % 97) % (hi - lo) + rng.integers(-24, 25, (h, w)), lo, hi).astype(np.uint8)
    cy, cx = np.mgrid[0:h // 2, 0:w // 2]
    clo, chi = (0, 255) if fmt == "yuvj420" else (16, 240)
    u = np.clip(128 + 60 * np.sin(cx / 7.0 + seed % 13) + rng.integers(-12, 13, (h // 2, w // 2)), clo, chi).astype(np.uint8)
    v = np.clip(128 + 60 * np.cos(cy / 5.0 + seed % 11) + rng.integers(-12, 13, (h // 2, w // 2)), clo, chi).astype(np.uint8)
    if fmt == "nv12":
        return [y, np.ascontiguousarray(np.stack([u, v], axis=-1))]
    return [y, u, v]


def visible_frames(op_render, frames, registered):
    """populate_inputs (render_loop.rs:19-42): input id -> frame spec for the inputs that have a texture at this render — registered, a
    frame present, and its pts not older than the stream fallback timeout."""
    pts = op_render["pts_ns"]
    out = {}
    for k, f in frames.items():
        if f is None or k not in registered:
            continue
        if op_render["frame_pts"].get(k, pts) < max(pts - TIMEOUT_NS, 0):
            continue
        out[k] = f
    return out


def input_ids_of(scene):
    """input_id of every input stream under a layout root that is not below a Shader node, in order of appearance: the root layout node's children
    for a scene of layout components only."""
    out = []

    def visit(c):
        if c["type"] == "input_stream":
            out.append(c["input_id"])
        for k in c.get("children", []):
            visit(k)
        if "child" in c:
            visit(c["child"])
    visit(scene)
    return out


class OracleOutputs:
    """The independent witness: one oracle.transition.SceneState per live output, fed through tests/scene_json.to_oracle."""

    def __init__(self):
        self.state, self.inputs, self.info = {}, {}, {}

    def update(self, op):
        from oracle import transition as T
        from tests import scene_json
        root, ids = scene_json.to_oracle(op["scene"])
        st = self.state.setdefault(op["output_id"], T.SceneState())
        st.update(root, op["width"], op["height"])
        self.inputs[op["output_id"]] = ids
        self.info[op["output_id"]] = op
        return ids

    def unregister(self, oid):
        for d in (self.state, self.inputs, self.info):
            d.pop(oid, None)

    def resolutions(self, oid, visible):
        return [(visible[i][1], visible[i][2]) if i in visible else None for i in self.inputs[oid]]

    def layouts(self, oid, pts_ns, visible, srgb=True):
        return self.state[oid].layouts(pts_ns, self.resolutions(oid, visible), srgb=srgb)

    def fresh_layouts(self, oid, pts_ns, visible, srgb=True):
        """What a scene state that saw nothing but this output's last update lays out."""
        from oracle import transition as T
        from tests import scene_json
        op = self.info[oid]
        st = T.SceneState()
        st.update(scene_json.to_oracle(op["scene"])[0], op["width"], op["height"])
        return st.layouts(pts_ns, self.resolutions(oid, visible), srgb=srgb)
