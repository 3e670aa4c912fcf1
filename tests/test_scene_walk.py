"""Random walks of scene updates (tests/scene_walk.py) through BOTH restatements of the reference's scene state, frame by frame, no GPU:
the product's C++ scene engine (smelter_amd.scene.Scene) and the oracle's (oracle.transition.SceneState over tests/scene_json.to_oracle).
At every rendered pts of every live output both are asked for the root's flattened layout list, with that frame's input resolutions (None for
an absent, stale or unregistered input), and the lists must agree word for word (tests.test_scene_engine.assert_same_layouts), in both
rendering modes.  Outputs are independent scenes: one witness pair each.

What this can see: any order of updates, renders and input changes on which the two restatements — written independently from the Rust —
lay a scene out differently, by one ulp of one coordinate.  What it cannot: an error both share (each is pinned to the reference on its own
by the corpus scenes and hand-computed layouts of tests/test_oracle_transition.py), and anything below the layout list (the kernels:
tests/test_gpu_scene_walk.py).

The second half asserts, from the op lists and the oracle alone, that the walks contain what they were written to contain (conditions, not
measurements): see test_the_walks_cover_what_they_claim."""
import inspect

import pytest

from oracle import oracle as orc
from smelter_amd import _ffi
from smelter_amd.scene import Scene
from tests import scene_walk as SW
from tests.test_scene_engine import assert_same_layouts

# (an absent input has size 0 x 0: the reference's layout arithmetic divides by it, and so does the oracle's)
pytestmark = [pytest.mark.filterwarnings("ignore:invalid value encountered:RuntimeWarning"),
              pytest.mark.filterwarnings("ignore:divide by zero encountered:RuntimeWarning")]


def _max_layouts():
    """The default a context is created with (smelter_amd/hip.py Context, = SMR_DEFAULT_MAX_LAYOUTS of include/smr.h)."""
    from smelter_amd import hip
    return inspect.signature(hip.Context.__init__).parameters["max_layouts"].default


def _same_lists(a, b):
    return len(a) == len(b) and bytes(orc.pack_layouts(a)) == bytes(orc.pack_layouts(b)) if len(a) else len(b) == 0


def _nodes(n, out=None):
    out = [] if out is None else out
    if n is not None:
        out.append(n)
        for c in n.children:
            _nodes(c, out)
    return out


def _unfinished(state, pts_ns):
    """Nodes of an oracle scene state whose transition still runs at pts_ns."""
    return [n for n in _nodes(state.root) if n.transition is not None and not n.transition.is_finished(pts_ns)]


@pytest.mark.parametrize("mode", ["gpu_optimized", "cpu_optimized"])
@pytest.mark.parametrize("seed", SW.SEEDS)
def test_engine_and_oracle_agree_on_every_frame_of_a_walk(seed, mode):
    srgb = mode == "gpu_optimized"
    cmode = _ffi.MODE_GPU_OPTIMIZED if srgb else _ffi.MODE_CPU_OPTIMIZED
    ops = SW.walk(seed)
    oracle, engines = SW.OracleOutputs(), {}
    registered, frames, checked = set(), {}, 0
    for k, op in enumerate(ops):
        if op["op"] == "register_input":
            registered.add(op["input_id"])
        elif op["op"] == "unregister_input":
            registered.discard(op["input_id"])
        elif op["op"] == "frames":
            frames = op["frames"]
        elif op["op"] == "unregister_output":
            oracle.unregister(op["output_id"])
            engines.pop(op["output_id"]).close()
        elif op["op"] == "update":
            ids = oracle.update(op)
            graph = engines.setdefault(op["output_id"], Scene()).update(op["scene"], op["width"], op["height"])
            assert [graph[c].ref_id for c in graph[0].children] == ids, (seed, k)
        elif op["op"] == "render":
            vis = SW.visible_frames(op, frames, registered)
            for oid in sorted(engines):
                want = oracle.layouts(oid, op["pts_ns"], vis, srgb=srgb)
                arr, n, w, h = engines[oid].node_layouts(0, op["pts_ns"], oracle.resolutions(oid, vis), cmode)
                assert (w, h) == (oracle.info[oid]["width"], oracle.info[oid]["height"])
                try:
                    assert_same_layouts(arr, n, want)
                except AssertionError as e:
                    raise AssertionError(f"seed {seed} op {k} output {oid!r} pts {op['pts_ns']} ns: {e}") from None
                checked += 1
    assert checked >= 40


# ------------------------------------------------------------------------------------------------------------------------------- coverage
@pytest.fixture(scope="module")
def census():
    """Every walk through the oracle alone: what the walks contain."""
    c = {"ops": {}, "frames": 0, "in_transition": 0, "mid_updates": 0, "interrupts": 0, "continues": 0, "tiles_churn": 0, "easings": set(),
         "in_formats": set(), "in_sizes": set(), "out_sizes": set(), "out_formats": set(), "missing_input_frames": 0, "b_came_and_went": {},
         "settled": {}, "last_settled": {}, "lengths": [], "masks": [], "unsettled_claims": []}
    for seed in SW.SEEDS:
        ops = SW.walk(seed)
        oracle = SW.OracleOutputs()
        registered, frames = set(), {}
        b_alive = b_gone_after = False
        c["settled"][seed] = 0
        for k, op in enumerate(ops):
            c["ops"][op["op"]] = c["ops"].get(op["op"], 0) + 1
            if op["op"] == "register_input":
                registered.add(op["input_id"])
            elif op["op"] == "unregister_input":
                registered.discard(op["input_id"])
            elif op["op"] == "frames":
                frames = op["frames"]
            elif op["op"] == "unregister_output":
                oracle.unregister(op["output_id"])
            elif op["op"] == "update":
                oid = op["output_id"]
                c["out_sizes"].add((op["width"], op["height"]))
                c["out_formats"].add(op["format"])
                for comp in SW._layout_components(op["scene"]):
                    if "transition" in comp:
                        c["easings"].add((comp["transition"].get("easing_function") or {}).get("function_name", "linear"))
                st = oracle.state.get(oid)
                running, before = {}, {}
                if st is not None:
                    running = {n.component_id: n for n in _unfinished(st, st.last_ns) if n.component_id is not None}
                    before = {n.component_id: n for n in _nodes(st.root) if n.kind == "tiles" and n.component_id is not None}
                oracle.update(op)                       # (raises scene_json.Unsupported if the walk left what to_oracle reads)
                st = oracle.state[oid]
                if running:
                    c["mid_updates"] += 1
                    interrupted = continued = False
                    for n in _nodes(st.root):
                        old = running.get(n.component_id)
                        if old is None or old.kind != n.kind or n.transition is None:
                            continue
                        if n.transition.offset_progress > 0.0:
                            continued = True            # TransitionState::new: the rest of the running transition (transition.rs:50-67)
                        elif n.end.transition is not None and n.end.transition.should_interrupt and n.transition.duration_ns == n.end.transition.duration_ns:
                            interrupted = True          # a fresh one from the current pts (transition.rs:44-49)
                    c["interrupts"] += interrupted
                    c["continues"] += continued
                for n in _nodes(st.root):
                    old = before.get(n.component_id) if n.kind == "tiles" else None
                    if old is not None:
                        a, b = [x.component_id for x in old.children], [x.component_id for x in n.children]
                        if a != b and any(x is not None for x in a + b):
                            c["tiles_churn"] += 1
            elif op["op"] == "render":
                vis = SW.visible_frames(op, frames, registered)
                for f in vis.values():
                    c["in_formats"].add(f[0])
                    c["in_sizes"].add((f[1], f[2]))
                missing = False
                for oid in sorted(oracle.state):
                    want = oracle.layouts(oid, op["pts_ns"], vis)
                    c["frames"] += 1
                    c["in_transition"] += bool(_unfinished(oracle.state[oid], op["pts_ns"]))
                    c["lengths"].append(len(want))
                    c["masks"].append(max([len(l.masks) for l in want] or [0]))
                    missing |= any(i in registered and i not in vis for i in oracle.inputs[oid])
                    if oid in op["settled"] and not _same_lists(want, oracle.fresh_layouts(oid, op["pts_ns"], vis)):
                        c["unsettled_claims"].append((seed, k, oid))
                assert set(op["settled"]) <= set(oracle.state)
                c["missing_input_frames"] += missing
                c["settled"][seed] += bool(op["settled"])
                c["last_settled"][seed] = sorted(op["settled"]) == sorted(oracle.state)
                if "b" in oracle.state:
                    b_alive = True
                elif b_alive:
                    b_gone_after = True
        c["b_came_and_went"][seed] = b_alive and b_gone_after
    return c


def test_the_walks_cover_what_they_claim(census):
    c = census
    # every layout list fits a default context: non-empty, fewer layouts than max_layouts, no more masks than a layout holds
    assert min(c["lengths"]) >= 1 and max(c["lengths"]) < _max_layouts(), (min(c["lengths"]), max(c["lengths"]))
    assert max(c["masks"]) <= _ffi.MAX_MASKS == orc.MAX_MASKS
    assert set(c["ops"]) == {"register_input", "unregister_input", "update", "unregister_output", "frames", "render"}
    assert min(c["ops"].values()) >= 5, c["ops"]
    assert c["ops"]["render"] >= 12 * 40
    assert c["in_transition"] >= 0.25 * c["frames"], (c["in_transition"], c["frames"])
    assert c["mid_updates"] >= 10 and c["interrupts"] >= 3 and c["continues"] >= 3, (c["mid_updates"], c["interrupts"], c["continues"])
    assert c["tiles_churn"] >= 5
    assert c["easings"] == set(SW.EASINGS)
    assert c["in_formats"] == set(SW.INPUT_FORMATS) and c["in_sizes"] == set(SW.INPUT_SIZES)
    assert c["out_sizes"] == set(SW.OUTPUT_SIZES) and c["out_formats"] == set(SW.OUTPUT_FORMATS)
    assert c["missing_input_frames"] >= 8
    assert all(c["b_came_and_went"].values()), c["b_came_and_went"]


def test_frames_marked_settled_are_settled(census):
    """A new SceneState given only that output's last update returns the identical layout list; every walk has two such frames at least and
    ends on one."""
    assert census["unsettled_claims"] == []
    assert all(n >= 2 for n in census["settled"].values()), census["settled"]
    assert all(census["last_settled"].values()), census["last_settled"]


def test_a_walk_is_a_pure_function_of_its_seed():
    import json
    assert json.dumps(SW.walk(SW.SEEDS[0])) == json.dumps(SW.walk(SW.SEEDS[0])) != json.dumps(SW.walk(SW.SEEDS[1]))
    ops = SW.walk(SW.SEEDS[0])
    pts = [op["pts_ns"] for op in ops if op["op"] == "render"]
    assert all(b > a for a, b in zip(pts, pts[1:])) and pts[0] >= 0


def test_every_walk_rests_and_has_content_only_runs():
    """Runs of three renders with nothing between them (the scene at rest) and runs in which nothing but the frames' content changes."""
    for seed in SW.SEEDS:
        kinds = [op["op"] for op in SW.walk(seed)]
        assert any(kinds[i:i + 3] == ["render"] * 3 for i in range(len(kinds))), seed
        ops = SW.walk(seed)
        content_only = 0
        last = None
        for a, b in zip(ops, ops[1:]):
            if a["op"] == "frames":
                if last is not None and b["op"] == "render" and set(a["frames"]) == set(last) and all(
                        (f is None) == (last[k] is None) and (f is None or f[:3] == last[k][:3]) for k, f in a["frames"].items()) and a["frames"] != last:
                    content_only += 1
                last = a["frames"]
        assert content_only >= 2, seed
