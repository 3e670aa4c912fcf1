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
    _engine_against_oracle(seed, mode, SW.walk(seed), at_least=40)


@pytest.mark.parametrize("mode", ["gpu_optimized", "cpu_optimized"])
@pytest.mark.parametrize("seed", SW.FORMAT_SEEDS)
def test_engine_and_oracle_agree_on_every_frame_of_a_format_walk(seed, mode):
    """Both modes for every seed, whichever of the two the device test of that seed runs (SW.format_mode)."""
    _engine_against_oracle(seed, mode, SW.walk_formats(seed), at_least=30)


def _engine_against_oracle(seed, mode, ops, at_least):
    srgb = mode == "gpu_optimized"
    cmode = _ffi.MODE_GPU_OPTIMIZED if srgb else _ffi.MODE_CPU_OPTIMIZED
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
    assert checked >= at_least


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


# ------------------------------------------------------------------------------------------- the first two walks stay what they were
WALK_SHA256 = {
    11: "4ae8c8528a6d5293a4e8fb1e85a039e25d7934ba731310c9490a21fdf41877d3", 12: "a299c25702a1e33123a17c02e564146c7a142bf114b4efa17af70b95cc894ab3",
    13: "4bf41264edc0d219c8e080c06e4c21afa309b4ceb11cf8aca25a88c71438dca5", 14: "12caaa024bb6e161507aded8827200b8170495d8d58b11760aecd074529ecb28",
    15: "0c9802fb08ef1d86f44646b0b2beebcb11f890736931738a09c6ab0e4fc4a9e9", 16: "c65f725b316b460209b9478209e9caef729eead01de9fac29550bcec9271c81b",
    17: "9552430e96a09f05bc2424e28d0d4bccc938656d03ecc01040376608618cd824", 18: "27eacfb8edc7e0584c759cf1911c4ce421d97df2db9873976a70e3cadb6b7fb8",
    19: "f1e3cbe6ad3dbb1459b8ea9ec78e0f292457b8d3af3ca7b8adaf1fbf32e6a250", 20: "ab62e58353825f37ba764955c7022f7c8862503603f4e6264ced2880807ebbed",
    21: "a9cd2b8173f4a56c27d735ee8db939a7563be314ec0bdee9aa5e2e172c6e48e0", 22: "144aea13c5952b89cf70f71599e972f6459b51434d26e10cb3e104bf723f4030"}
NODE_WALK_SHA256 = {
    101: "025f4bedee60802d4e6bec99fd206d703dcab1cd7f8643eaa11a95d2588127f9", 102: "f5a79dd7148e1f05a732497d7feee0e6f8ae7ff8e0eb64438341e4d9862d585b",
    103: "c87b6da74d7472bffc97bb422b524a13d7fd099a716f5591689b97c74231aa7b", 104: "78b4b77dcd5f3d3aa09920e424d143f1247da061e72d5ba7326b49bdea813362"}


def test_the_first_two_walks_are_the_op_lists_they_were_before_the_format_walk():
    """sha256 of json.dumps(walk(seed)), recorded at the commit before tests/scene_walk.py gained walk_formats."""
    import hashlib
    import json
    sha = lambda ops: hashlib.sha256(json.dumps(ops).encode()).hexdigest()  # noqa: E731
    assert sorted(WALK_SHA256) == SW.SEEDS and sorted(NODE_WALK_SHA256) == SW.NODE_SEEDS
    assert {s: sha(SW.walk(s)) for s in SW.SEEDS} == WALK_SHA256
    assert {s: sha(SW.walk_nodes(s)) for s in SW.NODE_SEEDS} == NODE_WALK_SHA256


# --------------------------------------------------------------------------------------------------------- what the format walk contains
def _boxes_intersect(a, b):
    return a.left < b.left + b.width and b.left < a.left + a.width and a.top < b.top + b.height and b.top < a.top + a.height


def _is_alpha(spec):
    return SW.split_format(spec[0])[0] in SW.ALPHA_FORMATS


def _changes(p, q):
    """What an input id's frame spec p -> q (two consecutive renders, shown in both) is, of the changes of state (a) - (e)."""
    (pb, pm), (qb, qm) = SW.split_format(p[0]), SW.split_format(q[0])
    same_size = p[1:3] == q[1:3]
    ycc, eight = SW.YCBCR_FORMATS, SW.RGB12_FORMATS + SW.OTHER_8BIT_FORMATS
    out = []
    if same_size and pb in ycc and _is_alpha(q) and not SW.alpha_everywhere_255(q):
        out.append("a_to_alpha")
    if same_size and qb in ycc and _is_alpha(p) and not SW.alpha_everywhere_255(p):
        out.append("a_back")
    if same_size and {pb, qb} <= set(eight) and (pb in SW.RGB12_FORMATS) != (qb in SW.RGB12_FORMATS):
        out.append("b")
    if same_size and ((pb in eight and qb in SW.HI_FORMATS) or (pb in SW.HI_FORMATS and qb in eight)):
        out.append("c")
    if same_size and pb == qb and pm != qm:
        out.append("d_same_content" if p[3] == q[3] else "d_new_content")
    if p[0] == q[0] and not same_size:
        out.append("e")
        if tuple(q[1:3]) in SW.ODD_SIZES:
            out.append("e_odd")
    return out


@pytest.fixture(scope="module")
def format_census():
    """Every format walk through the oracle alone.  An input counts as SHOWN at a render when it has a texture then (SW.visible_frames) and a
    live output's scene names it."""
    c = {"formats": set(), "matrices": {}, "sizes": set(), "changes": {}, "pair_frames": 0, "family_frames": 0, "overlap_frames": 0, "tagged_sets": set(),
         "tag_set_changes": 0, "settled": {}, "last_settled": {}, "unsettled_claims": [], "lengths": [], "masks": [], "not_block420": {}, "renders": {},
         "wrapped": 0, "wrapped_seeds": set(), "b_came_and_went": {}}
    for seed in SW.FORMAT_SEEDS:
        ops = SW.walk_formats(seed)
        oracle = SW.OracleOutputs()
        registered, frames, prev, prev_tagged = set(), {}, {}, None
        b_alive = b_gone_after = False
        c["settled"][seed] = c["renders"][seed] = 0
        c["not_block420"][seed] = False
        for k, op in enumerate(ops):
            if op["op"] == "register_input":
                registered.add(op["input_id"])
            elif op["op"] == "unregister_input":
                registered.discard(op["input_id"])
            elif op["op"] == "frames":
                frames = op["frames"]
            elif op["op"] == "unregister_output":
                oracle.unregister(op["output_id"])
            elif op["op"] == "update":
                oracle.update(op)
            elif op["op"] == "render":
                c["renders"][seed] += 1
                vis = SW.visible_frames(op, frames, registered)
                shown = {i: vis[i] for oid in oracle.state for i in oracle.inputs[oid] if i in vis}
                overlap = False
                for oid in sorted(oracle.state):
                    want = oracle.layouts(oid, op["pts_ns"], vis)
                    c["lengths"].append(len(want))
                    c["masks"].append(max([len(l.masks) for l in want] or [0]))
                    if oid in op["settled"] and not _same_lists(want, oracle.fresh_layouts(oid, op["pts_ns"], vis)):
                        c["unsettled_claims"].append((seed, k, oid))
                    textures = [(j, l, oracle.inputs[oid][l.source_index]) for j, l in enumerate(want) if l.type == 0 and l.source_index < len(oracle.inputs[oid])]
                    textures = [(j, l, i) for j, l, i in textures if i in vis]
                    for j, l, i in textures:
                        if _is_alpha(vis[i]) and not SW.alpha_everywhere_255(vis[i]) and any(_boxes_intersect(l, m) for jj, m, _ in textures if jj < j):
                            overlap = True
                c["overlap_frames"] += overlap
                assert set(op["settled"]) <= set(oracle.state)
                c["settled"][seed] += bool(op["settled"])
                c["last_settled"][seed] = sorted(op["settled"]) == sorted(oracle.state)
                split = {i: SW.split_format(f[0]) for i, f in shown.items()}
                for i, f in shown.items():
                    base, matrix = split[i]
                    c["formats"].add(base)
                    c["sizes"].add((f[1], f[2]))
                    c["wrapped"] += f[3] % 6 == 0
                    if f[3] % 6 == 0:
                        c["wrapped_seeds"].add(seed)
                    if base in SW.YCBCR_FORMATS:
                        c["matrices"].setdefault(matrix, set()).add(base)
                    c["not_block420"][seed] |= base not in SW.RGB12_FORMATS
                    if i in prev and prev[i] != f:
                        for what in _changes(prev[i], f):
                            c["changes"][what] = c["changes"].get(what, 0) + 1
                ids = sorted(shown)
                c["pair_frames"] += any(split[i][0] == split[j][0] and split[i][1] != split[j][1] and split[i][0] in SW.YCBCR_FORMATS for i in ids for j in ids if i < j)
                c["family_frames"] += len({SW.CONVERTER_FAMILIES[b] for b, _ in split.values() if b in SW.CONVERTER_FAMILIES}) >= 3
                tagged = frozenset(i for i in ids if split[i][1] is not None)
                c["tagged_sets"].add(tagged)
                c["tag_set_changes"] += prev_tagged is not None and tagged != prev_tagged
                prev, prev_tagged = shown, tagged
                if "b" in oracle.state:
                    b_alive = True
                elif b_alive:
                    b_gone_after = True
        c["b_came_and_went"][seed] = b_alive and b_gone_after
    return c


def test_the_format_walks_cover_what_they_claim(format_census):
    c = format_census
    print({k: v for k, v in c.items() if k not in ("lengths", "masks")})
    assert min(c["lengths"]) >= 1 and max(c["lengths"]) < _max_layouts(), (min(c["lengths"]), max(c["lengths"]))
    assert max(c["masks"]) <= _ffi.MAX_MASKS == orc.MAX_MASKS
    assert 6 <= len(SW.FORMAT_SEEDS) <= 8 and not set(SW.FORMAT_SEEDS) & set(SW.SEEDS + SW.NODE_SEEDS)
    assert {SW.format_mode(s) for s in SW.FORMAT_SEEDS} == {"gpu_optimized", "cpu_optimized"}
    # every base format, in the order of smr_frame_format
    from smelter_amd import hip
    assert [getattr(hip, "FRAME_" + n) for n in ("PLANAR_YUV420", "PLANAR_YUV422", "PLANAR_YUV444", "PLANAR_YUVJ420", "UYVY422", "YUYV422", "NV12", "BGRA", "ARGB", "RGBA",
                                                 "P010", "PLANAR_YUV420P10", "PLANAR_YUV422P10", "P210", "V210")] == list(range(len(SW.BASE_FORMATS)))
    assert c["formats"] == set(SW.BASE_FORMATS) and len(SW.BASE_FORMATS) == 15
    # every matrix on an 8-bit 4:2:0, a packed and a 10-bit format
    assert set(c["matrices"]) == set(SW.MATRICES)
    for m, seen in c["matrices"].items():
        assert seen & set(SW.RGB12_FORMATS) and seen & set(SW.PACKED_8BIT_FORMATS) and seen & set(SW.HI_FORMATS), (m, seen)
    assert c["sizes"] >= set(SW.ODD_SIZES), set(SW.ODD_SIZES) - c["sizes"]
    assert max(max(s) for s in c["sizes"]) <= 160 and all(w <= 160 and h <= 90 or (w, h) == (36, 64) for w, h in c["sizes"])
    ch = c["changes"]
    assert ch.get("a_to_alpha", 0) >= 2 and ch.get("a_back", 0) >= 2, ch
    assert ch.get("b", 0) >= 2 and ch.get("c", 0) >= 2 and ch.get("e", 0) >= 2 and ch.get("e_odd", 0) >= 1, ch
    assert ch.get("d_same_content", 0) >= 1 and ch.get("d_new_content", 0) >= 1 and ch.get("d_same_content", 0) + ch.get("d_new_content", 0) >= 2, ch
    assert c["pair_frames"] >= 3 and c["family_frames"] >= 3, (c["pair_frames"], c["family_frames"])
    assert len(c["tagged_sets"]) >= 4 and c["tag_set_changes"] >= 12, (c["tagged_sets"], c["tag_set_changes"])
    assert c["overlap_frames"] >= 5, c["overlap_frames"]
    # frame specs the device test keeps in caller memory (content_seed % 6 == 0): in every seed
    assert c["wrapped"] >= 6 and c["wrapped_seeds"] == set(SW.FORMAT_SEEDS), (c["wrapped"], c["wrapped_seeds"])
    assert all(c["not_block420"].values()), c["not_block420"]   # every seed shows a frame the 4:2:0 block converter does not take
    assert all(c["b_came_and_went"].values()), c["b_came_and_went"]
    assert all(n >= 30 for n in c["renders"].values()), c["renders"]


def test_format_walk_frames_marked_settled_are_settled(format_census):
    assert format_census["unsettled_claims"] == []
    assert all(n >= 2 for n in format_census["settled"].values()), format_census["settled"]
    assert all(format_census["last_settled"].values()), format_census["last_settled"]


def test_a_format_walk_is_a_pure_function_of_its_seed():
    import json
    a, b = SW.FORMAT_SEEDS[:2]
    assert json.dumps(SW.walk_formats(a)) == json.dumps(SW.walk_formats(a)) != json.dumps(SW.walk_formats(b))
    pts = [op["pts_ns"] for op in SW.walk_formats(a) if op["op"] == "render"]
    assert all(y > x for x, y in zip(pts, pts[1:])) and pts[0] >= 0


def test_format_walk_frames_are_what_the_walk_says_they_are():
    """frame_planes on every format at an even and a ragged size: valid frames of the library's plane shapes; premultiplied BGRA / ARGB with runs of 0 and
    255; 10-bit codes that use their low two bits; junk in the bits the formats ignore; a tag changes no plane; the first walks' planes unchanged."""
    import hashlib
    import numpy as np
    from tests import hi422_model
    for base in SW.BASE_FORMATS:
        for (w, h) in [(64, 36), (131, 75) if SW.format_accepts(base, 131, 75) else (50, 22)]:
            p = SW.frame_planes([base, w, h, 1234567])
            q = SW.frame_planes([SW.join_format(base, "bt2020") if base in SW.YCBCR_FORMATS else base, w, h, 1234567])
            assert all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(p, q))
            if base in ("bgra", "argb"):
                a = p[0][..., 3 if base == "bgra" else 0].astype(int)
                colour = p[0][..., :3] if base == "bgra" else p[0][..., 1:]
                assert (colour.astype(int) <= a[..., None]).all() and a.min() == 0 and a.max() == 255 and 0 < a[(a > 0) & (a < 255)].size
                rows = ["".join("0" if v == 0 else "F" if v == 255 else "." for v in row) for row in a]
                assert any("0" * 8 in row for row in rows) and any("F" * 8 in row for row in rows)
                assert (SW.frame_planes([base, w, h, 1234568])[0][..., 3 if base == "bgra" else 0] == 255).all()   # (one in four: 1234568 % 4 == 0)
            if base in ("p010", "p210"):
                assert all(x.dtype == np.uint16 and (x & 63).any() and ((x >> 6) & 3).any() for x in p)
            if base in ("yuv420p10", "yuv422p10"):
                assert all(x.dtype == np.uint16 and (x >> 10).any() and (x & 3).any() for x in p)
            if base == "v210":
                assert p[0].dtype == np.uint32 and p[0].shape == (h, 4 * hi422_model.groups(w)) and (p[0] >> 30).any()
                y, cb, cr = hi422_model.v210_unpack(p[0], w)
                assert (y & 3).any() and (cb & 3).any() and (cr & 3).any()
                if w % 6:   # components beyond the width in the last group hold junk too
                    assert not np.array_equal(hi422_model.v210_pack(y, cb, cr), p[0] & 0x3FFFFFFF)
    # (recorded before frame_planes learned the other formats)
    old = SW.frame_planes(["nv12", 64, 36, 99])
    assert hashlib.sha256(b"".join(x.tobytes() for x in old)).hexdigest() == "4012e4b78af92981277176dd7b184f2cedb63e8833acbe8550bd3b164825bb7f"
