"""The host side of the library (scene engine, text pipeline, renderer: smelter_amd/csrc/host) under AddressSanitizer + UBSan.

tests/san/host_fuzz.cpp is compiled by g++ together with the host sources (no HIP involved: they are plain C++17) and drives the scene
engine and the text pipeline through the C ABI with the reference's own scenes, mutated scenes and corrupted fonts.
tests/san/renderer_fuzz.cpp does the same to the renderer (registry, update_scene, render-graph walk, lanes, text nodes), linked against
tests/san/null_device.cpp — a stand-in for the GPU half of the ABI that checks and reads every argument, counts the surfaces it hands
out and fails allocations on request.  A rejected input is an answer; a memory error, undefined behaviour, a leaked device surface or a
hang fails the test.  (What they found when they were written: an empty-contour glyph whose extents stayed at infinity, pen positions
of absurd font sizes cast to int, a cmap-12 group count above 2^31 that sent the binary search round in circles, an output frame
leaked when the second of a lane's two frames could not be allocated, float -> integer casts of hostile node sizes.)"""
import json
import os
import shutil
import subprocess

import pytest

from tests import san_build

HERE = os.path.dirname(os.path.abspath(__file__))
FONT_DIRS = ["/usr/share/fonts/truetype/dejavu", os.path.join(HERE, "golden", "fonts")]


@pytest.fixture(scope="module")
def harness():
    return {"host_fuzz": san_build.build("host_fuzz", ("host_fuzz.cpp",)),
            "renderer_fuzz": san_build.build("renderer_fuzz", ("renderer_fuzz.cpp", "null_device.cpp", "renderer.cpp"))}


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """One file per scene: the reference's API vectors (smelter-api/tests/scene_deserialization.rs, accepted and rejected ones alike) and
    every update of its render tests (tests/golden/*.json, extracted by the scripts beside them); the fonts this machine has."""
    out = tmp_path_factory.mktemp("host_fuzz_corpus")
    n = 0
    with open(os.path.join(HERE, "golden", "scene_api_vectors.json")) as f:
        for v in json.load(f)["vectors"]:
            (out / f"api_{n:04d}.json").write_text(json.dumps(v["scene"]))
            n += 1
    with open(os.path.join(HERE, "golden", "render_test_scenes.json")) as f:
        for t in json.load(f)["tests"]:
            for step in t["steps"]:
                if "update" in step:
                    (out / f"render_{n:04d}.json").write_text(json.dumps(step["update"]))
                    n += 1
    fonts = 0
    for d in FONT_DIRS:
        if os.path.isdir(d):
            for name in sorted(os.listdir(d)):
                if name.endswith(".ttf") and fonts < 6:
                    shutil.copy(os.path.join(d, name), out / f"{fonts}_{name}")
                    fonts += 1
    return str(out), n, fonts


def _run(exe, corpus_dir, iterations, seed, timeout):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, corpus_dir, str(iterations), str(seed)], capture_output=True, text=True, timeout=timeout, env=env)
    assert r.returncode == 0, f"seed {seed}: rc {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-6000:]}"
    assert "runtime error" not in r.stderr, r.stderr[-6000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_scene_engine_and_text_pipeline_survive_hostile_input(harness, corpus, seed):
    corpus_dir, n_scenes, n_fonts = corpus
    got = _run(harness["host_fuzz"], corpus_dir, 4000, seed, timeout=600)
    assert got["corpus_scenes"] == n_scenes
    # every scene of the corpus runs twice (alone; as an update of a scene that lives on): what the reference accepts must be accepted
    assert got["corpus_ok"] >= n_scenes, got
    assert got["scenes_ok"] > got["corpus_ok"] + 500 and got["scenes_rejected"] > 500, got   # mutations reach both sides of the validator
    assert got["layouts"] > 10000, got
    if n_fonts:
        assert got["runs"] > 500 and got["glyphs"] > 5000, got
        assert got["fonts_ok"] > n_fonts and got["fonts_rejected"] > 50, got                  # corrupted fonts: some load, some are refused


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_renderer_survives_hostile_hosts_and_a_failing_device(harness, corpus, seed):
    """smr_renderer_* on the null device: scenes (also mutated) on three outputs, frames of every format — fresh, stale, missing, for
    unknown inputs — on one to three lanes, registrations coming and going, glyph runs, a font book, device allocations that fail.  The
    null device refuses what the library would refuse and aborts on what would corrupt memory; every surface it handed out must be back
    when a renderer is destroyed."""
    corpus_dir, n_scenes, n_fonts = corpus
    got = _run(harness["renderer_fuzz"], corpus_dir, 12000, seed, timeout=600)
    assert got["updates_ok"] > 1000 and got["updates_refused"] > 500, got
    assert got["renders_ok"] > 4000 and got["frames_out"] > got["renders_ok"], got     # several outputs per render
    assert got["renders_refused"] > 50 and got["injected_failures"] > 100, got          # the error paths ran
    assert got["text_runs"] > 10, got


def test_replay_modes(harness, corpus, tmp_path):
    """--scene / --font replay one input (what HOST_FUZZ_TRACE leaves behind after an abort)."""
    harness = harness["host_fuzz"]
    corpus_dir = corpus[0]
    scene = sorted(f for f in os.listdir(corpus_dir) if f.endswith(".json"))[0]
    r = subprocess.run([harness, "--scene", os.path.join(corpus_dir, scene)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    fonts = sorted(f for f in os.listdir(corpus_dir) if f.endswith(".ttf"))
    if fonts:
        r = subprocess.run([harness, "--font", os.path.join(corpus_dir, fonts[0])], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]


def test_edges_that_end_on_the_bitmap_border_stay_inside_the_accumulator(harness):
    """x advanced row by row could arrive at -1e-17 for an edge that ends exactly on column 0 (floor -> column -1, eight bytes in
    front of the accumulator).  A million random edges ending on the first / last column, the advisor's own case first, into accumulators of
    exactly w * h + 1 doubles under AddressSanitizer."""
    r = subprocess.run([harness["host_fuzz"], "--edges", "1000000"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "runtime error" not in r.stderr, r.stderr[-4000:]
    assert json.loads(r.stdout.strip().splitlines()[-1])["edges"] == 1000000
