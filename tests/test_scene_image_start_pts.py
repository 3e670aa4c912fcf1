"""start_pts of Image components in the scene engine (smelter-render/src/scene/image_component.rs:91-120; the reference pins it with
gif_progress_between_updates, integration-tests/src/render_tests/image.rs:184) through smr_scene_* — CPU only.

An Image component with an id keeps its start_pts across an update while the previous scene holds an Image of the same id, image_id, width
and height; otherwise, and always without an id, it is the pts of the last render before the update (0 before any render)."""
import pytest

from smelter_amd import _ffi
from smelter_amd.scene import Scene, SceneError

S = 1_000_000_000


def image_nodes(scene):
    return [n.index for n in scene.nodes() if n.kind == _ffi.NODE_IMAGE]


def view(*children):
    return {"type": "view", "children": list(children)}


def render_at(scene, pts_ns):
    """A render of the root layout node: what advances the clock the next update reads (SceneState::register_render_event)."""
    root = scene.nodes()[0]
    scene.node_layouts(0, pts_ns, [(8, 8)] * len(root.children))


@pytest.fixture
def scene():
    s = Scene()
    s.register_image("a", 12, 10)
    s.register_image("b", 12, 10)
    yield s
    s.close()


def start_of(scene, k=0):
    return scene.node_start_pts(image_nodes(scene)[k])


def test_first_update_starts_at_zero(scene):
    scene.update(view({"type": "image", "id": "img", "image_id": "a"}, {"type": "image", "image_id": "b"}), 64, 36)
    assert start_of(scene, 0) == 0 and start_of(scene, 1) == 0


def test_unchanged_component_keeps_its_clock(scene):
    comp = {"type": "image", "id": "img", "image_id": "a", "width": 37, "height": 21}
    scene.update(view(comp), 64, 36)
    render_at(scene, 1 * S)
    scene.update(view(comp), 64, 36)
    assert start_of(scene) == 0
    render_at(scene, 2 * S)
    scene.update(view({"type": "view"}, comp), 64, 36)   # moved within the tree: the id decides, not the place
    assert start_of(scene) == 0


def test_changed_width_restarts(scene):
    scene.update(view({"type": "image", "id": "img", "image_id": "a", "width": 37, "height": 21}), 64, 36)
    render_at(scene, 1 * S)
    scene.update(view({"type": "image", "id": "img", "image_id": "a", "width": 38, "height": 21}), 64, 36)
    assert start_of(scene) == 1 * S
    render_at(scene, 3 * S)
    scene.update(view({"type": "image", "id": "img", "image_id": "a", "width": 38}), 64, 36)   # height given -> not given
    assert start_of(scene) == 3 * S


def test_changed_image_id_restarts(scene):
    scene.update(view({"type": "image", "id": "img", "image_id": "a"}), 64, 36)
    render_at(scene, 1 * S)
    scene.update(view({"type": "image", "id": "img", "image_id": "b"}), 64, 36)
    assert start_of(scene) == 1 * S
    render_at(scene, 2 * S)
    scene.update(view({"type": "image", "id": "img", "image_id": "b"}), 64, 36)
    assert start_of(scene) == 1 * S   # ... and the new clock is then kept


def test_component_without_id_restarts_on_every_update(scene):
    comp = {"type": "image", "image_id": "a"}
    scene.update(view(comp), 64, 36)
    assert start_of(scene) == 0
    render_at(scene, 1 * S)
    scene.update(view(comp), 64, 36)
    assert start_of(scene) == 1 * S
    render_at(scene, 1 * S + 5)
    scene.update(view(comp), 64, 36)
    assert start_of(scene) == 1 * S + 5


def test_kind_change_under_the_same_id_resets(scene):
    scene.update(view({"type": "image", "id": "x", "image_id": "a"}), 64, 36)
    render_at(scene, 1 * S)
    scene.update(view({"type": "view", "id": "x"}), 64, 36)
    render_at(scene, 2 * S)
    scene.update(view({"type": "image", "id": "x", "image_id": "a"}), 64, 36)
    assert start_of(scene) == 2 * S


def test_failed_update_changes_nothing(scene):
    scene.update(view({"type": "image", "id": "img", "image_id": "a"}), 64, 36)
    render_at(scene, 1 * S)
    with pytest.raises(SceneError):
        scene.update(view({"type": "image", "id": "img", "image_id": "missing"}), 64, 36)
    assert start_of(scene) == 0


def test_only_image_nodes_have_one(scene):
    scene.update(view({"type": "image", "id": "img", "image_id": "a"}), 64, 36)
    with pytest.raises(SceneError, match="not an Image node"):
        scene.node_start_pts(0)
    with pytest.raises(SceneError, match="out of range"):
        scene.node_start_pts(9)
