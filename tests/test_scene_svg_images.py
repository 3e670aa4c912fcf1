"""An SVG asset in the scene engine is its resolution and nothing else (include/smr.h, "SVG image assets": what
smr_renderer_register_svg_image hands to smr_scene_register_image is SvgAsset::resolution(), svg_image.rs:89-94).  Through smr_scene_* alone:
an id registered with an SVG tree's truncated size gives the node sizes of scene/image_component.rs:67-89 for (w, h), (w, -), (-, h) and
(-, -) — the integer aspect ratio included.  A pin: it passes without the SVG feature, and says that the scene engine needed no change to
size the nodes the rasteriser is then asked for."""
import pytest

from smelter_amd import _ffi
from smelter_amd.scene import Scene

# (tree size truncated, component width, component height) -> node size.  aspect = usize width / usize height (integer division),
# (w, -) -> (w, round(w / aspect)), (-, h) -> (round(h * aspect), h).
CASES = [
    ((512, 512), 1600, 900, (1600, 900)),
    ((512, 512), 1600, None, (1600, 1600)),
    ((512, 512), None, 300, (300, 300)),
    ((512, 512), None, None, (512, 512)),
    ((640, 320), 100, None, (100, 50)),        # aspect 2
    ((640, 320), None, 100, (200, 100)),
    ((700, 320), 100, None, (100, 50)),        # 700 / 320 = 2 as integers, not 2.1875
    ((700, 320), None, 33, (66, 33)),
    ((700, 320), 101, None, (101, 51)),        # round(50.5): half away from zero
    ((64, 64), 160, 100, (160, 100)),
    ((64, 64), 0, 5, (0, 5)),                  # a node without texels: no raster, transparent
    ((300, 512), None, 100, (0, 100)),         # aspect 0: (-, h) collapses to zero width
    ((512, 512), 20.4, 10.5, (20, 11)),        # f32::round on both
]


@pytest.mark.parametrize("tree,w,h,want", CASES)
def test_svg_node_sizes_follow_the_image_component(tree, w, h, want):
    s = Scene()
    try:
        s.register_image("logo", *tree)
        comp = {"type": "image", "image_id": "logo"}
        if w is not None:
            comp["width"] = w
        if h is not None:
            comp["height"] = h
        nodes = s.update({"type": "view", "children": [comp]}, 1920, 1080)
        img = [n for n in nodes if n.kind == _ffi.NODE_IMAGE]
        assert len(img) == 1 and img[0].ref_id == "logo"
        assert (img[0].width, img[0].height) == want
    finally:
        s.close()


def test_one_asset_at_two_sizes_is_two_node_sizes():
    s = Scene()
    try:
        s.register_image("logo", 64, 64)
        nodes = s.update({"type": "view", "children": [{"type": "image", "image_id": "logo"},
                                                       {"type": "image", "image_id": "logo", "width": 160, "height": 100}]}, 640, 360)
        assert [(n.width, n.height) for n in nodes if n.kind == _ffi.NODE_IMAGE] == [(64, 64), (160, 100)]
    finally:
        s.close()
