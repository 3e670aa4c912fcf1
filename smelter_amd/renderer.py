"""`Renderer` of the reference (smelter-render/src/state.rs:96-252) on the HIP library: register inputs / images / shaders,
update_scene(output, resolution, format, scene JSON), render(frame set) -> output frames in HBM.

The implementation is C++ (smelter_amd/csrc/host/renderer.cpp behind `smr_renderer_*`, include/smr.h); this is the ctypes
binding used by bench.py, smoke() and the tests.
"""
from __future__ import annotations

import ctypes as C
import json
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np

from . import _ffi
from .hip import Context, DeviceFrame, FRAME_PLANAR_YUV420
from .scene import Node, SceneError


class BorrowedFrame(DeviceFrame):
    """An output frame owned by the renderer (valid until the render after the next)."""

    def __init__(self, ctx: Context, c_frame: _ffi.Frame):  # noqa: super().__init__ would allocate
        self.ctx, self.fmt, self.w, self.h = ctx, c_frame.format, c_frame.width, c_frame.height
        self.c = c_frame

    def destroy(self):
        pass


class Renderer:
    def __init__(self, ctx: Context, stream_fallback_timeout_s: float = 0.5, lanes: Sequence[Context] = (), max_outputs: int = 16,
                 shards: Sequence[Context] = ()):
        """`shards`: further contexts — usually one per device — that take a share of the inputs (smr_renderer_add_shard): the k-th registered
        input lives on context k mod (1 + len(shards)) of [ctx] + shards, `input_context(id)` says which; its frames are created / uploaded
        there.  Outputs are composed on `ctx`.  Does not combine with `lanes`.
        `lanes`: extra contexts on the same device — consecutive frames rotate through `ctx` and these, so up to
        1 + len(lanes) frames are in flight on the GPU while the scene stays one state (smr_renderer_add_lane).
        `max_outputs`: how many output frames one render call can hand back (the `cap` of smr_renderer_render)."""
        self.ctx, self.lib = ctx, ctx.lib
        h = C.c_void_p()
        if self.lib.smr_renderer_create(ctx.handle, int(stream_fallback_timeout_s * 1e9), C.byref(h)) != 0:
            raise RuntimeError("smr_renderer_create failed")
        self._h = h
        self._max_outputs = max(int(max_outputs), 1)
        self._outs = (_ffi.OutputFrame * self._max_outputs)()
        self._ctx_of = {ctx.handle.value: ctx}
        for c in lanes:
            self._check(self.lib.smr_renderer_add_lane(self._h, c.handle))
            self._ctx_of[c.handle.value] = c
        for c in shards:
            self._check(self.lib.smr_renderer_add_shard(self._h, c.handle))
            self._ctx_of[c.handle.value] = c

    def add_shard(self, ctx: Context):
        self._check(self.lib.smr_renderer_add_shard(self._h, ctx.handle))
        self._ctx_of[ctx.handle.value] = ctx

    def add_lane(self, ctx: Context):
        self._check(self.lib.smr_renderer_add_lane(self._h, ctx.handle))
        self._ctx_of[ctx.handle.value] = ctx

    def input_context(self, input_id: str) -> Context:
        """The context the frames of `input_id` must be resident on (smr_renderer_input_ctx)."""
        h = C.c_void_p()
        self._check(self.lib.smr_renderer_input_ctx(self._h, input_id.encode(), C.byref(h)))
        return self._ctx_of[h.value]

    def sync(self):
        """Waits for the frames in flight on every lane and shard."""
        self._check(self.lib.smr_renderer_sync(self._h))

    def output(self, i: int = 0) -> "BorrowedFrame":
        """Output `i` of the last render call, bound to the context (lane) that produced it."""
        return BorrowedFrame(self._ctx_of[self._outs[i].ctx], self._outs[i].frame.contents)

    def close(self):
        if self._h:
            self.lib.smr_renderer_destroy(self._h)
            self._h = None

    def _check(self, rc: int) -> int:
        if rc < 0:
            raise SceneError(self.lib.smr_renderer_last_error(self._h).decode())
        return rc

    # -- registry (state.rs:102-171)
    def register_input(self, input_id: str):
        self._check(self.lib.smr_renderer_register_input(self._h, input_id.encode()))

    def unregister_input(self, input_id: str):
        self._check(self.lib.smr_renderer_unregister_input(self._h, input_id.encode()))

    def register_image(self, image_id: str, rgba_straight: np.ndarray):
        px = np.ascontiguousarray(rgba_straight, dtype=np.uint8)
        h, w = px.shape[:2]
        self._check(self.lib.smr_renderer_register_image(self._h, image_id.encode(), px.ctypes.data, w, h))

    def register_animated_image(self, image_id: str, frames: np.ndarray, delays_ns: Sequence[int]):
        """The decoded frames of an animated image, `frames[n, h, w, 4]` straight-alpha RGBA8, and their delays in ns
        (smr_renderer_register_animated_image): an Image node of it shows the frame of the render's pts on the node's own clock."""
        px = np.ascontiguousarray(frames, dtype=np.uint8)
        if px.ndim != 4 or px.shape[3] != 4:
            raise ValueError("frames must be [n, h, w, 4]")
        n, h, w = px.shape[:3]
        if len(delays_ns) != n:
            raise ValueError("one delay per frame")
        delays = (C.c_uint64 * max(n, 1))(*[int(d) for d in delays_ns])
        self._check(self.lib.smr_renderer_register_animated_image(self._h, image_id.encode(), px.ctypes.data, w, h, n, delays))

    def image_launches(self) -> int:
        """Launches of the image pass so far, all lanes (smr_renderer_image_launches)."""
        n = C.c_uint64()
        self._check(self.lib.smr_renderer_image_launches(self._h, C.byref(n)))
        return n.value

    # -- SVG image assets: the vector library is the caller's, everything after the pixmap the library's (include/smr.h, "SVG image assets")
    def register_svg_image(self, image_id: str, width: int, height: int, rasterise):
        """An SVG asset of intrinsic width x height (smr_renderer_register_svg_image).  `rasterise(w, h)` returns the asset drawn at w x h as
        an (h, w, 4) uint8 array, premultiplied and gamma-encoded; it runs inside update_scene, once per node size no resident raster covers.
        An exception refuses that update, with its text appended to the error.  It must not call into this renderer."""
        errors = self._svg_errors = getattr(self, "_svg_errors", {})

        def call(_user, _id, w, h, rgba, pitch):
            try:
                px = np.asarray(rasterise(int(w), int(h)))
                if px.dtype != np.uint8 or px.shape != (h, w, 4):
                    raise ValueError(f"rasterise({w}, {h}) returned {px.dtype} {px.shape}, not uint8 ({h}, {w}, 4)")
                dst = np.ctypeslib.as_array(rgba, shape=(h, pitch))
                dst[:, :w * 4] = px.reshape(h, w * 4)
                return 0
            except BaseException as e:  # (nothing may unwind through the C frames above)
                errors[image_id] = f"{type(e).__name__}: {e}"
                return 1
        cb = _ffi.SVG_RASTERISE_FN(call)
        self._check(self.lib.smr_renderer_register_svg_image(self._h, image_id.encode(), int(width), int(height), cb, None))
        self._svg_callbacks = getattr(self, "_svg_callbacks", {})
        self._svg_callbacks[image_id] = cb  # kept alive for the registration's life

    def unregister_image(self, image_id: str):
        """A static, animated or SVG image (smr_renderer_unregister_image); refused while an active scene uses it."""
        self._check(self.lib.smr_renderer_unregister_image(self._h, image_id.encode()))
        getattr(self, "_svg_callbacks", {}).pop(image_id, None)

    def svg_stats(self) -> Tuple[int, int, int]:
        """(calls of the rasterisers so far, k_svg_nodes launches so far, rasters resident now) (smr_renderer_svg_stats)."""
        calls, launches, resident = C.c_uint64(), C.c_uint64(), C.c_uint32()
        self._check(self.lib.smr_renderer_svg_stats(self._h, C.byref(calls), C.byref(launches), C.byref(resident)))
        return calls.value, launches.value, resident.value

    def text_stats(self) -> Tuple[int, int, int]:
        """(smr_fontbook_rasterise calls so far, k_text_nodes launches so far, Text rasters resident now) (smr_renderer_text_stats)."""
        calls, launches, resident = C.c_uint64(), C.c_uint64(), C.c_uint32()
        self._check(self.lib.smr_renderer_text_stats(self._h, C.byref(calls), C.byref(launches), C.byref(resident)))
        return calls.value, launches.value, resident.value

    # -- WebView nodes: the browser is the caller's, the node's compositing is the library's (include/smr.h, "WebView nodes")
    def register_web_renderer(self, instance_id: str, width: int, height: int, embedding: int = _ffi.WEB_NATIVE_OVER_CONTENT):
        """A web renderer instance of width x height; `embedding`: _ffi.WEB_CHROMIUM_EMBEDDING / WEB_NATIVE_OVER_CONTENT /
        WEB_NATIVE_UNDER_CONTENT (smr_renderer_register_web_renderer)."""
        self._check(self.lib.smr_renderer_register_web_renderer(self._h, instance_id.encode(), int(width), int(height), int(embedding)))

    def unregister_web_renderer(self, instance_id: str):
        self._check(self.lib.smr_renderer_unregister_web_renderer(self._h, instance_id.encode()))

    def web_paint(self, instance_id: str, bgra: np.ndarray):
        """The browser's latest paint, `bgra[h, w, 4]` premultiplied BGRA8 at the instance's resolution (smr_renderer_web_paint); a view with
        padded rows is handed over with its pitch.  Copied before the call returns."""
        px = np.asarray(bgra)
        if px.dtype != np.uint8 or px.ndim != 3 or px.shape[2] != 4:
            raise ValueError("bgra must be a uint8 [h, w, 4] array")
        if px.strides[2] != 1 or px.strides[1] != 4 or px.strides[0] < px.shape[1] * 4:
            px = np.ascontiguousarray(px)
        self._check(self.lib.smr_renderer_web_paint(self._h, instance_id.encode(), px.ctypes.data, px.strides[0]))

    def web_positions(self, instance_id: str, rects: Sequence[Tuple[float, float, float, float]]):
        """One (x, y, width, height) per child, in child order, in page pixels (smr_renderer_web_positions)."""
        arr = (_ffi.WebRect * max(len(rects), 1))(*[_ffi.WebRect(*[float(v) for v in q]) for q in rects])
        self._check(self.lib.smr_renderer_web_positions(self._h, instance_id.encode(), arr, len(rects)))

    def web_launches(self) -> int:
        """k_web_view launches so far, all lanes (smr_renderer_web_launches)."""
        n = C.c_uint64()
        self._check(self.lib.smr_renderer_web_launches(self._h, C.byref(n)))
        return n.value

    def set_text_measurer(self, measurer):
        """The caller's text shaper for Text nodes without explicit width / height (tests.text_twin.Shaper(...).measurer)."""
        self._measurer = measurer  # keep the callback alive
        self._check(self.lib.smr_renderer_set_text_measurer(self._h, measurer if measurer is not None else _ffi.TEXT_MEASURE_FN(0), None))

    def set_fontbook(self, book):
        """A smelter_amd.fontbook.NativeFontBook (smr_fontbook): the renderer measures and draws every Text node itself at update_scene."""
        self._fontbook = book  # keep it alive: the renderer does not own it
        self._check(self.lib.smr_renderer_set_fontbook(self._h, book.handle if book is not None else None))

    def register_shader(self, shader_id: str, builtin_id: int = _ffi.SHADER_GAUSSIAN_BLUR):
        self._check(self.lib.smr_renderer_register_shader(self._h, shader_id.encode(), builtin_id))

    def register_shader_source(self, shader_id: str, source: str):
        """A user shader written in HIP C++ (include/smr.h "user shaders"), compiled here; a compile error raises SceneError with the log."""
        self._check(self.lib.smr_renderer_register_shader_source(self._h, shader_id.encode(), source.encode()))

    def register_shader_program(self, shader_id: str, program):
        """A compiled smelter_amd.hip.ShaderProgram the caller keeps: it must outlive the registration."""
        self._programs = getattr(self, "_programs", {})
        self._programs[shader_id] = program  # keep it alive: the renderer does not own it
        self._check(self.lib.smr_renderer_register_shader_program(self._h, shader_id.encode(), program.handle))

    # -- scenes (state.rs:177-189)
    def update_scene(self, output_id: str, width: int, height: int, scene: Union[str, dict], output_format: int = FRAME_PLANAR_YUV420) -> List[Node]:
        """`output_format`: FRAME_PLANAR_YUV420 / _YUV422 / _YUV444, FRAME_NV12, FRAME_RGBA, or packed 4:2:2 — FRAME_UYVY422 / FRAME_YUYV422, one
        plane of (width / 2) x height texels, an even `width` only.  Outputs are 8-bit, BT.709, limited range; a refused update leaves the
        output's previous scene active."""
        text = scene if isinstance(scene, str) else json.dumps(scene)
        svg_errors = getattr(self, "_svg_errors", {})
        svg_errors.clear()
        rc = self.lib.smr_renderer_update_scene(self._h, output_id.encode(), width, height, output_format, text.encode())
        if rc < 0 and svg_errors:  # an SVG rasteriser raised: its text goes with the library's
            raise SceneError(self.lib.smr_renderer_last_error(self._h).decode() + ": " + "; ".join(svg_errors.values()))
        self._check(rc)
        return self.nodes(output_id)

    def unregister_output(self, output_id: str):
        self._check(self.lib.smr_renderer_unregister_output(self._h, output_id.encode()))

    def nodes(self, output_id: str) -> List[Node]:
        out = []
        oid = output_id.encode()
        for i in range(self._check(self.lib.smr_renderer_node_count(self._h, oid))):
            info = _ffi.SceneNode()
            self._check(self.lib.smr_renderer_node_info(self._h, oid, i, C.byref(info)))
            out.append(Node(i, info.kind, info.parent, [], info.width, info.height, (info.ref_id or b"").decode(),
                            (info.id or b"").decode(), (info.payload or b"").decode()))
        for n in out:
            if n.parent >= 0:
                out[n.parent].children.append(n.index)
        return out

    def set_text(self, output_id: str, node: int, glyphs: Sequence, atlas: np.ndarray, bg: Sequence[float] = (0.0, 0.0, 0.0, 0.0)):
        """The glyph run of a Text node (shaping / rasterisation is the caller's); to be supplied once after every update_scene."""
        atlas = np.ascontiguousarray(atlas, dtype=np.uint8)
        garr = (_ffi.Glyph * max(len(glyphs), 1))()
        for i, g in enumerate(glyphs):
            garr[i].dst_x, garr[i].dst_y, garr[i].w, garr[i].h = g.dst_x, g.dst_y, g.w, g.h
            garr[i].atlas_x, garr[i].atlas_y = g.atlas_x, g.atlas_y
            garr[i].color[:] = list(g.color)
        bgc = (C.c_float * 4)(*[float(x) for x in bg])
        self._check(self.lib.smr_renderer_set_text(self._h, output_id.encode(), node, bgc, garr, len(glyphs), atlas.ctypes.data,
                                                   atlas.shape[1], atlas.shape[0]))

    # -- per frame (state.rs:173, 220-252)
    def make_frame_set(self, frames: Dict[str, DeviceFrame], pts_s: Optional[float] = None, frame_pts_s: Optional[Dict[str, float]] = None):
        """Pre-packs a FrameSet (ctypes array) for `render_packed`; keeps the DeviceFrames alive."""
        arr = (_ffi.InputFrame * max(len(frames), 1))()
        keep = []
        for i, (k, f) in enumerate(frames.items()):
            key = k.encode()
            keep.append((key, f))
            arr[i].input_id = key
            arr[i].frame = C.pointer(f.c)
            arr[i].pts_ns = int((frame_pts_s or {}).get(k, pts_s or 0.0) * 1e9)
        return arr, len(frames), keep

    def render_packed(self, pts_ns: int, packed) -> int:
        """One frame for every output; returns the number of outputs (frames are read with `output`)."""
        arr, n, _ = packed
        cnt = C.c_uint32()
        self._check(self.lib.smr_renderer_render(self._h, pts_ns, arr, n, self._outs, self._max_outputs, C.byref(cnt)))
        return cnt.value

    def render(self, pts_s: float, frames: Dict[str, DeviceFrame], frame_pts_s: Optional[Dict[str, float]] = None) -> Dict[str, BorrowedFrame]:
        packed = self.make_frame_set(frames, pts_s, frame_pts_s)
        n = self.render_packed(int(pts_s * 1e9), packed)
        return {self._outs[i].output_id.decode(): self.output(i) for i in range(min(n, self._max_outputs))}
