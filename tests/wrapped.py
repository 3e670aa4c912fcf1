"""Destinations in caller memory for the write-footprint tests (tests/test_gpu_write_footprint.py): the WRITE half of smr_surface_wrap's
contract in include/smr.h — of a surface it does not own the library writes the w x h texels and no other byte.  (The READ half and wrapped
sources: tests/test_gpu_wrap.py and its _device_plane, which stays as it is.)

A destination plane is one torch.uint8 buffer on the device: 256-byte head, pitch * h body, 256-byte tail.  The WHOLE buffer is filled from
a seeded numpy generator before the call — not a constant: a stray store of a value that happens to equal a constant canary would pass —
and a host copy is kept; after the call every byte outside the h rows' first w * bpp bytes must equal that copy.  Three geometries:

    tight   pitch = the row's bytes rounded up to `align` (4: what smr_surface_wrap demands; 16 where a route demands 16-byte pitches)
    slack   tight + 16
    window  the destination is a sub-rectangle of a buffer three times as wide: its base is 16-byte aligned, its pitch is the big row, so
            the bytes left and right of every row are live data (an encoder surface that is a window inside a larger allocation)
"""
import numpy as np

HEAD = TAIL = 256
GEOMETRIES = ("tight", "slack", "window")


def _up(x, a):
    return (x + a - 1) // a * a


class Dest:
    """One destination plane: .ptr / .pitch for smr_surface_wrap, .texels() after the call."""

    def __init__(self, torch, w, h, bpp, geometry, seed, align=4):
        assert geometry in GEOMETRIES and align in (4, 16)
        self.w, self.h, self.bpp, self.geometry = w, h, bpp, geometry
        self.row = w * bpp
        tight = _up(self.row, align)
        if geometry == "window":
            self.x_off = _up(self.row, 16)  # one (16-byte aligned) window width of live data on the left, at least as much on the right
            self.pitch = 3 * self.x_off
        else:
            self.x_off = 0
            self.pitch = tight + (16 if geometry == "slack" else 0)
        self.size = HEAD + self.pitch * h + TAIL
        self.before = np.random.default_rng(seed).integers(0, 256, self.size, dtype=np.uint8)
        self.buf = torch.from_numpy(self.before.copy()).cuda()
        torch.cuda.synchronize()
        self._torch = torch
        self.ptr = self.buf.data_ptr() + HEAD + self.x_off
        assert self.ptr % 16 == 0

    def where(self, off):
        """buffer offset -> 'head' | 'tail' | (row, byte in row: relative to the row's first texel, so < 0 is left of a window)"""
        if off < HEAD:
            return "head"
        if off >= HEAD + self.pitch * self.h:
            return "tail"
        r, b = divmod(off - HEAD, self.pitch)
        return f"row {r}, byte {b - self.x_off} of the row (row bytes {self.row}, pitch {self.pitch})"

    def texels(self, what=""):
        """Downloads the buffer (the caller has synchronised the context), asserts that no byte outside the texels changed and returns the
        texels as an (h, w * bpp) uint8 array."""
        self._torch.cuda.synchronize()
        after = self.buf.cpu().numpy()
        body = after[HEAD:HEAD + self.pitch * self.h].reshape(self.h, self.pitch)
        inside = np.zeros(self.size, bool)
        inside[HEAD:HEAD + self.pitch * self.h].reshape(self.h, self.pitch)[:, self.x_off:self.x_off + self.row] = True
        touched = np.flatnonzero((after != self.before) & ~inside)
        assert touched.size == 0, (f"{what} [{self.geometry} {self.w}x{self.h} bpp {self.bpp}]: {touched.size} bytes outside the texels were written, the first at "
                                   f"{self.where(int(touched[0]))}: 0x{after[touched[0]]:02x} over 0x{self.before[touched[0]]:02x}")
        return body[:, self.x_off:self.x_off + self.row].copy()


_BPP = {0: 4, 1: 8, 2: 1, 3: 2}  # smr_pixel_format -> bytes per texel


class WrappedSurface:
    """A Dest wrapped as a surface of `ctx`: .surface for the call, .texels() -> (h, w, c) array of the format's dtype."""

    def __init__(self, torch, ctx, w, h, fmt, geometry, seed, align=4):
        self.dest = Dest(torch, w, h, _BPP[fmt], geometry, seed, align)
        self.surface = ctx.wrap(self.dest.ptr, self.dest.pitch, w, h, fmt)
        self.fmt = fmt

    def texels(self, what=""):
        t = self.dest.texels(what)
        h, w = self.dest.h, self.dest.w
        if self.fmt == 0:
            return t.reshape(h, w, 4)
        if self.fmt == 1:
            return t.view(np.uint16).reshape(h, w, 4)
        if self.fmt == 3:
            return t.reshape(h, w, 2)
        return t.reshape(h, w)


class WrappedFrame:
    """An output frame whose planes are Dests: .frame for the call, .planes() -> the planes shaped like DeviceFrame.download()'s."""

    def __init__(self, torch, ctx, fmt, w, h, geometry, seed, align=4):
        from smelter_amd import hip
        probe = hip.DeviceFrame.__new__(hip.DeviceFrame)
        probe.fmt, probe.w, probe.h = fmt, w, h
        self.shapes = [tuple(max(int(d), 1) for d in s) for s in probe.plane_shapes()]  # (empty chroma planes are 1 x 1 placeholders)
        self.true_shapes = probe.plane_shapes()
        self.dests = []
        for i, s in enumerate(self.shapes):
            bpp = s[2] if len(s) == 3 else 1
            self.dests.append(Dest(torch, s[1], s[0], bpp, geometry, seed * 3 + i, align))
        self.frame = ctx.wrapped_frame(fmt, w, h, [(d.ptr, d.pitch) for d in self.dests])

    def planes(self, what=""):
        out = []
        for i, (d, s, ts) in enumerate(zip(self.dests, self.shapes, self.true_shapes)):
            t = d.texels(f"{what} plane {i}").reshape(s)
            out.append(t if 0 not in ts else np.empty(ts, np.uint8))
        return out
