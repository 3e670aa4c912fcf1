"""smelter_amd — Smelter's renderer on AMD Instinct GPUs (HIP, gfx950)."""


def animated_frame_index(delays_ns, pts_ns, start_pts_ns=0):
    """The frame an animated image shows at `pts_ns` on a clock started at `start_pts_ns` (include/smr.h: smr_animated_frame_index)."""
    from .scene import animated_frame_index as impl  # (the library is loaded when something is asked of it, not at import)
    return impl(delays_ns, pts_ns, start_pts_ns)
