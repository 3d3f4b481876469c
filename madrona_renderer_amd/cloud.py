"""The point-cloud output of a ``MadronaRenderer``: N points per view from the HIP compaction
stage, attached after creation through the C-ABI.

    from madrona_renderer_amd import cloud
    c = cloud.attach(r, 1024, frame="world", max_depth=30.0)
    r.step()
    pts = c.points_tensor()      # float32 [views, 1024, 4], zero-copy, on the renderer's device
    pix = c.pixel_tensor()       # int32 [views, 1024]: y * W + x of every point's pixel, -1 in an empty slot
    m = c.count_tensor()         # int32 [views]: the valid pixels of the view

Pure Python over ``load_capi()``: no rendering code, no fallback.  The tensors are views of the renderer's own memory,
handed to torch as DLPack capsules built with ctypes; each keeps the renderer alive.
"""
import ctypes

from . import _dlpack
# (the DLPack helpers live in _dlpack.py, shared with shadows.py; the names this module always had stay)
from ._dlpack import Exported as _Exported, _LIVE, kDLCPU as _kDLCPU, kDLInt as _kDLInt, kDLFloat as _kDLFloat  # noqa: F401

__all__ = ["attach", "Cloud", "MAX_POINTS", "FRAMES"]

MAX_POINTS = 65536
FRAMES = {"world": 1, "view": 2}                    # mrx_positions' values
MRX_BUF_CLOUD, MRX_BUF_CLOUD_PIXEL, MRX_BUF_CLOUD_COUNT = 23, 24, 25


def _check_arguments(points, frame, max_depth):
    """The ValueErrors of attach(), before any native call -> (N, frame id, max_depth as the C-ABI takes it)"""
    if isinstance(points, bool) or not isinstance(points, int) or not 1 <= points <= MAX_POINTS:
        raise ValueError("points must be an int in 1 ... %d, not %r" % (MAX_POINTS, points))
    if not isinstance(frame, str) or frame not in FRAMES:
        raise ValueError("frame must be \"world\" or \"view\", not %r" % (frame,))
    return points, FRAMES[frame], _dlpack.positive_or_none("max_depth", max_depth) or 0.0


def _capi():
    return _dlpack.private_capi(__name__, {
        "mrx_cloud_create": [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int, ctypes.c_float],
        "mrx_compact": [ctypes.c_void_p], "mrx_cloud": [ctypes.c_void_p]})


_error = _dlpack.last_error


class Cloud:
    """The point-cloud output of one renderer (attach() makes it)."""

    def __init__(self, renderer, handle, points, frame, max_depth):
        self._r = renderer                          # the tensors are its memory
        self._h = handle
        self._points, self._frame, self._max_depth = points, frame, max_depth

    points = property(lambda self: self._points, doc="N, the slots per view")
    frame = property(lambda self: self._frame, doc="\"world\" or \"view\"")
    max_depth = property(lambda self: self._max_depth, doc="the far crop, or None")

    def _tensor(self, which, shard):
        return _dlpack.buffer_tensor(_capi(), self._h, which, shard, self._r)

    def points_tensor(self, shard=None):
        """float32 [views, N, 4]: (x, y, z, 1) per filled slot, (0, 0, 0, 0) per empty one"""
        return self._tensor(MRX_BUF_CLOUD, shard)

    def pixel_tensor(self, shard=None):
        """int32 [views, N]: y * W + x of the slot's pixel in image coordinates, -1 in an empty slot"""
        return self._tensor(MRX_BUF_CLOUD_PIXEL, shard)

    def count_tensor(self, shard=None):
        """int32 [views]: the valid pixels of the view, however many slots there are"""
        return self._tensor(MRX_BUF_CLOUD_COUNT, shard)

    def compact(self):
        """Enqueue the compaction stage alone on the renderer's stream (every shard's on its own)."""
        lib = _capi()
        if lib.mrx_compact(self._h) != 0:
            raise RuntimeError(_error(lib))


def attach(r, points, frame="world", max_depth=None):
    """Attach the point-cloud output to the ``MadronaRenderer`` `r`: `points` slots per view (1 ... 65536), in
    "world" or "view" space, pixels farther than `max_depth` dropped (None: no crop).  From then on every step runs
    the compaction stage.  Once per renderer."""
    n, frame_id, far = _check_arguments(points, frame, max_depth)
    lib = _capi()
    handle = ctypes.c_void_p(r.native_handle())
    if lib.mrx_cloud_create(handle, n, frame_id, far) != 0:
        raise RuntimeError(_error(lib))
    return Cloud(r, handle, n, frame, None if max_depth is None else float(max_depth))
