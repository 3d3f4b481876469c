"""Cast shadows of a ``MadronaRenderer``: a shadow mask, and rgb darkened where the light of the
pixel's world does not reach, from the HIP shadow stage, attached after creation through the C-ABI.

    from madrona_renderer_amd import shadows
    s = shadows.attach(r, apply=True)        # r was made with normals=True
    r.step()
    m = s.mask_tensor()          # uint8 [views, H, W], zero-copy, on the renderer's device: 0 in shadow, 255 elsewhere
    rgb = r.rgb_tensor()         # occluded pixels hold their ambient-only colour

Pure Python over ``load_capi()``: no rendering code, no fallback.  The tensor is a view of the renderer's own memory,
handed to torch as a DLPack capsule built with ctypes; it keeps the renderer alive.
"""
import ctypes

from . import _dlpack

__all__ = ["attach", "Shadows", "DEFAULT_BIAS"]

DEFAULT_BIAS = 2.0 ** -10
MRX_BUF_SHADOW = 26
_FLT_MAX = ctypes.c_float(3.402823466e+38).value        # MRX_SHADOW_NO_MAX_DISTANCE: no max_distance


def _check_arguments(apply, bias, max_distance):
    """The ValueErrors of attach(), before any native call -> (apply as 0 / 1, bias, max_distance as the C-ABI takes
    them)"""
    if not isinstance(apply, bool):
        raise ValueError("apply must be True or False, not %r" % (apply,))
    b = _dlpack.float32_argument("bias", bias, "a finite number >= 0", lambda v: v >= 0)
    return int(apply), b, _dlpack.positive_or_none("max_distance", max_distance) or _FLT_MAX


def _capi():
    return _dlpack.private_capi(__name__, {
        "mrx_shadow_create": [ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_float],
        "mrx_shadow": [ctypes.c_void_p], "mrx_shadows": [ctypes.c_void_p]})


class Shadows:
    """The shadow stage of one renderer (attach() makes it)."""

    def __init__(self, renderer, handle, apply, bias, max_distance):
        self._r = renderer                          # the tensor is its memory
        self._h = handle
        self._apply, self._bias, self._max_distance = apply, bias, max_distance

    apply = property(lambda self: self._apply, doc="True: every step darkens the rgb of occluded pixels")
    bias = property(lambda self: self._bias, doc="tmin of a shadow ray is bias * depth")
    max_distance = property(lambda self: self._max_distance, doc="the reach of a shadow ray, or None")

    def mask_tensor(self, shard=None):
        """uint8 [views, H, W] (Raytracer mode: [views, res, res], transposed), stored exactly like depth: 0 where the
        pixel is in shadow, 255 on every other pixel, background included"""
        return _dlpack.buffer_tensor(_capi(), self._h, MRX_BUF_SHADOW, shard, self._r)

    def cast(self):
        """Enqueue the shadow stage alone on the renderer's stream (every shard's on its own), in its mask-only form
        whatever `apply` is: rgb stays as the last step left it, however often this is called."""
        lib = _capi()
        if lib.mrx_shadow(self._h) != 0:
            raise RuntimeError(_dlpack.last_error(lib))


def attach(r, apply=True, bias=DEFAULT_BIAS, max_distance=None):
    """Attach cast shadows to the ``MadronaRenderer`` `r`.  From then on every step runs the shadow stage behind the
    render: one ray per pixel from the pixel's world point towards its world's light, from `bias` * depth to
    `max_distance` (None: no limit).  With `apply` (needs rgb and a renderer made with normals=True) occluded pixels are
    darkened to their ambient-only colour.  Once per renderer."""
    a, b, far = _check_arguments(apply, bias, max_distance)
    lib = _capi()
    handle = ctypes.c_void_p(r.native_handle())
    if lib.mrx_shadow_create(handle, a, b, far) != 0:
        raise RuntimeError(_dlpack.last_error(lib))
    return Shadows(r, handle, bool(apply), float(bias), None if max_distance is None else float(max_distance))
