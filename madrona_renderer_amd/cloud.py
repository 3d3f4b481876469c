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
import math

from . import load_capi

__all__ = ["attach", "Cloud", "MAX_POINTS", "FRAMES"]

MAX_POINTS = 65536
FRAMES = {"world": 1, "view": 2}                    # mrx_positions' values
MRX_BUF_CLOUD, MRX_BUF_CLOUD_PIXEL, MRX_BUF_CLOUD_COUNT = 23, 24, 25
_MRX_DTYPE_I32, _MRX_DTYPE_F32 = 1, 2

# ---- minimal DLPack (v0.8 ABI), as the compiled module's Tensor.__dlpack__ builds it
_kDLCPU, _kDLROCM = 1, 10
_kDLInt, _kDLFloat = 0, 2


class _DLDevice(ctypes.Structure):
    _fields_ = [("device_type", ctypes.c_int32), ("device_id", ctypes.c_int32)]


class _DLDataType(ctypes.Structure):
    _fields_ = [("code", ctypes.c_uint8), ("bits", ctypes.c_uint8), ("lanes", ctypes.c_uint16)]


class _DLTensor(ctypes.Structure):
    _fields_ = [("data", ctypes.c_void_p), ("device", _DLDevice), ("ndim", ctypes.c_int32), ("dtype", _DLDataType),
                ("shape", ctypes.POINTER(ctypes.c_int64)), ("strides", ctypes.POINTER(ctypes.c_int64)),
                ("byte_offset", ctypes.c_uint64)]


class _DLManagedTensor(ctypes.Structure):
    pass


_DELETER = ctypes.CFUNCTYPE(None, ctypes.POINTER(_DLManagedTensor))
_DLManagedTensor._fields_ = [("dl_tensor", _DLTensor), ("manager_ctx", ctypes.c_void_p), ("deleter", _DELETER)]

# what the capsules in flight point into, by address: the managed tensor, its shape array and the owner of the memory
_LIVE = {}


@_DELETER
def _dl_deleter(managed):
    _LIVE.pop(ctypes.addressof(managed.contents), None)


_CAPSULE_DTOR = ctypes.CFUNCTYPE(None, ctypes.c_void_p)


@_CAPSULE_DTOR
def _capsule_destructor(capsule):
    # a capsule nobody consumed still owns its tensor (a consumed one is renamed "used_dltensor" and owns nothing)
    api = ctypes.pythonapi
    if api.PyCapsule_IsValid(ctypes.c_void_p(capsule), b"dltensor"):
        _LIVE.pop(api.PyCapsule_GetPointer(ctypes.c_void_p(capsule), b"dltensor"), None)


def _capsule(ptr, shape, code, bits, device_type, device_id, owner):
    """A "dltensor" capsule for a dense row-major tensor at address `ptr`; `owner` lives as long as the consumer's
    tensor does."""
    api = ctypes.pythonapi
    api.PyCapsule_New.restype = ctypes.py_object
    api.PyCapsule_New.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_void_p]
    api.PyCapsule_IsValid.restype = ctypes.c_int
    api.PyCapsule_IsValid.argtypes = [ctypes.c_void_p, ctypes.c_char_p]
    api.PyCapsule_GetPointer.restype = ctypes.c_void_p
    api.PyCapsule_GetPointer.argtypes = [ctypes.c_void_p, ctypes.c_char_p]
    dims = (ctypes.c_int64 * len(shape))(*shape)
    m = _DLManagedTensor()
    m.dl_tensor.data = ptr
    m.dl_tensor.device = _DLDevice(device_type, device_id)
    m.dl_tensor.ndim = len(shape)
    m.dl_tensor.dtype = _DLDataType(code, bits, 1)
    m.dl_tensor.shape = ctypes.cast(dims, ctypes.POINTER(ctypes.c_int64))
    m.dl_tensor.strides = None
    m.dl_tensor.byte_offset = 0
    m.manager_ctx = None
    m.deleter = _dl_deleter
    addr = ctypes.addressof(m)
    _LIVE[addr] = (m, dims, owner)
    return api.PyCapsule_New(addr, b"dltensor", ctypes.cast(_capsule_destructor, ctypes.c_void_p))


class _Exported:
    """What torch.from_dlpack takes: one tensor of the renderer's memory"""

    def __init__(self, ptr, shape, code, bits, device_type, device_id, owner):
        self._args = (ptr, tuple(shape), code, bits, device_type, device_id, owner)

    def __dlpack__(self, **kwargs):
        return _capsule(*self._args)

    def __dlpack_device__(self):
        return (self._args[4], self._args[5])


def _check_arguments(points, frame, max_depth):
    """The ValueErrors of attach(), before any native call -> (N, frame id, max_depth as the C-ABI takes it)"""
    if isinstance(points, bool) or not isinstance(points, int) or not 1 <= points <= MAX_POINTS:
        raise ValueError("points must be an int in 1 ... %d, not %r" % (MAX_POINTS, points))
    if not isinstance(frame, str) or frame not in FRAMES:
        raise ValueError("frame must be \"world\" or \"view\", not %r" % (frame,))
    if max_depth is None:
        return points, FRAMES[frame], 0.0
    if isinstance(max_depth, bool) or not isinstance(max_depth, (int, float)) or not math.isfinite(max_depth) \
            or not max_depth > 0:
        raise ValueError("max_depth must be None or a finite positive number, not %r" % (max_depth,))
    # (the C-ABI takes a float32: a number that is finite and positive only in double precision is neither there)
    as_f32 = ctypes.c_float(max_depth).value
    if not math.isfinite(as_f32) or not as_f32 > 0:
        raise ValueError("max_depth must be None or a finite positive number in single precision, not %r" % (max_depth,))
    return points, FRAMES[frame], float(max_depth)


_LIB = None


def _capi():
    """The library load_capi() mapped, through a handle of this module's own: the prototypes set here are not imposed
    on other users of the shared handle."""
    global _LIB
    if _LIB is not None:
        return _LIB
    lib = ctypes.CDLL(load_capi()._name)
    lib.mrx_cloud_create.restype = ctypes.c_int
    lib.mrx_cloud_create.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int, ctypes.c_float]
    for name in ("mrx_compact", "mrx_cloud"):
        getattr(lib, name).restype = ctypes.c_int
        getattr(lib, name).argtypes = [ctypes.c_void_p]
    lib.mrx_num_shards.restype = ctypes.c_int
    lib.mrx_num_shards.argtypes = [ctypes.c_void_p]
    lib.mrx_last_error.restype = ctypes.c_char_p
    lib.mrx_last_error.argtypes = []
    for name in ("mrx_buffer", "mrx_buffer_shard"):
        getattr(lib, name).restype = ctypes.c_void_p
    lib.mrx_buffer.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int64),
                               ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    lib.mrx_buffer_shard.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int64),
                                     ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int),
                                     ctypes.POINTER(ctypes.c_int)]
    _LIB = lib
    return lib


def _error(lib):
    return (lib.mrx_last_error() or b"").decode("utf-8", "replace")


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
        import torch
        lib = _capi()
        dims = (ctypes.c_int64 * 4)(1, 1, 1, 1)
        nd, dt, dev = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
        if shard is None:
            n = lib.mrx_num_shards(self._h)
            if n > 1:
                raise ValueError("this renderer spans %d devices: say which shard's tensor (shard=i)" % n)
            ptr = lib.mrx_buffer(self._h, which, dims, ctypes.byref(nd), ctypes.byref(dt), ctypes.byref(dev))
        else:
            ptr = lib.mrx_buffer_shard(self._h, int(shard), which, dims, ctypes.byref(nd), ctypes.byref(dt),
                                       ctypes.byref(dev))
        if not ptr:
            raise RuntimeError(_error(lib))
        code = _kDLFloat if dt.value == _MRX_DTYPE_F32 else _kDLInt
        return torch.from_dlpack(_Exported(ptr, list(dims)[:nd.value], code, 32, _kDLROCM, dev.value, self._r))

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
