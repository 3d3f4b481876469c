"""Minimal DLPack (v0.8 ABI) export of the renderer's own memory, as the compiled module's Tensor.__dlpack__ builds it:
what the pure-Python outputs (cloud.py, shadows.py) hand to torch.from_dlpack.  ctypes only; each capsule keeps its
owner alive for as long as the consumer's tensor lives.  With it, what those modules share beside it: their handle of
the C-ABI and the check of a float argument."""
import ctypes
import math

kDLCPU, kDLROCM = 1, 10
kDLInt, kDLUInt, kDLFloat = 0, 1, 2
MRX_DTYPE_U8, MRX_DTYPE_I32, MRX_DTYPE_F32 = 0, 1, 2
# the C-ABI's dtype -> (DLPack type code, bits)
DTYPES = {MRX_DTYPE_U8: (kDLUInt, 8), MRX_DTYPE_I32: (kDLInt, 32), MRX_DTYPE_F32: (kDLFloat, 32)}


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


def capsule(ptr, shape, code, bits, device_type, device_id, owner):
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


class Exported:
    """What torch.from_dlpack takes: one tensor of the renderer's memory"""

    def __init__(self, ptr, shape, code, bits, device_type, device_id, owner):
        self._args = (ptr, tuple(shape), code, bits, device_type, device_id, owner)

    def __dlpack__(self, **kwargs):
        return capsule(*self._args)

    def __dlpack_device__(self):
        return (self._args[4], self._args[5])


def declare_buffers(lib):
    """The prototypes of the C-ABI's tensor export on the handle `lib`"""
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


_HANDLES = {}


def private_capi(module, prototypes):
    """The library load_capi() mapped, through a handle of `module`'s own: the prototypes set here -- `prototypes`, name
    -> argument types of an entry that returns int, and the tensor export's -- are not imposed on other users of the
    shared handle."""
    if module not in _HANDLES:
        from . import load_capi
        lib = ctypes.CDLL(load_capi()._name)
        for name, argtypes in prototypes.items():
            getattr(lib, name).restype = ctypes.c_int
            getattr(lib, name).argtypes = argtypes
        declare_buffers(lib)
        _HANDLES[module] = lib
    return _HANDLES[module]


def float32_argument(name, value, what, holds):
    """`value` as a float where holds(value), for a finite number, also in single precision; else the ValueError that
    says `name` must be `what`."""
    if isinstance(value, bool) or not isinstance(value, (int, float)) or not math.isfinite(value) or not holds(value):
        raise ValueError("%s must be %s, not %r" % (name, what, value))
    # (the C-ABI takes a float32: a number that is finite, or positive, only in double precision is neither there)
    as_f32 = ctypes.c_float(value).value
    if not math.isfinite(as_f32) or not holds(as_f32):
        raise ValueError("%s must be %s in single precision, not %r" % (name, what, value))
    return float(value)


def positive_or_none(name, value):
    """None, or a finite positive number, also in single precision"""
    return None if value is None else float32_argument(name, value, "None or a finite positive number", lambda v: v > 0)


def last_error(lib):
    return (lib.mrx_last_error() or b"").decode("utf-8", "replace")


def buffer_tensor(lib, handle, which, shard, owner):
    """Buffer `which` of the renderer behind `handle` (of shard `shard`, or of a single-device renderer) as a zero-copy
    torch tensor on the renderer's device"""
    import torch
    dims = (ctypes.c_int64 * 4)(1, 1, 1, 1)
    nd, dt, dev = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    if shard is None:
        n = lib.mrx_num_shards(handle)
        if n > 1:
            raise ValueError("this renderer spans %d devices: say which shard's tensor (shard=i)" % n)
        ptr = lib.mrx_buffer(handle, which, dims, ctypes.byref(nd), ctypes.byref(dt), ctypes.byref(dev))
    else:
        ptr = lib.mrx_buffer_shard(handle, int(shard), which, dims, ctypes.byref(nd), ctypes.byref(dt),
                                   ctypes.byref(dev))
    if not ptr:
        raise RuntimeError(last_error(lib))
    code, bits = DTYPES[dt.value]
    return torch.from_dlpack(Exported(ptr, list(dims)[:nd.value], code, bits, kDLROCM, dev.value, owner))
