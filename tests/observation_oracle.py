"""DESIGN.md S15 in NumPy: the packed observation the observation stage writes, restated operation by operation in
float32 -- every product, sum and conversion a separately rounded NumPy operation -- so that the GPU tests compare bit
patterns.  bfloat16, which NumPy does not have, is integer arithmetic on the float32 bit patterns and comes out as
uint16."""
import numpy as np

LAYOUTS = {"rgb": 1, "rgbd": 2, "d": 3, "y": 4, "yd": 5}
CHANNELS = {"rgb": 3, "rgbd": 4, "d": 1, "y": 1, "yd": 2}
DTYPES = {"float32": 0, "float16": 1, "bfloat16": 2, "uint8": 3}
# what pack() returns for each dtype (bfloat16: the bit patterns)
NP_DTYPES = {"float32": np.float32, "float16": np.float16, "bfloat16": np.uint16, "uint8": np.uint8}
ELEM_BYTES = {"float32": 4, "float16": 2, "bfloat16": 2, "uint8": 1}

K = np.float32(1.0) / np.float32(255.0)         # S8's constant


def field(layout, dtype, stack):
    """MRX_FLAG_OBSERVATIONS(layout, dtype, stack)"""
    return (LAYOUTS[layout] << 23) | (DTYPES[dtype] << 26) | ((stack - 1) << 28)


def bf16_bits(x):
    """float32 -> bfloat16 bit patterns, round to nearest even: (u + 0x7FFF + ((u >> 16) & 1)) >> 16 in 32 bits"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFFFFFF) >> 16).astype(np.uint16)


def luma(rgb):
    r, g, b = (rgb[..., c].astype(np.uint32) for c in range(3))
    return ((77 * r + 150 * g + 29 * b + 128) >> 8).astype(np.uint8)


def depth_value(d, rng):
    """o of S15: raw depth without a range; with one, (d - lo) * inv clamped to 0 ... 1 by selects, the background 1"""
    d = np.asarray(d, np.float32)
    if rng is None:
        return d
    lo, hi = np.float32(rng[0]), np.float32(rng[1])
    inv = np.float32(1.0) / np.float32(hi - lo)
    with np.errstate(over="ignore", invalid="ignore"):
        t = ((d - lo).astype(np.float32) * inv).astype(np.float32)
    t = np.where(t > 0, t, np.float32(0.0))
    t = np.where(t < 1, t, np.float32(1.0))
    return np.where(d == 0, np.float32(1.0), t).astype(np.float32)


def _colour(b, dtype):
    if dtype == "uint8":
        return b.astype(np.uint8)
    return _convert((b.astype(np.float32) * K).astype(np.float32), dtype)


def _convert(v, dtype):
    if dtype == "float32":
        return v.astype(np.float32)
    if dtype == "float16":
        with np.errstate(over="ignore"):
            return v.astype(np.float16)
    return bf16_bits(v)


def _depth(o, dtype):
    if dtype == "uint8":
        c = np.where(o > 0, o, np.float32(0.0))
        c = np.where(c < 1, c, np.float32(1.0)).astype(np.float32)
        return ((c * np.float32(255.0)).astype(np.float32) + np.float32(0.5)).astype(np.float32).astype(np.uint32).astype(np.uint8)
    return _convert(o, dtype)


def pack(rgb, depth, layout, dtype, rng=None, transposed=False):
    """One frame: rgb u8 [views, nslow, nfast, 4] and depth f32 [views, nslow, nfast(, 1)] as the caller sees them (either
    None when the layout does not read it) -> [views, C, H, W]; transposed: the storage is [x][y] and is undone."""
    planes = []
    if layout in ("rgb", "rgbd"):
        planes += [_colour(rgb[..., c], dtype) for c in range(3)]
    elif layout in ("y", "yd"):
        planes.append(_colour(luma(rgb), dtype))
    if layout in ("rgbd", "d", "yd"):
        d = np.asarray(depth, np.float32)
        d = d.reshape(d.shape[:3])
        planes.append(_depth(depth_value(d, rng), dtype))
    out = np.stack(planes, axis=1)
    assert out.shape[1] == CHANNELS[layout] and out.dtype == NP_DTYPES[dtype]
    return np.ascontiguousarray(out.transpose(0, 1, 3, 2)) if transposed else out


class Stack:
    """The tensor of a stacked renderer: push() is one run of the stage."""

    def __init__(self, stack):
        self.stack = stack
        self.tensor = None

    def push(self, frame, reset_mask=None):
        """frame [views, C, H, W]; reset_mask: the views whose every frame becomes this one (the first push: all)"""
        views, C = frame.shape[:2]
        if self.tensor is None:
            self.tensor = np.zeros((views, self.stack * C) + frame.shape[2:], frame.dtype)
            reset_mask = np.ones(views, bool)
        reset = np.zeros(views, bool) if reset_mask is None else np.asarray(reset_mask, bool)
        t = self.tensor
        if self.stack > 1:
            t[:, :-C] = t[:, C:].copy()                     # frames 1 ... S-1 move to 0 ... S-2
        t[:, -C:] = frame
        t[reset] = np.tile(frame[reset], (1, self.stack, 1, 1))
        return t


def bits(a):
    """the bit patterns of an array of any of the four element types"""
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.dtype.itemsize])
