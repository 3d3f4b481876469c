"""The expected images of a supersampled renderer: the oracle's render of the sample image --
the same desc at s * W x s * H, nothing under oracle/ changes -- resolved with NumPy integer arithmetic:

    rgb[y][x][c]  = (sum over 0 <= i, j < s of sample[s*y + j][s*x + i][c] + s*s // 2) // (s*s)
    other[y][x]   = sample[s*y + s//2][s*x + s//2]          (depth, tri_id, segmask, normals, labels: not filtered)

in storage coordinates; the rule is the same along both axes, so it commutes with the Raytracer transposition.  It
composes with the projection, light, colour, material, label and normal oracles by taking their renders of the
sample-sized desc as input: `resolve` accepts any dict of [views, slow, fast(, 4)] arrays."""
import dataclasses

import numpy as np

FILTERED = ("rgb",)


def sample_desc(desc, s=None):
    """The desc of the sample image: `desc` at s times the width and height, itself not supersampled."""
    s = int(desc.supersample if s is None else s)
    return dataclasses.replace(desc, width=desc.width * s, height=desc.height * s, supersample=1)


def box(a, s):
    """[V, s*H, s*W, C] uint8 -> [V, H, W, C] uint8: the box filter, round half up."""
    a = np.asarray(a)
    assert a.dtype == np.uint8 and a.shape[1] % s == 0 and a.shape[2] % s == 0, (a.dtype, a.shape, s)
    v, hh, ww = a.shape[:3]
    t = a.reshape((v, hh // s, s, ww // s, s) + a.shape[3:]).astype(np.uint32)
    return ((t.sum(axis=(2, 4)) + (s * s) // 2) // (s * s)).astype(np.uint8)


def point(a, s):
    """[V, s*H, s*W, ...] -> [V, H, W, ...]: sample (s // 2, s // 2) of every footprint, bits untouched."""
    a = np.asarray(a)
    assert a.shape[1] % s == 0 and a.shape[2] % s == 0, (a.shape, s)
    return np.ascontiguousarray(a[:, s // 2::s, s // 2::s])


def resolve(ref, s):
    """A render (a dict of images, or one rgb array) of the sample image -> the native images."""
    if not isinstance(ref, dict):
        return box(ref, s) if s > 1 else np.asarray(ref)
    out = {}
    for k, a in ref.items():
        if not isinstance(a, np.ndarray):
            continue
        out[k] = a if s == 1 else box(a, s) if k in FILTERED else point(a, s)
    return out


def render(desc, s=None, render_fn=None, **kw):
    """The oracle at s * W x s * H, resolved.  `render_fn(sample_desc, **kw)` (default: oracle.FlatScene(d).render)
    is where another oracle's render goes in."""
    s = int(desc.supersample if s is None else s)
    d = sample_desc(desc, s)
    if render_fn is None:
        from oracle import oracle
        ref = oracle.FlatScene(d).render(**kw)
    else:
        ref = render_fn(d, **kw)
    return resolve(ref, s)
