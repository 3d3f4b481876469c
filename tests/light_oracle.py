"""The oracle under per-world lights: oracle/oracle.py reads LIGHT_DIR, AMBIENT and DIFFUSE as module globals at
render time, so worlds are rendered in groups of equal light -- the globals set per group to the float32 values the
renderer is given -- through tests/projection_oracle.py (with their views' projections), and the results merged.
Nothing under oracle/ changes."""
import numpy as np

from tests import projection_oracle as po

# the light every world has by default.  The oracle's direction is written in double and -0.05 is not a float: a
# light whose float32 direction is the default's rounding IS the default, resolved from the doubles.
DEFAULT_DIR = (1.0, -1.0, -0.05)
DEFAULT = (DEFAULT_DIR, 0.25, 0.75)


def _key(light):
    d, a, f = light
    d32 = tuple(float(np.float32(x)) for x in d)
    if d32 == tuple(float(np.float32(x)) for x in DEFAULT_DIR):
        d32 = DEFAULT_DIR
    return d32, float(np.float32(a)), float(np.float32(f))


def world_lights(desc):
    """(direction, ambient, diffuse) of every world of `desc`."""
    lights = getattr(desc, "world_lights", None)
    return list(lights) if lights is not None else [DEFAULT] * desc.num_worlds


def render(desc, lights=None, projections=None, view_begin=0, view_end=None, **kw):
    """projection_oracle.render(desc, projections, view_begin, view_end, **kw) with world w under lights[w] (default:
    the desc's own).  Each group of worlds of one light is rendered under that light -- its views a world each, under
    their own projections -- and scattered back; views outside [view_begin, view_end) are left as the oracle leaves
    them (zeros / -1)."""
    import dataclasses

    from oracle import oracle
    per_world = list(lights) if lights is not None else world_lights(desc)
    assert len(per_world) == desc.num_worlds
    per_view_proj = list(projections) if projections is not None else po.view_projections(desc)
    view_world = [(w, (ni, io, 1, co + c)) for w, (ni, io, nc, co) in enumerate(desc.worlds) for c in range(nc)]
    if view_end is None:
        view_end = len(view_world)
    groups = {}
    for v in range(view_begin, view_end):
        groups.setdefault(_key(per_world[view_world[v][0]]), []).append(v)
    saved = (oracle.LIGHT_DIR, oracle.AMBIENT, oracle.DIFFUSE)
    merged = None
    try:
        for (d, a, f), views in groups.items():
            oracle.LIGHT_DIR, oracle.AMBIENT, oracle.DIFFUSE = d, a, f
            sub = dataclasses.replace(desc)
            sub.worlds = [view_world[v][1] for v in views]
            sub.num_worlds = len(views)
            sub.camera_projections = None
            if hasattr(sub, "world_lights"):
                sub.world_lights = None
            out = po.render(sub, [per_view_proj[v] for v in views], **kw)
            if merged is None:
                merged = {}
                for k, arr in out.items():
                    if isinstance(arr, np.ndarray):
                        full = np.zeros((len(view_world),) + arr.shape[1:], arr.dtype)
                        if arr.dtype == np.int32:
                            full[:] = -1
                        merged[k] = full
                    else:
                        merged[k] = arr
            idx = np.asarray(views)
            for k, arr in out.items():
                if isinstance(arr, np.ndarray):
                    merged[k][idx] = arr
    finally:
        oracle.LIGHT_DIR, oracle.AMBIENT, oracle.DIFFUSE = saved
    return merged


# a deterministic cycle: the default (those worlds keep the pixels they always had), the light along +/- each axis,
# a grazing one, ambient only, diffuse only and an over-bright setting (the u8 clamp decides)
CYCLE = (
    DEFAULT,
    ((1.0, 0.0, 0.0), 0.2, 0.8),
    ((-1.0, 0.0, 0.0), 0.3, 0.6),
    ((0.0, 1.0, 0.0), 0.1, 0.9),
    ((0.0, -1.0, 0.0), 0.25, 0.75),
    ((0.0, 0.0, 1.0), 0.15, 0.7),
    ((0.0, 0.0, -1.0), 0.1, 0.9),
    ((3.0, 2.0, -0.01), 0.2, 0.75),          # grazing: almost in the ground plane, not unit length
    ((-0.3, 0.7, -0.4), 1.0, 0.0),           # ambient only
    ((0.5, -0.25, -2.0), 0.0, 1.0),          # diffuse only
    ((-1.0, -1.0, -1.0), 0.9, 0.9),          # over-bright
)


def mixed(n, shift=0):
    """n lights cycling through CYCLE (from entry `shift` on)."""
    return [CYCLE[(i + shift) % len(CYCLE)] for i in range(n)]
