"""The oracle under per-view projections: oracle/oracle.py reads VFOV_DEG, RASTER_ZNEAR and RT_ZNEAR as module
globals at render time, so views are rendered in groups of equal projection, the globals set per group to the
float32 values the renderer is given, and the results merged.  Nothing under oracle/ changes."""
import numpy as np


def view_projections(desc):
    """(vfov, znear or None) of every view of `desc`, in view order (a view takes its camera row's)."""
    projs = desc.camera_projections or [(90.0, None)] * len(desc.cameras)
    out = []
    for _, _, nc, co in desc.worlds:
        out += [tuple(projs[co + c]) for c in range(nc)]
    return out


def _key(p):
    f, z = p
    return float(np.float32(f)), (None if z is None else float(np.float32(z)))


def render(desc, projections=None, view_begin=0, view_end=None, **kw):
    """oracle.FlatScene(desc).render(view_begin, view_end, **kw) with view v under projections[v] (default: the
    desc's own).  Each group of views of one projection is rendered as a scene of its own -- a world per view,
    aliasing that view's instance rows and camera row -- and scattered back; views outside [view_begin, view_end)
    are left as the oracle leaves them (zeros / -1)."""
    import dataclasses

    from oracle import oracle
    per_view = list(projections) if projections is not None else view_projections(desc)
    view_world = [(ni, io, 1, co + c) for ni, io, nc, co in desc.worlds for c in range(nc)]
    if view_end is None:
        view_end = len(view_world)
    groups = {}
    for v in range(view_begin, view_end):
        groups.setdefault(_key(per_view[v]), []).append(v)
    saved = (oracle.VFOV_DEG, oracle.RASTER_ZNEAR, oracle.RT_ZNEAR)
    merged = None
    try:
        for (f, z), views in groups.items():
            oracle.VFOV_DEG = f
            oracle.RASTER_ZNEAR = saved[1] if z is None else z
            oracle.RT_ZNEAR = saved[2] if z is None else z
            sub = dataclasses.replace(desc)
            sub.worlds = [view_world[v] for v in views]
            sub.num_worlds = len(views)
            out = oracle.FlatScene(sub).render(**kw)
            if merged is None:
                merged = {}
                for k, a in out.items():
                    if isinstance(a, np.ndarray):
                        full = np.zeros((len(view_world),) + a.shape[1:], a.dtype)
                        if a.dtype == np.int32:
                            full[:] = -1
                        merged[k] = full
                    else:
                        merged[k] = a
            idx = np.asarray(views)
            for k, a in out.items():
                if isinstance(a, np.ndarray):
                    merged[k][idx] = a
    finally:
        oracle.VFOV_DEG, oracle.RASTER_ZNEAR, oracle.RT_ZNEAR = saved
    return merged


def mixed(n, fovs=(30.0, 60.0, 90.0, 120.0, 150.0), znears=(None, 0.5, 2.0, None, 3.0)):
    """n projections cycling through the fovs and the znears (a period of 5 x 5 = 25 views)."""
    return [(fovs[i % len(fovs)], znears[(i // len(fovs)) % len(znears)]) for i in range(n)]
