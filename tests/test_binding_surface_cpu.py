"""The surface of the compiled ``madrona_renderer`` module, pinned (no GPU): the public names of the module and of every
bound class, the first line of every callable's pybind11 ``__doc__`` (the generated signature: argument names, types
and defaults), the members of the enums and the value of every ``MRX_*`` attribute, against
tests/golden/binding_surface.json.

That file was produced by ``python -m tests.test_binding_surface_cpu --record`` against the build of the commit before
the front ends' per-feature copies were folded (the binding then still had one hand-written lambda per getter), and
is regenerated the same way when the surface changes on purpose.  It holds what ``surface()`` below returns."""
import inspect
import json
import os
import sys

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "binding_surface.json")

# what every pybind11 class carries, whatever is bound to it
GENERIC = {"__doc__", "__module__", "__dict__", "__weakref__", "__new__", "__qualname__"}


def _first_line(obj):
    return (getattr(obj, "__doc__", None) or "").split("\n")[0]


def _class(cls):
    out = {}
    for name, v in sorted(vars(cls).items()):
        if name in GENERIC:
            continue
        if isinstance(v, property):
            out[name] = {"kind": "property", "doc": _first_line(v.fget), "settable": v.fset is not None}
        elif isinstance(v, cls):                         # an enum's member
            out[name] = {"kind": "member", "value": int(v)}
        elif callable(v):
            out[name] = {"kind": "callable", "doc": _first_line(v)}
        else:
            out[name] = {"kind": type(v).__name__}
    return out


def surface(m):
    out = {"doc": m.__doc__, "constants": {}, "functions": {}, "classes": {}}
    for name in sorted(n for n in dir(m) if not n.startswith("_")):
        v = getattr(m, name)
        if inspect.isclass(v):
            out["classes"][name] = _class(v)
        elif callable(v):
            out["functions"][name] = _first_line(v)
        else:
            out["constants"][name] = v
    return out


def test_the_surface_is_the_recorded_one(native):
    got = surface(native.load_module())
    want = json.load(open(GOLDEN))
    assert sorted(got) == sorted(want)
    assert got["doc"] == want["doc"]
    assert got["constants"] == want["constants"]
    assert all(isinstance(v, int) and not isinstance(v, bool) for v in got["constants"].values())
    assert got["functions"] == want["functions"]
    assert sorted(got["classes"]) == sorted(want["classes"])
    for name, members in want["classes"].items():
        assert sorted(got["classes"][name]) == sorted(members), name
        for member, what in members.items():
            assert got["classes"][name][member] == what, (name, member)
    # the file is not empty-handed: the renderer, its tensor and the camera are in it, with their signatures
    r = want["classes"]["MadronaRenderer"]
    assert r["__init__"]["doc"].startswith("__init__(self: madrona_renderer.MadronaRenderer, gpu_id: ")
    assert r["__init__"]["doc"].endswith("rays: object = None, flow: bool = False) -> None")
    assert r["rgb_tensor"]["doc"].startswith("rgb_tensor(self: object, shard: object = None)")
    assert "__dlpack__" in want["classes"]["Tensor"] and "znear" in want["classes"]["ImportedCamera"]
    assert sum(n.startswith("MRX_") for n in want["constants"]) == 42 and "MRX_FLAG_OBSERVATIONS" in want["functions"]


if __name__ == "__main__":
    if "--record" not in sys.argv:
        sys.exit("usage: python -m tests.test_binding_surface_cpu --record")
    import madrona_renderer_amd
    with open(GOLDEN, "w") as f:
        json.dump(surface(madrona_renderer_amd.load_module()), f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", GOLDEN)
