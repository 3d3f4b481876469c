"""The refusals of the binding that need a live renderer (-m gpu): every ValueError of set_camera_projection,
set_world_light, set_instance_labels, set_instance_materials, set_observation_depth_range and sample_tensor, the
IndexError of shard= out of range, and the RuntimeError of an output the renderer lacks, with exact types and
messages, and which refusal wins where two apply.  One renderer serves every case: 2 worlds at 16 x 16, Rasterizer,
the cube-and-plane scene, with the label and the material column; a refused call leaves it as it was.

The expected strings are the literals of csrc/py_module.cpp and of the library (csrc/scene.cpp, mrx_api.cpp,
stages.cpp) at the commit before the front ends' per-feature copies were folded."""
import numpy as np
import pytest

from madrona_renderer_amd import scenes

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
ZNEAR = "znear must be finite and > 0 (None: the mode's default)"
VFOV = "vfov must be finite and in (0, 180) degrees"
RANGE = "observations: depth_range must be None or (lo, hi) with 0 <= lo < hi, both finite"
NO_OBS = "no observation depth range: this renderer was created without MRX_FLAG_OBSERVATIONS"
DIRECTION = "direction must be one (x, y, z) or an array of shape [n, 3]"
X = (1.0, 0.0, 0.0)

# (method, positional arguments, keyword arguments, exception, message)
CASES = [
    # set_camera_projection(vfov, znear=None, first_view=0): the renderer has 2 views
    ("set_camera_projection", (60.0,), dict(first_view=-1), ValueError, "first_view out of range"),
    ("set_camera_projection", (60.0,), dict(first_view=3), ValueError, "first_view out of range"),
    ("set_camera_projection", (60.0,), dict(znear=0.0), ValueError, ZNEAR),
    ("set_camera_projection", (60.0,), dict(znear=-0.5), ValueError, ZNEAR),
    ("set_camera_projection", (60.0,), dict(znear=INF), ValueError, ZNEAR),
    ("set_camera_projection", (60.0,), dict(znear=[0.5, NAN]), ValueError, ZNEAR),
    ("set_camera_projection", ([60.0, 70.0],), dict(znear=[0.1, 0.2, 0.3]), ValueError, "vfov and znear differ in length"),
    ("set_camera_projection", ([60.0, 70.0, 80.0],), {}, ValueError, "more projections than views from first_view on"),
    ("set_camera_projection", (60.0,), dict(znear=[0.1, 0.2, 0.3]), ValueError, "more projections than views from first_view on"),
    ("set_camera_projection", ([60.0, 70.0],), dict(first_view=1), ValueError, "more projections than views from first_view on"),
    ("set_camera_projection", (0.0,), {}, ValueError, VFOV),
    ("set_camera_projection", (180.0,), {}, ValueError, VFOV),
    ("set_camera_projection", (NAN,), {}, ValueError, VFOV),
    ("set_camera_projection", ([60.0, -60.0],), {}, ValueError, VFOV),
    # ... in the order first_view, znear, the lengths, the count, vfov
    ("set_camera_projection", (0.0,), dict(znear=0.0, first_view=-1), ValueError, "first_view out of range"),
    ("set_camera_projection", ([0.0, 70.0],), dict(znear=[0.1, 0.2, 0.0]), ValueError, ZNEAR),
    ("set_camera_projection", ([0.0, 70.0, 80.0],), dict(znear=[0.1, 0.2]), ValueError, "vfov and znear differ in length"),
    ("set_camera_projection", ([0.0, 70.0, 80.0],), {}, ValueError, "more projections than views from first_view on"),
    # set_world_light(direction, ambient=None, diffuse=None, first_world=0): 2 worlds
    ("set_world_light", (X,), dict(first_world=-1), ValueError, "first_world out of range"),
    ("set_world_light", (X,), dict(first_world=3), ValueError, "first_world out of range"),
    ("set_world_light", ((1.0, 0.0),), {}, ValueError, DIRECTION),
    ("set_world_light", (1.0,), {}, ValueError, DIRECTION),
    ("set_world_light", ([[1.0, 0.0, 0.0, 0.0]],), {}, ValueError, DIRECTION),
    ("set_world_light", (np.zeros((1, 1, 3), np.float32),), {}, ValueError, DIRECTION),
    ("set_world_light", ([X, X],), dict(ambient=[0.1, 0.2, 0.3]), ValueError, "direction, ambient and diffuse differ in length"),
    ("set_world_light", ([X, X],), dict(diffuse=[0.5]), ValueError, "direction, ambient and diffuse differ in length"),
    ("set_world_light", (X,), dict(ambient=[0.1, 0.2], diffuse=[0.5]), ValueError, "direction, ambient and diffuse differ in length"),
    ("set_world_light", ([X, X, X],), {}, ValueError, "more lights than worlds from first_world on"),
    ("set_world_light", (X,), dict(ambient=[0.1, 0.2, 0.3]), ValueError, "more lights than worlds from first_world on"),
    ("set_world_light", ([X, X],), dict(first_world=1), ValueError, "more lights than worlds from first_world on"),
    ("set_world_light", ((0.0, 0.0, 0.0),), {}, ValueError, "light direction is zero"),
    ("set_world_light", ((INF, 0.0, 0.0),), {}, ValueError, "light direction is not finite"),
    ("set_world_light", (X,), dict(ambient=-0.25), ValueError, "light ambient -0.250000 is not a finite value >= 0"),
    ("set_world_light", (X,), dict(diffuse=-2.0), ValueError, "light diffuse -2.000000 is not a finite value >= 0"),
    ("set_world_light", (X,), dict(ambient=INF), ValueError, "light ambient inf is not a finite value >= 0"),
    # ... in the order first_world, the direction's shape, the lengths, the count, the values
    ("set_world_light", ((1.0, 0.0),), dict(first_world=-1), ValueError, "first_world out of range"),
    ("set_world_light", ((1.0, 0.0),), dict(ambient=[0.1, 0.2], diffuse=[0.5]), ValueError, DIRECTION),
    ("set_world_light", ([X, X, X],), dict(ambient=[0.1]), ValueError, "direction, ambient and diffuse differ in length"),
    ("set_world_light", (np.zeros((3, 3), np.float32),), {}, ValueError, "more lights than worlds from first_world on"),
    ("set_world_light", ((0.0, 0.0, 0.0),), dict(ambient=-0.25), ValueError, "light direction is zero"),
    # set_instance_labels(labels, first_row=0) and set_instance_materials(materials, first_row=0): 4 rows
    ("set_instance_labels", (np.zeros((2, 2), np.int32),), {}, ValueError, "labels must be a one-dimensional int32 array"),
    ("set_instance_labels", (np.zeros(2, np.int32),), dict(first_row=-1), ValueError, "more labels than instance rows from first_row on"),
    ("set_instance_labels", (np.zeros(5, np.int32),), {}, ValueError, "more labels than instance rows from first_row on"),
    ("set_instance_labels", (np.zeros(2, np.int32),), dict(first_row=3), ValueError, "more labels than instance rows from first_row on"),
    ("set_instance_labels", (np.zeros(0, np.int32),), dict(first_row=5), ValueError, "more labels than instance rows from first_row on"),
    ("set_instance_labels", (np.zeros((3, 3), np.int32),), dict(first_row=-1), ValueError, "labels must be a one-dimensional int32 array"),
    ("set_instance_materials", (np.zeros((2, 2), np.int32),), {}, ValueError, "materials must be a one-dimensional int32 array"),
    ("set_instance_materials", (np.zeros(2, np.int32),), dict(first_row=-1), ValueError, "more material ids than instance rows from first_row on"),
    ("set_instance_materials", (np.zeros(5, np.int32),), {}, ValueError, "more material ids than instance rows from first_row on"),
    ("set_instance_materials", (np.zeros(2, np.int32),), dict(first_row=3), ValueError, "more material ids than instance rows from first_row on"),
    ("set_instance_materials", (np.zeros(0, np.int32),), dict(first_row=5), ValueError, "more material ids than instance rows from first_row on"),
    ("set_instance_materials", (np.zeros((3, 3), np.int32),), dict(first_row=-1), ValueError, "materials must be a one-dimensional int32 array"),
    # set_observation_depth_range(lo, hi=None): a malformed range is a ValueError, and the renderer has no observations
    ("set_observation_depth_range", (1.0,), {}, ValueError, RANGE),
    ("set_observation_depth_range", (None, 1.0), {}, ValueError, RANGE),
    ("set_observation_depth_range", ("0", "1"), {}, ValueError, RANGE),
    ("set_observation_depth_range", (False, 1.0), {}, ValueError, RANGE),
    ("set_observation_depth_range", ((0.0, 1.0),), {}, ValueError, RANGE),
    ("set_observation_depth_range", (5.0, 1.0), {}, ValueError, RANGE),
    ("set_observation_depth_range", (1.0, 1.0), {}, ValueError, RANGE),
    ("set_observation_depth_range", (-1.0, 1.0), {}, ValueError, RANGE),
    ("set_observation_depth_range", (0.0, INF), {}, ValueError, RANGE),
    ("set_observation_depth_range", (NAN, 1.0), {}, ValueError, RANGE),
    ("set_observation_depth_range", (0.1, 20.0), {}, RuntimeError, NO_OBS),
    ("set_observation_depth_range", (0, 20), {}, RuntimeError, NO_OBS),
    ("set_observation_depth_range", (None, None), {}, RuntimeError, NO_OBS),
    ("set_observation_depth_range", (None,), {}, RuntimeError, NO_OBS),
    # sample_tensor(name, shard=None): the name, then the shard, then the renderer (supersample 1: no sample tensors)
    ("sample_tensor", ("alpha",), {}, ValueError, "sample_tensor: no output named alpha (rgb, depth, segmask, visibility, normal)"),
    ("sample_tensor", ("",), {}, ValueError, "sample_tensor: no output named  (rgb, depth, segmask, visibility, normal)"),
    ("sample_tensor", ("RGB",), dict(shard=7), ValueError, "sample_tensor: no output named RGB (rgb, depth, segmask, visibility, normal)"),
    ("sample_tensor", ("position",), {}, ValueError, "sample_tensor: no output named position (rgb, depth, segmask, visibility, normal)"),
    ("sample_tensor", ("rgb",), dict(shard=1), IndexError, "shard 1 of 1"),
    ("sample_tensor", ("normal",), dict(shard=-1), IndexError, "shard -1 of 1"),
    ("sample_tensor", ("rgb",), {}, RuntimeError, "no sample tensors: this renderer was created without supersampling"),
    ("sample_tensor", ("depth",), dict(shard=0), RuntimeError, "no sample tensors: this renderer was created without supersampling"),
    # shard= of a getter
    ("rgb_tensor", (), dict(shard=1), IndexError, "shard 1 of 1"),
    ("rgb_tensor", (1,), {}, IndexError, "shard 1 of 1"),
    ("rgb_tensor", (), dict(shard=-1), IndexError, "shard -1 of 1"),
    ("instance_label_tensor", (), dict(shard=2), IndexError, "shard 2 of 1"),
    ("rgb_cuda_ptr", (), dict(shard=1), IndexError, "shard 1 of 1"),
]


def _state(r):
    r.sync()
    return [np.array(a) for a in r.camera_projection() + r.world_light()] + [
        r.instance_labels(), r.instance_materials(), r.rgb_tensor().to_torch().cpu().numpy(),
        r.depth_tensor().to_torch().cpu().numpy()]


def test_every_refusal_of_a_live_renderer():
    desc = scenes.synthetic_scene(2, width=16, height=16)
    desc.instance_labels = True
    desc.instance_materials = True
    r = scenes.make_renderer(desc)
    assert r.num_shards == 1 and r.supersample == 1 and r.observations is None
    assert len(r.camera_projection()[0]) == 2 and len(r.instance_labels()) == 4
    r.step()
    before = _state(r)
    for method, args, kwargs, exc, message in CASES:
        with pytest.raises(exc) as e:
            getattr(r, method)(*args, **kwargs)
        assert type(e.value) is exc, (method, args, kwargs, type(e.value))
        assert str(e.value) == message, (method, args, kwargs)
    # a refused call changed nothing: the tables and the next frame are what they were
    r.step()
    after = _state(r)
    assert len(before) == len(after) == 9
    for a, b in zip(before, after):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    # ... and the calls that were refused go through when they are well-formed
    r.set_camera_projection([60.0, 70.0], znear=[0.1, 0.2])
    r.set_world_light([X, X], ambient=[0.1, 0.2], diffuse=0.5)
    r.set_instance_labels(np.array([7, 8], np.int32), first_row=2)
    r.set_instance_materials(np.array([1], np.int32), first_row=3)
    assert r.camera_projection()[0].tolist() == [60.0, 70.0]
    assert r.world_light()[1].tolist() == [np.float32(0.1), np.float32(0.2)]
    assert r.instance_labels().tolist() == [scenes.LABEL_OBJECT, scenes.LABEL_OBJECT, 7, 8]
    assert r.instance_materials().tolist() == [-1, -1, -1, 1]
