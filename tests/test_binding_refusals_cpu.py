"""Every ValueError the ``MadronaRenderer`` constructor and ``ImportedCamera`` raise before a ``Manager`` exists, with
its exact message (no GPU: the refused call never reaches the device), and which refusal wins where two apply.

The scene is the cube-and-plane one of madrona_renderer_amd/scenes.py, 1 world at 16 x 16.  A case is a name and the
keyword arguments it changes; the messages are tests/golden/binding_refusals.json, name -> message, recorded by
``python -m tests.test_binding_refusals_cpu --record`` against the build of the commit before the front ends'
per-feature copies were folded, exactly as that build raised them."""
import json
import os
import sys

import numpy as np
import pytest

from madrona_renderer_amd import scenes

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "binding_refusals.json")
NAN, INF = float("nan"), float("inf")


def _kwargs(m, desc):
    """the constructor's keyword arguments for a SceneDesc, as scenes.make_renderer passes them"""
    return dict(
        gpu_id=0, num_worlds=desc.num_worlds, render_mode=getattr(m.RenderMode, desc.render_mode),
        batch_render_view_width=desc.width, batch_render_view_height=desc.height,
        asset_paths=[m.ImportedAsset(path=p, mat_id=i) for p, i in desc.asset_paths],
        mesh_vertices=desc.mesh_vertices, mesh_uvs=desc.mesh_uvs, mesh_indices=desc.mesh_indices,
        mesh_vertex_offsets=desc.mesh_vertex_offsets, mesh_indices_offsets=desc.mesh_indices_offsets,
        mesh_materials=desc.mesh_materials,
        materials=[m.AdditionalMaterial(color=list(c), texture_id=t, roughness=r, metalness=me)
                   for c, t, r, me in desc.materials],
        texture_paths=list(desc.texture_paths),
        instances=[m.ImportedInstance(position=list(p), rotation=list(q), scale=list(s), object_id=o)
                   for p, q, s, o in desc.instances],
        cameras=[m.ImportedCamera(position=list(p), rotation=list(q)) for p, q in desc.cameras],
        worlds=[m.WorldInit(num_instances=a, instance_offset=b, num_cameras=c, camera_offset=d)
                for a, b, c, d in desc.worlds])


def _obs(**kw):
    return dict(observations=dict(**kw))


def _rng(r, channels="rgbd"):
    return dict(observations=dict(channels=channels, depth_range=r))


TRI = dict(mesh_vertices=np.zeros((3, 3), np.float32), mesh_uvs=np.zeros((3, 2), np.float32),
           mesh_indices=np.arange(3, dtype=np.uint32), mesh_vertex_offsets=np.zeros(1, np.uint32),
           mesh_indices_offsets=np.zeros(1, np.uint32), mesh_materials=np.full(1, -1, np.int32))
LIGHT = ((1.0, -1.0, -0.05), 0.25, 0.75)

# name -> the keyword arguments the case changes ("render_outputs" and "render_mode" by member name; "znear" is no
# keyword of the constructor: the case's cameras are built with that near plane)
CASES = {
    # parseObservations, in the order of its checks
    "obs_key_not_a_string": dict(observations={"channels": "rgb", 3: 4}),
    "obs_channels_not_a_string": _obs(channels=2),
    "obs_dtype_not_a_string": _obs(channels="rgb", dtype=16),
    "obs_stack_a_bool": _obs(channels="rgb", stack=True),
    "obs_stack_a_float": _obs(channels="rgb", stack=2.0),
    "obs_unknown_key": _obs(channels="rgb", frames=4),
    "obs_unknown_key_case": _obs(channels="rgb", Stack=4),
    "obs_dict_without_channels": _obs(dtype="float16"),
    "obs_an_int": dict(observations=3),
    "obs_a_float": dict(observations=1.5),
    "obs_true": dict(observations=True),
    "obs_a_list": dict(observations=["rgb"]),
    "obs_bytes": dict(observations=b"rgb"),
    "obs_unknown_channels": dict(observations="rgba"),
    "obs_empty_channels": dict(observations=""),
    "obs_channels_upper_case": dict(observations="RGB"),
    "obs_unknown_channels_in_dict": _obs(channels="rgbx"),
    "obs_unknown_dtype": _obs(channels="rgb", dtype="float64"),
    "obs_stack_zero": _obs(channels="rgb", stack=0),
    "obs_stack_nine": _obs(channels="rgb", stack=9),
    "obs_rgb_needs_rgb": dict(observations="rgb", render_outputs="Depth"),
    "obs_y_needs_rgb": dict(observations="y", render_outputs="Depth"),
    "obs_rgbd_needs_rgb": dict(observations="rgbd", render_outputs="Depth"),
    "obs_yd_needs_rgb": dict(observations="yd", render_outputs="Depth"),
    "obs_d_needs_depth": dict(observations="d", render_outputs="RGB"),
    "obs_rgbd_needs_depth": dict(observations="rgbd", render_outputs="RGB"),
    "obs_yd_needs_depth": dict(observations=dict(channels="yd", dtype="uint8"), render_outputs="RGB"),
    # parseObsRange
    "range_a_number": _rng(5.0),
    "range_a_string": _rng("01"),
    "range_one_entry": _rng((1.0,)),
    "range_three_entries": _rng((0.0, 1.0, 2.0)),
    "range_three_entries_list": _rng([0.0, 1.0, 2.0]),
    "range_strings": _rng(("0", "1")),
    "range_a_bool": _rng((False, 1.0)),
    "range_none_inside": _rng((0.0, None)),
    "range_empty": _rng((0.0, 0.0)),
    "range_reversed": _rng((5.0, 1.0)),
    "range_negative": _rng((-1.0, 1.0)),
    "range_infinite": _rng((0.0, INF)),
    "range_nan": _rng((NAN, 1.0)),
    "range_beyond_float32": _rng((0.0, 1e39)),
    "range_without_depth_rgb": _rng((0.1, 20.0), "rgb"),
    "range_without_depth_y": _rng((0.1, 20.0), "y"),
    # the constructor, in the order of its checks
    "rays_true": dict(rays=True),
    "rays_false": dict(rays=False),
    "rays_a_float": dict(rays=1.5),
    "rays_a_string": dict(rays="4"),
    "rays_zero": dict(rays=0),
    "rays_negative": dict(rays=-1),
    "rays_too_many": dict(rays=65537),
    "boxes_true": dict(boxes=True),
    "boxes_negative": dict(boxes=-1),
    "boxes_too_many": dict(boxes=1025),
    "boxes_a_float": dict(boxes=1.5),
    "boxes_a_string": dict(boxes="4"),
    "supersample_zero": dict(supersample=0),
    "supersample_five": dict(supersample=5),
    "supersample_negative": dict(supersample=-2),
    "flow_without_depth": dict(flow=True, render_outputs="RGB"),
    "flow_with_boxes": dict(flow=True, boxes=4),
    "positions_unknown_frame": dict(positions="screen"),
    "positions_an_int": dict(positions=3),
    "positions_a_float": dict(positions=1.0),
    "positions_true_without_depth": dict(positions=True, render_outputs="RGB"),
    "positions_view_without_depth": dict(positions="view", render_outputs="RGB"),
    "mesh_vertices_two_columns": dict(TRI, mesh_vertices=np.zeros((3, 2), np.float32)),
    "mesh_vertices_flat": dict(TRI, mesh_vertices=np.zeros(9, np.float32)),
    "mesh_uvs_three_columns": dict(TRI, mesh_uvs=np.zeros((3, 3), np.float32)),
    "mesh_uvs_flat": dict(TRI, mesh_uvs=np.zeros(6, np.float32)),
    "num_worlds_too_many": dict(num_worlds=2),
    "num_worlds_zero": dict(num_worlds=0),
    "mesh_index_offsets_short": dict(TRI, mesh_indices_offsets=np.zeros(0, np.uint32)),
    "mesh_materials_long": dict(TRI, mesh_materials=np.full(2, -1, np.int32)),
    "mesh_uvs_fewer_rows": dict(TRI, mesh_uvs=np.zeros((2, 2), np.float32)),
    "mesh_uvs_none": dict(TRI, mesh_uvs=np.zeros((0, 2), np.float32)),
    "raytracer_znear_at_the_far_plane": dict(render_mode="Raytracer", znear=1000.0),
    "raytracer_znear_beyond_the_far_plane": dict(render_mode="Raytracer", znear=2500.0),
    "max_instances_negative": dict(max_instances_per_world=-1),
    "world_lights_too_few": dict(world_lights=[]),
    "world_lights_too_many": dict(world_lights=[LIGHT, LIGHT]),
    "world_lights_entry_of_two": dict(world_lights=[((1.0, 0.0, 0.0), 0.25)]),
    "world_lights_entry_of_four": dict(world_lights=[((1.0, 0.0, 0.0), 0.25, 0.75, 1.0)]),
    "world_lights_zero_direction": dict(world_lights=[((0.0, 0.0, 0.0), 0.25, 0.75)]),
    "world_lights_direction_not_finite": dict(world_lights=[((INF, 0.0, 0.0), 0.25, 0.75)]),
    "world_lights_negative_ambient": dict(world_lights=[((1.0, 0.0, 0.0), -0.25, 0.75)]),
    "world_lights_nan_diffuse": dict(world_lights=[((1.0, 0.0, 0.0), 0.25, NAN)]),
    "instance_colors_three_columns": dict(instance_colors=np.zeros((2, 3), np.uint8)),
    "instance_colors_too_few_rows": dict(instance_colors=np.zeros((1, 4), np.uint8)),
    "instance_colors_flat": dict(instance_colors=np.zeros(8, np.uint8)),
    "instance_colors_not_an_array": dict(instance_colors="red"),
    "instance_materials_too_many": dict(instance_materials=np.zeros(3, np.int32)),
    "instance_materials_two_dimensional": dict(instance_materials=np.zeros((2, 1), np.int32)),
    "instance_materials_not_an_array": dict(instance_materials="one"),
    "instance_labels_too_few": dict(instance_labels=np.zeros(1, np.int32)),
    "instance_labels_two_dimensional": dict(instance_labels=np.zeros((1, 2), np.int32)),
    "instance_labels_not_an_array": dict(instance_labels="cube"),
    # which of two refusals wins
    "order_observations_before_rays": dict(observations="rgba", rays=0),
    "order_channels_before_dtype": _obs(channels="rgbx", dtype="float64"),
    "order_dtype_before_stack": _obs(channels="rgb", dtype="float64", stack=9),
    "order_stack_before_outputs": dict(observations=dict(channels="rgb", stack=9), render_outputs="Depth"),
    "order_outputs_before_range": dict(observations=dict(channels="d", depth_range=(5.0, 1.0)), render_outputs="RGB"),
    "order_range_before_no_depth": _rng((5.0, 1.0), "rgb"),
    "order_rays_before_supersample": dict(supersample=5, rays=0),
    "order_rays_before_boxes": dict(rays=0, boxes=True),
    "order_boxes_before_supersample": dict(boxes=1025, supersample=5),
    "order_supersample_before_flow": dict(supersample=5, flow=True, render_outputs="RGB"),
    "order_flow_depth_before_flow_boxes": dict(flow=True, render_outputs="RGB", boxes=4),
    "order_flow_before_positions": dict(flow=True, boxes=4, positions="screen"),
    "order_positions_before_meshes": dict(TRI, positions="screen", mesh_vertices=np.zeros((3, 2), np.float32)),
    "order_vertices_before_uvs": dict(TRI, mesh_vertices=np.zeros((3, 2), np.float32), mesh_uvs=np.zeros((3, 3), np.float32)),
    "order_uvs_before_num_worlds": dict(TRI, mesh_uvs=np.zeros((3, 3), np.float32), num_worlds=2),
    "order_num_worlds_before_per_mesh": dict(TRI, num_worlds=2, mesh_materials=np.full(2, -1, np.int32)),
    "order_per_mesh_before_uv_rows": dict(TRI, mesh_materials=np.full(2, -1, np.int32), mesh_uvs=np.zeros((2, 2), np.float32)),
    "order_uv_rows_before_znear": dict(TRI, mesh_uvs=np.zeros((2, 2), np.float32), render_mode="Raytracer", znear=1000.0),
    "order_znear_before_max_instances": dict(render_mode="Raytracer", znear=1000.0, max_instances_per_world=-1),
    "order_max_instances_before_lights": dict(max_instances_per_world=-1, world_lights=[]),
    "order_lights_before_colors": dict(world_lights=[], instance_colors=np.zeros((2, 3), np.uint8)),
    "order_colors_before_materials": dict(instance_colors=np.zeros((2, 3), np.uint8), instance_materials=np.zeros(3, np.int32)),
    "order_materials_before_labels": dict(instance_materials=np.zeros(3, np.int32), instance_labels=np.zeros(1, np.int32)),
}

# ImportedCamera(position, rotation, **these)
CAMERA_CASES = {
    "camera_vfov_zero": dict(vfov=0.0),
    "camera_vfov_negative": dict(vfov=-30.0),
    "camera_vfov_180": dict(vfov=180.0),
    "camera_vfov_nan": dict(vfov=NAN),
    "camera_vfov_infinite": dict(vfov=INF),
    "camera_znear_zero": dict(znear=0.0),
    "camera_znear_negative": dict(znear=-0.5),
    "camera_znear_infinite": dict(znear=INF),
    "camera_znear_nan": dict(znear=NAN),
    "order_camera_znear_before_vfov": dict(vfov=0.0, znear=0.0),
}


def _construct(m, changes):
    desc = scenes.synthetic_scene(1, width=16, height=16)
    changes = dict(changes)
    if "render_mode" in changes:
        desc.render_mode = changes.pop("render_mode")
    kw = _kwargs(m, desc)
    if "znear" in changes:
        znear = changes.pop("znear")
        kw["cameras"] = [m.ImportedCamera(position=list(p), rotation=list(q), znear=znear) for p, q in desc.cameras]
    if "render_outputs" in changes:
        changes["render_outputs"] = getattr(m.RenderOutputs, changes["render_outputs"])
    kw.update(changes)
    return m.MadronaRenderer(**kw)


def _camera(m, changes):
    return m.ImportedCamera(position=[0.0, 0.0, 0.0], rotation=[1.0, 0.0, 0.0, 0.0], **changes)


def _golden():
    return json.load(open(GOLDEN))


@pytest.mark.parametrize("name", list(CASES))
def test_the_constructor_refuses_with_the_recorded_message(native, name):
    with pytest.raises(ValueError) as e:
        _construct(native.load_module(), CASES[name])
    assert type(e.value) is ValueError
    assert str(e.value) == _golden()[name]


@pytest.mark.parametrize("name", list(CAMERA_CASES))
def test_the_camera_refuses_with_the_recorded_message(native, name):
    with pytest.raises(ValueError) as e:
        _camera(native.load_module(), CAMERA_CASES[name])
    assert type(e.value) is ValueError
    assert str(e.value) == _golden()[name]


def test_every_message_of_the_source_is_recorded():
    """each text the constructor's checks can raise is some case's message, and the file has no case this module lacks"""
    golden = _golden()
    assert sorted(golden) == sorted(list(CASES) + list(CAMERA_CASES))
    messages = set(golden.values())
    for text in ("observations: the keys are channels, dtype, stack and depth_range",
                 "observations: channels must be a string", "observations: dtype must be a string",
                 "observations: stack must be an int in 1 ... 8",
                 "observations: unknown key frames (channels, dtype, stack, depth_range)",
                 "observations: the dict needs channels (rgb, rgbd, d, y, yd)",
                 "observations must be None, a channels string or a dict (channels, dtype, stack, depth_range)",
                 "observations: unknown channels rgba (rgb, rgbd, d, y, yd)",
                 "observations: unknown dtype float64 (float32, float16, bfloat16, uint8)",
                 "observations: channels rgb need rgb: render_outputs Depth renders none",
                 "observations: channels d need depth: render_outputs RGB renders none",
                 "observations: depth_range must be None or (lo, hi) with 0 <= lo < hi, both finite",
                 "observations: depth_range with channels rgb, which have no depth",
                 "rays must be None or an int in 1 ... 65536 (the number of rays per world)",
                 "boxes must be None or an int in 1 ... 1024 (the number of labels)",
                 "supersample must be 1, 2, 3 or 4",
                 "flow needs depth: render_outputs RGB renders none",
                 "flow and boxes exclude each other: under flow the ids tensor holds visibility ids, the box stage needs a segmask",
                 "positions must be False, True, \"world\" or \"view\"",
                 "positions need depth: render_outputs RGB renders none",
                 "mesh_vertices must have shape [N, 3]", "mesh_uvs must have shape [N, 2]",
                 "num_worlds does not match len(worlds)",
                 "mesh_vertex_offsets, mesh_indices_offsets and mesh_materials must have one entry per mesh",
                 "mesh_uvs must have one row per row of mesh_vertices",
                 "znear must be below the Raytracer far plane (1000)",
                 "max_instances_per_world must not be negative",
                 "world_lights needs one (direction, ambient, diffuse) per world",
                 "world_lights entries are (direction, ambient, diffuse)",
                 "light direction is zero",
                 "instance_colors must be None, True or a uint8 array of shape [num_instances, 4]",
                 "instance_materials must be None, True or an int32 array of shape [num_instances]",
                 "instance_labels must be None, True or an int32 array of shape [num_instances]",
                 "vfov must be finite and in (0, 180) degrees",
                 "znear must be finite and > 0 (None: the mode's default)"):
        assert text in messages, text


if __name__ == "__main__":
    if "--record" not in sys.argv:
        sys.exit("usage: python -m tests.test_binding_refusals_cpu --record")
    import madrona_renderer_amd
    mod = madrona_renderer_amd.load_module()
    recorded = {}
    for cases, call in ((CASES, _construct), (CAMERA_CASES, _camera)):
        for case, changed in cases.items():
            try:
                call(mod, changed)
            except ValueError as err:
                assert type(err) is ValueError, (case, type(err))
                recorded[case] = str(err)
            else:
                sys.exit("%s: not refused" % case)
    with open(GOLDEN, "w") as f:
        json.dump(recorded, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", GOLDEN, len(recorded))
