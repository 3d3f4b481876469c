"""Every refusal of renderer_headless's command line (no GPU: parse() ends the program before any device call), with
the whole stderr text and the exit status, and which refusal comes first where two apply.

A case is a name and an argv (argv[0] is always ``renderer_headless``, whatever the path of the program).  What each
printed is tests/golden/headless_refusals.json, name -> {"stderr", "status"}, recorded by
``python -m tests.test_headless_refusals_cpu --record`` against the build of the commit before the front ends'
per-feature copies were folded, exactly as that build printed it."""
import json
import os
import subprocess
import sys

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "headless_refusals.json")
BASE = ["4", "1", "rast", "64", "64"]
RT = ["4", "1", "rt", "64", "64"]

CASES = {
    # usage()
    "usage_no_arguments": [],
    "usage_four_arguments": ["4", "1", "rast", "64"],
    "usage_unknown_mode": ["4", "1", "raster", "64", "64"],
    "usage_unknown_option": BASE + ["--frobnicate"],
    "usage_positional_after_the_five": BASE + ["7"],
    "usage_dump_without_a_name": BASE + ["--dump-last-frame"],
    "usage_scene_without_a_value": BASE + ["--scene"],
    "usage_gpus_without_a_value": BASE + ["--gpus"],
    "usage_vfov_without_a_value": BASE + ["--vfov"],
    "usage_light_without_a_value": BASE + ["--light"],
    "usage_colors_without_a_value": BASE + ["--instance-colors"],
    "usage_materials_without_a_value": BASE + ["--instance-materials"],
    "usage_labels_without_a_value": BASE + ["--instance-labels"],
    "usage_supersample_without_a_value": BASE + ["--supersample"],
    "usage_boxes_without_a_value": BASE + ["--boxes"],
    "usage_rays_without_a_value": BASE + ["--rays"],
    "usage_observations_without_a_value": BASE + ["--observations"],
    "usage_obs_depth_range_without_a_value": BASE + ["--obs-depth-range"],
    "usage_znear_without_a_value": BASE + ["--znear"],
    "usage_outputs_without_a_value": BASE + ["--outputs"],
    "usage_unknown_outputs": BASE + ["--outputs", "rgba"],
    "usage_no_worlds": ["0", "1", "rast", "64", "64"],
    "usage_worlds_not_a_number": ["many", "1", "rast", "64", "64"],
    "usage_no_width": ["4", "1", "rast", "0", "64"],
    "usage_no_height": ["4", "1", "rast", "64", "0"],
    "usage_no_gpus": BASE + ["--gpus", "0"],
    "usage_more_gpus_than_worlds": BASE + ["--gpus", "5"],
    # --vfov, --znear
    "vfov_not_a_number": BASE + ["--vfov", "wide"],
    "vfov_empty": BASE + ["--vfov", ""],
    "vfov_trailing_characters": BASE + ["--vfov", "60deg"],
    "vfov_infinite": BASE + ["--vfov", "inf"],
    "vfov_zero": BASE + ["--vfov", "0"],
    "vfov_180": BASE + ["--vfov", "180"],
    "vfov_negative": BASE + ["--vfov", "-60"],
    "znear_not_a_number": BASE + ["--znear", "near"],
    "znear_nan": BASE + ["--znear", "nan"],
    "znear_zero": BASE + ["--znear", "0"],
    "znear_negative": BASE + ["--znear", "-0.1"],
    "znear_at_the_raytracer_far_plane": RT + ["--znear", "1000"],
    "znear_beyond_the_raytracer_far_plane": RT + ["--znear", "2500"],
    # --light
    "light_not_a_number": BASE + ["--light", "1,x,0"],
    "light_empty_field": BASE + ["--light", "1,,0"],
    "light_empty": BASE + ["--light", ""],
    "light_two_fields": BASE + ["--light", "1,0"],
    "light_four_fields": BASE + ["--light", "1,0,0,0.5"],
    "light_six_fields": BASE + ["--light", "1,0,0,0.5,0.5,1"],
    "light_sixth_field_not_a_number": BASE + ["--light", "1,0,0,0.5,0.5,x"],
    "light_zero_direction": BASE + ["--light", "0,0,0"],
    "light_negative_ambient": BASE + ["--light", "1,0,0,-0.5,0.5"],
    "light_negative_diffuse": BASE + ["--light", "1,0,0,0.5,-0.5"],
    # the seeds
    "colors_seed_not_a_number": BASE + ["--instance-colors", "red"],
    "colors_seed_empty": BASE + ["--instance-colors", ""],
    "colors_seed_negative": BASE + ["--instance-colors", "-1"],
    "colors_seed_signed": BASE + ["--instance-colors", "+1"],
    "colors_seed_trailing_characters": BASE + ["--instance-colors", "12x"],
    "colors_seed_beyond_64_bits": BASE + ["--instance-colors", "18446744073709551616"],
    "materials_seed_not_a_number": BASE + ["--instance-materials", "steel"],
    "materials_seed_empty": BASE + ["--instance-materials", ""],
    "materials_seed_negative": BASE + ["--instance-materials", "-1"],
    "materials_seed_signed": BASE + ["--instance-materials", "+1"],
    "materials_seed_trailing_characters": BASE + ["--instance-materials", "0x1g"],
    "materials_seed_beyond_64_bits": BASE + ["--instance-materials", "0x10000000000000000"],
    "labels_seed_not_a_number": BASE + ["--instance-labels", "cube"],
    "labels_seed_empty": BASE + ["--instance-labels", ""],
    "labels_seed_negative": BASE + ["--instance-labels", "-7"],
    "labels_seed_signed": BASE + ["--instance-labels", "+7"],
    "labels_seed_trailing_characters": BASE + ["--instance-labels", "7 "],
    "labels_seed_beyond_64_bits": BASE + ["--instance-labels", "99999999999999999999"],
    # the bounded counts
    "supersample_zero": BASE + ["--supersample", "0"],
    "supersample_five": BASE + ["--supersample", "5"],
    "supersample_negative": BASE + ["--supersample", "-2"],
    "supersample_signed": BASE + ["--supersample", "+2"],
    "supersample_empty": BASE + ["--supersample", ""],
    "supersample_hexadecimal": BASE + ["--supersample", "0x2"],
    "supersample_trailing_characters": BASE + ["--supersample", "2x"],
    "supersample_beyond_64_bits": BASE + ["--supersample", "18446744073709551618"],
    "supersample_too_many_pixels": ["4", "1", "rast", "8192", "64", "--supersample", "3"],
    "supersample_too_many_rows": ["4", "1", "rast", "64", "4097", "--supersample", "4"],
    "boxes_zero": BASE + ["--instance-labels", "1", "--boxes", "0"],
    "boxes_too_many": BASE + ["--instance-labels", "1", "--boxes", "1025"],
    "boxes_negative": BASE + ["--boxes", "-4"],
    "boxes_signed": BASE + ["--boxes", "+4"],
    "boxes_empty": BASE + ["--boxes", ""],
    "boxes_not_a_number": BASE + ["--boxes", "four"],
    "boxes_beyond_64_bits": BASE + ["--boxes", "18446744073709551620"],
    "boxes_rast_without_labels": BASE + ["--boxes", "4"],
    "rays_zero": BASE + ["--rays", "0"],
    "rays_too_many": BASE + ["--rays", "65537"],
    "rays_negative": BASE + ["--rays", "-8"],
    "rays_signed": BASE + ["--rays", "+8"],
    "rays_empty": BASE + ["--rays", ""],
    "rays_a_fraction": BASE + ["--rays", "8.5"],
    "rays_beyond_64_bits": BASE + ["--rays", "18446744073709551624"],
    # --positions, --depth, --flow against --outputs
    "positions_unknown_frame": BASE + ["--positions", "screen"],
    "positions_without_depth": BASE + ["--positions", "--outputs", "rgb"],
    "positions_view_without_depth": BASE + ["--outputs", "rgb", "--positions", "view"],
    "depth_dump_without_depth": BASE + ["--depth", "--outputs", "rgb"],
    "flow_without_depth": BASE + ["--flow", "--outputs", "rgb"],
    "flow_with_boxes": RT + ["--flow", "--boxes", "4"],
    "flow_with_labels": BASE + ["--flow", "--instance-labels", "3"],
    # --observations, --obs-depth-range
    "observations_unknown_channels": BASE + ["--observations", "rgba"],
    "observations_empty": BASE + ["--observations", ""],
    "observations_unknown_dtype": BASE + ["--observations", "rgb,float64"],
    "observations_empty_dtype": BASE + ["--observations", "rgb,,2"],
    "observations_stack_zero": BASE + ["--observations", "rgb,float16,0"],
    "observations_stack_nine": BASE + ["--observations", "rgb,float16,9"],
    "observations_stack_a_word": BASE + ["--observations", "rgb,float16,two"],
    "observations_stack_two_digits": BASE + ["--observations", "rgb,float16,12"],
    "observations_four_fields": BASE + ["--observations", "rgb,float16,2,1"],
    "observations_rgb_without_rgb": BASE + ["--observations", "rgb", "--outputs", "depth"],
    "observations_yd_without_rgb": BASE + ["--observations", "yd", "--outputs", "depth"],
    "observations_d_without_depth": BASE + ["--observations", "d", "--outputs", "rgb"],
    "observations_yd_without_depth": BASE + ["--outputs", "rgb", "--observations", "yd,uint8"],
    "obs_depth_range_one_field": BASE + ["--observations", "rgbd", "--obs-depth-range", "5"],
    "obs_depth_range_three_fields": BASE + ["--observations", "rgbd", "--obs-depth-range", "0,1,2"],
    "obs_depth_range_not_numbers": BASE + ["--observations", "rgbd", "--obs-depth-range", "a,b"],
    "obs_depth_range_second_not_a_number": BASE + ["--observations", "rgbd", "--obs-depth-range", "0,b"],
    "obs_depth_range_infinite": BASE + ["--observations", "rgbd", "--obs-depth-range", "0,inf"],
    "obs_depth_range_reversed": BASE + ["--observations", "rgbd", "--obs-depth-range", "5,1"],
    "obs_depth_range_empty": BASE + ["--observations", "rgbd", "--obs-depth-range", "1,1"],
    "obs_depth_range_negative": BASE + ["--observations", "rgbd", "--obs-depth-range", "-1,1"],
    "obs_depth_range_without_depth_channels": BASE + ["--observations", "rgb", "--obs-depth-range", "0.1,20"],
    "obs_depth_range_without_observations": BASE + ["--obs-depth-range", "0.1,20"],
    # which of two refusals comes first: the options in the order they are given, then the checks after the loop
    "order_light_number_before_field_count": BASE + ["--light", "1,x"],
    "order_light_field_count_before_the_library": BASE + ["--light", "0,0"],
    "order_options_in_the_order_given": BASE + ["--rays", "0", "--boxes", "0"],
    "order_options_in_the_order_given_reversed": BASE + ["--boxes", "0", "--rays", "0"],
    "order_option_before_usage": BASE + ["--rays", "0", "--frobnicate"],
    "order_usage_before_option": BASE + ["--frobnicate", "--rays", "0"],
    "order_option_before_the_checks_after_the_loop": BASE + ["--outputs", "rgb", "--depth", "--vfov", "0"],
    "order_usage_before_supersample_size": ["0", "1", "rast", "8192", "64", "--supersample", "3"],
    "order_supersample_size_before_znear": ["4", "1", "rt", "8192", "64", "--supersample", "3", "--znear", "1000"],
    "order_znear_before_depth_dump": RT + ["--znear", "1000", "--depth", "--outputs", "rgb"],
    "order_depth_dump_before_positions": BASE + ["--positions", "--depth", "--outputs", "rgb"],
    "order_positions_before_flow": BASE + ["--flow", "--positions", "--outputs", "rgb"],
    "order_flow_depth_before_flow_boxes": RT + ["--flow", "--boxes", "4", "--outputs", "rgb"],
    "order_flow_boxes_before_boxes_rast": BASE + ["--flow", "--boxes", "4"],
    "order_boxes_rast_before_observations": BASE + ["--boxes", "4", "--observations", "rgb", "--outputs", "depth"],
    "order_observations_rgb_before_range": BASE + ["--observations", "rgb", "--outputs", "depth", "--obs-depth-range", "0.1,20"],
    "order_observations_depth_before_range": BASE + ["--observations", "d", "--outputs", "rgb", "--obs-depth-range", "0.1,20"],
}


def _run(native, argv, cwd):
    from madrona_renderer_amd import build
    return subprocess.run(["renderer_headless"] + argv, executable=build.headless_path(), cwd=cwd, capture_output=True,
                          text=True, timeout=60)


@pytest.mark.parametrize("name", list(CASES))
def test_headless_refuses_with_the_recorded_text_and_status(native, tmp_path, name):
    want = json.load(open(GOLDEN))[name]
    p = _run(native, CASES[name], tmp_path)
    assert p.returncode == want["status"] == 1
    assert p.stderr == want["stderr"]
    assert p.stdout == "" and not list(tmp_path.iterdir())


def test_the_file_holds_these_cases_and_no_others():
    golden = json.load(open(GOLDEN))
    assert sorted(golden) == sorted(CASES)
    assert all(g["stderr"].endswith("\n") and g["stderr"].count("\n") == 1 for g in golden.values())
    # the two kinds of refusal: the usage line, which names the program, and a line that starts with the option
    usage = {n for n, g in golden.items() if g["stderr"].startswith("renderer_headless [NUM_WORLDS]")}
    assert usage == {n for n in CASES if n.startswith(("usage_", "order_usage_"))}
    assert all(golden[n]["stderr"].startswith("--") for n in CASES if n not in usage)


if __name__ == "__main__":
    if "--record" not in sys.argv:
        sys.exit("usage: python -m tests.test_headless_refusals_cpu --record")
    import tempfile
    recorded = {}
    with tempfile.TemporaryDirectory() as tmp:
        for case, args in CASES.items():
            done = _run(None, args, tmp)
            recorded[case] = {"stderr": done.stderr, "status": done.returncode}
    with open(GOLDEN, "w") as f:
        json.dump(recorded, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", GOLDEN, len(recorded))
