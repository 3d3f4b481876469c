"""renderer_headless --outputs rgbd|depth|rgb (-m gpu): the last-frame dump writes the output that
exists -- rgb as the oracle's image, depth-only as a grey tile of 1/depth (nearest hit of the frame
white, background black)."""
import numpy as np
import pytest

from madrona_renderer_amd import scenes
from tests.test_headless_gpu import _run, _tiles
from tests.util import render_oracle

pytestmark = pytest.mark.gpu


def test_outputs_argument_errors(native, tmp_path):
    r = _run([4, 2, "rast", 64, 64, "--outputs", "colour"], tmp_path)
    assert r.returncode != 0 and "--outputs rgbd|depth|rgb" in r.stderr
    r = _run([4, 2, "rast", 64, 64, "--outputs", "rgb", "--depth", "--dump-last-frame", "f"], tmp_path)
    assert r.returncode != 0 and "not rendered" in r.stderr


@pytest.mark.parametrize("mode", ["rast", "rt"])
def test_rgb_only_dump_matches_oracle(native, tmp_path, mode):
    r = _run([5, 2, mode, 64, 64, "--dump-last-frame", "frame", "--scene", "demo", "--outputs", "rgb"], tmp_path)
    assert r.returncode == 0, r.stderr
    ref = render_oracle(scenes.demo_scene(num_worlds=5, render_mode="Rasterizer"))
    for i, tile in enumerate(_tiles(tmp_path / "frame.png", 5, 64, 64)):
        assert np.array_equal(tile, ref["rgb"][i])


@pytest.mark.parametrize("mode", ["rast", "rt"])
def test_depth_only_dump_is_inverse_depth(native, tmp_path, mode):
    r = _run([5, 2, mode, 64, 64, "--dump-last-frame", "frame", "--scene", "synthetic", "--outputs", "depth"],
             tmp_path)
    assert r.returncode == 0, r.stderr
    desc = scenes.synthetic_scene(5, render_mode="Raytracer" if mode == "rt" else "Rasterizer")
    d = render_oracle(desc, want_ids=False)["depth"]
    if mode == "rt":
        d = d.transpose(0, 2, 1)          # the dump un-transposes Raytracer storage
    dmin = d[d > 0].min()
    inv = np.where(d > 0, np.float32(255.0) * np.minimum(dmin / np.where(d > 0, d, 1), np.float32(1.0)), 0)
    for i, tile in enumerate(_tiles(tmp_path / "frame.png", 5, 64, 64)):
        assert np.array_equal(tile[..., 0], tile[..., 1]) and np.array_equal(tile[..., 0], tile[..., 2])
        assert (tile[..., 3] == 255).all()
        # depth is within 1e-4 of the oracle's, so a grey level may land one step off
        assert np.abs(tile[..., 0].astype(int) - inv[i].astype(np.uint8).astype(int)).max() <= 1
        assert (tile[..., 0][d[i] == 0] == 0).all()          # background black
