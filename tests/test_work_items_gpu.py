"""The group kernel's ready-made work items (16 slots, one-tile views): the FAST entry takes them
(raster.hip: readyItems = FAST && !TEX); the plain entry (MRX_GROUP_FAST=0) keeps the per-tile masks.
Each renders the headline scene, a textured 64x64 scene (26 triangles a world: the plain entry either
way) and a ragged-edge scene; each must match the CPU oracle and the other entry byte for byte, depth
included, and Manager.raster_entry() names the entry that ran."""
import numpy as np
import pytest

from madrona_renderer_amd import scenes
from tests.util import assert_parity, fetch, make_product, render_oracle

pytestmark = pytest.mark.gpu

SCENES = {
    "headline": dict(num_worlds=4096),
    "textured64": dict(num_worlds=64, with_wall=True, textured=True),
    "ragged50x30": dict(num_worlds=6, width=50, height=30),
}
# the entry MRX_GROUP_FAST=1 reaches: cube + plane + wall is 26 triangles a world, 32 slots, never FAST
# (tests/test_uniform_worlds_gpu.py has the textured FAST instantiation)
FAST_ENTRY = {"headline": "group-fast", "textured64": "group", "ragged50x30": "group-fast"}


@pytest.mark.parametrize("visibility", [False, True])
@pytest.mark.parametrize("name", list(SCENES))
def test_plain_and_fast_entries_match_the_oracle(native, monkeypatch, name, visibility):
    desc = scenes.synthetic_scene(**SCENES[name])
    ref = render_oracle(desc)
    outs = {}
    for fast in ("0", "1"):
        monkeypatch.setenv("MRX_GROUP_FAST", fast)
        r = make_product(desc, visibility=visibility)
        r.step()
        assert r.raster_entry() == (FAST_ENTRY[name] if fast == "1" else "group")
        got = fetch(r, visibility=visibility)
        del r
        assert_parity(got, ref)
        outs[fast] = got
    for key in outs["0"]:
        assert np.array_equal(outs["0"][key].view(np.uint8), outs["1"][key].view(np.uint8)), key
