"""The group kernel's ready-made work items (16 slots, one-tile views): the plain entry
(MRX_GROUP_FAST=0) and the FAST entry both take them.  Each renders the headline scene,
a textured 64x64 scene and a ragged-edge scene; each must match the CPU oracle and the
other path byte for byte, depth included."""
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
        got = fetch(r, visibility=visibility)
        del r
        assert_parity(got, ref)
        outs[fast] = got
    for key in outs["0"]:
        assert np.array_equal(outs["0"][key].view(np.uint8), outs["1"][key].view(np.uint8)), key
