"""The FAST raster group kernel (raster.hip, rasterGroupKernelFast) on adversarial uniform worlds (-m gpu).

Every scene comes from tests/uniform_worlds.py and must reach the entry it targets (Manager.raster_entry).
On the FAST entry the ids / segmask and RGBA8 equal the oracle's, depth is within 1 ulp of it, and the
plain group entry (MRX_GROUP_FAST=0) stores the same bytes.  Covered: ids on and off in both render modes,
depth-only and RGB-only, forced group shapes and XCD splits (the items a workgroup leaves to the other
of its pair), a pose loop through the live tensors that puts cubes around the eye, the textured FAST
instantiation and both sides of every header limit."""
import numpy as np
import pytest
import torch

from madrona_renderer_amd import scenes
from oracle import oracle
from tests import uniform_worlds as uw
from tests.util import assert_parity, fetch, make_product, render_oracle

pytestmark = pytest.mark.gpu


def _same_bytes(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8)), k


def _render(desc, ids, entry, outputs=None):
    rt = desc.render_mode == "Raytracer"
    if outputs is None:
        r = make_product(desc, visibility=ids)
    else:
        import os
        old = os.environ.get("MADRONA_MI355_VISIBILITY")
        os.environ["MADRONA_MI355_VISIBILITY"] = "1" if ids else "0"
        try:
            r = scenes.make_renderer(desc, render_outputs=outputs)
        finally:
            if old is None:
                os.environ.pop("MADRONA_MI355_VISIBILITY", None)
            else:
                os.environ["MADRONA_MI355_VISIBILITY"] = old
    r.step()
    assert r.raster_entry() == entry
    if outputs is not None:
        return r
    out = fetch(r, visibility=ids, raytracer=rt)
    del r
    return out


def _check(monkeypatch, desc, ids, entry="group-fast", ref=None):
    """Render `desc`, assert the entry and parity with the oracle; on the FAST entry the plain group entry
    must store the same bytes."""
    ref = render_oracle(desc) if ref is None else ref
    got = _render(desc, ids, entry)
    assert_parity(got, ref)
    if entry == "group-fast":
        monkeypatch.setenv("MRX_GROUP_FAST", "0")
        _same_bytes(_render(desc, ids, "group"), got)
        monkeypatch.delenv("MRX_GROUP_FAST")
    return got


@pytest.mark.parametrize("ids", [False, True], ids=["no-ids", "ids"])
@pytest.mark.parametrize("name", sorted(uw.CASES))
def test_fast_entry_matches_the_oracle(native, monkeypatch, name, ids):
    _check(monkeypatch, uw.case(name), ids)


@pytest.mark.parametrize("outputs", ["Depth", "RGB"])
@pytest.mark.parametrize("name", ["raster-64x64-w1024", "raster-50x30-w130", "rt-64-w130", "tex-raster-64x64-w130"])
def test_selected_output_is_byte_identical_to_rgbd(native, name, outputs):
    desc = uw.case(name)
    rt = desc.render_mode == "Raytracer"
    full = _render(desc, True, "group-fast", outputs="RGBD")
    sel = _render(desc, True, "group-fast", outputs=outputs)
    full.sync()
    sel.sync()
    if outputs == "Depth":
        a, b = sel.depth_tensor().to_torch(), full.depth_tensor().to_torch()
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    else:
        assert torch.equal(sel.rgb_tensor().to_torch(), full.rgb_tensor().to_torch())
    assert torch.equal(sel.visibility_tensor().to_torch(), full.visibility_tensor().to_torch())
    # ... and that is the oracle's
    ref = render_oracle(desc)
    got = fetch(full, visibility=True, raytracer=rt)
    assert_parity(got, ref)


@pytest.mark.parametrize("name", ["raster-64x57-w7", "raster-50x30-w130"])
def test_forced_group_shapes_and_xcd_splits(native, monkeypatch, name):
    # MRX_XCD_SKEW moves strips of a view from the odd to the even workgroup of a pair: S2 leaves the moved
    # items to the other workgroup (itemPos 0xFF); MRX_XCD_PHASE 1 trades the places within the pair
    desc = uw.case(name)
    ref = render_oracle(desc)
    first = None
    shapes = [(1, 0, 0), (1, 0, 1)] + [(v, s, ph) for v in (2, 4) for s in range(8) for ph in (0, 1)]
    for views, skew, phase in shapes:
        monkeypatch.setenv("MRX_GROUP_VIEWS", str(views))
        monkeypatch.setenv("MRX_XCD_SKEW", str(skew))
        monkeypatch.setenv("MRX_XCD_PHASE", str(phase))
        got = _render(desc, True, "group-fast")
        if first is None:
            assert_parity(got, ref)
            first = got
        else:
            _same_bytes(got, first)


def test_pose_loop_puts_cubes_around_the_eye(native):
    # poses written through the live tensors on the render's stream, no host synchronisation before step();
    # the oracle renders the poses read back afterwards
    desc = uw.uniform_scene(101, 130, layout=("cube", "tie"), cams=2)
    r = make_product(desc, visibility=True)
    pos = r.instance_position_tensor().to_torch()
    rot = r.instance_rotation_tensor().to_torch()
    scl = r.instance_scale_tensor().to_torch()
    cpos = r.camera_position_tensor().to_torch()
    crot = r.camera_rotation_tensor().to_torch()
    g = torch.Generator().manual_seed(5)
    for step in range(4):
        # cube of every world: centred a little off its first camera's eye, a new rotation and scale signs
        off = (torch.rand(130, 3, generator=g) - 0.5) * (0.2 * (step + 1))
        pos[0::2] = cpos[0::2] + off.to(pos.device)
        q = torch.randn(130, 4, generator=g)
        q = q / q.norm(dim=1, keepdim=True)
        rot[0::2] = q.to(rot.device)
        sign = torch.where(torch.rand(130, 3, generator=g) < 0.4, -1.0, 1.0)
        scl[0::2] = (sign * (0.5 + torch.rand(130, 3, generator=g))).to(scl.device)
        # the soup follows the second camera
        pos[1::2] = cpos[1::2] + (torch.randn(130, 3, generator=g) * 0.3).to(pos.device)
        r.step()
        assert r.raster_entry() == "group-fast"
        got = fetch(r, visibility=True)
        P, Q, S = pos.cpu().numpy(), rot.cpu().numpy(), scl.cpu().numpy()
        desc.instances = [(tuple(map(float, P[i])), tuple(map(float, Q[i])), tuple(map(float, S[i])), o)
                          for i, (_, _, _, o) in enumerate(desc.instances)]
        desc.cameras = [(tuple(map(float, p)), tuple(map(float, q)))
                        for p, q in zip(cpos.cpu().numpy(), crot.cpu().numpy())]
        ref = render_oracle(desc)
        assert_parity(got, ref)
        # the eye sits inside a cube in a good share of the views
        assert uw.edge_counts(oracle.FlatScene(desc), ref)["inside_views"] >= 10


@pytest.mark.parametrize("mode", ["Rasterizer", "Raytracer"])
def test_header_limits(native, monkeypatch, mode):
    # the first triangle of a used object: 65535 fits the header's 16 bits, 65536 does not
    for first, entry in ((65535, "group-fast"), (65536, "group")):
        desc = uw.uniform_scene(5, 7, mode=mode, layout=("cube", "tie"), first_raw_tri=first)
        _check(monkeypatch, desc, True, entry)
    # cameras per world: 255 fit the header's 8 bits, 256 do not
    for cams, entry in ((255, "group-fast"), (256, "group")):
        desc = uw.uniform_scene(6, 1, width=16, height=16, mode=mode, layout=("cube", "tie"), cams=cams)
        _check(monkeypatch, desc, True, entry)
    # five instances per world: not uniform in the host's sense
    desc = uw.uniform_scene(7, 7, mode=mode, layout=("tie", "one", "one", "one", "one"))
    _check(monkeypatch, desc, True, "group")
