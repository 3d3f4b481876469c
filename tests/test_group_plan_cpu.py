"""The raster group kernel's launch plan on the host (no GPU), through mrx_group_plan: the shapes of
the BASELINE batches and of the small, tiled, textured and large-world ones, worked out by hand from the launcher's rules;
the overrides; what keeps a launch off the FAST entry; XMODE; the packed header words against the layout written at
GroupHeader (raster.hpp), packed here in Python; the refusals.  Everything here decides speed only -- every shape renders
the same pixels -- so no parity test would notice a slip."""
import ctypes

import pytest

MRX_E_INVALID = -1
FAST, GROUP = 1, 2          # MRX_ENTRY_GROUP_FAST, MRX_ENTRY_GROUP


class PlanIn(ctypes.Structure):
    _fields_ = [("views", ctypes.c_uint32), ("nfast", ctypes.c_uint32), ("nslow", ctypes.c_uint32),
                ("max_world_triangles", ctypes.c_uint32), ("textured", ctypes.c_int32), ("num_cus", ctypes.c_uint32),
                ("uni_instances", ctypes.c_uint32), ("uni_cams_per_world", ctypes.c_uint32),
                ("uni_prefix", ctypes.c_uint32 * 5), ("uni_first_tri", ctypes.c_uint32 * 4),
                ("has_blocks", ctypes.c_int32), ("diagnostics", ctypes.c_int32),
                ("group_views", ctypes.c_int32), ("group_tiles", ctypes.c_int32), ("xcd_skew", ctypes.c_int32),
                ("xcd_rotate", ctypes.c_int32), ("debug_slots", ctypes.c_int32), ("fast_allowed", ctypes.c_int32),
                ("xcd_phase", ctypes.c_uint32), ("has_report", ctypes.c_int32)]


class PlanOut(ctypes.Structure):
    _fields_ = [("slots", ctypes.c_int32), ("group_views", ctypes.c_uint32), ("chunk_tiles", ctypes.c_uint32),
                ("groups_per_view", ctypes.c_uint32), ("workgroups", ctypes.c_uint32), ("threads", ctypes.c_uint32),
                ("xcd_skew", ctypes.c_uint32), ("xcd_rotate", ctypes.c_uint32), ("xmode", ctypes.c_int32),
                ("fast", ctypes.c_int32), ("shape", ctypes.c_uint32), ("prefix", ctypes.c_uint32),
                ("first01", ctypes.c_uint32), ("first23", ctypes.c_uint32)]


@pytest.fixture(scope="module")
def capi(native):
    lib = ctypes.CDLL(native.load_capi()._name)        # a handle of this module's own: its prototypes stay here
    lib.mrx_group_plan.restype = ctypes.c_int
    lib.mrx_group_plan.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    return lib


# tiles per view -> a view of that many 64x64 tiles (the last one not a whole number of tiles: the count rounds up)
PIXELS = {1: (64, 64), 2: (128, 64), 4: (128, 128), 16: (250, 256)}


def world(tris):
    """a cube and a plane of `tris` triangles together, the plane's two last: (instances, cameras, prefix, first)"""
    return 2, 1, [0, tris - 2, tris, tris, tris], [0, tris - 2, 0, 0]


def plan(capi, views=4096, tiles=1, tris=14, tex=0, cus=256, uni=None, want=None, **kw):
    inst, cams, prefix, first = uni if uni is not None else world(tris)
    q = PlanIn(views=views, nfast=PIXELS[tiles][0], nslow=PIXELS[tiles][1], max_world_triangles=tris, textured=tex,
               num_cus=cus, uni_instances=inst, uni_cams_per_world=cams, uni_prefix=(ctypes.c_uint32 * 5)(*prefix),
               uni_first_tri=(ctypes.c_uint32 * 4)(*first), has_blocks=1, diagnostics=0, group_views=0, group_tiles=0,
               xcd_skew=-1, xcd_rotate=-1, debug_slots=0, fast_allowed=1, xcd_phase=0, has_report=0)
    for k, v in kw.items():
        assert hasattr(q, k), k
        setattr(q, k, v)
    out = PlanOut()
    rc = capi.mrx_group_plan(ctypes.byref(q), ctypes.byref(out))
    if want is not None:
        assert rc == want, (rc, want)
    return rc, out


def shape_of(rc, o):
    return (o.slots, o.group_views, o.chunk_tiles, o.groups_per_view, o.workgroups, o.threads, o.xcd_skew, o.xcd_rotate, rc)


def pack(group_views, skew, rotate, inst, cams, prefix, first):
    """the layout written at GroupHeader (raster.hpp), by hand:
    shape   grpViews | xcdSkew << 8 | xcdRotate << 12 | uniInstances << 13 | uniCamsPerWorld << 16 | valid << 31
    prefix  uniPrefix[1..4], eight bits each;  first01, first23  uniFirstTri[0..3], sixteen bits each"""
    return (group_views | skew << 8 | rotate << 12 | inst << 13 | cams << 16 | 1 << 31,
            prefix[1] | prefix[2] << 8 | prefix[3] << 16 | prefix[4] << 24,
            first[0] | first[1] << 16, first[2] | first[3] << 16)


#        views  tiles tris tex cus   slots vg ct gpv workgroups threads skew rotate entry
TABLE = [(4096,  1,  14, 0, 256,     16, 4, 1, 1,  1024, 512, 3, 1, FAST),
         (16384, 1,  14, 0, 256,     16, 4, 1, 1,  4096, 512, 3, 1, FAST),
         (4092,  1,  14, 0, 256,     16, 2, 1, 1,  2046, 512, 1, 1, FAST),
         (2048,  1,  14, 0, 256,     16, 2, 1, 1,  1024, 512, 1, 1, FAST),
         (1024,  1,  14, 0, 256,     16, 2, 1, 1,   512, 512, 0, 0, FAST),
         (1022,  1,  14, 0, 256,     16, 1, 1, 1,  1022, 512, 0, 0, FAST),
         (256,   1,  14, 0, 256,     16, 1, 1, 1,   256, 512, 0, 0, FAST),
         (16384, 1,  14, 1, 256,     16, 2, 1, 1,  8192, 256, 1, 1, FAST),
         (4096,  1, 100, 0, 256,    128, 1, 1, 1,  4096, 512, 0, 1, GROUP),
         (1024,  4,  14, 0, 256,     16, 1, 4, 1,  1024, 512, 0, 0, GROUP),
         (512,   4,  14, 0, 256,     16, 1, 2, 2,  1024, 512, 0, 0, GROUP),
         (64,   16,  14, 0, 256,     16, 1, 1, 16, 1024, 512, 0, 0, GROUP),
         (4096, 16,  14, 1, 256,     16, 1, 4, 4, 16384, 256, 0, 0, GROUP),
         (4096, 16, 200, 0, 256,    256, 1, 8, 2,  8192, 512, 0, 0, GROUP),
         (1024,  1,  14, 0, 64,      16, 4, 1, 1,   256, 512, 3, 1, FAST)]


@pytest.mark.parametrize("row", TABLE, ids=lambda r: "v%d_t%d_k%d_tex%d_cu%d" % r[:5])
def test_the_shapes_worked_out_by_hand(capi, row):
    views, tiles, tris, tex, cus = row[:5]
    rc, o = plan(capi, views, tiles, tris, tex, cus)
    assert shape_of(rc, o) == row[5:]
    assert o.fast == (1 if rc == FAST else 0)
    # the header words: packed here from the inputs for the FAST entry, untouched otherwise
    inst, cams, prefix, first = world(tris)
    words = (o.shape, o.prefix, o.first01, o.first23)
    assert words == (pack(o.group_views, o.xcd_skew, o.xcd_rotate, inst, cams, prefix, first) if rc == FAST else (0, 0, 0, 0))


def test_the_overrides(capi):
    base = shape_of(*plan(capi))
    assert base == (16, 4, 1, 1, 1024, 512, 3, 1, FAST)
    # three views per workgroup: no pairs of four or two to skew, the chip still full
    assert shape_of(*plan(capi, group_views=3)) == (16, 3, 1, 1, 1366, 512, 0, 1, FAST)
    assert plan(capi, xcd_skew=9)[1].xcd_skew == 7 and plan(capi, xcd_skew=0)[1].xcd_skew == 0
    assert plan(capi, xcd_rotate=0)[1].xcd_rotate == 0 and plan(capi, views=256, xcd_rotate=1)[1].xcd_rotate == 1
    # tiles wanted: one view per workgroup; slots wanted: a power of two from the world's own count up
    assert shape_of(*plan(capi, tiles=16, group_tiles=2)) == (16, 1, 2, 8, 32768, 512, 0, 0, GROUP)
    assert shape_of(*plan(capi, debug_slots=32)) == (32, 2, 1, 1, 2048, 512, 0, 1, GROUP)
    assert plan(capi, debug_slots=48)[1].slots == 16 and plan(capi, tris=17, debug_slots=16)[1].slots == 32
    # compute units 0: the 256 of the device the constants were measured on
    for views in (256, 1024, 2048, 4096):
        assert shape_of(*plan(capi, views, cus=0)) == shape_of(*plan(capi, views, cus=256))


def test_what_keeps_a_launch_off_the_fast_entry(capi):
    base = shape_of(*plan(capi, want=FAST))
    inst, cams, prefix, first = world(14)
    off = [dict(fast_allowed=0), dict(diagnostics=1), dict(diagnostics=2), dict(diagnostics=3), dict(diagnostics=4),
           dict(diagnostics=-1), dict(has_blocks=0),
           dict(uni=(0, 0, [0] * 5, [0] * 4)),
           # one past a field's width: cameras per world (8 bits), the last prefix (8), a first triangle (16)
           dict(uni=(inst, 256, prefix, first)), dict(uni=(2, 1, [0, 12, 256, 256, 256], first))]
    off += [dict(uni=(4, 1, [0, 3, 6, 9, 12], [65536 if i == j else 7 for j in range(4)])) for i in range(4)]
    for kw in off:
        rc, o = plan(capi, want=GROUP, **kw)
        assert (o.shape, o.prefix, o.first01, o.first23, o.fast) == (0, 0, 0, 0, 0), kw
        assert shape_of(rc, o)[:-1] == base[:-1], kw             # the same shape, the other entry
    # ... and the widths themselves fit
    full = (4, 255, [0, 85, 170, 255, 255], [65535, 65534, 65533, 65532])
    rc, o = plan(capi, tris=16, want=FAST, uni=full)
    assert (o.shape, o.prefix, o.first01, o.first23) == pack(4, 3, 1, *full)
    assert o.shape == 0x80FF9304 and o.prefix == 0xFFFFAA55 and o.first01 == 0xFFFEFFFF and o.first23 == 0xFFFCFFFD


def test_xmode(capi):
    for phase in (0, 1, 2, 3):
        for report in (0, 1):
            for views in (4096, 256):                # with and without a skew
                rc, o = plan(capi, views, xcd_phase=phase, has_report=report)
                assert o.slots == 16 and (o.xcd_skew != 0) == (views == 4096)
                assert o.xmode == (1 if o.xcd_skew and phase & 1 else 0) | (2 if report else 0)
            for tris in (17, 33, 65, 129):
                rc, o = plan(capi, tris=tris, xcd_phase=phase, has_report=report)
                assert o.slots == 2 * (tris - 1) and o.xmode == 0


def test_the_refusals(capi):
    out = PlanOut()
    q = PlanIn(views=4, nfast=64, nslow=64, max_world_triangles=14, xcd_skew=-1, xcd_rotate=-1)
    assert capi.mrx_group_plan(None, ctypes.byref(out)) == MRX_E_INVALID
    assert capi.mrx_group_plan(ctypes.byref(q), None) == MRX_E_INVALID
    assert capi.mrx_group_plan(ctypes.byref(q), ctypes.byref(out)) == GROUP
    plan(capi, tris=256, want=GROUP)
    for kw in (dict(tris=257), dict(uni=(5, 1, [0] * 5, [0] * 4)), dict(group_views=-1), dict(group_tiles=-1),
               dict(debug_slots=-1), dict(xcd_skew=-2), dict(xcd_rotate=-2)):
        plan(capi, want=MRX_E_INVALID, **kw)
    # no views, no pixels: nothing is launched
    for kw in (dict(views=0), dict(nfast=0), dict(nslow=0)):
        rc, o = plan(capi, want=0, **kw)
        assert (o.slots, o.workgroups, o.threads) == (0, 0, 0)
