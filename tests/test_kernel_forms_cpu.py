"""How many instantiations of each kernel template the launchers' dispatch makes.  The dispatch
turns run-time values into template arguments with generic helpers (raster.hpp withBool / withValue), so a slip there
instantiates more kernels (build time, code size) or fewer (a launch of something else) without a compile error.  The
counts are read off the committed resource table, which tests/test_kernel_resources.py pins to what HEAD compiles to."""
import os
import re
from collections import Counter

from tests.conftest import ROOT

FORMS = ["Uniform", "PV", "PVL", "C", "PVLC", "M", "PVLM", "N", "NPV", "L", "LN", "PVM"]


def _counts():
    """{source: Counter of (kernel template, form name or None)} and the legend of the table's header"""
    per_source, legend, src = {}, None, None
    for line in open(os.path.join(ROOT, "profiles", "kernel_resources_latest.txt")):
        if line.startswith("##"):
            if "(mrx::KernelForm)N" in line:
                legend = line.split("row:", 1)[1].strip()
            continue
        if line.startswith("# "):
            src = os.path.basename(line[2:].strip())
            per_source[src] = Counter()
            continue
        m = re.match(r"(\w+)<(?:\(mrx::KernelForm\)(\d+),)?", line)
        assert m, line
        per_source[src][(m.group(1), FORMS[int(m.group(2))] if m.group(2) else None)] += 1
    return per_source, legend


def test_the_table_names_the_forms_as_this_test_does():
    _, legend = _counts()
    assert legend == ", ".join("%d %s" % (i, n) for i, n in enumerate(FORMS))


def test_instantiations_per_kernel_template_and_form():
    per_source, _ = _counts()
    group = {("rasterGroupKernel", None): 96,        # ids x textured x output x (16 slots: XMODE 0..3; 32 .. 256 slots)
             ("rasterGroupKernelFast", None): 48,    # ids x textured x output x XMODE
             ("rasterBruteKernel", None): 12, ("rasterChunkedKernel", None): 2}
    for form in ("PV", "PVL", "C", "PVLC", "M", "PVLM", "N", "NPV"):
        group[("rasterGroupFormKernel", form)] = 20          # ids x textured x five slot counts
        group[("rasterGroupFormKernelFast", form)] = 4       # ids x textured
    for form in ("L", "LN"):                                 # with ids only
        group[("rasterGroupFormKernel", form)] = 10
        group[("rasterGroupFormKernelFast", form)] = 2
    for form in ("PV", "N", "NPV"):
        group[("rasterBruteFormKernel", form)] = 4
        group[("rasterChunkedFormKernel", form)] = 2
    assert dict(per_source["raster.hip"]) == group
    assert sum(group.values()) == 392

    bvh = {("bvhTileKernel", None): 36,                      # ids (3) x textured x six tile shapes
           ("bvhTileFormKernel", "PV"): 36, ("bvhTileFormKernel", "PVM"): 36, ("bvhTileFormKernel", "N"): 36,
           ("bvhTileFormKernel", "NPV"): 30,                 # textured: no classifying instantiation
           ("bvhFlatKernel", None): 18,                      # ids (3) x textured x output
           ("bvhFlatFormKernel", "PV"): 6, ("bvhFlatFormKernel", "N"): 6, ("bvhFlatFormKernel", "NPV"): 6}
    assert dict(per_source["bvh.hip"]) == bvh
    assert sum(bvh.values()) == 210
