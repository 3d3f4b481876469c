"""In-tree build of the native pieces (no cmake needed):

  libmrx_hip.so         C-ABI + HIP kernels for gfx950      (hipcc)
  libmadrona_mi355.so   madRender::Manager C++ API          (g++)
  madrona_renderer.*.so Python module, reference API        (g++ / pybind11)

Everything lands next to this file so the built objects travel with the
source tree (they are git-ignored, not gpurun-ignored).
"""
import os
import shutil
import subprocess
import sys
import sysconfig

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
ARCH = "gfx950"

HIP_SOURCES = ["raster.hip", "bvh.hip", "resolve.hip", "unproject.hip", "boxes.hip", "observe.hip", "rays.hip", "rays_host.cpp", "flow.hip", "flow_host.cpp", "cloud.hip", "cloud_host.cpp", "shadow.hip", "shadow_host.cpp", "bvh.cpp", "mrx_api.cpp", "scene.cpp", "stages.cpp", "shards.cpp", "host_tools.cpp", "assets.cpp", "ktx2.cpp"]
HIP_DEPS = HIP_SOURCES + ["raster.hpp", "raster_dev.hpp", "bvh.hpp", "resolve.hpp", "unproject.hpp", "boxes.hpp", "observe.hpp", "rays.hpp", "rays_core.hpp", "flow.hpp", "flow_core.hpp", "cloud.hpp", "cloud_core.hpp", "shadow.hpp", "shadow_core.hpp", "stage_core.hpp", "assets.hpp", "bc7_tables.inc",
                          "renderer.hpp", "shards.hpp", "error.hpp",
                          "../../include/mrx.h"]
MGR_SOURCES = ["manager.cpp"]
MGR_DEPS = MGR_SOURCES + ["../../include/madrona_mi355/manager.hpp",
                          "../../include/madrona_mi355/types.hpp", "../../include/mrx.h"]
PY_SOURCES = ["py_module.cpp", "manager.cpp"]


def ext_suffix():
    return sysconfig.get_config_var("EXT_SUFFIX") or ".so"


def lib_path():
    return os.path.join(HERE, "libmrx_hip.so")


def mgr_path():
    return os.path.join(HERE, "libmadrona_mi355.so")


def module_path():
    return os.path.join(HERE, "madrona_renderer" + ext_suffix())


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(os.path.join(CSRC, d)) > t for d in deps)


def _run(cmd, verbose):
    if verbose:
        print("+", " ".join(cmd), flush=True)
    subprocess.check_call(cmd)


def hipcc():
    exe = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(exe):
        raise RuntimeError("hipcc not found: the HIP library cannot be built")
    return exe


def hip_command(out, extra_flags=()):
    """The hipcc line of libmrx_hip.so, written to `out` (scripts/ab_build.sh builds its variants with it)."""
    cmd = [hipcc(), "--offload-arch=" + ARCH, "-O3", "-std=c++17", "-fPIC",
           "-shared", "-ffp-contract=off", "-fno-fast-math",
           # per-pixel state lives in small unrolled arrays; LLVM's AMDGPU
           # promote-alloca pass turns them into 16-wide vector registers
           # whose every conditional update copies the whole tuple
           "-mllvm", "-disable-promote-alloca-to-vector",
           # the SLP vectorizer packs scalar f32 math into v_pk_* pairs and
           # pays for it in v_mov shuffles and ~40 extra VGPRs (no rate gain
           # on gfx950: packed f32 issues at the scalar-f32 rate)
           "-fno-slp-vectorize",
           # the command processor writes the first 12 dwords of a kernel's arguments into SGPRs at wave
           # launch: the group kernel's argument header (raster.hpp GroupHeader)
           "-mllvm", "-amdgpu-kernarg-preload-count=12",
           "-Wall", "-Wno-unused-function"]
    cmd += list(extra_flags)
    # e.g. MRX_EXTRA_HIPCC_FLAGS=-DMRX_BVH_DIAG=1 python -m madrona_renderer_amd.build --force
    # (the BVH kernel's in-kernel stamps and phase switches: scripts/bvh_stamps.py, bvh_ablate.py)
    cmd += os.environ.get("MRX_EXTRA_HIPCC_FLAGS", "").split()
    cmd += [os.path.join(CSRC, s) for s in HIP_SOURCES]
    cmd += ["-lz", "-ldl", "-Wl,-rpath,/opt/rocm/lib", "-o", out]
    return cmd


def build_hip(force=False, verbose=False, extra_flags=()):
    out = lib_path()
    if force or _stale(out, HIP_DEPS):
        _run(hip_command(out, extra_flags), verbose)
    return out


def build_manager(force=False, verbose=False):
    out = mgr_path()
    if force or _stale(out, MGR_DEPS) or \
            os.path.getmtime(out) < os.path.getmtime(lib_path()):
        cmd = ["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall"]
        cmd += [os.path.join(CSRC, s) for s in MGR_SOURCES]
        cmd += ["-L" + HERE, "-lmrx_hip", "-Wl,-rpath,$ORIGIN", "-o", out]
        _run(cmd, verbose)
    return out


def build_module(force=False, verbose=False):
    import pybind11
    out = module_path()
    if force or _stale(out, PY_SOURCES + MGR_DEPS + ["obs_names.hpp"]) or \
            os.path.getmtime(out) < os.path.getmtime(lib_path()):
        cmd = ["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall",
               "-fvisibility=hidden",
               "-I" + pybind11.get_include(),
               "-I" + sysconfig.get_paths()["include"]]
        cmd += [os.path.join(CSRC, s) for s in PY_SOURCES]
        cmd += ["-L" + HERE, "-lmrx_hip", "-Wl,-rpath,$ORIGIN", "-o", out]
        _run(cmd, verbose)
    return out


def headless_path():
    return os.path.join(HERE, "renderer_headless")


def build_headless(force=False, verbose=False):
    """The reference's headless CLI (src/headless.cpp) over the MI355X Manager."""
    out = headless_path()
    deps = ["headless.cpp", "assets.cpp", "assets.hpp", "obs_names.hpp"] + MGR_DEPS
    if force or _stale(out, deps) or os.path.getmtime(out) < os.path.getmtime(lib_path()):
        cmd = ["g++", "-O2", "-std=c++17", "-Wall",
               "-DMRX_DATA_DIR=\"%s\"" % os.path.join(ROOT, "data"),
               os.path.join(CSRC, "headless.cpp"), os.path.join(CSRC, "manager.cpp"),
               os.path.join(CSRC, "assets.cpp"), os.path.join(CSRC, "ktx2.cpp"),
               "-L" + HERE, "-lmrx_hip", "-lz", "-ldl", "-lpthread", "-Wl,-rpath,$ORIGIN", "-o", out]
        _run(cmd, verbose)
    return out


# The sanitizer builds of host code, each with its stand-alone driver csrc/<name>.cpp: host compiler only (the HIP
# runtime header bvh.hpp pulls in is declarations), run by the CPU tests as stand-alone programs -- never on the GPU box.
# name -> (sources behind the driver, headers, flags, libraries)
_ASAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
         "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include"]
_STRICT = ["-ffp-contract=off"] + _ASAN             # the stages' arithmetic: one rounding per operation
_ASSETS = ["bvh.cpp", "assets.cpp", "ktx2.cpp"]
_ASSET_DEPS = ["assets.hpp", "bvh.hpp", "raster.hpp", "bc7_tables.inc"]
_STAGE_DEPS = ["stage_core.hpp", "bvh.hpp", "raster.hpp", "host_driver.hpp", "../../include/mrx.h"]
DRIVERS = {
    # the host code that reads untrusted input: OBJ / MTL / PNG / KTX2 / BC7 readers, BLAS builder (test_sanitizers.py)
    "host_asan_driver": (["assets.cpp", "ktx2.cpp", "bvh.cpp"], _ASSET_DEPS + ["host_driver.hpp"], _ASAN, ["-lz", "-ldl"]),
    # the ray-cast sensor's host entry: rays_core.hpp on the CPU, over the BLAS builder (test_ray_cpu.py)
    "rays_host_driver": (["rays_host.cpp"] + _ASSETS, ["rays.hpp", "rays_core.hpp"] + _STAGE_DEPS + _ASSET_DEPS,
                         _STRICT, ["-lz", "-ldl"]),
    # the optical-flow output's host entry: flow_core.hpp on the CPU (test_flow_cpu.py)
    "flow_host_driver": (["flow_host.cpp"], ["flow.hpp", "flow_core.hpp"] + _STAGE_DEPS, _STRICT, []),
    # the point-cloud output's host entry: cloud_core.hpp on the CPU (test_cloud_cpu.py)
    "cloud_host_driver": (["cloud_host.cpp"], ["cloud.hpp", "cloud_core.hpp"] + _STAGE_DEPS, _STRICT, []),
    # the shadow stage's host entry: shadow_core.hpp on the CPU, over the host scene of rays_host.cpp and the BLAS
    # builder (test_shadow_cpu.py)
    "shadow_host_driver": (["shadow_host.cpp", "rays_host.cpp"] + _ASSETS,
                           ["shadow.hpp", "shadow_core.hpp", "cloud_core.hpp", "rays.hpp", "rays_core.hpp"] +
                           _STAGE_DEPS + _ASSET_DEPS, _STRICT, ["-lz", "-ldl"]),
    # ThreadSanitizer: the shard-worker protocol (shards.cpp: no HIP in it); the driver's stub callback stands in for
    # the renderer (test_sanitizers.py)
    "shards_tsan_driver": (["shards.cpp"], ["shards.hpp", "error.hpp", "../../include/mrx.h"],
                           ["-fsanitize=thread", "-fno-omit-frame-pointer"], ["-lpthread"]),
}


def driver_path(name):
    return os.path.join(ROOT, "build", name)


def build_driver(name, force=False, verbose=False):
    srcs, deps, flags, libs = DRIVERS[name]
    srcs = [name + ".cpp"] + srcs
    out = driver_path(name)
    if force or _stale(out, srcs + deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        _run(["g++", "-O1", "-g", "-std=c++17", "-Wall"] + flags + [os.path.join(CSRC, s) for s in srcs] + libs +
             ["-o", out], verbose)
    return out


# the names the tests and the scripts use
def build_asan(force=False, verbose=False): return build_driver("host_asan_driver", force, verbose)
def build_rays_driver(force=False, verbose=False): return build_driver("rays_host_driver", force, verbose)
def build_flow_driver(force=False, verbose=False): return build_driver("flow_host_driver", force, verbose)
def build_cloud_driver(force=False, verbose=False): return build_driver("cloud_host_driver", force, verbose)
def build_shadow_driver(force=False, verbose=False): return build_driver("shadow_host_driver", force, verbose)
def build_shards_driver(force=False, verbose=False): return build_driver("shards_tsan_driver", force, verbose)
def asan_driver_path(): return driver_path("host_asan_driver")
def rays_driver_path(): return driver_path("rays_host_driver")
def flow_driver_path(): return driver_path("flow_host_driver")
def cloud_driver_path(): return driver_path("cloud_host_driver")
def shadow_driver_path(): return driver_path("shadow_host_driver")
def shards_driver_path(): return driver_path("shards_tsan_driver")


def build_all(force=False, verbose=False):
    build_hip(force, verbose)
    build_manager(force, verbose)
    build_module(force, verbose)
    build_headless(force, verbose)
    return lib_path(), mgr_path(), module_path()


if __name__ == "__main__":
    force = "--force" in sys.argv
    flags = {"--asan": build_asan, "--rays-driver": build_rays_driver, "--flow-driver": build_flow_driver,
             "--cloud-driver": build_cloud_driver, "--shadow-driver": build_shadow_driver,
             "--shards-driver": build_shards_driver}
    chosen = [fn for flag, fn in flags.items() if flag in sys.argv]
    if chosen:
        print(chosen[0](force=force, verbose=True))
    else:
        print("\n".join(build_all(force=force, verbose=True)))
