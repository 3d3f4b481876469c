"""bench.py's argument checks and the size of its --dump-outputs files: no GPU needed (parse() runs
before torch or the renderer is imported)."""
import os
import subprocess
import sys

from tests.conftest import ROOT

BENCH = os.path.join(ROOT, "bench.py")


def _run(args):
    e = dict(os.environ)
    e.pop("RANK", None)
    return subprocess.run([sys.executable, BENCH] + args, capture_output=True, text=True, timeout=300,
                          cwd=ROOT, env=e)


def test_steps_below_one_is_refused():
    p = _run(["--steps", "0"])
    assert p.returncode == 2 and "--steps must be at least 1" in p.stderr


def test_a_view_too_large_to_dump_is_refused_before_anything_runs(tmp_path):
    out = tmp_path / "dump"
    p = _run(["--dump-outputs", str(out), "--width", "2048", "--height", "2048"])
    assert p.returncode == 2 and "does not fit" in p.stderr
    assert not out.exists()


def test_dump_budget_per_view():
    import bench
    a = bench.parse(["--dump-outputs", "d"])
    assert bench.ids_output(a) is None
    assert bench.dump_bytes_per_view(a) == 64 * 64 * (16 + 4)
    # the headline's 4096 views are sampled down to what fits, with room for the .npy headers and the index
    n = bench.DUMP_BYTES // bench.dump_bytes_per_view(a)
    assert 0 < n < 4096 and bench.DUMP_BYTES + 8 * n + 4 * 4096 <= 64 * 10 ** 6
    rt = bench.parse(["--dump-outputs", "d", "--mode", "Raytracer", "--width", "256", "--height", "64"])
    assert bench.ids_output(rt) == "segmask"
    assert bench.dump_bytes_per_view(rt) == 256 * 256 * (16 + 4 + 8)      # Raytracer views are square
