#!/usr/bin/env python3
"""Do two versions of the device sources compile to the same kernels?  Each is compiled to assembly with the product's
flags (build.py hip_command) plus --cuda-device-only -S, and every kernel's instruction stream is compared after
normalising what a source reorganisation may legitimately move: label numbers, the __hip_cuid symbol and the order
of the two source operands of commutative scalar instructions.  No GPU needed.

  python scripts/bvh_asm_diff.py HEAD~1 HEAD            # two revisions of madrona_renderer_amd/csrc/bvh.hip
  python scripts/bvh_asm_diff.py HEAD WORK              # WORK = the working tree
  python scripts/bvh_asm_diff.py a.s b.s                # two assembly files made that way
  python scripts/bvh_asm_diff.py --source rays.hip --source shadow.hip HEAD WORK      # names inside csrc/, or paths

A revision is compiled against its own headers: csrc/ and include/ of it are unpacked (git archive) into a temporary
directory, which also takes the assembly; nothing is written into the tree.  Prints one summary line per source with
the identical / different counts, and for every kernel that differs its code length, resource lines and mnemonic
counts on both sides.
"""
import collections
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from madrona_renderer_amd import build  # noqa: E402

COMMUTATIVE = re.compile(r"^(s_(?:and|or|xor|nand|nor|xnor)_b(?:32|64)|s_(?:add|mul)_(?:u32|i32)|s_(?:min|max)_[iu]32)\s+([^,]+),\s*([^,]+),\s*([^,]+)$")
RESOURCE = ("NumVgprs", "NumSgprs", "ScratchSize", "Occupancy", "codeLenInByte")


def device_flags():
    cmd = build.hip_command("/dev/null")
    return [a for a in cmd[1:cmd.index(os.path.join(build.CSRC, build.HIP_SOURCES[0]))] if a != "-shared"]


def tree(what, tmp):
    """The root of `what`'s sources: the working tree for WORK, else csrc/ and include/ of the revision, unpacked."""
    if what == "WORK":
        return ROOT
    root = os.path.join(tmp, re.sub(r"\W", "_", what))
    if not os.path.isdir(root):
        os.makedirs(root)
        tar = subprocess.check_output(["git", "-C", ROOT, "archive", what, "madrona_renderer_amd/csrc", "include"])
        subprocess.run(["tar", "-x", "-C", root], input=tar, check=True)
    return root


def assembly(what, source, tmp):
    """Path of the assembly of `source` in `what`: an .s file as it is, else compiled inside what's tree."""
    if what.endswith(".s"):
        return what
    out = os.path.join(tmp, "%s_%s.s" % (re.sub(r"\W", "_", what), re.sub(r"\W", "_", source)))
    src = os.path.join(tree(what, tmp), source)
    subprocess.check_call([build.hipcc()] + device_flags() + ["--cuda-device-only", "-S", "-x", "hip", src, "-o", out])
    return out


def kernels(path):
    """name -> (normalised instruction lines, resource lines) of every function of an assembly file"""
    out, name, body, labels = {}, None, [], {}
    for raw in open(path):
        line = raw.rstrip("\n")
        if name is None:
            m = re.match(r"^(_Z\w+|\w+):\s*(;.*)?$", line)
            if m and not line.startswith(".") and not line.startswith("__hip_cuid"):
                name, body, labels = m.group(1), [], {}
            continue
        if line.startswith(".Lfunc_end"):
            out[name] = [body, {}]
            last, name = name, None
            continue
        code = line.split(";")[0].strip()
        if not code or code.startswith(".") and not code.startswith(".LBB"):
            continue
        code = re.sub(r"__hip_cuid_\w+", "__hip_cuid", code)
        code = re.sub(r"\.LBB\d+_\d+", lambda m: labels.setdefault(m.group(0), ".L%d" % len(labels)), code)
        m = COMMUTATIVE.match(code)
        if m:
            a, b = sorted((m.group(3).strip(), m.group(4).strip()))
            code = "%s %s, %s, %s" % (m.group(1), m.group(2).strip(), a, b)
        body.append(code)
    # the resource comments follow each function: "; NumVgprs: 128" ... up to the next function
    cur = None
    for raw in open(path):
        m = re.match(r"^(_Z\w+|\w+):\s*(;.*)?$", raw)
        if m and m.group(1) in out:
            cur = m.group(1)
        m = re.match(r"^; (\w+)(?::| =) (\S+)", raw)
        if m and cur and m.group(1) in RESOURCE:
            out[cur][1].setdefault(m.group(1), m.group(2))
    return out


def demangle(name):
    s = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
    return s.replace("void mrx::(anonymous namespace)::", "").replace("(mrx::RasterParams)", "")


def main(argv):
    sources = []
    while argv[:1] == ["--source"]:
        sources.append(argv[1] if "/" in argv[1] else "madrona_renderer_amd/csrc/" + argv[1])
        argv = argv[2:]
    if len(argv) != 2:
        raise SystemExit(__doc__)
    with tempfile.TemporaryDirectory(prefix="asmdiff_") as tmp:
        for what in argv:
            if not what.endswith(".s"):
                tree(what, tmp)
        jobs = [(what, source) for source in sources or ["madrona_renderer_amd/csrc/bvh.hip"] for what in argv]
        with ThreadPoolExecutor(min(8, os.cpu_count() or 1)) as ex:
            parsed = list(ex.map(lambda j: kernels(assembly(j[0], j[1], tmp)), jobs))
    return max(compare(jobs[i][1], parsed[i], parsed[i + 1]) for i in range(0, len(jobs), 2))


def compare(source, a, b):
    same, differ = 0, []
    for name in sorted(set(a) | set(b)):
        if name in a and name in b and a[name][0] == b[name][0]:
            same += 1
            if a[name][1] != b[name][1]:
                print("resources differ though the instructions do not:", demangle(name), a[name][1], b[name][1])
        else:
            differ.append(name)
    print("%s: %d functions on the left, %d on the right: %d identical, %d different"
          % (os.path.basename(source), len(a), len(b), same, len(differ)))
    for name in differ:
        print("--", demangle(name))
        for side, k in (("left ", a.get(name)), ("right", b.get(name))):
            if k is None:
                print("   %s: absent" % side)
                continue
            print("   %s: %d instructions, %s" % (side, len(k[0]), " ".join("%s %s" % kv for kv in sorted(k[1].items()))))
        if name in a and name in b:
            ca = collections.Counter(l.split()[0] for l in a[name][0])
            cb = collections.Counter(l.split()[0] for l in b[name][0])
            delta = {m: cb[m] - ca[m] for m in set(ca) | set(cb) if ca[m] != cb[m]}
            print("   mnemonic counts, right - left:", " ".join("%s %+d" % kv for kv in sorted(delta.items())) or "none (order only)")
    return 1 if differ else 0


if __name__ == "__main__":
    raise SystemExit(main(sys.argv[1:]))
