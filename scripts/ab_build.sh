#!/bin/bash
# Build libmrx_hip.so variants for an A/B on the GPU box:
#   scripts/ab_build.sh <name> [extra hipcc flags]   ->  ab/libmrx_hip.so.<name>
# The sources and the flags are build.py's (HIP_SOURCES, hip_command): a variant is the product's library.
set -eu
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
NAME="$1"; shift
mkdir -p "$ROOT/ab"
cd "$ROOT"
exec python3 - "$ROOT/ab/libmrx_hip.so.$NAME" "$@" <<'PY'
import subprocess, sys
from madrona_renderer_amd import build
subprocess.check_call(build.hip_command(sys.argv[1], sys.argv[2:]))
PY
