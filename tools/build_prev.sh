#!/bin/bash
# Build tools/ab/liblmm_hip_prev.so from the library sources of a git revision (default HEAD), for same-box A/B runs (tools/ab_lib.sh,
# LMM_HIP_LIB).  The revision's own build recipe compiles it: every file under csrc/ and include/ as that revision has them, with the
# per-source flags of its __graft_entry__.SOURCES.
REV=${1:-HEAD}
set -e
ROOT=$(git rev-parse --show-toplevel)
T=$(mktemp -d)
trap 'rm -rf "$T"' EXIT
git -C "$ROOT" archive "$REV" __graft_entry__.py lmm_amd.py linearmixingmodels.jl_amd include | tar -x -C "$T"
(cd "$T" && python -c "import __graft_entry__ as e; e.build(force=True)")
mkdir -p "$ROOT/tools/ab"
cp "$T/linearmixingmodels.jl_amd/liblmm_hip.so" "$ROOT/tools/ab/liblmm_hip_prev.so"
echo "built prev from $REV"
