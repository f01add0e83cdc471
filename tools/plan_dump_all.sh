#!/bin/bash
# tools/plan_dump_all.sh <plan_dump binary> — runs plan_dump (tools/plan_dump.cpp) over every golden scene and the downscaled benchmark
# stand-ins (tools/make_scenes.py bench_small, regenerated into a temporary directory), one process per scene: once with no switch set,
# and the scenes with object instances again under the tree builder's switches.  Prints plan_dump's lines, each section under a header;
# two builds of the planning code agree when their outputs are equal (profiles/plan_unit_trees_parent_vs_change.txt).  Host only.
set -u
BIN=$(realpath "$1")
ROOT=$(cd "$(dirname "$0")/.." && pwd)
TMP=$(mktemp -d)
trap 'rm -rf "$TMP"' EXIT
python3 -c "
import sys
sys.path.insert(0, '$ROOT/tools')
import make_scenes
for n in make_scenes.BENCH_SMALL: make_scenes.bench_small(n, '$TMP/' + n)
" > /dev/null || exit 1
unset WF_BRAID WF_BRAID_MIN_FRAC WF_TIGHT_INSTANCES WF_LEAF_COLLAPSE WF_BRAID_VERBOSE WF_NO_FAST WF_ANIM_FAST WF_DEFER_GENERAL WF_LEAN_SHADE WF_LEAN_PER_TYPE WF_MEDIUM_LEAN
SCENES=$(ls "$ROOT"/tests/golden/*.pbrt "$TMP"/*/*.pbrt)
run() {   # run <scene>: one line; a scene file that is no scene of its own (an include) or a crash still gives a line
  local out
  out=$( cd "$(dirname "$1")" && timeout 900 "$BIN" --datadir "$ROOT/pbrt-v4_amd/data" "$(basename "$1")" 2>"$TMP/err" )
  local rc=$?
  if [ -n "$out" ]; then echo "$out"; else echo "$(basename "$1"): no line (exit $rc): $(grep -v '^Warning' "$TMP/err" | head -1)"; fi
  grep -E "runtime error|AddressSanitizer" -A6 "$TMP/err" | head -20
}
echo "== default"
INST=""
for s in $SCENES; do
  line=$(run "$s")
  echo "$line"
  case "$line" in *" nInstances=0 "*) ;; *" nInstances="*) INST="$INST $s" ;; esac
done
for sw in "WF_BRAID=0" "WF_BRAID=8" "WF_BRAID=64 WF_BRAID_MIN_FRAC=0" "WF_TIGHT_INSTANCES=0 WF_BRAID=0" "WF_LEAF_COLLAPSE=4"; do
  echo "== $sw"
  for s in $INST; do ( export $sw; run "$s" ); done
done
