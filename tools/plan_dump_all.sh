#!/bin/bash
# tools/plan_dump_all.sh <plan_dump binary> — runs plan_dump (tools/plan_dump.cpp) over every golden scene and the downscaled benchmark
# stand-ins (tools/make_scenes.py bench_small, regenerated into a temporary directory), one process per scene: once with no switch set,
# and the scenes with object instances again under the tree builder's switches.  Prints plan_dump's lines, each section under a header;
# two builds of the planning code agree when their outputs are equal (profiles/plan_unit_trees_parent_vs_change.txt).  Host only.
# tools/plan_dump_all.sh <plan_dump binary> tables — the table builder's check instead: plan_dump --tables over every golden scene, every
# fuzz scene and the stand-ins, no switch set, each line followed by that run's stderr (indented).  Two builds of scene_build.cpp agree when
# these outputs are equal (profiles/scene_build_tables_parent_vs_change.txt).  WF_BUILD_THREADS defaults to 3 and JOBS (scenes at a time) to 1:
# more threads than cores make scenes run past the limit.  A scene without a line is a failed check: the exit status is 1 when a run was
# killed (the limit, a signal, an abort: exit status 124 or more); a scene file that is refused with an error message (an include file) is not.
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
unset WF_BRAID WF_BRAID_MIN_FRAC WF_TIGHT_INSTANCES WF_LEAF_COLLAPSE WF_BRAID_VERBOSE WF_NO_FAST WF_ANIM_FAST WF_DEFER_GENERAL WF_LEAN_SHADE WF_LEAN_PER_TYPE WF_MEDIUM_LEAN WF_VISIBLE_SURFACE WF_RARE_LIGHTS
SCENES=$(ls "$ROOT"/tests/golden/*.pbrt "$TMP"/*/*.pbrt)
run() {   # run <scene>: one line; a scene file that is no scene of its own (an include) or a crash still gives a line
  local out
  out=$( cd "$(dirname "$1")" && timeout 900 "$BIN" --datadir "$ROOT/pbrt-v4_amd/data" "$(basename "$1")" 2>"$TMP/err" )
  local rc=$?
  if [ -n "$out" ]; then echo "$out"; else echo "$(basename "$1"): no line (exit $rc): $(grep -v '^Warning' "$TMP/err" | head -1)"; fi
  grep -E "runtime error|AddressSanitizer" -A6 "$TMP/err" | head -20
}
if [ "${2:-}" = tables ]; then
  export WF_BUILD_THREADS=${WF_BUILD_THREADS:-3}
  one() {   # one <scene>: its line (or why there is none), then its stderr
    local d; d=$(mktemp -d -p "$TMP")
    ( cd "$(dirname "$1")" && timeout 900 "$BIN" --datadir "$ROOT/pbrt-v4_amd/data" --tables "$(basename "$1")" >"$d/out" 2>"$d/err" )
    local rc=$?
    if [ -s "$d/out" ]; then cat "$d/out"; else echo "$(basename "$1"): no line (exit $rc)"; fi
    sed 's/^/    | /' "$d/err"
    [ $rc -lt 124 ] || echo "$1" >> "$TMP/killed"
  }
  export -f one; export BIN ROOT TMP
  echo "== tables"
  ls "$ROOT"/tests/golden/*.pbrt "$ROOT"/tests/golden/fuzz/*.pbrt "$TMP"/*/*.pbrt | xargs -P "${JOBS:-1}" -I{} bash -c 'one "{}" > "$TMP/$(echo "{}" | tr / _).res"'
  for s in $(ls "$ROOT"/tests/golden/*.pbrt "$ROOT"/tests/golden/fuzz/*.pbrt "$TMP"/*/*.pbrt); do cat "$TMP/$(echo "$s" | tr / _).res"; done
  [ ! -s "$TMP/killed" ] || { echo "no line, killed: $(tr '\n' ' ' < "$TMP/killed")" >&2; exit 1; }
  exit 0
fi
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
