#!/bin/bash
# tools/sanitize_checker.sh — the CPU checker (oracle/wf_cpu: the per-item bodies the HIP kernels run, compiled for the host) built with
# AddressSanitizer + UndefinedBehaviorSanitizer and run over every golden and fuzz scene.  Round 5: three wrong-code
# incidents of the material kernels were put down to a toolchain defect; an out-of-bounds private-array index or an uninitialised read
# in the shared source would look the same.  This rules the shared source out on these inputs (device-only code — the LDS regroup,
# the queue allocation — is not covered).  About ten minutes on 8 cores.  Test infrastructure only.
# Second section: the library's host-only planning units (scene checks, PlanScene, the builder of the production traversal layout and
# its self-check) as the stand-alone program tools/plan_dump.cpp, built the same way and run over the golden scenes and the downscaled
# benchmark stand-ins under the builder's switches, then with --tables (every table of BuildSceneTables hashed) over the golden AND the fuzz
# scenes and the stand-ins (tools/plan_dump_all.sh).  Every unit of it is compiled by the clang that hipcc drives (two compilers' sanitizer
# runtimes do not mix).  About twenty minutes more.
# KNOWN FINDING, open: the --tables pass reports "wf_scene.h:478 runtime error: nan is outside the range of representable values of type
# 'int'" (MIPLevel, reached from the displacement evaluation of a plymesh) on fuzz/s6300046.pbrt, so this script ends non-zero until
# csrc/common/wf_scene.h is fixed.  The first section runs the same scene without a report: its compiler's -fsanitize=undefined does not
# include the float-to-integer conversion check (GCC enables -fsanitize=float-cast-overflow separately), clang's does.
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=${1:-/tmp/asan_build}
mkdir -p $OUT
make -C $ROOT/oracle OUT=$OUT CXXFLAGS="-std=c++17 -O1 -g -mfma -ffp-contract=off -pthread -I ../include -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer" $OUT/wf_cpu > /dev/null
cd $ROOT/tests/golden
export ASAN_OPTIONS=detect_leaks=0:abort_on_error=0 UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=0
n=0; bad=0
for f in *.pbrt fuzz/*.pbrt; do
  d=$(dirname $f)
  out=$( (cd $d && timeout 600 $OUT/wf_cpu --quiet --nthreads 2 --outfile /tmp/asan_out.pfm $(basename $f)) 2>&1 ) || true
  if echo "$out" | grep -qE "runtime error|AddressSanitizer"; then bad=$((bad+1)); echo "=== $f"; echo "$out" | grep -E "runtime error|AddressSanitizer|#[0-4] " | head -12; fi
  n=$((n+1))
done
echo "scenes $n, with sanitizer findings $bad"
SAN="-fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -g -O1"
CLANG=$(hipconfig -l)/clang++
make -C $ROOT/pbrt-v4_amd -j8 OUT=$OUT/plan CXX=$CLANG PLANCXX=$CLANG SAN="$SAN" $OUT/plan/plan_dump > /dev/null
$ROOT/tools/plan_dump_all.sh $OUT/plan/plan_dump > $OUT/plan_dump.txt 2>&1
$ROOT/tools/plan_dump_all.sh $OUT/plan/plan_dump tables >> $OUT/plan_dump.txt 2>&1 || true   # the table builder over the fuzz scenes too, hashing every table
pbad=$(grep -cE "runtime error|AddressSanitizer|no line \(exit 1[2-9][0-9]\)" $OUT/plan_dump.txt || true)   # (a run that was killed counts too)
grep -E "runtime error|AddressSanitizer" -B1 -A6 $OUT/plan_dump.txt | head -40
echo "plan_dump lines $(grep -vcE '^==|^    \|' $OUT/plan_dump.txt), sanitizer reports $pbad"
[ $bad -eq 0 ] && [ $pbad -eq 0 ]
