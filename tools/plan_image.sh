#!/bin/bash
# Plan images of two source trees, compared: the host plan compiler of commit PARENT against the one in the
# working tree.  CPU only; needs g++, gcov and the Python package importable (for the case writer).
#
#     tools/plan_image.sh [PARENT_REV [WORK_DIR]]        (default: HEAD^, a fresh temporary directory)
#
# Steps (1, 2 and 4 must pass; 3 and 5 report):
#   1. the case directory (tools/plan_image_cases.py)
#   2. tools/plan_image.cpp built against both trees (-O3 -ffp-contract=off), both run, outputs diffed:
#      zero differing lines; in each run every witness differs from its baseline and the interleaved
#      second pass equals the first
#   3. which attempts of the retry ladder the case list reached (a --coverage build of the new tree, gcov)
#   4. the new tree under ASan + UBSan over the whole list, and under TSan over the block cases
#   5. host compile time: nine alternating runs per tree of the three timing workloads; the new tree's
#      median against the parent's own min-to-max range
set -euo pipefail
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
REV="${1:-HEAD^}"
WORK="${2:-$(mktemp -d)}"
mkdir -p "$WORK/parent"
echo "work directory: $WORK"

git -C "$ROOT" archive "$REV" waveforms_amd/csrc include | tar -x -C "$WORK/parent"
OLD_DEF=""
grep -q wfk_internal_keep_mixed_short "$WORK/parent/waveforms_amd/csrc/wfk_internal.h" && OLD_DEF="-DPLAN_IMAGE_OLD_SWITCHES"
NEW_DEF=""
grep -q wfk_internal_keep_mixed_short "$ROOT/waveforms_amd/csrc/wfk_internal.h" && NEW_DEF="-DPLAN_IMAGE_OLD_SWITCHES"

build() {   # build OUT TREE DEF FLAGS...
  local out="$1" tree="$2" def="$3"; shift 3
  g++ -std=c++17 -ffp-contract=off -pthread "$@" $def -I"$tree/include" -I"$tree/waveforms_amd/csrc" \
      "$ROOT/tools/plan_image.cpp" "$tree/waveforms_amd/csrc/wfk_compile.cpp" -o "$out"
}

echo "== 1. cases"
python3 "$ROOT/tools/plan_image_cases.py" "$WORK/cases"

echo "== 2. images: $REV against the working tree"
build "$WORK/image_parent" "$WORK/parent" "$OLD_DEF" -O3
build "$WORK/image_new" "$ROOT" "$NEW_DEF" -O3
"$WORK/image_parent" "$WORK/cases" > "$WORK/parent.txt" 2> "$WORK/parent.err" || { cat "$WORK/parent.err"; echo "parent run FAILED"; exit 1; }
"$WORK/image_new" "$WORK/cases" > "$WORK/new.txt" 2> "$WORK/new.err" || { cat "$WORK/new.err"; echo "new run FAILED"; exit 1; }
cat "$WORK/new.err"
if ! diff "$WORK/parent.txt" "$WORK/new.txt" > "$WORK/images.diff"; then
  head -40 "$WORK/images.diff"
  echo "plan images DIFFER in $(grep -c '^>' "$WORK/images.diff") of $(wc -l < "$WORK/new.txt") cases"
  exit 1
fi
echo "plan images: 0 differing lines over $(wc -l < "$WORK/new.txt") cases"

echo "== 3. ladder attempts reached (executions per attempt of compile_ladder; ##### = never)"
mkdir -p "$WORK/cov"
(cd "$WORK/cov" && build "$WORK/cov/image_cov" "$ROOT" "$NEW_DEF" -O0 --coverage && ./image_cov "$WORK/cases" --no-interleave > /dev/null 2>&1 &&
 gcov -o . image_cov-wfk_compile.gcda > /dev/null 2>&1 || gcov -o . wfk_compile.cpp > /dev/null 2>&1)
grep -E '= attempt\((H|S),' "$WORK/cov/wfk_compile.cpp.gcov" | sed -E 's/^ *([0-9#=-]+)[*]?: *([0-9]+):/\1 x  line \2:/'

echo "== 4. sanitizers (new tree)"
SAN="-O1 -g -fno-omit-frame-pointer"
build "$WORK/image_asan" "$ROOT" "$NEW_DEF" $SAN -fsanitize=address,undefined -fno-sanitize-recover=undefined
ASAN_OPTIONS=detect_leaks=1 UBSAN_OPTIONS=print_stacktrace=1 "$WORK/image_asan" "$WORK/cases" > "$WORK/asan.txt" 2> "$WORK/asan.err" || { tail -40 "$WORK/asan.err"; echo "ASan+UBSan run FAILED"; exit 1; }
diff -q "$WORK/new.txt" "$WORK/asan.txt" > /dev/null && echo "ASan+UBSan: clean over the whole list, images equal the -O3 build's" || echo "ASan+UBSan: clean (images differ from the -O3 build's: optimisation level)"
build "$WORK/image_tsan" "$ROOT" "$NEW_DEF" $SAN -fsanitize=thread
"$WORK/image_tsan" "$WORK/cases" --only blocks. > "$WORK/tsan.txt" 2> "$WORK/tsan.err" || { tail -40 "$WORK/tsan.err"; echo "TSan run FAILED"; exit 1; }
if grep -q 'WARNING: ThreadSanitizer' "$WORK/tsan.err"; then tail -40 "$WORK/tsan.err"; echo "TSan reports"; exit 1; fi
echo "TSan: clean over $(wc -l < "$WORK/tsan.txt") block cases"

echo "== 5. host compile time (ms; nine alternating runs per tree, each the median of 5 compiles)"
: > "$WORK/time_parent.txt"; : > "$WORK/time_new.txt"
for run in 1 2 3 4 5 6 7 8 9; do
  "$WORK/image_parent" "$WORK/cases" --time 5 >> "$WORK/time_parent.txt"
  "$WORK/image_new" "$WORK/cases" --time 5 >> "$WORK/time_new.txt"
done
python3 - "$WORK/time_parent.txt" "$WORK/time_new.txt" <<'EOF'
import statistics, sys
def load(path):
    runs = {}
    for line in open(path):
        f = line.split()
        runs.setdefault(f[1], []).append(float(f[5]))      # time NAME min A median B max C ...
    return runs
parent, new = load(sys.argv[1]), load(sys.argv[2])
for name in parent:
    lo, hi, med = min(parent[name]), max(parent[name]), statistics.median(new[name])
    print('%-24s parent %8.3f .. %8.3f (median %8.3f)   new median %8.3f   %s' % (
        name, lo, hi, statistics.median(parent[name]), med, 'inside' if lo <= med <= hi else 'OUTSIDE the parent range'))
EOF
echo "all steps passed"
