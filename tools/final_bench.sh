#!/bin/bash
# The full bench line of a round (bench.py --full) and the rocprofv3 per-kernel table of the same command.
#   usage: tools/final_bench.sh <tag> [OUTDIR]   -> OUTDIR/<tag>.json, OUTDIR/<tag>_kernel_stats.csv   (copy both to profiles/)
tag=${1:-r03_bench_v1}
cd "$(dirname "$0")/.." || exit 1
out=${2:-build/final_bench}
mkdir -p "$out"
export TMPDIR=${TMPDIR:-/tmp}
python3 __graft_entry__.py > "$out/fb_build.log" 2>&1 || { echo "build failed"; tail -5 "$out/fb_build.log"; exit 1; }
python3 -u bench.py --full > "$out/$tag.json" 2> "$out/$tag.err" || exit 1
rocprofv3 --kernel-trace --stats --output-format csv -d "$out/${tag}_prof" -- python3 bench.py --full --skip-cpu > "$out/${tag}_rocprof.json" 2> "$out/${tag}_rocprof.err" || exit 1
f=$(find "$out/${tag}_prof" -name "*kernel_stats.csv" | head -1); cp "$f" "$out/${tag}_kernel_stats.csv"
rm -rf "$out/${tag}_prof"
head -c 600 "$out/$tag.json"; echo; head -5 "$out/${tag}_kernel_stats.csv"
