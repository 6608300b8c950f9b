#!/bin/bash
# rocprofv3 kernel-trace + stats of the bench run with its per-kernel taps (--full --quick); summaries land under
# $OUT/<tag>/ (default build/profiles; copy the *_kernel_stats.csv you want judged into profiles/).
# usage: bash scripts/profile_bench.sh <tag> [bench args]
set -e
TAG=${1:-prof}; shift || true
ROOT=${GRAFT_REPO_ROOT:-$(cd "$(dirname "$0")/.." && pwd)}
OUT=${OUT:-build/profiles}
cd /tmp && export TMPDIR=/tmp
cd "$ROOT"
mkdir -p "$OUT"
rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/$TAG" -- python3 bench.py --full --quick "$@" > "$OUT/$TAG.log" 2>&1
echo "rc=$?"
tail -1 "$OUT/$TAG.log"
F=$(find "$OUT/$TAG" -name "*kernel_stats.csv" | head -1)
echo "stats: $F"
head -25 "$F"
