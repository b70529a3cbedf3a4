#!/bin/bash
# HBM traffic of one eager denoising step by kernel class, from rocprofv3 PMC counters collected as
# /opt/skills/guides/MI355X_MICROARCH.md (section HBM) prescribes: FETCH_SIZE and WRITE_SIZE in SEPARATE passes
# (they do not fit one), no trace domains besides --kernel-trace, FETCH_SIZE doubled on gfx950.
# Run on a GPU machine from the repo root:  [OUT=dir] bash tools/pmc_traffic.sh   ->  $OUT/traffic.json (OUT: bench_out)
set -e
cd "${GRAFT_REPO_ROOT:?}"
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
export TMPDIR=/tmp
for c in FETCH_SIZE WRITE_SIZE; do
  rocprofv3 --kernel-trace --pmc $c --output-format csv -d "$OUT"/pmc_$c -- \
    python bench.py --full --steps 1 --warmup 1 --no-cpu-baseline --no-graph > "$OUT"/pmc_$c.log 2>&1
done
python tools/summarize_traffic.py "$OUT"/pmc_FETCH_SIZE "$OUT"/pmc_WRITE_SIZE "$OUT"/traffic.json
[ -n "$KEEP_RAW" ] || rm -rf "$OUT"/pmc_FETCH_SIZE "$OUT"/pmc_WRITE_SIZE
