#!/bin/bash
# Per-stage times per frame vs frames per launch: a stage whose per-frame time
# falls as the batch grows is latency-bound at the smaller batch.
# Usage (on the box): bash tools/sweep_frames.sh "2 4 8 16" [OUTDIR]
set -o pipefail
cd $GRAFT_REPO_ROOT
O=${2:-out}/frames
mkdir -p $O
for f in $1; do
  timeout -k 10 200 python bench.py --full --no-cpu-baseline --steps 10 --frames $f > $O/f$f.json 2> $O/f$f.err || { echo "bench $f failed"; tail -5 $O/f$f.err; exit 1; }
  python -c "import json; d=json.load(open('$O/f$f.json')); print('frames=$f', d['value'], d['ms_per_step'], {k: round(v/$f, 4) for k, v in d['stages_ms_per_step'].items()})"
done
