#!/bin/bash
# the last GPU call of a round: smoke, the whole GPU suite, the contract bench line -- on the final tree
# usage (from the repo root): bash scripts/gpu_final_check.sh OUTDIR
OUT=${1:?usage: bash scripts/gpu_final_check.sh OUTDIR}
mkdir -p "$OUT"
python -c "import __graft_entry__ as g; g.smoke()" > "$OUT/smoke.log" 2>&1; echo "smoke rc=$?"; tail -4 "$OUT/smoke.log" | cut -c1-300
python -m pytest tests/ -q -m gpu --durations=8 > "$OUT/suite.log" 2>&1; echo "suite rc=$?"
tail -14 "$OUT/suite.log" | cut -c1-200
python bench.py --full > "$OUT/bench.json" 2> "$OUT/bench.err"; echo "bench rc=$?"
python - "$OUT/bench.json" <<'P'
import json, sys
o=json.load(open(sys.argv[1]))
print({k:o[k] for k in ('value','ms_per_step','ms_per_step_events_off','gpu_active_s')}, o['sustained']['ms_per_step'])
print(o['roofline']['frac'], o['roofline']['traffic_source'][:60])
print(o['secondary']['ms_per_step'], o['inference']['generate']['refine']['host_refine_ms'], o['inference']['generate']['refine']['end_to_end_grids_per_s'])
P
