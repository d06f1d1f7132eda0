#!/bin/bash
# A/B of two builds of the library on the same box, same session: tools/ab_bench.sh <workload> <steps> <out.json> [extra bench args]
# (the third argument is the output file, the workload defaults to C4: the flagship -- earlier versions took the bench arguments there and defaulted to C5)
# A = firstordersolvers.jl_amd/csrc/libfoship_ab.so (the comparison build: the parent commit's), B = libfoship.so (the tree's).
# A_TREE=<dir>: arm A is a whole checkout of the comparison commit, built there -- its own bench.py, package and library (for a change that adds an entry
# to the C ABI: the tree's package does not load the parent's library).  C_ENV="NAME=value ...": a third arm "new_off", the tree's library under those
# environment settings (a switch that restores the parent's path must sit within the parent's spread).
# REPS (default 5) runs each of plain `python bench.py`, alternating the arms, every run under its own time limit (RUN_LIMIT seconds, default 240);
# the first run that fails or runs out of time ends the sequence.  Medians and min-max spreads of ms_per_step and of
# roofline.us_per_cg_iteration go to <out.json>.
set -o pipefail
W=${1:-C4}; K=${2:-200}; OUT=${3:-ab_bench.json}; shift; shift; shift
REPS=${REPS:-5}; RUN_LIMIT=${RUN_LIMIT:-240}
LINES=$(mktemp)
trap 'rm -f "$LINES" "$LINES.one"' EXIT
ARMS="parent new"; [ -n "$C_ENV" ] && ARMS="parent new new_off"
for rep in $(seq 1 "$REPS"); do
  for arm in $ARMS; do
    case $arm in
      parent) if [ -n "$A_TREE" ]; then dir=$A_TREE; set_env=""; else dir=$PWD; set_env="FOSHIP_LIB=$PWD/firstordersolvers.jl_amd/csrc/libfoship_ab.so"; fi ;;
      new) dir=$PWD; set_env="FOSHIP_LIB=$PWD/firstordersolvers.jl_amd/csrc/libfoship.so" ;;
      new_off) dir=$PWD; set_env="FOSHIP_LIB=$PWD/firstordersolvers.jl_amd/csrc/libfoship.so $C_ENV" ;;
    esac
    (cd "$dir" && env $set_env timeout -k 10 "$RUN_LIMIT" python bench.py --workload "$W" --steps "$K" "$@" 2>/dev/null) | tail -n 1 > "$LINES.one"
    rc=$?
    if [ $rc -ne 0 ]; then echo "ab_bench: $arm, repetition $rep: exit status $rc -- stopping" >&2; rm -f "$LINES" "$LINES.one"; exit $rc; fi
    python - "$arm" "$LINES.one" >> "$LINES" <<'EOF' || { echo "ab_bench: no result line -- stopping" >&2; exit 1; }
import json, sys
d = json.loads(open(sys.argv[2]).read().strip())
r = d['roofline_kkt'] if isinstance(d.get('roofline_kkt'), dict) else d['roofline']
us = next((x['us_per_cg_iteration'] for x in (d.get('roofline'), d.get('roofline_kkt')) if isinstance(x, dict) and x.get('us_per_cg_iteration') is not None), None)
row = dict(lib=sys.argv[1], ms_per_step=d['ms_per_step'], us_per_cg_iteration=us, sweep_ms=r.get('avg_kernel_ms'),
           cg_iters_per_step=d['config']['cg_iters_per_step'], setup_s=d['config'].get('setup_s'))
print(json.dumps(row))
sys.stderr.write(json.dumps(row) + "\n")
EOF
  done
done
python - "$LINES" "$OUT" "$W" "$K" <<'EOF'
import json, statistics, sys
rows = [json.loads(l) for l in open(sys.argv[1]) if l.strip()]
out = dict(workload=sys.argv[3], steps=int(sys.argv[4]), runs=rows)
for key in ("parent", "new", "new_off"):
    mine = [r for r in rows if r["lib"] == key]
    if not mine:
        continue
    ms = [r["ms_per_step"] for r in mine]
    us = [r["us_per_cg_iteration"] for r in mine if r["us_per_cg_iteration"] is not None]
    out[key] = dict(median_ms_per_step=statistics.median(ms), min_ms_per_step=min(ms), max_ms_per_step=max(ms), spread_ms_per_step=max(ms) - min(ms),
                    median_us_per_cg_iteration=statistics.median(us) if us else None, cg_iters_per_step=sorted(set(r["cg_iters_per_step"] for r in mine)),
                    median_setup_s=statistics.median([r["setup_s"] for r in mine]) if all(r.get("setup_s") is not None for r in mine) else None)
gain = out["parent"]["median_ms_per_step"] - out["new"]["median_ms_per_step"]
out["gain_ms_per_step"] = gain
out["gain_clears_parent_spread"] = bool(gain > out["parent"]["spread_ms_per_step"])
out["gain_clears_three_spreads"] = bool(gain > 3 * max(out["parent"]["spread_ms_per_step"], out["new"]["spread_ms_per_step"]))
if "new_off" in out:
    off = out["new_off"]["median_ms_per_step"]
    out["new_off_within_parent_spread"] = bool(out["parent"]["min_ms_per_step"] <= off <= out["parent"]["max_ms_per_step"])
json.dump(out, open(sys.argv[2], "w"), indent=1)
print(json.dumps({k: out[k] for k in out if k != "runs"}))
EOF
rm -f "$LINES" "$LINES.one"
