"""Driver of tools/ub_stream_reread.hip: one process per (mode, buffer size, load policy), each under its own time limit, the first that fails ends the run.
    hipcc --offload-arch=gfx950 -O3 tools/ub_stream_reread.hip -o build/ub_stream_reread
    python tools/stream_reread.py [out.json = profiles/stream_reread_ceiling.json]
Per (mode, size, policy): microseconds per round, round 1 (the fill, behind a flush of the Infinity Cache) apart from rounds 2..R, and the event time
of all R rounds, for every launch.  Modes: "meet" = one launch per round (the rounds meet, as the solve's sweeps do at an exchange), "persistent" = R rounds
inside one launch (the wavefronts drift apart: its per-round figures describe the slowest wavefront, its total is the figure to read)."""
import json, os, statistics, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
exe = os.path.join(ROOT, "build", "ub_stream_reread")
out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "stream_reread_ceiling.json")
SIZES_MB, POLICIES, ROUNDS, LAUNCHES = (69, 138, 200, 240, 300), ("plain", "nt", "sc1"), 13, 5
res = dict(kernel="256 workgroups x 8 wavefronts, 2 KB chunks of eight 256-byte wave loads, 4 chunks in flight, widen + 4 fp64 FMAs per value",
           rounds=ROUNDS, launches_each=LAUNCHES, runs=[], summary=[])
for mode, mb, pol in [(m, s, p) for m in ("meet", "persistent") for s in SIZES_MB for p in POLICIES]:
    p = subprocess.run([exe, str(mb), pol, str(ROUNDS), str(LAUNCHES), mode], capture_output=True, text=True, timeout=60)
    if p.returncode != 0:
        sys.exit("ub_stream_reread %s %s %s: exit status %d\n%s" % (mb, pol, mode, p.returncode, p.stderr))
    r = json.loads(p.stdout.strip().splitlines()[-1])
    res["runs"].append(r)
    r1 = [l["round1_us"] for l in r["launches"]]
    r2 = [l["rounds2_median_us"] for l in r["launches"]]
    tot = [l["all_rounds_us"] for l in r["launches"]]
    row = dict(mode=mode, mb=mb, policy=pol, round1_us_median=statistics.median(r1), rounds2_us_median=statistics.median(r2), rounds2_us_min=min(r2),
               rounds2_us_max=max(r2), rounds2_tb_per_s=r["bytes"] / statistics.median(r2) / 1e6, all_rounds_us_median=statistics.median(tot),
               all_rounds_us_min=min(tot), all_rounds_us_max=max(tot))
    res["summary"].append(row)
    print(json.dumps(row), flush=True)
    json.dump(res, open(out, "w"), indent=1)
