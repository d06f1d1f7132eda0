"""Host overhead of the sparse sets of the Feasibility form, one library per process (the other build through FOSHIP_LIB), for a parent / new / parent protocol:
the quantities of tools/sparse_affine_bench.py, tools/sparse_factored_bench.py and tools/nspace_cg_bench.py at reduced shapes and the set-up time of each one's
largest instance -> one JSON line.

    FOSHIP_LIB=<parent>/libfoship.so python tools/sparse_intake_speed.py > s1_parent1.json ;  python tools/sparse_intake_speed.py > s1_new.json ;  ... parent2, session 2
    python tools/sparse_intake_speed.py --merge <dir with speed_s{1,2}_{parent1,new,parent2}.json> profiles/sparse_intake_refactor_bench.json
"""
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests")); sys.path.insert(0, str(ROOT / "tools"))


def measure_all():
    import __graft_entry__ as ge
    import nspace_cg_bench as ncb
    import sparse_factored_cases as sfc
    from test_gpu_sparse_affine import sparse_instance
    pkg = ge.load_package()
    out = {"counts": {}, "times": {}, "setup_s": {}}

    def timed(fn):
        t0 = time.perf_counter()
        r = fn()
        return r, time.perf_counter() - t0

    # ---- tools/sparse_affine_bench.py's measurements, its two small sizes; the set-up of m = 200 000, n = 10^6
    for (m, n, per_row) in [(2000, 8000, 8), (40000, 120000, 5)]:
        A, b = sparse_instance(1, m, n, per_row)
        d, ts = timed(lambda: pkg.HipFeasibility(pkg.Feasibility(pkg.IndAffine(A, b), pkg.IndBox(0.0, np.inf), n)))
        x = np.random.default_rng(0).standard_normal(n)
        d.prox(1, x)
        cold = []
        for _ in range(7):
            d.set_iterate(None)
            t = time.perf_counter(); d.prox(1, x); cold.append(1e6 * (time.perf_counter() - t))
        c = d.affine_stats(1)
        d.set_alg(pkg.DR()); d.set_iterate(x)
        d.step(1, 50, 10 ** 9, 0.0)
        s0 = d.affine_stats(1)
        per = []
        for k in range(5):
            t = time.perf_counter(); d.step(51 + 40 * k, 40, 10 ** 9, 0.0); d.get_iterate(); per.append(1e6 * (time.perf_counter() - t) / 40)
        s1 = d.affine_stats(1)
        key = "sparse_affine %dx%d" % (m, n)
        out["counts"][key] = {"cold_cg_iterations": c["last_cg_iterations"], "cold_restarts": c["last_restarts"], "dr_cg_iterations": s1["cg_iterations"] - s0["cg_iterations"],
                              "lanes_per_row": list(s1["lanes_per_row"]), "nnz": s1["nnz"]}
        out["times"][key + " cold_projection_us"] = statistics.median(cold)
        out["times"][key + " dr_iteration_us"] = statistics.median(per)
        out["setup_s"][key] = ts
        d.close()
    A, b = sparse_instance(1, 200000, 1000000, 10)
    d, ts = timed(lambda: pkg.HipFeasibility(pkg.Feasibility(pkg.IndAffine(A, b), pkg.IndBox(0.0, np.inf), 1000000)))
    out["setup_s"]["sparse_affine 200000x1000000"] = ts
    d.close()

    # ---- tools/sparse_factored_bench.py's one-step protocol, two small cases; the set-up of rand_10000x1000000x10
    for name, (A, b) in {"rand_2000x8000x8": sfc.rand(2000, 8000, 8), "hann4_band_2000": sfc.band(2000, sfc.HANN4)}.items():
        m, n = A.shape
        free = lambda: pkg.IndBox(-np.inf, np.inf)
        x0 = np.random.default_rng(0).standard_normal(n)
        hs = {}
        for k, S in {"factored": pkg.IndAffine(A, b, form="sparse_factored"), "factored_refine1": pkg.IndAffine(A, b, form="sparse_factored", refine=1),
                     "sparse_cg": pkg.IndAffine(A, b), "empty": free()}.items():
            if k == "sparse_cg" and name.startswith("hann4"):      # (the CG form refuses this ill-conditioned band: tools/sparse_factored_bench.py records the message)
                continue
            hs[k], ts = timed(lambda: pkg.HipFeasibility(pkg.Feasibility(S, free(), n)))
            if k != "empty":
                out["setup_s"]["sparse_factored %s %s" % (name, k)] = ts
            hs[k].set_alg(pkg.AP())
        times = {k: [] for k in hs}
        for rep in range(3 + 21):
            for k, h in hs.items():
                h.set_iterate(x0)
                t0 = time.perf_counter(); h.step(1, 1, 10 ** 9, 1e-30); t = 1e6 * (time.perf_counter() - t0)
                if rep >= 3:
                    times[k].append(t)
        for k, v in times.items():
            out["times"]["sparse_factored %s %s step_us" % (name, k)] = statistics.median(v)
        st = hs["factored"].affine_sparse_factored_stats(1)
        out["counts"]["sparse_factored " + name] = {"launches": st["launches"], "launches_refine1": hs["factored_refine1"].affine_sparse_factored_stats(1)["launches"],
                                                    "items_rows": st["items_rows"], "items_cols": st["items_cols"], "segments": st["segments"], "bytes": st["bytes"],
                                                    "cold_cg_iterations": hs["sparse_cg"].affine_stats(1)["last_cg_iterations"] if "sparse_cg" in hs else None}
        for h in hs.values():
            h.close()
    A, b = sfc.rand(10000, 1000000, 10)
    d, ts = timed(lambda: pkg.HipFeasibility(pkg.Feasibility(pkg.IndAffine(A, b, form="sparse_factored"), pkg.IndBox(-np.inf, np.inf), 1000000)))
    out["setup_s"]["sparse_factored rand_10000x1000000x10"] = ts
    d.close()

    # ---- tools/nspace_cg_bench.py's measure(), n = 10^5 for the times and n = 10^6 for the set-up
    rng = np.random.default_rng(0)
    for n, reps in [(100000, 7), (1000000, 2)]:
        Q, q, x = ncb.pentadiagonal(n), rng.standard_normal(n), rng.standard_normal(n)
        A, b = ncb.sparse_a(n // 10, n, 10, rng), rng.standard_normal(n // 10)
        for key, S in {"quadratic_cg pentadiagonal n=%d" % n: pkg.Quadratic(Q, q, form="cg"), "ls_cg %dx%d" % (n // 10, n): pkg.LeastSquares(A, b, 1.0, form="cg")}.items():
            row = ncb.measure(pkg, S, n, x, reps)
            out["setup_s"]["nspace_cg " + key] = row["setup_s"]
            if n == 100000:
                out["counts"]["nspace_cg " + key] = {k: row[k] for k in ("cold_iters", "warm_iters", "restarts", "launches_per_iter", "stored")}
                out["times"]["nspace_cg %s cold_us" % key] = row["cold_us"]
                out["times"]["nspace_cg %s warm_us" % key] = row["warm_us"]
    print(json.dumps(out), flush=True)


def merge(src, dst):
    src, dst = Path(src), Path(dst)
    S = {s: {w: json.loads((src / ("speed_s%d_%s.json" % (s, w))).read_text().strip().splitlines()[-1]) for w in ("parent1", "new", "parent2")} for s in (1, 2)}
    doc = {"what": "parent (cadb716), this change, parent in one session with the libraries alternating (one process each), the session twice, one MI355X; "
                   "the measurements of tools/sparse_affine_bench.py, tools/sparse_factored_bench.py and tools/nspace_cg_bench.py at reduced shapes, "
                   "and the set-up time of each one's largest instance",
           "band": "a timed metric is inside when the new value lies within [min(p1, p2) - |p1 - p2|, max(p1, p2) + |p1 - p2|] of that session",
           "sessions": {}, "counts_equal": True, "metrics": {}}
    for s in (1, 2):
        doc["sessions"][str(s)] = S[s]
        for w in ("new", "parent2"):
            if S[s][w]["counts"] != S[s]["parent1"]["counts"]:
                doc["counts_equal"] = False
    for group in ("times", "setup_s"):
        for k in S[1]["parent1"][group]:
            row = {}
            for s in (1, 2):
                p1, p2, nw = (S[s][w][group][k] for w in ("parent1", "parent2", "new"))
                spread = abs(p1 - p2)
                row["session%d" % s] = {"parent1": p1, "parent2": p2, "new": nw, "parents_spread_rel": round(spread / ((p1 + p2) / 2), 4),
                                        "new_over_parents_mean": round(nw / ((p1 + p2) / 2), 4), "inside": min(p1, p2) - spread <= nw <= max(p1, p2) + spread}
            row["outside_in_both"] = not row["session1"]["inside"] and not row["session2"]["inside"]
            doc["metrics"]["%s: %s" % (group, k)] = row
    rows = doc["metrics"]
    doc["summary"] = {
        "metrics": len(rows), "outside_session1": sum(not r["session1"]["inside"] for r in rows.values()), "outside_session2": sum(not r["session2"]["inside"] for r in rows.values()),
        "outside_in_both": [k for k, r in rows.items() if r["outside_in_both"]],
        "geomean_new_over_parents_mean": {"session%d" % s: round(statistics.geometric_mean(r["session%d" % s]["new_over_parents_mean"] for r in rows.values()), 4) for s in (1, 2)},
        "median_parents_spread_rel": {"session%d" % s: round(statistics.median(r["session%d" % s]["parents_spread_rel"] for r in rows.values()), 4) for s in (1, 2)},
    }
    dst.write_text(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(doc["summary"], indent=1), "counts_equal:", doc["counts_equal"])
    for k, r in rows.items():
        a, b = r["session1"], r["session2"]
        print("%-72s s1 p %.4g/%.4g new %.4g %s | s2 p %.4g/%.4g new %.4g %s" % (k, a["parent1"], a["parent2"], a["new"], "in" if a["inside"] else "OUT",
                                                                                 b["parent1"], b["parent2"], b["new"], "in" if b["inside"] else "OUT"))


if __name__ == "__main__":
    if sys.argv[1:2] == ["--merge"]:
        merge(sys.argv[2], sys.argv[3])
    else:
        measure_all()
