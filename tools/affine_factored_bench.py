#!/usr/bin/env python
"""Feasibility form: the FACTORED dense IndAffine (csrc/affine_dense.hip) against what a dense A gets without it.

    narrow shapes (n <= 46 000)   against the PROJECTOR form (fos_feas_set_affine: the n x n matrix A'(A A')^-1 A, 8 n^2 bytes per projection whatever m is)
    wide shapes (n > 46 000)      against the SPARSE-CG form on a CSC matrix holding every entry, which is what IndAffine(A, b) turns a dense A of that
                                  width into (fos_feas_set_affine_sparse)

Protocol of tools/feas_sets_bench.py: ONE step of AP (S1 = the set under test, S2 = IndBox(-inf, inf)) from the same seeded start, a host clock around
fos_feas_step (which ends in a stream synchronise), the start vector re-loaded (untimed) before every repetition, the handles alternating in one process,
warm-up first, median of --reps repetitions; `empty` (S1 = IndBox(-inf, inf)) is the cost of the step around the projection.  The projector's projection reads
the same 8 n^2 bytes whatever A is, and its set-up (Newton-Schulz on n x n matrices) takes minutes at n = 40 000: the shapes of one n share ONE projector
handle, built for the first of them (`projector_built_for`), which alternates with each shape's factored handle.
Per shape: set-up seconds of each form, bytes kept, and the bytes the factored projection must read by the model 16 m ld + 24 Lm^2 (A twice; X, G, X once)
over the difference of the step times.  Writes one JSON document (--out)."""
import argparse
import json
import statistics
import sys
import threading
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import __graft_entry__ as ge  # noqa: E402

HBM_BYTES_PER_S = 8e12
NARROW = [(2000, 40000), (10000, 40000), (20000, 40000)]
WIDE = [(2000, 200000), (100, 1000000)]


def instance(m, n):
    rng = np.random.default_rng(m + n)
    A = rng.standard_normal((m, n))
    return A, A @ np.maximum(rng.standard_normal(n), 0.0)


def one_step_us(h, x0):
    h.set_iterate(x0)                                       # untimed: the same start for every repetition (ends in a synchronise)
    t0 = time.perf_counter()
    h.step(1, 1, 10 ** 9, 1e-30)                            # fos_feas_step ends in hipStreamSynchronize
    return (time.perf_counter() - t0) * 1e6


def timed(label, fn):
    """fn() with a line on stderr every 60 s while it runs (a set-up may take minutes)"""
    stop = threading.Event()

    def beat():
        t0 = time.time()
        while not stop.wait(60.0):
            print("... %s: %.0f s" % (label, time.time() - t0), file=sys.stderr, flush=True)
    th = threading.Thread(target=beat, daemon=True)
    th.start()
    t0 = time.perf_counter()
    try:
        return fn(), time.perf_counter() - t0
    finally:
        stop.set()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join("%dx%d" % s for s in NARROW + WIDE))
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--refine", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = ge.load_package()
    free = lambda: pkg.IndBox(-np.inf, np.inf)
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")]
    results, projector = [], {}                             # projector: n -> (handle, set-up seconds, m it was built for)

    def write():
        if a.out:
            doc = {"tool": "tools/affine_factored_bench.py", "timing": "host clock around one fos_feas_step (ends in a stream synchronise), median of %d after %d warm-ups" % (a.reps, a.warmup),
                   "bytes_model": "16 m ld + 24 Lm^2", "results": results}
            Path(a.out).parent.mkdir(parents=True, exist_ok=True)
            Path(a.out).write_text(json.dumps(doc, indent=1) + "\n")

    for m, n in shapes:
        A, b = instance(m, n)
        x0 = np.random.default_rng(0).standard_normal(n)
        handles, setup_s = {}, {}
        handles["factored"], setup_s["factored"] = timed("factored set-up %dx%d" % (m, n),
                                                         lambda: pkg.HipFeasibility(pkg.Feasibility(pkg.IndAffine(A, b, form="factored", refine=a.refine), free(), n)))
        if n <= pkg.IndAffine.DENSE_MAX:
            other = "projector"
            if n not in projector:
                h, s = timed("projector set-up %dx%d" % (m, n), lambda: pkg.HipFeasibility(pkg.Feasibility(pkg.IndAffine(A, b), free(), n)))
                projector[n] = (h, s, m)
            handles[other], setup_s[other], built_for = projector[n]
        else:
            other, built_for = "sparse_cg", m
            handles[other], setup_s[other] = timed("sparse-CG set-up %dx%d" % (m, n), lambda: pkg.HipFeasibility(pkg.Feasibility(pkg.IndAffine(A, b), free(), n)))
        handles["empty"] = pkg.HipFeasibility(pkg.Feasibility(free(), free(), n))
        for h in handles.values():
            h.set_alg(pkg.AP())
        y_f = handles["factored"].prox(1, x0)
        diff = float(np.abs(handles[other].prox(1, x0) - y_f).max()) if built_for == m else None
        times = {k: [] for k in handles}
        for rep in range(a.warmup + a.reps):
            for k, h in handles.items():                    # alternating
                t = one_step_us(h, x0)
                if rep >= a.warmup:
                    times[k].append(t)
        med = {k: statistics.median(v) for k, v in times.items()}
        st = handles["factored"].affine_factored_stats(1)
        model_bytes = 16 * m * st["ld"] + 24 * st["gram_order"] ** 2
        proj_us = {k: med[k] - med["empty"] for k in ("factored", other)}
        row = {"m": m, "n": n, "against": other, "reps": a.reps, "refine": a.refine, "max_abs_diff_between_forms": diff,
               "step_us": {k: round(v, 1) for k, v in med.items()}, "step_us_min_max": {k: [round(min(v), 1), round(max(v), 1)] for k, v in times.items()},
               "projection_us": {k: round(v, 1) for k, v in proj_us.items()}, "factored_speedup": round(proj_us[other] / proj_us["factored"], 2),
               "setup_s": {k: round(v, 2) for k, v in setup_s.items()}, "bytes_kept": {"factored": st["bytes"]},
               "model_bytes_per_projection": model_bytes, "model_share_of_8TBps": round(model_bytes / (proj_us["factored"] * 1e-6) / HBM_BYTES_PER_S, 4),
               "factored_stats": st}
        if other == "projector":
            L = (n + 63) // 64 * 64
            row["projector_built_for"] = [built_for, n]
            row["bytes_kept"]["projector"] = 8 * (L * L + L)
            row["projector_share_of_8TBps"] = round(8 * L * L / (proj_us[other] * 1e-6) / HBM_BYTES_PER_S, 4)
        else:
            sa = handles[other].affine_stats(1)
            row["bytes_kept"]["sparse_cg"] = 2 * 12 * sa["nnz"]
            row["sparse_cg_last_iterations"] = sa["last_cg_iterations"]
        results.append(row)
        print(json.dumps(row), flush=True)
        write()
        for k, h in handles.items():
            if k != "projector":
                h.close()
        del A
    for h, _, _ in projector.values():
        h.close()
    write()


if __name__ == "__main__":
    main()
