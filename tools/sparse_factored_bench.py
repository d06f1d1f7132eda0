#!/usr/bin/env python
"""Feasibility form: the FACTORED sparse IndAffine (csrc/affine_sparse_factored.hip) against the conjugate-gradient sparse form of the same A
(csrc/affine_sparse.hip), one case per run (--case), the results merged by case name into one JSON document (--out).

Protocol of tools/affine_factored_bench.py: ONE step of AP (S1 = the set under test, S2 = IndBox(-inf, inf)) from the same seeded start, a host clock around
fos_feas_step (which ends in a stream synchronise), the start vector re-loaded (untimed) before every repetition -- which also sets the CG form's multipliers to
zero: its projection is a COLD one -- the handles alternating in one process, warm-up first, median of --reps repetitions; `empty` (S1 = IndBox(-inf, inf)) is the
cost of the step around the projection.  The steady state of a solve (the CG form warm-started) is measured beside it: iterations 51 .. 100 of DR on
IndAffine n IndBox(0, inf), per iteration, with the CG iterations per projection.

The factored form runs with refine = 0 and refine = 1.  A refinement step adds one of each pass and one m-space product, so with T0, T1 the two projection times
    passes (both, once) + one product = T1 - T0,     one product = (T0 - (T1 - T0)) / 2
which gives the rate of the passes on the model 2 * 12 nnz + 8 (2 n + 2 m) bytes and of the m-space on 8 L^2 bytes per product (24 L^2 per projection)."""
import argparse
import json
import os
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import __graft_entry__ as ge  # noqa: E402
import sparse_factored_cases as cases  # noqa: E402

HBM_BYTES_PER_S = 8e12
CASES = {
    "rand_2000x8000x8": lambda: cases.rand(2000, 8000, 8),
    "rand_40000x120000x5": lambda: cases.rand(40000, 120000, 5),
    "rand_2000x200000x10": lambda: cases.rand(2000, 200000, 10),
    "rand_10000x1000000x10": lambda: cases.rand(10000, 1000000, 10),
    "skew_100_rows_of_50000": lambda: cases.skew(2000, 1000000, [50000] * 100, 5),
    "hann4_band_2000": lambda: cases.band(2000, cases.HANN4),
}


def one_step_us(h, x0):
    h.set_iterate(x0)                                       # untimed: the same start for every repetition (ends in a synchronise)
    t0 = time.perf_counter()
    h.step(1, 1, 10 ** 9, 1e-30)                            # fos_feas_step ends in hipStreamSynchronize
    return (time.perf_counter() - t0) * 1e6


def timed(fn):
    t0 = time.perf_counter()
    return fn(), time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", required=True, choices=sorted(CASES))
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-steady", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = ge.load_package()
    free = lambda: pkg.IndBox(-np.inf, np.inf)
    A, b = CASES[a.case]()
    m, n = A.shape
    x0 = np.random.default_rng(0).standard_normal(n)
    sets = {"factored": lambda: pkg.IndAffine(A, b, form="sparse_factored"), "factored_refine1": lambda: pkg.IndAffine(A, b, form="sparse_factored", refine=1),
            "sparse_cg": lambda: pkg.IndAffine(A, b)}
    handles, setup_s = {}, {}
    for k, S in sets.items():
        handles[k], setup_s[k] = timed(lambda: pkg.HipFeasibility(pkg.Feasibility(S(), free(), n)))
        print("%s set-up: %.2f s" % (k, setup_s[k]), file=sys.stderr, flush=True)
    handles["empty"] = pkg.HipFeasibility(pkg.Feasibility(free(), free(), n))
    for h in handles.values():
        h.set_alg(pkg.AP())
    y_f = handles["factored"].prox(1, x0)
    cg_error = None                                         # the CG form may refuse an ill-conditioned A (the residual stays above its rounding level)
    try:
        diff = float(np.abs(handles["sparse_cg"].prox(1, x0) - y_f).max())
    except pkg.lib.FosError as e:
        diff, cg_error = None, str(e)
    times = {k: [] for k in handles}
    cold_its = []
    for rep in range(a.warmup + a.reps):
        for k, h in handles.items():                        # alternating
            if k == "sparse_cg" and cg_error:
                continue
            try:
                t = one_step_us(h, x0)
            except pkg.lib.FosError as e:
                if k != "sparse_cg":
                    raise
                cg_error = str(e)
                continue
            if rep >= a.warmup:
                times[k].append(t)
                if k == "sparse_cg":
                    cold_its.append(h.affine_stats(1)["last_cg_iterations"])
    if cg_error:
        times.pop("sparse_cg")
    med = {k: statistics.median(v) for k, v in times.items()}
    st = handles["factored"].affine_sparse_factored_stats(1)
    proj = {k: med[k] - med["empty"] for k in sets if k in med}
    t0, t1 = proj["factored"], proj["factored_refine1"]
    symv_us = (t0 - (t1 - t0)) / 2
    passes_us = (t1 - t0) - symv_us
    pass_bytes = 2 * 12 * st["nnz"] + 8 * (2 * n + 2 * m)
    L = st["gram_order"]
    rate = lambda bytes_, us: round(bytes_ / (us * 1e-6) / HBM_BYTES_PER_S, 4) if us > 0 else None
    row = {"case": a.case, "m": m, "n": n, "nnz": st["nnz"], "reps": a.reps, "seg": st["seg"], "FOS_SF_SEG": os.environ.get("FOS_SF_SEG"),
           "max_abs_diff_between_forms": diff,
           "step_us": {k: round(v, 1) for k, v in med.items()}, "step_us_min_max": {k: [round(min(v), 1), round(max(v), 1)] for k, v in times.items()},
           "projection_us": {k: round(v, 1) for k, v in proj.items()}, "factored_speedup_over_cold_cg": None if cg_error else round(proj["sparse_cg"] / proj["factored"], 2),
           "cold_cg_iterations": None if cg_error else int(statistics.median(cold_its)), "sparse_cg_error": cg_error,
           "launches": {"factored": st["launches"], "factored_refine1": handles["factored_refine1"].affine_sparse_factored_stats(1)["launches"]},
           "derived_us": {"both_passes": round(passes_us, 1), "one_mspace_product": round(symv_us, 1)},
           "pass_model_bytes": pass_bytes, "passes_share_of_8TBps": rate(pass_bytes, passes_us),
           "mspace_model_bytes": 24 * L * L, "mspace_share_of_8TBps": rate(8 * L * L, symv_us),
           "setup_s": {k: round(v, 2) for k, v in setup_s.items()}, "bytes_kept": {"factored": st["bytes"], "sparse_cg": 2 * 12 * st["nnz"]}, "factored_stats": st}
    if not a.no_steady:                                     # the steady state of a solve: DR iterations 51 .. 100 on IndAffine n IndBox(0, inf)
        steady = {}
        for k in ("factored", "sparse_cg"):
            h = pkg.HipFeasibility(pkg.Feasibility(sets[k](), pkg.IndBox(0.0, np.inf), n))
            h.set_alg(pkg.DR()); h.set_iterate(x0)
            try:
                h.step(1, 50, 10 ** 9, 0.0)
                s0 = h.affine_stats(1)["cg_iterations"] if k == "sparse_cg" else 0
                t = time.perf_counter(); h.step(51, 50, 10 ** 9, 0.0); dt = time.perf_counter() - t
                steady[k + "_dr_iteration_us"] = round(1e6 * dt / 50, 1)
                if k == "sparse_cg":
                    steady["cg_iterations_per_projection"] = (h.affine_stats(1)["cg_iterations"] - s0) / 50.0
            except pkg.lib.FosError as e:
                steady[k + "_error"] = str(e)
            h.close()
        row["steady_state"] = steady
    print(json.dumps(row), flush=True)
    if a.out:
        path = Path(a.out)
        doc = json.loads(path.read_text()) if path.exists() else {}
        results = [r for r in doc.get("results", []) if not (r["case"] == a.case and r.get("FOS_SF_SEG") == row["FOS_SF_SEG"])] + [row]
        doc = {"tool": "tools/sparse_factored_bench.py",
               "timing": "host clock around one fos_feas_step (ends in a stream synchronise), median of %d after %d warm-ups; one case per process" % (a.reps, a.warmup),
               "bytes_model": "passes: 2 * 12 nnz + 8 (2 n + 2 m); m-space: 24 L^2 (8 L^2 per product)", "results": results}
        path.parent.mkdir(parents=True, exist_ok=True)
        path.write_text(json.dumps(doc, indent=1) + "\n")
    for h in handles.values():
        h.close()


if __name__ == "__main__":
    main()
