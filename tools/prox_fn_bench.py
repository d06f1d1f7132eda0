#!/usr/bin/env python
"""Feasibility form: the proximable functions that are not indicators (csrc/sets.hip kinds FOS_FN_*, LeastSquares on csrc/affine_dense.hip) on the device.

(1) Every separable kind at n = 10^6, as ONE block and as 10^4 blocks of 100, in the style of tools/feas_sets_bench.py: ONE step of AP (S1 = the function
    under test, S2 = IndBox(-inf, inf)) from the same seeded start, on handles that alternate in the same process:
        device     S1 by the kernels (fos_feas_set_blocks)
        sibling    the indicator of the same class of work -- IndBox (elementwise), IndBallL2 (one reduction), IndBallL1 (threshold search) -- by the kernels
        callback   S1 = the numpy reference of tests/prox_fn_cases.py through fos_feas_set_callback (fewer repetitions: it is 10^3 times slower)
        empty      S1 = IndBox(-inf, inf): the cost of the step around the prox
(2) One LeastSquares(A, b, lam) prox at (m, n) = (2000, 40000) against the IndAffine(form="factored") projection of the same A: the same launches.
(3) DR on LeastSquares(A, b, lam) and NormL1(mu) at that shape (the lasso): time per step and iterations to eps = 1e-6.
Times are a host clock around fos_feas_step, which ends in a stream synchronise; warm-up first, median of --reps repetitions.  Prints one JSON document.
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import __graft_entry__ as ge  # noqa: E402
from prox_fn_cases import ELEMENTWISE, KINDS, REDUCTION, make_fn  # noqa: E402
from set_cases import RefSeparableSum, make_set  # noqa: E402


def sibling_of(kind):
    return "IndBox" if kind in ELEMENTWISE else "IndBallL2" if kind in REDUCTION else "IndBallL1"


def build(pkg, kind, n, nblocks, seed):
    rng = np.random.default_rng(seed)
    length = n // nblocks
    dev, ref = [], []
    for _ in range(nblocks):
        r, args, _ = make_fn(kind, length, rng) if kind in KINDS else make_set(kind, length, rng, variant=0)
        dev.append((getattr(pkg, kind)(*args), length))
        ref.append((r, length))
    return pkg.SeparableSum(dev), (ref[0][0] if nblocks == 1 else RefSeparableSum(ref))


def one_step_us(h, x0):
    h.set_iterate(x0)                                       # untimed: the same start for every repetition (ends in a synchronise)
    t0 = time.perf_counter()
    h.step(1, 1, 10 ** 9, 1e-30)                            # fos_feas_step ends in hipStreamSynchronize
    return (time.perf_counter() - t0) * 1e6


def alternate(handles, x0, warmup, reps, slow=()):
    """median, min and max step time of every handle; the handles named in `slow` run a fifth of the repetitions"""
    times = {k: [] for k in handles}
    for rep in range(warmup + reps):
        for k, h in handles.items():
            if k in slow and rep % 5:
                continue
            t = one_step_us(h, x0)
            if rep >= warmup:
                times[k].append(t)
    return {k: statistics.median(v) for k, v in times.items()}, {k: [round(min(v), 1), round(max(v), 1)] for k, v in times.items()}


def separable(pkg, a):
    n = a.n
    free = lambda: pkg.IndBox(-np.inf, np.inf)
    x0 = np.random.default_rng(0).standard_normal(n)
    rows = []
    for kind in a.kinds.split(","):
        for nblocks in (1, a.blocks):
            S, ref = build(pkg, kind, n, nblocks, seed=nblocks)
            Ssib, _ = build(pkg, sibling_of(kind), n, nblocks, seed=nblocks)
            handles = {"device": pkg.HipFeasibility(pkg.Feasibility(S, free(), n)), "sibling": pkg.HipFeasibility(pkg.Feasibility(Ssib, free(), n)),
                       "callback": pkg.HipFeasibility(pkg.Feasibility(ref, free(), n)), "empty": pkg.HipFeasibility(pkg.Feasibility(free(), free(), n))}
            for h in handles.values():
                h.set_alg(pkg.AP())
            y_dev, y_ref = handles["device"].prox(1, x0), handles["callback"].prox(1, x0)
            med, spread = alternate(handles, x0, a.warmup, a.reps, slow=("callback",))
            st, sts = handles["device"].set_stats(1), handles["sibling"].set_stats(1)
            row = {"kind": kind, "sibling": sibling_of(kind), "n": n, "blocks": nblocks, "reps": a.reps, "max_abs_diff_vs_reference": float(np.abs(y_dev - y_ref).max()),
                   "step_us": {k: round(v, 1) for k, v in med.items()}, "step_us_min_max": spread,
                   "prox_us": {k: round(med[k] - med["empty"], 1) for k in ("device", "sibling", "callback")},
                   "device_step_over_sibling_step": round(med["device"] / med["sibling"], 3), "device_faster_than_callback": med["device"] < med["callback"],
                   "launches": st["launches"], "sibling_launches": sts["launches"], "threshold_passes": st["last_passes"], "sibling_threshold_passes": sts["last_passes"]}
            rows.append(row)
            print(json.dumps(row), flush=True)
            for h in handles.values():
                h.close()
    return rows


def least_squares(pkg, a):
    m, n = a.m, a.ncols
    rng = np.random.default_rng(7)
    A = rng.standard_normal((m, n))
    xs = np.where(rng.random(n) < 0.01, rng.standard_normal(n), 0.0)       # a sparse signal: b = A xs + noise
    b = A @ xs + 0.01 * rng.standard_normal(m)
    x0 = rng.standard_normal(n)
    free = lambda: pkg.IndBox(-np.inf, np.inf)
    t0 = time.perf_counter()
    hl = pkg.HipFeasibility(pkg.Feasibility(pkg.LeastSquares(A, b, a.lam), free(), n))
    t1 = time.perf_counter()
    ha = pkg.HipFeasibility(pkg.Feasibility(pkg.IndAffine(A, b, form="factored"), free(), n))
    t2 = time.perf_counter()
    handles = {"least_squares": hl, "ind_affine_factored": ha, "empty": pkg.HipFeasibility(pkg.Feasibility(free(), free(), n))}
    for h in handles.values():
        h.set_alg(pkg.AP())
    y = hl.prox(1, x0)
    kkt = float(np.abs(a.lam * (A.T @ (A @ y - b)) + y - x0).max())        # the prox's optimality condition, in the caller's units
    med, spread = alternate(handles, x0, a.warmup, a.reps)
    sl, sa = hl.affine_factored_stats(1), ha.affine_factored_stats(1)
    prox = {"m": m, "n": n, "lam": a.lam, "setup_s": {"least_squares": round(t1 - t0, 2), "ind_affine_factored": round(t2 - t1, 2)},
            "optimality_residual_inf": kkt, "step_us": {k: round(v, 1) for k, v in med.items()}, "step_us_min_max": spread,
            "prox_us": {k: round(med[k] - med["empty"], 1) for k in ("least_squares", "ind_affine_factored")},
            "least_squares_over_ind_affine": round((med["least_squares"] - med["empty"]) / (med["ind_affine_factored"] - med["empty"]), 3),
            "launches": {"least_squares": sl["launches"], "ind_affine_factored": sa["launches"]}, "bytes_of_A_per_prox": 16 * m * sl["ld"],
            "plan": {k: sl[k] for k in ("ld", "gram_order", "span_cols", "spans", "rows_per_block", "row_blocks")}, "probe_resid": sl["probe_resid"]}
    print(json.dumps(prox), flush=True)
    ha.close()
    handles["empty"].close()
    # the lasso by DR on the same object
    d = pkg.HipFeasibility(pkg.Feasibility(pkg.LeastSquares(A, b, a.lam), pkg.NormL1(a.mu), n))
    hl.close()
    d.set_alg(pkg.DR())
    d.set_iterate(None)
    d.step(1, 20, 10, 1e-30)                                # warm-up
    d.set_iterate(None)
    t0 = time.perf_counter()
    done, status, err, _ = d.step(1, a.max_iters, 10, 1e-6)
    dt = time.perf_counter() - t0
    x = d.prox(1, d.get_iterate())
    g = a.lam * (A.T @ (A @ x - b))
    on = np.abs(x) > 1e-6
    res = float(max(np.abs(g[on] + a.mu * np.sign(x[on])).max(initial=0.0), np.maximum(np.abs(g[~on]) - a.mu, 0.0).max(initial=0.0)))
    lasso = {"m": m, "n": n, "lam": a.lam, "mu": a.mu, "eps": 1e-6, "checki": 10, "status": status, "iterations": int(done), "max_iters": a.max_iters, "err": err,
             "us_per_step": round(dt / max(done, 1) * 1e6, 1), "solve_s": round(dt, 3), "support": int(on.sum()), "kkt_residual_inf": res}
    print(json.dumps(lasso), flush=True)
    d.close()
    return prox, lasso


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10 ** 6)
    ap.add_argument("--blocks", type=int, default=10 ** 4)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kinds", default=",".join(KINDS))
    ap.add_argument("--m", type=int, default=2000)
    ap.add_argument("--ncols", type=int, default=40000)
    ap.add_argument("--lam", type=float, default=1e-3)       # lam |A'A| ~ 1 for standard normal entries at these shapes: the step-1 prox is well scaled
    ap.add_argument("--mu", type=float, default=0.05)
    ap.add_argument("--max-iters", type=int, default=20000)
    ap.add_argument("--skip-separable", action="store_true")
    ap.add_argument("--skip-least-squares", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = ge.load_package()
    doc = {"tool": "tools/prox_fn_bench.py", "timing": "host clock around one fos_feas_step (ends in a stream synchronise)"}
    if not a.skip_separable:
        doc["separable"] = separable(pkg, a)
        doc["all_faster_than_callback"] = all(r["device_faster_than_callback"] for r in doc["separable"])
    if not a.skip_least_squares:
        doc["least_squares_prox"], doc["lasso_dr"] = least_squares(pkg, a)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(doc, indent=1) + "\n")
    print(json.dumps({"cases": len(doc.get("separable", [])), "all_faster_than_callback": doc.get("all_faster_than_callback")}))


if __name__ == "__main__":
    main()
