#!/usr/bin/env python
"""Feasibility form: the n-space forms (csrc/nspace.hip) on the device -- Quadratic(Q, q) and LeastSquares(form="normal").

(1) One Quadratic prox at n = 2000, 10000, 20000 (Q = U U' + diag, U of 32 columns): ONE step of AP (S1 = the Quadratic, S2 = IndBox(-inf, inf)) against the
    empty step (S1 = S2 = IndBox(-inf, inf)) and, up to --callback-max, against the same prox as a host callback (a numpy Cholesky solve), on handles that
    alternate in the same process.  The prox reads both tile streams: 4 L^2 bytes of K twice, 4 L^2 of Mt once.
(2) The one-right-hand-side tile product alone (ns_symv_kernel + fold) against red_symm_kernel + fold on the SAME tiles with a zero second right-hand side, in the
    same process (fos_bench_symv_packed, device events around --product-reps products each), with the bytes of the stream per second of both.
(3) One tall LeastSquares prox at (m, n) = (10^6, 100) and (40000, 2000) against the callback path.
(4) DR on Quadratic n IndBox(0, 1) (a box QP) and (5) DR on a tall LeastSquares + NormL1 (the lasso): time per step, iterations to eps = 1e-6, residuals.
Step times are a host clock around fos_feas_step, which ends in a stream synchronise; warm-up first, median of --reps repetitions.  Prints one JSON document.
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import scipy.linalg

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import __graft_entry__ as ge  # noqa: E402


class HostSolve:
    """y = M^-1 (x + c) by a numpy Cholesky solve: the prox as the callback path runs it"""

    def __init__(self, M, c):
        self.chol, self.c = scipy.linalg.cho_factor(M), c

    def prox(self, y, x):
        y[:] = scipy.linalg.cho_solve(self.chol, x + self.c)


def one_step_us(h, x0):
    h.set_iterate(x0)                                       # untimed: the same start for every repetition (ends in a synchronise)
    t0 = time.perf_counter()
    h.step(1, 1, 10 ** 9, 1e-30)                            # fos_feas_step ends in hipStreamSynchronize
    return (time.perf_counter() - t0) * 1e6


def alternate(handles, x0, warmup, reps):
    times = {k: [] for k in handles}
    for rep in range(warmup + reps):
        for k, h in handles.items():
            t = one_step_us(h, x0)
            if rep >= warmup:
                times[k].append(t)
    return {k: statistics.median(v) for k, v in times.items()}, {k: [round(min(v), 1), round(max(v), 1)] for k, v in times.items()}


def prox_row(pkg, a, S, host, n, x0, setup_s, extra):
    free = lambda: pkg.IndBox(-np.inf, np.inf)
    handles = {"device": pkg.HipFeasibility(pkg.Feasibility(S, free(), n)), "empty": pkg.HipFeasibility(pkg.Feasibility(free(), free(), n))}
    if host is not None:
        handles["callback"] = pkg.HipFeasibility(pkg.Feasibility(host, free(), n))
    for h in handles.values():
        h.set_alg(pkg.AP())
    med, spread = alternate(handles, x0, a.warmup, a.reps)
    st = handles["device"].nspace_stats(1)
    row = dict(extra, n=n, setup_s=round(setup_s, 2), step_us={k: round(v, 1) for k, v in med.items()}, step_us_min_max=spread,
               prox_us={k: round(med[k] - med["empty"], 1) for k in med if k != "empty"}, launches=st["launches"], tiles=st["tiles"], bytes_kept=st["bytes"],
               bytes_read_per_prox=3 * st["tiles"] * 16384, probe_resid=st["probe_resid"], factor=st["factor"])
    row["GB_per_s"] = round(row["bytes_read_per_prox"] / max(row["prox_us"]["device"], 1e-9) / 1e3, 1)
    if host is not None:
        row["max_abs_diff_vs_callback"] = float(np.abs(handles["device"].prox(1, x0) - handles["callback"].prox(1, x0)).max())
    for h in handles.values():
        h.close()
    print(json.dumps(row), flush=True)
    return row


def make_quadratic(n, seed):
    rng = np.random.default_rng(seed)
    U = rng.standard_normal((n, 32)) / np.sqrt(32.0)
    Q = U @ U.T
    Q[np.diag_indices(n)] += rng.uniform(0.0, 2.0, n)
    return Q, rng.standard_normal(n), rng.standard_normal(n)


def quadratic(pkg, a):
    rows = []
    for n in a.quad_n:
        Q, q, x0 = make_quadratic(n, n)
        t0 = time.perf_counter()
        S = pkg.Quadratic(Q, q)
        host = HostSolve(np.eye(n) + Q, -q) if n <= a.callback_max else None
        h = pkg.HipFeasibility(pkg.Feasibility(S, pkg.IndBox(-np.inf, np.inf), n))      # (the set-up alone, timed)
        setup = time.perf_counter() - t0
        y = h.prox(1, x0)
        h.close()
        res = float(np.abs(y + Q @ y - (x0 - q)).max())                                 # |(I + Q) y - (x - q)|_inf
        rows.append(prox_row(pkg, a, S, host, n, x0, setup, {"what": "Quadratic", "optimality_residual_inf": res}))
    return rows


def product(pkg, a):
    lib = pkg.lib.load()
    rows = []
    for k in a.product_k:
        out = np.zeros(4)
        pkg.lib.check(lib.fos_bench_symv_packed(0, k, a.product_reps, pkg.lib.dptr(out)))
        row = {"k": k, "reps": a.product_reps, "tile_bytes": int(out[2]), "one_rhs_ms": round(out[0], 4), "two_rhs_kernel_ms": round(out[1], 4),
               "one_rhs_GB_per_s": round(out[2] / out[0] / 1e6, 1), "two_rhs_kernel_GB_per_s": round(out[2] / out[1] / 1e6, 1),
               "one_rhs_over_two_rhs_time": round(out[0] / out[1], 3), "max_abs_diff": float(out[3])}
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def tall(pkg, a):
    rows = []
    for m, n in a.tall:
        rng = np.random.default_rng(m + n)
        A = rng.standard_normal((m, n))
        b = A @ rng.standard_normal(n) + 0.1 * rng.standard_normal(m)
        x0 = rng.standard_normal(n)
        lam = 1.0 / m                                                                   # lam |A'A| ~ 1: the step-1 prox is well scaled
        t0 = time.perf_counter()
        S = pkg.LeastSquares(A, b, lam, form="normal")
        h = pkg.HipFeasibility(pkg.Feasibility(S, pkg.IndBox(-np.inf, np.inf), n))
        setup = time.perf_counter() - t0
        y = h.prox(1, x0)
        h.close()
        res = float(np.abs(lam * (A.T @ (A @ y - b)) + y - x0).max())
        host = HostSolve(np.eye(n) + lam * (A.T @ A), lam * (A.T @ b))
        rows.append(prox_row(pkg, a, S, host, n, x0, setup, {"what": "LeastSquares(form=normal)", "m": m, "lam": lam, "optimality_residual_inf": res}))
    return rows


def solves(pkg, a):
    out = {}
    n = a.qp_n
    Q, q, _ = make_quadratic(n, 3)
    q = q - Q @ np.full(n, 0.5)                                                         # the unconstrained minimiser near the middle of the box: a mixed active set
    d = pkg.HipFeasibility(pkg.Feasibility(pkg.Quadratic(Q, q), pkg.IndBox(0.0, 1.0), n))
    d.set_alg(pkg.DR())
    d.set_iterate(None)
    d.step(1, 20, 10, 1e-30)                                                            # warm-up
    d.set_iterate(None)
    t0 = time.perf_counter()
    done, status, err, _ = d.step(1, a.max_iters, 10, 1e-6)
    dt = time.perf_counter() - t0
    x = np.clip(d.prox(1, d.get_iterate()), 0.0, 1.0)
    out["box_qp_dr"] = {"n": n, "eps": 1e-6, "checki": 10, "status": status, "iterations": int(done), "max_iters": a.max_iters, "err": err,
                        "us_per_step": round(dt / max(done, 1) * 1e6, 1), "solve_s": round(dt, 3), "inside": int(((x > 0) & (x < 1)).sum()),
                        "projected_gradient_residual_inf": float(np.abs(x - np.clip(x - (Q @ x + q), 0.0, 1.0)).max())}
    print(json.dumps(out["box_qp_dr"]), flush=True)
    d.close()
    m, n = a.lasso
    rng = np.random.default_rng(11)
    A = rng.standard_normal((m, n))
    xs = np.where(rng.random(n) < 0.05, rng.standard_normal(n), 0.0)
    b = A @ xs + 0.01 * rng.standard_normal(m)
    lam = 1.0 / m
    d = pkg.HipFeasibility(pkg.Feasibility(pkg.LeastSquares(A, b, lam, form="normal"), pkg.NormL1(a.mu), n))
    d.set_alg(pkg.DR())
    d.set_iterate(None)
    d.step(1, 20, 10, 1e-30)
    d.set_iterate(None)
    t0 = time.perf_counter()
    done, status, err, _ = d.step(1, a.max_iters, 10, 1e-6)
    dt = time.perf_counter() - t0
    x = d.prox(1, d.get_iterate())
    g = lam * (A.T @ (A @ x - b))
    on = np.abs(x) > 1e-6
    res = float(max(np.abs(g[on] + a.mu * np.sign(x[on])).max(initial=0.0), np.maximum(np.abs(g[~on]) - a.mu, 0.0).max(initial=0.0)))
    out["tall_lasso_dr"] = {"m": m, "n": n, "lam": lam, "mu": a.mu, "eps": 1e-6, "checki": 10, "status": status, "iterations": int(done), "max_iters": a.max_iters,
                            "err": err, "us_per_step": round(dt / max(done, 1) * 1e6, 1), "solve_s": round(dt, 3), "support": int(on.sum()), "kkt_residual_inf": res}
    print(json.dumps(out["tall_lasso_dr"]), flush=True)
    d.close()
    return out


def pairs(s):
    return [tuple(int(v) for v in p.split("x")) for p in s.split(",")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quad-n", type=lambda s: [int(v) for v in s.split(",")], default=[2000, 10000, 20000])
    ap.add_argument("--product-k", type=lambda s: [int(v) for v in s.split(",")], default=[2000, 10000, 20000])
    ap.add_argument("--product-reps", type=int, default=50)
    ap.add_argument("--tall", type=pairs, default=[(10 ** 6, 100), (40000, 2000)])
    ap.add_argument("--callback-max", type=int, default=10000)
    ap.add_argument("--qp-n", type=int, default=10000)
    ap.add_argument("--lasso", type=lambda s: pairs(s)[0], default=(40000, 2000))
    ap.add_argument("--mu", type=float, default=0.05)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--max-iters", type=int, default=20000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = ge.load_package()
    doc = {"tool": "tools/nspace_bench.py", "timing": "host clock around one fos_feas_step (ends in a stream synchronise); products: device events"}
    doc["product"] = product(pkg, a)
    doc["quadratic_prox"] = quadratic(pkg, a)
    doc["tall_least_squares_prox"] = tall(pkg, a)
    doc.update(solves(pkg, a))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(doc, indent=1) + "\n")
    print(json.dumps({"one_rhs_not_slower_per_byte": all(r["one_rhs_over_two_rhs_time"] <= 1.0 for r in doc["product"])}))


if __name__ == "__main__":
    main()
