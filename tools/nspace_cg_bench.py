#!/usr/bin/env python
"""Feasibility form: the cg forms (csrc/nspace_cg.hip) on the device -- Quadratic(form="cg") and LeastSquares(form="cg").  Writes profiles/nspace_cg_bench.json.

Shapes: (i) a pentadiagonal Q, n = 10^6;  (ii) a sparse A, 10^5 x 10^6 with 10 entries per column, lam = 1;  (iii) a sparse A, (m, n) = (20 000, 40 000) with 5
entries per column, which form="normal" and form="sparse_factored" accept;  (iv) an arrow Q, n = 300 000 (one row and column of n entries).
  * per prox, cold and warm (the warm one at x + 1e-6 delta after the cold one), at (i), (ii), (iv): a host clock around fos_feas_prox, which ends in a stream
    synchronise, MINUS the same call on a handle whose set is a box (the two copies of the vector and the call itself); median of --reps.
  * per CG iteration: the cold prox divided by its iterations (the cold prox at these shapes IS its iterations: 50 and more), and the bytes it must move per second:
        Quadratic:     12 B per stored entry of I + Q  +  12 n-vectors of 8 B   (the pass gathers z and p and writes p and w; the update reads p, w, y, r, D^-1 and
                                                                                writes y, r, z -- a gathered vector counted once)
        LeastSquares:  12 B per stored entry of A and of A'  +  16 n-vectors and 2 m-vectors of 8 B   (A z gathers z and writes t; the A' pass gathers t, reads r
                                                                                and z and writes w; the update reads z, w, p, s, y, r, D^-1 and writes p, s, y, r, z)
  * against the host-callback path: the same prox as an object with prox(y, x) around scipy.sparse.linalg.cg (Jacobi-preconditioned, warm-started, rtol 1e-12) -- what
    a user had to write before.
  * fused against unfused (FOS_NC_UNFUSED=1: p in a launch of its own, three resp. four launches per iteration; for LeastSquares that is the plain recurrence
    against the merged one) at (i) and (ii).
  * segmented and packed row items against lanes-per-row (FOS_NC_ROWS=lpr) at (ii) and (iv).
  * (iii): set-up and prox of the three forms; break_even_iters = the kept-inverse prox divided by the time of one CG iteration: a warm-started prox that needs fewer
    iterations than that is faster by CG.
Handles alternate in one process; every figure is printed as it is measured.
"""
import argparse
import json
import os
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import __graft_entry__ as ge  # noqa: E402


class HostCG:
    """y = M^-1 rhs(x) by scipy's CG, Jacobi-preconditioned and warm-started: the prox as the callback path runs it"""

    def __init__(self, matvec, diag, rhs, n):
        self.op = spla.LinearOperator((n, n), matvec=matvec, dtype=np.float64)
        self.pre = spla.LinearOperator((n, n), matvec=lambda v: v / diag, dtype=np.float64)
        self.rhs, self.y0 = rhs, None

    def prox(self, y, x):
        sol, _ = spla.cg(self.op, self.rhs(np.asarray(x)), x0=self.y0, rtol=1e-12, atol=0.0, M=self.pre, maxiter=2000)
        self.y0 = sol
        y[:] = sol


def pentadiagonal(n):
    return sp.diags([np.ones(n - 2), -4.0 * np.ones(n - 1), 6.5 * np.ones(n), -4.0 * np.ones(n - 1), np.ones(n - 2)], [-2, -1, 0, 1, 2]).tocsc()


def arrow(n, rng):
    v = (0.5 / np.sqrt(n)) * rng.standard_normal(n)
    v[0] = 0.0
    Q = sp.diags(1.0 + rng.random(n)).tocsc() + sp.csc_matrix((v, (np.zeros(n, dtype=np.int64), np.arange(n))), shape=(n, n))
    Q = Q + sp.csc_matrix((v, (np.arange(n), np.zeros(n, dtype=np.int64))), shape=(n, n))
    return sp.csc_matrix(Q)


def sparse_a(m, n, per_col, rng):
    A = sp.csc_matrix((rng.standard_normal(n * per_col) / np.sqrt(per_col), (rng.integers(0, m, n * per_col), np.repeat(np.arange(n), per_col))), shape=(m, n))
    A.sum_duplicates(); A.sort_indices()
    return A


def timed(fn, reps):
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(t)


def measure(pkg, S, n, x, reps, env=None):
    """-> dict: set-up seconds, cold / warm prox microseconds (the box handle's call subtracted), iterations, microseconds per iteration"""
    for k, v in (env or {}).items():
        os.environ[k] = v
    t0 = time.perf_counter()
    d = pkg.HipFeasibility(pkg.Feasibility(S, pkg.IndFree(), n))
    setup = time.perf_counter() - t0
    for k in (env or {}):
        del os.environ[k]
    box = pkg.HipFeasibility(pkg.Feasibility(pkg.IndBox(-np.inf, np.inf), pkg.IndFree(), n))
    x2 = x + 1e-6 * np.random.default_rng(1).standard_normal(n)
    d.prox(1, x); box.prox(1, x)                                                   # warm-up of both
    base = timed(lambda: box.prox(1, x), reps)
    cold, warm, it_c, it_w = [], [], 0, 0
    for _ in range(reps):
        d.set_iterate(None)
        t0 = time.perf_counter(); d.prox(1, x); cold.append((time.perf_counter() - t0) * 1e6)
        it_c = d.nspace_cg_stats(1)["last_iters"]
        t0 = time.perf_counter(); d.prox(1, x2); warm.append((time.perf_counter() - t0) * 1e6)
        it_w = d.nspace_cg_stats(1)["last_iters"]
    st = d.nspace_cg_stats(1)
    c, w = statistics.median(cold) - base, statistics.median(warm) - base
    row = {"setup_s": round(setup, 2), "box_call_us": round(base, 1), "cold_us": round(c, 1), "warm_us": round(w, 1), "cold_iters": it_c, "warm_iters": it_w,
           "restarts": st["last_restarts"], "us_per_iter": round(c / max(it_c, 1), 2), "launches_per_iter": st["launches_per_iter"], "stored": st["stored"]}
    d.close(); box.close()
    return row


def callback(pkg, host, n, x, reps):
    d = pkg.HipFeasibility(pkg.Feasibility(host, pkg.IndFree(), n))
    x2 = x + 1e-6 * np.random.default_rng(1).standard_normal(n)
    cold, warm = [], []
    for _ in range(reps):
        host.y0 = None
        t0 = time.perf_counter(); d.prox(1, x); cold.append((time.perf_counter() - t0) * 1e6)
        t0 = time.perf_counter(); d.prox(1, x2); warm.append((time.perf_counter() - t0) * 1e6)
    d.close()
    return {"cold_us": round(statistics.median(cold), 1), "warm_us": round(statistics.median(warm), 1)}


def say(out, key, row):
    out[key] = row
    print(json.dumps({key: row}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=10 ** 6)
    ap.add_argument("--kept-n", type=int, default=40000, help="n of shape (iii); 0 skips it")
    ap.add_argument("--callback-reps", type=int, default=1)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "nspace_cg_bench.json"))
    a = ap.parse_args()
    pkg = ge.load_package()
    rng = np.random.default_rng(0)
    out = {"tool": "tools/nspace_cg_bench.py", "reps": a.reps,
           "bytes_per_iter": {"quadratic": "12 stored + 96 n", "least_squares": "12 stored + 128 n + 16 m"}}
    UNF, LPR = {"FOS_NC_UNFUSED": "1"}, {"FOS_NC_ROWS": "lpr"}

    # (i) pentadiagonal Q
    n = a.n
    Q, q, x = pentadiagonal(n), rng.standard_normal(n), rng.standard_normal(n)
    M = sp.csr_matrix(sp.identity(n) + Q)
    row = measure(pkg, pkg.Quadratic(Q, q, form="cg"), n, x, a.reps)
    row["GB_per_s"] = round((12 * row["stored"] + 96 * n) / row["us_per_iter"] / 1e3, 1)
    say(out, "i_pentadiagonal_n%d" % n, row)
    say(out, "i_unfused", measure(pkg, pkg.Quadratic(Q, q, form="cg"), n, x, a.reps, env=UNF))
    say(out, "i_callback_scipy_cg", callback(pkg, HostCG(lambda v: M @ v, M.diagonal(), lambda xx: xx - q, n), n, x, a.callback_reps))

    # (ii) sparse A, m = n / 10, 10 entries per column
    m = n // 10
    A, b = sparse_a(m, n, 10, rng), rng.standard_normal(m)
    At = sp.csr_matrix(A.T)
    Ar = sp.csr_matrix(A)
    row = measure(pkg, pkg.LeastSquares(A, b, 1.0, form="cg"), n, x, a.reps)
    row["GB_per_s"] = round((12 * row["stored"] + 128 * n + 16 * m) / row["us_per_iter"] / 1e3, 1)
    say(out, "ii_sparse_%dx%d" % (m, n), row)
    say(out, "ii_unfused", measure(pkg, pkg.LeastSquares(A, b, 1.0, form="cg"), n, x, a.reps, env=UNF))
    say(out, "ii_lanes_per_row", measure(pkg, pkg.LeastSquares(A, b, 1.0, form="cg"), n, x, a.reps, env=LPR))
    diag = 1.0 + np.asarray(A.multiply(A).sum(axis=0)).ravel()
    c = At @ b
    say(out, "ii_callback_scipy_cg", callback(pkg, HostCG(lambda v: v + At @ (Ar @ v), diag, lambda xx: xx + c, n), n, x, a.callback_reps))

    # (iv) the arrow matrix: one row of n entries
    na = 300000
    Qa, qa, xa = arrow(na, rng), rng.standard_normal(na), rng.standard_normal(na)
    say(out, "iv_arrow_n%d" % na, measure(pkg, pkg.Quadratic(Qa, qa, form="cg"), na, xa, a.reps))
    say(out, "iv_lanes_per_row", measure(pkg, pkg.Quadratic(Qa, qa, form="cg"), na, xa, a.reps, env=LPR))

    # (iii) against the kept-inverse forms
    if a.kept_n:
        nk, mk = a.kept_n, a.kept_n // 2
        Ak, bk, xk = sparse_a(mk, nk, 5, rng), rng.standard_normal(mk), rng.standard_normal(nk)
        row = measure(pkg, pkg.LeastSquares(Ak, bk, 1.0, form="cg"), nk, xk, a.reps)
        say(out, "iii_cg_%dx%d" % (mk, nk), row)
        for form in ("sparse_factored", "normal"):
            t0 = time.perf_counter()
            d = pkg.HipFeasibility(pkg.Feasibility(pkg.LeastSquares(Ak, bk, 1.0, form=form), pkg.IndFree(), nk))
            setup = time.perf_counter() - t0
            box = pkg.HipFeasibility(pkg.Feasibility(pkg.IndBox(-np.inf, np.inf), pkg.IndFree(), nk))
            d.prox(1, xk); box.prox(1, xk)
            t = timed(lambda: d.prox(1, xk), a.reps) - timed(lambda: box.prox(1, xk), a.reps)
            say(out, "iii_" + form, {"setup_s": round(setup, 2), "prox_us": round(t, 1), "break_even_iters": round(t / row["us_per_iter"], 1)})
            d.close(); box.close()
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps({"written": a.out}))


if __name__ == "__main__":
    main()
