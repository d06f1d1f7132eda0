#!/usr/bin/env python
"""Feasibility form: the dense Quadratic blocks of a SeparableSum (csrc/dense_blocks.hip) against the two routes the same problem had before.

Four problems -- 10^4 private blocks of order 64, 10^5 of order 8, 10^3 of order 256, 10^4 of order 64 sharing one matrix -- each as
    packed     SeparableSum of dense Quadratic blocks, the packed lower triangle of G on the device (FOS_DENSE_BLOCKS_SQUARE=0 at set-up)
    square     the same with the full square of G (FOS_DENSE_BLOCKS_SQUARE=1 at set-up); y must have the same bits
    default    the same as the library stores it when nothing is forced: the triangle where it is staged in LDS, the square above
    cg         the same problem as ONE block-diagonal sparse Quadratic(form="cg")
    callback   a numpy object (the stacked inverses, one batched product) through fos_feas_set_callback
    empty      IndBox(-inf, inf): the cost of the step around the prox
Every handle runs AP steps (S1 = the set under test, S2 = IndBox(-inf, inf)) from the same seeded start; a timed call is --steps steps of packed / square / empty
(ONE step of cg and callback) inside one fos_feas_step, which ends in a stream synchronise; host clock; the handles alternate; warm-up first; median, min and max
of --reps repetitions.  prox_us = (step time - empty step time) per step.  bytes = the kept matrices once + x read + d read + y written; its share of 8 TB/s is
bytes / prox time / 8e12 (memory bound: the bytes of G are the cost).  Prints one JSON document.
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

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import __graft_entry__ as ge  # noqa: E402

HBM_BYTES_PER_S = 8e12
CASES = [("1e4 private blocks of order 64", 10 ** 4, 64, False), ("1e5 private blocks of order 8", 10 ** 5, 8, False),
         ("1e3 private blocks of order 256", 10 ** 3, 256, False), ("1e4 blocks of order 64 sharing one matrix", 10 ** 4, 64, True)]


class BatchedQuadratic:
    """prox of sum_k 1/2 x_k'Q_k x_k + q_k'x_k by numpy: the stacked inverses of I + Q_k, one batched product"""

    def __init__(self, Q, q):
        self.inv = np.linalg.inv(np.eye(Q.shape[-1]) + Q)                 # (nb, p, p), or (p, p) when the blocks share their matrix
        self.q = q

    def prox(self, y, x):
        r = x.reshape(self.q.shape) - self.q
        y[:] = (r @ self.inv if self.inv.ndim == 2 else np.einsum("kij,kj->ki", self.inv, r)).reshape(-1)


def problem(nb, p, shared, seed):
    """-> (Q (nb, p, p) or (p, p), q (nb, p)): Q = 0.05 A'A, A standard normal (p + 3) x p, made exactly symmetric"""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((1 if shared else nb, p + 3, p))
    Q = 0.05 * np.matmul(np.transpose(A, (0, 2, 1)), A)
    Q = np.tril(Q) + np.transpose(np.tril(Q, -1), (0, 2, 1))
    return (np.ascontiguousarray(Q[0]) if shared else np.ascontiguousarray(Q)), rng.standard_normal((nb, p))


def timed_us(h, x0, steps):
    h.set_iterate(x0)                                                     # untimed: the same start for every repetition (ends in a synchronise)
    t0 = time.perf_counter()
    h.step(1, steps, 10 ** 9, 1e-30)                                      # fos_feas_step ends in hipStreamSynchronize
    return (time.perf_counter() - t0) * 1e6 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--scale", type=float, default=1.0, help="multiplies the block counts (a rehearsal at a small size)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = ge.load_package()
    free = lambda: pkg.IndBox(-np.inf, np.inf)
    results = []
    for case, (name, nb, p, shared) in enumerate(CASES):
        nb = max(1, int(nb * a.scale))
        n = nb * p
        Q, q = problem(nb, p, shared, case)
        S = pkg.SeparableSum([(pkg.Quadratic(Q if shared else Q[k], q[k]), p) for k in range(nb)], dense=True)
        Qb = sp.bsr_matrix(((np.broadcast_to(Q, (nb, p, p)) if shared else Q), np.arange(nb), np.arange(nb + 1)), shape=(n, n)).tocsc()
        handles, setup_s = {}, {}

        def make(key, S1):
            t0 = time.perf_counter()
            handles[key] = pkg.HipFeasibility(pkg.Feasibility(S1, free(), n))
            setup_s[key] = round(time.perf_counter() - t0, 3)
        for key, force in (("packed", "0"), ("square", "1")):             # (unset, the library keeps the triangle where it is staged in LDS, the square above)
            os.environ["FOS_DENSE_BLOCKS_SQUARE"] = force
            try:
                make(key, S)
            finally:
                del os.environ["FOS_DENSE_BLOCKS_SQUARE"]
        make("default", S)
        make("cg", pkg.Quadratic(Qb, q.reshape(-1), form="cg"))
        make("callback", BatchedQuadratic(Q, q))
        make("empty", free())
        for h in handles.values():
            h.set_alg(pkg.AP())
        x0 = np.random.default_rng(100 + case).standard_normal(n)
        y = {k: handles[k].prox(1, x0) for k in ("packed", "square", "default", "cg", "callback")}
        steps = {"packed": a.steps, "square": a.steps, "default": a.steps, "empty": a.steps, "cg": 1, "callback": 1}
        times = {k: [] for k in handles}
        for rep in range(a.warmup + a.reps):
            for k, h in handles.items():                                  # alternating
                t = timed_us(h, x0, steps[k])
                if rep >= a.warmup:
                    times[k].append(t)
        med = {k: statistics.median(v) for k, v in times.items()}
        st = {k: handles[k].dense_block_stats(1) for k in ("packed", "square")}
        row = {"case": name, "blocks": nb, "order": p, "n": n, "shared_matrix": shared, "reps": a.reps, "steps_per_timed_call": steps,
               "step_us": {k: round(v, 2) for k, v in med.items()}, "step_us_min_max": {k: [round(min(v), 2), round(max(v), 2)] for k, v in times.items()},
               "prox_us": {k: round(med[k] - med["empty"], 2) for k in ("packed", "square", "default", "cg", "callback")},
               "setup_s": setup_s, "stats": st["packed"], "cg_iterations_last_prox": handles["cg"].nspace_cg_stats(1)["last_iters"],
               "square_same_bits_as_packed": y["packed"].tobytes() == y["square"].tobytes() == y["default"].tobytes(),
               "default_storage": "square" if handles["default"].dense_block_stats(1)["matrix_bytes"] == st["square"]["matrix_bytes"] else "packed",
               "max_abs_diff_vs_callback": float(np.abs(y["packed"] - y["callback"]).max()), "max_abs_diff_vs_cg": float(np.abs(y["packed"] - y["cg"]).max())}
        for k in ("packed", "square"):
            nbytes = st[k]["matrix_bytes"] + 3 * 8 * n
            row["bytes_" + k] = nbytes
            row["share_of_8TBps_" + k] = round(nbytes / ((med[k] - med["empty"]) * 1e-6) / HBM_BYTES_PER_S, 4) if med[k] > med["empty"] else None
        row["faster_storage"] = "packed" if med["packed"] <= med["square"] else "square"
        results.append(row)
        print(json.dumps(row), flush=True)
        for h in handles.values():
            h.close()
    doc = {"tool": "tools/dense_blocks_bench.py", "timing": "host clock around one fos_feas_step of `steps_per_timed_call` AP steps (ends in a stream synchronise), per step; "
           "median of `reps` repetitions after warm-up, the handles alternating; prox_us = step - empty step", "hbm_bytes_per_s": HBM_BYTES_PER_S, "results": results}
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
