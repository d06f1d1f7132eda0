#!/usr/bin/env python
"""Opt-in equilibration (fos_create3, HipHSDE(..., equilibrate=10)) against the problem as given, on the MI355X.

Workloads: C4 as the survey writes it (scale = 1), C4 conditioned by hand (the BASELINE instance), C2, mid_mixed, and mid_mixed with rows and columns multiplied
by 10^U(-2, 2) (tests/equilibrate_cases.py badly_scaled).  Per workload and per handle (plain, equilibrated):

    setup_s             wall seconds of HipHSDE(...): for the equilibrated handle this includes the host scaling
    solve               DR(0.5) from the handle's standard start, a check every --checki iterations at eps = --eps, at most --max-iters iterations or --max-solve-s seconds:
                        status, iterations, CG iterations per step over the whole solve, wall seconds
    ms_per_step         from the standard start, after --warmup steps: the two handles alternate blocks of --block steps without a check; a host clock around
                        fos_step (which ends in a stream synchronise); median of --reps blocks, per step; the CG iterations per step of the timed blocks beside it
    us_per_check        a host clock around fos_check on the current iterate (upload of z, the check, one poll of the device state), median of --reps

Nothing here is asserted: the numbers are recorded.  Writes one JSON document (--out)."""
import argparse
import ctypes
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import __graft_entry__ as ge  # noqa: E402
import equilibrate_cases as ec  # noqa: E402

PASSES = 10


def workloads(pkg, names):
    w = pkg.workloads
    table = {
        "C4_as_specified": lambda: w.c4_block_sdp(scale=1.0),
        "C4_conditioned": lambda: w.c4_block_sdp(),
        "C2": lambda: w.c2_lp(),
        "mid_mixed": lambda: w.mid_mixed(),
        "mid_mixed_badly_scaled": lambda: ec.badly_scaled(w.mid_mixed(), 1),
        "small_mixed_badly_scaled": lambda: ec.badly_scaled(w.small_mixed(), 1),       # (the tests' case; not in the default list)
    }
    return [(n, table[n]) for n in names]


def solve(pkg, dev, a):
    dev.set_alg(pkg.DR())
    dev.reset_affine()
    dev.set_iterate(None)
    cg0, t0, i, status = dev.cg_total(), time.perf_counter(), 0, "Continue"
    res = None
    while i < a.max_iters and status == "Continue" and time.perf_counter() - t0 < a.max_solve_s:
        done, checked, res = dev.step(i + 1, min(a.checki, a.max_iters - i), a.checki, a.eps)
        i += done
        if checked:
            status = pkg.lib.STATUS_NAMES[res.status]
    out = {"status": status if status != "Continue" else ("not optimal at %d iterations" % i), "iterations": i, "cg_per_step": round((dev.cg_total() - cg0) / max(i, 1), 2),
           "wall_s": round(time.perf_counter() - t0, 3)}
    if res is not None:
        out["last_check"] = {k: (v if v == v else None) for k, v in (("p", res.p), ("d", res.d), ("g", res.g))}       # (NaN: a diverged plain solve; null in JSON)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="C4_as_specified,C4_conditioned,C2,mid_mixed,mid_mixed_badly_scaled")
    ap.add_argument("--eps", type=float, default=1e-5)
    ap.add_argument("--checki", type=int, default=50)
    ap.add_argument("--max-iters", type=int, default=5000)
    ap.add_argument("--max-solve-s", type=float, default=150.0, help="a solve also stops (between checks) after this many wall seconds")
    ap.add_argument("--warmup", type=int, default=60)
    ap.add_argument("--block", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "equilibrate_bench.json"))
    a = ap.parse_args()
    assert a.reps >= 5
    pkg = ge.load_package()
    buf = ctypes.create_string_buffer(128)
    pkg.lib.check(pkg.lib.load().fos_device_name(0, buf, 128))
    device = buf.value.decode()
    results = []

    def write():
        doc = {"tool": "tools/equilibrate_bench.py", "device": device, "passes": PASSES, "eps": a.eps, "checki": a.checki,
               "max_iters": a.max_iters, "timing": "host clock around fos_step / fos_check (both end in a synchronise); ms_per_step: median of %d blocks of %d steps "
               "after %d warm-up steps, the two handles alternating" % (a.reps, a.block, a.warmup), "results": results}
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(doc, indent=1) + "\n")

    for name, make in workloads(pkg, a.workloads.split(",")):
        t0 = time.perf_counter()
        prob = make()
        row = {"workload": name, "m": prob.m, "n": prob.n, "nnz": prob.nnz, "generate_s": round(time.perf_counter() - t0, 2)}
        print("%s: m = %d, n = %d, nnz = %d" % (name, prob.m, prob.n, prob.nnz), flush=True)
        handles = {}
        for key, passes in (("plain", 0), ("equilibrated", PASSES)):
            t0 = time.perf_counter()
            handles[key] = pkg.HipHSDE(prob.A, prob.b, prob.c, prob.K1, prob.K2, equilibrate=passes)
            row[key] = {"setup_s": round(time.perf_counter() - t0, 3)}
        eq = handles["equilibrated"].equilibration()
        row["scaling"] = {"sigma": eq["sigma"], "rho": eq["rho"], "gamma": eq["gamma"], "D_min_max": [float(eq["D"].min()), float(eq["D"].max())],
                          "E_min_max": [float(eq["E"].min()), float(eq["E"].max())]}
        for key, dev in handles.items():
            row[key]["solve"] = solve(pkg, dev, a)
            print("  %-12s %s" % (key, json.dumps(row[key]["solve"])), flush=True)
        # steady-state step time: both from their standard start, alternating blocks
        step_ms = {k: [] for k in handles}
        cg = {}
        at = {}
        for key, dev in handles.items():
            dev.set_alg(pkg.DR())
            dev.reset_affine()
            dev.set_iterate(None)
            dev.step(1, a.warmup, 10 ** 9, a.eps)
            at[key], cg[key] = a.warmup, dev.cg_total()
        for _ in range(a.reps):
            for key, dev in handles.items():
                t0 = time.perf_counter()
                dev.step(at[key] + 1, a.block, 10 ** 9, a.eps)
                step_ms[key].append((time.perf_counter() - t0) * 1e3 / a.block)
                at[key] += a.block
        check_us = {k: [] for k in handles}
        for _ in range(a.reps + 2):
            for key, dev in handles.items():
                z = dev.get_iterate()
                t0 = time.perf_counter()
                dev.check(z, a.eps)
                check_us[key].append((time.perf_counter() - t0) * 1e6)
        for key, dev in handles.items():
            row[key]["ms_per_step"] = round(statistics.median(step_ms[key]), 4)
            row[key]["ms_per_step_min_max"] = [round(min(step_ms[key]), 4), round(max(step_ms[key]), 4)]
            row[key]["cg_per_step_timed"] = round((dev.cg_total() - cg[key]) / (a.reps * a.block), 2)
            row[key]["us_per_check"] = round(statistics.median(check_us[key][2:]), 1)
            dev.close()
        results.append(row)
        print("  " + json.dumps({k: {f: row[k][f] for f in ("setup_s", "ms_per_step", "cg_per_step_timed", "us_per_check")} for k in handles}), flush=True)
        write()


if __name__ == "__main__":
    main()
