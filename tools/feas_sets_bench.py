#!/usr/bin/env python
"""Feasibility form: the device projections of csrc/sets.hip against the host-callback path (fos_feas_set_callback) the same sets needed before.

For every set kind, at n = 10^6 as ONE block and as 10^4 blocks of 100, three handles run the same thing in the same process, alternating: ONE step of
AP (S1 = the set under test, S2 = IndBox(-inf, inf)) from the same seeded start, so that every timed projection is of a point outside the set:
    device     S1 projected by the kernels (fos_feas_set_blocks)
    callback   S1 = the numpy reference of tests/set_cases.py through fos_feas_set_callback -- what these sets cost without the kernels
    link       S1 = a callback that only copies (y[:] = x): the floor of ANY host callback, 16 n bytes over the host link and a synchronise
and `empty` (S1 = IndBox(-inf, inf)) is the cost of the step around the projection.  Times are a host clock around fos_feas_step, which ends in a stream
synchronise; the start vector is re-loaded (untimed) before every repetition; warm-up first, median of --reps repetitions.  Prints one JSON document.
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
from set_cases import KINDS, RefSeparableSum, make_set  # noqa: E402

HBM_BYTES_PER_S = 8e12
RESOLUTION_US = 20.0      # the step around a projection takes ~50 us with a spread of a few us


class CopyOnly:
    def prox(self, y, x):
        y[:] = x


def build(pkg, kind, n, nblocks, seed):
    rng = np.random.default_rng(seed)
    length = n // nblocks
    dev, ref = [], []
    for i in range(nblocks):
        r, args, _ = make_set(kind, length, rng, variant=0)
        dev.append((getattr(pkg, kind)(*args), length))
        ref.append((r, length))
    return pkg.SeparableSum(dev), (ref[0][0] if nblocks == 1 else RefSeparableSum(ref))


def one_step_us(h, x0):
    h.set_iterate(x0)                                       # untimed: the same start for every repetition (ends in a synchronise)
    t0 = time.perf_counter()
    h.step(1, 1, 10 ** 9, 1e-30)                            # fos_feas_step ends in hipStreamSynchronize
    return (time.perf_counter() - t0) * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10 ** 6)
    ap.add_argument("--blocks", type=int, default=10 ** 4)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kinds", default=",".join(KINDS))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = ge.load_package()
    n = a.n
    free = lambda: pkg.IndBox(-np.inf, np.inf)
    x0 = np.random.default_rng(0).standard_normal(n)
    results = []
    for kind in a.kinds.split(","):
        for nblocks in (1, a.blocks):
            S, ref = build(pkg, kind, n, nblocks, seed=nblocks)
            handles = {"device": pkg.HipFeasibility(pkg.Feasibility(S, free(), n)), "callback": pkg.HipFeasibility(pkg.Feasibility(ref, free(), n)),
                       "link": pkg.HipFeasibility(pkg.Feasibility(CopyOnly(), free(), n)), "empty": pkg.HipFeasibility(pkg.Feasibility(free(), free(), n))}
            for h in handles.values():
                h.set_alg(pkg.AP())
            y_dev, y_ref = handles["device"].prox(1, x0), handles["callback"].prox(1, x0)
            times = {k: [] for k in handles}
            for rep in range(a.warmup + a.reps):
                for k, h in handles.items():                # alternating
                    t = one_step_us(h, x0)
                    if rep >= a.warmup:
                        times[k].append(t)
            st = handles["device"].set_stats(1)
            med = {k: statistics.median(v) for k, v in times.items()}
            row = {"kind": kind, "n": n, "blocks": nblocks, "reps": a.reps, "max_abs_diff_vs_reference": float(np.abs(y_dev - y_ref).max()),
                   "step_us": {k: round(v, 1) for k, v in med.items()}, "step_us_min_max": {k: [round(min(v), 1), round(max(v), 1)] for k, v in times.items()},
                   "projection_us": {k: round(med[k] - med["empty"], 1) for k in ("device", "callback", "link")},
                   "device_faster_than_callback": med["device"] < med["callback"], "device_faster_than_link_floor": med["device"] < med["link"],
                   "launches": st["launches"], "threshold_passes": st["last_passes"]}
            if st["grid_blocks"]:                           # information only: x read once per pass and by the reduction, y written once, the vector read twice
                scalar = kind in ("IndBallL2", "IndHalfspace", "IndHyperslab")
                reads = st["last_passes"] + (2 if kind in ("IndSimplex", "IndBallL1") or scalar else 1) + (2 if scalar else 1 if kind == "IndPoint" else 0)
                row["grid_class_bytes"] = 8 * n * (reads + 1)
                # the projection's own time is a difference of two step times: below RESOLUTION_US it is inside their spread and no rate is derived from it
                proj_us = med["device"] - med["empty"]
                row["grid_class_share_of_8TBps"] = round(row["grid_class_bytes"] / (proj_us * 1e-6) / HBM_BYTES_PER_S, 4) if proj_us >= RESOLUTION_US else None
            results.append(row)
            print(json.dumps(row), flush=True)
            for h in handles.values():
                h.close()
    doc = {"tool": "tools/feas_sets_bench.py", "timing": "host clock around one fos_feas_step (ends in a stream synchronise)",
           "results": results, "all_faster_than_callback": all(r["device_faster_than_callback"] for r in results)}
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(doc, indent=1) + "\n")
    print(json.dumps({"all_faster_than_callback": doc["all_faster_than_callback"], "cases": len(results)}))


if __name__ == "__main__":
    main()
