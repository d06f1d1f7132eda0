"""direct = true: per-projection time of the cg, dense and reduced forms, set-up time, bytes read per projection and the break-even number of projections.

    python tools/direct_reduced_bench.py [--problem C3|c2_lp] [--reps 30] [--timeout 600] [--factor newton|cholesky|both]   -> one JSON object

--factor: how the stored inverse of the reduced and the dense form is built.  With `both` one child sets the same handle up with Newton-Schulz and then with the
blocked Cholesky factorisation (one process, one device): set-up seconds, the seconds of the inversion stage alone, the per-projection time, the certificate
on_set + in_range of one projection and the break-even number of projections are reported per factor, with the ratio of the two inversion stages.

Every form runs in a child process of its own under its own time limit; after a child that failed nothing more is started.  A projection is timed through
fos_prox_affine (host -> device -> host, the same on every form) on a fixed sequence of independent random inputs, so that the cg form's warm start is worth
what it is worth between unrelated inputs; the first projection (code objects) is left out.  tests/test_gpu_direct_reduced.py uses time_projections too."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def time_projections(d, reps, seed=0):
    """seconds of each of `reps` projections of independent random inputs on handle d (one unmeasured projection first)"""
    rng = np.random.default_rng(seed)
    d.prox_affine(rng.standard_normal(d.N))
    out = []
    for _ in range(reps):
        x = rng.standard_normal(d.N)
        t = time.perf_counter()
        d.prox_affine(x)
        out.append(time.perf_counter() - t)
    return out


def bytes_per_projection(form, m, n, nnz):
    """bytes of the stored inverse one projection reads (the sweeps over A come on top: 12 bytes per stored entry and sweep)"""
    l, k = n + m + 1, min(m, n)
    nt = (k + 63) // 64
    return {"dense": 8 * l * l, "reduced": nt * (nt + 1) * 64 * 32 * 8, "cg": 0}[form]


def problem(pkg, name):
    if name == "C3":
        return pkg.workloads.c3_socp()
    if name == "c2_lp":
        return pkg.workloads.c2_lp(m=5000, n=10000)
    raise SystemExit("unknown problem " + name)


def certificate(d, seed=1):
    """(|Q u - v| + |(x - y)_u - Q'(y - x)_v|) / |x| of one projection y = (u, v) of a random x: on the set, and x - y in the range of [Q -I]'"""
    x = np.random.default_rng(seed).standard_normal(d.N)
    y = d.prox_affine(x)
    l = d.l
    on_set = np.linalg.norm(d.q_apply(y[:l]) - y[l:])
    in_range = np.linalg.norm((x[:l] - y[:l]) - d.q_apply(y[l:] - x[l:], transpose=True))
    return float((on_set + in_range) / np.linalg.norm(x))


def child(name, form, reps, factors):
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    pkg = ge.load_package()
    prob = problem(pkg, name)
    m, n = prob.A.shape
    if form in ("cg", "dense"):
        os.environ["FOS_DIRECT_MODE"] = form
    d = pkg.HipHSDE(prob.A, prob.b, prob.c, prob.K1, prob.K2)
    runs = {}
    for factor in (factors if form in ("reduced", "dense") else ["newton"]):
        t = time.perf_counter()
        d.enable_direct(prob.A, form="reduced" if form == "reduced" else "auto", factor=factor)
        wall = time.perf_counter() - t
        assert d.direct_mode() == form, (d.direct_mode(), form)
        ts = time_projections(d, reps)
        cg = d.cgiter()
        st = d.direct_stats()
        runs[factor] = {"form": form, "m": m, "n": n, "nnz": int(prob.A.nnz), "setup_s": wall, "ns_steps": st["ns_steps"], "k": st["k"],
                        "factor": st["factor"], "invert_s": st["invert_s"], "probe_resid": st["probe_resid"], "fell_back": st["fell_back"],
                        "projection_ms_median": 1e3 * float(np.median(ts)), "projection_ms_min": 1e3 * float(np.min(ts)), "cg_iterations_last": cg,
                        "certificate": certificate(d), "inverse_bytes_per_projection": bytes_per_projection(form, m, n, int(prob.A.nnz))}
    d.close()
    first = dict(runs[next(iter(runs))])
    if len(runs) > 1:
        first["factors"] = runs
    print(json.dumps(first))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problem", default="C3")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--timeout", type=int, default=600)
    ap.add_argument("--factor", default="newton", choices=["newton", "cholesky", "both"])
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    factors = ["newton", "cholesky"] if a.factor == "both" else [a.factor]
    if a.child:
        return child(a.problem, a.child, a.reps, factors)
    forms = ["cg", "reduced"] + (["dense"] if a.problem != "C3" else [])       # (C3: l = 70 001 is past the dense form)
    res = {}
    for form in forms:
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--problem", a.problem, "--reps", str(a.reps),
               "--factor", a.factor, "--child", form]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:
            res[form] = {"failed": r.returncode}
            print(json.dumps({"problem": a.problem, "forms": res, "stopped_after": form}, indent=1))
            return 1
        res[form] = json.loads(r.stdout.strip().splitlines()[-1])
    out = {"problem": a.problem, "factor": a.factor, "forms": res}
    if "cg" in res and "reduced" in res:
        gain = (res["cg"]["projection_ms_median"] - res["reduced"]["projection_ms_median"]) * 1e-3
        out["reduced_over_cg"] = res["reduced"]["projection_ms_median"] / res["cg"]["projection_ms_median"]
        out["break_even_projections"] = (res["reduced"]["setup_s"] / gain) if gain > 0 else None
    for form in ("reduced", "dense"):                                          # per factor: break-even against cg, and Newton-Schulz over Cholesky
        runs = res.get(form, {}).get("factors")
        if not runs:
            continue
        cmp = {}
        for factor, r in runs.items():
            gain = (res["cg"]["projection_ms_median"] - r["projection_ms_median"]) * 1e-3
            cmp["break_even_projections_" + factor] = (r["setup_s"] / gain) if gain > 0 else None
        cmp["invert_newton_over_cholesky"] = runs["newton"]["invert_s"] / runs["cholesky"]["invert_s"]
        cmp["setup_newton_over_cholesky"] = runs["newton"]["setup_s"] / runs["cholesky"]["setup_s"]
        out[form + "_factors"] = cmp
    print(json.dumps(out, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
