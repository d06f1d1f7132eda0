"""Bit identity of the sparse sets of the Feasibility form across two builds with the same ABI (the other build through FOSHIP_LIB).

    python tools/feas_sparse_identity.py > new.jsonl                                          (device)
    FOSHIP_LIB=<parent>/libfoship.so python tools/feas_sparse_identity.py > parent1.jsonl
    python tools/feas_sparse_identity.py --host > host_new.jsonl                              (no GPU: the fos_host_* emulations)
    python tools/feas_sparse_identity.py --compare parent1.jsonl parent2.jsonl new.jsonl

The five objects: sparse IndAffine by CG, sparse factored IndAffine, sparse factored LeastSquares, sparse normal LeastSquares, Quadratic / LeastSquares by CG; two or
three small instances each from tests/sparse_factored_cases.py, tests/nspace_cases.py, tests/nspace_cg_cases.py and the generator of tests/test_gpu_sparse_affine.py,
among them rows that are cut (FOS_SF_SEG=64; a 3 000-entry row under the CG forms' 2 048) and a zero row where the object allows one.
One JSON record per case.  Device: the SHA-256 of three proxes (cold, warm at the same x, warm at a perturbed x), of the iterate after 30 DR steps against
IndBox(0, inf), and the object's statistics (iterations, restarts, launches, plan fields) after each.  --host: the SHA-256 of the emulation's prox at both points and
its iteration count (the CG form of IndAffine has no emulation: no record).
--compare: the first two files are two runs of the parent and must be equal before anything is said about the third; every record of every file must equal the first's.
"""
import base64
import hashlib
import json
import os
import sys
from pathlib import Path

import numpy as np
import scipy.sparse as sp

HERE = Path(__file__).resolve().parent.parent
STEPS = 30
LAM = 0.7


def sha(a):
    return base64.b64encode(hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).digest()).decode().rstrip("=")


def plain(v):
    if isinstance(v, dict):
        return {k: plain(x) for k, x in v.items()}
    if isinstance(v, (tuple, list, np.ndarray)):
        return [plain(x) for x in v]
    v = v.item() if isinstance(v, np.generic) else v
    return repr(v) if isinstance(v, float) else v                 # (a float keeps its bits through repr)


def cases(pkg):
    """-> (name, kind, matrix, vector, environment)"""
    import nspace_cases as nc
    import nspace_cg_cases as cg
    import sparse_factored_cases as sf
    from test_gpu_sparse_affine import sparse_instance
    for m, n, per_row in [(300, 1000, 6), (40, 5000, 300), (1, 50, 7)]:
        yield ("affine_cg/%dx%d" % (m, n), "affine_cg") + sparse_instance(m + n, m, n, per_row) + ({},)
    yield ("affine_factored/rand65x131", "affine_factored") + sf.rand(65, 131, 4) + ({},)
    yield ("affine_factored/rand300x1000", "affine_factored") + sf.rand(300, 1000, 6) + ({},)
    for name, (A, b) in sf.seg64_cases().items():
        yield ("affine_factored/seg64_" + name, "affine_factored", A, b, {"FOS_SF_SEG": "64"})
    yield ("ls_factored/rand64x640", "ls_factored") + sf.rand(64, 640, 5) + ({},)
    A, b = sf.seg64_cases()["skew"]
    Z = sp.lil_matrix(A); Z[5, :] = 0.0                                               # a zero row beside the rows that are cut
    yield ("ls_factored/seg64_skew_zero_row", "ls_factored", sp.csc_matrix(Z), b, {"FOS_SF_SEG": "64"})
    yield ("ls_normal/tall330x65", "ls_normal") + nc.tall_sparse(330, 65, 3) + ({},)
    for name in ("zero_row", "zero_col", "7x9"):
        A, b, _ = cg.ls_case(name)
        yield ("ls_normal/" + name, "ls_normal", A, b, {})
    for name in ("n65", "tridiag300", "arrow3000", "empty_rows"):
        Q, q, _ = cg.quadratic_case(name)
        yield ("quadratic_cg/" + name, "quadratic_cg", Q, q, {})
    for name in ("9x7", "zero_row", "tall5000x40", "dense_col3000"):
        A, b, _ = cg.ls_case(name)
        yield ("ls_cg/" + name, "ls_cg", A, b, {})


def make_set(pkg, kind, M, v):
    if kind == "affine_cg":
        return pkg.IndAffine(M, v), "affine_stats"
    if kind == "affine_factored":
        return pkg.IndAffine(M, v, form="sparse_factored", refine=1), "affine_sparse_factored_stats"
    if kind == "ls_factored":
        return pkg.LeastSquares(M, v, LAM, form="sparse_factored"), "affine_sparse_factored_stats"
    if kind == "ls_normal":
        return pkg.LeastSquares(M, v, LAM, form="normal"), "nspace_stats"
    if kind == "quadratic_cg":
        return pkg.Quadratic(M, v, form="cg"), "nspace_cg_stats"
    return pkg.LeastSquares(M, v, LAM, form="cg"), "nspace_cg_stats"


def points(n):
    rng = np.random.default_rng(n)
    x = rng.standard_normal(n)
    return x, x + 1e-3 * rng.standard_normal(n)


def device_record(pkg, kind, M, v):
    n = M.shape[1]
    S, stats = make_set(pkg, kind, M, v)
    d = pkg.HipFeasibility(pkg.Feasibility(S, pkg.IndBox(0.0, np.inf), n))
    x, x2 = points(n)
    rec = {"prox": [], "stats": []}
    for p in (x, x, x2):
        rec["prox"].append(sha(d.prox(1, p)))
        rec["stats"].append(plain(getattr(d, stats)(1)))
    d.set_alg(pkg.DR())
    d.set_iterate(None)
    d.step(1, STEPS, 10 ** 9, 1e-30)
    rec["dr%d" % STEPS] = sha(d.get_iterate())
    rec["stats"].append(plain(getattr(d, stats)(1)))
    d.close()
    return rec


def host_record(pkg, kind, M, v):
    import nspace_cases as nc
    import nspace_cg_cases as cg
    import sparse_factored_cases as sf
    if kind == "affine_cg":
        return None
    rec = {"prox": [], "iterations": []}
    for p in points(M.shape[1]):
        it = None
        if kind == "affine_factored":
            rc, y = sf.host_project(pkg, M, v, 1, p)
        elif kind in ("ls_factored", "ls_normal"):
            rc, y = nc.host_ls_sparse(pkg, M, v, LAM, "sparse_factored" if kind == "ls_factored" else "normal", p)
        elif kind == "quadratic_cg":
            rc, y, it = cg.host_quadratic_cg(pkg, M, v, p)
        else:
            rc, y, it = cg.host_ls_cg(pkg, M, v, LAM, p)
        pkg.lib.check(rc)
        rec["prox"].append(sha(y))
        rec["iterations"].append(it)
    return rec


def run(host):
    sys.path.insert(0, str(HERE / "tests"))
    sys.path.insert(0, str(HERE))
    import __graft_entry__ as ge
    pkg = ge.load_package()
    for name, kind, M, v, env in cases(pkg):
        os.environ.update(env)                                     # (read at every set-up)
        try:
            rec = (host_record if host else device_record)(pkg, kind, sp.csc_matrix(M), np.asarray(v, dtype=np.float64))
        finally:
            for k in env:
                del os.environ[k]
        if rec is not None:
            print(json.dumps(dict(case=name, **rec), separators=(",", ":")), flush=True)


def compare(files):
    load = lambda f: {r["case"]: r for r in map(json.loads, filter(str.strip, Path(f).read_text().splitlines()))}
    base, bad = load(files[0]), 0
    for other in files[1:]:
        got = load(other)
        diff = [c for c in sorted(set(base) | set(got)) if got.get(c) != base.get(c)]
        for c in diff:
            a, b = base.get(c, {}), got.get(c, {})
            print("DIFFER %s: %s" % (c, [k for k in sorted(set(a) | set(b)) if a.get(k) != b.get(k)]))
        bad += len(diff)
    print("%s: %d records each, %s" % (" = ".join(Path(f).name for f in files), len(base),
                                      "every field and digest equal" if not bad else "%d records DIFFER" % bad))
    return bad


if __name__ == "__main__":
    args = sys.argv[1:]
    if args[:1] == ["--compare"]:
        sys.exit(1 if compare(args[1:]) else 0)
    run("--host" in args)
