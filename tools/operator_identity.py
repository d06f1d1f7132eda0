"""Bit identity of the stacked operator's set-up across two builds of the library (FOSHIP_LIB=... selects the build, as tools/ab_bench.sh does).

    python tools/operator_identity.py > new.jsonl
    FOSHIP_LIB=.../libfoship_ab.so python tools/operator_identity.py > parent1.jsonl
    python tools/operator_identity.py --compare parent1.jsonl parent2.jsonl new.jsonl

Public Python API only.  One JSON record per case: operator_stats(), resident_stats(), cg_variant_name() and the SHA-256 of the raw fp64 results of
q_apply (both transposes), kkt_apply and the fields of check() on seeded vectors -- as the handle is built, and again after
set_tuning(spmv_workgroups=w) for w = 8, 64, 1000.  No CG solve goes into a digest: a solve ends on a host-observed stop.

Cases: every shape of status_cases.row_block_shapes() as the library stores it by itself; every window_shapes() entry under FOS_WINDOWS = 1 and 2;
row_sharded=True handles, single rank and no transport opened, on the instances of tests/test_gpu_peer_mailbox.py (without tiles: its "mixed" rows
problem; with tiles: its "dense" rows problem and its "sdp-tiles" problem; stored as window panels: its "mixed" rows problem under FOS_WINDOWS = 1 and 2); one handle with equilibrate=2.
--compare: every field and digest of the first file against each of the others.
"""
import hashlib
import json
import os
import sys
from pathlib import Path

import numpy as np
import scipy.sparse as sp

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "oracle"))
sys.path.insert(0, str(ROOT))

WORKGROUPS = (8, 64, 1000)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).hexdigest()


def digests(d, seed):
    rng = np.random.default_rng(seed)
    x, z = rng.standard_normal(d.l), rng.standard_normal(d.N)
    z[d.l - 1], z[d.N - 1] = 1.0 + rng.random(), rng.random()
    res = d.check(z, 1e-6)
    fields = [float(getattr(res, name)) for name, _ in res._fields_]
    return dict(q=sha(d.q_apply(x)), qt=sha(d.q_apply(x, transpose=True)), kkt=sha(d.kkt_apply(z)), check=sha(fields))


def record(name, make, seed, windows=None):
    os.environ.pop("FOS_WINDOWS", None)
    if windows:
        os.environ["FOS_WINDOWS"] = windows
    try:
        d = make()
    finally:
        os.environ.pop("FOS_WINDOWS", None)
    rec = dict(case=name, operator_stats=d.operator_stats(), resident_stats=d.resident_stats(), cg_variant=d.cg_variant_name(), built=digests(d, seed))
    for w in WORKGROUPS:
        d.set_tuning(spmv_workgroups=w)
        rec["wg%d" % w] = dict(digests(d, seed), waves=d.operator_stats()["waves"])
    d.close()
    print(json.dumps(rec), flush=True)


def run():
    import __graft_entry__ as ge
    import status_cases as cases
    import test_gpu_peer_mailbox as pm
    pkg = ge.load_package()

    def plain(name, A, **kw):
        A = sp.csc_matrix(A)
        m, n = A.shape
        b, c = cases.vectors_for(name, A)
        return lambda: pkg.HipHSDE(A, b, c, [("Free", m)], [("Free", n)], **kw)

    shapes = cases.row_block_shapes()
    for name, A in shapes:
        record(name, plain(name, A), cases._seed("identity", name))
    for name, A in cases.window_shapes():
        for geom in ("1", "2"):
            record("%s/FOS_WINDOWS=%s" % (name, geom), plain(name, A), cases._seed("identity", name, geom), windows=geom)
    for name, prob in (("rows-mixed", pm._rows_problem(pkg, "mixed")), ("rows-dense", pm._rows_problem(pkg, "dense")), ("sdp-tiles", pm._problem(pkg, "sdp-tiles"))):
        sharded = lambda p=prob: pkg.HipHSDE(p.A, p.b, p.c, p.K1, p.K2, row_sharded=True)
        record(name + "/row_sharded", sharded, cases._seed("identity", name))
        for geom in ("1", "2") if name == "rows-mixed" else ():
            record("%s/row_sharded/FOS_WINDOWS=%s" % (name, geom), sharded, cases._seed("identity", name, geom), windows=geom)
    name, A = next((nm, M) for nm, M in shapes if nm == "tile-mixed")
    record(name + "/equilibrate=2", plain(name, A, equilibrate=2), cases._seed("identity", name, "eq"))


def compare(files):
    load = lambda f: {r["case"]: r for r in map(json.loads, filter(str.strip, Path(f).read_text().splitlines()))}
    base, bad = load(files[0]), 0
    for other in files[1:]:
        got = load(other)
        diff = [c for c in base if got.get(c) != base[c]] + [c for c in got if c not in base]
        for c in diff:
            a, b = base.get(c, {}), got.get(c, {})
            print("DIFFER %s: %s" % (c, [k for k in sorted(set(a) | set(b)) if a.get(k) != b.get(k)]))
        print("%s vs %s: %d cases, %s" % (files[0], other, len(base), "every field and digest equal" if not diff else "%d DIFFER" % len(diff)))
        bad += len(diff)
    return bad


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--compare":
        sys.exit(1 if compare(sys.argv[2:]) else 0)
    run()
