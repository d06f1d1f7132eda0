"""Bit identity of the CG solve behind prox_affine across two builds (csrc/cg.cpp against the solve as solver.cpp held it).

    python tools/cg_identity.py [--kept new.npz] > new.jsonl
    python tools/cg_identity.py --tree <parent checkout> [--kept parent1.npz] > parent1.jsonl
    python tools/cg_identity.py --compare parent1.jsonl parent2.jsonl new.jsonl

Public Python API only (of the package of --tree: a build with another ABI brings its own mirror).  One JSON record per case.

"cg/<operator>[-win<g>]/<variant>/chunk<c>": every operator of tests/cg_cases.py (the row-block shapes as the library stores them, the window shapes under
FOS_WINDOWS = 1 and 2) on its tamed warm start; every variant the handle accepts (reference, fused_p off window panels, merged_sweep, merged_update, resident
where resident_stats() says the operator qualifies); cg_chunk 1 and 8.  After set_cg_variant, set_tuning(cg_chunk) and reset_affine: the SHA-256 and count of
cg_kkt at the case's decisive tolerance for k = 3 and at max_iters = 2, the digests of the two prox_affine calls of cg_cases.prox_sequence (the second sizes
its first batch by the first's count), cg_variant_name() and cg_total().
"steps/<alg>/<mode>": workloads.small_mixed() without direct, 12 steps of DR and of GAPA under profile(1): the digest of get_iterate() after every step and
the launch counts of profile_read_classes() (not its times); modes: FOS_SPECULATE unset, FOS_SPECULATE=0 (set before the handle is created), and behind a
one-rank host collective (comm_init_host with the identity: every sum passes the reduce kernel and the all-reduce).
--kept FILE also saves the hashed vectors (those of at most 100 000 entries), an .npz beside the records, not for the history.
--compare: the first two files are two runs of the parent.  Where they agree bit for bit the third must agree with them in every field; where they do not (a
solve ends on a host-observed stop) the kept vectors are compared at the project's same-step tolerance, 1e-9 relative, and the output says so.
"""
import base64
import hashlib
import json
import os
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent.parent
STEPS = 12
TOL = 1e-9
KEEP_MAX = 100000
KEPT = {}


def sha(key, a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.size <= KEEP_MAX:
        KEPT[key] = a.copy()
    return base64.b64encode(hashlib.sha256(a.tobytes()).digest()).decode().rstrip("=")


def load_pkg(tree):
    sys.path[:0] = [str(tree), str(HERE / "tests"), str(HERE / "oracle")]      # (the instances: the same in every checkout compared)
    import __graft_entry__ as ge
    return ge.load_package()


def cg_records(pkg):
    import cg_cases as cases
    import cg_reference as cref
    ops = [(name, None) for name in cases.row_names()] + [(name, g) for g in ("1", "2") for name in cases.window_names()]
    for name, geom in ops:
        A, b, c = cases.scaled_operator(name)
        os.environ.pop("FOS_WINDOWS", None)
        if geom:
            os.environ["FOS_WINDOWS"] = geom
        try:
            d = pkg.HipHSDE(A, b, c, [("Free", A.shape[0])], [("Free", A.shape[1])])
        finally:
            os.environ.pop("FOS_WINDOWS", None)
        cs, prox = cases.case(name, "warm"), cases.prox_sequence(name)
        tol3 = cref.decisive_tol(cs, 3)
        variants = ["reference"] + (["fused_p"] if d.operator_stats()["win_panels"] == 0 else []) + ["merged_sweep", "merged_update"]
        variants += ["resident"] if d.resident_stats()["qualifies"] else []
        for variant in variants:
            for chunk in (1, 8):
                case = "cg/%s%s/%s/chunk%d" % (name, "-win" + geom if geom else "", variant, chunk)
                d.set_cg_variant(variant)
                d.set_tuning(cg_chunk=chunk)
                d.reset_affine()
                rec = dict(case=case)
                for what, tol, cap in (("tol3", tol3, 10000), ("cap2", 1e-300, 2)):
                    x, it = d.cg_kkt(cs.x0, cs.rhs, tol, cap)
                    rec[what] = [sha(case + "@" + what, x), int(it)]
                rec["prox"] = [sha("%s@prox%d" % (case, q), d.prox_affine(x)) for q, (x, _, _, _) in enumerate(prox)]
                rec["variant"], rec["cg_total"] = d.cg_variant_name(), int(d.cg_total())
                yield rec
        d.close()


def step_records(pkg):
    prob = pkg.workloads.small_mixed()
    for mode in ("speculate", "FOS_SPECULATE=0", "host-collective"):
        os.environ.pop("FOS_SPECULATE", None)
        if mode == "FOS_SPECULATE=0":
            os.environ["FOS_SPECULATE"] = "0"
        try:
            for algname, alg in (("DR", pkg.DR()), ("GAPA", pkg.GAPA(0.8, 0.5))):
                case = "steps/%s/%s" % (algname, mode)
                d = pkg.HipHSDE(prob.A, prob.b, prob.c, prob.K1, prob.K2)
                if mode == "host-collective":
                    d.comm_init_host(1, 0, lambda a: None)
                d.set_alg(alg)
                d.set_iterate(None)
                d.profile(1)
                its = []
                for i in range(1, STEPS + 1):
                    d.step(i, 1, 10 ** 9, 1e-30)
                    its.append(sha("%s@%d" % (case, i), d.get_iterate()))
                counts = {k: int(v[0]) for k, v in d.profile_read_classes().items()}
                yield dict(case=case, iterates=its, launches=counts, variant=d.cg_variant_name(), cg_total=int(d.cg_total()))
                d.close()
        finally:
            os.environ.pop("FOS_SPECULATE", None)


def run(tree, kept_file):
    pkg = load_pkg(tree)
    for records in (cg_records, step_records):
        for rec in records(pkg):
            print(json.dumps(rec, separators=(",", ":")), flush=True)
    if kept_file:
        np.savez(kept_file, **KEPT)


def compare(files):
    load = lambda f: {r["case"]: r for r in map(json.loads, filter(str.strip, Path(f).read_text().splitlines()))}
    p1, p2, new = (load(f) for f in files)
    npz = [Path(f).with_suffix(".npz") for f in files]
    kept = [np.load(f) for f in npz] if all(f.exists() for f in npz) else None
    bad = agree = 0
    for c in p1:
        if c not in new or c not in p2:
            print("MISSING %s" % c)
            bad += 1
        elif p1[c] == p2[c]:
            agree += 1
            if new[c] != p1[c]:
                print("DIFFER %s: %s" % (c, [k for k in sorted(set(p1[c]) | set(new[c])) if p1[c].get(k) != new[c].get(k)]))
                bad += 1
        else:
            keys = [k for k in (kept[0].files if kept else ()) if k.startswith(c + "@")]
            if not keys or any(k not in kept[2].files for k in keys):
                print("%s: the two parent runs do NOT agree bit for bit and the vectors were not kept" % c)
                bad += 1
                continue
            rel = lambda k: max(float(np.linalg.norm(k[key] - kept[0][key]) / max(np.linalg.norm(kept[0][key]), 1e-300)) for key in keys)
            wp, wn = rel(kept[1]), rel(kept[2])
            counts = all(p1[c].get(k) == new[c].get(k) for k in ("launches", "variant", "cg_total"))
            print("%s: the two parent runs do NOT agree bit for bit (a CG solve ends on a host-observed stop); largest |x - x_parent1| / |x_parent1|: parent2 %.2e, "
                  "new %.2e (tolerance %.0e): %s; counts %s" % (c, wp, wn, TOL, "within" if wn <= TOL else "OUTSIDE", "equal" if counts else "DIFFER"))
            bad += not (wn <= TOL and counts)
    bad += sum(1 for c in new if c not in p1)
    print("%d cases; the two parent runs agree bit for bit on %d; the new build %s" % (len(p1), agree, "agrees with the parent on every case" if not bad else "FAILS on %d" % bad))
    return bad


if __name__ == "__main__":
    args = sys.argv[1:]
    if args[:1] == ["--compare"]:
        sys.exit(1 if compare(args[1:4]) else 0)
    tree = Path(args[args.index("--tree") + 1]).resolve() if "--tree" in args else HERE
    run(tree, args[args.index("--kept") + 1] if "--kept" in args else None)
