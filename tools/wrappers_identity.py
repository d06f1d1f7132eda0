"""Bit identity of the three wrappers (LineSearchWrapper, GAPP, LongstepWrapper) across two builds, on both problem forms.

    python tools/wrappers_identity.py [--kept new.npz] > new.jsonl
    python tools/wrappers_identity.py --tree <parent checkout> [--kept parent1.npz] > parent1.jsonl        (or FOSHIP_LIB=... where the ABI did not change)
    python tools/wrappers_identity.py --compare parent1.jsonl parent2.jsonl new.jsonl
    python tools/wrappers_identity.py [--tree ...] --time > new_times.json ;  --compare-times parent1_times.json parent2_times.json new_times.json

Public Python API only (of the package of --tree: a build with another ABI brings its own mirror).  One JSON record per case: the SHA-256 of get_iterate() after
every one of 30 steps (base64), and the log of every search or projection as the mirror returns it.

Groups: "hsde" -- workloads.small_mixed() with enable_direct (no CG solve in a digest); "feas" -- affine_box_instance(m=50, n=100) as IndAffine n IndBox(0, inf);
each with LineSearchWrapper(GAP(0.8, 1.5, 1.6), 10), LineSearchWrapper(GAPA(0.8, 0.5), 10), GAPP(iproj=10), LongstepWrapper(., 7, 2) around DR, GAPA, FISTA and
Dykstra, LongstepWrapper(DR, 25, 10).  "cg" -- c1_readme_nnls(seed=2) without direct: LineSearchWrapper(DR), GAPP, LongstepWrapper(DR, 7, 2); a CG solve ends on a
host-observed stop, so --kept FILE also saves the iterates of their search / projection steps and of the last one (an .npz beside the records, not for the history).
--compare: the first two files are two runs of the parent.  hsde and feas: every field and digest of the first file against each other file.  cg: where the two
parent runs agree bit for bit the new build must too; where they do not, the iterates kept beside the records (<records>.jsonl -> <records>.npz) are compared at
1e-4 max(1, |x|) -- the tolerance tests/test_gpu_linesearch.py follows the oracle with under CG -- and the output says so.
--time: the median of five wall times of the 30 steps per case; --compare-times: the geometric mean over the cases of new / parent1 next to parent2 / parent1.
"""
import base64
import hashlib
import json
import math
import statistics
import sys
import time
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent.parent
STEPS = 30
CG_TOL = 1e-4


def sha(a):
    return base64.b64encode(hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).digest()).decode().rstrip("=")


def plain(v):
    """a log as the mirror returns it (tuple / dict of numbers and arrays) -> JSON values; floats keep their bits through repr"""
    if isinstance(v, dict):
        return {k: plain(x) for k, x in v.items()}
    if isinstance(v, (tuple, list, np.ndarray)):
        return [plain(x) for x in v]
    return v.item() if isinstance(v, np.generic) else v


def wrappers(pkg, direct):
    kw = dict(direct=True) if direct else {}
    L = lambda alg, li, ns: (pkg.LongstepWrapper(alg, longinterval=li, nsave=ns), "longstep_log", li)
    return {
        "LineSearch(GAP,10)": (pkg.LineSearchWrapper(pkg.GAP(0.8, 1.5, 1.6, **kw), lsinterval=10), "linesearch_log", 10),
        "LineSearch(GAPA,10)": (pkg.LineSearchWrapper(pkg.GAPA(0.8, 0.5, **kw), lsinterval=10), "linesearch_log", 10),
        "GAPP(10)": (pkg.GAPP(0.8, 1.8, 1.8, iproj=10, direct=direct), "gapp_log", 10),
        "Longstep(DR,7,2)": L(pkg.DR(**kw), 7, 2), "Longstep(GAPA,7,2)": L(pkg.GAPA(0.8, 0.5, **kw), 7, 2),
        "Longstep(FISTA,7,2)": L(pkg.FISTA(**kw), 7, 2), "Longstep(Dykstra,7,2)": L(pkg.Dykstra(**kw), 7, 2),
        "Longstep(DR,25,10)": L(pkg.DR(**kw), 25, 10),
    }


def cases(pkg):
    from feasibility_cases import affine_box_instance
    sm = pkg.workloads.small_mixed()

    def hsde(prob, direct):
        def make():
            d = pkg.HipHSDE(prob.A, prob.b, prob.c, prob.K1, prob.K2)
            if direct:
                d.enable_direct(prob.A)
            return d
        return make
    for name, w in wrappers(pkg, True).items():
        yield "hsde/" + name, hsde(sm, True), w, False
    A, b = affine_box_instance(m=50, n=100)
    feas = lambda: pkg.HipFeasibility(pkg.Feasibility(pkg.IndAffine(A, b), pkg.IndBox(0.0, np.inf), 100))
    for name, w in wrappers(pkg, False).items():
        yield "feas/" + name, feas, w, False
    nnls = pkg.workloads.c1_readme_nnls(seed=2)
    cg = wrappers(pkg, False)
    cg["LineSearch(DR,10)"] = (pkg.LineSearchWrapper(pkg.DR(), lsinterval=10), "linesearch_log", 10)
    for name in ("LineSearch(DR,10)", "GAPP(10)", "Longstep(DR,7,2)"):
        yield "cg/" + name, hsde(nnls, False), cg[name], True


def run_case(make, w, keep):
    alg, logname, every = w
    d = make()
    d.set_alg(alg)
    d.set_iterate(None)
    rec = dict(iterates=[], logs=[], kept={})
    t0 = time.perf_counter()
    for i in range(1, STEPS + 1):
        d.step(i, 1, 10 ** 9, 1e-30)
        z = d.get_iterate()
        rec["iterates"].append(sha(z))
        if i % every == 0:
            rec["logs"].append(plain(getattr(d, logname)()))
        if keep and (i % every == 0 or i == STEPS):
            rec["kept"][str(i)] = z
    rec["wall_s"] = time.perf_counter() - t0
    d.close()
    return rec


def load_pkg(tree):
    sys.path.insert(0, str(HERE / "tests"))           # (the instances: the same in every checkout compared)
    sys.path.insert(0, str(tree))
    import __graft_entry__ as ge
    return ge.load_package()


def run(tree, timing, kept_file):
    pkg = load_pkg(tree)
    times, kept = {}, {}
    for name, make, w, keep in cases(pkg):
        if timing:
            times[name] = statistics.median(run_case(make, w, False)["wall_s"] for _ in range(5))
            continue
        rec = run_case(make, w, keep)
        kept.update({"%s@%s" % (name, i): z for i, z in rec["kept"].items()})
        print(json.dumps(dict(case=name, iterates=rec["iterates"], logs=rec["logs"]), separators=(",", ":")), flush=True)
    if kept_file:
        np.savez(kept_file, **kept)
    if timing:
        print(json.dumps(times, indent=1))


def compare(files):
    load = lambda f: {r["case"]: r for r in map(json.loads, filter(str.strip, Path(f).read_text().splitlines()))}
    base, bad = load(files[0]), 0
    exact = [c for c in base if not c.startswith("cg/")]
    for other in files[1:]:
        got = load(other)
        diff = [c for c in exact if got.get(c) != base[c]] + [c for c in got if c not in base]
        for c in diff:
            a, b = base.get(c, {}), got.get(c, {})
            print("DIFFER %s: %s" % (c, [k for k in sorted(set(a) | set(b)) if a.get(k) != b.get(k)]))
        print("%s vs %s: %d cases (hsde, feas), %s" % (files[0], other, len(exact), "every field and digest equal" if not diff else "%d DIFFER" % len(diff)))
        bad += len(diff)
    if len(files) >= 3:
        p2, new = load(files[1]), load(files[2])
        for c in (c for c in base if c.startswith("cg/")):
            if base[c] == p2[c]:
                same = new[c] == base[c]
                print("%s: the two parent runs agree bit for bit; the new build %s" % (c, "agrees with them bit for bit" if same else "DIFFERS"))
                bad += not same
                continue
            npz = [Path(f).with_suffix(".npz") for f in files[:3]]
            if not all(f.exists() for f in npz):
                print("%s: the two parent runs do NOT agree bit for bit and the iterates were not kept (run with --kept <records>.npz)" % c)
                bad += 1
                continue
            k1, k2, kn = (np.load(f) for f in npz)
            worst = lambda k: max(float(np.abs(k[key] - k1[key]).max() / max(1.0, np.linalg.norm(k1[key]))) for key in k1.files if key.startswith(c + "@"))
            wp, wn = worst(k2), worst(kn)
            print("%s: the two parent runs do NOT agree bit for bit (a CG solve ends on a host-observed stop); largest |x - x_parent1| / max(1, |x|) at the search / "
                  "projection steps and the last: parent2 %.2e, new %.2e (tolerance %.0e): %s" % (c, wp, wn, CG_TOL, "within" if wn <= CG_TOL else "OUTSIDE"))
            bad += not wn <= CG_TOL
    return bad


def compare_times(files):
    p1, p2, new = (json.loads(Path(f).read_text()) for f in files)
    gm = lambda a, b: math.exp(statistics.fmean(math.log(a[c] / b[c]) for c in p1))
    band, ratio = gm(p2, p1), gm(new, p1)
    lo, hi = min(band, 1 / band), max(band, 1 / band)
    for c in p1:
        print("%-28s parent1 %8.2f ms  parent2 %8.2f ms  new %8.2f ms" % (c, 1e3 * p1[c], 1e3 * p2[c], 1e3 * new[c]))
    print("geometric mean over %d cases: parent2 / parent1 = %.4f (band %.4f .. %.4f), new / parent1 = %.4f: %s" % (len(p1), band, lo, hi, ratio, "within the band" if lo <= ratio <= hi else "OUTSIDE the band"))
    return 0


if __name__ == "__main__":
    args = sys.argv[1:]
    if args[:1] == ["--compare"]:
        sys.exit(1 if compare(args[1:]) else 0)
    if args[:1] == ["--compare-times"]:
        sys.exit(compare_times(args[1:]))
    tree = Path(args[args.index("--tree") + 1]).resolve() if "--tree" in args else HERE
    run(tree, "--time" in args, args[args.index("--kept") + 1] if "--kept" in args else None)
