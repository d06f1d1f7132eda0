"""Bit identity of the outer iteration (csrc/step.cpp: the four algorithms, their gated `post`, the status check) across two builds of the library.

    python tools/step_digest.py [--kept new.npz] > new.jsonl
    FOSHIP_LIB=/path/to/parent/libfoship.so python tools/step_digest.py [--kept parent1.npz] > parent1.jsonl        (the ABI is the same)
    python tools/step_digest.py --compare parent1.jsonl parent2.jsonl new.jsonl

Public Python API only.  One JSON record per case, kept short (116 cases): "iterates" is the SHA-256 over the SHA-256 digests of get_iterate() after each of 30
steps (one fos_step call per step, so that a step with and a step without a status check both occur at every check interval but 1), "iterate_tags" the first
two characters of each of the 30, which name the first step that differs (the digest decides); "checks" the number of check results and the SHA-256 over every field of every
one of them, floats by repr; at the end the digests of get_alg_state(), get_affine_state() and get_checked() (null where no check ran), prox_count(),
psd_fused_steps() and the launch counts per class of profile_read_classes() under profile(1).

Groups:
  "direct"  workloads.small_mixed() with enable_direct: GAP(0.8, 1.5, 1.6), DR, AP, GAPA(0.8, 0.5), FISTA, Dykstra; checki 1, 4 and 1000; the step's
            switches unset and FOS_PSD_FUSE=0, FOS_RELAX_EW=0, FOS_SHIFT_FUSE=0, FOS_FUSED_RHS=0 one at a time.  The first three are read per handle; the
            last is read once per process, so its cases run in a child process of their own (--only-env).
  "fused"   tests/step_identity.one_problem and mixed_problem under DR with enable_direct, checki 4 and 1000: the one-launch step.  The counter of fused
            steps must be non-zero (checked when the record is made) and equal.
  "eq"      small_mixed() created with equilibrate=10, enable_direct, DR and GAPA(0.8, 0.5), checki 1: the status fill in the caller's units.
  "cg"      c1_readme_nnls(seed=2) without direct: DR, GAPA(0.8, 0.5), FISTA, Dykstra; checki 1 and 1000; FOS_SPECULATE unset and = 0 (and, in the child
            process, FOS_FUSED_RHS=0 at checki 1000).  A CG solve ends on a stop the host observes, so --kept FILE saves the iterates after steps 10, 20
            and 30 beside the records.
--compare: the first two files are two runs of the parent.  direct, fused, eq: every field of the first file against each other file.  cg: where the two
parent runs agree bit for bit the new build must too; where they do not, the kept iterates (<records>.jsonl -> <records>.npz) are compared at
1e-4 max(1, |x|) -- the tolerance tests/test_gpu_linesearch.py follows the oracle with under CG -- and the output says so.
"""
import base64
import hashlib
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent.parent
STEPS = 30
CG_TOL = 1e-4
FIELDS = ("p", "d", "g", "ctx", "bty", "kappa", "tau", "norm_axs", "norm_aty", "norm_b", "norm_c", "cgiter", "status", "cg_maxiter_hit")
PROCESS_ENV = "FOS_FUSED_RHS=0"                  # read once per process: its cases run in a child


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    return base64.b64encode(h.digest()).decode().rstrip("=")


def sha_text(v):
    return base64.b64encode(hashlib.sha256(json.dumps(v, separators=(",", ":")).encode()).digest()).decode().rstrip("=")


def algorithms(pkg, direct, names):
    kw = dict(direct=True) if direct else {}
    table = {"GAP": lambda: pkg.GAP(0.8, 1.5, 1.6, **kw), "DR": lambda: pkg.DR(**kw), "AP": lambda: pkg.AP(**kw), "GAPA": lambda: pkg.GAPA(0.8, 0.5, **kw),
             "FISTA": lambda: pkg.FISTA(**kw), "Dykstra": lambda: pkg.Dykstra(**kw)}
    return [(n, table[n]) for n in names]


def cases(pkg, only_env):
    """(name, environment for the create, problem, direct, equilibrate, algorithm, checki, keep the iterates)"""
    import step_identity as si
    w = pkg.workloads
    sm, nnls = w.small_mixed(), w.c1_readme_nnls(seed=2)
    four = ("DR", "GAPA", "FISTA", "Dykstra")
    if only_env:
        for an, alg in algorithms(pkg, True, ("GAP", "DR", "AP") + four[1:]):
            for checki in (1, 4, 1000):
                yield "direct/%s/checki=%d/%s" % (an, checki, only_env), {}, sm, True, 0, alg, checki, False
        for an, alg in algorithms(pkg, False, four):
            yield "cg/%s/checki=1000/%s" % (an, only_env), {}, nnls, False, 0, alg, 1000, True
        return
    for env in ({}, {"FOS_PSD_FUSE": "0"}, {"FOS_RELAX_EW": "0"}, {"FOS_SHIFT_FUSE": "0"}):
        tag = "".join("/%s=%s" % kv for kv in env.items())
        for an, alg in algorithms(pkg, True, ("GAP", "DR", "AP") + four[1:]):
            for checki in (1, 4, 1000):
                yield "direct/%s/checki=%d%s" % (an, checki, tag), env, sm, True, 0, alg, checki, False
    for pn, prob in (("one", si.one_problem(w)), ("mixed", si.mixed_problem(w))):
        for checki in (4, 1000):
            yield "fused/%s/DR/checki=%d" % (pn, checki), {}, prob, True, 0, algorithms(pkg, True, ("DR",))[0][1], checki, False
    for an, alg in algorithms(pkg, True, ("DR", "GAPA")):
        yield "eq/%s/checki=1" % an, {}, sm, True, 10, alg, 1, False
    for env in ({}, {"FOS_SPECULATE": "0"}):
        tag = "".join("/%s=%s" % kv for kv in env.items())
        for an, alg in algorithms(pkg, False, four):
            for checki in (1, 1000):
                yield "cg/%s/checki=%d%s" % (an, checki, tag), env, nnls, False, 0, alg, checki, True


def run_case(pkg, env, prob, direct, equilibrate, alg, checki):
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        d = pkg.HipHSDE(prob.A, prob.b, prob.c, prob.K1, prob.K2, equilibrate=equilibrate)
    finally:
        for k, v in saved.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    if direct:
        d.enable_direct(prob.A)
    d.set_alg(alg())
    d.set_iterate(None)
    d.profile(1)
    rec, kept, any_check = dict(iterates=[], checks=[]), {}, False
    for i in range(1, STEPS + 1):
        _, checked, res = d.step(i, 1, checki, 1e-30)
        z = d.get_iterate()
        rec["iterates"].append(sha(z))
        if checked:
            any_check = True
            rec["checks"].append(dict(step=i, **{f: repr(getattr(res, f)) for f in FIELDS}))
        if i % 10 == 0:
            kept[str(i)] = z
    rec = dict(iterates=sha_text(rec["iterates"]), iterate_tags="".join(s[:2] for s in rec["iterates"]), checks=[len(rec["checks"]), sha_text(rec["checks"])])
    rec["launches"] = {k: int(n) for k, (n, _) in d.profile_read_classes().items()}
    a, b, t, a12 = d.get_alg_state()
    xinit, pi, firstrun = d.get_affine_state()
    rec["alg_state"] = [sha(a, b), repr(t), repr(a12)]
    rec["affine_state"] = [sha(xinit), int(pi), bool(firstrun)]
    rec["checked"] = sha(d.get_checked()) if any_check else None
    rec["prox_count"] = int(d.prox_count())
    rec["psd_fused_steps"] = int(d.psd_fused_steps())
    d.close()
    return rec, kept


def run(only_env, kept_file):
    sys.path.insert(0, str(HERE / "tests"))
    sys.path.insert(0, str(HERE / "oracle"))
    sys.path.insert(0, str(HERE))
    import __graft_entry__ as ge
    pkg = ge.load_package()
    kept = {}
    for name, env, prob, direct, equilibrate, alg, checki, keep in cases(pkg, only_env):
        rec, zs = run_case(pkg, env, prob, direct, equilibrate, alg, checki)
        if name.startswith("fused/") and rec["psd_fused_steps"] <= 0:
            raise SystemExit("%s: no step took the one-launch form" % name)
        if keep:
            kept.update({"%s@%s" % (name, i): z for i, z in zs.items()})
        print(json.dumps(dict(case=name, **rec), separators=(",", ":")), flush=True)
    if not only_env:                                     # the per-process switch: a fresh child, its records behind ours, its kept iterates beside ours
        child_kept = str(Path(kept_file).with_suffix(".child.npz")) if kept_file else None
        cmd = [sys.executable, str(Path(__file__).resolve()), "--only-env", PROCESS_ENV] + (["--kept", child_kept] if child_kept else [])
        name, value = PROCESS_ENV.split("=")
        out = subprocess.run(cmd, env=dict(os.environ, **{name: value}), check=True, stdout=subprocess.PIPE, text=True).stdout
        sys.stdout.write(out)
        sys.stdout.flush()
        if child_kept:
            with np.load(child_kept) as k:
                kept.update({key: k[key] for key in k.files})
            os.remove(child_kept)
    if kept_file:
        np.savez(kept_file, **kept)


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
        print("%s vs %s: %d cases (direct, fused, eq), %s" % (files[0], other, len(exact), "every field and digest equal" if not diff else "%d DIFFER" % len(diff)))
        bad += len(diff)
    if len(files) >= 3:
        p2, new = load(files[1]), load(files[2])
        cg = [c for c in base if c.startswith("cg/")]
        agree = [c for c in cg if base[c] == p2.get(c)]
        same = [c for c in agree if new.get(c) == base[c]]
        for c in agree:
            if c not in same:
                print("DIFFER %s: the two parent runs agree bit for bit, the new build does not" % c)
        print("cg: %d cases; the two parent runs agree bit for bit on %d of them, the new build agrees with them on %d of those" % (len(cg), len(agree), len(same)))
        bad += len(agree) - len(same)
        loose = [c for c in cg if c not in agree]
        if loose:
            npz = [Path(f).with_suffix(".npz") for f in files[:3]]
            if not all(f.exists() for f in npz):
                print("cg: %d cases where the parent runs do NOT agree and the iterates were not kept (run with --kept <records>.npz)" % len(loose))
                return bad + len(loose)
            k1, k2, kn = (np.load(f) for f in npz)
            for c in loose:
                worst = lambda k: max(float(np.abs(k[key] - k1[key]).max() / max(1.0, np.linalg.norm(k1[key]))) for key in k1.files if key.startswith(c + "@"))
                wp, wn = worst(k2), worst(kn)
                print("%s: the two parent runs do NOT agree bit for bit (a CG solve ends on a host-observed stop); largest |x - x_parent1| / max(1, |x|) after "
                      "steps 10, 20, 30: parent2 %.2e, new %.2e (tolerance %.0e): %s" % (c, wp, wn, CG_TOL, "within" if wn <= CG_TOL else "OUTSIDE"))
                bad += not wn <= CG_TOL
    return bad


if __name__ == "__main__":
    args = sys.argv[1:]
    if args[:1] == ["--compare"]:
        sys.exit(1 if compare(args[1:]) else 0)
    run(args[args.index("--only-env") + 1] if "--only-env" in args else None, args[args.index("--kept") + 1] if "--kept" in args else None)
