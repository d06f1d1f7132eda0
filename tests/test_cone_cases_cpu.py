"""The cone cases of cone_cases.py on the CPU: every reference is regenerated with mpmath, certified in extended precision and compared with
tests/golden/cone_edges.npz exactly; the oracle's restatement (prox_soc, prox_socrot, prox_exp_primal, prox_exp_dual and the Moreau copies) is run on every
case -- it must stay within a quarter of the derived SOC tolerance, it defines the Exp allowance of the benign class, and the ill-conditioned triples on
which it misses the certified projection at 1e-8 are pinned; and Case.check must reject the mistakes it exists to catch.

    python tests/test_cone_cases_cpu.py        prints the CPU part of profiles/cone_edges_allowance.txt
"""
import math

import numpy as np

import cone_cases as cc

# the ill-conditioned triples whose restated projection is further than 1e-8 max(1, ||z||) from the certified one: the ported algorithm's known behaviour
# (cone_certificates.py).  Indices into cone_cases.exp_triples(op); a change of the algorithm shows up here.
# (12 and 16 are points 1e-9 outside the surface, where the Newton solve ends on noise: 2e-8 and 4e-8; their neighbours 14 and 18 end at 7e-9 and 3e-9.)
ILL_MISSES = {"P": [12, 16, 79, 80, 118], "D": [12, 16, 79, 80, 96, 122, 138]}


def _oracle():
    import fos_oracle
    return fos_oracle


_computed = {}


def computed():
    """every reference again (certified on the way), once per session"""
    if not _computed:
        full = {}
        _computed["data"], _computed["full"] = cc.compute_fixture(_oracle(), full), full
    return _computed


def oracle_soc(kind, x, dual=False):
    orc = _oracle()
    y = np.empty_like(x)
    (orc.cone_prox_dual if dual else orc.cone_prox)(orc.CONE_CODES[kind], y, x)
    return y


def test_fixture_is_current_and_every_reference_certifies():
    """a stale fixture fails; compute_fixture raises on a reference that does not certify (no case is skipped: a triple without a certified projection has
    to be replaced in the case list)"""
    data = computed()["data"]
    with np.load(cc.FIXTURE) as f:
        assert sorted(f.files) == sorted(data)
        for key in data:
            assert np.array_equal(f[key], data[key]), key + ": run tests/golden/make_cone_edges.py"
    assert cc.FIXTURE.stat().st_size < 512 * 1024


def test_long_cones_are_rebuilt_to_the_correctly_rounded_outputs():
    """4097 / 4098 entries: (r_hi + r_lo) x_k in long double against the correctly rounded extended-precision product, element by element"""
    for (kind, length, name), want in computed()["full"].items():
        got = cc.Case.get(kind, length, name).ref
        assert np.abs(got - want).max() <= 0.0 or np.all(np.abs(got - want) <= np.spacing(np.abs(want))), (kind, length, name)
        assert np.count_nonzero(got != want) <= length // 200, (kind, length, name, np.count_nonzero(got != want))


def soc_ratios():
    """worst error / tolerance of the oracle's restatement per (kind, length): primal and Moreau copy, every finite case; the exact cases' bit identities and
    the homogeneity cases ride along"""
    worst = {}
    for kind, length, name in cc.soc_keys():
        case = cc.Case.get(kind, length, name)
        for dual in (False, True):
            r = case.check(oracle_soc(kind, case.x, dual), what="oracle dual" if dual else "oracle", dual=dual)
            worst[(kind, length)] = max(worst.get((kind, length), 0.0), r)
        if name in cc.HOMOGENEITY_BASE:
            y0 = oracle_soc(kind, case.x)
            for k in cc.HOMOGENEITY_BITS:
                assert np.array_equal(oracle_soc(kind, np.ldexp(case.x, k)), np.ldexp(y0, k)), (case.label(), k)
            for k in cc.HOMOGENEITY_RANGE:
                for dual in (False, True):
                    r = case.check(oracle_soc(kind, np.ldexp(case.x, k), dual), scale=k, what="oracle, rescaled norm", dual=dual)
                    worst[(kind, length)] = max(worst[(kind, length)], r)
    return worst


def test_oracle_soc_within_a_quarter_of_the_tolerance():
    for key, r in soc_ratios().items():
        assert r <= 0.25, (key, r)


def test_oracle_soc_nonfinite_cases_run():
    """NaN / Inf inputs: the restatement answers (the GPU test compares patterns with it) and a NaN poisons the whole cone"""
    for kind in cc.KINDS:
        for length in cc.LENGTHS[kind]:
            for name in cc._NONFINITE:
                case = cc.Case.get(kind, length, name)
                y = oracle_soc(kind, case.x)
                case.check_pattern(y, y)
                if name.startswith("nan"):
                    assert np.isnan(y).all(), case.label()


def exp_report():
    """-> (worst oracle error of the benign class relative to max(1, ||z||), {op: indices of ill triples missed at 1e-8}, worst miss)"""
    orc = _oracle()
    worst, misses, worst_miss = 0.0, {"P": [], "D": []}, 0.0
    for op in "PD":
        for case in cc.exp_cases(op):
            y = cc.exp_oracle(op, case.x, orc)
            err = float(np.abs(y - case.ref).max()) / case.scale
            case.check(y, y, what="oracle")                       # hand: the exact answer's bits; benign: within the allowance; ill: trivially
            if case.cls == "benign":
                worst = max(worst, err)
            elif case.cls == "ill" and err > 1e-8:
                misses[op].append(case.index)
                worst_miss = max(worst_miss, err)
    return worst, misses, worst_miss


def test_oracle_exp_defines_the_allowance_and_the_known_misses():
    worst, misses, _ = exp_report()
    assert cc.fixture().exp_allowance == 4.0 * worst
    assert 0.0 < worst < 1e-11                                    # (the benign class is benign)
    assert misses == ILL_MISSES
    for op in "PD":                                               # both losses named in cone_certificates.py are among them
        lost = [c.index for c in cc.exp_cases(op) if c.note == "known loss"]
        assert set(lost) <= set(misses[op]), (op, lost)


# ---------------------------------------------------------------------------------------------- sensitivity: what the check must reject

def soc_fp64(kind, x, drop_lane63=False, drop_x2=False, c=0.7071067811865475, tail_unscaled=False):
    """the kernel's arithmetic in fp64, with the mistakes of the mutants switched on"""
    rot = kind == "SOCRotated"
    head = 2 if rot else 1
    t, x2 = (c * x[0] + c * x[1], c * x[0] - c * x[1]) if rot else (x[0], 0.0)
    tail = x[head:]
    seen = np.delete(tail, np.arange(63, len(tail), 64)) if drop_lane63 else tail
    nx = math.sqrt(float(seen @ seen) + (0.0 if drop_x2 else x2 * x2))
    y = np.empty_like(x)
    if t <= -nx:
        r, y0 = 0.0, 0.0
    elif t >= nx:
        r, y0 = 1.0, t
    else:
        r = 0.5 * (1.0 + t / nx)
        y0 = r * nx
    y[head:] = tail if (tail_unscaled and r > 0.0) else r * tail
    if rot:
        y[0], y[1] = c * y0 + c * (r * x2), c * y0 - c * (r * x2)
    else:
        y[0] = y0
    return y


def exp_bisection_1e10(v):
    """prox_exp_primal with the bisection on rho stopped at 1e-10"""
    orc = _oracle()
    y = np.empty(3)
    orc.prox_exp_primal(y, v)
    v = tuple(float(a) for a in v)
    if cc.exp_branch(v) != "surface":
        return y
    ub, lb = orc._exp_rho_ub(v)
    z = v
    for _ in range(100):
        rho = (ub + lb) / 2
        g, z = orc._exp_calc_grad(v, rho, z)
        if g > 0:
            lb = rho
        else:
            ub = rho
        if ub - lb < 1e-10:
            break
    return np.array(z)


def mutant_factors():
    """worst error / tolerance of every deliberately wrong restatement over the cases it is run on"""
    finite = [cc.Case.get(*key) for key in cc.soc_keys()]
    by = lambda fn, cases: max(c.error_ratio(fn(c)) for c in cases)
    rot = [c for c in finite if c.kind == "SOCRotated"]
    f = {
        "unmutated fp64 restatement": by(lambda c: soc_fp64(c.kind, c.x), finite),
        "norm without lane 63's entries": by(lambda c: soc_fp64(c.kind, c.x, drop_lane63=True), finite),
        "norm without the rotated second entry": by(lambda c: soc_fp64(c.kind, c.x, drop_x2=True), rot),
        "rotation constant rounded to fp32": by(lambda c: soc_fp64(c.kind, c.x, c=float(np.float32(0.7071067811865475))), rot),
        "dual copy taken from the other part": by(lambda c: oracle_soc(c.kind, cc.Case.get(c.kind, c.length, "gauss_1" if c.name != "gauss_1" else "inside").x), [c for c in finite if c.tol > 0.0]),
        "r applied to the head, not the tail": by(lambda c: soc_fp64(c.kind, c.x, tail_unscaled=True), finite),
    }
    orc = _oracle()
    benign = [c for c in cc.exp_cases("P") if c.cls == "benign"]
    f["Exp: bisection stopped at 1e-10"] = max(c.error_ratio(exp_bisection_1e10(c.x), cc.exp_oracle("P", c.x, orc)) for c in benign)
    return f


def test_the_check_rejects_each_mutant():
    f = mutant_factors()
    assert f.pop("unmutated fp64 restatement") <= 0.25
    for name, factor in f.items():
        assert factor > 1.0, (name, factor)


def report():
    lines = ["== CPU: the oracle's fp64 restatement against the certified references (tests/test_cone_cases_cpu.py) ==",
             "worst error / tolerance per kind and length, primal and Moreau copy, +-600 homogeneity cases included (bound asserted: 0.25)"]
    for (kind, length), r in soc_ratios().items():
        lines.append("%-11s %5d   %.3f" % (kind, length, r))
    worst, misses, worst_miss = exp_report()
    lines += ["", "Exp, benign class (|r/s|, |s/r| <= 10): worst oracle error %.3e max(1, ||z||); GPU allowance = 4 x that = %.3e" % (worst, 4 * worst),
              "Exp, ill-conditioned class: triples whose restated projection misses the certified one at 1e-8 max(1, ||z||) (worst %.3e):" % worst_miss]
    for op in "PD":
        for i in misses[op]:
            c = cc.exp_cases(op)[i]
            y = cc.exp_oracle(op, c.x, _oracle())
            lines.append("  %s #%-3d %-26s x = (%.6g, %.6g, %.6g)  error %.2e" % (op, i, c.note, *c.x, float(np.abs(y - c.ref).max()) / c.scale))
    lines += ["", "mutants: worst error / tolerance over the cases (each must exceed 1)"]
    for name, factor in mutant_factors().items():
        lines.append("  %-40s %.3g" % (name, factor))
    return lines


if __name__ == "__main__":
    import sys
    from pathlib import Path
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "oracle"))
    print("\n".join(report()))
