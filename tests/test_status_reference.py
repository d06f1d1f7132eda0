"""
The extended-precision status reference (tests/status_reference.py) against the fp64 oracle, before a GPU is involved: on the golden
operators, on every operator shape of the device tests and on their scaled inputs the oracle's residuals must lie within the reference's
worst-case fp64 allowance (x 1: the oracle is one fp64 evaluation of the formulas), and the oracle's decision must be the reference's
wherever the reference is farther from each threshold than its allowance -- which, with the seeds of status_cases.py, is everywhere.
"""
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse as sp

import fos_oracle as orc
import status_cases as cases
import status_reference as sref

GOLDEN = Path(__file__).resolve().parent / "golden"


def _oracle_vs_reference(label, A, b, c, z, worst):
    ref = orc.residuals(SimpleNamespace(A=A, b=b, c=c), z)
    vals, allow = sref.reference(A, b, c, z)
    rat = sref.ratios(ref, vals, allow)
    for k, v in rat.items():
        worst[k] = max(worst.get(k, 0.0), v)
    assert max(rat.values()) <= 1.0, (label, rat)
    skipped = 0
    for eps in cases.EPS:
        if sref.margin(vals, eps) > 2 * sref.relative_allowance(vals, allow, eps):
            assert orc.decide_status(ref, eps) == sref.decide(vals, eps), (label, eps)
        else:
            skipped += 1
    return skipped


def _report(what, worst):
    print("%s: worst |oracle - reference| / allowance per field: %s" % (what, ", ".join("%s %.3g" % kv for kv in sorted(worst.items()))))


def test_longdouble_is_extended():
    assert np.finfo(np.longdouble).eps <= 1.1e-19


def test_reference_on_a_hand_computed_point():
    """A 2 x 2 example worked by hand: A = [[1, 2], [0, 3]], x = (1, -1), y = (2, 1), tau = 2."""
    A = sp.csc_matrix(np.array([[1.0, 2.0], [0.0, 3.0]]))
    b, c = np.array([1.0, 2.0]), np.array([0.5, -1.0])
    #             x        y       tau   r        s        kappa
    z = np.array([1.0, -1.0, 2.0, 1.0, 2.0, 4.0, 0.0, 1.0, -2.0, 0.25])
    vals, allow = sref.reference(A, b, c, z)
    # A x = (-1, -3), A'y = (2, 7); rp = (-1 + 1) / 2 - 1, (-3 - 2) / 2 - 2 = (-1, -4.5); rd = 2/2 + .5 - 4/2, 7/2 - 1 - 0 = (-.5, 2.5)
    assert float(vals["p"]) == pytest.approx(np.hypot(1.0, 4.5) / (1 + np.sqrt(5.0)), rel=1e-15)
    assert float(vals["d"]) == pytest.approx(np.hypot(0.5, 2.5) / (1 + np.sqrt(1.25)), rel=1e-15)
    assert float(vals["ctx"]) == 1.5 and float(vals["bty"]) == 4.0
    assert float(vals["g"]) == pytest.approx(2.75 / (1 + 0.75 + 2.0), rel=1e-15)
    assert float(vals["nAxs"]) == pytest.approx(5.0, rel=1e-15)          # (-1 + 1, -3 - 2)
    assert float(vals["nATy"]) == pytest.approx(np.hypot(2.0, 7.0), rel=1e-15)
    assert float(vals["tau"]) == 2.0 and float(vals["kappa"]) == 0.25
    assert all(float(allow[k]) > 0 for k in ("p", "d", "g", "ctx", "bty", "nAxs", "nATy")) and all(float(allow[k]) < 1e-13 for k in sref.FIELDS)
    assert sref.decide(vals, 1e-3) == "Continue"


def test_decide_reproduces_julias_division_by_zero():
    base = dict(p=1.0, d=1.0, g=1.0, ctx=-1.0, bty=1.0, nAxs=1.0, nATy=1.0, nb=1.0, nc=0.0, tau=1.0, kappa=0.0)
    res = {k: np.longdouble(v) for k, v in base.items()}
    assert sref.decide(res, 1e-3) == "Unbounded"                         # -ctx / 0 = +Inf
    res["ctx"] = np.longdouble(0.0)
    assert sref.decide(res, 1e-3) == "Continue"                          # 0 / 0 = NaN: the comparison is false
    res.update(nc=np.longdouble(1.0), nb=np.longdouble(0.0), bty=np.longdouble(-1.0), ctx=np.longdouble(1.0))
    assert sref.decide(res, 1e-3) == "Infeasible"
    res.update(p=np.longdouble(np.nan), tau=np.longdouble(0.0))
    assert sref.decide(res, 1e-3) == "Infeasible"                        # NaN residuals: not Optimal, the later tests still run
    assert sref.margin(res, 1e-3) > 0


def test_oracle_within_allowance_on_golden_operators():
    worst, seen = {}, 0
    for f in sorted(GOLDEN.glob("*_operators.npz")):
        g = np.load(f)
        A = sp.csc_matrix((g["data"], g["indices"], g["indptr"]), shape=(int(g["m"]), int(g["n"])))
        b, c = g["b"], g["c"]
        rng = np.random.default_rng(cases._seed("golden", f.name))
        pts = [np.asarray(g["zc"], dtype=np.float64)]                     # the point whose check result the golden file records
        for trial in range(3):
            z = rng.standard_normal(2 * (sum(A.shape) + 1))
            z[sum(A.shape)] = abs(z[sum(A.shape)]) + 0.1
            pts.append(z)
        for trial, z in enumerate(pts):
            assert _oracle_vs_reference((f.name, trial), A, b, c, z, worst) == 0
            seen += 1
    assert seen > 0
    _report("golden operators", worst)


def _all_operators():
    return cases.row_block_shapes() + cases.window_shapes()


def test_oracle_within_allowance_on_device_test_shapes_and_points():
    """every operator and every point of the device test, the scaled problems included; the reference skips no status comparison"""
    worst = {}
    for name, A in _all_operators():
        A = sp.csc_matrix(A)
        b, c = cases.vectors_for(name, A)
        for label, z in cases.points(name, A, b, c):
            assert _oracle_vs_reference((name, label), A, b, c, z, worst) == 0, (name, label)
        As, bs, cs, zs = cases.scaled_problem(name, A, b, c)
        assert _oracle_vs_reference((name, "scaled"), As, bs, cs, zs, worst) == 0, name
    _report("device test shapes", worst)


@pytest.mark.parametrize("which", ["tile-mixed", "tall"])
def test_constructed_certificates(which):
    """the four constructed points are what they are built to be, at both eps, with a margin of at least 1e-3 -- by the reference and the oracle"""
    A = sp.csc_matrix(dict(_all_operators())[which])
    b, c = cases.vectors_for(which, A)
    worst = {}
    for want, z in cases.certificates(A, b, c):
        vals, allow = sref.reference(A, b, c, z)
        for eps in cases.EPS:
            assert sref.decide(vals, eps) == want, (want, eps)
            assert sref.margin(vals, eps) >= 1e-3, (want, eps, sref.margin(vals, eps))
        assert _oracle_vs_reference((which, want), A, b, c, z, worst) == 0
    _report("certificates on %s" % which, worst)


def test_stacked_q_reference_against_oracle():
    A = sp.csc_matrix(dict(_all_operators())["tile-mixed"])
    b, c = cases.vectors_for("tile-mixed", A)
    rng = np.random.default_rng(5)
    u = rng.standard_normal(sum(A.shape) + 1)
    Qu, E = sref.stacked_q_reference(A, b, c, u)
    y = np.empty(u.size)
    orc.HSDEMatrixQ(A, b, c).mul(y, u)
    assert np.all(np.abs(y - Qu) <= E)
    assert float(np.max(np.abs(y - Qu) / E)) > 0                          # (the comparison sees the fp64 rounding: it is not vacuous)
