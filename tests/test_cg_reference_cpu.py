"""
The extended-precision CG reference (tests/cg_reference.py) and the cases of tests/cg_cases.py, before a GPU is involved: the reference
against a dense solve, the two screening conditions of every case, each fp64 evaluation within its own allowance, the allowance table,
and the detection power of the allowance: a first step length off by 1e-12 (relative) and one stored entry of A left out of the sweep
both exceed it.
"""
import numpy as np
import pytest
import scipy.sparse as sp

import cg_cases as cases
import cg_reference as cref

LD = cref.LD
SMALL = ("tiny-dense", "tile-1chunk", "tile-mixed", "all-zero", "tiny")
ALL_CASES = [(name, start) for name in cases.operators() for start in cases.STARTS]


def _dense_m(A, b, c):
    m, n = A.shape
    l = n + m + 1
    Q = np.zeros((l, l))
    Ad = A.toarray()
    Q[:n, n:n + m], Q[:n, l - 1] = Ad.T, c
    Q[n:n + m, :n], Q[n:n + m, l - 1] = -Ad, b
    Q[l - 1, :n], Q[l - 1, n:n + m] = -c, -b
    return np.block([[np.eye(l), Q.T], [Q, -np.eye(l)]])


def test_longdouble_is_extended():
    assert np.finfo(LD).eps <= 1.1e-19


@pytest.mark.parametrize("name", SMALL)
def test_reference_against_dense_solve(name):
    """On the small operators: M v of the reference is the dense product; x_1 is x_0 + (r.r / r.Mr) r; run to the end, the recurrence
    arrives at np.linalg.solve(M, rhs) -- on the scaled operator (cond M < 1.04) within 1e-13 max|x|."""
    for start in cases.STARTS:
        cs = cases.case(name, start)
        Md = _dense_m(cs.A, cs.b, cs.c)
        v = np.random.default_rng(3).standard_normal(cs.x0.shape[0])
        Mv = cref.kkt_mul(cs.A, cs.b, cs.c, v, LD)
        assert Mv.dtype == LD
        assert np.max(np.abs(Mv.astype(np.float64) - Md @ v)) <= 1e-13 * max(1.0, np.max(np.abs(Md @ v)))
        r0 = cs.rhs - Md @ cs.x0
        x1 = cs.x0 + (r0 @ r0) / (r0 @ (Md @ r0)) * r0
        xs, rn = cref.iterates(cs.A, cs.b, cs.c, cs.x0, cs.rhs, 1)
        assert len(xs) == 1 and len(rn) == 2
        assert np.max(np.abs(xs[0].astype(np.float64) - x1)) <= 1e-12 * np.max(np.abs(x1))
        assert float(rn[0]) == pytest.approx(np.linalg.norm(r0), rel=1e-12)
        if start in cases.TAMED:
            k = min(40, cs.x0.shape[0])
            xs, rn = cref.iterates(cs.A, cs.b, cs.c, cs.x0, cs.rhs, k)
            done = next(j for j in range(1, k + 1) if float(rn[j]) <= 1e-17 * float(rn[0]))      # (past convergence: 0 / 0)
            sol = np.linalg.solve(Md, cs.rhs)
            assert np.max(np.abs(xs[done - 1].astype(np.float64) - sol)) <= 1e-13 * np.max(np.abs(sol)), (start, done)


@pytest.mark.parametrize("name,start", ALL_CASES, ids=["%s-%s" % t for t in ALL_CASES])
def test_case_conditions_and_fp64_evaluations(name, start):
    """The two conditions the cases are screened for, and each of the three fp64 evaluations within the allowance measured from them
    (<= 1 / 4 by construction: a guard against later edits)."""
    cs = cases.case(name, start)
    ext = cref.extended(cs)
    assert cs.ks == ((1, 2, 3, 4) if start in cases.TAMED else (1,))
    if start in cases.TAMED:
        for k in (2, 3):
            tol = cref.decisive_tol(cs, k)
            assert tol is not None, (name, start, k, [float(v) for v in ext.rn])
            assert float(ext.rn[k]) * np.sqrt(3.0) <= tol <= float(ext.rn[k - 1]) / np.sqrt(3.0)
            assert all(float(ext.rn[j]) > tol for j in range(k))
    assert cases.first_step_visible(cs)
    assert cref.allowance(cs, 1) < 1e-12 * float(np.max(np.abs(ext.alphas[0] * ext.r0)))
    for k in cs.ks:
        assert cref.allowance(cs, k) >= 4 * cref.U * float(np.max(np.abs(ext.xs[k - 1])))
        for which, x in cref.fp64_evaluations(cs, k).items():
            assert cref.ratio(x, cs, k) <= 1.0 / cref.MARGIN + 1e-12, (which, k)


def test_allowance_table():
    tab = cases.table()
    print()
    print(cases.format_table(tab))
    assert len(tab) == len(ALL_CASES)
    worst = max(max(row.values()) for row in tab.values())
    print("largest allowance / max|x_k|: %.3g" % worst)
    assert all(np.isfinite(v) and v >= 4 * cref.U for row in tab.values() for v in row.values())


def test_prox_sequences_stop_decisively():
    """the two prox_affine calls of every operator: 1 .. 3 iterations each at the schedule's tolerances, every count of 1 .. 3 present"""
    counts = set()
    for name in cases.operators():
        seq = cases.prox_sequence(name)
        assert len(seq) == 2
        for x, k, xk, allow in seq:
            assert 1 <= k <= 3 and allow >= 4 * cref.U * float(np.max(np.abs(xk)))
            counts.add(k)
        print("%-24s iterations %s, allowance / max|y| %s" % (name, [t[1] for t in seq], ["%.2e" % (t[3] / float(np.max(np.abs(t[2])))) for t in seq]))
    assert counts == {1, 2, 3}


@pytest.mark.parametrize("name,start", [("sparse", "warm"), ("tile-chunks", "cold"), ("mixed-lengths", "raw")])
def test_allowance_detects_a_wrong_step_length_and_a_missing_entry(name, start):
    """An otherwise correct fp64 evaluation (pairwise dots) lies within the allowance; with alpha_0 scaled by 1 + 1e-12 it exceeds it at
    k = 1, and with ONE stored entry of A left out of every sweep M p it exceeds it at every k of the case."""
    cs = cases.case(name, start)
    kmax = max(cs.ks)
    run = lambda **kw: cref.recurrence(cs.coo, cs.b, cs.c, cs.x0, cs.rhs, kmax, np.float64, **kw).xs
    good = run()
    for k in cs.ks:
        assert cref.ratio(good[k - 1], cs, k) <= 1.0, k
    scaled = cref.ratio(run(alpha_scale=1.0 + 1e-12)[0], cs, 1)
    print("%s/%s: alpha_0 (1 + 1e-12): error / allowance %.3g at k = 1" % (name, start, scaled))
    assert scaled > 1.0
    nnz = cs.coo.i.size
    dropped = run(drop=nnz // 2)
    for k in cs.ks:
        rat = cref.ratio(dropped[k - 1], cs, k)
        print("%s/%s: entry %d of %d left out: error / allowance %.3g at k = %d" % (name, start, nnz // 2, nnz, rat, k))
        assert rat > 1.0, k
