"""
direct = true: the transitions between its forms on ONE handle (csrc/direct.cpp, the table at its top).  A fixed sequence of enable / disable calls; after
every call the form, the order of the stored inverse, whether a set-up ran (direct_setup_s changed) and one projection against the oracle's IndAffineDirect.

The expected (form, order, set-up ran) triples are literals: they are what the library reported for the same sequence BEFORE the form state became one enum
(commit 0904590, four booleans; its report: profiles/direct_refactor_sequences.txt), so the test pins the transitions of that version, the odd ones included:
  * AUTO on a handle that stores a dense inverse or a ready block form returns to it at once (no set-up, whatever FOS_DIRECT_MODE says),
  * REDUCED releases the dense inverse (AUTO after it sets the dense form up again) but leaves the block form's data in place,
  * AUTO after REDUCED releases the reduced data (REDUCED after it sets up again),
  * another factor rebuilds the stored dense inverse.
"""
import numpy as np
import pytest
import scipy.sparse as sp

import fos_oracle as orc
from test_gpu_direct_reduced import _rect_problem

pytestmark = pytest.mark.gpu


def _block_problem(pkg, seed=11):
    """block-diagonal A: three blocks of four columns each (I + A'A: three diagonal blocks of order 4 -> the block form)"""
    rng = np.random.default_rng(seed)
    A = sp.block_diag([sp.csc_matrix(rng.standard_normal((6, 4))) for _ in range(3)], format="csc")
    A.sort_indices()
    m, n = A.shape
    x0, s0 = np.abs(rng.standard_normal(n)), np.abs(rng.standard_normal(m))
    return pkg.workloads.ConicProblem("blocks-3x4", A, A @ x0 + s0, rng.standard_normal(n), [("NonNeg", m)], [("NonNeg", n)], x0=x0, y0=np.zeros(m), s0=s0)


OPERATORS = {
    "lp_40x30": lambda pkg: _rect_problem(pkg, 40, 30, 5),       # l = 71 (dense inverse padded to 128), reduced order 30 (padded to 64); n <= 64: AUTO takes the block form
    "lp_90x70": lambda pkg: _rect_problem(pkg, 90, 70, 6),       # l = 161 (padded to 192), reduced order 70: past one 64 tile
    "blocks_3x4": _block_problem,
}

SEQUENCE = [("enable", "auto", "newton"), ("disable",), ("enable", "auto", "newton"), ("enable", "reduced", "newton"), ("enable", "auto", "newton"),
            ("enable", "auto", "cholesky"), ("enable", "reduced", "cholesky"), ("disable",)]

# (direct_mode(), direct_stats()["k"], a set-up ran) after each call of SEQUENCE, as reported by commit 0904590
EXPECTED = {
    "lp_40x30": [("block", 0, True), ("off", 0, False), ("block", 0, False), ("reduced", 30, True), ("block", 0, False),
                 ("block", 0, False), ("reduced", 30, True), ("off", 0, False)],
    "lp_90x70": [("dense", 161, True), ("off", 0, False), ("dense", 161, False), ("reduced", 70, True), ("dense", 161, True),
                 ("dense", 161, True), ("reduced", 70, True), ("off", 0, False)],
    "blocks_3x4": [("block", 0, True), ("off", 0, False), ("block", 0, False), ("reduced", 12, True), ("block", 0, False),
                   ("block", 0, False), ("reduced", 12, True), ("off", 0, False)],
}
# lp_40x30 with FOS_DIRECT_MODE=dense set for the whole sequence (its 30 columns are one block of A'A, so AUTO alone never reaches the dense form at l = 71)
EXPECTED_DENSE_71 = [("dense", 71, True), ("off", 0, False), ("dense", 71, False), ("reduced", 30, True), ("dense", 71, True),
                     ("dense", 71, True), ("reduced", 30, True), ("off", 0, False)]
# FOS_DIRECT_MODE=cg on lp_40x30: on a fresh handle; on a handle that stores a dense inverse (built under FOS_DIRECT_MODE=dense; disable, then enable under cg)
EXPECTED_CG_FRESH = [("cg", 0, True)]
EXPECTED_CG_STORED = [("dense", 71, True), ("off", 0, False), ("dense", 71, False)]

_CACHE = {}


def _case(pkg, name):
    """problem, fixed input, the oracle's projection of it and the condition number of I + Q Q' -- computed once per operator"""
    if name not in _CACHE:
        prob = OPERATORS[name](pkg)
        S1 = orc.IndAffineDirect(orc.HSDEMatrixQ(prob.A, prob.b, prob.c))
        l = sum(prob.A.shape) + 1
        x = np.random.default_rng(9).standard_normal(2 * l)
        ref = np.empty(2 * l)
        S1.prox(ref, x)
        x.setflags(write=False)
        ref.setflags(write=False)
        _CACHE[name] = (prob, x, ref, float(np.linalg.cond(np.eye(l) + S1.Qd @ S1.Qd.T)))
    return _CACHE[name]


def _check_projection(d, x, ref, cond):
    """one projection against the oracle at the tolerance tests/test_gpu_direct.py uses for the form the handle is in"""
    mode = d.direct_mode()
    if mode in ("dense", "block", "reduced"):
        y = d.prox_affine(x)
        assert d.cgiter() == 0
        err, tol = np.linalg.norm(y - ref), 1e-12 * np.linalg.norm(ref) * max(1.0, cond / 1e3)
    elif mode == "cg":                                        # the tolerance floor from the first call on
        y = d.prox_affine(x)
        assert d.cgiter() > 0
        err, tol = np.linalg.norm(y - ref), 1e-9 * np.linalg.norm(ref)
    else:                                                     # off: AffinePlusLinear's schedule, advanced to its floor
        d.reset_affine()
        for _ in range(400):
            y = d.prox_affine(x)
        err, tol = np.linalg.norm(y - ref), 1e-9 * np.linalg.norm(ref)
    print("   ", mode, "projection error", err, "bound", tol)
    assert err <= tol, (mode, err, tol)


def run_sequence(d, A, sequence, check=None):
    """[(mode, order, set-up ran)] after every call of `sequence` on handle d; check(d) runs after each call"""
    out = []
    for call in sequence:
        before = d.direct_stats()["setup_s"]
        if call[0] == "enable":
            d.enable_direct(A, form=call[1], factor=call[2])
        else:
            d.disable_direct()
        st = d.direct_stats()
        assert st["form"] == d.direct_mode()
        out.append((d.direct_mode(), st["k"], st["setup_s"] != before))
        print(call, "->", out[-1])
        if check:
            check(d)
    return out


@pytest.mark.parametrize("name", list(OPERATORS))
def test_form_transitions_on_one_handle(pkg, name, monkeypatch):
    monkeypatch.delenv("FOS_DIRECT_MODE", raising=False)
    prob, x, ref, cond = _case(pkg, name)
    d = pkg.HipHSDE(prob.A, prob.b, prob.c, prob.K1, prob.K2)
    got = run_sequence(d, prob.A, SEQUENCE, lambda d: _check_projection(d, x, ref, cond))
    d.close()
    assert got == EXPECTED[name]


def test_form_transitions_with_the_dense_form_forced(pkg, monkeypatch):
    monkeypatch.setenv("FOS_DIRECT_MODE", "dense")
    prob, x, ref, cond = _case(pkg, "lp_40x30")
    d = pkg.HipHSDE(prob.A, prob.b, prob.c, prob.K1, prob.K2)
    got = run_sequence(d, prob.A, SEQUENCE, lambda d: _check_projection(d, x, ref, cond))
    d.close()
    assert got == EXPECTED_DENSE_71


def test_mode_cg_on_a_fresh_handle(pkg, monkeypatch):
    prob, x, ref, cond = _case(pkg, "lp_40x30")
    monkeypatch.setenv("FOS_DIRECT_MODE", "cg")
    d = pkg.HipHSDE(prob.A, prob.b, prob.c, prob.K1, prob.K2)
    got = run_sequence(d, prob.A, SEQUENCE[:1], lambda d: _check_projection(d, x, ref, cond))
    d.close()
    assert got == EXPECTED_CG_FRESH


def test_mode_cg_on_a_handle_that_stores_an_inverse(pkg, monkeypatch):
    """the stored dense inverse wins over FOS_DIRECT_MODE=cg: AUTO returns to it at once"""
    prob, x, ref, cond = _case(pkg, "lp_40x30")
    monkeypatch.setenv("FOS_DIRECT_MODE", "dense")
    d = pkg.HipHSDE(prob.A, prob.b, prob.c, prob.K1, prob.K2)
    check = lambda d: _check_projection(d, x, ref, cond)
    got = run_sequence(d, prob.A, SEQUENCE[:2], check)
    monkeypatch.setenv("FOS_DIRECT_MODE", "cg")
    got += run_sequence(d, prob.A, SEQUENCE[:1], check)
    d.close()
    assert got == EXPECTED_CG_STORED
