"""
CPU: the LongstepWrapper's projection onto the saved planes (csrc/wrappers.cpp: the small dual in 113-bit arithmetic) through the host entry
fos_host_long_project -- the function the device path calls between reading the Gram sums and writing the multipliers -- against the oracle's
project_onto_planes (60 digits, itself checked against SLSQP by test_longstep_oracle.py).
"""
import functools

import numpy as np
import pytest

from feasibility_cases import affine_box_instance

# Worst relative disagreement max |x_out - v| / max(1, max |v|) with the oracle over the cases below, measured on the CPU: 0.0 in every case, the 22 rows at
# cond 1e10 included -- both sides solve in far more than 53 bits and round the result once, so they return the same doubles.  The bound is 16 times the measured
# value, and never more than the project's same-step tolerance of 1e-9 (a larger disagreement is a finding, not a tolerance): 16 x 0.0, bit-for-bit agreement.
# (The first disagreement the format can show is one unit of the last place, 2.2e-16: another compiler's summation order of G in __float128 would have to move a
# result across a rounding boundary of a double to produce it.)
MEASURED = 0.0
TOL = min(16 * MEASURED, 1e-9)


def _seeded(seed):
    """the cases of test_projection_onto_planes_matches_slsqp, the duplicated plane of every third seed included"""
    rng = np.random.default_rng(seed)
    n, ne, ni = int(rng.integers(8, 40)), int(rng.integers(1, 5)), int(rng.integers(1, 5))
    A, C, x, v0 = rng.standard_normal((ne, n)), rng.standard_normal((ni, n)), rng.standard_normal(n), rng.standard_normal(n)
    b = A @ v0
    d = C @ v0 - rng.random(ni) * (rng.random(ni) < 0.6)
    if seed % 3 == 0:
        A = np.vstack([A, A[:1]])
        b = np.concatenate([b, b[:1]])
    return A, b, C, d, x


def _built(ne, ni, n, active, seed):
    """a projection whose answer is known by construction: v = x + A'lam + C'mu with mu > 0 exactly on `active`, the other inequalities slack at v"""
    rng = np.random.default_rng(seed)
    A, C, v = rng.standard_normal((ne, n)), rng.standard_normal((ni, n)), rng.standard_normal(n)
    mu = np.zeros(ni)
    mu[list(active)] = 0.3 + rng.random(len(active))
    slack = 0.5 + rng.random(ni)
    slack[list(active)] = 0.0
    return A, A @ v, C, C @ v - slack, v - A.T @ rng.standard_normal(ne) - C.T @ mu


def _zero_row():
    """GAP's plane of an inactive bound: an inequality row that is exactly zero (0 v >= 0)"""
    A, b, C, d, x = _seeded(1)
    return A, b, np.vstack([C[:1], np.zeros((1, C.shape[1])), C[1:]]), np.concatenate([d[:1], [0.0], d[1:]]), x


def _saved_planes():
    """The 22 nearly dependent rows (sigma_max / sigma_min ~ 1e10) the oracle's own LongstepWrapper(AP, 25, 10) hands to its first projection on
    affine_box_instance(50, 100): the situation of test_default_nsave_projection_is_extended_precision."""
    import fos_oracle as orc
    A, b = affine_box_instance(m=50, n=100)
    owrap = orc.LongstepWrapper(orc.AP(), longinterval=25, nsave=10)
    omodel = orc.FeasibilityModel(orc.Feasibility(orc.IndAffine(A, b), orc.IndBox(0.0, np.inf), 100), owrap)
    ost = orc.FeasibilityStatus(omodel, 10 ** 9, 1e-30, 0, 1)
    got, orig = [], orc.project_onto_planes

    def hook(A_, b_, C_, d_, x_, tol=1e-12):
        got.append((A_.copy(), b_.copy(), C_.copy(), d_.copy(), x_.copy()))
        return x_.copy(), 0.0                                       # (the planes are what is wanted; the projection itself is computed once, in _reference)
    xo = np.zeros(100)
    try:
        orc.project_onto_planes = hook
        for i in range(1, 26):
            ost.i = i
            owrap.step(xo, i, ost)
    finally:
        orc.project_onto_planes = orig
    assert len(got) == 1 and got[0][0].shape[0] + got[0][2].shape[0] == 22
    return got[0]


CASES = {**{"seed%d" % s: functools.partial(_seeded, s) for s in range(8)},
         "K=2": functools.partial(_built, 1, 1, 9, (0,), 11),
         "K=32": functools.partial(_built, 16, 16, 67, (5,), 12),
         "zero-row": _zero_row,
         "saved-planes": _saved_planes}


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(the planes, the oracle's v, the size of its support) -- computed once per case and left unchanged"""
    import fos_oracle as orc
    import mpmath
    A, b, C, d, x = CASES[name]()
    # the oracle tries the supports smallest first and stops at the first KKT point: the order of its last eigen-decomposition is neq + |support|
    orders, eigsy = [], mpmath.eigsy
    try:
        mpmath.eigsy = lambda M, *a, **k: (orders.append(M.rows), eigsy(M, *a, **k))[1]
        v, viol = orc.project_onto_planes(A, b, C, d, x)
    finally:
        mpmath.eigsy = eigsy
    assert viol <= 1e-10
    return (A, b, C, d, x), v, orders[-1] - A.shape[0]


def _project(pkg, A, b, C, d, x, max_supports=4096):
    lib = pkg.lib.load()
    P = np.ascontiguousarray(np.vstack([A, C]), dtype=np.float64)
    beta = np.ascontiguousarray(np.concatenate([b, d]), dtype=np.float64)
    x = np.ascontiguousarray(x, dtype=np.float64)
    out, log = np.full(x.size, np.nan), np.zeros(8)
    rc = lib.fos_host_long_project(x.size, A.shape[0], C.shape[0], pkg.lib.dptr(P), pkg.lib.dptr(beta), pkg.lib.dptr(x), max_supports, pkg.lib.dptr(out), pkg.lib.dptr(log))
    assert rc == 0, lib.fos_last_error()
    return out, dict(active=int(log[1]), violation=log[2], step=log[3], rows=int(log[4]), tried=int(log[5]), failed=bool(log[6]), given_up=int(log[7]))


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_projection_matches_oracle(pkg, name):
    """x_out against the oracle's v at TOL = 16 x the worst measured relative disagreement (measured: 0.0 in all twelve cases, so the doubles must be equal);
    the support, the budget and |x_out - x| from the log."""
    (A, b, C, d, x), v, support = _reference(name)
    out, log = _project(pkg, A, b, C, d, x)
    err = np.abs(out - v).max() / max(1.0, np.abs(v).max())
    print("%s: K = %d, active %d (oracle %d), tried %d, relative disagreement %.2e (bound %.2e)" % (name, log["rows"], log["active"], support, log["tried"], err, TOL))
    assert not log["failed"] and log["given_up"] == 0
    assert log["rows"] == A.shape[0] + C.shape[0]
    assert log["active"] == support
    assert log["tried"] <= 4096
    assert err <= TOL, (name, err)
    assert log["step"] == pytest.approx(np.linalg.norm(v - x), rel=1e-9, abs=1e-300)


@pytest.mark.parametrize("name", ["K=32", "seed3"])
def test_a_budget_of_zero_supports_leaves_x(pkg, name):
    A, b, C, d, x = CASES[name]()
    out, log = _project(pkg, A, b, C, d, x, max_supports=0)
    assert log["failed"] and log["tried"] == 0 and log["step"] == 0.0 and log["given_up"] == 1
    assert out.tobytes() == np.ascontiguousarray(x, dtype=np.float64).tobytes()          # bit for bit


def test_bad_arguments_are_refused(pkg):
    lib = pkg.lib.load()
    z = np.zeros(40 * 4)
    for n, neq, nin in ((4, 17, 16), (4, 0, 0), (0, 1, 1), (4, 1, 17)):
        assert lib.fos_host_long_project(n, neq, nin, pkg.lib.dptr(z), pkg.lib.dptr(z), pkg.lib.dptr(z), 10, pkg.lib.dptr(z), pkg.lib.dptr(z)) == -1, (n, neq, nin)
