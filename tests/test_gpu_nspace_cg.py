"""
GPU: the cg forms -- Quadratic(Q, q, form="cg") and LeastSquares(A, b, lam, form="cg") (csrc/nspace_cg.hip) -- through a handle: the cases of
tests/test_nspace_cg_cpu.py at the error bar derived in tests/nspace_cg_cases.py, device against host emulation at TOL max(1, |y|_inf), the launch budget (two
resp. three launches per CG iteration), the warm start and its reset, the shapes the kept-inverse forms refuse, tol, set_set on a live handle, and DR end to end
on a box QP and a lasso against the handles built on the dense resp. form="normal" objects.

LeastSquares with tall_sparse(120 000, 50 000, 3) was to be held against scipy.sparse.linalg.splu.  splu of I + lam A'A at that shape -- a random graph of mean
degree 6 on 50 000 nodes, 362 268 stored entries -- did not finish within 25 minutes (COLAMD; the factor fills in), which no test can take.  The case, the shape and
the bar are kept; the reference is nspace_cg_cases.certified_ls (scipy CG refined on a longdouble residual, 3 s), whose own error is BOUNDED by its last longdouble
residual (lambda_min >= 1) and asserted to be below a thousandth of the bar, and which is held against splu_ls at (6 000, 2 500), where splu can run.
"""
import numpy as np
import pytest
import scipy.sparse as sp

import nspace_cases as nc
import nspace_cg_cases as cg
from feasibility_cases import ALGS
from nspace_cases import LAMS, TOL
from prox_fn_cases import RefLeastSquares, lasso_kkt

pytestmark = pytest.mark.gpu


def _handle(pkg, S, n):
    return pkg.HipFeasibility(pkg.Feasibility(S, pkg.IndFree(), n))


def _held(tag, y, yref, bar, st):
    err = float(np.linalg.norm(y - yref))
    print("%s: |y - ref|_2 = %.2e (bar %.2e), %d CG iterations, %d restarts, |r| = %.2e, level %.2e" %
          (tag, err, bar, st["last_iters"], st["last_restarts"], st["last_resid"], st["last_level"]))
    assert err <= bar, (tag, err, bar)


def _agree(tag, y, yh):
    d, s = float(np.abs(y - yh).max()), max(1.0, float(np.abs(yh).max()))
    print("%s: |device - host emulation| = %.2e (bar %.2e)" % (tag, d, TOL * s))
    assert d <= TOL * s, (tag, d)


@pytest.mark.parametrize("name", cg.QUAD_CASES)
def test_quadratic_cases_through_a_handle(pkg, name):
    Q, q, x = cg.quadratic_case(name)
    n = Q.shape[0]
    d = _handle(pkg, pkg.Quadratic(Q, q, form="cg"), n)
    y = d.prox(1, x)
    st = d.nspace_cg_stats(1)
    ref = cg.quadratic_ref(name)
    _held("Quadratic " + name, y, ref, cg.quadratic_bar(Q, q, x, ref), st)
    assert st["launches_per_iter"] <= 2 and st["calls"] == 1 and st["iters_total"] == st["last_iters"], st
    P = sp.csc_matrix(cg.sym_lower(Q))
    P.data[:] = 1.0
    assert st["stored"] == (P + sp.identity(n)).nnz, st                          # I + Q mirrored, the unit diagonal included
    rc, yh, iters = cg.host_quadratic_cg(pkg, Q, q, x)
    assert rc == 0
    _agree("Quadratic " + name, y, yh)
    print("Quadratic %s: %d CG iterations on the device, %d in the host emulation" % (name, st["last_iters"], iters))
    if name in cg.TINY:
        assert st["last_iters"] <= cg.TINY[name] + cg.SMALL, st
    d.close()


@pytest.mark.parametrize("name", cg.LS_CASES)
def test_least_squares_cases_through_a_handle(pkg, name):
    A, b, x = cg.ls_case(name)
    n = A.shape[1]
    for lam in LAMS:
        d = _handle(pkg, pkg.LeastSquares(A, b, lam, form="cg"), n)
        y = d.prox(1, x)
        st = d.nspace_cg_stats(1)
        ref = cg.ls_ref(name, lam)
        _held("LeastSquares %s lam %g" % (name, lam), y, ref, cg.ls_bar(A, b, lam, x, ref), st)
        assert st["launches_per_iter"] <= 3 and st["stored"] == 2 * A.nnz, st
        rc, yh, iters = cg.host_ls_cg(pkg, A, b, lam, x)
        assert rc == 0
        _agree("LeastSquares %s lam %g" % (name, lam), y, yh)
        if name in cg.TINY:
            assert st["last_iters"] <= cg.TINY[name] + cg.SMALL, st
        d.close()


def test_warm_start_and_reset(pkg):
    Q, q, x = cg.quadratic_case("tridiag300")
    n = Q.shape[0]
    d = _handle(pkg, pkg.Quadratic(Q, q, form="cg"), n)
    cold = d.prox(1, x)
    cold_iters = d.nspace_cg_stats(1)["last_iters"]
    assert cold_iters > 0
    again = d.prox(1, x)                                                       # from its own answer: the recomputed residual is already at its level
    st = d.nspace_cg_stats(1)
    assert st["last_iters"] == 0 and again.tobytes() == cold.tobytes() and st["calls"] == 2, st
    delta = np.random.default_rng(5).standard_normal(n)
    x2 = x + 1e-6 * delta
    y2 = d.prox(1, x2)
    warm_iters = d.nspace_cg_stats(1)["last_iters"]
    print("tridiag300: %d CG iterations cold, %d warm at x + 1e-6 delta" % (cold_iters, warm_iters))
    assert 0 < warm_iters < cold_iters
    ref2 = nc.RefQuadratic(cg.sym_lower(Q).toarray(), q).project(x2)
    assert np.linalg.norm(y2 - ref2) <= cg.quadratic_bar(Q, q, x2, ref2)
    d.set_iterate(None)                                                        # a new solve: cold again, the same bits as the first prox
    back = d.prox(1, x)
    st = d.nspace_cg_stats(1)
    assert back.tobytes() == cold.tobytes() and st["last_iters"] == cold_iters, st
    # the same on a LeastSquares
    A, b, xa = cg.ls_case("dup_rows")
    d.close()
    d = _handle(pkg, pkg.LeastSquares(A, b, 1.0, form="cg"), A.shape[1])
    cold = d.prox(1, xa)
    cold_iters = d.nspace_cg_stats(1)["last_iters"]
    assert d.prox(1, xa).tobytes() == cold.tobytes() and d.nspace_cg_stats(1)["last_iters"] == 0
    d.prox(1, xa + 1e-6 * np.random.default_rng(6).standard_normal(A.shape[1]))
    assert d.nspace_cg_stats(1)["last_iters"] < cold_iters
    d.set_iterate(None)
    assert d.prox(1, xa).tobytes() == cold.tobytes() and d.nspace_cg_stats(1)["last_iters"] == cold_iters
    d.close()


def test_quadratic_past_the_dense_limit(pkg):
    n = 50000
    Q, q, x = cg.pentadiagonal(n)
    with pytest.raises(ValueError, match="Quadratic: Q must be dense"):          # what form=None still says to a sparse Q
        pkg.Quadratic(Q, q)
    d = _handle(pkg, pkg.Quadratic(Q, q, form="cg"), n)
    y = d.prox(1, x)
    st = d.nspace_cg_stats(1)
    ref = cg.splu_quadratic(Q, q, x)
    _held("Quadratic pentadiagonal n = %d" % n, y, ref, cg.quadratic_bar(Q, q, x, ref), st)
    assert st["launches_per_iter"] == 2 and st["stored"] == 5 * n - 6, st
    assert d.prox(1, x).tobytes() == y.tobytes()
    d.close()


def test_least_squares_past_the_dense_limit(pkg):
    m, n, lam = 120000, 50000, 1.0
    A, b = nc.tall_sparse(m, n, 3)
    x = np.random.default_rng(3).standard_normal(n)
    with pytest.raises(ValueError, match="46000"):                               # form="normal" still refuses it
        pkg.LeastSquares(A, b, lam, form="normal")
    with pytest.raises(ValueError):                                            # and so does form="sparse_factored" (m > n)
        pkg.LeastSquares(A, b, lam, form="sparse_factored")
    As, bs = nc.tall_sparse(6000, 2500, 3)                                    # the reference of the large case against splu where splu can run
    xs = x[:2500]
    ys, es = cg.certified_ls(As, bs, lam, xs)
    assert np.linalg.norm(ys - cg.splu_ls(As, bs, lam, xs)) <= 1e-3 * cg.ls_bar(As, bs, lam, xs, ys) and es <= 1e-3 * cg.ls_bar(As, bs, lam, xs, ys)
    ref, e = cg.certified_ls(A, b, lam, x)
    bar = cg.ls_bar(A, b, lam, x, ref)
    print("the reference's own error is at most %.2e (bar %.2e)" % (e, bar))
    assert e <= 1e-3 * bar
    d = _handle(pkg, pkg.LeastSquares(A, b, lam, form="cg"), n)
    y = d.prox(1, x)
    st = d.nspace_cg_stats(1)
    _held("LeastSquares tall_sparse(%d, %d, 3)" % (m, n), y, ref, bar, st)
    assert st["launches_per_iter"] == 3 and st["stored"] == 2 * A.nnz, st
    assert d.prox(1, x).tobytes() == y.tobytes()
    d.close()


def test_tol_ends_earlier_at_its_looser_bar(pkg):
    Q, q, x = cg.quadratic_case("tridiag300")
    n = Q.shape[0]
    ref = cg.quadratic_ref("tridiag300")
    d = _handle(pkg, pkg.Quadratic(Q, q, form="cg"), n)
    d.prox(1, x)
    it0 = d.nspace_cg_stats(1)["last_iters"]
    d.set_set(1, pkg.Quadratic(Q, q, form="cg", tol=1e-8))
    y8 = d.prox(1, x)
    st = d.nspace_cg_stats(1)
    _held("Quadratic tridiag300 tol 1e-8", y8, ref, cg.quadratic_bar(Q, q, x, ref, tol=1e-8), st)
    assert 0 < st["last_iters"] < it0, (st, it0)
    assert st["last_resid"] <= 1e-8 * np.linalg.norm(x - q)
    d.close()


def test_set_set_on_a_live_handle(pkg):
    Q, q, x = cg.quadratic_case("n65")
    n = 65
    Qd = cg.sym_lower(Q).toarray()
    ref = cg.quadratic_ref("n65")
    d = _handle(pkg, pkg.Quadratic(Qd, q), n)                                   # the dense Quadratic ...
    assert np.abs(d.prox(1, x) - ref).max() <= nc.bar(np.eye(n) + Qd, x, ref) and d.nspace_stats(1)["n"] == n
    with pytest.raises(pkg.lib.FosError):
        d.nspace_cg_stats(1)                                                   # (another kind: FOS_EINVAL)
    d.set_set(1, pkg.Quadratic(Q, q, form="cg"))                               # ... -> the cg Quadratic ...
    y = d.prox(1, x)
    _held("set_set: Quadratic cg", y, ref, cg.quadratic_bar(Q, q, x, ref), d.nspace_cg_stats(1))
    with pytest.raises(pkg.lib.FosError):
        d.nspace_stats(1)
    lib = pkg.lib.load()                                                       # a refused set-up leaves the object in place
    keep, ptrs = nc.csc_ptrs(pkg, Q)
    bad = keep[2].copy(); bad[0] = np.nan
    assert lib.fos_feas_set_quadratic_sparse(d._h, 1, ptrs[0], ptrs[1], pkg.lib.dptr(bad), pkg.lib.dptr(q), 0.0) == cg.FOS_EINVAL
    assert lib.fos_feas_set_quadratic_sparse(d._h, 1, ptrs[0], ptrs[1], ptrs[2], pkg.lib.dptr(q), 1.5) == cg.FOS_EINVAL
    assert lib.fos_feas_set_quadratic_sparse(d._h, 3, ptrs[0], ptrs[1], ptrs[2], pkg.lib.dptr(q), 0.0) == cg.FOS_EINVAL
    assert d.prox(1, x).tobytes() == y.tobytes() and d.nspace_cg_stats(1)["last_iters"] == 0
    with pytest.raises(ValueError):
        d.set_set(1, pkg.Quadratic(Q[:50, :50], q[:50], form="cg"))             # the wrong order
    A, b = nc.tall_sparse(500, n, 3)
    d.set_set(1, pkg.LeastSquares(A, b, 0.7, form="cg"))                       # ... -> the cg LeastSquares
    refa = RefLeastSquares(A.toarray(), b, 0.7).project(x)
    _held("set_set: LeastSquares cg", d.prox(1, x), refa, cg.ls_bar(A, b, 0.7, x, refa), d.nspace_cg_stats(1))
    assert d.nspace_cg_stats(1)["launches_per_iter"] == 3 and d.nspace_cg_stats(1)["calls"] == 1
    ind = sp.csc_matrix((np.array([3.0, 3.0]), (np.array([1, 0]), np.array([0, 1]))), shape=(n, n))      # indefinite, zero diagonal: the PROX meets p'(I + Q)p <= 0
    d.set_set(1, pkg.Quadratic(ind, np.zeros(n), form="cg"))
    xi = np.zeros(n); xi[0], xi[1] = 1.0, -1.0
    with pytest.raises(pkg.lib.FosError, match="positive semidefinite"):
        d.prox(1, xi)
    d.set_set(1, pkg.Quadratic(Q, q, form="cg"))                               # and the handle goes on working
    assert d.prox(1, x).tobytes() == y.tobytes()
    assert d._callbacks == []
    d.close()


STEPS = 100


def _run_dr(pkg, S1, S2, n):
    d = pkg.HipFeasibility(pkg.Feasibility(S1, S2, n))
    d.set_alg(ALGS["DR"](pkg))
    d.set_iterate(None)
    assert d.step(1, STEPS, 10 * STEPS, 1e-30)[0] == STEPS
    return d, d.get_iterate()


def test_box_qp_end_to_end(pkg):
    """DR on Quadratic(Q, q, form="cg") n IndBox(0, 1), n = 2 000, against the handle built on the dense Quadratic: after STEPS = 100 steps the iterates agree to
    100 x the prox bar (the two differ only in their prox errors, DR is nonexpansive, so k steps accumulate at most k prox errors of each), and the projected-gradient
    residual of the QP is the one the dense handle reaches, up to the Lipschitz constant 2 + |Q|_inf of that residual times the same distance."""
    n = 2000
    rng = np.random.default_rng(21)
    Q = cg._sym_psd(n, rng)
    q = rng.standard_normal(n)
    box = pkg.IndBox(0.0, 1.0)
    dd, zd = _run_dr(pkg, pkg.Quadratic(Q.toarray(), q), box, n)
    dc, zc = _run_dr(pkg, pkg.Quadratic(Q, q, form="cg"), box, n)
    st = dc.nspace_cg_stats(1)
    yd = dd.prox(1, zd)
    bar = cg.quadratic_bar(Q, q, zd, yd)
    dist = float(np.linalg.norm(zc - zd))
    print("box QP, %d DR steps: |z_cg - z_dense|_2 = %.2e (100 x prox bar = %.2e), %d prox calls, %.1f CG iterations per prox" %
          (STEPS, dist, 100 * bar, st["calls"], st["iters_total"] / st["calls"]))
    assert dist <= 100 * bar
    Qd = Q.toarray()
    rd = nc.box_qp_residual(Qd, q, 0.0, 1.0, np.clip(yd, 0.0, 1.0))
    rc = nc.box_qp_residual(Qd, q, 0.0, 1.0, np.clip(dc.prox(1, zc), 0.0, 1.0))
    print("box QP: projected-gradient residual %.3e (cg), %.3e (dense)" % (rc, rd))
    assert abs(rc - rd) <= (2.0 + float(abs(Q).sum(axis=1).max())) * 100 * bar
    assert dc._callbacks == []
    dd.close(); dc.close()


def test_lasso_end_to_end(pkg):
    """DR on LeastSquares(A, b, lam, form="cg") n NormL1(mu) at (3 000, 400) against the handle built on form="normal": the same two assertions, lasso_kkt in place
    of the projected-gradient residual (its gradient part has the Lipschitz constant lam |A'A|_inf; both supports are asserted equal)."""
    m, n, lam, mu = 3000, 400, 0.7, 0.5
    A, b = nc.tall_sparse(m, n, 3)
    dn, zn = _run_dr(pkg, pkg.LeastSquares(A, b, lam, form="normal"), pkg.NormL1(mu), n)
    dc, zc = _run_dr(pkg, pkg.LeastSquares(A, b, lam, form="cg"), pkg.NormL1(mu), n)
    st = dc.nspace_cg_stats(1)
    yn = dn.prox(1, zn)
    bar = cg.ls_bar(A, b, lam, zn, yn)
    dist = float(np.linalg.norm(zc - zn))
    print("lasso, %d DR steps: |z_cg - z_normal|_2 = %.2e (100 x prox bar = %.2e), %d prox calls, %.1f CG iterations per prox" %
          (STEPS, dist, 100 * bar, st["calls"], st["iters_total"] / st["calls"]))
    assert dist <= 100 * bar
    yc = dc.prox(1, zc)
    assert np.array_equal(np.abs(yc) > 1e-6, np.abs(yn) > 1e-6)
    Ad = A.toarray()
    kn, kc = lasso_kkt(Ad, b, lam, mu, yn), lasso_kkt(Ad, b, lam, mu, yc)
    print("lasso: lasso_kkt %.3e (cg), %.3e (normal)" % (kc, kn))
    assert abs(kc - kn) <= lam * float(abs(A.T @ A).sum(axis=1).max()) * 100 * bar
    assert dc._callbacks == []
    dn.close(); dc.close()
