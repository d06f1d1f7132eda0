"""
GPU: the n-space forms -- Quadratic(Q, q) and LeastSquares(form="normal"), dense and sparse (csrc/nspace.hip) -- and the sparse wide LeastSquares
(form="sparse_factored", csrc/affine_sparse_factored.hip) through a handle: the shapes of tests/test_nspace_cpu.py at the bar of tests/nspace_cases.py with both
factors, the fixed launch count, bit-identical repeats, device against host emulation on every family (the column-scaled one included, which is held to nothing
else), set_set sequences and refusals, and the iterates of a tall lasso and of a box QP against the oracle and the device's own callback path.

Device against host emulation: TOL max(1, |y|_inf).  The host entries emulate the Cholesky factor, rounding as the device does (the Gram sums, the scaling, the
blocked Cholesky inverse and the tile products: one fused operation per multiply-add, k ascending), so the n-space forms agree to the bit in practice; handles
built with factor="newton" are held to the reference's bar only.
"""
import numpy as np
import pytest
import scipy.sparse as sp

import nspace_cases as nc
from feasibility_cases import ALGS
from nspace_cases import FOS_EINVAL, LAMS, SHAPES, TOL
from prox_fn_cases import RefLeastSquares, RefNormL1, lasso_kkt
from set_cases import RefBox
from sparse_factored_cases import RAND_SHAPES, rand, seg64_cases

pytestmark = pytest.mark.gpu


def _handle(pkg, S, n):
    return pkg.HipFeasibility(pkg.Feasibility(S, pkg.IndFree(), n))


def _agree(tag, y, yh):
    d, s = float(np.abs(y - yh).max()), max(1.0, float(np.abs(yh).max()))
    print("%s: |device - host emulation| = %.2e (bar %.2e)" % (tag, d, TOL * s))
    assert d <= TOL * s, (tag, d)


def _stats_ok(st, n, m, factor):
    assert (st["n"], st["m"], st["launches"], st["fell_back"]) == (n, m, 6, 0), st
    assert st["factor"] == factor and st["probe_resid"] <= 1e-7 and st["tiles"] == ((n + 63) // 64) * ((n + 63) // 64 + 1) and st["bytes"] >= 2 * st["tiles"] * 16384, st


@pytest.mark.parametrize("factor", ["cholesky", "newton"])
@pytest.mark.parametrize("m,n", SHAPES)
def test_dense_shapes_through_a_handle(pkg, m, n, factor):
    A, b = nc.instance("gauss", m, n)
    rng = np.random.default_rng(m + n)
    x = rng.standard_normal(n)
    for lam in LAMS:
        M = np.eye(n) + lam * (A.T @ A)
        d = _handle(pkg, pkg.LeastSquares(A, b, lam, factor=factor, form="normal"), n)
        _stats_ok(d.nspace_stats(1), n, m, factor)
        y = d.prox(1, x)
        ref = RefLeastSquares(A, b, lam).project(x)
        err, bar = np.abs(y - ref).max(), nc.bar(M, x, ref)
        print("LeastSquares (%d, %d) lam %g %s: |y - ref| = %.2e (bar %.2e)" % (m, n, lam, factor, err, bar))
        assert err <= bar
        assert d.prox(1, x).tobytes() == y.tobytes()                           # every sum has a fixed order: the same bits
        if factor == "cholesky":                                               # (the path the host entry emulates)
            _agree("LeastSquares (%d, %d) lam %g" % (m, n, lam), y, nc.host_ls_normal(pkg, A, b, lam, x)[1])
        Q, q = nc.quadratic_of(A, b, lam)
        d.set_set(1, pkg.Quadratic(Q, q, factor=factor))                       # replaces the LeastSquares on the same handle
        _stats_ok(d.nspace_stats(1), n, 0, factor)
        yq = d.prox(1, x)
        refq = nc.RefQuadratic(Q, q).project(x)
        errq, barq = np.abs(yq - refq).max(), nc.bar(np.eye(n) + Q, x, refq)
        print("Quadratic n = %d lam %g %s: |y - ref| = %.2e (bar %.2e)" % (n, lam, factor, errq, barq))
        assert errq <= barq and d.prox(1, x).tobytes() == yq.tobytes()
        if factor == "cholesky":
            _agree("Quadratic n = %d lam %g" % (n, lam), yq, nc.host_quadratic(pkg, Q, q, x)[1])
        d.close()


@pytest.mark.parametrize("family,m,n", nc.EXTRA + [("cols", 1000, 200)])
def test_other_families_and_the_column_scaled_one(pkg, family, m, n):
    """Every family at every lambda: the reference's bar (not `cols`), the same bits twice, and device against host emulation at TOL max(1, |y|_inf).  The
    last check is the sharp one at lambda = 1e3 of `rankdef` (|K|_2 ~ 1e5) and of `cols` (lam A'b five orders above the answer it cancels to): there a last-bit
    difference of Mt or K between the two evaluations shows as 1e-11, so they agree only because the emulation rounds every sum as the device does."""
    A, b = nc.instance(family, m, n)
    x = np.random.default_rng(m + n).standard_normal(n)
    for lam in LAMS:
        d = _handle(pkg, pkg.LeastSquares(A, b, lam, form="normal"), n)
        y = d.prox(1, x)
        ref = RefLeastSquares(A, b, lam).project(x)
        err, bar = np.abs(y - ref).max(), nc.bar(np.eye(n) + lam * (A.T @ A), x, ref)
        print("%s (%d, %d) lam %g: |y - ref| = %.2e (bar %.2e%s)" % (family, m, n, lam, err, bar, "" if family in nc.HELD else ", not held to it"))
        if family in nc.HELD:
            assert err <= bar
        assert d.prox(1, x).tobytes() == y.tobytes()
        _agree("%s lam %g" % (family, lam), y, nc.host_ls_normal(pkg, A, b, lam, x)[1])
        d.close()


def test_more_than_one_unit_per_strip(pkg):
    """n = 1100: 18 row blocks, so the first strips split into two units (RED_CHUNK = 16) and the fold adds two column slots"""
    n, m, lam = 1100, 1300, 0.5
    A, b = nc.instance("gauss", m, n)
    x = np.random.default_rng(n).standard_normal(n)
    d = _handle(pkg, pkg.LeastSquares(A, b, lam, form="normal"), n)
    _stats_ok(d.nspace_stats(1), n, m, "cholesky")
    y = d.prox(1, x)
    ref = RefLeastSquares(A, b, lam).project(x)
    assert np.abs(y - ref).max() <= nc.bar(np.eye(n) + lam * (A.T @ A), x, ref) and d.prox(1, x).tobytes() == y.tobytes()


@pytest.mark.parametrize("m,n,per_col", [(500, 40, 6), (1000, 300, 4), (131, 65, 3), (50, 1, 20)])
def test_sparse_normal_form(pkg, m, n, per_col):
    A, b = nc.tall_sparse(m, n, per_col)
    Ad = A.toarray()
    x = np.random.default_rng(m + n).standard_normal(n)
    for lam in LAMS:
        for factor in ("cholesky", "newton"):
            d = _handle(pkg, pkg.LeastSquares(A, b, lam, factor=factor, form="normal"), n)
            _stats_ok(d.nspace_stats(1), n, m, factor)
            y = d.prox(1, x)
            ref = RefLeastSquares(Ad, b, lam).project(x)
            assert np.abs(y - ref).max() <= nc.bar(np.eye(n) + lam * (Ad.T @ Ad), x, ref), (lam, factor)
            assert d.prox(1, x).tobytes() == y.tobytes()
            if factor == "cholesky":
                _agree("sparse normal (%d, %d) lam %g" % (m, n, lam), y, nc.host_ls_sparse(pkg, A, b, lam, "normal", x)[1])
            d.close()


@pytest.mark.parametrize("m,n,per_row,decades", [s for s in RAND_SHAPES if s[1] <= 1000])
def test_sparse_wide_form(pkg, m, n, per_row, decades):
    A, b = rand(m, n, per_row, decades)
    x = np.random.default_rng(m).standard_normal(n)
    for lam in (LAMS if m <= 300 else [1.0]):
        for factor in ("cholesky", "newton"):
            d = _handle(pkg, pkg.LeastSquares(A, b, lam, factor=factor, form="sparse_factored"), n)
            st = d.affine_sparse_factored_stats(1)
            assert (st["m"], st["n"], st["refine"], st["factor"]) == (m, n, 0, factor) and st["launches"] == 5 + (st["folded_rows"] > 0) + (st["folded_cols"] > 0), st
            y = d.prox(1, x)
            err = np.abs(y - RefLeastSquares(A.toarray(), b, lam).project(x)).max()
            print("sparse wide (%d, %d) lam %g %s: |y - dense solve| = %.2e" % (m, n, lam, factor, err))
            assert err <= TOL * max(1.0, np.abs(x).max()) and d.prox(1, x).tobytes() == y.tobytes()
            if factor == "cholesky":
                _agree("sparse wide (%d, %d) lam %g" % (m, n, lam), y, nc.host_ls_sparse(pkg, A, b, lam, "sparse_factored", x)[1])
            d.close()


def test_sparse_wide_form_cut_rows(pkg, monkeypatch):
    monkeypatch.setenv("FOS_SF_SEG", "64")
    for name, (A, b) in seg64_cases().items():
        x = np.random.default_rng(len(name)).standard_normal(A.shape[1])
        d = _handle(pkg, pkg.LeastSquares(A, b, 1.0, form="sparse_factored"), A.shape[1])
        st = d.affine_sparse_factored_stats(1)
        assert st["seg"] == 64 and (st["folded_rows"] + st["folded_cols"] > 0 or name == "band"), (name, st)      # (the band's rows and columns are short: nothing is cut)
        y = d.prox(1, x)
        assert np.abs(y - RefLeastSquares(A.toarray(), b, 1.0).project(x)).max() <= TOL * max(1.0, np.abs(x).max()), name
        _agree(name, y, nc.host_ls_sparse(pkg, A, b, 1.0, "sparse_factored", x)[1])
        d.close()


def test_set_sequences_and_refusals(pkg):
    n = 129
    A, b = nc.instance("gauss", 200, n)
    Q, q = nc.quadratic_of(A, b, 0.3)
    x = np.random.default_rng(9).standard_normal(n)
    box = pkg.IndBox(0.0, 1.0)
    d = pkg.HipFeasibility(pkg.Feasibility(pkg.Quadratic(Q, q), box, n))       # Quadratic as S1 ...
    before = d.prox(1, x)
    d2 = pkg.HipFeasibility(pkg.Feasibility(box, pkg.Quadratic(Q, q), n))       # ... and as S2
    assert d2.prox(2, x).tobytes() == before.tobytes() and d2.nspace_stats(2)["n"] == n
    lib = pkg.lib.load()
    bad = Q.copy(); bad[5, 5] = -2.0
    ind = np.zeros((n, n)); ind[70, 3] = 4.0                                   # indefinite with a zero diagonal: the device's Cholesky pivot fails
    nanq = Q.copy(); nanq[8, 2] = np.nan
    for M_, what in ((bad, "column 5"), (ind, "column"), (nanq, "non-finite")):
        assert lib.fos_feas_set_quadratic(d._h, 1, pkg.lib.dptr(np.ascontiguousarray(M_)), pkg.lib.dptr(q), 1) == FOS_EINVAL
        assert what in lib.fos_last_error().decode(), lib.fos_last_error()
    assert lib.fos_feas_set_quadratic(d._h, 1, pkg.lib.dptr(Q), pkg.lib.dptr(q), 7) == FOS_EINVAL                               # an unknown factor
    assert lib.fos_feas_set_least_squares_normal(d._h, 1, 200, pkg.lib.dptr(A), pkg.lib.dptr(b), 0.0, 1) == FOS_EINVAL        # lambda = 0
    assert lib.fos_feas_set_least_squares_normal(d._h, 1, 0, pkg.lib.dptr(A), pkg.lib.dptr(b), 1.0, 1) == FOS_EINVAL          # m = 0
    keep, ptrs = nc.csc_ptrs(pkg, sp.csc_matrix(A))
    assert lib.fos_feas_set_least_squares_sparse(d._h, 1, 200, ptrs[0], ptrs[1], ptrs[2], pkg.lib.dptr(b), 1.0, 5, 1) == FOS_EINVAL      # an unknown form
    assert lib.fos_feas_set_least_squares_sparse(d._h, 1, 200, ptrs[0], ptrs[1], ptrs[2], pkg.lib.dptr(b), 1.0, 0, 1) == FOS_EINVAL      # sparse wide: m > n
    assert d.prox(1, x).tobytes() == before.tobytes()                          # every refused call left the Quadratic working
    with pytest.raises(ValueError):
        d.set_set(1, pkg.Quadratic(Q[:50, :50], q[:50]))                       # the wrong order
    with pytest.raises(pkg.lib.FosError):
        d.nspace_stats(2)                                                      # a box has none
    d.set_set(1, box)                                                          # Quadratic -> box -> Quadratic
    assert np.array_equal(d.prox(1, x), np.clip(x, 0.0, 1.0))
    with pytest.raises(pkg.lib.FosError):
        d.nspace_stats(1)
    d.set_set(1, pkg.Quadratic(2.0 * Q, q))
    ref = nc.RefQuadratic(2.0 * Q, q).project(x)
    assert np.abs(d.prox(1, x) - ref).max() <= nc.bar(np.eye(n) + 2.0 * Q, x, ref)
    d.set_set(1, pkg.LeastSquares(sp.csc_matrix(A), b, 0.3, form="normal"))    # the same matrix as the first Quadratic
    ref = RefLeastSquares(A, b, 0.3).project(x)
    assert np.abs(d.prox(1, x) - ref).max() <= nc.bar(np.eye(n) + Q, x, ref) and np.abs(d.prox(1, x) - before).max() <= nc.bar(np.eye(n) + Q, x, ref)
    assert d._callbacks == []


LASSO_LAM, LASSO_MU = 0.7, 0.5


@pytest.mark.parametrize("algname", ["DR", "GAPA", "FISTA"])
def test_tall_lasso_iterates_match_oracle_and_callback_path(pkg, oracle, algname):
    """LeastSquares(A, b, 0.7, form="normal") over a tall A (300 x 40) and NormL1(0.5): the same iterates as the oracle running the reference objects
    (<= 1e-11 max(1, |x|_inf)) and as the device's own callback path running them -- the bar and the pattern of
    test_gpu_prox_fn.test_lasso_iterates_match_oracle_and_callback_path (two iterations for GAPA, 30 otherwise).  Then DR to eps = 1e-9: lasso_kkt is printed."""
    orc = oracle
    A, b = nc.instance("gauss", 300, 40)
    n = 40
    ref_o, ref_cb = [(RefLeastSquares(A, b, LASSO_LAM), RefNormL1(LASSO_MU)) for _ in range(2)]
    oalg = ALGS[algname](orc, verbose=0)
    ost = orc.FeasibilityStatus(orc.FeasibilityModel(orc.Feasibility(ref_o[0], ref_o[1], n), oalg), 4, 1e-30, 0, 1)
    d = pkg.HipFeasibility(pkg.Feasibility(pkg.LeastSquares(A, b, LASSO_LAM, form="normal"), pkg.NormL1(LASSO_MU), n))
    dc = pkg.HipFeasibility(pkg.Feasibility(ref_cb[0], ref_cb[1], n))
    for h in (d, dc):
        h.set_alg(ALGS[algname](pkg))
        h.set_iterate(None)
    xo = np.zeros(n)
    nsame = 2 if algname == "GAPA" else 30
    for i in range(1, nsame + 1):
        ost.i = i
        oalg.step(xo, i, ost)
        assert d.step(i, 1, 4, 1e-30)[0] == 1 and dc.step(i, 1, 4, 1e-30)[0] == 1
        z = d.get_iterate()
        assert np.abs(z - xo).max() <= 1e-11 * max(1.0, np.abs(xo).max()), (algname, i)
        assert np.abs(z - dc.get_iterate()).max() <= 1e-11 * max(1.0, np.abs(xo).max()), (algname, i)
    for k in (0, 1):
        assert ref_cb[k].calls == ref_o[k].calls > 0               # the callback path really ran the objects ...
    assert d._callbacks == [] and len(dc._callbacks) == 2          # ... and the device objects have no way to call back
    if algname == "DR":
        done, status, err, checked = d.step(nsame + 1, 3000, 10, 1e-9)
        xs = d.prox(1, d.get_iterate())
        print("DR tall lasso: %s after %d iterations, lasso_kkt %.2e, %d of %d entries on the support" %
              (status, nsame + done, lasso_kkt(A, b, LASSO_LAM, LASSO_MU, xs), (np.abs(xs) > 1e-6).sum(), n))


def test_box_qp_iterates_match_oracle_and_callback_path(pkg, oracle):
    """DR on Quadratic(Q, q) n IndBox(0, 1), n = 129: 30 iterations against the oracle and the callback path at 1e-11 max(1, |x|_inf); then to eps = 1e-9 and the
    projected-gradient residual of the QP at x = prox_S1(z), printed"""
    orc = oracle
    n = 129
    A, b = nc.instance("gauss", 200, n)
    Q, q = nc.quadratic_of(A, b, 0.05)
    ref_o, ref_cb = [(nc.RefQuadratic(Q, q), RefBox(0.0, 1.0)) for _ in range(2)]
    oalg = ALGS["DR"](orc, verbose=0)
    ost = orc.FeasibilityStatus(orc.FeasibilityModel(orc.Feasibility(ref_o[0], ref_o[1], n), oalg), 4, 1e-30, 0, 1)
    d = pkg.HipFeasibility(pkg.Feasibility(pkg.Quadratic(Q, q), pkg.IndBox(0.0, 1.0), n))
    dc = pkg.HipFeasibility(pkg.Feasibility(ref_cb[0], ref_cb[1], n))
    for h in (d, dc):
        h.set_alg(ALGS["DR"](pkg))
        h.set_iterate(None)
    xo = np.zeros(n)
    for i in range(1, 31):
        ost.i = i
        oalg.step(xo, i, ost)
        assert d.step(i, 1, 4, 1e-30)[0] == 1 and dc.step(i, 1, 4, 1e-30)[0] == 1
        z = d.get_iterate()
        assert np.abs(z - xo).max() <= 1e-11 * max(1.0, np.abs(xo).max()), i
        assert np.abs(z - dc.get_iterate()).max() <= 1e-11 * max(1.0, np.abs(xo).max()), i
    assert ref_cb[0].calls == ref_o[0].calls > 0 and d._callbacks == [] and len(dc._callbacks) == 2
    done, status, err, checked = d.step(31, 3000, 10, 1e-9)
    xs = np.clip(d.prox(1, d.get_iterate()), 0.0, 1.0)
    print("DR box QP: %s after %d iterations, projected-gradient residual %.2e, %d of %d entries strictly inside the box" %
          (status, 30 + done, nc.box_qp_residual(Q, q, 0.0, 1.0, xs), ((xs > 0.0) & (xs < 1.0)).sum(), n))
