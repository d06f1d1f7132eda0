"""GPU: IndAffine(A, b) with a dense A in its FACTORED form (fos_feas_set_affine_factored, csrc/affine_dense.hip): A kept once, the inverse of A A' of order m,
a projection is two passes over A.  The projection is unique, so the checks are against the oracle's IndAffine (dense Cholesky of A A') at the project's
tolerance for an exact affine projection, 1e-12 max(1, |x|_inf), against the projector form of the same handle type where that exists (n <= 46 000), the true
residual after a refinement step against the rounding level of its own evaluation, and whole solves against the oracle's solve of the same problem."""
import numpy as np
import pytest

from affine_factored_cases import SHAPES, TOL, instance
from feasibility_cases import ALGS, GAPP

pytestmark = pytest.mark.gpu

# beyond the projector's width, odd n, more than one column span, m not a multiple of the row group of pass 1
WIDE = [("gauss", 3, 120001), ("gauss", 300, 50001)]


def factored(pkg, A, b, n, **kw):
    return pkg.HipFeasibility(pkg.Feasibility(pkg.IndAffine(A, b, form="factored", **kw), pkg.IndBox(0.0, np.inf), n))


@pytest.mark.parametrize("factor", ["cholesky", "newton"])
@pytest.mark.parametrize("family,m,n", SHAPES + WIDE)
def test_projection_matches_the_oracle_and_the_projector_form(pkg, oracle, family, m, n, factor):
    A, b = instance(family, m, n)
    d = factored(pkg, A, b, n, factor=factor)
    st = d.affine_factored_stats(1)
    dd = pkg.HipFeasibility(pkg.Feasibility(pkg.IndAffine(A, b), pkg.IndBox(0.0, np.inf), n)) if n <= pkg.IndAffine.DENSE_MAX else None
    ref = oracle.IndAffine(A, b)
    rng = np.random.default_rng(1)
    x = rng.standard_normal(n)
    y = np.empty(n)
    for rep in range(4):                                          # a slowly moving input, as the iterates of a solve
        ref.prox(y, x)
        yd = d.prox(1, x)
        scale = max(1.0, np.abs(x).max())
        print("%s (%d, %d) %s rep %d: |y - oracle| = %.2e (bar %.2e)%s" % (family, m, n, factor, rep, np.abs(yd - y).max(), TOL * scale,
              "" if dd is None else ", |y - projector| = %.2e (bar %.2e)" % (np.abs(dd.prox(1, x) - yd).max(), 1e-10 * scale)), st)
        assert np.abs(yd - y).max() <= TOL * scale, (rep, st)
        if dd is not None:
            assert np.abs(dd.prox(1, x) - yd).max() <= 1e-10 * scale      # (the dense projector is the less accurate of the two)
        x = x + 1e-3 * rng.standard_normal(n)
    assert np.array_equal(d.prox(1, x), d.prox(1, x))             # every sum has a fixed order: the same bits
    xl = 1e6 * x
    ref.prox(y, xl)
    assert np.abs(d.prox(1, xl) - y).max() <= TOL * np.abs(xl).max()


@pytest.mark.parametrize("m,n", [(64, 64), (500, 500)])
def test_true_residual_after_a_refinement_step(pkg, oracle, m, n):
    """refine = 1: |A y - b| (rows scaled to unit norm) at the rounding level of its own evaluation, 16 eps max(|A||y| + |b|) -- the criterion affine_sparse.hip
    ends on; an emulation of the steps in numpy gives 1.3e-15 against a bound of about 6e-14.  The error against the oracle is not larger than without the step
    (plus 1e-13 scale, the oracle's own error)."""
    A, b = instance("gauss", m, n)
    x = np.random.default_rng(1).standard_normal(n)
    ref = np.empty(n)
    oracle.IndAffine(A, b).prox(ref, x)
    scale = max(1.0, np.abs(x).max())
    y0 = factored(pkg, A, b, n, refine=0).prox(1, x)
    y1 = factored(pkg, A, b, n, refine=1).prox(1, x)
    L = np.longdouble
    rowscale = np.sqrt((A.astype(L) ** 2).sum(axis=1))
    resid = float((np.abs(A.astype(L) @ y1.astype(L) - b.astype(L)) / rowscale).max())
    level = float(((np.abs(A).astype(L) @ np.abs(y1).astype(L) + np.abs(b).astype(L)) / rowscale).max())
    e0, e1 = np.abs(y0 - ref).max(), np.abs(y1 - ref).max()
    print("(%d, %d): |A y - b| / rowscale = %.2e (bar %.2e), |y - oracle| = %.2e with refine = 0, %.2e with refine = 1" % (m, n, resid, 16 * 2.3e-16 * level, e0, e1))
    assert resid <= 16 * 2.3e-16 * level
    assert e1 <= e0 + 1e-13 * scale
    assert e1 <= TOL * scale


@pytest.mark.parametrize("algname", ["DR", "GAPA", "FISTA"])
def test_whole_solves_match_the_oracle(pkg, oracle, algname):
    orc = oracle
    m, n = 120, 400
    A, b = instance("gauss", m, n)
    hp = pkg.Feasibility(pkg.IndAffine(A, b, form="factored"), pkg.IndBox(0.0, np.inf), n)
    op = orc.Feasibility(orc.IndAffine(A, b), orc.IndBox(0.0, np.inf), n)
    kw = dict(eps=1e-9, max_iters=3000, verbose=0)
    sol, model = pkg.solve_feasibility(hp, ALGS[algname](pkg, **kw), checki=10)
    osol, _ = orc.feasibility_solve(op, ALGS[algname](orc, **kw), checki=10)
    assert sol.status == osol.status
    assert abs(sol.iterations - osol.iterations) <= 10
    assert np.abs(sol.x - osol.x).max() <= 1e-7
    if sol.status == "Optimal":
        assert sol.x.min() > -1e-8 and np.abs(A @ sol.x - b).max() < 1e-7


@pytest.mark.parametrize("wrapped", ["linesearch", "gapp"])
def test_search_wrappers_reach_the_projector_forms_status(pkg, wrapped):
    m, n = 120, 400
    A, b = instance("gauss", m, n)
    alg = (lambda: pkg.LineSearchWrapper(ALGS["GAP"](pkg, eps=1e-8, verbose=0), lsinterval=20)) if wrapped == "linesearch" else (lambda: GAPP(pkg, eps=1e-8, verbose=0))
    sols = [pkg.solve_feasibility(pkg.Feasibility(S, pkg.IndBox(0.0, np.inf), n), alg(), checki=10)[0] for S in (pkg.IndAffine(A, b, form="factored"), pkg.IndAffine(A, b))]
    assert sols[0].status == sols[1].status
    if sols[0].status == "Optimal":
        assert sols[0].x.min() > -1e-8 and np.abs(A @ sols[0].x - b).max() < 1e-6


def test_stats_and_replacement(pkg, oracle):
    m, n = 40, 5000
    A, b = instance("gauss", m, n)
    d = factored(pkg, A, b, n, factor="newton", refine=2)
    st = d.affine_factored_stats(1)
    assert (st["m"], st["n"], st["refine"], st["factor"], st["fell_back"]) == (m, n, 2, "newton", 0)
    assert st["ld"] == 5056 and st["gram_order"] == 64 and st["spans"] * st["span_cols"] >= st["ld"] and st["row_blocks"] * st["rows_per_block"] >= m
    assert st["bytes"] >= 8 * (m * st["ld"] + 2 * 64 * 64)
    assert st["launches"] == (6 + (st["row_blocks"] > 1)) + 2 * (3 + (st["row_blocks"] > 1) + 1)
    rng = np.random.default_rng(5)
    for _ in range(10):
        d.prox(1, rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 3))
    assert d.affine_factored_stats(1) == st                       # the launch count does not depend on the data
    assert factored(pkg, A, b, n).affine_factored_stats(1)["factor"] == "cholesky"
    with pytest.raises(pkg.lib.FosError):
        d.affine_stats(1)                                         # (the sparse form's counters)
    # factored, then a box, then factored with another A: the projection is onto the last one
    x = rng.standard_normal(n)
    d.set_set(1, pkg.IndBox(-1.0, 1.0))
    assert np.array_equal(d.prox(1, x), np.clip(x, -1.0, 1.0))
    with pytest.raises(pkg.lib.FosError):
        d.affine_factored_stats(1)
    A2, b2 = instance("corr", 33, n)
    d.set_set(1, pkg.IndAffine(A2, b2, form="factored", refine=1))
    st2 = d.affine_factored_stats(1)
    assert (st2["m"], st2["refine"], st2["factor"]) == (33, 1, "cholesky")
    y = np.empty(n)
    oracle.IndAffine(A2, b2).prox(y, x)
    assert np.abs(d.prox(1, x) - y).max() <= TOL * max(1.0, np.abs(x).max())
    d.set_set(1, pkg.IndAffine(A, b, form="factored"))            # factored over factored: the old one is freed, the new one projects
    oracle.IndAffine(A, b).prox(y, x)
    assert np.abs(d.prox(1, x) - y).max() <= TOL * max(1.0, np.abs(x).max())


def test_error_paths(pkg):
    A, b = instance("gauss", 10, 30)
    box = pkg.IndBox(0.0, 1.0)
    with pytest.raises(pkg.lib.FosError):                          # m > n
        pkg.HipFeasibility(pkg.Feasibility(pkg.IndAffine(A.T.copy(), np.ones(30), form="factored"), box, 10))
    D = A.copy(); D[7] = D[2]                                      # a duplicated row with an inconsistent right-hand side: refused at set-up
    b2 = b.copy(); b2[7] = b[2] + 1.0
    for factor in ("cholesky", "newton"):
        with pytest.raises(pkg.lib.FosError, match="full row rank"):
            pkg.HipFeasibility(pkg.Feasibility(pkg.IndAffine(D, b2, form="factored", factor=factor), box, 30))
    Z = A.copy(); Z[4] = 0.0
    with pytest.raises(pkg.lib.FosError, match="zero"):
        pkg.HipFeasibility(pkg.Feasibility(pkg.IndAffine(Z, b, form="factored"), box, 30))
    with pytest.raises((ValueError, pkg.lib.FosError)):
        pkg.HipFeasibility(pkg.Feasibility(pkg.IndAffine(A, b, form="factored", refine=3), box, 30))
    d = pkg.HipFeasibility(pkg.Feasibility(box, box, 30))
    lib = pkg.lib.load()
    assert lib.fos_feas_set_affine_factored(d._h, 1, 10, pkg.lib.dptr(A), pkg.lib.dptr(b), 1, 3) == -1      # refine = 3 at the C entry
    assert lib.fos_feas_set_affine_factored(d._h, 1, 10, pkg.lib.dptr(A), pkg.lib.dptr(b), 7, 0) == -1      # an unknown factor
    assert np.array_equal(d.prox(1, np.full(30, 2.0)), np.ones(30))                                          # a refused call leaves the set as it was
    n = 120000                                                     # without `form` a dense A of that width still has no device form
    with pytest.raises(pkg.lib.FosError):
        pkg.HipFeasibility(pkg.Feasibility(pkg.IndAffine(np.ones((3, n)), np.ones(3), sparse=False), box, n))
