"""GPU: IndAffine(A, b) with a sparse A in its FACTORED form (fos_feas_set_affine_sparse_factored, csrc/affine_sparse_factored.hip): A and A' kept as CSR, the dense
inverse of A A' of order m, a projection is two segmented sparse passes and three products of order m.  The projection is unique, so the checks are against the
oracle's IndAffine (dense Cholesky of A A') at the project's tolerance for an exact affine projection, 1e-12 max(1, |x|_inf), against the host emulation, against
the conjugate-gradient sparse form of the same A, and whole solves against that form's.

The Hann(4) band (cond(A A') = 3.3e6) is held against an 80-bit Cholesky solve with refine = 1: the oracle itself is 6.65e-12 from that solve there."""
import numpy as np
import pytest
import scipy.sparse as sp

from feasibility_cases import ALGS
from sparse_factored_cases import HANN4, RAND_SHAPES, TOL, band, csc_args, host_project, longdouble_projection, rand, seg64_cases, segments, skew

pytestmark = pytest.mark.gpu


def factored(pkg, A, b, **kw):
    n = A.shape[1]
    return pkg.HipFeasibility(pkg.Feasibility(pkg.IndAffine(A, b, form="sparse_factored", **kw), pkg.IndBox(0.0, np.inf), n))


def check_projection(pkg, oracle, name, A, b, refine, cg=False):
    """the device projection of a slowly moving x against the oracle, the host emulation and (cg) the conjugate-gradient form; the same bits twice"""
    n = A.shape[1]
    d = factored(pkg, A, b, refine=refine)
    st = d.affine_sparse_factored_stats(1)
    dc = pkg.HipFeasibility(pkg.Feasibility(pkg.IndAffine(A, b), pkg.IndBox(0.0, np.inf), n)) if cg else None
    ref = oracle.IndAffine(A.toarray(), b)
    rng = np.random.default_rng(1)
    x = rng.standard_normal(n)
    y = np.empty(n)
    empty = np.flatnonzero(np.diff(A.indptr) == 0)
    for rep in range(2):
        ref.prox(y, x)
        yd = d.prox(1, x)
        scale = max(1.0, np.abs(x).max())
        print("%s refine %d rep %d: |y - oracle| = %.2e (bar %.2e)" % (name, refine, rep, np.abs(yd - y).max(), TOL * scale), st)
        assert np.abs(yd - y).max() <= TOL * scale, (rep, st)
        if rep == 0:                                                              # (the host inverts A A' again at every call: once)
            rc, yh = host_project(pkg, A, b, refine, x)
            assert rc == 0
            print("    |y - host emulation| = %.2e" % np.abs(yd - yh).max())
            assert np.abs(yd - yh).max() <= TOL * scale, st                       # (two inverses: not bit for bit)
        assert np.array_equal(yd[empty], x[empty])                                # an empty column of A: y_i = x_i, exactly
        if dc is not None:
            assert np.abs(dc.prox(1, x) - yd).max() <= 1e-12 * scale
        assert d.affine_sparse_factored_stats(1) == st                            # the launch count: cold and warm
        x = x + 1e-3 * rng.standard_normal(n)
    assert np.array_equal(d.prox(1, x), d.prox(1, x))                             # every sum has a fixed order: the same bits
    return st


@pytest.mark.parametrize("refine", [0, 1])
@pytest.mark.parametrize("m,n,per_row,decades", RAND_SHAPES)
def test_projection_matches_the_oracle_the_host_emulation_and_the_cg_form(pkg, oracle, m, n, per_row, decades, refine):
    A, b = rand(m, n, per_row, decades)
    st = check_projection(pkg, oracle, "rand (%d, %d, %d)" % (m, n, per_row), A, b, refine, cg=True)
    assert (st["m"], st["n"], st["refine"], st["factor"], st["fell_back"], st["nnz"]) == (m, n, refine, "cholesky", 0, A.nnz)
    assert st["gram_order"] == (m + 63) // 64 * 64                                # orders 64 and 65: no padding / 63 rows of it


@pytest.mark.parametrize("refine", [0, 1])
@pytest.mark.parametrize("name", ["skew", "dense_column", "band"])
def test_projection_with_short_segments(pkg, oracle, monkeypatch, name, refine):
    monkeypatch.setenv("FOS_SF_SEG", "64")
    A, b = seg64_cases()[name]
    st = check_projection(pkg, oracle, name, A, b, refine)
    rows, cols = np.diff(sp.csr_matrix(A).indptr), np.diff(A.indptr)
    (f1, s1), (f2, s2) = segments(rows, 64), segments(cols, 64)
    assert (st["seg"], st["folded_rows"], st["folded_cols"], st["segments"]) == (64, f1, f2, s1 + s2)
    assert f1 > 0 if name == "skew" else f2 > 0 if name == "dense_column" else f1 + f2 == 0      # pass 1 folds / pass 2 folds / neither
    assert st["launches"] == (5 + (f1 > 0) + (f2 > 0)) + refine * (3 + (f1 > 0) + (f2 > 0))


@pytest.mark.parametrize("refine", [0, 1])
def test_rows_at_the_default_segment_length(pkg, oracle, refine):
    probe = factored(pkg, *rand(7, 9, 3))
    seg = probe.affine_sparse_factored_stats(1)["seg"]
    long_rows = [seg - 1, seg, seg + 1, 2 * seg + 1, 1]
    A, b = skew(70, 2 * seg + 2000, long_rows, 3)
    st = check_projection(pkg, oracle, "skew at SEG = %d" % seg, A, b, refine)
    assert (st["seg"], st["folded_rows"], st["folded_cols"], st["segments"]) == (seg, 2, 0, 2 + 3)
    assert st["items_rows"] >= 5 + 3 and st["items_cols"] >= 1 and st["launches"] == 6 + refine * 4


@pytest.mark.skipif(np.finfo(np.longdouble).eps > 1e-18, reason="needs an 80-bit long double for the reference")
@pytest.mark.parametrize("refine", [1, 2])
def test_hann_band_matches_an_extended_precision_solve(pkg, refine):
    A, b = band(300, HANN4)
    x = np.random.default_rng(1).standard_normal(A.shape[1])
    y = factored(pkg, A, b, refine=refine).prox(1, x)
    err = np.abs(y - longdouble_projection(A, b, x)).max()
    print("Hann(4) band, refine %d: |y - 80-bit solve| = %.2e (bar %.2e)" % (refine, err, TOL * max(1.0, np.abs(x).max())))
    assert err <= TOL * max(1.0, np.abs(x).max())


@pytest.mark.parametrize("factor", ["cholesky", "newton"])
def test_two_handles_give_the_same_bits(pkg, monkeypatch, factor):
    monkeypatch.setenv("FOS_SF_SEG", "64")
    for A, b in (seg64_cases()["skew"], seg64_cases()["dense_column"], rand(300, 1000, 6)):
        x = np.random.default_rng(4).standard_normal(A.shape[1])
        d1, d2 = factored(pkg, A, b, factor=factor), factored(pkg, A, b, factor=factor)
        assert d1.affine_sparse_factored_stats(1)["factor"] == factor
        assert np.array_equal(d1.prox(1, x), d2.prox(1, x))                       # the Gram kernel and the folds: a fixed order


@pytest.mark.parametrize("algname", sorted(ALGS) + ["LineSearch(GAPA)"])
def test_whole_solves_match_the_cg_form(pkg, algname):
    m, n = 120, 400
    A, b = rand(m, n, 8)
    kw = dict(eps=1e-9, max_iters=3000, verbose=0)
    alg = (lambda: pkg.LineSearchWrapper(ALGS["GAPA"](pkg, **kw), lsinterval=20)) if algname.startswith("LineSearch") else (lambda: ALGS[algname](pkg, **kw))
    sols = [pkg.solve_feasibility(pkg.Feasibility(S, pkg.IndBox(0.0, np.inf), n), alg(), checki=10)[0] for S in (pkg.IndAffine(A, b, form="sparse_factored"), pkg.IndAffine(A, b))]
    print(algname, [(s.status, s.iterations) for s in sols], np.abs(sols[0].x - sols[1].x).max())
    assert sols[0].status == sols[1].status
    assert abs(sols[0].iterations - sols[1].iterations) <= 10
    assert np.abs(sols[0].x - sols[1].x).max() <= 1e-7
    if sols[0].status == "Optimal":
        assert sols[0].x.min() > -1e-8 and np.abs(A @ sols[0].x - b).max() < 1e-7


def test_sets_replace_one_another(pkg, oracle):
    """kinds 5 (sparse, CG), 7 (dense, factored) and 8 (sparse, factored) over one another on one handle, both ways: the projection is onto the last one"""
    n = 1000
    insts = [rand(300, n, 6), rand(40, n, 30), rand(64, n, 5)]
    forms = {5: dict(), 7: dict(form="factored"), 8: dict(form="sparse_factored")}
    d = pkg.HipFeasibility(pkg.Feasibility(pkg.IndBox(-1.0, 1.0), pkg.IndBox(0.0, np.inf), n))
    x = np.random.default_rng(9).standard_normal(n)
    y = np.empty(n)
    for k, kind in enumerate([8, 5, 8, 7, 8, 8, 7, 5, 7]):
        A, b = insts[k % 3]
        d.set_set(1, pkg.IndAffine(A, b, **forms[kind]))
        oracle.IndAffine(A.toarray(), b).prox(y, x)
        assert np.abs(d.prox(1, x) - y).max() <= TOL * max(1.0, np.abs(x).max()), (k, kind)
        if kind == 8:
            assert d.affine_sparse_factored_stats(1)["m"] == A.shape[0]
        else:
            with pytest.raises(pkg.lib.FosError):
                d.affine_sparse_factored_stats(1)
    d.set_set(1, pkg.IndBox(-1.0, 1.0))
    assert np.array_equal(d.prox(1, x), np.clip(x, -1.0, 1.0))


def test_error_paths(pkg):
    n = 30
    A, b = rand(10, n, 4)
    box = pkg.IndBox(0.0, 1.0)
    make = lambda M, rhs, **kw: pkg.HipFeasibility(pkg.Feasibility(pkg.IndAffine(sp.csc_matrix(M), rhs, form="sparse_factored", **kw), box, M.shape[1]))
    D = sp.lil_matrix(A); D[7, :] = D[2, :]                         # a duplicated row with an inconsistent right-hand side: refused at set-up
    b2 = b.copy(); b2[7] = b[2] + 1.0
    for factor in ("cholesky", "newton"):
        with pytest.raises(pkg.lib.FosError, match="full row rank"):
            make(D, b2, factor=factor)
    C = sp.lil_matrix(A); C[5, :] = C[1, :] + C[3, :]               # a row in the span of two others
    with pytest.raises(pkg.lib.FosError, match="full row rank"):
        make(C, b)
    Z = sp.lil_matrix(A); Z[4, :] = 0.0
    with pytest.raises(pkg.lib.FosError, match="zero"):
        make(Z, b)
    with pytest.raises(pkg.lib.FosError, match="m <= n"):
        make(sp.csc_matrix(A.T), np.ones(n))
    d = pkg.HipFeasibility(pkg.Feasibility(box, box, n))
    lib = pkg.lib.load()
    keep, (cp, rv, nz) = csc_args(pkg, A)
    assert lib.fos_feas_set_affine_sparse_factored(d._h, 1, 10, cp, rv, nz, pkg.lib.dptr(b), 1, 3) == -1      # refine = 3 at the C entry
    assert "refine" in lib.fos_last_error().decode()
    assert lib.fos_feas_set_affine_sparse_factored(d._h, 1, 10, cp, rv, nz, pkg.lib.dptr(b), 7, 0) == -1      # an unknown factor
    nan = keep[2].copy(); nan[3] = np.nan
    assert lib.fos_feas_set_affine_sparse_factored(d._h, 1, 10, cp, rv, pkg.lib.dptr(nan), pkg.lib.dptr(b), 1, 0) == -1
    assert "non-finite" in lib.fos_last_error().decode()
    zero_based = keep[0] - 1
    assert lib.fos_feas_set_affine_sparse_factored(d._h, 1, 10, zero_based.ctypes.data_as(type(cp)), rv, nz, pkg.lib.dptr(b), 1, 0) == -1
    assert "1-based" in lib.fos_last_error().decode()
    assert np.array_equal(d.prox(1, np.full(n, 2.0)), np.ones(n))                                            # a refused call leaves the set as it was
    with pytest.raises(pkg.lib.FosError):
        d.affine_sparse_factored_stats(1)
    assert lib.fos_feas_set_affine_sparse_factored(d._h, 1, 10, cp, rv, nz, pkg.lib.dptr(b), 1, 0) == 0
    assert d.affine_sparse_factored_stats(1)["launches"] == 5
