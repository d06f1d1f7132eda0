"""
The n-space forms -- Quadratic(Q, q) and LeastSquares in the normal-equations form (csrc/nspace.hip) -- and the sparse wide LeastSquares
(csrc/affine_sparse_factored.hip with a shifted diagonal): the parts that need no GPU.  The one-right-hand-side tile product and its packing
(fos_host_symv_packed) against X @ v, the host emulations against the references at the bar of tests/nspace_cases.py, the refusals, and every new entry in
every layer.

fos_host_symv_packed: y = X v over k terms per entry, summed in a fixed tree; |error| <= (k + 2) eps |X|_row |v| entrywise (the standard bound for any summation
order with fused or unfused products) -- asserted in that form.
"""
import re
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp

import nspace_cases as nc
from nspace_cases import FOS_EINVAL, FOS_EUNSUPPORTED, LAMS, SHAPES, TOL
from prox_fn_cases import RefLeastSquares
from sparse_factored_cases import RAND_SHAPES, rand, seg64_cases

ROOT = Path(__file__).resolve().parent.parent
EPS = 2.0 ** -52


@pytest.mark.parametrize("k", [1, 7, 33, 64, 65, 129, 300, 1100])
def test_symv_packed_matches_the_dense_product_and_stores_every_entry_once(pkg, k):
    """the tile edge (64 / 65), the strip edge (33), and at k = 1100 18 row blocks: more than RED_CHUNK = 16, so that a strip splits into units"""
    rng = np.random.default_rng(k)
    X = rng.standard_normal((k, k))
    X = np.tril(X) + np.tril(X, -1).T
    v = rng.standard_normal(k)
    rc, y, cnt = nc.host_symv_packed(pkg, X, v, count=True)
    assert rc == 0, pkg.lib.load().fos_last_error()
    bound = (k + 2) * EPS * (np.abs(X) @ np.abs(v))
    err = np.abs(y - X @ v)
    print("k = %d: max |y - X v| = %.2e, max bound %.2e" % (k, err.max(), bound.max()))
    assert (err <= 2.0 * bound + 1e-300).all()                                 # (X @ v itself carries the same bound)
    low = np.tril(np.ones((k, k), dtype=bool))
    blk = np.arange(k) // 64
    diag_block = blk[:, None] == blk[None, :]
    assert (cnt[low] == 1).all()                                               # every entry of the lower triangle exactly once ...
    assert (cnt[~low & diag_block] == 1).all() and (cnt[~low & ~diag_block] == 0).all()      # ... the diagonal blocks whole, nothing else


def _check(tag, y, ref, M, x, held=True):
    err, b = float(np.abs(y - ref).max()), nc.bar(M, x, ref)
    print("%s: |y - ref| = %.2e, bar %.2e, cond(Mt) = %.3g" % (tag, err, b, nc.scaled_cond(M)))
    if held:
        assert err <= b, (tag, err, b)
    return err


@pytest.mark.parametrize("lam", LAMS)
@pytest.mark.parametrize("m,n", SHAPES)
def test_host_least_squares_normal_and_quadratic_match_the_references(pkg, m, n, lam):
    A, b = nc.instance("gauss", m, n)
    x = np.random.default_rng(m + n).standard_normal(n)
    M = np.eye(n) + lam * (A.T @ A)
    rc, y = nc.host_ls_normal(pkg, A, b, lam, x)
    assert rc == 0, pkg.lib.load().fos_last_error()
    _check("LeastSquares (%d, %d) lam %g" % (m, n, lam), y, RefLeastSquares(A, b, lam).project(x), M, x)
    Q, q = nc.quadratic_of(A, b, lam)
    rc, y = nc.host_quadratic(pkg, Q, q, x)
    assert rc == 0, pkg.lib.load().fos_last_error()
    _check("Quadratic n = %d lam %g" % (n, lam), y, nc.RefQuadratic(Q, q).project(x), np.eye(n) + Q, x)


@pytest.mark.parametrize("lam", LAMS)
@pytest.mark.parametrize("family,m,n", nc.EXTRA + [("cols", 1000, 200)])
def test_host_emulation_on_the_other_families(pkg, family, m, n, lam):
    """corr, row-scaled, wide, a zero column, rank-deficient: held to the bar.  Column-scaled: printed only (the Gram matrix in fp64 loses it: nspace_cases)."""
    A, b = nc.instance(family, m, n)
    x = np.random.default_rng(m + n).standard_normal(n)
    rc, y = nc.host_ls_normal(pkg, A, b, lam, x)
    assert rc == 0, pkg.lib.load().fos_last_error()
    _check("%s (%d, %d) lam %g" % (family, m, n, lam), y, RefLeastSquares(A, b, lam).project(x), np.eye(n) + lam * (A.T @ A), x, held=family in nc.HELD)
    assert np.all(np.isfinite(y))


def test_quadratic_zero_and_lower_triangle_only(pkg):
    n = 70
    rng = np.random.default_rng(5)
    x, q = rng.standard_normal(n), rng.standard_normal(n)
    rc, y = nc.host_quadratic(pkg, np.zeros((n, n)), q, x)
    assert rc == 0 and np.array_equal(y, x - q)                               # Q = 0: D = 1, K = I, the residual is exactly zero
    A, b = nc.instance("gauss", 90, n)
    Q, q = nc.quadratic_of(A, b, 0.5)
    rc, y = nc.host_quadratic(pkg, Q, q, x)
    junk = Q + np.triu(rng.standard_normal((n, n)), 1)                        # the upper triangle is never read
    rc2, y2 = nc.host_quadratic(pkg, junk, q, x)
    assert rc == 0 and rc2 == 0 and y.tobytes() == y2.tobytes()


SPARSE_WIDE = [s for s in RAND_SHAPES if s[1] <= 1000]


@pytest.mark.parametrize("m,n,per_row,decades", SPARSE_WIDE)
def test_host_sparse_factored_least_squares(pkg, m, n, per_row, decades):
    """the sparse wide form against the dense solve at the dense wide form's bar, TOL max(1, |x|_inf); every lambda on the shapes of order <= 300"""
    A, b = rand(m, n, per_row, decades)
    x = np.random.default_rng(m).standard_normal(n)
    for lam in (LAMS if m <= 300 else [1.0]):
        rc, y = nc.host_ls_sparse(pkg, A, b, lam, "sparse_factored", x)
        assert rc == 0, pkg.lib.load().fos_last_error()
        err = np.abs(y - RefLeastSquares(A.toarray(), b, lam).project(x)).max()
        print("(%d, %d) lam %g: |y - dense solve| = %.2e (bar %.2e)" % (m, n, lam, err, TOL * max(1.0, np.abs(x).max())))
        assert err <= TOL * max(1.0, np.abs(x).max()), lam


def test_host_sparse_factored_cut_rows_zero_and_dependent_rows(pkg, monkeypatch):
    monkeypatch.setenv("FOS_SF_SEG", "64")                                     # rows longer than 64 entries are cut into segments
    for name, (A, b) in seg64_cases().items():
        x = np.random.default_rng(len(name)).standard_normal(A.shape[1])
        for lam in LAMS:
            rc, y = nc.host_ls_sparse(pkg, A, b, lam, "sparse_factored", x)
            assert rc == 0, (name, pkg.lib.load().fos_last_error())
            err = np.abs(y - RefLeastSquares(A.toarray(), b, lam).project(x)).max()
            assert err <= TOL * max(1.0, np.abs(x).max()), (name, lam, err)
    monkeypatch.delenv("FOS_SF_SEG")
    A, b = rand(65, 131, 4)
    A = sp.lil_matrix(A)
    A[7, :] = 0.0                                                              # a zero row
    A[9, :] = A[3, :]                                                          # a dependent one, with an inconsistent right-hand side
    A = sp.csc_matrix(A)
    A.eliminate_zeros()
    b = b.copy(); b[9] = b[3] + 1.0
    x = np.random.default_rng(3).standard_normal(131)
    for lam in LAMS:
        rc, y = nc.host_ls_sparse(pkg, A, b, lam, "sparse_factored", x)
        assert rc == 0, pkg.lib.load().fos_last_error()
        assert np.abs(y - RefLeastSquares(A.toarray(), b, lam).project(x)).max() <= TOL * max(1.0, np.abs(x).max()), lam


@pytest.mark.parametrize("lam", LAMS)
@pytest.mark.parametrize("m,n,per_col", [(500, 40, 6), (1000, 300, 4), (131, 65, 3), (50, 1, 20)])
def test_host_sparse_normal_on_tall_instances(pkg, m, n, per_col, lam):
    A, b = nc.tall_sparse(m, n, per_col)
    Ad = A.toarray()
    x = np.random.default_rng(m + n).standard_normal(n)
    rc, y = nc.host_ls_sparse(pkg, A, b, lam, "normal", x)
    assert rc == 0, pkg.lib.load().fos_last_error()
    _check("sparse normal (%d, %d) lam %g" % (m, n, lam), y, RefLeastSquares(Ad, b, lam).project(x), np.eye(n) + lam * (Ad.T @ Ad), x)
    rc, yd = nc.host_ls_normal(pkg, Ad, b, lam, x)                             # the dense entry on the same matrix: the same M up to the Gram sums' order
    assert rc == 0 and np.abs(y - yd).max() <= nc.bar(np.eye(n) + lam * (Ad.T @ Ad), x, y)


def test_refusals(pkg):
    lib = pkg.lib.load()
    msg = lambda: lib.fos_last_error().decode()
    n = 40
    rng = np.random.default_rng(0)
    x = rng.standard_normal(n)
    A, b = nc.instance("gauss", 60, n)
    # Quadratic: Q not positive semidefinite -- the failed pivot's column is named
    Q, q = nc.quadratic_of(A, b, 1.0)
    bad = Q.copy(); bad[17, 17] = -3.0                                         # 1 + Q[17, 17] < 0: refused before the scaling
    rc, _ = nc.host_quadratic(pkg, bad, q, x)
    assert rc == FOS_EINVAL and "column 17" in msg() and "positive semidefinite" in msg(), msg()
    ind = np.zeros((n, n)); ind[5, 4] = ind[4, 5] = 4.0                        # an indefinite Q with a zero diagonal: the Cholesky pivot of column 5 fails
    rc, _ = nc.host_quadratic(pkg, ind, q, x)
    assert rc == FOS_EINVAL and "column 5" in msg(), msg()
    nanq = Q.copy(); nanq[3, 1] = np.nan
    assert nc.host_quadratic(pkg, nanq, q, x)[0] == FOS_EINVAL and "non-finite" in msg()
    # lambda
    for lam in (0.0, -1.0, np.inf, np.nan):
        assert nc.host_ls_normal(pkg, A, b, lam, x)[0] == FOS_EINVAL and "lambda" in msg(), lam
        assert nc.host_ls_sparse(pkg, sp.csc_matrix(A), b, lam, "normal", x)[0] == FOS_EINVAL and "lambda" in msg(), lam
        assert nc.host_ls_sparse(pkg, sp.csc_matrix(A[:30]), b[:30], lam, "sparse_factored", x)[0] == FOS_EINVAL and "lambda" in msg(), lam
    # n > 46 000 (refused before anything is read)
    one = np.ones(1)
    assert lib.fos_host_least_squares_normal(1, 46001, pkg.lib.dptr(one), pkg.lib.dptr(one), 1.0, pkg.lib.dptr(one), pkg.lib.dptr(one)) == FOS_EUNSUPPORTED
    assert "46000" in msg()
    assert lib.fos_host_quadratic(46001, pkg.lib.dptr(one), pkg.lib.dptr(one), pkg.lib.dptr(one), pkg.lib.dptr(one)) == FOS_EUNSUPPORTED
    # an unknown form; the sparse wide form with m > n; unsorted entries
    S = sp.csc_matrix(A)
    assert nc.host_ls_sparse(pkg, S, b, 1.0, 7, x)[0] == FOS_EINVAL and "form" in msg()
    assert nc.host_ls_sparse(pkg, S, b, 1.0, "sparse_factored", x)[0] == FOS_EINVAL                # 60 x 40
    keep, _ = nc.csc_ptrs(pkg, S)
    rowval = keep[1].copy(); rowval[[0, 1]] = rowval[[1, 0]]
    assert nc.host_ls_sparse(pkg, S, b, 1.0, "normal", x, raw=(keep[0], rowval, keep[2]))[0] == FOS_EINVAL and "ascending" in msg()
    nz = keep[2].copy(); nz[3] = np.inf
    assert nc.host_ls_sparse(pkg, S, b, 1.0, "normal", x, raw=(keep[0], keep[1], nz))[0] == FOS_EINVAL and "non-finite" in msg()
    assert nc.host_symv_packed(pkg, np.ones((1, 1)), np.ones(1))[0] == 0 and lib.fos_host_symv_packed(0, None, None, None, None) == FOS_EINVAL


def test_constructors_validate(pkg):
    A, b = nc.instance("gauss", 12, 5)
    Q, q = nc.quadratic_of(A, b, 1.0)
    S = pkg.Quadratic(Q, q)
    assert S.factor == "cholesky" and S.Q.flags.c_contiguous
    for args, kw in (((Q[:4], q), {}), ((Q, q[:3]), {}), ((Q, q), {"factor": "lu"}), ((sp.csc_matrix(Q), q), {}), ((np.full((5, 5), np.nan), q), {})):
        with pytest.raises(ValueError):
            pkg.Quadratic(*args, **kw)
    up = Q.copy(); up[0, 4] = np.nan                                           # the upper triangle is not read, so not validated either
    pkg.Quadratic(up, q)
    # LeastSquares: form=None behaves as before, refusals included
    with pytest.raises(ValueError, match="must be dense"):
        pkg.LeastSquares(sp.csc_matrix(A), b, 1.0)
    assert pkg.LeastSquares(A, b, 1.0).form is None
    L = pkg.LeastSquares(A, b, 2.0, form="normal")                             # tall and dense
    assert (L.form, L.sparse, L.lam) == ("normal", False, 2.0)
    L = pkg.LeastSquares(sp.csr_matrix(A), b, 2.0, form="normal")
    assert L.sparse and sp.isspmatrix_csc(L.A) and L.A.has_sorted_indices
    L = pkg.LeastSquares(sp.csr_matrix(A.T), np.ones(5), 2.0, form="sparse_factored")
    assert L.sparse and L.form == "sparse_factored"
    for args, kw in (((A, b, 1.0), {"form": "sparse_factored"}),               # a dense A
                     ((sp.csc_matrix(A), b, 1.0), {"form": "sparse_factored"}),      # m > n
                     ((A, b, 1.0), {"form": "tall"}), ((A, b, 0.0), {"form": "normal"}), ((A, b[:3], 1.0), {"form": "normal"}),
                     ((sp.csc_matrix(A), b[:3], 1.0), {"form": "normal"}), ((A, b, 1.0), {"form": "normal", "factor": "qr"})):
        with pytest.raises(ValueError):
            pkg.LeastSquares(*args, **kw)
    with pytest.raises(ValueError, match="46000"):
        pkg.LeastSquares(sp.csc_matrix((2, 46001)), np.ones(2), 1.0, form="normal")
    with pytest.raises(ValueError):                                            # neither is a block of a SeparableSum
        pkg.SeparableSum([(S, 5)])
    with pytest.raises(ValueError):
        pkg.SeparableSum([(pkg.LeastSquares(A, b, 1.0, form="normal"), 5)])


NEW_ENTRIES = ["fos_feas_set_quadratic", "fos_feas_set_least_squares_normal", "fos_feas_set_least_squares_sparse", "fos_feas_nspace_stats", "fos_host_quadratic",
               "fos_host_least_squares_normal", "fos_host_least_squares_sparse", "fos_host_symv_packed"]


def test_every_layer_has_the_new_entries(pkg):
    lib = pkg.lib.load(check_symbols=True)
    hdr = (ROOT / "include" / "foship.h").read_text()
    jl = (ROOT / "firstordersolvers.jl_amd" / "julia" / "FOSHip.jl").read_text()
    for name in NEW_ENTRIES:
        assert name in pkg.lib.PROTOTYPES and name in pkg.lib.header_symbols() and hasattr(lib, name), name
        assert re.search(r"ccall\(\(:%s, libfoship\)" % name, jl), name
    assert set(pkg.lib.header_symbols()) == set(pkg.lib.PROTOTYPES)                 # header and binding still list the same symbols
    for macro, key in (("FOS_LS_FORM_SPARSE_FACTORED", "sparse_factored"), ("FOS_LS_FORM_NORMAL", "normal")):
        v = int(re.search(r"#define\s+%s\s+(\d+)" % macro, hdr).group(1))
        assert pkg.lib.LS_FORM_CODES[key] == v and re.search(r"const %s = Int32\(%d\)" % (macro, v), jl)
    assert "nspace" in (ROOT / "firstordersolvers.jl_amd" / "csrc" / "Makefile").read_text()
    assert hasattr(pkg, "Quadratic") and hasattr(pkg.HipFeasibility, "nspace_stats")
    for routed in ("ProximalOperators.Quadratic", "feas_set_least_squares_normal!(d.handle", "feas_set_least_squares_sparse!(d.handle", "feas_set_quadratic!(d.handle"):
        assert routed in jl, routed
