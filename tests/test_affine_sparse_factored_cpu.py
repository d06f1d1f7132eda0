"""The sparse factored IndAffine (csrc/affine_sparse_factored.hip), the parts that need no GPU: fos_host_affine_sparse_factored -- the set-up's validation and row
scaling, A A' summed in the set-up kernel's order, the blocked Cholesky inverse accepted by the set-up's probe, the segment tables and both passes with the kernels'
summation order -- against the oracle's IndAffine (dense Cholesky of A A') at the project's tolerance for an exact affine projection, 1e-12 max(1, |x|_inf), and
against the same formula with scipy.sparse products in place of the passes; its refusals; the entries in every layer.

The Hann(4) band (cond(A A') = 3.3e6) is held against an 80-bit Cholesky solve with refine = 1: there the oracle itself is 6.65e-12 from that solve, and the
formula without a refinement step 1.46e-11 (1.8e-14 with one)."""
import re
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp

from affine_factored_cases import range_defect
from sparse_factored_cases import HANN4, RAND_SHAPES, TOL, band, host_project, longdouble_projection, rand, seg64_cases

ROOT = Path(__file__).resolve().parent.parent
FOS_EINVAL = -1                                     # include/foship.h


def check_against_oracle(pkg, oracle, name, A, b, refine):
    n = A.shape[1]
    x = np.random.default_rng(1).standard_normal(n)
    ref = np.empty(n)
    Ad = A.toarray()
    oracle.IndAffine(Ad, b).prox(ref, x)
    rc, y = host_project(pkg, A, b, refine, x)
    assert rc == 0, pkg.lib.load().fos_last_error().decode()
    scale = max(1.0, np.abs(x).max())
    rows = np.sqrt((Ad * Ad).sum(axis=1))
    err, resid, defect = np.abs(y - ref).max(), np.abs((Ad @ y - b) / rows).max(), range_defect(Ad, x, y)
    print("%s refine %d: |y - oracle| = %.2e, |A y - b| / rowscale = %.2e, range defect %.2e (bar %.2e)" % (name, refine, err, resid, defect, TOL * scale))
    assert err <= TOL * scale and resid <= TOL * scale and defect <= TOL * scale


@pytest.mark.parametrize("refine", [0, 1])
@pytest.mark.parametrize("m,n,per_row,decades", RAND_SHAPES)
def test_host_emulation_matches_the_oracle(pkg, oracle, m, n, per_row, decades, refine):
    A, b = rand(m, n, per_row, decades)
    check_against_oracle(pkg, oracle, "rand (%d, %d, %d)" % (m, n, per_row), A, b, refine)


@pytest.mark.parametrize("refine", [0, 1])
@pytest.mark.parametrize("name", ["skew", "dense_column", "band"])
def test_host_emulation_with_short_segments_matches_the_oracle(pkg, oracle, monkeypatch, name, refine):
    monkeypatch.setenv("FOS_SF_SEG", "64")            # rows of 65 and 129 entries (skew) and columns of 70 and 129 (the dense columns) are cut and folded
    A, b = seg64_cases()[name]
    check_against_oracle(pkg, oracle, name, A, b, refine)


@pytest.mark.skipif(np.finfo(np.longdouble).eps > 1e-18, reason="needs an 80-bit long double for the reference")
def test_host_emulation_on_the_hann_band_matches_an_extended_precision_solve(pkg, monkeypatch):
    monkeypatch.setenv("FOS_SF_SEG", "64")
    A, b = band(300, HANN4)
    x = np.random.default_rng(1).standard_normal(A.shape[1])
    rc, y = host_project(pkg, A, b, 1, x)
    assert rc == 0, pkg.lib.load().fos_last_error().decode()
    err = np.abs(y - longdouble_projection(A, b, x)).max()
    print("Hann(4) band, refine 1: |y - 80-bit solve| = %.2e (bar %.2e)" % (err, TOL * max(1.0, np.abs(x).max())))
    assert err <= TOL * max(1.0, np.abs(x).max())


@pytest.mark.parametrize("seg", ["64", None])
def test_host_emulation_matches_scipy_products(pkg, monkeypatch, seg):
    """the segment tables, the packets and the folds alone: the formula with scipy.sparse products for the passes and numpy's inverse"""
    if seg:
        monkeypatch.setenv("FOS_SF_SEG", seg)
    cases = dict(seg64_cases())
    cases["rand"] = rand(300, 1000, 6)
    cases["rand wide rows"] = rand(40, 5000, 300)
    for name, (A, b) in cases.items():
        x = np.random.default_rng(2).standard_normal(A.shape[1])
        rc, y = host_project(pkg, A, b, 0, x)
        assert rc == 0
        s = 1.0 / np.sqrt(np.asarray(A.multiply(A).sum(axis=1)).ravel())
        As = sp.csr_matrix(sp.diags(s) @ A)
        G = (As @ As.T).toarray()
        X = np.linalg.inv(G)
        r = As @ x - s * b
        d = X @ r
        d = d + X @ (r - G @ d)
        ref = x - As.T @ d
        err = np.abs(y - ref).max()
        print("%s (SEG %s): |host - scipy| = %.2e" % (name, seg or "default", err))
        assert err <= TOL * max(1.0, np.abs(x).max())
        empty = np.flatnonzero(np.diff(A.indptr) == 0)
        assert np.array_equal(y[empty], x[empty])                     # an empty column of A: y_i = x_i


def test_refusals(pkg, monkeypatch):
    lib = pkg.lib.load()
    msg = lambda: lib.fos_last_error().decode()
    A, b = rand(10, 30, 4)
    x = np.ones(30)
    D = sp.lil_matrix(A); D[7, :] = D[2, :]                         # a duplicated row
    assert host_project(pkg, sp.csc_matrix(D), b, 0, x)[0] == FOS_EINVAL and "full row rank" in msg()
    C = sp.lil_matrix(A); C[5, :] = C[1, :] + C[3, :]               # a row in the span of two others
    assert host_project(pkg, sp.csc_matrix(C), b, 0, x)[0] == FOS_EINVAL and "full row rank" in msg()
    Z = sp.lil_matrix(A); Z[4, :] = 0.0
    assert host_project(pkg, sp.csc_matrix(Z), b, 0, x)[0] == FOS_EINVAL and "zero" in msg()
    Ac = sp.csc_matrix(A); Ac.sort_indices()
    nz = Ac.data.copy(); nz[3] = np.nan
    assert host_project(pkg, A, b, 0, x, raw=(Ac.indptr.astype(np.int64) + 1, Ac.indices.astype(np.int64) + 1, nz))[0] == FOS_EINVAL and "non-finite" in msg()
    assert host_project(pkg, A, b, 3, x)[0] == FOS_EINVAL and "refine" in msg()
    assert host_project(pkg, sp.csc_matrix(A.T), np.ones(30), 0, np.ones(10))[0] == FOS_EINVAL and "m <= n" in msg()
    assert host_project(pkg, A, b, 0, x, raw=(Ac.indptr.astype(np.int64), Ac.indices.astype(np.int64) + 1, Ac.data))[0] == FOS_EINVAL and "1-based" in msg()
    rv = Ac.indices.astype(np.int64) + 1
    col = int(np.flatnonzero(np.diff(Ac.indptr) >= 2)[0])
    rv[Ac.indptr[col] + 1] = rv[Ac.indptr[col]]                     # the same row twice in one column: the set-up kernel would add them side by side
    assert host_project(pkg, A, b, 0, x, raw=(Ac.indptr.astype(np.int64) + 1, rv, Ac.data))[0] == FOS_EINVAL and "ascending" in msg()
    monkeypatch.setenv("FOS_SF_SEG", "100")                         # not a multiple of 64
    assert host_project(pkg, A, b, 0, x)[0] == FOS_EINVAL and "FOS_SF_SEG" in msg()
    monkeypatch.setenv("FOS_SF_SEG", "4096")                        # above the default
    assert host_project(pkg, A, b, 0, x)[0] == FOS_EINVAL
    monkeypatch.delenv("FOS_SF_SEG")
    assert host_project(pkg, A, b, 0, x)[0] == 0


def test_python_layer_validates_the_form(pkg):
    A, b = rand(7, 9, 3)
    S = pkg.IndAffine(A, b, form="sparse_factored")
    assert (S.form, S.factor, S.refine) == ("sparse_factored", "cholesky", 0) and S.sparse is True
    assert sp.isspmatrix_csc(S.A) and S.A.has_sorted_indices
    S = pkg.IndAffine(A.toarray(), b, form="sparse_factored", factor="newton", refine=2, sparse=True)      # a dense A is converted
    assert sp.isspmatrix_csc(S.A) and (S.factor, S.refine, S.sparse) == ("newton", 2, True)
    dup = sp.coo_matrix(([1.0, 2.0, 3.0], ([0, 0, 1], [1, 1, 0])), shape=(2, 3))
    S = pkg.IndAffine(dup, np.ones(2), form="sparse_factored")
    assert S.A.nnz == 2 and S.A[0, 1] == 3.0                        # duplicates summed
    for kw in (dict(sparse=False), dict(refine=3), dict(factor="ldl")):
        with pytest.raises(ValueError):
            pkg.IndAffine(A, b, form="sparse_factored", **kw)
    wide = sp.csc_matrix((pkg.IndAffine.FACTORED_MAX + 1, pkg.IndAffine.FACTORED_MAX + 2))
    with pytest.raises(ValueError):
        pkg.IndAffine(wide, np.zeros(wide.shape[0]), form="sparse_factored")
    D = pkg.IndAffine(A, b)                                         # form=None: today's selection, to the letter
    assert D.form is None and D.sparse is True and pkg.IndAffine(A.toarray(), b).sparse is False
    F = pkg.IndAffine(A, b, form="factored")                        # still densifies
    assert isinstance(F.A, np.ndarray) and F.sparse is False
    for kw in (dict(form="projector"), dict(form="factored", sparse=True)):
        with pytest.raises(ValueError):
            pkg.IndAffine(A, b, **kw)


def test_entries_exist_in_every_layer(pkg):
    lib = pkg.lib.load(check_symbols=True)
    hdr = (ROOT / "include" / "foship.h").read_text()
    jl = (ROOT / "firstordersolvers.jl_amd" / "julia" / "FOSHip.jl").read_text()
    for name in ("fos_feas_set_affine_sparse_factored", "fos_feas_affine_sparse_factored_stats", "fos_feas_affine_sparse_factored_plan",
                 "fos_host_affine_sparse_factored"):
        assert getattr(lib, name) is not None
        assert name in pkg.lib.PROTOTYPES and name in pkg.lib.header_symbols()
        assert "ccall((:%s, libfoship)" % name in jl
    assert re.search(r"#define\s+FOS_ABI_VERSION\s+1\b", hdr)
    assert ":sparse_factored" in jl and ":affine_factor" in jl and ":affine_refine" in jl
