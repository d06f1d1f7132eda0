"""
No GPU: the cg forms (csrc/nspace_cg.hip) through their host emulations, fos_host_quadratic_cg and fos_host_least_squares_cg, which run the kernels' work items,
recurrence, stop rule and summation order -- at the shapes where the indexing can go wrong (one entry, a wavefront's edge, a row that crosses a 2 048-entry
segment, empty rows and columns) and at the error bar derived in tests/nspace_cg_cases.py.  Plus the refusals, each followed by a valid call, and the interface.
"""
import re
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp

import nspace_cases as nc
import nspace_cg_cases as cg
from nspace_cases import LAMS
from nspace_cg_cases import FOS_EINVAL

ROOT = Path(__file__).resolve().parent.parent


def _held(tag, y, yref, bar, iters):
    err = float(np.linalg.norm(y - yref))
    print("%s: |y - ref|_2 = %.2e (bar %.2e), %d CG iterations" % (tag, err, bar, iters))
    assert err <= bar, (tag, err, bar)


@pytest.mark.parametrize("name", cg.QUAD_CASES)
def test_quadratic_host_emulation(pkg, name):
    Q, q, x = cg.quadratic_case(name)
    rc, y, iters = cg.host_quadratic_cg(pkg, Q, q, x)
    assert rc == 0, pkg.lib.load().fos_last_error().decode()
    _held("Quadratic " + name, y, cg.quadratic_ref(name), cg.quadratic_bar(Q, q, x, cg.quadratic_ref(name)), iters)
    if name in cg.TINY:
        assert iters <= cg.TINY[name] + cg.SMALL, (name, iters)
    if name in ("n1", "diag", "zero"):                                         # M is diagonal: the cold start D^-1 (x + c) is the answer
        assert iters == 0, (name, iters)
    assert cg.host_quadratic_cg(pkg, Q, q, x)[1].tobytes() == y.tobytes()


def test_quadratic_reads_the_entries_on_and_below_the_diagonal(pkg):
    Q, q, x = cg.quadratic_case("n65")
    y = cg.host_quadratic_cg(pkg, Q, q, x)[1]
    junk = sp.csc_matrix(sp.tril(Q, 0) + 7.0 * sp.triu(Q, 1))                  # another upper triangle: not read
    assert cg.host_quadratic_cg(pkg, junk, q, x)[1].tobytes() == y.tobytes()
    assert cg.host_quadratic_cg(pkg, sp.csc_matrix(sp.tril(Q, 0)), q, x)[1].tobytes() == y.tobytes()


@pytest.mark.parametrize("lam", LAMS)
@pytest.mark.parametrize("name", cg.LS_CASES)
def test_least_squares_host_emulation(pkg, name, lam):
    A, b, x = cg.ls_case(name)
    rc, y, iters = cg.host_ls_cg(pkg, A, b, lam, x)
    assert rc == 0, pkg.lib.load().fos_last_error().decode()
    ref = cg.ls_ref(name, lam)
    _held("LeastSquares %s lam %g" % (name, lam), y, ref, cg.ls_bar(A, b, lam, x, ref), iters)
    if name in cg.TINY:
        assert iters <= cg.TINY[name] + cg.SMALL, (name, iters)
    if A.shape[1] == 1:
        assert iters == 0, (name, iters)


def test_tol_ends_earlier_at_its_looser_bar(pkg):
    Q, q, x = cg.quadratic_case("tridiag300")
    ref = cg.quadratic_ref("tridiag300")
    _, y0, it0 = cg.host_quadratic_cg(pkg, Q, q, x)
    rc, y8, it8 = cg.host_quadratic_cg(pkg, Q, q, x, tol=1e-8)
    assert rc == 0 and it8 < it0, (it8, it0)
    _held("Quadratic tridiag300 tol 1e-8", y8, ref, cg.quadratic_bar(Q, q, x, ref, tol=1e-8), it8)
    A, b, x = cg.ls_case("dup_rows")
    ref = cg.ls_ref("dup_rows", 1.0)
    _, _, it0 = cg.host_ls_cg(pkg, A, b, 1.0, x)
    rc, y8, it8 = cg.host_ls_cg(pkg, A, b, 1.0, x, tol=1e-8)
    assert rc == 0 and it8 < it0, (it8, it0)
    _held("LeastSquares dup_rows tol 1e-8", y8, ref, cg.ls_bar(A, b, 1.0, x, ref, tol=1e-8), it8)


def test_refusals_leave_the_next_call_working(pkg):
    lib = pkg.lib.load()
    msg = lambda: lib.fos_last_error().decode()
    Q, q, x = cg.quadratic_case("n63")
    A, b, xa = cg.ls_case("9x7")
    good_q = cg.host_quadratic_cg(pkg, Q, q, x)[1]
    good_a = cg.host_ls_cg(pkg, A, b, 1.0, xa)[1]

    def still_works():
        rc, y, _ = cg.host_quadratic_cg(pkg, Q, q, x)
        assert rc == 0 and y.tobytes() == good_q.tobytes()
        rc, y, _ = cg.host_ls_cg(pkg, A, b, 1.0, xa)
        assert rc == 0 and y.tobytes() == good_a.tobytes()

    for M, call in ((Q, lambda raw: cg.host_quadratic_cg(pkg, Q, q, x, raw=raw)), (A, lambda raw: cg.host_ls_cg(pkg, A, b, 1.0, xa, raw=raw))):
        (colptr, rowval, nzval), _ = nc.csc_ptrs(pkg, M)
        assert call((colptr - 1, rowval, nzval))[0] == FOS_EINVAL and "1-based" in msg(), msg()              # 0-based colptr
        still_works()
        dec = colptr.copy(); dec[2] = dec[1] - 1
        assert call((dec, rowval, nzval))[0] == FOS_EINVAL and "decreases" in msg(), msg()                   # decreasing colptr
        still_works()
        out = rowval.copy(); out[1] = M.shape[0] + 1
        assert call((colptr, out, nzval))[0] == FOS_EINVAL and "outside" in msg(), msg()                     # a row index out of range
        still_works()
        nan = nzval.copy(); nan[2] = np.nan
        assert call((colptr, rowval, nan))[0] == FOS_EINVAL and "non-finite" in msg(), msg()                 # a NaN entry
        still_works()
        swap = rowval.copy(); swap[[0, 1]] = swap[[1, 0]]
        assert call((colptr, swap, nzval))[0] == FOS_EINVAL and "ascending" in msg(), msg()                  # unsorted entries
        still_works()
    for lam in (0.0, -1.0, np.inf, np.nan):
        assert cg.host_ls_cg(pkg, A, b, lam, xa)[0] == FOS_EINVAL and "lambda" in msg(), lam
        still_works()
    for tol in (-1e-3, 1.0, np.nan):
        assert cg.host_quadratic_cg(pkg, Q, q, x, tol=tol)[0] == FOS_EINVAL and "tol" in msg(), tol
        assert cg.host_ls_cg(pkg, A, b, 1.0, xa, tol=tol)[0] == FOS_EINVAL and "tol" in msg(), tol
    bad = sp.lil_matrix(Q); bad[17, 17] = -1.0                                  # 1 + Q[18, 18] = 0 (1-based in the message)
    assert cg.host_quadratic_cg(pkg, sp.csc_matrix(bad), q, x)[0] == FOS_EINVAL and "Q[18, 18]" in msg() and "positive semidefinite" in msg(), msg()
    still_works()
    ind = sp.csc_matrix(np.array([[1.0, 0.5], [0.5, -3.0]]))                    # diag(1, -3) plus coupling: indefinite, 1 + Q[2, 2] < 0
    assert cg.host_quadratic_cg(pkg, ind, np.zeros(2), np.array([1.0, -1.0]))[0] == FOS_EINVAL and "positive semidefinite" in msg(), msg()
    still_works()
    ind = sp.csc_matrix(np.array([[0.0, 3.0], [3.0, 0.0]]))                     # indefinite with a zero diagonal: set-up cannot see it, CG meets p'(I + Q)p <= 0
    assert cg.host_quadratic_cg(pkg, ind, np.zeros(2), np.array([1.0, -1.0]))[0] == FOS_EINVAL and "positive semidefinite" in msg() and "CG" in msg(), msg()
    still_works()


def test_interface(pkg):
    Q, q, _ = cg.quadratic_case("n63")
    with pytest.raises(ValueError, match="Quadratic: Q must be dense"):          # form=None: to the letter
        pkg.Quadratic(Q, q)
    S = pkg.Quadratic(Q.toarray(), q)
    assert S.form is None and S.tol == 0.0 and isinstance(S.Q, np.ndarray)
    S = pkg.Quadratic(sp.csr_matrix(Q), q, form="cg", tol=1e-8)
    assert S.form == "cg" and S.tol == 1e-8 and sp.isspmatrix_csc(S.Q) and S.Q.has_sorted_indices
    assert sp.isspmatrix_csc(pkg.Quadratic(Q.toarray(), q, form="cg").Q)         # a dense Q is converted
    big = sp.identity(50001, format="csc")
    assert pkg.Quadratic(big, np.zeros(50001), form="cg").Q.shape == (50001, 50001)      # no bound on n
    with pytest.raises(ValueError, match="46000"):                               # the kept-inverse forms keep their limit
        pkg.LeastSquares(sp.csc_matrix((2, 46001)), np.ones(2), 1.0, form="normal")
    for args, kw in (((Q, q), {"form": "normal"}), ((Q, q), {"form": "cg", "tol": 1.0}), ((Q, q), {"form": "cg", "tol": -1.0}), ((Q.toarray(), q), {"tol": 1e-8}),
                     ((Q, q[:3]), {"form": "cg"}), ((Q[:5], q), {"form": "cg"}), ((Q, q), {"form": "cg", "factor": "lu"})):
        with pytest.raises(ValueError):
            pkg.Quadratic(*args, **kw)
    A, b, _ = cg.ls_case("9x7")
    with pytest.raises(ValueError, match="must be dense"):
        pkg.LeastSquares(A, b, 1.0)
    L = pkg.LeastSquares(A, b, 2.0, form="cg", tol=1e-9)
    assert (L.form, L.sparse, L.lam, L.tol) == ("cg", True, 2.0, 1e-9) and sp.isspmatrix_csc(L.A)
    L = pkg.LeastSquares(A.toarray(), b, 2.0, form="cg")                         # a dense A is converted
    assert L.sparse and sp.isspmatrix_csc(L.A) and L.tol == 0.0
    assert pkg.LeastSquares(sp.csc_matrix((60000, 50001)), np.ones(60000), 1.0, form="cg").A.shape == (60000, 50001)      # no bound on m, n
    for args, kw in (((A, b, 1.0), {"form": "iterative"}), ((A, b, 0.0), {"form": "cg"}), ((A, b[:3], 1.0), {"form": "cg"}), ((A, b, 1.0), {"form": "cg", "tol": 2.0}),
                     ((A, b, 1.0), {"form": "normal", "tol": 1e-8})):
        with pytest.raises(ValueError):
            pkg.LeastSquares(*args, **kw)


NEW_ENTRIES = ["fos_feas_set_quadratic_sparse", "fos_feas_set_least_squares_cg", "fos_feas_nspace_cg_stats", "fos_host_quadratic_cg", "fos_host_least_squares_cg"]


def test_every_layer_has_the_new_entries(pkg):
    lib = pkg.lib.load(check_symbols=True)
    hdr = (ROOT / "include" / "foship.h").read_text()
    jl = (ROOT / "firstordersolvers.jl_amd" / "julia" / "FOSHip.jl").read_text()
    for name in NEW_ENTRIES:
        assert name in pkg.lib.PROTOTYPES and name in pkg.lib.header_symbols() and hasattr(lib, name), name
        assert re.search(r"ccall\(\(:%s, libfoship\)" % name, jl), name
    assert set(pkg.lib.header_symbols()) == set(pkg.lib.PROTOTYPES)
    assert "Feasibility.jl:2-6" in hdr[hdr.index("csrc/nspace_cg.hip"):hdr.index("fos_feas_set_quadratic_sparse(")]
    assert re.search(r"\bnspace_cg\b", (ROOT / "firstordersolvers.jl_amd" / "csrc" / "Makefile").read_text())
    assert "FEAS_NSPACE_CG = 10" in (ROOT / "firstordersolvers.jl_amd" / "csrc" / "fos_internal.hpp").read_text()
    assert hasattr(pkg.HipFeasibility, "nspace_cg_stats")
