"""No GPU: the sparse intake of the Feasibility sets (csrc/sparse_rows.cpp: csc_check, csc_to_csr_pair) through every host entry that takes CSC arrays --
fos_host_affine_sparse_factored (lambda = 0), fos_host_least_squares_sparse in both forms (sparse factored, lambda > 0; normal), fos_host_quadratic_cg and
fos_host_least_squares_cg.

FAULTS: one row per single fault of the caller's arrays, with the return code and the message each entry gives written out (the message always starts with the
entry's own name).  The file uses nothing but the C ABI, so it runs unchanged against an older library through FOSHIP_LIB: the table is what pins the messages.

PAIR: the CSR pair is not visible through the ABI, its effect is: a misplaced entry of A or A' moves the prox by O(1).  The emulations' answers are held to the bars
of the case files (sparse_factored_cases.TOL, nspace_cases.bar, nspace_cg_cases.ls_bar / quadratic_bar) against the same formula evaluated with scipy.sparse
products, at the shapes where a counting pass goes wrong.
"""
import numpy as np
import pytest
import scipy.sparse as sp

import nspace_cases as nc
import nspace_cg_cases as cg
import sparse_factored_cases as sf
from sparse_intake_cases import MUTATIONS, base

OK, EINVAL = 0, -1
LAM = 0.7
ENTRIES = ["affine_factored", "ls_factored", "ls_normal", "quadratic_cg", "ls_cg"]
WHAT = {"affine_factored": "IndAffine (sparse, factored)", "ls_factored": "LeastSquares (sparse, factored)", "ls_normal": "LeastSquares (sparse, normal)",
        "quadratic_cg": "Quadratic (cg)", "ls_cg": "LeastSquares (cg)"}


def call(pkg, entry, rows, cols, colptr, rowval, nzval, vec, x=None):
    """-> (code, message, y)"""
    colptr, rowval = np.ascontiguousarray(colptr, dtype=np.int64), np.ascontiguousarray(rowval, dtype=np.int64)
    nzval, vec = np.ascontiguousarray(nzval, dtype=np.float64), np.ascontiguousarray(vec, dtype=np.float64)
    if rowval.size == 0:                                                          # (nnz = 0: the arrays still exist)
        rowval, nzval = np.ones(1, dtype=np.int64), np.zeros(1)
    x = np.linspace(-1.0, 1.0, cols) if x is None else np.ascontiguousarray(x, dtype=np.float64)
    A = sp.csc_matrix((rows, cols))
    raw = (colptr, rowval, nzval)
    if entry == "affine_factored":
        rc, y = sf.host_project(pkg, A, vec, 1, x, raw=raw)
    elif entry == "ls_factored":
        rc, y = nc.host_ls_sparse(pkg, A, vec, LAM, "sparse_factored", x, raw=raw)
    elif entry == "ls_normal":
        rc, y = nc.host_ls_sparse(pkg, A, vec, LAM, "normal", x, raw=raw)
    elif entry == "quadratic_cg":
        rc, y, _ = cg.host_quadratic_cg(pkg, A, vec, x, raw=raw)
    else:
        rc, y, _ = cg.host_ls_cg(pkg, A, vec, LAM, x, raw=raw)
    msg = pkg.lib.load().fos_last_error()
    return rc, (msg.decode() if msg else ""), y


ASC = "the row indices of column 1 are not strictly ascending (duplicated or unsorted entries)"
A_NONFINITE, M_NONFINITE = "A has non-finite entries", "the matrix has non-finite entries"
EMPTY = "0 stored entries (1 .. 2e9 supported)"


def same(code, text):
    return {e: (code, text) for e in ENTRIES}


def nonfinite():
    return {e: (EINVAL, M_NONFINITE if e in ("quadratic_cg", "ls_cg") else A_NONFINITE) for e in ENTRIES}


# fault -> entry -> (return code, the message behind "<name of the entry>: "); (OK, None): the input is accepted and the answer is finite
FAULTS = {
    "colptr0_is_0": same(EINVAL, "colptr must be 1-based (colptr[0] = 0)"),
    "colptr_decreases": same(EINVAL, "colptr decreases at column 2"),
    "row_index_0": {**same(EINVAL, "row index 0 outside 1..3"), "quadratic_cg": (EINVAL, "row index 0 outside 1..5")},
    "row_index_m_plus_1": {**same(EINVAL, "row index 4 outside 1..3"), "quadratic_cg": (EINVAL, "row index 6 outside 1..5")},
    "two_entries_swapped": same(EINVAL, ASC),
    "duplicated_entry": same(EINVAL, ASC),
    "nan": nonfinite(),
    "inf": nonfinite(),
    "1e301": nonfinite(),
    "zero_row": {**same(OK, None), "affine_factored": (EINVAL, "row 2 of A is zero (A must have full row rank)")},
    "nnz_0": {**same(OK, None), "affine_factored": (EINVAL, EMPTY), "ls_factored": (EINVAL, EMPTY)},
    "nan_in_vector": {**same(EINVAL, "b has non-finite entries"), "quadratic_cg": (EINVAL, "q has non-finite entries")},
}


def test_the_table_names_every_fault_and_entry():
    assert set(FAULTS) == set(MUTATIONS) and all(set(row) == set(ENTRIES) for row in FAULTS.values())


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("fault", list(FAULTS))
def test_single_fault(pkg, entry, fault):
    args = base(entry)
    rc, msg, y = call(pkg, entry, *args)
    assert rc == OK and np.isfinite(y).all(), (entry, msg)                          # the arrays without the fault are accepted
    code, text = FAULTS[fault][entry]
    rc, msg, yf = call(pkg, entry, *MUTATIONS[fault](entry, *args))
    print("%s / %s: %d %r" % (fault, entry, rc, msg if rc else ""))
    assert rc == code, (fault, entry, rc, msg)
    if code == OK:
        assert np.isfinite(yf).all()
    else:
        assert msg == WHAT[entry] + ": " + text, (fault, entry, msg)
    assert call(pkg, entry, *args)[2].tobytes() == y.tobytes()                      # and a refusal leaves nothing behind


# ---------------------------------------------------------------------------------------------- the CSR pair, at the shapes where a counting pass goes wrong
def _full_rank(rng, m, n, A):
    """A with a band entry 2 + U(0, 1) per row added at column 1 + i (the columns 0 and n - 1 are left to the caller)"""
    return sp.csc_matrix(A + sp.csc_matrix((2.0 + rng.random(m), (np.arange(m), 1 + np.arange(m))), shape=(m, n)))


def pair_shapes():
    rng = np.random.default_rng(20)
    out = {}
    A = sp.lil_matrix((4, 7))
    A[[0, 2, 3, 1], [3, 3, 5, 5]] = rng.standard_normal(4)
    out["first_and_last_column_empty"] = _full_rank(rng, 4, 7, A.tocsc())
    A = _full_rank(rng, 4, 7, sp.random(4, 7, 0.4, random_state=3, format="csc")).tolil()
    A[2, :] = 0.0
    out["empty_row"] = sp.csc_matrix(A)
    out["m1"] = sp.csc_matrix(np.array([[0.0, 1.5, 0.0, -2.0, 0.25, 0.0]]))
    out["1x1"] = sp.csc_matrix(np.array([[3.0]]))
    out["n1"] = sp.csc_matrix(np.array([[1.0], [0.0], [-2.0], [0.5], [0.0]]))
    D = sp.lil_matrix((6, 8))
    D[np.arange(6), 1 + np.arange(6)] = 2.0 + rng.random(6)
    D[:, 0] = rng.standard_normal((6, 1))
    out["dense_column_beside_a_diagonal"] = sp.csc_matrix(D)
    R = sp.lil_matrix((3, 260))
    R[0, 40 + np.arange(200)] = rng.standard_normal(200)
    out["row_of_200"] = _full_rank(rng, 3, 260, R.tocsc())
    for A in out.values():
        A.eliminate_zeros()
    return out


PAIR = pair_shapes()
NOT_FOR = {"affine_factored": ("empty_row", "n1"), "ls_factored": ("n1",)}          # a zero row; m > n


@pytest.mark.parametrize("entry,shape", [(e, s) for e in ["affine_factored", "ls_factored", "ls_normal", "ls_cg"] for s in PAIR if s not in NOT_FOR.get(e, ())])
def test_pair_against_scipy(pkg, monkeypatch, entry, shape):
    monkeypatch.setenv("FOS_SF_SEG", "64")                                          # (the factored forms: the row of 200 is cut in four)
    A = PAIR[shape]
    m, n = A.shape
    rng = np.random.default_rng(m + n)
    b, x = rng.standard_normal(m), rng.standard_normal(n)
    keep, _ = sf.csc_args(pkg, A)
    rc, msg, y = call(pkg, entry, m, n, *keep, b, x=x)
    assert rc == OK, (entry, shape, msg)
    At = sp.csr_matrix(A.T)
    if entry in ("affine_factored", "ls_factored"):
        lam = 0.0 if entry == "affine_factored" else LAM
        G = (A @ At).toarray() + (np.eye(m) / lam if lam else 0.0)
        ref = x - At @ np.linalg.solve(G, A @ x - b)
        err, bar = float(np.abs(y - ref).max()), sf.TOL * max(1.0, float(np.abs(x).max()))
    elif entry == "ls_normal":
        ref = cg.splu_ls(A, b, LAM, x)
        err, bar = float(np.abs(y - ref).max()), nc.bar(np.eye(n) + LAM * (At @ A).toarray(), x, ref)
    else:
        ref = cg.splu_ls(A, b, LAM, x)
        err, bar = float(np.linalg.norm(y - ref)), cg.ls_bar(A, b, LAM, x, ref)
    print("%s / %s: error %.2e (bar %.2e)" % (entry, shape, err, bar))
    assert err <= bar, (entry, shape, err, bar)


@pytest.mark.parametrize("shape", ["first_and_last_column_empty", "1x1", "arrow", "row_of_200"])
def test_quadratic_mirror_against_scipy(pkg, shape):
    rng = np.random.default_rng(len(shape))
    n = {"first_and_last_column_empty": 7, "1x1": 1, "arrow": 8, "row_of_200": 260}[shape]
    Q = sp.lil_matrix((n, n))
    if shape == "first_and_last_column_empty":
        Q[1:6, 1:6] = sp.diags([[-0.5] * 4, [2.0] * 5, [-0.5] * 4], [-1, 0, 1]).toarray()
    elif shape == "1x1":
        Q[0, 0] = 3.0
    else:                                                                           # column 0 (and row 0) full beside a dominant diagonal
        k = n if shape == "arrow" else 201
        Q[np.arange(n), np.arange(n)] = float(k)
        Q[1:k, 0] = rng.uniform(-0.9, 0.9, (k - 1, 1))
        Q[0, 1:k] = Q[1:k, 0].T
    Q = sp.csc_matrix(Q)
    q, x = rng.standard_normal(n), rng.standard_normal(n)
    keep, _ = sf.csc_args(pkg, Q)
    rc, msg, y = call(pkg, "quadratic_cg", n, n, *keep, q, x=x)
    assert rc == OK, (shape, msg)
    ref = cg.splu_quadratic(Q, q, x)
    err, bar = float(np.linalg.norm(y - ref)), cg.quadratic_bar(Q, q, x, ref)
    print("quadratic_cg / %s: error %.2e (bar %.2e)" % (shape, err, bar))
    assert err <= bar, (shape, err, bar)
