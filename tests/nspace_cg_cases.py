"""Instances, references and the error bar of the cg forms (csrc/nspace_cg.hip): Quadratic(Q, q, form="cg") and LeastSquares(A, b, lam, form="cg"), whose prox
y = M^-1 (x + c), M = I + Q resp. I + lam A'A, c = -q resp. lam A'b, is solved by warm-started Jacobi-preconditioned CG.  Seeded; shared by the CPU emulation
tests and the GPU tests; every reference is computed once and cached.

The bar is derived, not tuned.  lambda_min(M) >= 1, so |y - y*|_2 <= |r_true|_2 with r_true = x + c - M y.  The prox ends when the residual IT EVALUATES is at most
max(tol |x + c|_2, 16 eps level), level = | |M||y| + |x + c| |_2, and evaluating a row of l entries errs by at most (l + 2) eps times the same row of level
(l products and sums, the sum x + c, the subtraction).  So
    |y - y*|_2  <=  (16 + l + 2) eps level + tol |x + c|_2,     l = the longest row of M,
with level computed HERE by numpy from the reference answer.  LeastSquares evaluates M y as y + lam A'(A y): |M| is read as I + lam |A'||A| (what the device sums
and what bounds its rounding) and l is the longest row of A plus the longest row of A'.

References: the dense Cholesky solve with two refinement steps whose residual is evaluated in np.longdouble (nspace_cases.RefQuadratic, prox_fn_cases.RefLeastSquares);
the two cases beyond the dense forms: scipy.sparse.linalg.splu with the same two refinement steps, the residual summed entry by entry in np.longdouble."""
import ctypes as C
import functools

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import nspace_cases as nc
from prox_fn_cases import RefLeastSquares

EPS = 2.0 ** -52
FOS_EINVAL = -1
SMALL = 10              # CG iterations allowed beyond n on the tiny shapes: exact CG ends in n, each restart on the recomputed residual may add a few
QUAD_CASES = ["n1", "n63", "n64", "n65", "diag", "tridiag300", "arrow3000", "empty_rows", "zero"]
LS_CASES = ["1x1", "50x1", "9x7", "7x9", "tall5000x40", "zero_col", "zero_row", "dup_rows", "dense_col3000"]
TINY = {"n1": 1, "n63": 63, "n64": 64, "n65": 65, "1x1": 1, "50x1": 1, "9x7": 7, "7x9": 9}      # cases held to n + SMALL iterations


def _sym_psd(n, rng, per_row=4):
    """B'B + a diagonal for a sparse B: symmetric positive semidefinite with a few entries per row"""
    B = sp.random(n, n, density=min(1.0, per_row / n), random_state=np.random.RandomState(int(rng.integers(1 << 30))), data_rvs=rng.standard_normal)
    Q = (B.T @ B).tocsc() + sp.diags(rng.random(n))
    return sp.csc_matrix((Q + Q.T) * 0.5)


@functools.lru_cache(maxsize=None)
def quadratic_case(name):
    """-> (Q csc symmetric, q, x)"""
    rng = np.random.default_rng([7, QUAD_CASES.index(name)])
    if name in ("n1", "n63", "n64", "n65"):
        n = int(name[1:])
        Q = _sym_psd(n, rng)
    elif name == "diag":
        n = 100
        Q = sp.diags(10.0 ** rng.uniform(-2, 2, n)).tocsc()
    elif name == "tridiag300":
        n = 300
        Q = (10.0 * sp.diags([-np.ones(n - 1), 2.0 * np.ones(n), -np.ones(n - 1)], [-1, 0, 1])).tocsc()
    elif name == "arrow3000":                                  # one row and column of 3 000 entries: crosses a 2 048-entry segment
        n = 3000
        v = 0.02 * rng.standard_normal(n)
        Q = sp.lil_matrix((n, n))
        Q.setdiag(1.0 + rng.random(n))
        Q[0, :] = v
        Q[:, 0] = v.reshape(-1, 1)
        Q[0, 0] = 5.0                                           # (diagonally dominant: positive definite)
        Q = Q.tocsc()
    elif name == "empty_rows":                                 # rows / columns 40..119 and the last one hold nothing
        n = 200
        Q = sp.lil_matrix((n, n))
        Q[:40, :40] = _sym_psd(40, rng).toarray()
        Q[120:199, 120:199] = _sym_psd(79, rng).toarray()
        Q = Q.tocsc()
    else:                                                      # "zero"
        n = 50
        Q = sp.csc_matrix((n, n))
    Q = sp.csc_matrix(Q, dtype=np.float64)
    Q.sum_duplicates(); Q.sort_indices()
    return Q, rng.standard_normal(n), rng.standard_normal(n)


@functools.lru_cache(maxsize=None)
def ls_case(name):
    """-> (A csc, b, x)"""
    rng = np.random.default_rng([11, LS_CASES.index(name)])
    if name in ("1x1", "50x1", "9x7"):
        m, n = (int(v) for v in name.split("x"))
        A, b = nc.instance("gauss", m, n)
    elif name == "7x9":
        A, b = nc.instance("wide", 7, 9)
    elif name == "tall5000x40":
        A, b = nc.tall_sparse(5000, 40, 3)
    elif name == "zero_col":
        A, b = nc.instance("zero_col", 60, 33)
    elif name == "zero_row":
        A, b = nc.instance("gauss", 40, 30)
        A[5, :] = 0.0
    elif name == "dup_rows":
        A0, b0 = nc.instance("gauss", 20, 30)
        A, b = np.vstack([A0, A0]), np.r_[b0, b0]
    else:                                                      # "dense_col3000": column 0 has 3 000 entries, the others three each
        A, b = nc.tall_sparse(3000, 20, 3)
        A = sp.lil_matrix(A)
        A[:, 0] = 0.05 * rng.standard_normal((3000, 1))
        A = A.tocsc()
    A = sp.csc_matrix(A, dtype=np.float64)
    A.eliminate_zeros(); A.sum_duplicates(); A.sort_indices()
    return A, np.asarray(b, dtype=np.float64), rng.standard_normal(A.shape[1])


def sym_lower(Q):
    """the matrix the cg form reads: the entries i >= j of Q, mirrored"""
    L = sp.tril(sp.csc_matrix(Q), 0)
    return sp.csc_matrix(L + sp.tril(L, -1).T)


def _longest(M):
    M = sp.csr_matrix(M)
    return int(np.diff(M.indptr).max(initial=0))


def quadratic_bar(Q, q, x, yref, tol=0.0):
    """(16 + l + 2) eps | |M||y*| + |x - q| |_2 + tol |x - q|_2, M = I + Q, l = its longest row"""
    M = sp.csr_matrix(sp.identity(Q.shape[0]) + sym_lower(Q))
    rhs = x - q
    level = float(np.linalg.norm(abs(M) @ np.abs(yref) + np.abs(rhs)))
    return (16 + _longest(M) + 2) * EPS * level + tol * float(np.linalg.norm(rhs))


def ls_bar(A, b, lam, x, yref, tol=0.0):
    """the same with |M| = I + lam |A'||A| and l = the longest row of A plus the longest row of A'"""
    A = sp.csr_matrix(A)
    rhs = x + lam * (A.T @ b)
    level = float(np.linalg.norm(np.abs(yref) + lam * (abs(A).T @ (abs(A) @ np.abs(yref))) + np.abs(rhs)))
    return (16 + _longest(A) + _longest(A.T) + 2) * EPS * level + tol * float(np.linalg.norm(rhs))


@functools.lru_cache(maxsize=None)
def quadratic_ref(name):
    Q, q, x = quadratic_case(name)
    return nc.RefQuadratic(sym_lower(Q).toarray(), q).project(x)


@functools.lru_cache(maxsize=None)
def ls_ref(name, lam):
    A, b, x = ls_case(name)
    return RefLeastSquares(A.toarray(), b, lam).project(x)


def _ld_matvec(M, v):
    """M v with every product and sum in np.longdouble (M sparse)"""
    M = sp.coo_matrix(M)
    out = np.zeros(M.shape[0], dtype=np.longdouble)
    np.add.at(out, M.row, M.data.astype(np.longdouble) * v[M.col])
    return out


def splu_quadratic(Q, q, x):
    """(I + Q)^-1 (x - q) by splu and two refinement steps with a longdouble residual"""
    L = np.longdouble
    M = sp.csc_matrix(sp.identity(Q.shape[0]) + sym_lower(Q))
    lu = spla.splu(M)
    rhs = x.astype(L) - q.astype(L)
    y = lu.solve(x - q).astype(L)
    for _ in range(2):
        y = y + lu.solve((rhs - _ld_matvec(M, y)).astype(np.float64)).astype(L)
    return y.astype(np.float64)


def splu_ls(A, b, lam, x):
    """(I + lam A'A)^-1 (x + lam A'b) by splu and two refinement steps, the residual evaluated from A itself in longdouble"""
    L = np.longdouble
    A = sp.csc_matrix(A)
    lu = spla.splu(sp.csc_matrix(sp.identity(A.shape[1]) + lam * (A.T @ A)))
    rhs = x.astype(L) + L(lam) * _ld_matvec(A.T, b.astype(L))
    y = lu.solve(rhs.astype(np.float64)).astype(L)
    for _ in range(2):
        res = rhs - y - L(lam) * _ld_matvec(A.T, _ld_matvec(A, y))
        y = y + lu.solve(res.astype(np.float64)).astype(L)
    return y.astype(np.float64)


def certified_ls(A, b, lam, x):
    """-> (y, e) with |y - y*|_2 <= e for y* = (I + lam A'A)^-1 (x + lam A'b), WITHOUT a factorisation: scipy's CG, refined three times on a residual summed entry by
    entry in np.longdouble from A itself; e is the 2-norm of the last such residual, which bounds the error because lambda_min(I + lam A'A) >= 1.  For
    tall_sparse(120 000, 50 000, 3): A'A is a random graph of mean degree 6 on 50 000 nodes, and splu of I + lam A'A fills in until it takes far longer than a test
    may (see test_gpu_nspace_cg.py); the caller asserts that e is negligible against its bar."""
    L = np.longdouble
    A = sp.csr_matrix(A)
    At = sp.csr_matrix(A.T)
    n = A.shape[1]
    op = spla.LinearOperator((n, n), matvec=lambda v: v + lam * (At @ (A @ v)), dtype=np.float64)
    rhs = x.astype(L) + L(lam) * _ld_matvec(At, b.astype(L))
    residual = lambda y: rhs - y - L(lam) * _ld_matvec(At, _ld_matvec(A, y))
    y = np.zeros(n, dtype=L)
    for _ in range(3):
        d, info = spla.cg(op, residual(y).astype(np.float64), rtol=1e-12, atol=0.0, maxiter=5000)
        assert info == 0
        y = y + d.astype(L)
    return y.astype(np.float64), float(np.linalg.norm(residual(y)))


def pentadiagonal(n):
    """a positive definite pentadiagonal Q (the fourth-difference stencil) with q, x"""
    rng = np.random.default_rng([13, n])
    Q = sp.diags([np.ones(n - 2), -4.0 * np.ones(n - 1), 6.5 * np.ones(n), -4.0 * np.ones(n - 1), np.ones(n - 2)], [-2, -1, 0, 1, 2]).tocsc()
    Q.sort_indices()
    return Q, rng.standard_normal(n), rng.standard_normal(n)


# ---- the host emulations (no GPU)
def _i32(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def host_quadratic_cg(pkg, Q, q, x, tol=0.0, raw=None):
    """fos_host_quadratic_cg -> (rc, y, iterations); raw = (colptr, rowval, nzval) replaces the arrays of Q (refusals)"""
    keep, ptrs = nc.csc_ptrs(pkg, Q)
    if raw is not None:
        keep = tuple(np.ascontiguousarray(a) for a in raw)
        ptrs = (keep[0].ctypes.data_as(C.POINTER(C.c_int64)), keep[1].ctypes.data_as(C.POINTER(C.c_int64)), pkg.lib.dptr(keep[2]))
    q, x = np.ascontiguousarray(q, dtype=np.float64), np.ascontiguousarray(x, dtype=np.float64)
    y, it = np.full(x.shape[0], np.nan), np.zeros(1, dtype=np.int32)
    rc = pkg.lib.load().fos_host_quadratic_cg(x.shape[0], ptrs[0], ptrs[1], ptrs[2], pkg.lib.dptr(q), tol, pkg.lib.dptr(x), pkg.lib.dptr(y), _i32(it))
    return rc, y, int(it[0])


def host_ls_cg(pkg, A, b, lam, x, tol=0.0, raw=None):
    """fos_host_least_squares_cg -> (rc, y, iterations)"""
    m, n = A.shape
    keep, ptrs = nc.csc_ptrs(pkg, A)
    if raw is not None:
        keep = tuple(np.ascontiguousarray(a) for a in raw)
        ptrs = (keep[0].ctypes.data_as(C.POINTER(C.c_int64)), keep[1].ctypes.data_as(C.POINTER(C.c_int64)), pkg.lib.dptr(keep[2]))
    b, x = np.ascontiguousarray(b, dtype=np.float64), np.ascontiguousarray(x, dtype=np.float64)
    y, it = np.full(n, np.nan), np.zeros(1, dtype=np.int32)
    rc = pkg.lib.load().fos_host_least_squares_cg(m, n, ptrs[0], ptrs[1], ptrs[2], pkg.lib.dptr(b), lam, tol, pkg.lib.dptr(x), pkg.lib.dptr(y), _i32(it))
    return rc, y, int(it[0])
