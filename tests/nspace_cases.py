"""Instances, references and the accuracy bar of the n-space forms (csrc/nspace.hip): Quadratic(Q, q) and LeastSquares(A, b, lam) in the normal-equations form,
whose prox is y = M^-1 (x + c) with M = I + Q resp. I + lam A'A.  Seeded; shared by the CPU emulation tests and the GPU tests.

The bar:  TOL max(1, cond(Mt) / 1e3) max(1, |x|_inf, |y_ref|_inf),  TOL = 1e-12 (the project's constant), Mt = D M D with D = diag(M)^-1/2 (what the device
inverts) and cond(Mt) computed by numpy from the instance.  The forward error of an fp64 solve grows as eps cond, and TOL is 4.5 eps 1e3.  A numpy restatement of
the prox formula (z = K w, z += K (w - Mt z), y = D z) measured, worst case: 2.7e-14 up to cond 1.8e3; 3.0e-13 at cond 4e4 (gauss 65 x 64, lam = 1e3; bar 4e-11);
2.2e-13 on `corr` (1000, 200); 1.4e-13 on `rows` (1000, 200): the formula alone stays a factor of at least 30 inside the bar.

NOT held to it: `cols`, columns scaled by 10^U(-3, 3).  The Gram matrix A'A formed in fp64 loses it (the restatement: 1.1e-11 relative at cond(Mt) = 6): that family
is checked device against host emulation only, its error against the reference printed."""
import ctypes as C

import numpy as np
import scipy.linalg
import scipy.sparse as sp

TOL = 1e-12
# (m, n) of the dense instances: tile edge (64 / 65), strip edge (33 columns and up), one entry, a single column, tall and very tall
SHAPES = [(1, 1), (50, 1), (9, 7), (65, 64), (131, 65), (330, 300), (1000, 300), (5000, 40)]
LAMS = [1e-3, 1.0, 1e3]
EXTRA = [("corr", 1000, 200), ("rows", 1000, 200), ("wide", 7, 9), ("zero_col", 60, 33), ("rankdef", 80, 40)]
HELD = ("gauss", "corr", "rows", "wide", "zero_col", "rankdef")            # families held to the bar; "cols" is not
FOS_EINVAL, FOS_EUNSUPPORTED = -1, -4


def instance(family, m, n):
    """-> (A m x n, b): gauss; corr = gauss + 3 u v'; rows / cols = rows / columns scaled by 10^U(-3, 3); wide = gauss with m < n; zero_col: column n // 2 zero;
    rankdef: the second half of the columns repeats the first."""
    rng = np.random.default_rng([m, n, ["gauss", "corr", "rows", "cols", "wide", "zero_col", "rankdef"].index(family)])
    A = rng.standard_normal((m, n))
    if family == "corr":
        A = A + 3.0 * rng.standard_normal((m, 1)) @ rng.standard_normal((1, n))
    elif family == "rows":
        A = (10.0 ** rng.uniform(-3.0, 3.0, m))[:, None] * A
    elif family == "cols":
        A = A * (10.0 ** rng.uniform(-3.0, 3.0, n))[None, :]
    elif family == "zero_col":
        A[:, n // 2] = 0.0
    elif family == "rankdef":
        A[:, n // 2:2 * (n // 2)] = A[:, :n // 2]
    b = A @ np.maximum(rng.standard_normal(n), 0.0) + 0.1 * rng.standard_normal(m)
    return np.ascontiguousarray(A), b


def quadratic_of(A, b, lam):
    """the Quadratic with the same n-space matrix as LeastSquares(A, b, lam): Q = lam A'A (made exactly symmetric), q = -lam A'b"""
    Q = lam * (A.T @ A)
    Q = np.tril(Q) + np.tril(Q, -1).T
    return np.ascontiguousarray(Q), -lam * (A.T @ b)


def tall_sparse(m, n, per_col, seed=0):
    """m x n sparse, m > n: `per_col` entries per column at random rows plus one on a band"""
    rng = np.random.default_rng([m, n, per_col, seed])
    cols = np.repeat(np.arange(n), per_col)
    rows = rng.integers(0, m, n * per_col)
    A = sp.csc_matrix((np.r_[rng.standard_normal(n * per_col), 2.0 + rng.random(n)], (np.r_[rows, (np.arange(n) * (m // n)) % m], np.r_[cols, np.arange(n)])), shape=(m, n))
    A.sum_duplicates(); A.sort_indices()
    return A, rng.standard_normal(m)


def scaled_cond(M):
    """cond(D M D), D = diag(M)^-1/2"""
    d = 1.0 / np.sqrt(np.diag(M))
    return float(np.linalg.cond(d[:, None] * M * d[None, :]))


def bar(M, x, yref):
    return TOL * max(1.0, scaled_cond(M) / 1e3) * max(1.0, float(np.abs(x).max()), float(np.abs(yref).max()))


class RefQuadratic:
    """f(x) = 1/2 x'Qx + q'x: the Cholesky solve of (I + Q) y = x - q followed by two refinement steps whose residual is evaluated in np.longdouble (the pattern of
    prox_fn_cases.RefLeastSquares, which serves the LeastSquares instances here, tall A included)."""
    calls = 0

    def __init__(self, Q, q):
        self.Q, self.q = np.array(Q, dtype=np.float64), np.array(q, dtype=np.float64)
        n = self.Q.shape[0]
        self.M = np.eye(n) + self.Q
        self.chol = scipy.linalg.cho_factor(self.M)
        self.ML, self.qL = self.M.astype(np.longdouble), self.q.astype(np.longdouble)

    def project(self, x):
        L = np.longdouble
        rhs = x.astype(L) - self.qL
        y = scipy.linalg.cho_solve(self.chol, x - self.q).astype(L)
        for _ in range(2):
            res = rhs - self.ML @ y
            y = y + scipy.linalg.cho_solve(self.chol, res.astype(np.float64)).astype(L)
        return y.astype(np.float64)

    def prox(self, y, x):
        self.calls += 1
        y[:] = self.project(np.asarray(x, dtype=np.float64))

    def value(self, x):
        return 0.5 * float(x @ (self.Q @ x)) + float(self.q @ x)


def csc_ptrs(pkg, A):
    """the 1-based CSC arrays of the C ABI (kept alive by the caller) and their pointers"""
    A = sp.csc_matrix(A, dtype=np.float64)
    A.sum_duplicates(); A.sort_indices()
    keep = (np.ascontiguousarray(A.indptr, dtype=np.int64) + 1, np.ascontiguousarray(A.indices, dtype=np.int64) + 1, np.ascontiguousarray(A.data, dtype=np.float64))
    i64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
    return keep, (i64(keep[0]), i64(keep[1]), pkg.lib.dptr(keep[2]))


def host_quadratic(pkg, Q, q, x):
    Q, q, x = (np.ascontiguousarray(v, dtype=np.float64) for v in (Q, q, x))
    y = np.full(x.shape[0], np.nan)
    return pkg.lib.load().fos_host_quadratic(x.shape[0], pkg.lib.dptr(Q), pkg.lib.dptr(q), pkg.lib.dptr(x), pkg.lib.dptr(y)), y


def host_ls_normal(pkg, A, b, lam, x):
    A, b, x = (np.ascontiguousarray(v, dtype=np.float64) for v in (A, b, x))
    y = np.full(A.shape[1], np.nan)
    return pkg.lib.load().fos_host_least_squares_normal(A.shape[0], A.shape[1], pkg.lib.dptr(A), pkg.lib.dptr(b), lam, pkg.lib.dptr(x), pkg.lib.dptr(y)), y


def host_ls_sparse(pkg, A, b, lam, form, x, raw=None):
    """fos_host_least_squares_sparse; form: "normal" | "sparse_factored" or a raw code; raw = (colptr, rowval, nzval) replaces the arrays of A (refusals)"""
    m, n = A.shape
    keep, ptrs = csc_ptrs(pkg, A)
    if raw is not None:
        keep = tuple(np.ascontiguousarray(a) for a in raw)
        ptrs = (keep[0].ctypes.data_as(C.POINTER(C.c_int64)), keep[1].ctypes.data_as(C.POINTER(C.c_int64)), pkg.lib.dptr(keep[2]))
    b, x = np.ascontiguousarray(b, dtype=np.float64), np.ascontiguousarray(x, dtype=np.float64)
    y = np.full(n, np.nan)
    code = pkg.lib.LS_FORM_CODES[form] if isinstance(form, str) else form
    return pkg.lib.load().fos_host_least_squares_sparse(m, n, ptrs[0], ptrs[1], ptrs[2], pkg.lib.dptr(b), lam, code, pkg.lib.dptr(x), pkg.lib.dptr(y)), y


def host_symv_packed(pkg, X, v, count=False):
    k = X.shape[0]
    Xc = np.asfortranarray(X, dtype=np.float64)                  # column-major
    v = np.ascontiguousarray(v, dtype=np.float64)
    y = np.full(k, np.nan)
    cnt = np.zeros((k, k), dtype=np.int32, order="F") if count else None
    rc = pkg.lib.load().fos_host_symv_packed(k, Xc.ctypes.data_as(C.POINTER(C.c_double)), pkg.lib.dptr(v), pkg.lib.dptr(y),
                                             cnt.ctypes.data_as(C.POINTER(C.c_int32)) if count else None)
    return rc, y, cnt


def box_qp_residual(Q, q, lo, hi, x):
    """the projected-gradient residual of min 1/2 x'Qx + q'x over [lo, hi]^n: |x - clip(x - (Q x + q), lo, hi)|_inf"""
    return float(np.abs(x - np.clip(x - (Q @ x + q), lo, hi)).max())
