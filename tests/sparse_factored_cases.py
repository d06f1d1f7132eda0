"""Instances of the sparse factored IndAffine's tests (CPU emulation and GPU), seeded.  `rand`: the instances of test_gpu_sparse_affine.py restated; `skew`: a few
rows of given lengths among short ones, one (nearly) dense column and one empty column; `dense_column`: column 0 full; `band`: a banded Toeplitz matrix.  In every
family b = A max(randn, 0)."""
import numpy as np
import scipy.sparse as sp

TOL = 1e-12                                          # the project's tolerance for an exact affine projection, times max(1, |x|_inf) (affine_factored_cases.TOL)

# (m, n, entries per row, decades of row scaling)
RAND_SHAPES = [(300, 1000, 6, 0.0), (900, 1000, 3, 0.0), (1500, 6000, 12, 3.0), (40, 5000, 300, 0.0), (1, 50, 7, 0.0), (64, 640, 5, 0.0), (65, 131, 4, 0.0),
               (7, 9, 3, 0.0)]
HANN4 = np.hanning(6)[1:-1]


def _rhs(rng, A):
    return A @ np.maximum(rng.standard_normal(A.shape[1]), 0.0)


def rand(m, n, per_row, row_scale_decades=0.0):
    """`per_row` entries per row at random columns (+ one on a diagonal band: full row rank)"""
    rng = np.random.default_rng(m + n)
    rows = np.repeat(np.arange(m), per_row)
    cols = rng.integers(0, n, m * per_row)
    vals = rng.standard_normal(m * per_row)
    band = (np.arange(m) * (n // m)) % n
    A = sp.csr_matrix((np.r_[vals, 2.0 + rng.random(m)], (np.r_[rows, np.arange(m)], np.r_[cols, band])), shape=(m, n))
    if row_scale_decades:
        A = sp.diags(10.0 ** rng.uniform(-row_scale_decades, row_scale_decades, m)) @ A
    A = sp.csc_matrix(A)
    return A, _rhs(rng, A)


def skew(m, n, long_rows, short):
    """row i < len(long_rows) stores exactly long_rows[i] entries, the others `short`: a band entry (column 1 + i, 2 + U(0, 1): full row rank), then an entry of
    column 0 (the dense column), then random columns of m + 1 .. n - 2; column n - 1 stays empty."""
    rng = np.random.default_rng(m + n + sum(long_rows))
    assert n - 2 - m >= max(max(long_rows), short) and m + 1 < n
    rows, cols, vals = [], [], []
    for i in range(m):
        k = long_rows[i] if i < len(long_rows) else short
        c = [1 + i] + ([0] if k >= 2 else []) + list(m + 1 + rng.choice(n - 2 - m, max(k - 2, 0), replace=False))
        v = np.r_[2.0 + rng.random(), rng.standard_normal(len(c) - 1)]
        rows += [i] * len(c); cols += c; vals += list(v)
    A = sp.csc_matrix((vals, (rows, cols)), shape=(m, n))
    assert (np.diff(sp.csr_matrix(A).indptr)[:len(long_rows)] == long_rows).all() and A[:, [n - 1]].nnz == 0
    return A, _rhs(rng, A)


def dense_column(m):
    """n = 2 m; column 0 full, two random entries of the columns m + 1 .. and a band entry (column 1 + i) per row"""
    n = 2 * m
    rng = np.random.default_rng(3 * m)
    i = np.arange(m)
    rows = np.r_[i, i, i, i]
    cols = np.r_[np.zeros(m, dtype=int), 1 + i, rng.integers(m + 1, n, m), rng.integers(m + 1, n, m)]
    vals = np.r_[rng.standard_normal(m), 2.0 + rng.random(m), rng.standard_normal(2 * m)]
    A = sp.csc_matrix((vals, (rows, cols)), shape=(m, n))
    return A, _rhs(rng, A)


def band(m, taps):
    """row i holds `taps` at the columns i, i + 1, ...: a banded Toeplitz matrix, n = m + len(taps) - 1"""
    taps = np.asarray(taps, dtype=np.float64)
    n = m + len(taps) - 1
    rng = np.random.default_rng(m + len(taps))
    A = sp.csc_matrix(sp.diags(list(taps), list(range(len(taps))), shape=(m, n)))
    return A, _rhs(rng, A)


# the instances run with FOS_SF_SEG=64 (the CPU file and the GPU file): pass 1 folds (skew), pass 2 folds (the dense columns), a smooth band
def seg64_cases():
    return {"skew": skew(70, 600, [63, 64, 65, 129, 1], 3), "dense_column": dense_column(129), "band": band(300, [1.0, 0.98])}


def csc_args(pkg, A):
    """the 1-based CSC arrays of the C ABI (kept alive by the caller) and their pointers"""
    import ctypes as C
    A = sp.csc_matrix(A, dtype=np.float64)
    A.sum_duplicates(); A.sort_indices()
    colptr = np.ascontiguousarray(A.indptr, dtype=np.int64) + 1
    rowval = np.ascontiguousarray(A.indices, dtype=np.int64) + 1
    nzval = np.ascontiguousarray(A.data, dtype=np.float64)
    i64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
    return (colptr, rowval, nzval), (i64(colptr), i64(rowval), pkg.lib.dptr(nzval))


def host_project(pkg, A, b, refine, x, raw=None):
    """fos_host_affine_sparse_factored; raw = (colptr, rowval, nzval) replaces the arrays of A (refusals)"""
    import ctypes as C
    lib = pkg.lib.load()
    m, n = A.shape
    keep, ptrs = csc_args(pkg, A)
    if raw is not None:
        keep = tuple(np.ascontiguousarray(a) for a in raw)
        ptrs = (keep[0].ctypes.data_as(C.POINTER(C.c_int64)), keep[1].ctypes.data_as(C.POINTER(C.c_int64)), pkg.lib.dptr(keep[2]))
    b, x = np.ascontiguousarray(b, dtype=np.float64), np.ascontiguousarray(x, dtype=np.float64)
    y = np.full(n, np.nan)
    rc = lib.fos_host_affine_sparse_factored(m, n, ptrs[0], ptrs[1], ptrs[2], pkg.lib.dptr(b), refine, pkg.lib.dptr(x), pkg.lib.dptr(y))
    return rc, y


def longdouble_projection(A, b, x):
    """x - A'(A A')^-1 (A x - b) with an 80-bit Cholesky solve (rows scaled to unit norm first)"""
    L = np.longdouble
    Ad = np.asarray(A.toarray(), dtype=L)
    s = 1 / np.sqrt((Ad * Ad).sum(axis=1))
    Ad, bl, xl = Ad * s[:, None], b.astype(L) * s, x.astype(L)
    m = Ad.shape[0]
    G = Ad @ Ad.T
    C = np.zeros((m, m), dtype=L)
    for j in range(m):
        C[j, j] = np.sqrt(G[j, j] - C[j, :j] @ C[j, :j])
        C[j + 1:, j] = (G[j + 1:, j] - C[j + 1:, :j] @ C[j, :j]) / C[j, j]
    r = Ad @ xl - bl
    for j in range(m):                                  # C w = r
        r[j] = (r[j] - C[j, :j] @ r[:j]) / C[j, j]
    for j in range(m - 1, -1, -1):                      # C' d = w
        r[j] = (r[j] - C[j + 1:, j] @ r[j + 1:]) / C[j, j]
    return np.asarray(xl - Ad.T @ r, dtype=np.float64)


def segments(lengths, seg):
    """(rows cut, their segments) of a pass over rows of these lengths"""
    cut = lengths[lengths > seg]
    return len(cut), int(((cut + seg - 1) // seg).sum())
