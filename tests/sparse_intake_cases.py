"""The single-fault table of the sparse intake, shared by tests/test_sparse_intake_cpu.py and tests/test_gpu_sparse_affine.py: the base arrays and, per fault, the
function that puts that fault alone into them."""
import numpy as np
import scipy.sparse as sp


def base(entry):
    """-> (rows, cols, colptr, rowval, nzval, vec): 3 x 5 of full row rank with two two-entry columns in front, or a 5 x 5 tridiagonal Q >= 0; 1-based"""
    if entry == "quadratic_cg":
        Q = sp.csc_matrix(sp.diags([[-0.5] * 4, [2.0] * 5, [-0.5] * 4], [-1, 0, 1]).toarray())
        return 5, 5, Q.indptr.astype(np.int64) + 1, Q.indices.astype(np.int64) + 1, Q.data.astype(np.float64), np.array([0.3, -1.0, 0.5, 2.0, -0.25])
    A = sp.csc_matrix(np.array([[2.0, 0, 1, 0, 3], [0, 4.0, 1, 0, 0], [1.0, 0, 0, 5, 2]]))
    return 3, 5, A.indptr.astype(np.int64) + 1, A.indices.astype(np.int64) + 1, A.data.astype(np.float64), np.array([1.0, -2.0, 0.5])


def swap01(a):
    a = a.copy()
    a[[0, 1]] = a[[1, 0]]
    return a


def put(a, i, v):
    a = a.copy()
    a[i] = v
    return a


def empty_row2(entry, rows, cols, cp, rv, nz, vec):
    """row 2 (and, of Q, column 2) without a stored entry"""
    col = np.repeat(np.arange(1, cols + 1), np.diff(cp))
    keep = (rv != 2) & ((col != 2) | (entry != "quadratic_cg"))
    return rows, cols, np.r_[1, 1 + np.cumsum(np.bincount(col[keep] - 1, minlength=cols))], rv[keep], nz[keep], vec


# fault -> the arrays with that fault alone
MUTATIONS = {
    "colptr0_is_0": lambda e, r, c, cp, rv, nz, v: (r, c, put(cp, 0, 0), rv, nz, v),
    "colptr_decreases": lambda e, r, c, cp, rv, nz, v: (r, c, np.r_[cp[0], cp[2], cp[1], cp[3:]], rv, nz, v),
    "row_index_0": lambda e, r, c, cp, rv, nz, v: (r, c, cp, put(rv, 1, 0), nz, v),
    "row_index_m_plus_1": lambda e, r, c, cp, rv, nz, v: (r, c, cp, put(rv, 1, r + 1), nz, v),
    "two_entries_swapped": lambda e, r, c, cp, rv, nz, v: (r, c, cp, swap01(rv), swap01(nz), v),
    "duplicated_entry": lambda e, r, c, cp, rv, nz, v: (r, c, cp, put(rv, 1, rv[0]), nz, v),
    "nan": lambda e, r, c, cp, rv, nz, v: (r, c, cp, rv, put(nz, 3, np.nan), v),
    "inf": lambda e, r, c, cp, rv, nz, v: (r, c, cp, rv, put(nz, 3, -np.inf), v),
    "1e301": lambda e, r, c, cp, rv, nz, v: (r, c, cp, rv, put(nz, 3, 1e301), v),
    "zero_row": empty_row2,
    "nnz_0": lambda e, r, c, cp, rv, nz, v: (r, c, np.ones(c + 1, dtype=np.int64), rv[:0], nz[:0], v),
    "nan_in_vector": lambda e, r, c, cp, rv, nz, v: (r, c, cp, rv, nz, put(v, 1, np.nan)),
}
