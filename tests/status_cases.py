"""
The operators and the points on which the status epilogue is compared with tests/status_reference.py: shared by the CPU test of the
reference itself (test_status_reference.py) and the device test (test_gpu_status_formats.py), so that the seeds are chosen where no GPU is
needed: on every case here the reference is farther from each threshold of the decision than its allowance (asserted on the CPU).
"""
import zlib

import numpy as np
import scipy.sparse as sp

EPS = (1e-3, 1e-8)
WINDOW_NAMES = ("wide", "tall", "mid", "tiny")


def _seed(*parts):
    return zlib.crc32("/".join(str(p) for p in parts).encode())


def row_block_shapes():
    """test_gpu_parity.shapes(): ELL / LDS / LONG row blocks, run-compressed values, dual tiles with deferred rows, all-zero"""
    import test_gpu_parity
    return test_gpu_parity.shapes(None)


def window_shapes():
    """the four matrices of test_operators_on_forced_window_panels"""
    import test_gpu_parity
    return list(zip(WINDOW_NAMES, test_gpu_parity.window_panel_shapes(np.random.default_rng(77))))


def vectors_for(name, A):
    """b, c of an operator: unit-scale random"""
    m, n = A.shape
    rng = np.random.default_rng(_seed("bc", name))
    return rng.standard_normal(m), rng.standard_normal(n)


def split(z, m, n):
    l = n + m + 1
    return z[0:n], z[n:n + m], z[l:l + n], z[l + n:l + n + m]


def scaled_problem(name, A, b, c):
    """rows of A, entries of b and c, and the x, y, r, s entries of z each scaled by its own 10**uniform(-6, 6)"""
    m, n = A.shape
    l = n + m + 1
    rng = np.random.default_rng(_seed("scaled", name))
    pw = lambda k: 10.0 ** rng.uniform(-6, 6, k)
    As = sp.csc_matrix(sp.diags(pw(m)) @ A)
    As.sort_indices()
    bs, cs = b * pw(m), c * pw(n)
    z = rng.standard_normal(2 * l) * pw(2 * l)
    z[l - 1], z[2 * l - 1] = 1.0 + rng.random(), rng.random()
    return As, bs, cs, z


def points(name, A, b, c):
    """[(label, z)] on the operator as it stands (the scaled case needs its own operator: scaled_problem)"""
    m, n = A.shape
    l = n + m + 1
    rng = np.random.default_rng(_seed("z", name))
    out = []
    for tau in (1e-6, 1.0, 1e6):
        z = rng.standard_normal(2 * l)
        z[l - 1] = tau
        out.append(("unit tau=%g" % tau, z))
    # one row and one column: x_j, r_j, y_i, s_i of a stored entry (i, j) where there is one
    z = np.zeros(2 * l)
    coo = sp.coo_matrix(A)
    if coo.nnz:
        k = int(rng.integers(coo.nnz))
        i, j = int(coo.row[k]), int(coo.col[k])
    else:
        i, j = m // 2, n // 2
    z[j], z[n + i], z[l + j], z[l + n + i] = rng.standard_normal(4) + 3.0
    z[l - 1], z[2 * l - 1] = 1.0, 0.5
    out.append(("one row, one column", z))
    z = rng.standard_normal(2 * l)
    z[l - 1] = -0.7
    out.append(("tau<0", z))
    z = rng.standard_normal(2 * l)
    z[l - 1] = 0.0
    out.append(("tau=0", z))
    # exactly consistent (to fp64 rounding of the products): s = b - A x, r = c + A'y, tau = 1
    z = rng.standard_normal(2 * l)
    x, y, _, _ = split(z, m, n)
    z[l - 1] = 1.0
    z[l:l + n] = c + A.T @ y
    z[l + n:l + n + m] = b - A @ x
    out.append(("consistent", z))
    return out


def certificates(A, b, c):
    """[(expected status, z)]: one constructed point per verdict, each far (>= 1e-3 relative) from every threshold at both EPS.
    Needs a left null vector of A' (dense QR: for small or thin A only)."""
    m, n = A.shape
    l = n + m + 1
    rng = np.random.default_rng(_seed("cert", m, n))
    Ad = A.toarray()
    out = []
    # Optimal: a consistent point with c'x + b'y = 0
    z = rng.standard_normal(2 * l)
    x, y, _, _ = split(z, m, n)
    x = x - c * ((c @ x + b @ y) / (c @ c))
    z[0:n], z[l - 1], z[2 * l - 1] = x, 1.0, 0.0
    z[l:l + n] = c + Ad.T @ y
    z[l + n:l + n + m] = b - Ad @ x
    out.append(("Optimal", z))
    # Unbounded: A x + s = 0 with c'x < 0 (and a dual residual of order one)
    z = np.zeros(2 * l)
    x = -c + 0.1 * rng.standard_normal(n)
    z[0:n], z[l - 1], z[2 * l - 1] = x, 1.0, 1.0
    z[n:n + m] = 0.1 * rng.standard_normal(m)                # (y = 0 would put the Infeasible test exactly on its threshold, 0 <= 0)
    z[l + n:l + n + m] = -(Ad @ x)
    out.append(("Unbounded", z))
    # Infeasible: A'y = 0 with b'y < 0; c'x > 0 so that the Unbounded test before it is false
    Qf, _ = np.linalg.qr(Ad)                                  # columns span range(A); y = (I - Q Q') y0 is orthogonal to it
    y0 = -b + 0.1 * rng.standard_normal(m)
    y = y0 - Qf @ (Qf.T @ y0)
    y = y - Qf @ (Qf.T @ y)
    z = rng.standard_normal(2 * l)
    z[0:n], z[n:n + m], z[l - 1] = 0.1 * c, y, 1.0
    out.append(("Infeasible", z))
    # Continue: a unit-scale random point
    z = rng.standard_normal(2 * l)
    z[l - 1] = 1.0
    out.append(("Continue", z))
    return out
