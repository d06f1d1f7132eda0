"""Instances of the factored dense IndAffine's tests (CPU emulation and GPU), seeded: `gauss` standard normal entries, `scaled` the same with rows
multiplied by 10^U(-3, 3), `corr` gauss plus 3 u v' (correlated rows); in every family b = A max(randn, 0)."""
import numpy as np

TOL = 1e-12                                          # the project's tolerance for an exact affine projection, times max(1, |x|_inf)
SHAPES = [("gauss", 1, 1), ("gauss", 1, 50), ("gauss", 7, 9), ("gauss", 64, 64), ("gauss", 65, 131), ("gauss", 300, 330), ("gauss", 300, 1000),
          ("gauss", 40, 5000), ("scaled", 200, 1000), ("corr", 200, 1000)]


def instance(family, m, n):
    rng = np.random.default_rng(m + n)
    A = rng.standard_normal((m, n))
    if family == "corr":
        A = A + 3.0 * rng.standard_normal((m, 1)) @ rng.standard_normal((1, n))
    if family == "scaled":
        A = (10.0 ** rng.uniform(-3.0, 3.0, m))[:, None] * A
    assert family in ("gauss", "scaled", "corr")
    xs = np.maximum(rng.standard_normal(n), 0.0)
    return np.ascontiguousarray(A), A @ xs


def range_defect(A, x, y):
    """max |(y - x) - A'w| for the least-squares w, rows of A scaled to unit norm (the same range, a conditioning the solve can carry)"""
    As = A / np.sqrt((A * A).sum(axis=1))[:, None]
    w = np.linalg.lstsq(As.T, y - x, rcond=None)[0]
    return float(np.abs((y - x) - As.T @ w).max())
