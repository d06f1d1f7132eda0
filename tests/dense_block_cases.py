"""Instances, references and calls of the dense blocks of a SeparableSum (csrc/dense_blocks.hip): Quadratic(Q, q), IndAffine(A, b) and LeastSquares(A, b, lam)
on a block of p <= 1024 entries, whose prox is one formula y = G x + d.  Seeded; shared by the CPU emulation tests and the GPU tests.  The instances are those of
nspace_cases (gauss, corr, rankdef; never `cols`) and affine_factored_cases (gauss); the references are RefQuadratic, RefLeastSquares and, for IndAffine, a
projection whose residuals are evaluated in np.longdouble.

The bars are the project's own: nspace_cases.bar(M, x, y_ref) for the two functions, affine_factored_cases.TOL max(1, |x|_inf) for IndAffine.
The kernel bound: with the G and d the device holds and y_L = G x + d evaluated in np.longdouble, |y - y_L| <= (p + 1) 2^-53 (|G||x| + |d|) elementwise -- the
textbook bound of a dot product of length p plus one addition, in any order of additions, with or without fused multiply-adds."""
import ctypes as C
import functools

import numpy as np
import scipy.linalg

import affine_factored_cases as ac
import nspace_cases as nc
from prox_fn_cases import RefLeastSquares

P = [1, 2, 7, 8, 9, 16, 17, 32, 33, 63, 64, 65, 128, 255, 256, 257, 1023, 1024]
WAVE_MAX, ORDER_MAX = 64, 1024
KINDS = ("Quadratic", "IndAffine", "LeastSquares")
LAMS = nc.LAMS
FOS_EINVAL = -1
U = 2.0 ** -53


def affine_rows(p):
    return sorted({1, max(1, p // 2), p})


class RefAffine:
    """{x : A x = b}: y = x - As'w with (As As') w = As x - bs, rows scaled to unit norm; w from an fp64 factorisation followed by refinement steps whose residuals
    are evaluated in np.longdouble from A itself (the pattern of RefLeastSquares).  m = p: the unique solution of A y = b, refined the same way."""

    def __init__(self, A, b):
        L = np.longdouble
        s = 1.0 / np.sqrt((A * A).sum(axis=1))
        self.As, self.bs = A * s[:, None], b * s
        self.AL, self.bL = self.As.astype(L), self.bs.astype(L)
        self.square = A.shape[0] == A.shape[1]
        self.fact = scipy.linalg.lu_factor(self.As) if self.square else scipy.linalg.cho_factor(self.As @ self.As.T)

    def project(self, x):
        L = np.longdouble
        if self.square:
            y = scipy.linalg.lu_solve(self.fact, self.bs).astype(L)
            for _ in range(3):
                y = y + scipy.linalg.lu_solve(self.fact, (self.bL - self.AL @ y).astype(np.float64)).astype(L)
            return y.astype(np.float64)
        xL = x.astype(L)
        r = self.AL @ xL - self.bL
        w = scipy.linalg.cho_solve(self.fact, r.astype(np.float64)).astype(L)
        for _ in range(3):
            w = w + scipy.linalg.cho_solve(self.fact, (r - self.AL @ (self.AL.T @ w)).astype(np.float64)).astype(L)
        return (xL - self.AL.T @ w).astype(np.float64)

    def prox(self, y, x):
        y[:] = self.project(np.asarray(x, dtype=np.float64))


class Block:
    """One dense block: the matrix and vector the library takes, the package's object, the reference and the bar at an input"""

    def __init__(self, kind, M, v, lam, ref, Mn):
        self.kind, self.M, self.v, self.lam, self.ref, self.Mn = kind, np.ascontiguousarray(M), np.ascontiguousarray(v), float(lam), ref, Mn
        self.p = self.M.shape[1]

    def code(self, pkg):
        return pkg.lib.BLK_CODES[self.kind]

    def device_set(self, pkg, v=None):
        v = self.v if v is None else v
        if self.kind == "Quadratic":
            return pkg.Quadratic(self.M, v)
        if self.kind == "IndAffine":
            return pkg.IndAffine(self.M, v)
        return pkg.LeastSquares(self.M, v, self.lam)

    def bar(self, x, yref):
        if self.kind == "IndAffine":
            return ac.TOL * max(1.0, float(np.abs(x).max()))
        return nc.bar(self.Mn, x, yref)


@functools.lru_cache(maxsize=None)
def block(kind, p, family="gauss", lam=1.0, m=None):
    """the block of `kind` and order p: Quadratic / LeastSquares on nspace_cases.instance(family, m, p) (m defaults to p + 3: I + lam A'A has full rank), IndAffine on
    affine_factored_cases.instance('gauss', m, p)"""
    if kind == "IndAffine":
        A, b = ac.instance("gauss", p if m is None else m, p)
        return Block(kind, A, b, 0.0, RefAffine(A, b), None)
    A, b = nc.instance(family, p + 3 if m is None else m, p)
    Mn = np.eye(p) + lam * (A.T @ A)
    if kind == "LeastSquares":
        return Block(kind, A, b, lam, RefLeastSquares(A, b, lam), Mn)
    Q, q = nc.quadratic_of(A, b, lam)
    return Block(kind, Q, q, 0.0, nc.RefQuadratic(Q, q), np.eye(p) + Q)


def blocks_of(kind, p):
    """the instances the CPU test holds at order p: gauss with the three lambdas; corr and rankdef at p = 64 and 65; IndAffine with m = 1, p // 2, p"""
    if kind == "IndAffine":
        return [("m=%d" % m, block(kind, p, m=m)) for m in affine_rows(p)]
    out = [("gauss lam=%g" % lam, block(kind, p, "gauss", lam)) for lam in LAMS]
    if p in (64, 65):
        out += [("%s lam=1" % fam, block(kind, p, fam, 1.0, 2 * p)) for fam in ("corr", "rankdef")]
    return out


def input_of(p, seed=0):
    return np.random.default_rng([p, seed]).standard_normal(p)


def host(pkg, code, M, v, lam, x, m=None, p=None):
    """fos_host_dense_block -> (return code, y, G, d); m, p override the shape of M (refusals)"""
    M = np.ascontiguousarray(M, dtype=np.float64)
    m = M.shape[0] if m is None else m
    p = M.shape[1] if p is None else p
    x = np.ascontiguousarray(x, dtype=np.float64)
    v = None if v is None else np.ascontiguousarray(v, dtype=np.float64)
    y, G, d = np.full(p, np.nan), np.full((p, p), np.nan), np.full(p, np.nan)
    dp = pkg.lib.dptr
    rc = pkg.lib.load().fos_host_dense_block(code, m, p, dp(M), None if v is None else dp(v), lam, dp(x), dp(y), dp(G), dp(d))
    return rc, y, G, d


def host_block(pkg, blk, x):
    return host(pkg, blk.code(pkg), blk.M, blk.v, blk.lam, x)


def last_error(pkg):
    return pkg.lib.load().fos_last_error().decode()


def kernel_bound(G, d, x):
    """-> (y_L = G x + d in np.longdouble, the elementwise bound (p + 1) 2^-53 (|G||x| + |d|))"""
    L = np.longdouble
    yL = G.astype(L) @ x.astype(L) + d.astype(L)
    return yL, (G.shape[0] + 1) * U * (np.abs(G) @ np.abs(x) + np.abs(d))


def set_blocks2_raw(pkg, d, which, kinds, lens, scal, vec, mats, rows, cols, block_mat, block_vec):
    """fos_feas_set_blocks2 with raw arrays and explicit shapes -> return code (refusals: nothing is validated on the Python side)"""
    lib, dp = pkg.lib.load(), pkg.lib.dptr
    dpp = C.POINTER(C.c_double)
    kinds, lens = np.ascontiguousarray(kinds, dtype=np.int32), np.ascontiguousarray(lens, dtype=np.int64)
    scal = np.ascontiguousarray(scal, dtype=np.float64)
    mats = [np.ascontiguousarray(M, dtype=np.float64) for M in mats]
    vecs = [None if v is None else np.ascontiguousarray(v, dtype=np.float64) for v in block_vec]
    rows, cols = np.ascontiguousarray(rows, dtype=np.int64), np.ascontiguousarray(cols, dtype=np.int64)
    block_mat = np.ascontiguousarray(block_mat, dtype=np.int64)
    mp = (dpp * max(len(mats), 1))(*[dp(M) for M in mats])
    vp = (dpp * max(len(vecs), 1))(*[C.cast(None, dpp) if v is None else dp(v) for v in vecs])
    i64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
    return lib.fos_feas_set_blocks2(d._h, which, len(kinds), kinds.ctypes.data_as(C.POINTER(C.c_int32)), i64(lens), dp(scal), None if vec is None else dp(vec),
                                    len(mats), i64(rows), i64(cols), mp, i64(block_mat), vp)
