"""Reference proxes (step 1) of the proximable functions of csrc/sets.hip that are not indicators -- NormL1, SqrNormL2, ElasticNet, Linear, NormL2, HuberLoss,
NormLinf -- and of LeastSquares (csrc/affine_dense.hip), written from their definitions as objects with prox(y, x) (the ProximableFunction protocol: the
same object serves the oracle's Feasibility and the device's callback path) and value(x) = f(x), and the seeded cases the CPU and GPU tests share.
Norms are math.fsum (exact), NormLinf's threshold is the sort-based one of set_cases.py, LeastSquares is the dense solve of (I + lam A'A) y = x + lam A'b."""
import math

import numpy as np
import scipy.linalg

from set_cases import KINDS as SET_KINDS
from set_cases import RefSeparableSum, _Ref, _threshold, make_set

KINDS = ["NormL1", "SqrNormL2", "ElasticNet", "Linear", "NormL2", "HuberLoss", "NormLinf"]
INPUTS = ["gauss", "gauss1e3", "equal", "onehot", "negative", "ties", "inactive", "lam0"]
ELEMENTWISE, REDUCTION, THRESHOLD = ("NormL1", "SqrNormL2", "ElasticNet", "Linear"), ("NormL2", "HuberLoss"), ("NormLinf",)
PASS_CAP = 11


def _norm2(x):
    return math.sqrt(math.fsum(x * x))


def _soft(x, t):
    return np.sign(x) * np.maximum(np.abs(x) - t, 0.0)


class RefNormL1(_Ref):
    def __init__(self, lam):
        self.lam = float(lam)

    def project(self, x):
        return x.copy() if self.lam == 0.0 else _soft(x, self.lam)

    def value(self, x):
        return self.lam * math.fsum(np.abs(x))


class RefSqrNormL2(_Ref):
    def __init__(self, lam):
        self.lam = float(lam)

    def project(self, x):
        return x / (1.0 + self.lam)

    def value(self, x):
        return 0.5 * self.lam * math.fsum(x * x)


class RefElasticNet(_Ref):
    def __init__(self, mu, lam):
        self.mu, self.lam = float(mu), float(lam)

    def project(self, x):
        return _soft(x, self.mu) / (1.0 + self.lam)

    def value(self, x):
        return self.mu * math.fsum(np.abs(x)) + 0.5 * self.lam * math.fsum(x * x)


class RefLinear(_Ref):
    def __init__(self, c):
        self.c = np.array(c, dtype=np.float64)

    def project(self, x):
        return x - self.c

    def value(self, x):
        return math.fsum(self.c * x)


class RefNormL2(_Ref):
    def __init__(self, lam):
        self.lam = float(lam)

    def project(self, x):
        nx = _norm2(x)
        if self.lam == 0.0:
            return x.copy()
        if nx <= self.lam:
            return np.zeros_like(x)
        return (1.0 - self.lam / nx) * x

    def value(self, x):
        return self.lam * _norm2(x)


class RefHuberLoss(_Ref):
    def __init__(self, rho, mu):
        self.rho, self.mu = float(rho), float(mu)

    def project(self, x):
        nx = _norm2(x)
        if nx <= self.rho * (1.0 + self.mu):
            return x / (1.0 + self.mu)
        return (1.0 - self.rho * self.mu / nx) * x

    def value(self, x):
        nx = _norm2(x)
        return 0.5 * self.mu * nx * nx if nx <= self.rho else self.rho * self.mu * (nx - 0.5 * self.rho)


class RefNormLinf(_Ref):
    def __init__(self, lam):
        self.lam = float(lam)

    def project(self, x):
        ax = np.abs(x)
        if self.lam == 0.0:
            return x.copy()
        if math.fsum(ax) <= self.lam:
            return np.zeros_like(x)
        return np.sign(x) * np.minimum(ax, _threshold(ax, self.lam))

    def value(self, x):
        return self.lam * float(np.abs(x).max())


class RefLeastSquares(_Ref):
    """f(x) = lam/2 |A x - b|^2: the dense solve of (I + lam A'A) y = x + lam A'b (Cholesky), followed by two refinement steps whose residual is evaluated from A
    itself in extended precision -- cond(I + lam A'A) reaches 1e13 on the `scaled` family at lam = 1e3, where the plain solve alone is only good to ~1e-4."""

    def __init__(self, A, b, lam):
        self.A, self.b, self.lam = np.array(A, dtype=np.float64), np.array(b, dtype=np.float64), float(lam)
        n = self.A.shape[1]
        self.chol = scipy.linalg.cho_factor(np.eye(n) + self.lam * (self.A.T @ self.A))
        L = np.longdouble
        self.AL, self.bL = self.A.astype(L), self.b.astype(L)

    def project(self, x):
        L = np.longdouble
        lam, xL = L(self.lam), x.astype(L)
        y = scipy.linalg.cho_solve(self.chol, x + self.lam * (self.A.T @ self.b)).astype(L)
        for _ in range(2):
            res = xL - y - lam * (self.AL.T @ (self.AL @ y - self.bL))
            y = y + scipy.linalg.cho_solve(self.chol, res.astype(np.float64)).astype(L)
        return y.astype(np.float64)

    def value(self, x):
        r = self.A @ x - self.b
        return 0.5 * self.lam * math.fsum(r * r)


REFS = {"NormL1": RefNormL1, "SqrNormL2": RefSqrNormL2, "ElasticNet": RefElasticNet, "Linear": RefLinear, "NormL2": RefNormL2, "HuberLoss": RefHuberLoss,
        "NormLinf": RefNormLinf}


class Case:
    """One function on `length` entries: its reference object, the arguments of the package's class, the input and what the tolerance is relative to."""

    def __init__(self, kind, ref, args, x, param):
        self.kind, self.ref, self.args, self.x, self.param = kind, ref, args, x, param

    def device_set(self, pkg):
        return getattr(pkg, self.kind)(*self.args)

    def expected(self):
        return self.ref.project(self.x)

    def tol(self):
        return 1e-13 * max(float(np.abs(self.x).max()), abs(self.param))

    def check(self, y, label=""):
        """within the tolerance; the same bits where the definition says y = x, exact zeros where it says y = 0"""
        ref = self.expected()
        err = float(np.abs(y - ref).max())
        assert err <= self.tol(), (label, self.kind, len(self.x), err, self.tol())
        if np.array_equal(ref, self.x):
            assert y.tobytes() == self.x.tobytes(), (label, self.kind, len(self.x), "not bit-identical to x")
        if not ref.any():
            assert not y.any(), (label, self.kind, len(self.x), "not exact zeros")
        return err


def make_fn(kind, length, rng, lam0=False):
    """-> (reference object, constructor arguments, |parameter|) of a function whose prox is ACTIVE (past every threshold) on a standard normal input;
    lam0: the parameters at which the definition gives y = x"""
    if kind == "NormL1":
        args = (0.0 if lam0 else 0.4,)
    elif kind == "SqrNormL2":
        args = (0.0 if lam0 else 0.7,)
    elif kind == "ElasticNet":
        args = (0.0, 0.0) if lam0 else (0.3, 0.6)
    elif kind == "Linear":
        args = (np.zeros(length) if lam0 else rng.standard_normal(length),)
    elif kind == "NormL2":
        args = (0.0 if lam0 else 0.5 * math.sqrt(length),)
    elif kind == "HuberLoss":
        args = (0.3 * math.sqrt(length), 0.0 if lam0 else 0.8)               # the branches meet at |x| = 0.54 sqrt(length)
    elif kind == "NormLinf":
        args = (0.0 if lam0 else 0.3 * length,)
    else:
        raise KeyError(kind)
    param = float(np.abs(args[0]).max()) if kind == "Linear" else max(abs(a) for a in args)
    return REFS[kind](*args), args, param


def make_case(kind, length, inp, seed=0):
    rng = np.random.default_rng([seed, 100 + KINDS.index(kind), length, INPUTS.index(inp)])
    ref, args, param = make_fn(kind, length, rng, lam0=(inp == "lam0"))
    g = rng.standard_normal(length)
    if inp == "gauss1e3":
        x = 1e3 * g
    elif inp == "equal":
        x = np.full(length, 0.37)
    elif inp == "onehot":
        x = np.zeros(length)
        x[length // 3] = 5.0
    elif inp == "negative":
        x = -np.abs(g) - 0.01
    elif inp == "ties":
        x = np.round(g, 1)
    elif inp == "inactive":                                     # below every threshold: y = 0, or the pure-quadratic branch of HuberLoss
        if kind == "NormL1":
            x = g * (0.5 * ref.lam / np.abs(g).max())
        elif kind == "ElasticNet":
            x = g * (0.5 * ref.mu / np.abs(g).max())
        elif kind == "NormL2":
            x = g * (0.5 * ref.lam / np.linalg.norm(g))
        elif kind == "HuberLoss":
            x = g * (0.5 * ref.rho * (1.0 + ref.mu) / np.linalg.norm(g))
        elif kind == "NormLinf":
            x = g * (0.5 * ref.lam / np.abs(g).sum())
        else:                                                   # SqrNormL2, Linear: no threshold
            x = 1e-3 * g
    else:                                                       # gauss, lam0
        x = g
    return Case(kind, ref, args, np.ascontiguousarray(x), param)


def random_mixed_sum(pkg, nblocks=300, max_len=3000, seed=6):
    """~nblocks blocks of seeded random kinds -- the 8 set kinds of set_cases.py and the 7 function kinds -- and lengths 1..max_len; the first and the last are
    IndFree, and IndFree blocks are scattered between.  -> (device SeparableSum, reference object, n, [(kind, start, length, |parameter|)])"""
    rng = np.random.default_rng(seed)
    allk = SET_KINDS + KINDS
    dev, ref, layout, pos = [], [], [], 0
    for i in range(nblocks):
        free = i == 0 or i == nblocks - 1 or rng.random() < 0.1
        kind = "IndFree" if free else allk[int(rng.integers(len(allk)))]
        length = int(rng.integers(1, max_len + 1)) if rng.random() < 0.5 else int(rng.integers(1, 130))
        r, args, param = make_fn(kind, length, rng) if kind in KINDS else make_set(kind, length, rng, variant=i)
        dev.append((getattr(pkg, kind)(*args), length))
        ref.append((r, length))
        layout.append((kind, pos, length, param))
        pos += length
    return pkg.SeparableSum(dev), RefSeparableSum(ref), pos, layout


def lasso_kkt(A, b, lam, mu, x, support=1e-6):
    """the residual of 0 in lam A'(A x - b) + mu d|x|_1: |g + mu sign(x)| on the support, max(|g| - mu, 0) off it.  The support is |x| > 1e-6, the accuracy the
    residual is asked for: x = prox_S1(z) of a DR fixed point found to eps = 1e-9 carries entries of that size where the minimiser has exact zeros."""
    g = lam * (A.T @ (A @ x - b))
    on = np.abs(x) > support
    return float(max(np.abs(g[on] + mu * np.sign(x[on])).max(initial=0.0), np.maximum(np.abs(g[~on]) - mu, 0.0).max(initial=0.0)))
