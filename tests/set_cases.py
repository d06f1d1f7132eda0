"""Reference projections of the vector sets of csrc/sets.hip (ProximalOperators' IndBallL2, IndBallL1, IndSimplex, IndHalfspace, IndHyperslab, IndPoint,
IndFree and the scalar IndBox), written as objects with prox(y, x) -- the ProximableFunction protocol, so the same object serves the oracle's Feasibility
and the device's callback path -- and the seeded cases the CPU and GPU tests share.  Sums are math.fsum (exact), the threshold sets are sort based."""
import math

import numpy as np

KINDS = ["IndBallL2", "IndBallL1", "IndSimplex", "IndHalfspace", "IndHyperslab", "IndPoint", "IndFree", "IndBox"]
INPUTS = ["gauss", "gauss1e3", "equal", "onehot", "negative", "ties", "feasible", "center_eq_x", "r0"]
PASS_CAP = 11                                   # ceil(52 / log2(32 + 1)): csrc/sets.hip


class _Ref:
    calls = 0

    def prox(self, y, x):
        self.calls += 1
        y[:] = self.project(np.asarray(x, dtype=np.float64))


class RefBallL2(_Ref):
    def __init__(self, r, center=None):
        self.r, self.c = float(r), None if center is None else np.array(center, dtype=np.float64)

    def project(self, x):
        c = np.zeros_like(x) if self.c is None else self.c
        d = x - c
        nd = math.sqrt(math.fsum(d * d))
        return x.copy() if nd <= self.r else c + d * (self.r / nd)


def _threshold(v, a):
    """tau with sum max(v - tau, 0) = a (a > 0), by sorting: the active set from an extended-precision running sum, tau from the exact sum over it"""
    u = np.sort(v)[::-1]
    css = np.cumsum(u.astype(np.longdouble))
    j = np.arange(1, len(u) + 1)
    rho = int(np.nonzero(u * j > css - a)[0][-1]) + 1
    return (math.fsum(u[:rho]) - a) / rho


class RefBallL1(_Ref):
    def __init__(self, r):
        self.r = float(r)

    def project(self, x):
        ax = np.abs(x)
        if math.fsum(ax) <= self.r:
            return x.copy()
        if self.r == 0.0:
            return np.zeros_like(x)
        return np.sign(x) * np.maximum(ax - _threshold(ax, self.r), 0.0)


class RefSimplex(_Ref):
    def __init__(self, a):
        self.a = float(a)

    def project(self, x):
        return np.maximum(x - _threshold(x, self.a), 0.0)


class RefHyperslab(_Ref):
    def __init__(self, lo, a, hi):
        self.lo, self.a, self.hi = float(lo), np.array(a, dtype=np.float64), float(hi)
        self.aa = math.fsum(self.a * self.a)

    def project(self, x):
        s = math.fsum(self.a * x)
        if s > self.hi:
            return x - ((s - self.hi) / self.aa) * self.a
        if s < self.lo:
            return x - ((s - self.lo) / self.aa) * self.a
        return x.copy()


class RefHalfspace(RefHyperslab):
    def __init__(self, a, b):
        super().__init__(-np.inf, a, b)


class RefPoint(_Ref):
    def __init__(self, p):
        self.p = np.array(p, dtype=np.float64)

    def project(self, x):
        return self.p.copy()


class RefFree(_Ref):
    def project(self, x):
        return x.copy()


class RefBox(_Ref):
    def __init__(self, lo, hi):
        self.lo, self.hi = float(lo), float(hi)

    def project(self, x):
        return np.minimum(np.maximum(x, self.lo), self.hi)


class RefSeparableSum(_Ref):
    def __init__(self, blocks):
        self.blocks = blocks

    def project(self, x):
        y, pos = np.empty_like(x), 0
        for ref, length in self.blocks:
            y[pos:pos + length] = ref.project(x[pos:pos + length])
            pos += length
        return y


class Case:
    """One set on `length` entries: its reference object, the arguments of the package's class, the input and what the tolerance is relative to."""

    def __init__(self, kind, ref, args, x, param):
        self.kind, self.ref, self.args, self.x, self.param = kind, ref, args, x, param

    def device_set(self, pkg):
        return getattr(pkg, self.kind)(*self.args)

    def expected(self):
        return self.ref.project(self.x)

    def tol(self):
        return 1e-13 * max(float(np.abs(self.x).max()), abs(self.param))

    def check(self, y, label=""):
        """within the tolerance; the same bits where the definition says y = x (every set but the always-thresholded simplex) or y = p"""
        ref = self.expected()
        err = float(np.abs(y - ref).max())
        assert err <= self.tol(), (label, self.kind, len(self.x), err, self.tol())
        if self.kind == "IndPoint" or (self.kind != "IndSimplex" and np.array_equal(ref, self.x)):
            assert np.array_equal(y, ref), (label, self.kind, len(self.x), "not bit-identical")
        return err


def make_set(kind, length, rng, variant=0, r0=False):
    """-> (reference object, constructor arguments, |parameter|) of a set whose projection is ACTIVE on a standard normal input"""
    if kind == "IndBallL2":
        c = 0.5 * rng.standard_normal(length)
        r = 0.0 if r0 else 0.5 * math.sqrt(length)
        return RefBallL2(r, c), (r, c), r
    if kind == "IndBallL1":
        r = 0.0 if r0 else 0.3 * length
        return RefBallL1(r), (r,), r
    if kind == "IndSimplex":
        a = [1.0, 1e-3, 50.0, 1e6][variant % 4]
        return RefSimplex(a), (a,), a
    if kind == "IndHalfspace":
        a = rng.standard_normal(length) + (0.0 if length > 1 else 2.0)
        return RefHalfspace(a, 0.3), (a, 0.3), 0.3
    if kind == "IndHyperslab":
        a = rng.standard_normal(length) + (0.0 if length > 1 else 2.0)
        return RefHyperslab(-0.2, a, 0.3), (-0.2, a, 0.3), 0.3
    if kind == "IndPoint":
        p = rng.standard_normal(length)
        return RefPoint(p), (p,), float(np.abs(p).max())
    if kind == "IndFree":
        return RefFree(), (), 0.0
    if kind == "IndBox":
        return RefBox(-0.5, 0.25), (-0.5, 0.25), 0.5
    raise KeyError(kind)


def make_case(kind, length, inp, seed=0):
    rng = np.random.default_rng([seed, KINDS.index(kind), length, INPUTS.index(inp)])
    ref, args, param = make_set(kind, length, rng, variant=INPUTS.index(inp) + length, r0=(inp == "r0"))
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
    elif inp == "feasible":                                     # a point of the set
        if kind == "IndBallL2":
            x = ref.c + g * (0.5 * ref.r / np.linalg.norm(g))
        elif kind == "IndBallL1":
            x = g * (0.5 * ref.r / np.abs(g).sum())
        elif kind == "IndSimplex":
            x = np.abs(g) * (ref.a / np.abs(g).sum())
        elif kind in ("IndHalfspace", "IndHyperslab"):
            x = ref.a * (0.1 / ref.aa)                           # <a, x> = 0.1: inside both
        elif kind == "IndPoint":
            x = ref.p.copy()
        elif kind == "IndBox":
            x = np.clip(0.2 * g, -0.5, 0.25)
        else:
            x = g
    elif inp == "center_eq_x" and kind == "IndBallL2":
        x = ref.c.copy()
    else:                                                       # gauss; the centre / radius inputs of a set that has neither
        x = g
    return Case(kind, ref, args, np.ascontiguousarray(x), param)


def random_separable_sum(pkg, nblocks=300, max_len=3000, seed=5):
    """~nblocks blocks of seeded random kinds and lengths 1..max_len; the first and the last are IndFree, and IndFree blocks are scattered between.
    -> (device SeparableSum, reference object, n, [(kind, start, length, |parameter|)])"""
    rng = np.random.default_rng(seed)
    dev, ref, layout, pos = [], [], [], 0
    for i in range(nblocks):
        free = i == 0 or i == nblocks - 1 or rng.random() < 0.15
        kind = "IndFree" if free else KINDS[int(rng.integers(len(KINDS)))]
        length = int(rng.integers(1, max_len + 1)) if rng.random() < 0.5 else int(rng.integers(1, 130))
        r, args, param = make_set(kind, length, rng, variant=i)
        dev.append((getattr(pkg, kind)(*args), length))
        ref.append((r, length))
        layout.append((kind, pos, length, param))
        pos += length
    return pkg.SeparableSum(dev), RefSeparableSum(ref), pos, layout
