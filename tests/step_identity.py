"""
One GAP / DR / AP step checked against its own definition (gap.jl:42-80), from what a handle exposes around the step:

    t1 = a1 sol + (1 - a1) x,    t2 = prox(S2, t1),    x+ = alpha (alpha2 t2 + (1 - alpha2) t1) + (1 - alpha) x

with x the iterate before the step, x+ the iterate after it and sol the affine projection of THIS step (CGdata.xinit behind the
step, or the exact projection under direct = true).  sol is taken as given, so the check does not depend on where CG stopped and
applies to every step of a trajectory.  The cone projection of the reference is the oracle's DualConeProduct.prox (LAPACK eigh).

The bounds are derived, not measured:

  entries of elementwise cones and (tau, kappa)       |x+ - x+_ref| <= 4 eps (|alpha| (|alpha2| + |1 - alpha2|) (|a1| |sol| + |1 - a1| |x|) + |1 - alpha| |x|)
      the same arithmetic on both sides (a relaxation, a clamp, two more relaxations: four roundings per entry at the most, each
      relative to a partial sum that the bracket majorises); only fused multiply-adds may differ.
  entries of PSD cones, in norm                       ||x+ - x+_ref|| <= |alpha alpha2| 5e-13 max(1, ||t1||) + ||the entrywise bound over these entries||
      5e-13 ||input|| is the bar the PSD(64) kernels are held to against LAPACK where they are tested on their own; the projection
      enters x+ with the factor alpha alpha2.
  the affine projection in front of the step (CG)     ||M sol - [x1 + Q'x2; 0]|| <= tol_i (1 + 1e-9) + gamma_k || |M| |sol| + |rhs| ||
      tol_i = max(0.2^sqrt(i), l eps) (affinepluslinear.jl:108-112, i = the call counter before the call); the second term is the
      forward rounding bound of a sparse product with at most k - 2 entries per row in the solver's own precision (gamma_k =
      k u / (1 - k u), u = 2^-53): the solver stops on a residual it formed in double.  The checker forms its residual in
      np.longdouble, so that it adds nothing more.
"""
import math

import numpy as np
import scipy.sparse as sp

import fos_oracle as orc

EPS = 2.220446049250313e-16
PSD_BAR = 5e-13

_EW = ("Free", "Zero", "NonNeg", "NonPos")


def mixed_cones():
    """Every elementwise cone on the primal and on the dual side, between and behind three PSD(64) cones."""
    K1 = [("NonNeg", 5), ("SDP", 2080), ("Zero", 3), ("SDP", 2080), ("NonPos", 70), ("SDP", 2080), ("Free", 2)]
    K2 = [("Free", 6), ("NonNeg", 4), ("NonPos", 3), ("Zero", 1)]
    return K1, K2


def mixed_problem(workloads, seed=11):
    """6320 x 14, density 0.02."""
    rng = np.random.default_rng(seed)
    K1, K2 = mixed_cones()
    m, n = sum(ln for _, ln in K1), sum(ln for _, ln in K2)
    A = sp.random(m, n, density=0.02, format="csc", random_state=rng, data_rvs=rng.standard_normal)
    return workloads.from_complementary_pair("mixed", A, K1, K2, rng)


def one_problem(workloads, seed=12):
    """One PSD(64) cone and three free variables: two matrices, l = 2084 (below the 16 x 256 entries of the fused launch's tail
    workgroups, no multiple of 256)."""
    rng = np.random.default_rng(seed)
    A = sp.random(2080, 3, density=0.02, format="csc", random_state=rng, data_rvs=rng.standard_normal)
    return workloads.from_complementary_pair("one", A, [("SDP", 2080)], [("Free", 3)], rng)


def oracle_model(prob):
    return orc.Model(prob.A, prob.b, prob.c, [(orc.CONE_CODES[k], ln) for k, ln in prob.K1], [(orc.CONE_CODES[k], ln) for k, ln in prob.K2])


class StepDeviation:
    """What check() found: deviations and their bounds (ew_*: arrays over the elementwise entries; the rest scalars)."""

    def __init__(self):
        self.ew_dev = self.ew_bound = None
        self.psd_dev = self.psd_bound = 0.0
        self.affine_res = self.affine_bound = None
        self.tol = None

    @property
    def ew_ok(self):
        return bool(np.all(self.ew_dev <= self.ew_bound))

    @property
    def psd_ok(self):
        return bool(self.psd_dev <= self.psd_bound)

    @property
    def affine_ok(self):
        return self.affine_res is None or bool(self.affine_res <= self.affine_bound)

    @property
    def ok(self):
        return self.ew_ok and self.psd_ok and self.affine_ok

    def ew_worst(self):
        """largest deviation / bound over the elementwise entries (inf where a bound of zero is exceeded)"""
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(self.ew_bound > 0, self.ew_dev / self.ew_bound, np.where(self.ew_dev > 0, np.inf, 0.0))
        return float(r.max()) if r.size else 0.0

    def __str__(self):
        s = "elementwise: worst dev/bound %.3g; PSD: %.3e (bound %.3e)" % (self.ew_worst(), self.psd_dev, self.psd_bound)
        if self.affine_res is not None:
            s += "; affine: %.3e (tol %.3e, bound %.3e)" % (self.affine_res, self.tol, self.affine_bound)
        return s


class StepIdentity:
    """The checker for one problem (A, b, c, K1, K2); cones as (name, length) pairs, elementwise and SDP only."""

    def __init__(self, A, b, c, K1, K2):
        A = sp.csc_matrix(A)
        self.m, self.n = A.shape
        m, n = self.m, self.n
        self.l = l = m + n + 1
        for name, _ in list(K1) + list(K2):
            assert name in _EW or name == "SDP", "step identity: elementwise and SDP cones only (%s)" % name
        assert sum(ln for _, ln in K1) == m and sum(ln for _, ln in K2) == n
        self.K1, self.K2 = list(K1), list(K2)
        self.S2 = orc.DualConeProduct(orc.ConeProduct.from_lengths([(orc.CONE_CODES[k], ln) for k, ln in K1]),
                                      orc.ConeProduct.from_lengths([(orc.CONE_CODES[k], ln) for k, ln in K2]))
        # entries of PSD cones in one half [K2 (n); K1 (m); scalar], then in both halves [x1; x2]
        half = np.zeros(l, dtype=bool)
        self.psd_segments = []                            # (start in the half, length) of every PSD cone
        pos = 0
        for name, ln in list(K2) + list(K1):
            if name == "SDP":
                half[pos:pos + ln] = True
                self.psd_segments.append((pos, ln))
            pos += ln
        self.psd_mask = np.concatenate([half, half])
        self.ew_mask = ~self.psd_mask
        # Q = [0 A' c; -A 0 b; -c' -b' 0] (HSDEAffine.jl:2-20) in CSR, values in long double
        bcol = sp.csc_matrix(np.asarray(b, dtype=np.float64).reshape(-1, 1))
        ccol = sp.csc_matrix(np.asarray(c, dtype=np.float64).reshape(-1, 1))
        Q = sp.bmat([[None, A.T, ccol], [-A, None, bcol], [-ccol.T, -bcol.T, None]], format="csr")
        Q.sum_duplicates()
        Q.sort_indices()
        assert Q.shape == (l, l)
        self._q = (Q.indptr.astype(np.int64), Q.indices.astype(np.int64), Q.data.astype(np.longdouble))
        self.kmax = int(np.diff(Q.indptr).max()) + 1 + 2     # largest row count of M = [I Q'; Q -I] (Q' = -Q: same pattern), + 2

    def _qmul(self, v, absolute=False):
        indptr, indices, data = self._q
        v = np.asarray(v, dtype=np.longdouble)
        prod = (np.abs(data) if absolute else data) * (np.abs(v) if absolute else v)[indices]
        out = np.zeros(self.l, dtype=np.longdouble)
        nz = np.diff(indptr) > 0
        if prod.size:
            out[nz] = np.add.reduceat(prod, indptr[:-1][nz])
        return out

    def reference(self, x, sol, alpha, a1, a2):
        """(t1, t2, x+_ref) -- the expressions of gap.jl:48,58,78 as the oracle writes them."""
        t1 = a1 * sol + (1 - a1) * x
        t2 = np.empty_like(t1)
        self.S2.prox(t2, t1)
        return t1, t2, alpha * (a2 * t2 + (1 - a2) * t1) + (1 - alpha) * x

    def entry_bound(self, x, sol, alpha, a1, a2):
        return 4 * EPS * (abs(alpha) * (abs(a2) + abs(1 - a2)) * (abs(a1) * np.abs(sol) + abs(1 - a1) * np.abs(x)) + abs(1 - alpha) * np.abs(x))

    def psd_bound(self, t1, bound, alpha, a2):
        return abs(alpha * a2) * PSD_BAR * max(1.0, float(np.linalg.norm(t1[self.psd_mask]))) + float(np.linalg.norm(bound[self.psd_mask]))

    def affine_residual(self, x, sol):
        """(||M sol - rhs||, gamma_k || |M| |sol| + |rhs| ||) with M = [I Q'; Q -I], rhs = [x1 + Q'x2; 0] (affinepluslinear.jl:94-95)."""
        l = self.l
        ld = np.longdouble
        s1, s2, x1, x2 = (np.asarray(v, dtype=ld) for v in (sol[:l], sol[l:], x[:l], x[l:]))
        r = np.concatenate([s1 - self._qmul(s2) - (x1 - self._qmul(x2)), self._qmul(s1) - s2])
        mag = np.concatenate([np.abs(s1) + self._qmul(s2, True) + np.abs(x1) + self._qmul(x2, True), self._qmul(s1, True) + np.abs(s2)])
        u = EPS / 2
        gamma = self.kmax * u / (1 - self.kmax * u)
        return float(np.sqrt(np.sum(r * r))), float(gamma * np.sqrt(np.sum(mag * mag)))

    def tolerance(self, i):
        return max(0.2 ** math.sqrt(i), self.l * EPS)

    def check(self, x, sol, xp, alpha, a1, a2, i=None):
        """i: the affine projection's call counter in front of the step (CG), or None (exact projection: no residual check)."""
        t1, _, xref = self.reference(x, sol, alpha, a1, a2)
        bound = self.entry_bound(x, sol, alpha, a1, a2)
        diff = np.abs(xp - xref)
        diff[~np.isfinite(xp)] = np.inf
        out = StepDeviation()
        out.ew_dev, out.ew_bound = diff[self.ew_mask], bound[self.ew_mask]
        out.psd_dev = float(np.linalg.norm(diff[self.psd_mask]))
        out.psd_bound = self.psd_bound(t1, bound, alpha, a2)
        if i is not None:
            out.tol = self.tolerance(i)
            res, allowance = self.affine_residual(x, sol)
            out.affine_res, out.affine_bound = res, out.tol * (1 + 1e-9) + allowance
        return out


def check_step(x, sol, xp, alpha, a1, a2, K1, K2, A, b, c, i=None):
    return StepIdentity(A, b, c, K1, K2).check(x, sol, xp, alpha, a1, a2, i)
