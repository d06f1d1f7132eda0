"""
Extended-precision restatement of conjugategradient! (conjugategradients.jl:31-55) over the KKT operator M = [I Q'; Q -I]
(affinepluslinear.jl:37-52) of Q = [0 A' c; -A 0 b; -c' -b' 0] (HSDEAffine.jl:41-65), with MEASURED fp64 error allowances.

Written from the formulas of the reference, not from the oracle's classes: every product and sum of recurrence(.., dtype=np.longdouble)
is accumulated in x87 extended precision (64-bit mantissa, unit roundoff 2^-64) straight from the COO triplets of A with np.add.at;
nothing is densified.  In exact arithmetic the merged (Chronopoulos-Gear) recurrence has the same iterates, so iterates() serves every
CG variant of the library.

The allowance is not derived: first-order worst-case bounds propagated through the recurrence give 1e-11, 1e-9, 1e-5 x max|x| after one,
two, three iterations, looser than a norm-wise comparison.  It is measured from fp64 evaluations of the reference alone -- no device
result enters.  allowance(case, k) is FOUR times the largest elementwise distance from the extended iterate x_k over
    the oracle's conjugategradient,
    the oracle's conjugategradient_merged,
    recurrence(.., dtype=np.float64, sequential=True): products by fp64 np.add.at, dots added strictly left to right -- the least
    favourable legitimate order,
with a floor of 4 u max|x_k|.  The factor 4 is the margin for summation orders and fused multiply-adds that none of the three has; the
device's orders are fixed trees of per-lane and per-workgroup partial sums, between pairwise and sequential.  It is one number per case
and k, applied to every element, the tau element l - 1 and its twin N - 1 included.

decisive_tol(case, k) is a tolerance at which the stop rule ||r|| <= tol (conjugategradients.jl:42) ends the recurrence at iteration k
whatever the rounding: sqrt(||r_{k-1}|| ||r_k||), where the extended residuals satisfy ||r_{k-1}|| >= 3 ||r_k|| and ||r_j|| > ||r_{k-1}||
for every j < k - 1 (None otherwise).
"""
import warnings
from types import SimpleNamespace

import numpy as np
import scipy.sparse as sp

import fos_oracle as orc

LD = np.longdouble
U = 2.0 ** -53                      # unit roundoff of fp64
MARGIN = 4.0


def _require_extended():
    eps = float(np.finfo(LD).eps)
    assert eps <= 1.1e-19, "np.longdouble is not an extended type here (eps = %g): this reference would be no better than fp64" % eps


class Case:
    """one CG start: operator (A, b, c), warm start x0 and right-hand side rhs of length N = 2 (n + m + 1), the iteration numbers ks"""

    def __init__(self, name, A, b, c, x0, rhs, ks):
        self.name, self.A = name, sp.csc_matrix(A)
        self.b, self.c = np.asarray(b, dtype=np.float64), np.asarray(c, dtype=np.float64)
        self.x0, self.rhs, self.ks = np.asarray(x0), np.asarray(rhs), tuple(ks)
        self.coo, self._memo = Coo(self.A), {}


class Coo:
    """the stored non-zero entries (i, j, a) of A, column by column, converted once per number format"""

    def __init__(self, A):
        A = sp.coo_matrix(sp.csc_matrix(A))
        keep = A.data != 0                              # explicit zeros are not entries of the operator
        self.shape, self.i, self.j, self._a, self._as = A.shape, A.row[keep], A.col[keep], A.data[keep], {}

    def triplets(self, dtype):
        if dtype not in self._as:
            self._as[dtype] = self._a.astype(dtype)
        return self.i, self.j, self._as[dtype]


def coo(A):
    return A if isinstance(A, Coo) else Coo(A)


def _dot(a, b, sequential):
    if a.size == 0:
        return a.dtype.type(0)
    return np.cumsum(a * b)[-1] if sequential else np.sum(a * b)        # (cumsum adds left to right; sum is pairwise)


def q_mul(A, b, c, u, dtype, sequential=False, drop=None):
    """Q u (HSDEAffine.jl:41-59) in `dtype`.  drop: index of one stored entry left out of the product A x (a deliberately wrong sweep)"""
    A = coo(A)
    m, n = A.shape
    i, j, a = A.triplets(dtype)
    b, c, u = np.asarray(b, dtype=dtype), np.asarray(c, dtype=dtype), np.asarray(u, dtype=dtype)
    x, y, t = u[0:n], u[n:n + m], u[n + m]
    ATy, Ax = np.zeros(n, dtype), np.zeros(m, dtype)
    np.add.at(ATy, j, a * y[i])                                          # :51
    if drop is None:
        np.add.at(Ax, i, a * x[j])                                       # :52
    else:
        keep = np.arange(a.size) != drop
        np.add.at(Ax, i[keep], a[keep] * x[j[keep]])
    last = -_dot(c, x, sequential) - _dot(b, y, sequential)              # :57
    return np.concatenate([ATy + t * c, -(Ax - t * b), [last]])          # :54-56


def kkt_mul(A, b, c, v, dtype, sequential=False, drop=None):
    """M v = [v1 + Q'v2; Q v1 - v2] with Q' = -Q (affinepluslinear.jl:45-48, HSDEAffine.jl:61-65)"""
    A = coo(A)
    l = sum(A.shape) + 1
    v = np.asarray(v, dtype=dtype)
    v1, v2 = v[:l], v[l:]
    return np.concatenate([-q_mul(A, b, c, v2, dtype, sequential) + v1, q_mul(A, b, c, v1, dtype, sequential, drop) - v2])


def recurrence(A, b, c, x0, rhs, k, dtype=LD, sequential=False, alpha_scale=None, drop=None):
    """k iterations of conjugategradients.jl:32-51 in `dtype`: xs[j - 1] = x_j, rn[j] = ||r_j|| of the recursively updated residual
    (j = 0 .. k), alphas[j - 1] the step length of iteration j, r0.  alpha_scale multiplies the first step length and drop leaves one
    stored entry out of every sweep M p: the two deliberate errors of the detection test.  sequential = "mixed": r.r pairwise, Ap.p left to
    right -- two sums of the same terms then differ in their last bits, as sums taken by different kernels do."""
    seq_rr, seq_pap = (False, True) if sequential == "mixed" else (sequential, sequential)
    sequential = bool(sequential)
    if dtype is LD:
        _require_extended()
    x = np.array(x0, dtype=dtype)
    rhs = np.asarray(rhs, dtype=dtype)
    r = rhs - kkt_mul(A, b, c, x, dtype, sequential)                     # :32-33
    r0 = r.copy()
    p = r.copy()                                                         # :34
    rn = _dot(r, r, seq_rr)                                              # :35
    out = SimpleNamespace(xs=[], rn=[np.sqrt(rn)], alphas=[], r0=r0)
    with np.errstate(divide="ignore", invalid="ignore"):                 # Julia: x / 0.0 -> Inf / NaN silently
        for it in range(1, k + 1):
            Ap = kkt_mul(A, b, c, p, dtype, sequential, drop)            # :38
            alpha = rn / _dot(Ap, p, seq_pap)                            # :39
            if it == 1 and alpha_scale is not None:
                alpha = alpha * dtype(alpha_scale)
            x = x + alpha * p                                            # :40
            r = r - alpha * Ap                                           # :41
            rnold, rn = rn, _dot(r, r, seq_rr)                           # :45-46
            out.xs.append(x.copy())
            out.rn.append(np.sqrt(rn))
            out.alphas.append(alpha)
            p = p * (rn / rnold) + r                                     # :47-50
    return out


def iterates(A, b, c, x0, rhs, k):
    """(x_1 .. x_k, ||r_0|| .. ||r_k||) of conjugategradient! in extended precision; the residual norms of the issue's r_1 .. r_k are rn[1:]"""
    rec = recurrence(A, b, c, x0, rhs, k, LD)
    return rec.xs, rec.rn


def _oracle(fn, case, k):
    M = orc.KKTMatrix(orc.HSDEMatrixQ(case.A, case.b, case.c))
    N = case.x0.shape[0]
    x = np.array(case.x0, dtype=np.float64)
    nb = 4 if fn is orc.conjugategradient_merged else 3
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        it = fn(x, M, np.asarray(case.rhs, dtype=np.float64), *[np.empty(N) for _ in range(nb)], tol=1e-300, max_iters=k)
    assert it == k
    return x


def extended(case):
    """the extended-precision recurrence of a case through max(case.ks) iterations, computed once"""
    if "ext" not in case._memo:
        case._memo["ext"] = recurrence(case.coo, case.b, case.c, case.x0, case.rhs, max(case.ks), LD)
    return case._memo["ext"]


def fp64_evaluations(case, k):
    """{name: x_k} of the three fp64 evaluations the allowance is measured from"""
    key = ("fp64", k)
    if key not in case._memo:
        if "seq" not in case._memo:
            case._memo["seq"] = recurrence(case.coo, case.b, case.c, case.x0, case.rhs, max(case.ks), np.float64, sequential=True)
        case._memo[key] = {"oracle": _oracle(orc.conjugategradient, case, k), "oracle merged": _oracle(orc.conjugategradient_merged, case, k),
                           "sequential": case._memo["seq"].xs[k - 1]}
    return case._memo[key]


def distance(x, xk):
    """largest elementwise |x - x_k| against the extended iterate, as a float (inf where x is not finite)"""
    d = np.abs(np.asarray(x, dtype=LD) - xk)
    return float(np.max(d)) if np.all(np.isfinite(d)) else np.inf


def allowance(case, k):
    """MARGIN x the largest elementwise distance of the three fp64 evaluations from the extended x_k, at least MARGIN u max|x_k|"""
    key = ("allow", k)
    if key not in case._memo:
        xk = extended(case).xs[k - 1]
        worst = max(distance(x, xk) for x in fp64_evaluations(case, k).values())
        case._memo[key] = MARGIN * max(worst, U * float(np.max(np.abs(xk))))
    return case._memo[key]


def relative_allowance(case, k):
    """allowance(case, k) / max|x_k|"""
    return allowance(case, k) / float(np.max(np.abs(extended(case).xs[k - 1])))


def decisive_tol(case, k):
    """sqrt(||r_{k-1}|| ||r_k||) where the stop rule cannot end the recurrence anywhere but at iteration k, else None"""
    rn = extended(case).rn
    if not (1 <= k < len(rn)) or not np.all(np.isfinite(np.asarray(rn[:k + 1], dtype=np.float64))):
        return None
    if not (rn[k - 1] >= 3 * rn[k] and rn[k] > 0 and all(rn[j] > rn[k - 1] for j in range(k - 1))):
        return None
    return float(np.sqrt(rn[k - 1] * rn[k]))


def ratio(x, case, k):
    """largest elementwise |x - x_k| / allowance(case, k)"""
    return distance(x, extended(case).xs[k - 1]) / allowance(case, k)
