"""
Extended-precision restatement of checkstatus (HSDEStatus.jl:33-38, 53-63) with worst-case fp64 error allowances.

Written from the formulas of the reference, not from oracle.residuals: every product and sum is accumulated in np.longdouble (x87
extended, 64-bit mantissa: unit roundoff 2^-64, 2048 times below fp64's u = 2^-53), straight from the COO triplets of A with np.add.at, so
nothing is densified.  Against this reference an fp64 evaluation -- the oracle's numpy one or the device's -- can be judged on its own:
each returned value comes with an ALLOWANCE, the first-order worst-case rounding error of ANY fp64 evaluation of the same formula, whatever
its summation order, with or without fused multiply-adds.  The allowances are derived from the data, not measured:

  dual residual, row i of A' (k_i stored entries), evaluated as (A'y)_i / tau + c_i - r_i / tau:
      a k_i-term dot product errs by at most k_i u (|A|'|y|)_i; the division by tau, the two additions and the division of r_i add one u
      each on the partial results, all bounded by (|A|'|y|)_i / |tau| + |c_i| + |r_i| / |tau|:
          E_d,i = u [ (k_i + 3) (|A|'|y|)_i / |tau| + 3 |c_i| + 3 |r_i| / |tau| ]
  primal residual, row j of A, evaluated as (A x)_j / tau + s_j / tau - b_j: the analogue
          E_p,j = u [ (k_j + 3) (|A||x|)_j / |tau| + 3 |s_j| / |tau| + 3 |b_j| ]
  ||A x + s|| and ||A'y||: the same rows without the division by tau.
  a norm of l' <= l = n + m + 1 such rows:  | ||v~|| - ||v|| | <= ||E||_2 for the rows, plus the relative error of the sum of squares
      ((l' + 1) u, halved by the root), the root, the fp64 norm of b or c in the denominator ((l'/2 + 1) u), the 1 + and the division:
      below (l + 8) u relative.  Allowance  ||E||_2 + (l + 8) u ||v||.
  c'x, b'y:  (l + 8) u sum |c_i x_i|,  (l + 8) u sum |b_j y_j|   (dot products of at most l terms).
  g = |a + b| / (1 + |a| + |b|), a = c'x / tau, b = b'y / tau: with E_a = (E_ctx + u |c'x|) / |tau| and E_b alike, numerator and denominator
      each err by at most E_a + E_b; by the quotient rule  E_g = (E_a + E_b) (1 + g) / (1 + |a| + |b|) + 4 u g  (four more roundings).
  tau, kappa: copied, allowance 0.

decide() is the decision of HSDEStatus.jl:53-63 with Julia's silent division by zero; margin() the smallest relative distance of a
compared quantity from its threshold, relative_allowance() the largest relative allowance of such a comparison.
"""
import numpy as np
import scipy.sparse as sp

LD = np.longdouble
U = 2.0 ** -53                      # unit roundoff of fp64
FIELDS = ("p", "d", "g", "ctx", "bty", "nAxs", "nATy", "nb", "nc", "tau", "kappa")


def _require_extended():
    eps = float(np.finfo(LD).eps)
    assert eps <= 1.1e-19, "np.longdouble is not an extended type here (eps = %g): this reference would be no better than fp64" % eps


def _norm(v):
    return np.sqrt(np.sum(v * v)) if v.size else LD(0)


def coo_products(A, x, y):
    """(A x, A'y, |A||x|, |A|'|y|, entries per row of A, entries per column of A) in longdouble, from the COO triplets."""
    _require_extended()
    A = sp.coo_matrix(A)
    m, n = A.shape
    i, j, a = A.row, A.col, A.data.astype(LD)
    keep = a != 0                                       # explicit zeros are not entries of the operator
    i, j, a = i[keep], j[keep], a[keep]
    x, y = np.asarray(x, dtype=LD), np.asarray(y, dtype=LD)
    Ax, ATy, aAx, aATy = np.zeros(m, LD), np.zeros(n, LD), np.zeros(m, LD), np.zeros(n, LD)
    np.add.at(Ax, i, a * x[j])
    np.add.at(aAx, i, np.abs(a * x[j]))
    np.add.at(ATy, j, a * y[i])
    np.add.at(aATy, j, np.abs(a * y[i]))
    krow = np.bincount(i, minlength=m).astype(LD)
    kcol = np.bincount(j, minlength=n).astype(LD)
    return Ax, ATy, aAx, aATy, krow, kcol


def reference(A, b, c, z):
    """-> (values, allowances): two dicts over FIELDS, longdouble values and fp64 error allowances (module docstring)."""
    _require_extended()
    m, n = A.shape
    l = n + m + 1
    z = np.asarray(z, dtype=np.float64)
    assert z.shape == (2 * l,)
    b, c = np.asarray(b, dtype=LD), np.asarray(c, dtype=LD)
    x, y, tau = z[0:n].astype(LD), z[n:n + m].astype(LD), LD(z[l - 1])
    r, s, kappa = z[l:l + n].astype(LD), z[l + n:l + n + m].astype(LD), LD(z[2 * l - 1])
    Ax, ATy, aAx, aATy, krow, kcol = coo_products(A, x, y)
    u, lu = LD(U), LD(l + 8) * LD(U)
    at = np.abs(tau)
    nb, nc = _norm(b), _norm(c)
    with np.errstate(divide="ignore", invalid="ignore"):             # Julia: x / 0.0 -> Inf / NaN silently
        rp = Ax / tau + s / tau - b                                  # :34
        rd = ATy / tau + c - r / tau                                 # :35
        Ep = u * ((krow + 3) * aAx / at + 3 * np.abs(s) / at + 3 * np.abs(b))
        Ed = u * ((kcol + 3) * aATy / at + 3 * np.abs(c) + 3 * np.abs(r) / at)
        nrp, nrd = _norm(rp), _norm(rd)
        p = nrp / np.abs(1 + nb)
        d = nrd / np.abs(1 + nc)
        ctx, bty = np.sum(c * x), np.sum(b * y)                      # :36-37
        Ectx, Ebty = lu * np.sum(np.abs(c * x)), lu * np.sum(np.abs(b * y))
        a_, b_ = ctx / tau, bty / tau
        den = 1 + np.abs(a_) + np.abs(b_)
        g = np.abs(a_ + b_) / den                                    # :38
        Eab = (Ectx + u * np.abs(ctx)) / at + (Ebty + u * np.abs(bty)) / at
        Eg = Eab * (1 + g) / den + 4 * u * g
        axs = Ax + s                                                 # :59
        Eaxs = u * ((krow + 3) * aAx + 3 * np.abs(s))
        Eaty = u * (kcol + 3) * aATy                                 # :61
        naxs, naty = _norm(axs), _norm(ATy)
        vals = dict(p=p, d=d, g=g, ctx=ctx, bty=bty, nAxs=naxs, nATy=naty, nb=nb, nc=nc, tau=tau, kappa=kappa)
        allow = dict(p=(_norm(Ep) + lu * nrp) / np.abs(1 + nb), d=(_norm(Ed) + lu * nrd) / np.abs(1 + nc), g=Eg, ctx=Ectx, bty=Ebty,
                     nAxs=_norm(Eaxs) + lu * naxs, nATy=_norm(Eaty) + lu * naty, nb=lu * nb, nc=lu * nc, tau=LD(0), kappa=LD(0))
    return vals, allow


def _thresholds(res, eps):
    """the five comparisons of HSDEStatus.jl:54,59,61 as (name of the compared quantity, quantity, threshold, what the threshold is built from)"""
    eps = LD(eps)
    with np.errstate(divide="ignore", invalid="ignore"):
        a_, b_ = np.abs(res["ctx"] / res["tau"]), np.abs(res["bty"] / res["tau"])
        return [("p", res["p"], eps * (1 + res["nb"])),
                ("d", res["d"], eps * (1 + res["nc"])),
                ("g", res["g"], eps * (1 + a_ + b_)),
                ("nAxs", res["nAxs"], eps * (-res["ctx"] / res["nc"])),
                ("nATy", res["nATy"], eps * (-res["bty"] / res["nb"]))]


def decide(res, eps):
    """HSDEStatus.jl:53-63: comparisons with NaN are false, x / 0 is +-Inf or NaN."""
    t = {k: (q, th) for k, q, th in _thresholds(res, eps)}
    le = lambda k: bool(t[k][0] <= t[k][1])
    if le("p") and le("d") and le("g"):
        return "Optimal"
    if le("nAxs"):
        return "Unbounded"
    if le("nATy"):
        return "Infeasible"
    return "Continue"


def margin(res, eps):
    """smallest |quantity - threshold| / max(|quantity|, |threshold|) over the five comparisons; a comparison with a NaN or an infinite side
    cannot be turned by rounding and counts as infinitely far"""
    out = np.inf
    for _, q, th in _thresholds(res, eps):
        if not (np.isfinite(q) and np.isfinite(th)):
            continue
        scale = max(abs(q), abs(th))
        out = min(out, float(abs(q - th) / scale) if scale > 0 else 0.0)
    return out


def relative_allowance(res, allow, eps):
    """largest (allowance of the quantity + allowance of its threshold) / max(|quantity|, |threshold|) over the same comparisons"""
    eps = LD(eps)
    with np.errstate(divide="ignore", invalid="ignore"):
        at = np.abs(res["tau"])
        Eth = dict(p=eps * allow["nb"], d=eps * allow["nc"],
                   g=eps * ((allow["ctx"] + LD(U) * np.abs(res["ctx"])) / at + (allow["bty"] + LD(U) * np.abs(res["bty"])) / at),
                   nAxs=eps * (allow["ctx"] / res["nc"] + np.abs(res["ctx"]) * allow["nc"] / res["nc"] ** 2),
                   nATy=eps * (allow["bty"] / res["nb"] + np.abs(res["bty"]) * allow["nb"] / res["nb"] ** 2))
    out = 0.0
    for k, q, th in _thresholds(res, eps):
        if not (np.isfinite(q) and np.isfinite(th)):
            continue
        scale = max(abs(q), abs(th))
        if scale > 0:
            out = max(out, float((allow[k] + Eth[k]) / scale))
    return out


def ratios(got, vals, allow):
    """{field: |got - reference| / allowance} for the finite fields (0 / 0 counts as 0, a difference against a zero allowance as inf);
    non-finite reference values are compared as patterns: ratio 0 where the same Inf / NaN stands on both sides, inf otherwise"""
    out = {}
    for k in FIELDS:
        if k not in got:
            continue
        ref, g_ = vals[k], LD(got[k])
        if not np.isfinite(ref) or not np.isfinite(g_):
            same = (np.isnan(ref) and np.isnan(g_)) or (ref == g_)
            out[k] = 0.0 if same else np.inf
            continue
        diff, al = abs(g_ - ref), allow[k]
        out[k] = 0.0 if diff == 0 else (float(diff / al) if al > 0 else np.inf)
    return out


def stacked_q_reference(A, b, c, uvec, with_abs=False):
    """(Q u, componentwise allowance) for the stacked operator Q = [0 A' c; -A 0 b; -c' -b' 0] (HSDEAffine.jl:41-65) in longdouble.
    Rows of A' and A: u (k_i + 3) (|Q||u|)_i with k_i the entries of A in the row; the tau row: (l + 8) u sum |[c; b]_i u_i|.
    with_abs: |Q||u| as a third value."""
    _require_extended()
    m, n = A.shape
    l = n + m + 1
    uvec = np.asarray(uvec, dtype=np.float64)
    x, y, t = uvec[0:n].astype(LD), uvec[n:n + m].astype(LD), LD(uvec[l - 1])
    b, c = np.asarray(b, dtype=LD), np.asarray(c, dtype=LD)
    Ax, ATy, aAx, aATy, krow, kcol = coo_products(A, x, y)
    Qu = np.concatenate([ATy + c * t, -Ax + b * t, [-(np.sum(c * x) + np.sum(b * y))]])
    aQu = np.concatenate([aATy + np.abs(c * t), aAx + np.abs(b * t), [np.sum(np.abs(c * x)) + np.sum(np.abs(b * y))]])
    E = np.concatenate([LD(U) * (np.concatenate([kcol, krow]) + 3) * aQu[:-1], [LD(l + 8) * LD(U) * aQu[-1]]])
    if with_abs:
        return Qu, E, aQu
    return Qu, E
