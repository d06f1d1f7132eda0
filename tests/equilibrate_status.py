"""
The status check of an EQUILIBRATED handle (fos_create3, equil_passes > 0: csrc/equilibrate.hip eq_status_kernel, csrc/step.cpp status_check) held to
the standard of tests/status_reference.py: an fp64 numpy restatement of what the device evaluates, and the worst-case fp64 allowance of that evaluation
against the extended-precision reference ON THE CALLER'S A, b, c.  Shared by test_equilibrate_status_cpu.py (no GPU: the restatement within 1 x allowance,
every decision clear of its threshold) and test_gpu_equilibrate_formats.py (the device within 2 x).

What the device evaluates (header comment of equilibrate.hip), with D, E, sigma, rho the factors of the handle, all positive:
  stored     A^_ij = fl(fl(D_i a_ij) E_j),  b^_i = fl(sigma fl(D_i b_i)),  c^_j = fl(rho fl(E_j c_j))                      two roundings per entry
  iterate in x^_j = fl(x_j fl(sigma / E_j)),  y^_i = fl(y_i fl(rho / D_i)),  r^_j = fl(r_j fl(rho E_j)),  s^_i = fl(s_i fl(sigma D_i)),
             tau^ = tau,  kappa^ = fl(kappa fl(sigma rho))                                                                 two roundings per entry, tau none
  sweep      w_x = A^'y^,  w_y = -A^ x^      (the tau entry taken as zero: no c^ tau, b^ tau)                               k_i-term dot products
  rows       rd_j  = fl(1/E_j) ((w_x,j / tau + c^_j) - r^_j / tau)       aty_j = fl(1/E_j) w_x,j
             rp_i  = fl(1/D_i) ((s^_i / tau - w_y,i / tau) - b^_i)       axs_i = fl(1/D_i) (s^_i - w_y,i)
  epilogue   p = sqrt(sum rp^2) / sigma / |1 + ||b|||,  d = sqrt(sum rd^2) / rho / |1 + ||c|||,  ||A x + s|| = sqrt(sum axs^2) / sigma,
             ||A'y|| = sqrt(sum aty^2) / rho,  c'x = (sum c^_j x^_j) / fl(sigma rho),  b'y alike,  kappa = kappa^ / fl(sigma rho),  g from c'x, b'y, tau as
             the plain handle does; ||b||, ||c|| are fp64 norms of the caller's vectors.

In exact arithmetic every row is the reference's row times a positive factor that the epilogue divides out, WHATEVER the values of D, E, sigma, rho: their
own rounding is no error of the check.  The allowance therefore is that of status_reference.reference with the roundings of the scaled evaluation added,
term by term (u = 2^-53; every count is a first-order bound on the partial results, as there):

  dual residual row j, reference  u [(k_j + 3) (|A|'|y|)_j / |tau| + 3 |c_j| + 3 |r_j| / |tau|]:
      each product A^_ij y^_i carries 2 + 2 roundings more (A^, y^): k_j + 4 for the dot product; the division by tau 1; the addition of c^ 1; the
      subtraction of r^ / tau 1; fl(1 / E_j) and the product with it 2                                          -> (k_j + 9) (|A|'|y|)_j / |tau|
      c^_j: 2 (stored), the addition 1, the subtraction 1, the factor 2                                         -> 6 |c_j|
      r^_j: 2 (scaled in), its division 1, the subtraction 1, the factor 2                                      -> 6 |r_j| / |tau|
  primal residual row i, reference  u [(k_i + 3) (|A||x|)_i / |tau| + 3 |s_i| / |tau| + 3 |b_i|]:
      A^ x^: k_i + 4, the division 1, two subtractions 2, the factor 2                                          -> (k_i + 9) (|A||x|)_i / |tau|
      s^_i: 2, its division 1, two subtractions 2, the factor 2                                                 -> 7 |s_i| / |tau|
      b^_i: 2, the subtraction 1, the factor 2                                                                  -> 5 |b_i|
  A x + s row i, reference u [(k_i + 3) (|A||x|)_i + 3 |s_i|]:  k_i + 4, the subtraction 1, the factor 2        -> (k_i + 7) (|A||x|)_i;   s^: 2 + 1 + 2 -> 5 |s_i|
  A'y row j, reference u (k_j + 3) (|A|'|y|)_j:                 k_j + 4, the factor 2                           -> (k_j + 6) (|A|'|y|)_j
      Neither contains a tau |b| or tau |c| term: the reference's A x + s and A'y (HSDEStatus.jl:59,61) have none.
  norms: the reference's (l + 8) u ||v|| has 3.5 u to spare at l' <= l - 1 rows; the one division by sigma or rho fits.  Unchanged.
  c'x, b'y, reference (l + 8) u sum |c_j x_j|: each product carries 2 + 2 roundings more, fl(sigma rho) 1, the division by it 1 -> (l + 14) u sum |c_j x_j|
  g: the reference's quotient rule on these c'x, b'y allowances.
  kappa = fl(fl(kappa P) / P), P = fl(sigma rho): two roundings -> 2 u |kappa|.   tau: copied, 0.   ||b||, ||c||: the reference's.

restate() is that evaluation in numpy fp64 (scipy's CSR / CSC products for the sweep, numpy's pairwise sums): one fp64 evaluation, so it must lie within
1 x the allowance; restate(fixed=False) is the formula the kernel had before -- w = Q^ [x^; y^; tau] with c^ tau, b^ tau inside, subtracted again for
||A x + s|| and ||A'y||, and p, d as a finite norm over sigma |tau| -- kept to show that the allowance bites.
"""
import numpy as np
import scipy.sparse as sp

import equilibrate_cases as ec
import status_cases as cases
import status_reference as sref

LD = sref.LD
U = sref.U
PASSES = (1, 10)


def reference(A, b, c, z):
    """-> (values, allowances) over sref.FIELDS: the values of status_reference.reference on the caller's data, the allowances of the scaled evaluation
    (module docstring)"""
    vals, _ = sref.reference(A, b, c, z)
    m, n = A.shape
    l = n + m + 1
    z = np.asarray(z, dtype=np.float64)
    b, c = np.asarray(b, dtype=LD), np.asarray(c, dtype=LD)
    x, y, tau = z[0:n].astype(LD), z[n:n + m].astype(LD), LD(z[l - 1])
    r, s, kappa = z[l:l + n].astype(LD), z[l + n:l + n + m].astype(LD), LD(z[2 * l - 1])
    Ax, ATy, aAx, aATy, krow, kcol = sref.coo_products(A, x, y)
    u, lu, lu_dot = LD(U), LD(l + 8) * LD(U), LD(l + 14) * LD(U)
    at = np.abs(tau)
    nb, nc = vals["nb"], vals["nc"]
    with np.errstate(divide="ignore", invalid="ignore"):
        Ep = u * ((krow + 9) * aAx / at + 7 * np.abs(s) / at + 5 * np.abs(b))
        Ed = u * ((kcol + 9) * aATy / at + 6 * np.abs(c) + 6 * np.abs(r) / at)
        nrp, nrd = vals["p"] * np.abs(1 + nb), vals["d"] * np.abs(1 + nc)
        Ectx, Ebty = lu_dot * np.sum(np.abs(c * x)), lu_dot * np.sum(np.abs(b * y))
        a_, b_ = vals["ctx"] / tau, vals["bty"] / tau
        den = 1 + np.abs(a_) + np.abs(b_)
        Eab = (Ectx + u * np.abs(vals["ctx"])) / at + (Ebty + u * np.abs(vals["bty"])) / at
        Eg = Eab * (1 + vals["g"]) / den + 4 * u * vals["g"]
        Eaxs = u * ((krow + 7) * aAx + 5 * np.abs(s))
        Eaty = u * (kcol + 6) * aATy
        allow = dict(p=(sref._norm(Ep) + lu * nrp) / np.abs(1 + nb), d=(sref._norm(Ed) + lu * nrd) / np.abs(1 + nc), g=Eg, ctx=Ectx, bty=Ebty,
                     nAxs=sref._norm(Eaxs) + lu * vals["nAxs"], nATy=sref._norm(Eaty) + lu * vals["nATy"], nb=lu * nb, nc=lu * nc, tau=LD(0),
                     kappa=2 * u * np.abs(kappa))
    return vals, allow


def _decide(res, eps):
    """status_decide of csrc/step.cpp (HSDEStatus.jl:53-63) on fp64 values"""
    with np.errstate(divide="ignore", invalid="ignore"):
        if (res["p"] <= eps * (1 + res["nb"]) and res["d"] <= eps * (1 + res["nc"])
                and res["g"] <= eps * (1 + abs(res["ctx"] / res["tau"]) + abs(res["bty"] / res["tau"]))):
            return "Optimal"
        if res["nAxs"] <= eps * (-res["ctx"] / res["nc"]):
            return "Unbounded"
        if res["nATy"] <= eps * (-res["bty"] / res["nb"]):
            return "Infeasible"
    return "Continue"


def restate(b, c, eq, z, eps=None, fixed=True):
    """the check of an equilibrated handle on the caller's z, in numpy fp64.  eq: the factors and scaled data (pkg.host_equilibrate or
    equilibrate_cases.equilibrate_ref); b, c: the caller's vectors (their norms).  -> dict over sref.FIELDS (+ "status" when eps is given)"""
    f8 = np.float64
    As = sp.csc_matrix(eq["A"])
    m, n = As.shape
    l = n + m + 1
    z = np.asarray(z, dtype=f8)
    D, E, sg, rho = eq["D"], eq["E"], f8(eq["sigma"]), f8(eq["rho"])
    bs, cs = np.asarray(eq["b"], dtype=f8), np.asarray(eq["c"], dtype=f8)
    tau = f8(z[l - 1])
    xs, ys = z[0:n] * (sg / E), z[n:n + m] * (rho / D)
    rs, ss = z[l:l + n] * (rho * E), z[l + n:l + n + m] * (sg * D)
    ks = f8(z[2 * l - 1]) * (sg * rho)
    iE, iD = 1.0 / E, 1.0 / D
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if fixed:
            wx, wy = As.T @ ys, -(As @ xs)
            rd = iE * ((wx / tau + cs) - rs / tau)
            aty = iE * wx
            rp = iD * ((ss / tau - wy / tau) - bs)
            axs = iD * (ss - wy)
        else:
            wx, wy = As.T @ ys + tau * cs, -(As @ xs - tau * bs)
            rd = iE * (wx - rs)
            aty = iE * (wx - cs * tau)
            rp = iD * (ss - wy)
            axs = iD * ((bs * tau - wy) + ss)
        nb, nc = np.sqrt(np.sum(np.asarray(b, dtype=f8) ** 2)), np.sqrt(np.sum(np.asarray(c, dtype=f8) ** 2))
        ctx, bty = np.sum(cs * xs) / (sg * rho), np.sum(bs * ys) / (sg * rho)
        if fixed:
            p = np.sqrt(np.sum(rp * rp)) / sg / abs(1 + nb)
            d = np.sqrt(np.sum(rd * rd)) / rho / abs(1 + nc)
        else:
            p = np.sqrt(np.sum(rp * rp)) / (sg * abs(tau)) / abs(1 + nb)
            d = np.sqrt(np.sum(rd * rd)) / (rho * abs(tau)) / abs(1 + nc)
        g = abs(ctx / tau + bty / tau) / (1 + abs(ctx / tau) + abs(bty / tau))
        out = dict(p=p, d=d, g=g, ctx=ctx, bty=bty, nAxs=np.sqrt(np.sum(axs * axs)) / sg, nATy=np.sqrt(np.sum(aty * aty)) / rho, nb=nb, nc=nc, tau=tau,
                   kappa=ks / (sg * rho))
    if eps is not None:
        out["status"] = _decide(out, eps)
    return out


# ---- the cases of test_gpu_equilibrate_formats.py, chosen and checked on the CPU (test_equilibrate_status_cpu.py)

# l = 63, 64, 65: the last wavefront of eq_status_kernel partial, full, just exceeded; n + m > 131 072: the second trip of its grid-stride loop
EDGE_SHAPES = [(22, 40), (23, 40), (24, 40), (60000, 80000)]
CERTIFICATE_OPERATORS = ("tile-mixed", "tall")


def edge_problem(pkg, m, n):
    """(name, A, b, c) of the sparse LP of test_gpu_equilibrate.test_status_at_the_kernels_edges"""
    prob = ec.sparse_lp(pkg, m, n, seed=m + n)
    return "sparse-lp-%dx%d" % (m, n), prob.A, prob.b, prob.c


def point_sets(name, A, b, c, certificates=False):
    """[(label, A, b, c, z, expected verdict or None)]: status_cases.points, its scaled problem, and one constructed point per verdict where asked"""
    A = sp.csc_matrix(A)
    out = [(label, A, b, c, z, None) for label, z in cases.points(name, A, b, c)]
    As, bs, cs, zs = cases.scaled_problem(name, A, b, c)
    out.append(("scaled 1e-6..1e6", As, bs, cs, zs, None))
    if certificates:
        out += [("certificate " + want, A, b, c, z, want) for want, z in cases.certificates(A, b, c)]
    return out


def free_cones(A):
    m, n = A.shape
    return [("Free", m)], [("Free", n)]


# second handles whose cones couple rows and columns (SOC, SDP: the block means of the recipe), on a dual-tile and a window-panel operator
CONE_VARIANTS = {
    "tile-mixed": ([("SOC", 48), ("SDP", 120), ("Free", 20)], [("SOC", 50), ("SDP", 45), ("NonNeg", 55)]),                 # 188 x 150
    "tall": ([("SOC", 1000), ("SDP", 55), ("NonNeg", 7945)], [("SDP", 210), ("SOC", 40), ("NonNeg", 50)]),                                 # 9000 x 300
}
