"""Shared pieces of the equilibration tests (test_equilibrate_cpu.py, test_gpu_equilibrate.py): a numpy restatement of the scaling recipe, written from
its description and not from csrc/equilibrate.cpp; badly scaled versions of the generated problems; a problem that holds every cone kind on both sides.

The recipe (minimize c'x  s.t.  A x + s = b, s in K1, x in K2):  D = 1_m, E = 1_n; `passes` times: A^ = (D A) E from the original values, r = row maxima and
c = column maxima of |A^| (1 for an empty row / column), both replaced by their arithmetic mean over every SOC / SOCRotated / SDP / ExpPrimal / ExpDual cone,
D /= sqrt(r), E /= sqrt(c).  Then gamma = sqrt(min(m, n)) / |A^|_F (1 if A^ = 0) is folded into D, sigma = 10 / |D b|, rho = 10 / |E c| (1 where the norm is 0),
and the scaled problem is A^ = D A E, b^ = sigma D b, c^ = rho E c."""
import math

import numpy as np
import scipy.sparse as sp

NON_SEPARABLE = ("SOC", "SOCRotated", "SDP", "ExpPrimal", "ExpDual")
TARGET = 10.0


def blockmean(v, cones):
    """v with its mean over the range of every non-separable cone of `cones` ((name, length) in order); the other entries stay"""
    out = np.array(v, dtype=np.float64)
    at = 0
    for name, length in cones:
        if name in NON_SEPARABLE:
            out[at:at + length] = np.mean(out[at:at + length])
        at += length
    assert at == out.shape[0]
    return out


def equilibrate_ref(A, b, c, K1, K2, passes):
    A = sp.csc_matrix(A)
    A.sort_indices()
    m, n = A.shape
    rows = A.indices
    cols = np.repeat(np.arange(n), np.diff(A.indptr))
    nz = A.data
    D, E = np.ones(m), np.ones(n)
    for _ in range(passes):
        absA = np.abs((D[rows] * nz) * E[cols])
        r, cc = np.zeros(m), np.zeros(n)
        np.maximum.at(r, rows, absA)
        np.maximum.at(cc, cols, absA)
        r[r == 0] = 1.0
        cc[cc == 0] = 1.0
        D = D / np.sqrt(blockmean(r, K1))
        E = E / np.sqrt(blockmean(cc, K2))
    fro = math.sqrt(float(np.sum(((D[rows] * nz) * E[cols]) ** 2)))
    gamma = math.sqrt(min(m, n)) / fro if fro > 0 else 1.0
    D = D * gamma
    nzs = (D[rows] * nz) * E[cols]
    Db, Ec = D * b, E * c
    nb, nc = np.linalg.norm(Db), np.linalg.norm(Ec)
    sigma = TARGET / nb if nb > 0 else 1.0
    rho = TARGET / nc if nc > 0 else 1.0
    As = sp.csc_matrix((nzs, rows.copy(), A.indptr.copy()), shape=(m, n))
    return dict(passes=passes, D=D, E=E, sigma=sigma, rho=rho, gamma=gamma, A=As, b=sigma * Db, c=rho * Ec)


def badly_scaled(prob, seed, decades=2):
    """rows times blockmean(10 ** U(-decades, decades)) over K1, columns likewise over K2, b times the row and c times the column factors: the same
    cones, and the planted optimal pair moves with the data"""
    rng = np.random.default_rng(seed)
    rf = blockmean(10.0 ** rng.uniform(-decades, decades, prob.m), prob.K1)
    cf = blockmean(10.0 ** rng.uniform(-decades, decades, prob.n), prob.K2)
    A = sp.csc_matrix(sp.diags(rf) @ prob.A @ sp.diags(cf))
    A.sort_indices()
    kw = {}
    if prob.x0 is not None:
        kw = dict(x0=prob.x0 / cf, y0=prob.y0 / rf, s0=prob.s0 * rf)
    return type(prob)(prob.name + "-badly-scaled", A, prob.b * rf, prob.c * cf, list(prob.K1), list(prob.K2), meta=dict(prob.meta, row_factors=rf, col_factors=cf), **kw)


# ---- every cone kind on both sides (small_mixed has no rotated and no exponential cones)

ALL_K1 = [("Zero", 3), ("NonNeg", 4), ("SOC", 5), ("SOCRotated", 4), ("ExpPrimal", 3), ("ExpDual", 3), ("SDP", 6), ("NonPos", 2), ("Free", 2)]
ALL_K2 = [("Free", 3), ("NonNeg", 4), ("SOCRotated", 4), ("ExpPrimal", 3), ("ExpDual", 3), ("SDP", 6), ("SOC", 3), ("Zero", 1)]


def _pair(pkg, rng, name, length):
    """(s in K, y in K*, s'y = 0), both on the boundary for the kinds workloads._moreau_pair does not know"""
    if name == "SOCRotated":                     # { (a, b, v): 2 a b >= |v|^2, a, b >= 0 }, self-dual
        v = rng.standard_normal(length - 2)
        a = rng.uniform(0.5, 2.0)
        bb = float(v @ v) / (2 * a)
        return np.concatenate([[a, bb], v]), np.concatenate([[bb, a], -v])
    if name in ("ExpPrimal", "ExpDual"):         # K = cl{ y e^(x/y) <= z, y > 0 },  K* = cl{ -u e^(v/u) <= e w, u < 0 }
        t = rng.uniform(-1.0, 1.0)
        y = rng.uniform(0.5, 2.0)
        prim = np.array([t * y, y, y * math.exp(t)])
        dual = rng.uniform(0.5, 2.0) * np.array([-math.exp(t), -math.exp(t) * (1 - t), 1.0])
        return (prim, dual) if name == "ExpPrimal" else (dual, prim)
    return pkg.workloads._moreau_pair(rng, name, length)


def all_kinds(pkg, seed=5):
    rng = np.random.default_rng(seed)
    m, n = sum(k for _, k in ALL_K1), sum(k for _, k in ALL_K2)
    A = sp.random(m, n, density=0.35, format="csc", random_state=rng, data_rvs=rng.standard_normal)
    A.sort_indices()
    sy = [_pair(pkg, rng, name, k) for name, k in ALL_K1]
    xr = [_pair(pkg, rng, name, k) for name, k in ALL_K2]
    s0, y0 = np.concatenate([p[0] for p in sy]), np.concatenate([p[1] for p in sy])
    x0, r0 = np.concatenate([p[0] for p in xr]), np.concatenate([p[1] for p in xr])
    x0, s0, y0, r0, b, c = pkg.workloads.normalize_data(x0, s0, y0, r0, A)
    return pkg.workloads.ConicProblem("all-kinds", A, b, c, list(ALL_K1), list(ALL_K2), x0=x0, y0=y0, s0=s0)


def sparse_lp(pkg, m, n, seed):
    """at most 3 non-zeros per column, Zero rows and NonNeg columns (m = 1: NonNeg rows): the shapes at which the status kernel's grid changes"""
    rng = np.random.default_rng(seed)
    per = min(3, m)
    first = rng.integers(m, size=n)
    step = max(1, m // 3)                        # first, first + step, first + 2 step (mod m): distinct rows
    rows = np.stack([(first + k * step) % m for k in range(per)], axis=1).ravel()
    cols = np.repeat(np.arange(n), per)
    A = sp.csc_matrix((rng.standard_normal(per * n), (rows, cols)), shape=(m, n))
    A.sort_indices()
    K1 = [("Zero", m // 2), ("NonNeg", m - m // 2)] if m > 1 else [("NonNeg", 1)]
    return pkg.workloads.from_complementary_pair("sparse-lp-%dx%d" % (m, n), A, K1, [("NonNeg", n)], rng)


def map_to_caller(zhat, eq, m, n):
    """the scaled problem's iterate in the caller's units: x = E x^ / sigma, y = D y^ / rho, tau, r = r^ / (rho E), s = s^ / (sigma D), kappa = kappa^ / (sigma rho)"""
    l = m + n + 1
    D, E, sg, rho = eq["D"], eq["E"], eq["sigma"], eq["rho"]
    z = np.array(zhat, dtype=np.float64)
    z[0:n] = E * zhat[0:n] / sg
    z[n:n + m] = D * zhat[n:n + m] / rho
    z[l:l + n] = zhat[l:l + n] / (rho * E)
    z[l + n:l + n + m] = zhat[l + n:l + n + m] / (sg * D)
    z[2 * l - 1] = zhat[2 * l - 1] / (sg * rho)
    return z
