"""Seeded PSD-cone inputs with long-double references for the projection kernels of csrc/psd.hip (psd_kernel, psd64_wave_kernel, psd64_refine_kernel) and
csrc/psd_sign.hip, shared by test_psd_cases_cpu.py and test_gpu_psd_edges.py.  Nothing is stored: every case is regenerated from its seed.

REFERENCES.  Every case is built from a known eigen-decomposition in numpy.longdouble (64-bit mantissa, eps = 1.08e-19, asserted): Q is a product of k
Householder reflectors I - 2 v v' / v'v with seeded v, M = Q diag(w) Q', P = Q diag(max(w, 0)) Q'.  x = svec(M) is rounded to double ONCE and p_ref = svec(P)
stays in long double.  The projection is non-expansive and svec an isometry, so the exact projection of the rounded x is within 2^-53 ||x||_2 of svec(P);
Q is orthogonal to 1e-18 (test_psd_cases_cpu.py asserts it and recomputes the references with mpmath at 50 digits) -- how a reference was found does not
matter.  The cases without Q (diagonal, +-I, [[0,a],[a,0]] blocks, +-vv') have closed-form projections.

TOLERANCE.  Per matrix: max_i |y_i - p_ref_i| <= (a + b k) U, U = 2^-52 ||x_cone||_2 (+ a term per path, below).  The constants are a count of roundings, not
a fit: nothing here was taken from device output.  The model of the count:
  * u = 2^-53.  The kernels hold Mt = +-sqrt(2) M (diagonal of the packed vector x sqrt 2: ||Mt||_F = sqrt(2) ||x||) and return Pt's lower triangle with
    the diagonal / sqrt 2, so an output entry is off by at most the error of an entry of Pt.
  * a rounding is charged u x (a bound on the number it rounds): entries and column norms of the shifted array G by mu = (1 + 1.001) ||Mt||_F
    (u mu = 1.415 U), entries of Mt, Pt and the eigenvalues by ||Mt||_F (u ||Mt||_F = 0.707 U).  Rotations, being orthogonal, and the projection, being
    non-expansive, amplify nothing.  An error of G enters Pt = sum (n_j - sigma) / n_j^2 g_j g_j' twice and is scaled by (n_j - sigma) / n_j <= 2/3
    (sigma >= 0.505 ||Mt||_F): factor 4/3.
  * n roundings that enter ONE output entry with unrelated signs are charged sqrt(n), not n (Wilkinson's rule, Higham, Accuracy and Stability, 2.8): the
    bounds above are column NORMS where the number rounded is one ENTRY of the column, sqrt(k) smaller on average, which is the reserve of this model.
    The linear form comes from  sqrt(k) <= k / (2c) + c / 2  (tangent at k = c^2).

  Jacobi kernels, order <= 64 (tangent at k = 64: sqrt(k) <= k / 16 + 4):
    reference                x rounded to double                                                   0.5 U
    load                     diagonal x SQRT2 (the constant and the product)       2 u ||Mt||   =  1.41 U
    shift                    fl(Mt_ii + sigma); sigma itself need not be accurate: the same
                             number is subtracted from the column norms                1 u mu   =  1.41 U
    warm product             G0 = M' V_prev, k-term dot products             4/3 sqrt(k) u mu
    sweeps x rotations       at most PSD_MAX_SWEEPS = 40 sweeps of k - 1 rotations per column,
                             two roundings each (product, fused multiply-add)  4/3 sqrt(80 k) u mu
    stop criterion           a pair is left alone at |cos| <= k 2^-52: the two eigenvectors are
                             off by that angle x n_i n_j / (n_i^2 - n_j^2), Pt by
                             (n_i - n_j) x the angle <= k 2^-52 mu / 2                          =  1.415 k U
    weights                  column norm^2 (k terms, the root halves it) 0.5 sqrt(k) u mu, root 1 u mu,
                             n - sigma and the division 2 u ||Mt||
    rebuild                  weight x entry 1 u ||Mt||, k-term accumulation sqrt(k) u ||Mt||
    pack                     diagonal x INV_SQRT2 (constant and product) 2 u ||Mt||; dual copy x + P: 2 u ||x|| = 1 U
    sum:  constants 0.5 + 1.41 + 1.41 + (1.41 + 1.41) + 0.71 + 1.41 + 1 = 9.3 U;  sqrt(k) terms (4/3 (1 + 8.95) + 0.5 + 0.5) 1.415 U = 20.2 sqrt(k) U
          <= (1.26 k + 80.8) U;  linear 1.415 k U    ->    a = 90, b = 2.7    (95 U at order 2, 263 U at order 64)
    A matrix that psd64_refine_kernel ACCEPTS (record >= 100) is not iterated to a rotation-free sweep but to ||E||_F <= 1e-6 at the last update; its
    header states what that leaves: "error of the projection < 1e-13 ||M||".  That claim is the extra term of such a matrix, 1e-13 ||Mt||_F = 637 U.

  Sign iteration, order > 64 (padded order K <= k + 63; tangent at K = 256: sqrt(K) <= K / 32 + 8): an error dS of the computed sign enters
  P = (M + M S) / 2 as lambda dS / 2, so a rounding of a product is charged u ||Mt||_F / 2 = 0.354 U per unit of the iterate, and the K-term dot
  products of one 64 x 64 x K product sqrt(K) of those.  Between eigenvectors of equal sign the iteration damps an error, between opposite signs it
  carries it with a factor (a_0 + |b_0|) / (a_t + |b_t|) <= 1 (divided differences of the step polynomials), so every product counts once:
    growth step (26)         A = X X enters T through (2 c A + b) dA, |.| <= 4.8, and X T through ||X|| <= 1.19: (5.7)^2 = 32.7 K roundings;
                             T = c A A + b A + a I: three terms up to 4.8 that cancel to 0.7, x 1.19: (2.03 x 1.42 x 1.19)^2 + 2 = 13.8 K;  X T: K
    Newton-Schulz step (6)   A = X X through 0.5 X dA: 0.35 K;  (3 X - X A) / 2: K + 2
    last product             (M + M S) / 2: K
    sum:  26 x 47.5 K + 6 x 1.4 K + K = 1245 K roundings -> sqrt = 35.3 sqrt(K) x 0.354 U = 12.5 sqrt(K) U <= (0.39 K + 100) U <= (0.39 k + 125) U
    unpack (SQRT2, 1 / ||M||_F: 3 u ||Mt||), pack (symmetrise, INV_SQRT2, x + P: 3 u ||Mt|| + 1 U), reference 0.5 U, and the eigenvalues that rounding x
    moved off zero (at most 2^-53 ||x||, sign undecided: 0.5 U): 6.2 U            ->    a = 132, b = 0.39    (157 U at order 65, 210 U at order 200)
    Extra term: an eigenvalue below 1e-14 ||M||_F does not reach the Newton-Schulz basin in 26 growth steps (3.4445^26 = 9.3e13) and leaves an error of
    at most its own size: + sqrt(2) max{|w_i| : |w_i| < 1e-14 ||w||_2} (in Mt's scale).

Both forms are below today's whole-vector bound 5e-13 max(1, ||x||) (2252 U) at every order used, the accepted-refinement term included (900 U), and
numpy's LAPACK stays within a quarter of them (test_psd_cases_cpu.py; figures in profiles/psd_edges_allowance.txt)."""
import math

import numpy as np

LD = np.longdouble
U52 = 2.0 ** -52
JACOBI_AB = (90.0, 2.7)
SIGN_AB = (132.0, 0.39)
REFINE_CLAIM = 1e-13 * math.sqrt(2.0) / U52          # "error of the projection < 1e-13 ||M||" in units of U
SIGN_UNRESOLVED = 1e-14
OLD_BOUND = 5e-13                                    # today's whole-vector bound: 5e-13 max(1, ||x||)

MIXED_K1 = [1, 2, 3, 8, 9, 16, 17, 32, 33, 63, 64]
MIXED_K2 = [5, 64]
MANY_ORDERS = list(range(1, 10))
SIGN_ORDERS = [65, 128, 129, 200]
ORDERS = sorted(set(MIXED_K1 + MIXED_K2 + MANY_ORDERS + SIGN_ORDERS))
SPECTRA = ["gauss100", "decades", "rank_deficient", "pairs", "clusters", "near_zero", "one_large", "all_positive", "all_negative", "zero"]
PLAIN = ["diagonal", "plus_identity", "minus_identity", "offdiag_blocks", "rank_one_pos", "rank_one_neg"]
NAMES = SPECTRA + PLAIN
HOMOGENEITY_BASE = ["gauss100", "pairs"]             # every eigenvalue well away from the subnormals at 2^-400
HOMOGENEITY_SCALES = [100, -100, 400, -400]


def require_long_double():
    assert np.finfo(LD).eps < 2e-19, "numpy.longdouble has no 64-bit mantissa here: the references of psd_cases.py need it"


def tri(k):
    return k * (k + 1) // 2


def tolerance_units(k, refined=False):
    a, b = SIGN_AB if k > 64 else JACOBI_AB
    return a + b * k + (REFINE_CLAIM if refined else 0.0)


def svec(M):
    """lower triangle, column-major, off-diagonals x sqrt 2, in M's precision"""
    k = M.shape[0]
    r2 = np.sqrt(M.dtype.type(2))
    out = np.empty(tri(k), dtype=M.dtype)
    idx = 0
    for j in range(k):
        out[idx] = M[j, j]
        out[idx + 1:idx + k - j] = M[j + 1:, j] * r2
        idx += k - j
    return out


def smat(x, k):
    """the inverse of svec, in x's precision"""
    M = np.zeros((k, k), dtype=x.dtype)
    r2 = np.sqrt(x.dtype.type(2))
    idx = 0
    for j in range(k):
        M[j, j] = x[idx]
        M[j + 1:, j] = x[idx + 1:idx + k - j] / r2
        M[j, j + 1:] = M[j + 1:, j]
        idx += k - j
    return M


def reflectors(k, name):
    """the k seeded Householder vectors of a case"""
    return np.random.default_rng([31, k, NAMES.index(name)]).standard_normal((k, k))


def householder_q(V):
    """Q = H_1 H_2 ... H_k, H = I - 2 v v' / v'v, in long double"""
    k = V.shape[1]
    Q = np.eye(k, dtype=LD)
    for v in V.astype(LD):
        Q -= np.outer(Q @ v, (LD(2) / (v @ v)) * v)
    return Q


def spectrum(k, name):
    rng = np.random.default_rng([32, k, NAMES.index(name)])
    if name == "gauss100":
        w = 100.0 * rng.standard_normal(k)
    elif name == "decades":
        w = np.where(rng.random(k) < 0.5, -1.0, 1.0) * 10.0 ** rng.uniform(-14.0, 0.0, k)
    elif name == "rank_deficient":
        w = rng.standard_normal(k)
        w[k // 3 + (1 if k < 3 else 0):] = 0.0
    elif name == "pairs":
        lam = rng.integers(1, 10, (k + 1) // 2).astype(np.float64)
        w = (np.repeat(lam, 2) * np.tile([1.0, -1.0], (k + 1) // 2))[:k]
    elif name == "clusters":
        w = np.where(np.arange(k) % 2 == 0, 1.0, -1.0) * (1.0 + 1e-9 * rng.standard_normal(k))
    elif name == "near_zero":
        w = 1e-9 * rng.standard_normal(k)
    elif name == "one_large":
        w = 1e-12 * np.where(rng.random(k) < 0.5, -1.0, 1.0)
        w[int(rng.integers(k))] = 1.0
    elif name == "all_positive":
        w = 1.0 + 99.0 * rng.random(k)                    # (no eigenvalue within 1 % of zero: the kernels' weight test nr > sigma is beyond doubt)
    elif name == "all_negative":
        w = -(1.0 + 99.0 * rng.random(k))
    elif name == "zero":
        w = np.zeros(k)
    else:
        raise KeyError(name)
    return w


def plain_case(k, name):
    """-> (M, P) in long double for the cases that need no rotation"""
    rng = np.random.default_rng([33, k, NAMES.index(name)])
    M = np.zeros((k, k), dtype=LD)
    if name == "diagonal":
        d = (10.0 * rng.standard_normal(k)).astype(LD)
        return np.diag(d), np.diag(np.maximum(d, LD(0)))
    if name in ("plus_identity", "minus_identity"):
        I = np.eye(k, dtype=LD)
        return (I, I.copy()) if name == "plus_identity" else (-I, M)
    if name == "offdiag_blocks":                          # [[0, a], [a, 0]] has the eigenvalues +-a: P = |a| / 2 [[1, s], [s, 1]], s = sign a
        P = M.copy()
        for i in range(0, k - 1, 2):
            a = LD((1.0 + i) * (-1.0 if i % 4 else 1.0))
            M[i, i + 1] = M[i + 1, i] = a
            P[i, i] = P[i + 1, i + 1] = abs(a) / 2
            P[i, i + 1] = P[i + 1, i] = a / 2
        return M, P
    v = rng.standard_normal(k).astype(LD)
    vv = np.outer(v, v)
    if name == "rank_one_pos":
        return vv, vv.copy()
    if name == "rank_one_neg":
        return -vv, M
    raise KeyError(name)


class Case:
    """One matrix: x = svec(M) in double, p_ref = svec(P_PSD(M)) in long double, ||x||_2, and the sign path's extra term."""
    _cache = {}

    def __init__(self, k, name, V=None, w=None):
        """a named case, or (V, w given) the matrix with the reflectors V and the eigenvalues w"""
        require_long_double()
        self.k, self.name = k, name
        if V is not None or name in SPECTRA:
            self.w = (spectrum(k, name) if w is None else w).astype(LD)
            Q = householder_q(reflectors(k, name) if V is None else V)
            M, P = (Q * self.w) @ Q.T, (Q * np.maximum(self.w, LD(0))) @ Q.T
        else:
            M, P = plain_case(k, name)
            self.w = None
        M, P = (M + M.T) / 2, (P + P.T) / 2
        self.x = np.ascontiguousarray(svec(M).astype(np.float64))
        self.p_ref = svec(P)
        self.norm = float(np.sqrt(np.sum(self.x.astype(LD) ** 2)))
        # the matrix the kernel sees is all-negative (or zero) beyond doubt: its projection is exactly zero
        self.negative = name in ("all_negative", "zero", "minus_identity", "rank_one_neg") and not (name == "rank_one_neg" and k > 1)
        self.positive = name in ("all_positive", "zero", "plus_identity")
        self.unresolved = 0.0
        if self.w is not None and k > 64:
            w = np.abs(self.w.astype(np.float64))
            small = w[(w > 0.0) & (w < SIGN_UNRESOLVED * float(np.linalg.norm(w)))]
            self.unresolved = float(small.max()) if small.size else 0.0

    @classmethod
    def get(cls, k, name):
        if (k, name) not in cls._cache:
            cls._cache[(k, name)] = cls(k, name)
        return cls._cache[(k, name)]

    def label(self):
        return "PSD(%d) %s" % (self.k, self.name)

    def tol(self, refined=False, scale=0):
        return math.ldexp(tolerance_units(self.k, refined) * U52 * self.norm + math.sqrt(2.0) * self.unresolved, scale)

    def error_ratio(self, y, refined=False, scale=0):
        """worst |y - 2^scale p_ref| over the tolerance (0 for an exact answer, inf for anything not finite or for an error against a zero tolerance)"""
        if not np.isfinite(y).all():
            return math.inf
        err = float(np.abs(y.astype(LD) - np.ldexp(self.p_ref, scale)).max())
        tol = self.tol(refined, scale)
        return 0.0 if err == 0.0 else (err / tol if tol > 0.0 else math.inf)

    def check(self, y, dual=False, refined=False, scale=0, what="", exact=True):
        """y against the reference of this copy: a dual copy returns x + P(-x), which for the self-dual cone is P(x) again.  Bit identities (exact=True:
        the Jacobi kernels and, for the zero matrix, every path): the matrix the kernel projects -- x on a primal copy, -x on a dual copy -- has no
        positive eigenvalue: the primal copy is exactly zero, the dual copy exactly x.  -> error / tolerance"""
        ratio = self.error_ratio(y, refined, scale)
        assert ratio <= 1.0, (what, self.label(), "dual" if dual else "primal", "error / tolerance", ratio, "tolerance", self.tol(refined, scale))
        if exact or self.name == "zero":
            if not dual and self.negative:
                assert not y.any(), (what, self.label(), "primal copy of a matrix without positive eigenvalues: not exactly zero")
            if dual and self.positive:
                assert np.array_equal(y, np.ldexp(self.x, scale)), (what, self.label(), "dual copy of a matrix without negative eigenvalues: not exactly x")
        return ratio


DRIFT = 3e-4      # per call: every reflector vector moves by 3e-4 of a Gaussian, every eigenvalue by 3e-4 of the spacing -- an eigenvector turns by about 1e-3


def drift_case(k, seed, t):
    """the t-th matrix of a smooth sequence with a known eigen-decomposition: reflectors V0 + t DRIFT V1 (orthogonal by construction at every t),
    eigenvalues evenly spaced over [-100, 100] and moving by t DRIFT of the spacing -- what a solver's slowly changing iterate looks like"""
    key = ("drift", k, seed, t)
    if key not in Case._cache:
        rng = np.random.default_rng([35, k, seed])
        V0, V1, dw = rng.standard_normal((k, k)), rng.standard_normal((k, k)), rng.standard_normal(k)
        w = np.linspace(-100.0, 100.0, k) + t * DRIFT * (200.0 / max(1, k - 1)) * dw
        Case._cache[key] = Case(k, "drift %d, call %d" % (seed, t), V=V0 + t * DRIFT * V1, w=w)
    return Case._cache[key]


def order_class(k):
    return "sign iteration, order > 64" if k > 64 else "Jacobi kernels, order <= 64"


# ---------------------------------------------------------------------------------------------- the device handles' layouts

def sdp_between_guards(orders):
    K = [("Free", 3)]
    for k in orders:
        K += [("SDP", tri(k)), ("Free", 3)]
    return K


def handle_cones(name, cus=256):
    """-> (K1, K2) of an HSDE handle"""
    if name == "mixed":
        return sdp_between_guards(MIXED_K1), sdp_between_guards(MIXED_K2)
    if name == "many":                                   # cus + 3 small cones and one of order 64: more cones than CUs, the narrow form by count alone
        return sdp_between_guards([MANY_ORDERS[i % 9] for i in range(cus + 3)] + [64]), [("Free", 2)]
    if name == "all64":
        return sdp_between_guards([64, 64, 64]), sdp_between_guards([64])
    if name == "sign":
        return sdp_between_guards([65, 5, 128, 129, 64, 200]), [("Free", 2)]
    raise KeyError(name)


class Slot:
    def __init__(self, kind, length, dual, at, cone):
        self.kind, self.length, self.dual, self.at, self.cone = kind, length, dual, at, cone
        self.k = int(round(math.sqrt(0.25 + 2.0 * length) - 0.5)) if kind == "SDP" else 0


class Layout:
    """where every cone copy sits in the stacked iterate [x(n) -> K2; y(m) -> K1*; tau; r(n) -> K2*; s(m) -> K1; kappa] of an HSDE handle, or in the K1
    list alone (a Feasibility ConeProduct: primal copies only).  `cone` numbers the SDP cones in the order of the library's table (K2, then K1)."""

    def __init__(self, K1, K2=None):
        self.K1, self.K2, self.hsde = K1, K2, K2 is not None
        self.m = sum(l for _, l in K1)
        self.n = sum(l for _, l in K2) if self.hsde else 0
        self.l = self.n + self.m + 1
        self.N = 2 * self.l if self.hsde else self.m
        self.slots = []
        if self.hsde:
            n2 = self._add(K2, 0, False, 0)
            self._add(K1, self.n, True, n2)
            self._add(K2, self.l, True, 0)
            self._add(K1, self.l + self.n, False, n2)
        else:
            self._add(K1, 0, False, 0)
        self.sdp = [s for s in self.slots if s.kind == "SDP"]
        self._rank = None

    def _add(self, cones, at, dual, cone):
        for kind, length in cones:
            self.slots.append(Slot(kind, length, dual, at, cone))
            cone += kind == "SDP"
            at += length
        return cone

    def record_index(self, slot):
        """position of this copy in fos_psd_stats: 2 x (rank among the cones of order <= 64) + part (0: first half of the iterate)"""
        if self._rank is None:
            self._rank = {c: i for i, c in enumerate(sorted({s.cone for s in self.sdp if s.k <= 64}))}
        return 2 * self._rank[slot.cone] + (1 if slot.at >= self.l else 0)

    def fill(self, rnd, scale=0, names=NAMES, seed=0):
        """round `rnd`: the copy of SDP cone c takes the case names[(rnd + c) % len], its dual copy the next one; guard blocks, tau, kappa Gaussians.
        `seed` offsets the choice, so that another round gives every copy an unrelated matrix.  -> (z, [(slot, case)])"""
        z = np.random.default_rng([34, rnd, seed]).standard_normal(self.N)
        used = []
        for s in self.sdp:
            case = Case.get(s.k, names[(rnd + seed + s.cone + (1 if s.dual else 0)) % len(names)])
            z[s.at:s.at + s.length] = np.ldexp(case.x, scale)
            used.append((s, case))
        return z, used

    def check_guards(self, z, y, what=""):
        """Free blocks: the primal copy is the input's bits, the dual copy exactly zero -- no kernel wrote outside its cone"""
        for s in self.slots:
            if s.kind == "Free":
                seg = slice(s.at, s.at + s.length)
                assert np.array_equal(y[seg], np.zeros(s.length) if s.dual else z[seg]), (what, "guard block at %d overwritten" % s.at)
