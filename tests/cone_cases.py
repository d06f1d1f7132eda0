"""Seeded inputs and extended-precision references for the second-order, rotated second-order and exponential cones of csrc/vecops.hip
(cones_soc_kernel, cones_exp_kernel), shared by test_cone_cases_cpu.py and test_gpu_cone_edges.py.

The inputs are regenerated from their seeds here; the references are computed with mpmath at 50 digits, the exponential cones' at 100 (reference_*, certify_*: only these need mpmath) and
travel in tests/golden/cone_edges.npz, written by tests/golden/make_cone_edges.py.  Every reference certifies itself: p = P_K(z) is the unique point with
p in K, p - z in K*, <p, p - z> = 0 (cone_certificates.py), checked in extended precision to 1e-30 relative -- so how a reference was found does not matter.

SOC / rotated SOC.  The tolerance is per element, (16 + len/64) 2^-52 max(|t|, ||v||_2) of that cone's input: in units of u = 2^-53 a fixed-order sum over 64
lanes and a six-step butterfly carry at most (ceil(len/64) + 6) u into ||v||^2, the square root halves that, t/nx, the addition and the two products add
about 4 u; the formula leaves roughly a factor two.  The fixture stores every output of a cone up to 131 entries; for the cones of 4097 / 4098 entries it
stores the head outputs and the scale factor r of the tail as a (hi, lo) pair of doubles, and the expected tail entry is (hi + lo) x_k formed in long double:
the correctly rounded product up to 2^-10 ulp, where a stored double is the correctly rounded one (the CPU test compares the two element by element).

Exponential cones.  Every triple is classed twice.  Its BRANCH (inside, polar, the r < 0, s < 0 face, else the surface) is decided in extended precision; a
closed-form branch is exact.  Its CLASS is benign when |r/s| and |s/r| of the input to exp_project are at most 10 -- there the ported SCS algorithm is
accurate and is held to the certified reference, with an allowance measured from the oracle's restatement -- and ill-conditioned otherwise, where the
algorithm is known to be off by 1e-8 .. 3e-3 or to lose the projection (cone_certificates.py) and only parity with the restatement is asserted."""
import math
from pathlib import Path

import numpy as np

FIXTURE = Path(__file__).resolve().parent / "golden" / "cone_edges.npz"

SOC_LENGTHS = [1, 2, 3, 4, 5, 64, 65, 66, 128, 129, 130, 4097]       # (4 and 5: the K2 cone and the odd cone out of the GPU handles)
ROT_LENGTHS = [2, 3, 4, 65, 66, 67, 131, 4098]
LONG = 1000                                                          # cones longer than this are stored as (head outputs, r_hi, r_lo)
NEAR = 5e-10                                                         # "within 1e-9 relative of the boundary"
_COMMON = ["gauss_1e-3", "gauss_1", "gauss_1e3", "zero", "head_pos", "head_neg", "tail_only", "inside", "polar",
           "near_pos_in", "near_pos_out", "near_neg_in", "near_neg_out"]
_NONFINITE = ["nan_head", "nan_tail", "inf_head", "inf_tail"]
NAMES = {
    "SOC": _COMMON + ["bnd_p0", "bnd_pu", "bnd_pd", "bnd_n0", "bnd_nu", "bnd_nd", "bnd4_p0", "bnd4_n0"] + _NONFINITE,
    "SOCRotated": _COMMON + ["head_mixed", "rbnd_p", "rbnd_n"] + _NONFINITE,
}
LENGTHS = {"SOC": SOC_LENGTHS, "SOCRotated": ROT_LENGTHS}
KINDS = ["SOC", "SOCRotated"]
EXACT = {"zero", "head_pos", "head_neg", "inside", "polar", "bnd_p0", "bnd_n0", "bnd4_p0", "bnd4_n0"}     # the branch is beyond doubt: bit identities hold
HOMOGENEITY_BASE = ["gauss_1", "near_pos_out"]                       # every non-zero entry is above 2^-30: at 2^-480 the squares are still normal numbers
HOMOGENEITY_BITS = [100, -100, 480, -480]
HOMOGENEITY_RANGE = [600, -600]                                      # out of the range of a plain sum of squares: the rescaled norm


def soc_tol(length, t, nv):
    return (16.0 + length / 64.0) * 2.0 ** -52 * max(abs(t), nv)


def _head(kind):
    return 1 if kind == "SOC" else 2


def _last_lane_index(kind, length):
    """a tail entry that lane 63 reads (k = head + 63 + 64 j), else the last entry"""
    k = _head(kind) + 63
    return k if k < length else length - 1


def _boundary_tail(x, head, count):
    """`count` entries equal to 4 / sqrt(count) (2, 0.5 or 0.25), spread evenly over the tail: every partial sum of squares is exact and ||v|| = 4"""
    tail = len(x) - head
    for j in range(count):
        x[head + (j * tail) // count] = 4.0 / math.sqrt(count)


def _boundary_count(tail, name):
    fits = [c for c in (4, 64, 256) if c <= tail]
    if not fits:
        return 0
    return 4 if name.startswith("bnd4") else fits[-1]


def soc_input(kind, length, name):
    rng = np.random.default_rng([20, KINDS.index(kind), length, NAMES[kind].index(name)])
    head = _head(kind)
    g = rng.standard_normal(length)
    x = g.copy()
    rot = kind == "SOCRotated"
    r2 = math.sqrt(2.0)
    nt = math.sqrt(math.fsum(g[head:] ** 2))                     # the norm of the Gaussian tail

    def set_head(t, x2=0.0):                                     # head entries whose rotation is (t, x2) up to rounding
        if rot:
            x[0], x[1] = (t + x2) / r2, (t - x2) / r2
        else:
            x[0] = t

    if name.startswith("gauss_"):
        x *= float(name[6:])
    elif name == "zero":
        x[:] = 0.0
    elif name in ("head_pos", "head_neg", "head_mixed"):
        x[:] = 0.0
        x[0] = 1.5
        if rot:
            x[1] = -0.75 if name == "head_mixed" else 0.75
        if name == "head_neg":
            x[:head] *= -1.0
    elif name == "tail_only":
        x[:head] = 0.0
    elif name == "inside":
        set_head(10.0 * nt + 1.0)
    elif name == "polar":
        set_head(-(10.0 * nt + 1.0))
    elif name.startswith("near_"):
        x2 = g[1] if rot else 0.0
        nx = math.hypot(nt, x2)
        sign = 1.0 if "_pos_" in name else -1.0
        outward = name.endswith("_in")                           # inside the cone (pos) or inside the polar cone (neg): |t| above the norm
        set_head(sign * nx * (1.0 + NEAR if outward else 1.0 - NEAR), x2)
    elif name.startswith("bnd") or name.startswith("rbnd"):
        x[:] = 0.0
        count = _boundary_count(length - head, name)
        if count:
            _boundary_tail(x, head, count)
        elif length - head >= 1:
            x[head] = 4.0                                        # a tail too short for four entries: one entry of 4
        if rot:                                                  # u = w = fl(2 sqrt 2): (u + w) / sqrt 2 is 4 to 1e-15 relative, (u - w) / sqrt 2 is 0
            x[0] = x[1] = (2.0 * r2) * (1.0 if name == "rbnd_p" else -1.0)
        else:
            t = 4.0 if "_p" in name else -4.0
            if name.endswith("u"):
                t = float(np.nextafter(t, np.inf))
            elif name.endswith("d"):
                t = float(np.nextafter(t, -np.inf))
            x[0] = t
    elif name == "nan_head":
        x[0] = np.nan
    elif name == "nan_tail":
        x[_last_lane_index(kind, length)] = np.nan
    elif name == "inf_head":
        x[0] = np.inf
    elif name == "inf_tail":
        x[_last_lane_index(kind, length)] = -np.inf
    else:
        raise KeyError(name)
    return np.ascontiguousarray(x)


# ---------------------------------------------------------------------------------------------- extended precision (mpmath)

def _mp(dps=50):
    import mpmath
    mpmath.mp.dps = dps
    return mpmath.mp


EXP_DPS = 100        # the exponential cones' references: p - z is a difference that cancels 25 digits for an input like (-774.3, 12.71, -162.5), and the
#                      certificate then wants 30 more of what is left


CERT = "1e-30"


def _rotate(mp, a, b):
    c = mp.sqrt(2) / 2                                           # the exact pi/4 rotation, not the kernel's constant
    return c * (a + b), c * (a - b)


def reference_soc(kind, x):
    """-> (p as mpf list, r as mpf, t, ||v||): the closed form, rotated SOC through the exact rotation"""
    mp = _mp()
    v = [mp.mpf(float(a)) for a in x]
    if kind == "SOCRotated":
        v[0], v[1] = _rotate(mp, v[0], v[1])
    t, nx = v[0], mp.sqrt(mp.fsum(a * a for a in v[1:]))
    if t <= -nx:
        r, p = mp.mpf(0), [mp.mpf(0)] * len(v)
    elif t >= nx:
        r, p = mp.mpf(1), list(v)
    else:
        r = (1 + t / nx) / 2
        p = [r * nx] + [r * a for a in v[1:]]
    if kind == "SOCRotated":
        p[0], p[1] = _rotate(mp, p[0], p[1])
    return p, r, t, nx


def _soc_member(mp, kind, p, slack):
    if kind == "SOC":
        return mp.sqrt(mp.fsum(a * a for a in p[1:])) <= p[0] + slack
    return p[0] >= -slack and p[1] >= -slack and mp.fsum(a * a for a in p[2:]) <= 2 * p[0] * p[1] + slack * slack + slack * (abs(p[0]) + abs(p[1]))


def certify_soc(kind, x, p):
    """p in K, p - z in K* = K, <p, p - z> = 0 to 1e-30 relative, in extended precision"""
    mp = _mp()
    z = [mp.mpf(float(a)) for a in x]
    q = [a - b for a, b in zip(p, z)]
    scale = mp.sqrt(mp.fsum(a * a for a in z))
    slack = mp.mpf(CERT) * scale
    assert _soc_member(mp, kind, p, slack), (kind, len(x), "p outside the cone")
    assert _soc_member(mp, kind, q, slack), (kind, len(x), "p - z outside the dual cone")
    assert abs(mp.fsum(a * b for a, b in zip(p, q))) <= slack * scale, (kind, len(x), "<p, p - z> != 0")


def _split(mp, r):
    hi = float(r)
    return hi, float(r - mp.mpf(hi))


def soc_record(kind, length, name, full=None):
    """what the fixture stores for one finite case: every output, or (head outputs, r_hi, r_lo) for a long cone; certified.  `full`: a dict that takes every
    correctly rounded output of the long cones"""
    x = soc_input(kind, length, name)
    p, r, _, _ = reference_soc(kind, x)
    certify_soc(kind, x, p)
    if length <= LONG:
        return np.array([float(a) for a in p])
    if full is not None:
        full[(kind, length, name)] = np.array([float(a) for a in p])
    return np.array([float(a) for a in p[:_head(kind)]] + list(_split(_mp(), r)))


def exp_branch(v):
    """the class of the input of exp_project in extended precision: inside, polar, face (r < 0, s < 0), surface"""
    mp = _mp(EXP_DPS)
    r, s, t = (mp.mpf(float(a)) for a in v)
    if (s > 0 and s * mp.exp(r / s) <= t) or (r <= 0 and s == 0 and t >= 0):
        return "inside"
    if (r > 0 and r * mp.exp(s / r) <= -mp.e * t) or (r == 0 and s <= 0 and t <= 0):
        return "polar"
    if r < 0 and s < 0:
        return "face"
    return "surface"


def _exp_start(v, oracle):
    """a point of the surface near the projection: the oracle's fp64 answer, or (where it loses the projection and returns s = 0) the best of a scan over
    rho = r/s of the closest point of each ray s (rho, 1, e^rho)"""
    y = np.empty(3)
    oracle.prox_exp_primal(y, np.asarray(v, dtype=np.float64))
    if y[1] > 0.0 and y[2] > 0.0:
        return y
    mag = np.logspace(-4.0, math.log10(700.0), 150001)
    rho = np.concatenate([-mag[::-1], [0.0], mag])
    d = np.stack([rho, np.ones_like(rho), np.exp(rho)])
    with np.errstate(over="ignore", invalid="ignore"):
        s = np.maximum(0.0, (np.asarray(v) @ d) / (d * d).sum(axis=0))
        dist = ((np.asarray(v)[:, None] - s * d) ** 2).sum(axis=0)
    k = int(np.nanargmin(dist))
    return s[k] * d[:, k]


def reference_exp_primal(v, oracle):
    """P_K(v) as mpf list; on the surface Newton on p - v + lam grad f(p) = 0, p1 e^rho - p2 = 0, rho = p0/p1, grad f = (e^rho, e^rho (1 - rho), -1)"""
    mp = _mp(EXP_DPS)
    z = [mp.mpf(float(a)) for a in v]
    branch = exp_branch(v)
    if branch == "inside":
        return list(z)
    if branch == "polar":
        return [mp.mpf(0)] * 3
    if branch == "face":
        return [z[0], mp.mpf(0), max(z[2], mp.mpf(0))]
    p = _exp_newton(mp, z, [mp.mpf(float(a)) for a in _exp_start(v, oracle)])
    try:
        certify_exp_primal(v, p)
    except (AssertionError, ZeroDivisionError):
        p = _exp_by_rays(mp, v, z)                                 # (certified by the caller)
    return p


def _exp_by_rays(mp, v, z):
    """Where Newton has no usable start (the projection sits at s ~ e^-150, say): the closest point of the ray s (rho, 1, e^rho) is at s = N / D with
    N = <z, d>, D = <d, d>, at distance^2 ||z||^2 - N^2 / D; every local maximum of N^2 / D over rho with N > 0 is bracketed on a grid and bisected in
    extended precision, and the one that certifies is the projection."""
    def parts(rho):
        E = mp.exp(rho)
        N, D = z[0] * rho + z[1] + z[2] * E, rho * rho + 1 + E * E
        return N, D, 2 * (z[0] + z[2] * E) * D - N * (2 * rho + 2 * E * E)      # the last: the sign of d/drho (N^2 / D) where N > 0
    mag = [mp.mpf(10) ** (mp.mpf(k) / 40 - 4) for k in range(0, 40 * 7)]
    grid = [-a for a in reversed(mag)] + [mp.mpf(0)] + mag
    vals = [parts(r) for r in grid]
    for (a, fa), (b, fb) in zip(zip(grid, vals), zip(grid[1:], vals[1:])):
        if fa[0] > 0 and fb[0] > 0 and fa[2] > 0 >= fb[2]:
            for _ in range(420):
                c = (a + b) / 2
                if parts(c)[2] > 0:
                    a = c
                else:
                    b = c
            N, D, _ = parts(a)
            E = mp.exp(a)
            p = [N / D * a, N / D, N / D * E]
            try:
                certify_exp_primal(v, p)
                return p
            except AssertionError:
                continue
    raise AssertionError((tuple(v), "no certified projection found: replace this triple in the case list"))


def _exp_newton(mp, z, p):
    lam = p[2] - z[2]
    scale = max(mp.mpf(1), mp.sqrt(mp.fsum(a * a for a in z)))
    for _ in range(80):
        rho = p[0] / p[1]
        E = mp.exp(rho)
        F = mp.matrix([p[0] - z[0] + lam * E, p[1] - z[1] + lam * E * (1 - rho), p[2] - z[2] - lam, p[1] * E - p[2]])
        J = mp.matrix([[1 + lam * E / p[1], -lam * E * rho / p[1], 0, E],
                       [-lam * rho * E / p[1], 1 + lam * rho * rho * E / p[1], 0, E * (1 - rho)],
                       [0, 0, 1, -1],
                       [E, E * (1 - rho), -1, 0]])
        d = mp.lu_solve(J, -F)
        p = [p[0] + d[0], p[1] + d[1], p[2] + d[2]]
        lam += d[3]
        if mp.norm(d) <= mp.mpf("1e-95") * scale:
            break
    return p


def _in_exp_primal(mp, p, slack):
    r, s, t = p
    if s > 0 and s * mp.exp(r / s) <= t + slack:
        return True
    return abs(s) <= slack and r <= slack and t >= -slack


def _in_exp_dual(mp, q, slack):
    u, v, w = q
    if u < 0 and -u * mp.exp(v / u) <= mp.e * w + slack:
        return True
    return abs(u) <= slack and v >= -slack and w >= -slack


def certify_exp_primal(v, p):
    mp = _mp(EXP_DPS)
    z = [mp.mpf(float(a)) for a in v]
    q = [a - b for a, b in zip(p, z)]
    scale = max(mp.mpf(1), mp.sqrt(mp.fsum(a * a for a in z)))
    slack = mp.mpf(CERT) * scale
    assert _in_exp_primal(mp, p, slack), (tuple(v), "p outside the cone")
    assert _in_exp_dual(mp, q, slack), (tuple(v), "p - z outside the dual cone")
    assert abs(mp.fsum(a * b for a, b in zip(p, q))) <= slack * scale, (tuple(v), "<p, p - z> != 0")


def exp_record(op, x, oracle):
    """the certified reference of P_K(x) (op 'P') or of P_K*(x) = x + P_K(-x) (op 'D'), rounded to fp64"""
    mp = _mp(EXP_DPS)
    v = np.asarray(x, dtype=np.float64) if op == "P" else -np.asarray(x, dtype=np.float64)
    p = reference_exp_primal(v, oracle)
    certify_exp_primal(v, p)
    if op == "D":
        p = [mp.mpf(float(a)) + b for a, b in zip(x, p)]
    return np.array([float(a) for a in p])


# ---------------------------------------------------------------------------------------------- exponential-cone triples

RATIO = 10.0
HAND = [                                                             # (triple in the terms of exp_project's input, what it is)
    ((0.5, 1.0, 3.0), "inside with margin"),
    ((-2.0, 0.5, 1.0), "inside with margin"),
    ((1.0, -0.5, -2.0), "polar with margin"),                        # r e^(s/r) = 0.61 <= 2 e
    ((2.0, 1.0, -3.0), "polar with margin"),                         # 2 e^0.5 = 3.30 <= 3 e
    ((-1.0, -2.0, 3.0), "face, t > 0"),
    ((-1.0, -2.0, -3.0), "face, t < 0"),
    ((-0.25, -8.0, 0.0), "face, t = 0"),
    ((0.0, 0.0, 0.0), "origin"),
    ((-1.0, 0.0, 2.0), "s = 0, r <= 0 <= t"),
    ((0.0, 0.0, 2.0), "s = 0, r = 0"),
    ((-1.0, 0.0, 0.0), "s = 0, t = 0"),
]
KNOWN_LOST = [(-8.57, 0.067, -8.48), (-774.3, 12.71, -162.5)]        # the algorithm loses these projections (cone_certificates.py)


def _ratio_ok(v):
    a, b = abs(float(v[0])), abs(float(v[1]))
    return a <= RATIO * b and b <= RATIO * a


def _surface_points():
    """points of the surface s e^(r/s) = t, moved 1e-9 relative to either side along t"""
    out = []
    for r, s in ((0.3, 1.0), (-1.2, 0.7), (2.0, 1.5), (-0.4, 3.0)):
        t = s * math.exp(r / s)
        out.append(((r, s, t * (1.0 + 1e-9)), "surface + 1e-9 (inside)"))
        out.append(((r, s, t * (1.0 - 1e-9)), "surface - 1e-9 (outside)"))
    return out


def exp_triples(op):
    """-> [(x, class, note)] for the operation op ('P': P_K(x), 'D': P_K*(x) = x + P_K(-x)); the class is that of exp_project's input (x or -x):
    'hand' (closed-form branches with margin), 'benign', 'ill'"""
    sign = 1.0 if op == "P" else -1.0
    out = [(sign * np.array(v), "hand", note) for v, note in HAND]
    # beside the surface: inside is a closed-form branch; outside the dual variable rho is ~1e-9, 1/rho^2 multiplies rounding by 1e18 and the Newton solve ends
    # on noise -- the restatement is off by up to 4e-8 max(1, ||z||) there (more than the input's own distance from the cone; measured by the CPU test,
    # profiles/cone_edges_allowance.txt), so these belong with the ill-conditioned triples
    out += [(sign * np.array(v), "hand" if "inside" in note else "ill", note) for v, note in _surface_points()]
    rng = np.random.default_rng([21, "PD".index(op)])
    n = 0
    while n < 60:
        v = rng.standard_normal(3) * 10.0 ** rng.uniform(-1.5, 1.5)
        if _ratio_ok(v):
            out.append((sign * v, "benign", "seeded"))
            n += 1
    for v in KNOWN_LOST:
        out.append((sign * np.array(v), "ill", "known loss"))
    for k in range(58):
        v = rng.standard_normal(3) * 10.0 ** rng.uniform(-1.5, 1.5)
        ratio = 10.0 ** rng.uniform(1.05, 3.0)
        if k % 2:
            v[1] = math.copysign(abs(v[0]) / ratio, v[1])
        else:
            v[0] = math.copysign(abs(v[1]) / ratio, v[0])
        out.append((sign * v, "ill", "seeded"))
    return out


# ---------------------------------------------------------------------------------------------- the cases, with the fixture's references

def soc_keys():
    """the finite SOC / rotated SOC cases in the fixture's order"""
    return [(kind, length, name) for kind in KINDS for length in LENGTHS[kind] for name in NAMES[kind] if name not in _NONFINITE]


def _stored(kind, length):
    return length if length <= LONG else _head(kind) + 2


class Fixture:
    def __init__(self, path=FIXTURE):
        with np.load(path) as f:
            self.soc, self.exp = f["soc_ref"], {"P": f["exp_ref_P"], "D": f["exp_ref_D"]}
            self.exp_allowance = float(f["exp_allowance_benign"])
        self.where, pos = {}, 0
        for key in soc_keys():
            self.where[key] = (pos, _stored(key[0], key[1]))
            pos += self.where[key][1]
        assert pos == self.soc.size, "cone_edges.npz does not match the case list: run tests/golden/make_cone_edges.py"

    def soc_ref(self, kind, length, name):
        pos, n = self.where[(kind, length, name)]
        return self.soc[pos:pos + n]


_fixture = None


def fixture():
    global _fixture
    if _fixture is None:
        _fixture = Fixture()
    return _fixture


class Case:
    """One SOC or rotated SOC cone input with its reference (None: a NaN / Inf case, compared with the oracle's pattern)."""
    _cache = {}

    def __init__(self, kind, length, name):
        self.kind, self.length, self.name = kind, length, name
        self.x = soc_input(kind, length, name)
        self.finite = name not in _NONFINITE
        self.exact = name in EXACT
        self.ref = self.tol = None
        if self.finite:
            head = _head(kind)
            stored = fixture().soc_ref(kind, length, name)
            if length <= LONG:
                self.ref = stored.copy()
            else:
                hi, lo = np.longdouble(stored[head]), np.longdouble(stored[head + 1])
                tail = self.x[head:].astype(np.longdouble)
                self.ref = np.concatenate([stored[:head], (hi * tail + lo * tail).astype(np.float64)])
            v = self.x.copy()
            if kind == "SOCRotated":
                v[0], v[1] = (self.x[0] + self.x[1]) / math.sqrt(2.0), (self.x[0] - self.x[1]) / math.sqrt(2.0)
            self.tol = soc_tol(length, v[0], math.sqrt(math.fsum(v[1:] ** 2)))

    @classmethod
    def get(cls, kind, length, name):
        key = (kind, length, name)
        if key not in cls._cache:
            cls._cache[key] = cls(kind, length, name)
        return cls._cache[key]

    def label(self):
        return "%s(%d) %s" % (self.kind, self.length, self.name)

    def check(self, y, scale=0, what="", dual=False):
        """y = P(2^scale x) against 2^scale x the reference: per element within the tolerance; the same bits where the definition gives them: zero, or the
        input itself.  (A rotated cone's two head entries pass through both rotations where the projection is the identity -- P(x) = x on the primal copy,
        P(-x) = -x on the Moreau copy x + P(-x) -- and are held to the tolerance there.)  -> worst error / tolerance"""
        ratio = self.error_ratio(y, scale)
        assert ratio <= 1.0, (what, self.label(), scale, "error / tolerance", ratio, "tolerance", math.ldexp(self.tol, scale))
        if self.exact:
            head = _head(self.kind) if self.kind == "SOCRotated" else 0
            if not self.ref.any():
                lo = head if dual else 0
                assert not y[lo:].any(), (what, self.label(), "not exactly zero")
            elif np.array_equal(self.ref[head:], self.x[head:]):
                lo = 0 if dual else head
                assert np.array_equal(y[lo:], np.ldexp(self.x[lo:], scale)), (what, self.label(), "not bit-identical to the input")
            else:
                raise AssertionError((self.label(), "an exact case whose reference is neither zero nor the input"))
        return ratio

    def error_ratio(self, y, scale=0):
        """worst |y - 2^scale reference| over the tolerance (0 for an exact zero against a zero tolerance, inf for anything not finite)"""
        if not np.isfinite(y).all():
            return math.inf
        err, tol = float(np.abs(y - np.ldexp(self.ref, scale)).max()), math.ldexp(self.tol, scale)
        return 0.0 if err == 0.0 else (err / tol if tol > 0.0 else math.inf)

    def check_pattern(self, y, y_oracle, what=""):
        """a NaN / Inf input: the same NaN and Inf pattern as the oracle's, and its finite entries within the tolerance of the oracle's"""
        assert np.array_equal(np.isnan(y), np.isnan(y_oracle)), (what, self.label(), "NaN pattern")
        inf = np.isinf(y_oracle)
        assert np.array_equal(np.isinf(y), inf) and np.array_equal(y[inf], y_oracle[inf]), (what, self.label(), "Inf pattern")
        fin = np.isfinite(y_oracle)
        if fin.any():
            xf = self.x[np.isfinite(self.x)]
            assert np.abs(y[fin] - y_oracle[fin]).max() <= soc_tol(self.length, 0.0, math.sqrt(math.fsum(xf * xf))), (what, self.label())


class ExpCase:
    """One triple for P_K (op 'P') or P_K* (op 'D')."""

    def __init__(self, op, index, x, cls, note):
        self.op, self.index, self.x, self.cls, self.note = op, index, np.ascontiguousarray(x, dtype=np.float64), cls, note
        self.ref = fixture().exp[op][index]
        self.scale = max(1.0, float(np.linalg.norm(self.x)))

    def label(self):
        return "Exp %s #%d %s (%s) %r" % (self.op, self.index, self.cls, self.note, tuple(self.x))

    def closed_form(self, y_oracle):
        """the oracle answered from a closed-form branch: the input, zero or the face formula (for op D: x + that of -x)"""
        x = self.x
        v = x if self.op == "P" else -x
        for p in (v, np.zeros(3), np.array([v[0], max(v[1], 0.0), max(v[2], 0.0)])):
            if np.array_equal(y_oracle, p if self.op == "P" else x + p):
                return True
        return False

    def check(self, y, y_oracle, what=""):
        """hand: the oracle's bits, which are the exact answer.  benign: the certified reference within the measured allowance (and the oracle's bits
        in a closed-form branch).  ill: the oracle's restatement within 1e-9 max(1, ||z||), its bits in a closed-form branch.  -> error / bound"""
        closed = self.closed_form(y_oracle)
        if closed or self.cls == "hand":
            assert np.array_equal(y, y_oracle), (what, self.label(), "closed-form branch: not the oracle's bits", tuple(y), tuple(y_oracle))
        if self.cls == "hand":
            assert np.array_equal(y, self.ref), (what, self.label(), "not the exact answer")
            return 0.0
        ratio = self.error_ratio(y, y_oracle)
        assert ratio <= 1.0, (what, self.label(), "error / bound", ratio)
        return ratio

    def error_ratio(self, y, y_oracle):
        if self.cls == "ill":
            return float(np.linalg.norm(y - y_oracle)) / (1e-9 * self.scale)
        return float(np.abs(y - self.ref).max()) / (fixture().exp_allowance * self.scale)


_exp_cache = {}


def exp_cases(op):
    if op not in _exp_cache:
        _exp_cache[op] = [ExpCase(op, i, x, cls, note) for i, (x, cls, note) in enumerate(exp_triples(op))]
    return _exp_cache[op]


# ---------------------------------------------------------------------------------------------- the device handles' layouts

def k1_cones(extra_soc, n_exp_primal):
    """every SOC and rotated SOC length between two Free(3) guard blocks, then the exponential cones"""
    K1 = [("SOC", 5)] if extra_soc else []
    for kind in KINDS:
        for length in LENGTHS[kind]:
            if kind == "SOC" and length in (4, 5):
                continue
            K1 += [("Free", 3), (kind, length)]
    return K1 + [("Free", 3)] + [("ExpPrimal", 3)] * n_exp_primal + [("ExpDual", 3)] * 2


K2_CONES = [("SOC", 4), ("SOCRotated", 3), ("ExpDual", 3), ("ExpPrimal", 3), ("Free", 1)]
# A: 21 cones for the SOC kernel (one past a multiple of four) and 33 for the Exp kernel (one past a multiple of 32); B: 20 and 32; C: one cone with no tail
HANDLES = {"A": (k1_cones(True, 29), K2_CONES), "B": (k1_cones(False, 28), K2_CONES), "C": ([("SOCRotated", 2)], [("Free", 1)])}


class Slot:
    def __init__(self, kind, length, dual, at):
        self.kind, self.length, self.dual, self.at = kind, length, dual, at
        if kind.startswith("Exp"):
            self.op = "P" if (kind == "ExpPrimal") != dual else "D"      # the dual copy of P_K is P_K* and the other way round


class Layout:
    """where every cone copy sits: the stacked iterate [x(n) -> K2; y(m) -> K1*; tau; r(n) -> K2*; s(m) -> K1; kappa] of an HSDE handle (cones.jl:122-142),
    or the K1 list alone (a Feasibility ConeProduct: primal copies only)"""

    def __init__(self, K1, K2=None):
        self.K1, self.K2, self.hsde = K1, K2, K2 is not None
        self.m = sum(l for _, l in K1)
        self.n = sum(l for _, l in K2) if self.hsde else 0
        self.l = self.n + self.m + 1
        self.N = 2 * self.l if self.hsde else self.m
        self.slots = []
        if self.hsde:
            self._add(K2, 0, False)
            self._add(K1, self.n, True)
            self._add(K2, self.l, True)
            self._add(K1, self.l + self.n, False)
        else:
            self._add(K1, 0, False)

    def _add(self, cones, at, dual):
        for kind, length in cones:
            self.slots.append(Slot(kind, length, dual, at))
            at += length

    def fill(self, rnd, scale=0, exp=True):
        """the input of round `rnd`: SOC / rotated SOC copies take the rnd-th input name (dual copies the next one), scaled by 2^scale; exponential copies
        the next triples of their operation (zero with exp=False); guard blocks, tau and kappa Gaussians.  -> (z, [(slot, case)])"""
        z = np.random.default_rng([22, rnd]).standard_normal(self.N)
        taken, used = {"P": 0, "D": 0}, []
        per_round = {op: sum(1 for s in self.slots if getattr(s, "op", None) == op) for op in "PD"}
        for s in self.slots:
            seg = slice(s.at, s.at + s.length)
            if s.kind in KINDS:
                names = NAMES[s.kind]
                case = Case.get(s.kind, s.length, names[(rnd + (1 if s.dual else 0)) % len(names)])
                z[seg] = np.ldexp(case.x, scale)
                used.append((s, case))
            elif s.kind.startswith("Exp"):
                cases = exp_cases(s.op)
                case = cases[(rnd * per_round[s.op] + taken[s.op]) % len(cases)]
                taken[s.op] += 1
                z[seg] = case.x if exp else 0.0
                if exp:
                    used.append((s, case))
        return z, used

    def rounds(self):
        """enough rounds for every name on both copies and every triple"""
        need = max(len(NAMES[k]) for k in KINDS) + 1
        for op in "PD":
            per = sum(1 for s in self.slots if getattr(s, "op", None) == op)
            if per:
                need = max(need, -(-len(exp_triples(op)) // per))
        return need

    def check_guards(self, z, y, what=""):
        """Free blocks: the primal copy is the input's bits, the dual copy (the origin, the dual of Free) exactly zero -- no kernel wrote outside its cone"""
        for s in self.slots:
            if s.kind == "Free":
                seg = slice(s.at, s.at + s.length)
                assert np.array_equal(y[seg], np.zeros(s.length) if s.dual else z[seg]), (what, "guard block at %d overwritten" % s.at)


# ---------------------------------------------------------------------------------------------- what the fixture holds

def exp_oracle(op, x, oracle):
    y = np.empty(3)
    (oracle.prox_exp_primal if op == "P" else oracle.prox_exp_dual)(y, np.asarray(x, dtype=np.float64))
    return y


def compute_fixture(oracle, full=None):
    """every reference, certified, and the Exp allowances: 4 x the worst error of the oracle's restatement against the certified reference in the class,
    relative to max(1, ||z||) (the factor covers the device's log and exp differing from the host's by an ulp, which 1/rho^2 amplifies)"""
    out = {"soc_ref": np.concatenate([soc_record(*key, full=full) for key in soc_keys()])}
    worst = {"benign": 0.0}
    for op in "PD":
        triples = exp_triples(op)
        out["exp_ref_" + op] = np.array([exp_record(op, x, oracle) for x, _, _ in triples])
        for (x, cls, _), ref in zip(triples, out["exp_ref_" + op]):
            if cls in worst:
                err = float(np.abs(exp_oracle(op, x, oracle) - ref).max()) / max(1.0, float(np.linalg.norm(x)))
                worst[cls] = max(worst[cls], err)
    for cls, w in worst.items():
        out["exp_allowance_" + cls] = np.float64(4.0 * w)
    return out
