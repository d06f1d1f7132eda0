"""
The operators and starts on which the CG kernels are compared with tests/cg_reference.py: shared by the CPU test of the reference itself
(test_cg_reference_cpu.py) and the device test (test_gpu_cg_formats.py).  Everything here is chosen and screened on the CPU, from the
reference alone; no device result enters.

Operators: exactly those of status_cases.row_block_shapes() and status_cases.window_shapes(), with b, c of status_cases.vectors_for.
Plain CG on the indefinite KKT system amplifies rounding on unit-scale random inputs (1e-16 after one iteration, 1e-12 after ten); that is
a property of the inputs.  The TAMED starts scale A, b, c by a power of two so that ||[A b; c' 0]||_2 lies in (0.125, 0.25] (the
eigenvalues of M in +-[1, 1.031]) and give the start residual a second half one eighth the size of its first, so that p.Mp has no
cancellation: the residual then falls by a factor of 3 to 100 per iteration and fp64 evaluations stay within a few u max|x| of the
extended recurrence through four iterations.

    start   operator   x0           rhs                         k
    warm    scaled     unit normal  M x0 + [g1; g2 / 8] (fp64)  1 .. 4
    cold    scaled     0            [g1; g2 / 8]                1 .. 4
    raw     as it is   unit normal  unit normal                 1

Screened per case (a seed that fails takes the next one, nothing is widened): on the tamed starts decisive_tol exists for k = 2 and 3;
on every start the k = 1 allowance is below 1e-12 max|alpha_0 r_0|, so a relative error of 1e-12 in the first step length cannot pass.
The allowance table (allowance / max|x_k| per case and k) is cached here: table().
"""
from functools import lru_cache

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import cg_reference as cref
import fos_oracle as orc
import status_cases as scases

STARTS = ("warm", "cold", "raw")
TAMED = ("warm", "cold")
MAX_SEEDS = 16
TABLE = {}            # (operator, start) -> {k: allowance / max|x_k|}, filled as cases are built


@lru_cache(maxsize=None)
def operators():
    """{name: (A, b, c, window?)} of every operator, in the order of the two shape lists"""
    out = {}
    for windows, shapes in ((False, scases.row_block_shapes()), (True, scases.window_shapes())):
        for name, A in shapes:
            A = sp.csc_matrix(A)
            A.sort_indices()
            b, c = scases.vectors_for(name, A)
            assert name not in out
            out[name] = (A, b, c, windows)
    return out


def row_names():
    return [k for k, v in operators().items() if not v[3]]


def window_names():
    return [k for k, v in operators().items() if v[3]]


def sigma1(A, b, c):
    """largest singular value of [A b; c' 0] (1 for an empty operator)"""
    m, n = A.shape
    B = sp.bmat([[sp.csc_matrix(A), sp.csc_matrix(b.reshape(m, 1))], [sp.csc_matrix(c.reshape(1, n)), None]], format="csc")
    B.eliminate_zeros()
    if B.nnz == 0:
        return 1.0
    if min(B.shape) <= 64 or B.shape[0] * B.shape[1] <= 250000:
        return float(np.linalg.norm(B.toarray(), 2))
    return float(spla.svds(B, k=1, v0=np.ones(min(B.shape)), return_singular_vectors=False, tol=1e-6)[0])


@lru_cache(maxsize=None)
def scaled_operator(name):
    """(A, b, c) times 2^floor(log2(0.25 / sigma_1)): exact in fp64"""
    A, b, c, _ = operators()[name]
    f = 2.0 ** np.floor(np.log2(0.25 / sigma1(A, b, c)))
    As = sp.csc_matrix(A * f)
    As.sort_indices()
    return As, b * f, c * f


def _build(name, start, seed):
    A, b, c, _ = operators()[name]
    N = 2 * (sum(A.shape) + 1)
    rng = np.random.default_rng(scases._seed("cg", name, start, seed))
    if start == "raw":
        return cref.Case("%s/raw" % name, A, b, c, rng.standard_normal(N), rng.standard_normal(N), (1,))
    As, bs, cs = scaled_operator(name)
    g = rng.standard_normal(N)
    g[N // 2:] /= 8.0
    if start == "cold":
        return cref.Case("%s/cold" % name, As, bs, cs, np.zeros(N), g, (1, 2, 3, 4))
    x0 = rng.standard_normal(N)
    return cref.Case("%s/warm" % name, As, bs, cs, x0, cref.kkt_mul(As, bs, cs, x0, np.float64) + g, (1, 2, 3, 4))


def first_step_visible(case):
    """the k = 1 allowance is below 1e-12 |alpha_0 r_0| on at least one element"""
    ext = cref.extended(case)
    return cref.allowance(case, 1) < 1e-12 * float(np.max(np.abs(ext.alphas[0] * ext.r0)))


def screened(case, start):
    if start in TAMED and (cref.decisive_tol(case, 2) is None or cref.decisive_tol(case, 3) is None):
        return False
    return first_step_visible(case)


@lru_cache(maxsize=None)
def case(name, start):
    """the first seed's case that passes the screen, its reference and allowances computed once and kept"""
    for seed in range(MAX_SEEDS):
        cs = _build(name, start, seed)
        if screened(cs, start):
            cs.seed = seed
            TABLE[(name, start)] = {k: cref.relative_allowance(cs, k) for k in cs.ks}
            return cs
    raise AssertionError("no seed below %d passes the screen on %s/%s" % (MAX_SEEDS, name, start))


def table():
    """{(operator, start): {k: allowance / max|x_k|}} over every case"""
    for name in operators():
        for start in STARTS:
            case(name, start)
    return TABLE


def format_table(tab=None):
    tab = table() if tab is None else tab
    lines = ["%-24s %-5s %5s  %s" % ("operator", "start", "seed", "allowance / max|x_k|, k = 1 ..")]
    for (name, start), row in tab.items():
        lines.append("%-24s %-5s %5d  %s" % (name, start, case(name, start).seed, "  ".join("%.2e" % row[k] for k in sorted(row))))
    return "\n".join(lines)


# ---------------------------------------------------------------------------------------------- two prox_affine calls

PROX_TOLS = (0.2, 0.2 ** np.sqrt(2.0))          # affinepluslinear.jl:108-112 with decreasing accuracy: 0.2^sqrt(i), i = 1, 2
PROX_SCALES = tuple(2.0 ** e for e in range(8, -9, -1))


def _decisive_stop(rn, tol):
    """the iteration 1 .. 3 at which ||r|| <= tol stops, if every residual before it is above 1.5 tol and that one below tol / 1.5"""
    for k in range(1, len(rn)):
        if rn[k] <= tol / 1.5:
            return k
        if not rn[k] >= 1.5 * tol:
            return None
    return None


def _prox_rhs(A, b, c, x, dtype):
    """[x1 + Q'x2; 0] = [x1 - Q x2; 0]  (affinepluslinear.jl:94-95 with beta = 1, q = 0)"""
    l = x.shape[0] // 2
    x = np.asarray(x, dtype=dtype)
    return np.concatenate([x[:l] - cref.q_mul(A, b, c, x[l:], dtype), np.zeros(l, dtype)])


def _prox_inputs(name, seed):
    """[(input, iterations, extended result)] of the two calls, or None.  First input: 2^e g, the start is the input itself (:101-106), so
    the residuals are linear in the scale.  Second input: the first plus 2^e g', as consecutive outer iterations give; the start is the first
    result (:122).  Of the scales with a decisive stop the one with the wanted count is taken -- the counts 1, 2, 3 rotate over the operators
    -- else the largest."""
    As, bs, cs = scaled_operator(name)
    A = cref.Coo(As)
    N = 2 * (sum(As.shape) + 1)
    rng = np.random.default_rng(scases._seed("prox", name, seed))
    idx = list(operators()).index(name)
    want = (1 + idx % 3, 1 + (idx + 1) % 3)
    run = lambda x0, x: cref.recurrence(A, bs, cs, x0, _prox_rhs(A, bs, cs, x, cref.LD), 3, cref.LD)
    pick = lambda cands, k: next((t for t in cands if t[1] == k), cands[0]) if cands else None
    g, g2 = rng.standard_normal(N), rng.standard_normal(N)
    unit = run(np.asarray(g, dtype=cref.LD), g).rn
    first = pick([(s, _decisive_stop([s * v for v in unit], PROX_TOLS[0])) for s in PROX_SCALES
                  if _decisive_stop([s * v for v in unit], PROX_TOLS[0])], want[0])
    if first is None:
        return None
    x1 = first[0] * g
    rec = run(np.asarray(x1, dtype=cref.LD), x1)
    if _decisive_stop(rec.rn, PROX_TOLS[0]) != first[1]:
        return None
    y1 = rec.xs[first[1] - 1]
    cands = []
    for s in PROX_SCALES:
        x2 = x1 + s * g2
        rec = run(y1, x2)
        k = _decisive_stop(rec.rn, PROX_TOLS[1])
        if k is not None:
            cands.append((s, k, x2, rec.xs[k - 1]))
            if k == want[1]:
                break
        elif cands and rec.rn[1] < PROX_TOLS[1] / 1.5:
            break                                        # (smaller scales all stop at the first iteration)
    second = pick(cands, want[1])
    if second is None:
        return None
    return [(x1, first[1], y1), (second[2], second[1], second[3])]


@lru_cache(maxsize=None)
def prox_sequence(name):
    """Two consecutive prox_affine calls on the scaled operator, from the counter's first state: inputs scaled so that the extended
    recurrence stops decisively after 1 .. 3 iterations at the schedule's tolerances.  -> [(input x, iterations, extended result,
    allowance)], the allowance measured like cg_reference.allowance from fp64 evaluations of the WHOLE sequence (each starts its second
    call from its own first result, as the device does): the oracle's two recurrences, the left-to-right restatement, and a FOURTH, the
    restatement with r.r added pairwise and Ap.p left to right.  The fourth is needed here and only here: the first call starts from its
    own input, so r_0 = [0; x2 - Q x1], p.Mp = -(r_0.r_0) term by term and alpha_0 = -1 exactly.  An evaluation that adds both sums in
    ONE order returns -1 to the last bit and measures no rounding of the step length at all, whereas any evaluation that takes the two sums
    separately (the device: the start kernel's records and the sweep's records, two different trees) carries the relative difference of two
    roundings of the same sum into alpha_0 and from there into alpha_0 p, which is as large as the result."""
    As, bs, cs = scaled_operator(name)
    l = sum(As.shape) + 1
    N = 2 * l
    assert l * 2.3e-16 < PROX_TOLS[1]                       # (the tolerance floor size(A, 2) eps is not reached)
    for seed in range(MAX_SEEDS):
        out = _prox_inputs(name, seed)
        if out is None:
            continue
        dist = [0.0] * len(out)
        for variant in ("reference", "merged"):
            S = orc.AffinePlusLinear(orc.HSDEMatrixQ(As, bs, cs), np.zeros(l), np.zeros(l), 1, decreasing_accuracy=True)
            S.cg_variant = variant
            for q, (x, k, xk) in enumerate(out):
                y = np.empty(N)
                S.prox(y, x)
                assert S.getcgiter() == k, (name, variant, q, S.getcgiter(), k)
                dist[q] = max(dist[q], cref.distance(y, xk))
        for order in (True, "mixed"):
            start = None
            for q, (x, k, xk) in enumerate(out):
                x0 = x if start is None else start
                start = cref.recurrence(As, bs, cs, x0, _prox_rhs(As, bs, cs, x, np.float64), k, np.float64, sequential=order).xs[k - 1]
                dist[q] = max(dist[q], cref.distance(start, xk))
        return [(x, k, xk, cref.MARGIN * max(dq, cref.U * float(np.max(np.abs(xk))))) for (x, k, xk), dq in zip(out, dist)]
    raise AssertionError("no seed below %d gives two decisive prox_affine calls on %s" % (MAX_SEEDS, name))
