"""The PSD cases of psd_cases.py on the CPU: the long-double references are recomputed with mpmath at 50 digits (every case up to order 33, two cases each at
orders 64, 65 and 129) and the Householder products are checked for orthogonality; the oracle's restatement (prox_psd_scaled: LAPACK in double) is run on
every finite case and must stay within a quarter of the derived tolerance, which in turn must not be looser than today's whole-vector bound; and Case.check
must reject the mistakes it exists to catch.

    python tests/test_psd_cases_cpu.py        prints the CPU part of profiles/psd_edges_allowance.txt
"""
import math

import numpy as np

import psd_cases as pc

MP_ALL_UP_TO = 33
MP_LARGE = {64: ["gauss100", "decades"], 65: ["pairs", "clusters"], 129: ["gauss100", "one_large"]}
AGREE = 1e-17


def _oracle():
    import fos_oracle
    return fos_oracle


def _mp():
    import mpmath
    mpmath.mp.dps = 50
    return mpmath.mp


def _to_mp(a):
    """a double or long-double array as exact mpf objects"""
    mp = _mp()
    hi = np.asarray(a, dtype=np.float64)
    lo = (np.asarray(a, dtype=pc.LD) - hi).astype(np.float64)
    out = np.empty(hi.shape, dtype=object)
    for idx in np.ndindex(hi.shape):
        out[idx] = mp.mpf(float(hi[idx])) + mp.mpf(float(lo[idx]))
    return out


def mp_reference(k, name):
    """(svec(M), svec(P)) of a spectrum case with mpmath: the same reflectors and eigenvalues, nothing else shared with psd_cases.Case"""
    mp = _mp()
    Q = _to_mp(np.eye(k))
    for v in _to_mp(pc.reflectors(k, name)):
        Q = Q - np.outer(Q.dot(v), (mp.mpf(2) / v.dot(v)) * v)
    w = _to_mp(pc.spectrum(k, name))
    wp = np.array([max(a, mp.mpf(0)) for a in w], dtype=object)
    r2 = mp.sqrt(2)
    xs, ps = [], []
    for j in range(k):                                             # the lower triangle only
        rows = Q[j:]
        for out, lam in ((xs, w), (ps, wp)):
            col = rows.dot(lam * Q[j])
            col[1:] = col[1:] * r2
            out.extend(col)
    return np.array(xs, dtype=object), np.array(ps, dtype=object)


def mp_cases():
    keys = [(k, name) for k in pc.ORDERS if k <= MP_ALL_UP_TO for name in pc.SPECTRA]
    return keys + [(k, name) for k, names in MP_LARGE.items() for name in names]


def test_long_double_is_extended():
    pc.require_long_double()


def test_householder_products_are_orthogonal():
    worst = orthogonality()
    assert max(worst.values()) <= 1e-18, worst


def orthogonality():
    """max |Q'Q - I| per order, k reflectors each, over two seeds"""
    worst = {}
    for k in pc.ORDERS:
        for name in ("gauss100", "decades"):
            Q = pc.householder_q(pc.reflectors(k, name))
            worst[k] = max(worst.get(k, 0.0), float(np.abs(Q.T @ Q - np.eye(k, dtype=pc.LD)).max()))
    return worst


_agreement = {}


def agreement():
    """worst |long double - mpmath| / ||.||_2 of x and p_ref per certified case; x also within half an ulp of the mpmath value entry by entry"""
    if not _agreement:
        for k, name in mp_cases():
            case = pc.Case.get(k, name)
            xs, ps = mp_reference(k, name)
            norm = max(float(_mp().sqrt(sum(a * a for a in xs))), 1e-300)
            dp = max(abs(float(a - b)) for a, b in zip(_to_mp(case.p_ref), ps))
            dx = max(abs(float(a - b)) - 2.0 ** -53 * abs(float(b)) for a, b in zip(_to_mp(case.x), xs))
            _agreement[(k, name)] = (dp / norm, dx / norm)
    return _agreement


def test_references_agree_with_mpmath():
    for key, (dp, dx) in agreement().items():
        assert dp <= AGREE and dx <= AGREE, (key, dp, dx)


def test_plain_cases_are_projections():
    """the cases without Q: P is symmetric PSD, M - P is NSD and <P, M - P> = 0 in long double -- the closed forms certify themselves"""
    for k in pc.ORDERS:
        for name in pc.PLAIN:
            M, P = pc.plain_case(k, name)
            N = (P - M).astype(np.float64)
            scale = max(1.0, float(np.abs(M).max()))
            assert np.linalg.eigvalsh(P.astype(np.float64)).min() >= -1e-13 * scale * k, (k, name)
            assert np.linalg.eigvalsh(N).min() >= -1e-13 * scale * k, (k, name)
            assert abs(float(np.sum(P * (P - M)))) <= 1e-17 * scale * scale * k * k, (k, name)


def oracle_psd(x, dual=False):
    orc = _oracle()
    y = np.empty_like(x)
    (orc.cone_prox_dual if dual else orc.cone_prox)(orc.CONE_SDP, y, x)
    return y


_ratios = {}


def oracle_ratios():
    """worst error / tolerance of the oracle's restatement per order, primal and Moreau copy, every case, with the homogeneity scales; and the worst
    tolerance / today's bound.  The exact identities are not asked of LAPACK."""
    if not _ratios:
        for k in pc.ORDERS:
            worst = loose = units = 0.0
            for name in pc.NAMES:
                case = pc.Case.get(k, name)
                for dual in (False, True):
                    worst = max(worst, case.check(oracle_psd(case.x, dual), dual=dual, what="oracle", exact=False))
                    if case.norm > 0.0:
                        units = max(units, float(np.abs(oracle_psd(case.x, dual) - case.p_ref).max()) / (pc.U52 * case.norm))
                if name in pc.HOMOGENEITY_BASE:
                    for s in pc.HOMOGENEITY_SCALES:
                        worst = max(worst, case.check(oracle_psd(np.ldexp(case.x, s)), scale=s, what="oracle 2^%d" % s, exact=False))
                loose = max(loose, case.tol(refined=k == 64) / (pc.OLD_BOUND * max(1.0, case.norm)))
            _ratios[k] = (worst, units, loose)
    return _ratios


def test_oracle_within_a_quarter_of_the_tolerance():
    for k, (worst, _, _) in oracle_ratios().items():
        assert worst <= 0.25, (k, worst)


def test_tolerance_is_no_looser_than_the_whole_vector_bound():
    """per matrix and per entry against 5e-13 max(1, ||x||) on the norm of the whole iterate; the accepted-refinement term included at order 64"""
    for k, (_, _, loose) in oracle_ratios().items():
        assert loose <= 1.0, (k, loose)


# ---------------------------------------------------------------------------------------------- sensitivity: what the check must reject

def psd_fp64(x, diag_scale=math.sqrt(2.0), clamp_at_shift=False):
    """the kernels' formulation in fp64 with the mistakes of the mutants switched on: eigenvalues of the shifted matrix, kept where they exceed the shift"""
    k = _oracle().psd_dim(x.shape[0])
    dpos = np.cumsum([0] + [k - j for j in range(k - 1)])
    w = x.copy()
    w[dpos] *= diag_scale
    M = _oracle().svec_to_mat(w, k)
    sigma = 1.001 * np.linalg.norm(M)
    lam, V = np.linalg.eigh(M + sigma * np.eye(k))
    keep = np.where(lam > sigma * (1.0 + (1e-7 if clamp_at_shift else 0.0)), lam - sigma, 0.0)   # (the mutant keeps a column only 1e-7 above the shift)
    y = np.empty_like(x)
    _oracle().mat_to_svec((V * keep) @ V.T, y)
    y[dpos] /= diag_scale
    return y


def mutant_factors():
    """worst error / tolerance of every deliberately wrong answer over the cases it is run on (orders up to 33, where everything is quick)"""
    cases = [pc.Case.get(k, name) for k in pc.ORDERS if 2 <= k <= 33 for name in pc.NAMES if name != "zero"]
    by = lambda fn, sel=cases: max(c.error_ratio(fn(c)) for c in sel)

    def shifted_column(c):                                          # a packed index off by one column: column j read where column j + 1 starts
        y = oracle_psd(c.x)
        return np.concatenate([y[c.k:], y[:c.k]])

    def neighbour(c):                                               # the answer of the next case of the same order: one cone written into another
        other = pc.Case.get(c.k, pc.NAMES[(pc.NAMES.index(c.name) + 1) % len(pc.NAMES)])
        return oracle_psd(other.x)

    def one_entry(c):
        y = oracle_psd(c.x)
        y[len(y) // 2] += 4.0 * c.tol()
        return y

    small_pos = [c for c in cases if c.name in ("decades", "one_large")]        # a positive eigenvalue below 1e-7 ||M||_F among larger ones
    return {
        "unmutated fp64 restatement (shifted form)": by(lambda c: psd_fp64(c.x)),
        "diagonal not scaled by sqrt 2": by(lambda c: psd_fp64(c.x, diag_scale=1.0), [c for c in cases if c.name in pc.SPECTRA]),
        "eigenvalues clamped just above the shift": by(lambda c: psd_fp64(c.x, clamp_at_shift=True), small_pos),
        "dual copy without + x": by(lambda c: oracle_psd(-c.x), [c for c in cases if not c.positive and not c.negative]),
        "packed index off by one column": by(shifted_column),
        "a cone's answer written into its neighbour": by(neighbour),
        "one entry off by 4 x the tolerance": min(c.error_ratio(one_entry(c)) for c in cases),
    }


def test_the_check_rejects_each_mutant():
    f = mutant_factors()
    assert f.pop("unmutated fp64 restatement (shifted form)") <= 0.25
    assert len(f) >= 6
    for name, factor in f.items():
        assert factor > 1.0, (name, factor)


def report():
    lines = ["== the derivation's constants (tests/psd_cases.py) ==",
             "tolerance per matrix: (a + b k) 2^-52 ||x_cone||_2 on the worst entry",
             "  Jacobi kernels, order <= 64:   a = %g, b = %g;  a matrix accepted by the refinement kernel: + %.0f (its header's 1e-13 ||M||)" % (pc.JACOBI_AB + (pc.REFINE_CLAIM,)),
             "  sign iteration, order > 64:    a = %g, b = %g;  + sqrt(2) x the largest eigenvalue below %g ||M||_F" % (pc.SIGN_AB + (pc.SIGN_UNRESOLVED,)),
             "", "== CPU: references and the oracle's LAPACK restatement (tests/test_psd_cases_cpu.py) =="]
    orth = orthogonality()
    lines.append("max |Q'Q - I| over the orders, k reflectors each: %.2e (asserted: 1e-18)" % max(orth.values()))
    agree = agreement()
    lines.append("long double against mpmath at 50 digits, %d cases: p_ref %.2e, x beyond half an ulp %.2e, relative to ||x|| (asserted: %g)"
                 % (len(agree), max(a for a, _ in agree.values()), max(0.0, max(b for _, b in agree.values())), AGREE))
    lines.append("order   tolerance    oracle error   oracle / tolerance   tolerance / 5e-13 max(1, ||x||)")
    lines.append("        (2^-52 ||x||) (2^-52 ||x||)  (asserted: 0.25)     (asserted: 1; order 64 with the refinement term)")
    for k, (worst, units, loose) in oracle_ratios().items():
        lines.append("%5d   %9.1f    %9.2f      %.4f               %.4f" % (k, pc.tolerance_units(k), units, worst, loose))
    for cls in ("Jacobi kernels, order <= 64", "sign iteration, order > 64"):
        sel = [v for k, v in oracle_ratios().items() if pc.order_class(k) == cls]
        lines.append("worst of the class %-30s oracle / tolerance %.4f, tolerance / old bound %.4f" % (cls + ":", max(v[0] for v in sel), max(v[2] for v in sel)))
    lines += ["", "mutants: worst error / tolerance over the cases (each must exceed 1; the last one: the smallest over the cases)"]
    for name, factor in mutant_factors().items():
        lines.append("  %-45s %.3g" % (name, factor))
    return lines


if __name__ == "__main__":
    import sys
    from pathlib import Path
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "oracle"))
    print("\n".join(report()))
