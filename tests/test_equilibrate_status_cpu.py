"""
The reference and the allowance of the equilibrated status check (tests/equilibrate_status.py) before a GPU is involved, on every case of
test_gpu_equilibrate_formats.py: the fp64 restatement of the check lies within 1 x its allowance (it is one fp64 evaluation of the formulas), its
decision is the reference's, and the reference is farther from each threshold than the allowance -- so the device test can assert the decision
everywhere.  One test keeps the formula the kernel had before: it breaks the allowance of ||A x + s|| and ||A'y|| at tau = 1e6, and gives Inf where the
reference gives NaN at tau = 0.
"""
import numpy as np
import pytest
import scipy.sparse as sp

import equilibrate_cases as ec
import equilibrate_status as es
import status_cases as cases
import status_reference as sref


def _operators(pkg):
    """(name, A, b, c, certificates?) of every operator of the device test"""
    for name, A in cases.row_block_shapes() + cases.window_shapes():
        A = sp.csc_matrix(A)
        b, c = cases.vectors_for(name, A)
        yield name, A, b, c, name in es.CERTIFICATE_OPERATORS
    for m, n in es.EDGE_SHAPES:
        yield es.edge_problem(pkg, m, n) + (False,)


def _hold(label, b, c, eq, A, z, want, worst):
    """restatement within 1 x allowance, decision the reference's and clear of every threshold -> nothing returned, everything asserted"""
    vals, allow = es.reference(A, b, c, z)
    for eps in cases.EPS:
        got = es.restate(b, c, eq, z, eps)
        rat = sref.ratios(got, vals, allow)
        for k, v in rat.items():
            worst[k] = max(worst.get(k, 0.0), v)
        assert max(rat.values()) <= 1.0, (label, eps, rat)
        assert sref.margin(vals, eps) > 2 * sref.relative_allowance(vals, allow, eps), (label, eps)
        assert got["status"] == sref.decide(vals, eps), (label, eps)
        if want is not None:
            assert got["status"] == want and sref.margin(vals, eps) >= 1e-3, (label, eps)


@pytest.mark.parametrize("passes", es.PASSES)
def test_restatement_within_allowance_on_every_device_case(pkg, passes):
    worst, seen = {}, 0
    for name, A, b, c, certs in _operators(pkg):
        scaled = {}
        for label, Ap, bp, cp, z, want in es.point_sets(name, A, b, c, certs):
            key = id(Ap)
            if key not in scaled:                                     # (the operator as it stands, and its scaled problem)
                scaled[key] = pkg.host_equilibrate(Ap, bp, cp, *es.free_cones(Ap), passes)
            _hold((name, label, passes), bp, cp, scaled[key], Ap, z, want, worst)
            seen += 1
    assert seen > 150
    print("passes = %d, %d points: worst |restatement - reference| / allowance per field: %s" % (passes, seen, ", ".join("%s %.3g" % kv for kv in sorted(worst.items()))))


@pytest.mark.parametrize("name", sorted(es.CONE_VARIANTS))
def test_restatement_with_coupling_cones(pkg, name):
    """SOC and SDP blocks on both sides: D and E constant on each (the block means), the same bounds"""
    A = sp.csc_matrix(dict(cases.row_block_shapes() + cases.window_shapes())[name])
    b, c = cases.vectors_for(name, A)
    K1, K2 = es.CONE_VARIANTS[name]
    assert sum(k for _, k in K1) == A.shape[0] and sum(k for _, k in K2) == A.shape[1]
    worst, scaled = {}, {}
    for label, Ap, bp, cp, z, _ in es.point_sets(name, A, b, c):
        if id(Ap) not in scaled:
            eq = scaled[id(Ap)] = pkg.host_equilibrate(Ap, bp, cp, K1, K2, 10)
            assert np.all(eq["D"][0:K1[0][1]] == eq["D"][0]) and len(np.unique(eq["D"])) > 3
        _hold((name, label), bp, cp, scaled[id(Ap)], Ap, z, None, worst)
    print("%s with coupling cones: %s" % (name, ", ".join("%s %.3g" % kv for kv in sorted(worst.items()))))


def test_restatement_with_the_numpy_factors(pkg):
    """the same restatement fed by equilibrate_cases.equilibrate_ref instead of the library: whatever the factors, the bounds hold"""
    name, A = cases.row_block_shapes()[1]
    A = sp.csc_matrix(A)
    b, c = cases.vectors_for(name, A)
    eq = ec.equilibrate_ref(A, b, c, *es.free_cones(A), 10)
    for label, z in cases.points(name, A, b, c):
        _hold((name, label), b, c, eq, A, z, None, {})


def test_the_earlier_formula_breaks_the_allowance(pkg):
    """w = Q^ [x^; y^; tau] carries c^ tau and b^ tau; subtracting them again leaves ||A x + s|| and ||A'y|| an error in proportion to tau |b|, tau |c|, which
    their allowance does not contain: at tau = 1e6 the earlier formula is far outside, the present one within 1 x.  At tau = 0 the earlier p and d are a
    finite norm over 0 = Inf where the reference has NaN."""
    broken, worst_old = 0, 0.0
    for name, A, b, c, _ in _operators(pkg):
        if name not in ("random-structured-11", "tiny", "sparse-lp-24x40"):            # few entries per row: small allowances
            continue
        eq = pkg.host_equilibrate(A, b, c, *es.free_cones(A), 10)
        pts = dict(cases.points(name, A, b, c))
        z = pts["unit tau=1e+06"]
        vals, allow = es.reference(A, b, c, z)
        old, new = sref.ratios(es.restate(b, c, eq, z, fixed=False), vals, allow), sref.ratios(es.restate(b, c, eq, z), vals, allow)
        print("%s tau = 1e6: earlier formula nAxs %.3g nATy %.3g x allowance; present nAxs %.3g nATy %.3g" % (name, old["nAxs"], old["nATy"], new["nAxs"], new["nATy"]))
        assert old["nAxs"] > 2.0 and old["nATy"] > 2.0, old                                    # (outside even the device's 2 x)
        worst_old = max(worst_old, old["nAxs"], old["nATy"])
        assert max(new.values()) <= 1.0, new
        assert max(v for k, v in old.items() if k not in ("nAxs", "nATy")) <= 1.0, old         # (the other fields never lost anything)
        z = pts["tau=0"]
        vals, allow = es.reference(A, b, c, z)
        old, new = es.restate(b, c, eq, z, fixed=False), es.restate(b, c, eq, z)
        assert np.isnan(float(vals["p"])) and np.isnan(float(vals["d"]))
        assert np.isinf(old["p"]) and np.isinf(old["d"]) and np.isnan(new["p"]) and np.isnan(new["d"])
        assert max(sref.ratios(new, vals, allow).values()) <= 1.0
        broken += 1
    assert broken == 3 and worst_old > 1000


def test_allowance_has_no_tau_b_term():
    """||A x + s|| and ||A'y|| and their allowances do not move when b, c change (tau fixed): neither contains b tau or c tau"""
    rng = np.random.default_rng(3)
    A = sp.random(30, 20, density=0.3, format="csc", random_state=rng, data_rvs=rng.standard_normal)
    z = rng.standard_normal(2 * 51)
    z[50] = 1e6
    v1, a1 = es.reference(A, rng.standard_normal(30), rng.standard_normal(20), z)
    v2, a2 = es.reference(A, 1e9 * rng.standard_normal(30), 1e9 * rng.standard_normal(20), z)
    for k in ("nAxs", "nATy"):
        assert v1[k] == v2[k] and a1[k] == a2[k]
        assert 0 < float(a1[k]) < 1e-12 * float(v1[k])
