"""fos_host_equilibrate (csrc/equilibrate.cpp: the scaling fos_create3 computes, no GPU) against the numpy restatement of its recipe in
equilibrate_cases.py, its properties checked without the restatement, and its edge cases."""
import numpy as np
import pytest
import scipy.sparse as sp

import equilibrate_cases as ec

# At most 2 passes + 3 rounded operations touch an entry (a division by a rounded square root per pass, gamma, the two products of D A E; sigma / rho and
# their norms likewise for b, c), so with passes <= 50 two evaluations differ by at most ~103 * 2^-53 = 1.2e-14 relative.
RTOL = 1e-13
PASSES = 10


@pytest.fixture(scope="module")
def problems(pkg):
    w = pkg.workloads
    one = w.ConicProblem("one-by-one", sp.csc_matrix(np.array([[-3.0]])), np.array([2.0]), np.array([0.5]), [("NonNeg", 1)], [("Free", 1)])
    return {"small_mixed": w.small_mixed(), "small_mixed_bad": ec.badly_scaled(w.small_mixed(), 1), "all_kinds": ec.all_kinds(pkg),
            "small_lp": w.small_lp(), "one": one}


@pytest.fixture(scope="module")
def scaled(pkg, problems):
    """(library result, restatement) per problem, computed once"""
    return {k: (pkg.host_equilibrate(p.A, p.b, p.c, p.K1, p.K2, PASSES), ec.equilibrate_ref(p.A, p.b, p.c, p.K1, p.K2, PASSES)) for k, p in problems.items()}


NAMES = ["small_mixed", "small_mixed_bad", "all_kinds", "small_lp", "one"]


@pytest.mark.parametrize("name", NAMES)
def test_matches_the_restatement(scaled, name):
    got, ref = scaled[name]
    for key in ("D", "E", "b", "c"):
        np.testing.assert_allclose(got[key], ref[key], rtol=RTOL, atol=0, err_msg=key)
    for key in ("sigma", "rho", "gamma"):
        assert got[key] == pytest.approx(ref[key], rel=RTOL), key
    assert np.array_equal(got["A"].indptr, ref["A"].indptr) and np.array_equal(got["A"].indices, ref["A"].indices)
    np.testing.assert_allclose(got["A"].data, ref["A"].data, rtol=RTOL, atol=0)


@pytest.mark.parametrize("passes", [1, 3, 50])
def test_matches_the_restatement_at_other_pass_counts(pkg, problems, passes):
    p = problems["small_mixed_bad"]
    got, ref = pkg.host_equilibrate(p.A, p.b, p.c, p.K1, p.K2, passes), ec.equilibrate_ref(p.A, p.b, p.c, p.K1, p.K2, passes)
    for key in ("D", "E", "b", "c"):
        np.testing.assert_allclose(got[key], ref[key], rtol=RTOL, atol=0, err_msg=key)
    np.testing.assert_allclose(got["A"].data, ref["A"].data, rtol=RTOL, atol=0)


@pytest.mark.parametrize("name", NAMES)
def test_factors_are_positive_finite_and_constant_on_coupling_cones(problems, scaled, name):
    p, (got, _) = problems[name], scaled[name]
    for v, cones in ((got["D"], p.K1), (got["E"], p.K2)):
        assert np.all(np.isfinite(v)) and np.all(v > 0)
        at = 0
        for kind, length in cones:
            if kind in ec.NON_SEPARABLE:
                assert np.all(v[at:at + length] == v[at]), (kind, at)
            at += length
    for key in ("sigma", "rho", "gamma"):
        assert np.isfinite(got[key]) and got[key] > 0


@pytest.mark.parametrize("name", NAMES)
def test_scaled_problem_is_the_one_the_factors_describe(problems, scaled, name):
    """A^ = D A E, b^ = sigma D b, c^ = rho E c from the returned factors; |A^|_F^2 = min(m, n), |b^| = |c^| = 10"""
    p, (got, _) = problems[name], scaled[name]
    A = sp.csc_matrix(p.A)
    A.sort_indices()
    want = sp.csc_matrix(sp.diags(got["D"]) @ A @ sp.diags(got["E"]))
    want.sort_indices()
    np.testing.assert_allclose(got["A"].data, want.data, rtol=RTOL, atol=0)
    np.testing.assert_allclose(got["b"], got["sigma"] * got["D"] * p.b, rtol=RTOL, atol=0)
    np.testing.assert_allclose(got["c"], got["rho"] * got["E"] * p.c, rtol=RTOL, atol=0)
    assert float(np.sum(got["A"].data ** 2)) == pytest.approx(min(p.m, p.n), rel=RTOL)
    assert float(np.linalg.norm(got["b"])) == pytest.approx(10.0, rel=RTOL)
    assert float(np.linalg.norm(got["c"])) == pytest.approx(10.0, rel=RTOL)


def test_lp_rows_and_columns_are_balanced(scaled):
    """separable cones only: after 10 passes every row and column infinity-norm of D A E / gamma lies in [0.5, 1].  The restatement stays inside
    that interval on this problem (rows at 1.0000, columns in [0.9996, 1]), so the interval is kept as stated; the library is held to the same."""
    got, ref = scaled["small_lp"]
    for res in (ref, got):
        M = abs(res["A"]) / res["gamma"]
        rmax, cmax = M.max(axis=1).toarray().ravel(), M.max(axis=0).toarray().ravel()
        print("row maxima in [%.4f, %.4f], column maxima in [%.4f, %.4f]" % (rmax.min(), rmax.max(), cmax.min(), cmax.max()))
        assert rmax.min() >= 0.5 and rmax.max() <= 1.0 + 1e-12
        assert cmax.min() >= 0.5 and cmax.max() <= 1.0 + 1e-12


def test_zero_row_and_zero_column(pkg):
    rng = np.random.default_rng(3)
    A = sp.random(9, 7, density=0.5, format="lil", random_state=rng, data_rvs=rng.standard_normal)
    A[4, :] = 0
    A[:, 2] = 0
    A = sp.csc_matrix(A)
    A.eliminate_zeros()
    b, c = rng.standard_normal(9), rng.standard_normal(7)
    K1, K2 = [("NonNeg", 9)], [("Free", 7)]
    got, ref = pkg.host_equilibrate(A, b, c, K1, K2, PASSES), ec.equilibrate_ref(A, b, c, K1, K2, PASSES)
    for key in ("D", "E", "b", "c"):
        assert np.all(np.isfinite(got[key]))
        np.testing.assert_allclose(got[key], ref[key], rtol=RTOL, atol=0, err_msg=key)
    # an empty row / column counts 1 in every pass: its factor is 1 (times gamma for a row)
    assert got["D"][4] == got["gamma"] and got["E"][2] == 1.0


def test_zero_b_and_empty_matrix(pkg):
    rng = np.random.default_rng(4)
    A = sp.random(6, 5, density=0.5, format="csc", random_state=rng, data_rvs=rng.standard_normal)
    got = pkg.host_equilibrate(A, np.zeros(6), rng.standard_normal(5), [("Zero", 6)], [("NonNeg", 5)], PASSES)
    assert got["sigma"] == 1.0 and np.all(got["b"] == 0) and np.isfinite(got["rho"])
    empty = pkg.host_equilibrate(sp.csc_matrix((6, 5)), rng.standard_normal(6), np.zeros(5), [("Zero", 6)], [("NonNeg", 5)], PASSES)
    assert empty["gamma"] == 1.0 and empty["rho"] == 1.0 and empty["A"].nnz == 0
    assert np.all(empty["D"] == 1.0) and np.all(empty["E"] == 1.0)


def test_bad_arguments(pkg, problems):
    p = problems["small_lp"]
    for passes in (-1, 0, 51):
        with pytest.raises(pkg.lib.FosError) as e:
            pkg.host_equilibrate(p.A, p.b, p.c, p.K1, p.K2, passes)
        assert e.value.code == -1, passes                       # FOS_EINVAL
    with pytest.raises(pkg.lib.FosError) as e:                   # a cone table that leaves row 1 out
        pkg.host_equilibrate(p.A, p.b, p.c, [("NonNeg", range(2, p.m + 1))], p.K2, PASSES)
    assert e.value.code == -1
    with pytest.raises(pkg.lib.FosError) as e:                   # ... and one with a gap between two cones
        pkg.host_equilibrate(p.A, p.b, p.c, [("NonNeg", range(1, 5)), ("NonNeg", range(6, p.m + 1))], p.K2, PASSES)
    assert e.value.code == -1


def test_option_values(pkg):
    f = pkg.equilibrate_passes
    assert (f(False), f(None), f(0), f(True), f(7)) == (0, 0, 0, 10, 7)
    with pytest.raises(TypeError):
        f("yes")


def test_planted_points_of_the_cases_are_optimal(pkg, oracle, problems):
    """the test problems themselves: the planted (x0, y0, s0) of the badly scaled and the all-kinds problem is optimal for the ORIGINAL data, and its cone
    parts are fixed points of the oracle's projection onto K2 x K1* x R+ x K2* x K1 x R+"""
    for name in ("small_mixed_bad", "all_kinds"):
        p = problems[name]
        mo = oracle.Model(p.A, p.b, p.c, [(oracle.CONE_CODES[k], n) for k, n in p.K1], [(oracle.CONE_CODES[k], n) for k, n in p.K2])
        z = np.concatenate([p.x0, p.y0, [1.0], p.c + p.A.T @ p.y0, p.s0, [0.0]])
        assert oracle.decide_status(oracle.residuals(mo, z), 1e-8) == "Optimal", name
        out = np.empty_like(z)
        oracle.DualConeProduct(mo.K1, mo.K2).prox(out, z)
        # (the planted exponential-cone points lie on the boundary, where the oracle's projection is a root search that stops at ~1e-8)
        assert np.max(np.abs(out - z)) <= 1e-6 * np.max(np.abs(z)), name
