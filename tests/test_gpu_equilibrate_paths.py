"""
An equilibrated handle (fos_create3, equil_passes > 0) takes THE SAME STEPS as a plain handle built from host_equilibrate's scaled data, on every path a
solve can take: both start from set_iterate(None) and run the same kernels on the same bits, so after 1, 5 and 25 steps the equilibrated handle's iterate
is the plain handle's mapped to the caller's units (equilibrate_cases.map_to_caller), entry by entry within 4 ulp -- the two roundings of the numpy map
and the two of eq_deinterleave_kernel, the bound of test_iterate_round_trip_and_factors.  Where two PLAIN handles of the same data do not agree to the
bit, their largest difference (in the scaled units, carried to each entry's units) would be added to the bound; it is zero on every path here, and
Trio.assert_same asserts that (plain_allowance = 0: a path that turned non-deterministic fails instead of loosening its own bound).  Every test asserts from the handle's own stats that the intended path ran.

Then what comes back in the caller's units (get_checked, the in-loop check, getsol, set_iterate), what stays in the scaled problem's (the affine and the
algorithm state), and the verdicts other than Optimal.
"""
import numpy as np
import pytest

import equilibrate_cases as ec
import equilibrate_status as es
import fos_oracle as orc
import status_reference as sref
from test_gpu_cg_variants import VARIANTS
from test_gpu_status_formats import _got

pytestmark = pytest.mark.gpu

PASSES = 10
STEPS = (1, 5, 25)


def omodel(prob):
    codes = lambda cs: [(orc.CONE_CODES[k], n) for k, n in cs]
    return orc.Model(prob.A, prob.b, prob.c, codes(prob.K1), codes(prob.K2))


class Trio:
    """two plain handles of host_equilibrate's data and the equilibrated handle of the caller's"""

    def __init__(self, pkg, prob, passes=PASSES):
        self.pkg, self.prob = pkg, prob
        self.host = pkg.host_equilibrate(prob.A, prob.b, prob.c, prob.K1, prob.K2, passes)
        self.scaled = type(prob)("scaled", self.host["A"], self.host["b"], self.host["c"], prob.K1, prob.K2)
        mk = lambda p, **kw: pkg.HipHSDE(p.A, p.b, p.c, p.K1, p.K2, **kw)
        self.all = []
        for p, kw in ((self.scaled, {}), (self.scaled, {}), (prob, dict(equilibrate=passes))):
            self.all.append(mk(p, **kw))
        self.plain, self.plain2, self.eq = self.all
        self.worst_ulp, self.worst_plain = 0.0, 0.0
        self.plain_allowance = 0.0

    def close(self):
        for d in self.all:
            d.close()

    def each(self, fn):
        """fn(handle, the A that handle's caller holds)"""
        for d, A in ((self.plain, self.scaled.A), (self.plain2, self.scaled.A), (self.eq, self.prob.A)):
            fn(d, A)

    def to_caller(self, zhat):
        return ec.map_to_caller(zhat, self.host, self.prob.m, self.prob.n)

    def units(self):
        """what one unit of the scaled problem's entry i is in the caller's"""
        return self.to_caller(np.ones(2 * (self.prob.m + self.prob.n + 1)))

    def assert_same(self, what, get=lambda d: d.get_iterate()):
        za, zb = get(self.plain), get(self.plain2)
        delta = float(np.max(np.abs(za - zb)))                       # two plain handles: 0 where the path is bit-reproducible
        assert delta <= self.plain_allowance, (what, delta)          # every path here is (measured); an exception is declared per test, with its reason
        want, got = self.to_caller(za), get(self.eq)
        assert np.all(np.isfinite(got))
        bound = 4 * np.spacing(np.abs(want)) + delta * self.units()
        ulps = float(np.max(np.abs(got - want) / np.spacing(np.abs(want))))
        self.worst_ulp, self.worst_plain = max(self.worst_ulp, ulps), max(self.worst_plain, delta)
        print("%s: worst |eq - map(plain)| = %.2f ulp; plain vs plain max difference %.3g" % (what, ulps, delta))
        assert np.all(np.abs(got - want) <= bound), (what, ulps, delta)

    def run(self, steps=STEPS, eps=1e-5):
        at = 0
        for upto in steps:
            for d in self.all:
                done, checked, _ = d.step(at + 1, upto - at, 10 ** 6, eps)
                assert done == upto - at and not checked
            at = upto
            self.assert_same("after %d steps" % upto)


@pytest.fixture
def trio(pkg):
    made = []

    def make(prob, **kw):
        made.append(Trio(pkg, prob, **kw))
        return made[-1]
    yield make
    for t in made:
        t.close()


@pytest.fixture(scope="module")
def bad_mixed(pkg):
    return ec.badly_scaled(pkg.workloads.small_mixed(), 1)


@pytest.fixture(scope="module")
def bad_k16(pkg):
    return ec.badly_scaled(pkg.workloads.c4_block_sdp(nblocks=8, k=16, p=12), 2)        # (p = 6: blocks too narrow for dual tiles, no resident plan)


@pytest.fixture(scope="module")
def bad_k64(pkg):
    return ec.badly_scaled(pkg.workloads.c4_block_sdp(nblocks=4, k=64, p=4), 3)


ALGS = {"DR": lambda p, **kw: p.DR(**kw), "GAPA": lambda p, **kw: p.GAPA(**kw), "Dykstra": lambda p, **kw: p.Dykstra(**kw)}


def _start(t, alg, setup=None):
    def one(d, A):
        d.set_alg(alg)
        if setup:
            setup(d, A)
        d.set_iterate(None)
    t.each(one)


# ---------------------------------------------------------------------------------------------- the same steps, path by path


@pytest.mark.parametrize("algname", ["DR", "GAPA"])
@pytest.mark.parametrize("variant", ["reference"] + VARIANTS)
def test_same_steps_on_every_cg_variant(pkg, trio, bad_mixed, variant, algname):
    t = trio(bad_mixed)
    _start(t, ALGS[algname](pkg), lambda d, A: d.set_cg_variant(variant))
    for d in t.all:
        assert d.cg_variant_name() == variant
    t.run()
    assert t.eq.cg_total() == t.plain.cg_total() > 0


@pytest.mark.parametrize("form", ["registers", "streamed"])
def test_same_steps_on_the_resident_cg(pkg, trio, bad_k16, form, monkeypatch):
    if form == "streamed":
        monkeypatch.setenv("FOS_RESIDENT_STREAM", "2")
        monkeypatch.setenv("FOS_RESIDENT_GMAX", "2")
    t = trio(bad_k16)
    for d in t.all:
        st = d.resident_stats()
        assert st["qualifies"] == 1 and st["form"] == form, st
    assert t.eq.resident_stats() == t.plain.resident_stats()
    _start(t, pkg.DR(), lambda d, A: d.set_cg_variant("resident"))
    for d in t.all:
        assert d.cg_variant_name() == "resident"
    t.run()


def test_same_steps_on_the_fused_psd64_step(pkg, trio, bad_k64):
    """relaxation + PSD(64) + final pass in one launch, the refinement warm-started from the previous basis: 25 DR steps"""
    t = trio(bad_k64)
    _start(t, pkg.DR())
    t.run()
    fused = [d.psd_fused_steps() for d in t.all]
    print("fused steps:", fused)
    assert fused[0] > 0 and fused[0] == fused[1] == fused[2]


def test_same_steps_on_the_sign_function_psd(pkg, trio):
    """PSD cones of order 80 > 64: the sign-function path (psd_sign.hip), 5 DR steps.  The handle has no stat that names this path; a cone of order 80
    can only be projected by it (launch_cones_psd_sign takes every cone of order > 64, the batched kernels none), and the fused PSD(64) step is asserted
    not to have run."""
    prob = ec.badly_scaled(pkg.workloads.c4_block_sdp(nblocks=2, k=80, p=6), 4)
    t = trio(prob)
    _start(t, pkg.DR())
    t.run(steps=(1, 5))
    assert all(d.psd_fused_steps() == 0 for d in t.all)


DIRECT = [("dense", "newton"), ("dense", "cholesky"), ("block", "newton"), ("reduced", "newton"), ("reduced", "cholesky")]


@pytest.mark.parametrize("form,factor", DIRECT, ids=["%s-%s" % f for f in DIRECT])
def test_same_steps_with_direct_in_every_form(pkg, trio, bad_mixed, form, factor, monkeypatch):
    """direct = true: the equilibrated handle is given the CALLER's A and rescales it (fos_enable_direct*); small_mixed is block separable, so the block
    form is the library's own choice, the dense one is forced by FOS_DIRECT_MODE, the reduced one asked for"""
    if form == "dense":
        monkeypatch.setenv("FOS_DIRECT_MODE", "dense")
    t = trio(bad_mixed)
    _start(t, pkg.DR(direct=True), lambda d, A: d.enable_direct(A, form="reduced" if form == "reduced" else "auto", factor=factor))
    for d in t.all:
        assert d.direct_mode() == form
        if form != "block":
            assert d.direct_stats()["factor"] == factor and d.direct_stats()["fell_back"] == 0
    t.run()
    assert t.eq.cg_total() == t.plain.cg_total()


@pytest.mark.parametrize("geom", ["1", "2"])
def test_same_steps_on_window_panels(pkg, trio, geom, monkeypatch):
    import status_cases as cases
    A = dict(cases.window_shapes())["tall"]
    m, n = A.shape
    prob = ec.badly_scaled(pkg.workloads.from_complementary_pair("tall", A, [("Zero", m)], [("NonNeg", n)], np.random.default_rng(cases._seed("loop", "tall"))), 5)
    monkeypatch.setenv("FOS_WINDOWS", geom)
    t = trio(prob)
    for d in t.all:
        st = d.operator_stats()
        assert st["win_panels"] > 0 and st["blocks"] == 0, st
    _start(t, pkg.DR())
    t.run()


@pytest.mark.parametrize("algname", ["DR", "Dykstra"])
def test_same_steps_with_every_cone_kind(pkg, trio, algname):
    t = trio(ec.badly_scaled(ec.all_kinds(pkg), 6))
    _start(t, ALGS[algname](pkg))
    t.run()


# ---------------------------------------------------------------------------------------------- what comes back, in whose units


@pytest.mark.parametrize("which", ["bad_mixed", "bad_k64"])
def test_what_comes_back_in_the_callers_units(pkg, trio, request, which):
    prob = request.getfixturevalue(which)
    t = trio(prob)
    _start(t, pkg.DR())
    eps = 1e-8
    results = []
    for d in t.all:
        done, checked, res = d.step(1, 10, 10, eps)
        assert done == 10 and checked
        results.append(res)
    # the checked iterate, and the in-loop check: within 2 x allowance of the reference at get_checked() (which carries the two roundings per entry of
    # the way out, as the allowance's "iterate in" does), the verdict that of the stand-alone check of the same vector
    t.assert_same("checked iterate", lambda d: d.get_checked())
    z = t.eq.get_checked()
    vals, allow = es.reference(prob.A, prob.b, prob.c, z)
    # (a deliberate loosening of "equal field for field": eq_deinterleave divides and eq_interleave multiplies, so the stand-alone check sees a vector up
    # to 1 ulp per entry away from the one the in-loop check saw, and bitwise equality cannot hold)
    alone = t.eq.check(z, eps)
    for name, res in (("in-loop", results[2]), ("stand-alone", alone)):
        rat = sref.ratios(_got(res), vals, allow)
        print("%s check: worst error / allowance %.3g (%s)" % (name, max(rat.values()), max(rat, key=rat.get)))
        assert max(rat.values()) <= 2.0, (name, rat)
    assert results[2].status == alone.status and results[2].tau == alone.tau
    assert results[2].cgiter == results[0].cgiter
    # the states that speak the scaled problem: bit-identical
    for d in (t.plain, t.eq):
        d.step(11, 3, 10 ** 6, eps)
    xa, ia, fa = t.plain.get_affine_state()
    xb, ib, fb = t.eq.get_affine_state()
    assert np.array_equal(xa, xb) and ia == ib and fa == fb
    # getsol: the guess in the caller's units (the PSD projections are warm-started, so a second evaluation agrees to the eigen-solver's tolerance)
    za, ra = t.plain.getsol(force_check=True, eps=eps)
    zb, rb = t.eq.getsol(force_check=True, eps=eps)
    want = t.to_caller(za)
    n, m, l = prob.n, prob.m, prob.n + prob.m + 1
    for lo, hi, part in ((0, n, "x"), (n, n + m, "y"), (l + n, l + n + m, "s")):
        err, scale = np.max(np.abs(zb[lo:hi] - want[lo:hi])), np.max(np.abs(want[lo:hi]))
        print("getsol %s: max difference %.3e of %.3e" % (part, err, scale))
        assert err <= 1e-10 * scale, part
        tau = za[l - 1]                                            # x = E x^ / (sigma tau) and its siblings
        assert np.max(np.abs(zb[lo:hi] / zb[l - 1] - want[lo:hi] / tau)) <= 1e-10 * scale / abs(tau), part
    assert zb[l - 1] == za[l - 1] and rb.tau == ra.tau
    vals, allow = es.reference(prob.A, prob.b, prob.c, zb)
    assert max(sref.ratios(_got(rb), vals, allow).values()) <= 2.0


@pytest.mark.parametrize("which", ["bad_mixed", "bad_k64"])
@pytest.mark.parametrize("algname", ["Dykstra", "GAPA"])
def test_algorithm_state_speaks_the_scaled_problem(pkg, trio, request, which, algname):
    """get_alg_state (Dykstra: p, q; GAPA: alpha12) of the equilibrated handle and of the plain handle of the scaled data: bit-identical"""
    t = trio(request.getfixturevalue(which))
    _start(t, ALGS[algname](pkg))
    for d in (t.plain, t.eq):
        d.step(1, 7, 10 ** 6, 1e-5)
    a0, b0, t0, al0 = t.plain.get_alg_state()
    a1, b1, t1, al1 = t.eq.get_alg_state()
    assert np.array_equal(a0, a1) and np.array_equal(b0, b1) and t0 == t1 and al0 == al1
    if algname == "Dykstra":
        assert np.any(a0 != 0)


@pytest.mark.parametrize("which", ["bad_mixed", "bad_k64"])
def test_set_iterate_then_step(pkg, trio, request, which):
    """set_iterate(z) in the caller's units, then steps: the iterates of the plain handle set to the scaled z.  eq_interleave_kernel multiplies by
    (sigma / E, rho E), (rho / D, sigma D), (1, sigma rho) with contraction off: numpy forms the same products to the bit, so the handles hold the same
    vector and the 4 ulp bound of the way out applies after the steps as well."""
    prob = request.getfixturevalue(which)
    t = trio(prob)
    _start(t, pkg.DR())
    n, m, l = prob.n, prob.m, prob.m + prob.n + 1
    D, E, sg, rho = t.host["D"], t.host["E"], t.host["sigma"], t.host["rho"]
    z = np.random.default_rng(8).standard_normal(2 * l) * t.units()
    z[l - 1] = 1.3
    zhat = z.copy()
    zhat[0:n], zhat[n:n + m] = z[0:n] * (sg / E), z[n:n + m] * (rho / D)
    zhat[l:l + n], zhat[l + n:l + n + m], zhat[2 * l - 1] = z[l:l + n] * (rho * E), z[l + n:l + n + m] * (sg * D), z[2 * l - 1] * (sg * rho)
    t.eq.set_iterate(z)
    t.plain.set_iterate(zhat)
    t.plain2.set_iterate(zhat)
    t.assert_same("after set_iterate")
    t.run(steps=(1, 5))


# ---------------------------------------------------------------------------------------------- verdicts other than Optimal


def _infeasible_and_unbounded(pkg):
    """the two problems of test_gpu_parity.test_infeasible_and_unbounded_detection"""
    import scipy.sparse as sp
    rng = np.random.default_rng(0)
    m, n = 8, 12
    Ad = rng.standard_normal((m, n))
    y = rng.standard_normal(m)
    Ad = Ad * np.sign(Ad.T @ y)[None, :]                    # A'y >= 0
    b = -np.abs(rng.standard_normal(m)) * np.sign(y)        # b'y < 0  -> {Ax = b, x >= 0} is infeasible (Farkas)
    inf = pkg.workloads.ConicProblem("inf", sp.csc_matrix(Ad), b, rng.standard_normal(n), [("Zero", m)], [("NonNeg", n)])
    A2 = rng.standard_normal((m, n))
    dd = rng.standard_normal(n)
    A2 = A2 - np.outer(np.maximum(A2 @ dd, 0) + 0.1, dd) / (dd @ dd)     # A2 d <= -0.1, c'd < 0: unbounded ray
    unb = pkg.workloads.ConicProblem("unb", sp.csc_matrix(A2), np.abs(rng.standard_normal(m)) + 1, -dd, [("NonNeg", m)], [("Free", n)])
    return {"inf": inf, "unb": unb}


@pytest.mark.parametrize("which", ["inf", "unb"])
def test_verdicts_other_than_optimal(pkg, which):
    """The infeasible and the unbounded problem, badly scaled, solved with equilibrate = 10: tau runs to zero and ||A x + s||, ||A'y|| decide.  The verdict
    of the solve is the oracle's solving the caller's data (the reference's tests are literal, so it is one of Unbounded / Infeasible, not necessarily the
    problem's name).  The oracle's decision from its own residuals on the caller's data agrees on THE VECTOR THE DECIDING CHECK SAW, read with
    get_checked() right after the step that checked -- not on model.guess: getsol takes one more projection pair past that vector (and reuses its buffer),
    and at a certificate the new point fails the literal tests: the oracle's own guess gives Continue on all four of its own solves of these problems,
    scaled or not.  The deciding check itself is held to the reference at 2 x allowance."""
    eps, checki = 1e-6, 20
    prob = ec.badly_scaled(_infeasible_and_unbounded(pkg)[which], 7)
    sol = orc.solve(omodel(prob), orc.DR(eps=eps, verbose=0, max_iters=5000, checki=checki), out=[])
    assert sol.status in ("Unbounded", "Infeasible")
    model = pkg.solve(prob, pkg.DR(eps=eps, checki=checki, max_iters=5000, equilibrate=PASSES, verbose=0))
    try:
        print("%s: %s after %d iterations (oracle on the caller's data: %s after %d)" % (prob.name, model.status(), model.iterations, sol.status, sol.iterations))
        assert model.data.equilibration()["passes"] == PASSES
        assert model.status() == sol.status
        iterations = model.iterations
    finally:
        model.data.close()
    # the same solve by hand (solverwrapper.jl:23-29 as FOSMathProgModel.optimize runs it), stopping at the deciding check
    d = pkg.HipHSDE(prob.A, prob.b, prob.c, prob.K1, prob.K2, equilibrate=PASSES)
    try:
        d.set_alg(pkg.DR())
        d.set_iterate(None)
        i, name = 0, "Continue"
        while name == "Continue" and i < 5000:
            done, checked, res = d.step(i + 1, checki, checki, eps)
            assert done == checki and checked
            i += done
            name = pkg.lib.STATUS_NAMES[res.status]
        assert (name, i) == (sol.status, iterations)
        z = d.get_checked()
        assert orc.decide_status(orc.residuals(omodel(prob), z), eps) == sol.status
        vals, allow = es.reference(prob.A, prob.b, prob.c, z)
        rat = sref.ratios(_got(res), vals, allow)
        print("  tau = %.3e, ||A x + s|| = %.3e, ||A'y|| = %.3e; worst error / allowance %.3g (%s)" % (res.tau, res.norm_axs, res.norm_aty, max(rat.values()), max(rat, key=rat.get)))
        assert max(rat.values()) <= 2.0, rat
        assert sref.decide(vals, eps) == sol.status
    finally:
        d.close()
