"""An equilibrated handle (fos_create3, equil_passes > 0) on the device: status and iterates in the caller's units (csrc/equilibrate.hip), the same steps
as a plain handle built from the scaled data, a whole solve through the option, and the refusals."""
import ctypes as C

import numpy as np
import pytest

import equilibrate_cases as ec
import fos_oracle as orc

pytestmark = pytest.mark.gpu

PASSES = 10
# the kernels' grid (csrc/fos_internal.hpp): min(ceil(count / 256), 512) workgroups of 256 threads, so the grid-stride loops take a second trip once
# count > 512 * 256 = 131 072
GRID_ELEMENTS = 512 * 256


def omodel(prob):
    codes = lambda cs: [(orc.CONE_CODES[k], n) for k, n in cs]
    return orc.Model(prob.A, prob.b, prob.c, codes(prob.K1), codes(prob.K2))


@pytest.fixture
def handles(pkg):
    made = []

    def make(prob, **kw):
        d = pkg.HipHSDE(prob.A, prob.b, prob.c, prob.K1, prob.K2, **kw)
        made.append(d)
        return d
    yield make
    for d in made:
        d.close()


@pytest.fixture(scope="module")
def bad_mixed(pkg):
    return ec.badly_scaled(pkg.workloads.small_mixed(), 1)


@pytest.fixture(scope="module")
def all_kinds(pkg):
    return ec.all_kinds(pkg)


def compare_check(pkg, dev, prob, mo, z, eps=1e-5):
    """check(z) of an equilibrated handle against the oracle on the ORIGINAL data"""
    res = dev.check(z, eps)
    ref = orc.residuals(mo, z)
    n, m, l = prob.n, prob.m, prob.n + prob.m + 1
    for key in ("p", "d", "kappa", "tau"):
        print(key, getattr(res, key), ref[key])
        assert getattr(res, key) == pytest.approx(ref[key], rel=1e-12, abs=1e-14), key
    print("nAxs", res.norm_axs, ref["nAxs"], "nATy", res.norm_aty, ref["nATy"])
    assert res.norm_axs == pytest.approx(ref["nAxs"], rel=1e-12)
    assert res.norm_aty == pytest.approx(ref["nATy"], rel=1e-12)
    assert res.norm_b == pytest.approx(ref["nb"], rel=1e-14) and res.norm_c == pytest.approx(ref["nc"], rel=1e-14)
    # a dot product's rounding bound at these lengths
    ec_, eb_ = 1e-12 * float(np.sum(np.abs(prob.c * z[0:n]))), 1e-12 * float(np.sum(np.abs(prob.b * z[n:n + m])))
    print("ctx", res.ctx, ref["ctx"], ec_, "bty", res.bty, ref["bty"], eb_)
    assert abs(res.ctx - ref["ctx"]) <= ec_
    assert abs(res.bty - ref["bty"]) <= eb_
    # g = |a + b| / (1 + |a| + |b|), a = ctx / tau, b = bty / tau: |dg| <= 2 (|da| + |db|) / (1 + |a| + |b|)
    tau = z[l - 1]
    den = 1 + abs(ref["ctx"] / tau) + abs(ref["bty"] / tau)
    assert abs(res.g - ref["g"]) <= 2 * (ec_ + eb_) / abs(tau) / den + 1e-15
    assert pkg.lib.STATUS_NAMES[res.status] == orc.decide_status(ref, eps)


def random_points(prob, seed, count=4):
    rng = np.random.default_rng(seed)
    l = prob.n + prob.m + 1
    for _ in range(count):
        z = rng.standard_normal(2 * l)
        z[l - 1] = abs(z[l - 1]) + 0.1
        yield z


def planted(prob):
    return np.concatenate([prob.x0, prob.y0, [1.0], prob.c + prob.A.T @ prob.y0, prob.s0, [0.0]])


@pytest.mark.parametrize("which", ["bad_mixed", "all_kinds"])
def test_status_in_the_callers_units(pkg, handles, request, which):
    prob = request.getfixturevalue(which)
    dev = handles(prob, equilibrate=PASSES)
    mo = omodel(prob)
    for z in random_points(prob, 12):
        compare_check(pkg, dev, prob, mo, z)
    res = dev.check(planted(prob), 1e-8)
    print("planted: p %.3e d %.3e g %.3e" % (res.p, res.d, res.g))
    assert pkg.lib.STATUS_NAMES[res.status] == "Optimal"


# l = m + n + 1: a partial, an exact and a just-exceeded wavefront; a second workgroup; one column, one row; and l > GRID_ELEMENTS, where the grid-stride
# loops of all three kernels take a second trip
SHAPES = [(22, 40), (23, 40), (24, 40), (96, 160), (5, 1), (1, 5), (60000, 80000)]


@pytest.mark.parametrize("m,n", SHAPES)
def test_status_at_the_kernels_edges(pkg, handles, m, n):
    assert (m + n + 1) in (63, 64, 65, 257, 7) or m + n > GRID_ELEMENTS
    prob = ec.sparse_lp(pkg, m, n, seed=m + n)
    assert np.diff(prob.A.indptr).max() <= 3
    dev = handles(prob, equilibrate=PASSES)
    mo = omodel(prob)
    for z in random_points(prob, 3, count=2):
        compare_check(pkg, dev, prob, mo, z)
        dev.set_iterate(z)                                        # the (de)interleave kernels at the same shapes
        back = dev.get_iterate()
        assert np.all(np.abs(back - z) <= 4 * np.spacing(np.abs(z)))
    assert pkg.lib.STATUS_NAMES[dev.check(planted(prob), 1e-8).status] == "Optimal"


@pytest.mark.parametrize("which", ["bad_mixed", "all_kinds"])
def test_iterate_round_trip_and_factors(pkg, handles, request, which):
    prob = request.getfixturevalue(which)
    dev = handles(prob, equilibrate=PASSES)
    for z in random_points(prob, 5, count=2):
        dev.set_iterate(z)
        back = dev.get_iterate()
        ulps = np.abs(back - z) / np.spacing(np.abs(z))
        print("round trip: worst %.1f ulp" % ulps.max())
        assert ulps.max() <= 4
    got, host = dev.equilibration(), pkg.host_equilibrate(prob.A, prob.b, prob.c, prob.K1, prob.K2, PASSES)
    assert got["passes"] == PASSES
    for key in ("D", "E"):
        assert np.array_equal(got[key], host[key]), key
    for key in ("sigma", "rho", "gamma"):
        assert got[key] == host[key], key
    plain = handles(prob)
    eq0 = plain.equilibration()
    assert eq0["passes"] == 0 and np.all(eq0["D"] == 1) and np.all(eq0["E"] == 1) and (eq0["sigma"], eq0["rho"], eq0["gamma"]) == (1.0, 1.0, 1.0)


ALGS = {"DR": lambda p: p.DR(), "GAPA": lambda p: p.GAPA(), "FISTA": lambda p: p.FISTA(), "Dykstra": lambda p: p.Dykstra()}


def _same_steps(pkg, handles, prob, alg, direct=False):
    host = pkg.host_equilibrate(prob.A, prob.b, prob.c, prob.K1, prob.K2, PASSES)
    scaled = type(prob)("scaled", host["A"], host["b"], host["c"], prob.K1, prob.K2)
    plain, eq = handles(scaled), handles(prob, equilibrate=PASSES)
    for d, A in ((plain, scaled.A), (eq, prob.A)):
        d.set_alg(alg)
        if direct:
            d.enable_direct(A)                                    # the equilibrated handle receives the CALLER's values
        d.set_iterate(None)
    assert plain.direct_mode() == eq.direct_mode() and (eq.direct_mode() != "off") == direct
    at = 0
    for upto in (1, 5, 25):
        for d in (plain, eq):
            done, checked, _ = d.step(at + 1, upto - at, 10 ** 6, 1e-5)
            assert done == upto - at and not checked
        at = upto
        want = ec.map_to_caller(plain.get_iterate(), host, prob.m, prob.n)
        got = eq.get_iterate()
        err = float(np.max(np.abs(got - want)))
        print("after %d steps: max |dz| = %.3e, max |z| = %.3e" % (upto, err, np.max(np.abs(want))))
        assert err <= 1e-12 * np.max(np.abs(want))


@pytest.mark.parametrize("name", sorted(ALGS))
def test_same_steps_as_the_scaled_problem(pkg, handles, bad_mixed, name):
    _same_steps(pkg, handles, bad_mixed, ALGS[name](pkg))


def test_same_steps_with_direct(pkg, handles, bad_mixed):
    _same_steps(pkg, handles, bad_mixed, pkg.DR(direct=True), direct=True)


def test_whole_solve_through_the_option(pkg, bad_mixed):
    """DR(eps = 1e-6) through the option key on the badly scaled small_mixed: Optimal (measured: after 1350 iterations, 0.6 s).  The plain solve of this
    problem is not run here: its CG sits at the iteration cap for minutes (tools/equilibrate_bench.py: not optimal at 5000)."""
    prob = bad_mixed
    model = pkg.solve(prob, pkg.DR(eps=1e-6, checki=50, max_iters=6000, equilibrate=PASSES, verbose=0))
    try:
        print("status %s after %d iterations" % (model.status(), model.iterations))
        assert model.status() == "Optimal"
        assert orc.decide_status(orc.residuals(omodel(prob), model.guess), 1e-6) == "Optimal"
        # the guess in the scaled problem's own units: getsol left P_S1(x) in the affine state, the guess is its cone projection.  The PSD projections are
        # warm-started from the previous call, so the second evaluation agrees to the eigen-solver's tolerance, not to the bit.
        dev = model.data
        eq = dev.equilibration()
        assert eq["passes"] == PASSES
        zhat = dev.prox_cones(dev.get_affine_state()[0])
        l = prob.m + prob.n + 1
        want = eq["E"] * zhat[0:prob.n] / (eq["sigma"] * zhat[l - 1])
        got = model.getsolution()
        print("max |x - E x^ / (sigma tau)| = %.3e" % np.max(np.abs(got - want)))
        assert np.max(np.abs(got - want)) <= 1e-10 * np.max(np.abs(want))
    finally:
        model.data.close()


def _create2(pkg, prob):
    """a handle made by fos_create2 itself, as HipHSDE did before the option existed"""
    lib = pkg.lib.load()
    m, n, args, nnz = pkg.interface._problem_args(prob.A, prob.b, prob.c, prob.K1, prob.K2)
    h = C.c_void_p()
    pkg.lib.check(lib.fos_create2(*args, 0, 0, C.byref(h)))
    d = object.__new__(pkg.HipHSDE)
    d._lib, d._h, d.m, d.n, d.l, d.N, d.nnz = lib, h, m, n, m + n + 1, 2 * (m + n + 1), nnz
    return d


def test_zero_passes_is_the_plain_handle(pkg, handles, bad_mixed):
    prob = pkg.workloads.small_mixed()
    ref, dev = _create2(pkg, prob), handles(prob, equilibrate=0)
    try:
        z = next(random_points(prob, 9, count=1))
        a, b = ref.check(z, 1e-5), dev.check(z, 1e-5)
        for name, _ in pkg.lib.CheckResult._fields_:
            assert getattr(a, name) == getattr(b, name), name
        for d in (ref, dev):
            d.set_alg(pkg.DR())
            d.set_iterate(None)
        for i in range(1, 6):
            ref.step(i, 1, 10 ** 6, 1e-5)
            dev.step(i, 1, 10 ** 6, 1e-5)
            assert np.array_equal(ref.get_iterate(), dev.get_iterate()), i
    finally:
        ref.close()


def test_refusals(pkg, handles, bad_mixed):
    prob = bad_mixed
    with pytest.raises(pkg.lib.FosError) as e:
        pkg.HipHSDE(prob.A, prob.b, prob.c, prob.K1, prob.K2, row_sharded=True, equilibrate=PASSES)
    assert e.value.code == -4                                     # FOS_EUNSUPPORTED
    for passes in (-1, 51):
        with pytest.raises(pkg.lib.FosError) as e:
            pkg.HipHSDE(prob.A, prob.b, prob.c, prob.K1, prob.K2, equilibrate=passes)
        assert e.value.code == -1                                 # FOS_EINVAL
    dev = handles(prob, equilibrate=PASSES)
    with pytest.raises(pkg.lib.FosError) as e:
        dev.comm_init_host(1, 0, lambda a: None)
    assert e.value.code == -4
    assert "equilibrated" in str(e.value)
