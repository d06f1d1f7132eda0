"""
GPU: proximable functions that are not indicators as sets of the Feasibility form (Feasibility.jl:2-6 takes any two ProximableFunctions) -- NormL1, SqrNormL2,
ElasticNet, Linear, NormL2, HuberLoss, NormLinf as block kinds of csrc/sets.hip, alone and mixed with the vector sets in one SeparableSum, and
LeastSquares(A, b, lam) on the factored dense form of csrc/affine_dense.hip -- against the references of tests/prox_fn_cases.py: proxes on both sides of every
class boundary with their launch counts, a product of ~300 mixed blocks, the group-lasso shape, the LeastSquares prox on the factored form's plan edges, the
lasso LeastSquares + NormL1 in the algorithms against the oracle and against the device's own callback path, and the error paths.

Tolerance of a separable prox: 1e-13 max(|x|_inf, |parameter|) per element (tests/test_feas_sets_cpu.py derives it); y = x cases are compared bit for bit,
y = 0 cases are exact zeros.  LeastSquares: 1e-12 max(1, |x|_inf), the bar of the factored IndAffine's projection (the shift only raises the smallest
eigenvalue of the matrix that is inverted).
"""
import ctypes

import numpy as np
import pytest

from affine_factored_cases import SHAPES, TOL, instance
from feasibility_cases import ALGS, affine_box_instance
from prox_fn_cases import (ELEMENTWISE, INPUTS, KINDS, PASS_CAP, REDUCTION, THRESHOLD, RefLeastSquares, RefNormL1, RefNormL2, lasso_kkt, make_case,
                           random_mixed_sum)

pytestmark = pytest.mark.gpu

LENGTHS = [1, 64, 65, 1024, 1025, 16384, 16385, 100003]       # both sides of the wavefront / workgroup / grid class boundaries
FOS_EINVAL = -1


def _pack(pkg, S, n):
    return pkg.SeparableSum([(S, n)]).pack(n)


@pytest.mark.parametrize("length", LENGTHS)
@pytest.mark.parametrize("kind", KINDS)
def test_single_block_prox(pkg, kind, length):
    d = pkg.HipFeasibility(pkg.Feasibility(pkg.IndFree(), pkg.IndFree(), length))
    worst = 0.0
    for inp in INPUTS:
        case = make_case(kind, length, inp)
        d.set_blocks(1, *_pack(pkg, case.device_set(pkg), length))              # (replaces the set of the same handle)
        y = d.prox(1, case.x)
        worst = max(worst, case.check(y, inp) / max(case.tol(), 1e-300))
        st = d.set_stats(1)
        assert st["blocks"] == 1 and (st["wave_blocks"], st["workgroup_blocks"], st["grid_blocks"]) == (length <= 1024, 1024 < length <= 16384, length > 16384)
        grid_launches = 1 if kind in ELEMENTWISE else 3 if kind in REDUCTION else 3 + 2 * PASS_CAP
        assert st["launches"] == (1 if length <= 16384 else grid_launches), (inp, st)
        assert st["pass_cap"] == PASS_CAP and 0 <= st["last_passes"] <= PASS_CAP and (kind in THRESHOLD or st["last_passes"] == 0)
        assert d.prox(1, case.x).tobytes() == y.tobytes(), inp                  # a fixed summation order: the same bits
    print("%s, len %d: worst error / tolerance = %.3g" % (kind, length, worst))
    d.close()


def test_bare_function_as_a_set_is_one_block(pkg):
    n = 77
    case = make_case("NormLinf", n, "gauss")
    d = pkg.HipFeasibility(pkg.Feasibility(case.device_set(pkg), pkg.NormL1(0.4), n))
    assert d.set_stats(1)["blocks"] == 1 and d.set_stats(2)["blocks"] == 1
    case.check(d.prox(1, case.x))
    assert np.array_equal(d.prox(2, case.x), RefNormL1(0.4).project(case.x))


def test_separable_sum_of_300_mixed_blocks(pkg):
    S, ref, n, layout = random_mixed_sum(pkg)
    d = pkg.HipFeasibility(pkg.Feasibility(S, pkg.IndFree(), n))
    st = d.set_stats(1)
    assert st["blocks"] == len(layout) == 300 and st["wave_blocks"] + st["workgroup_blocks"] == 300 and st["workgroup_blocks"] > 0 and st["launches"] == 2
    kinds = {l[0] for l in layout}
    assert len(kinds) == 15 and layout[0][0] == layout[-1][0] == "IndFree" and sum(l[0] == "IndFree" for l in layout) > 10
    x = np.random.default_rng(8).standard_normal(n)
    y = d.prox(1, x)
    expect = ref.project(x)
    for kind, start, length, param in layout:
        xs, ys, es = x[start:start + length], y[start:start + length], expect[start:start + length]
        if kind == "IndFree":
            assert ys.tobytes() == xs.tobytes(), (start, length)               # no kernel writes outside its block
        else:
            assert np.abs(ys - es).max() <= 1e-13 * max(np.abs(xs).max(), abs(param)), (kind, start, length)
    assert d.prox(1, x).tobytes() == y.tobytes()
    assert 1 <= d.set_stats(1)["last_passes"] <= PASS_CAP


def test_group_lasso_shape_is_one_launch(pkg):
    nb, bl, lam = 2000, 50, 6.5                                                 # |x_block| ~ 7.07 on a standard normal input: about a quarter of the groups vanish
    n = nb * bl
    d = pkg.HipFeasibility(pkg.Feasibility(pkg.SeparableSum([(pkg.NormL2(lam), bl)] * nb), pkg.IndFree(), n))
    st = d.set_stats(1)
    assert (st["blocks"], st["wave_blocks"], st["launches"]) == (nb, nb, 1)
    x = np.random.default_rng(3).standard_normal(n)
    y = d.prox(1, x).reshape(nb, bl)
    ref = RefNormL2(lam)
    zero = 0
    for k, xb in enumerate(x.reshape(nb, bl)):
        e = ref.project(xb)
        assert np.abs(y[k] - e).max() <= 1e-13 * max(np.abs(xb).max(), lam), k
        if not e.any():
            zero += 1
            assert not y[k].any(), k
    assert 100 < zero < 1900


def _ls_handle(pkg, A, b, lam, n, **kw):
    return pkg.HipFeasibility(pkg.Feasibility(pkg.LeastSquares(A, b, lam, **kw), pkg.IndFree(), n))


@pytest.mark.parametrize("lam", [1e-3, 1.0, 1e3])
@pytest.mark.parametrize("family,m,n", SHAPES)
def test_least_squares_prox_matches_the_dense_solve(pkg, family, m, n, lam):
    A, b = instance(family, m, n)
    d = _ls_handle(pkg, A, b, lam, n)
    st = d.affine_factored_stats(1)
    assert (st["m"], st["n"], st["refine"], st["factor"]) == (m, n, 0, "cholesky") and st["launches"] == 6 + (st["row_blocks"] > 1)
    ref = RefLeastSquares(A, b, lam)
    rng = np.random.default_rng(1)
    x = rng.standard_normal(n)
    for rep in range(2):
        y = d.prox(1, x)
        err, scale = np.abs(y - ref.project(x)).max(), max(1.0, np.abs(x).max())
        print("%s (%d, %d) lam %g rep %d: |y - dense solve| = %.2e (bar %.2e)" % (family, m, n, lam, rep, err, TOL * scale), st)
        assert err <= TOL * scale, (rep, st)
        x = x + 1e-3 * rng.standard_normal(n)
    assert d.prox(1, x).tobytes() == d.prox(1, x).tobytes()                     # every sum has a fixed order: the same bits
    d.close()


def test_least_squares_rank_deficient_zero_row_and_refusals(pkg):
    A, b = instance("gauss", 10, 30)
    n = 30
    x = np.random.default_rng(2).standard_normal(n)
    D, bd = A.copy(), b.copy()
    D[7], bd[7] = D[2], b[2] + 1.0                                              # a duplicated row with an inconsistent right-hand side
    Z = A.copy(); Z[4] = 0.0
    for M, bb in ((D, bd), (Z, b)):
        for lam in (1e-3, 1.0, 1e3):
            for factor in ("cholesky", "newton"):
                y = _ls_handle(pkg, M, bb, lam, n, factor=factor).prox(1, x)
                err = np.abs(y - RefLeastSquares(M, bb, lam).project(x)).max()
                print("lam %g %s: |y - dense solve| = %.2e" % (lam, factor, err))
                assert err <= TOL * max(1.0, np.abs(x).max()), (lam, factor)
    box = pkg.IndBox(0.0, 1.0)
    with pytest.raises(pkg.lib.FosError, match="full row rank"):                # the same matrices are no IndAffine
        pkg.HipFeasibility(pkg.Feasibility(pkg.IndAffine(D, bd, form="factored"), box, n))
    with pytest.raises(pkg.lib.FosError, match="zero"):
        pkg.HipFeasibility(pkg.Feasibility(pkg.IndAffine(Z, b, form="factored"), box, n))
    with pytest.raises(pkg.lib.FosError, match="fos_feas_set_callback") as info:   # m > n: FOS_EINVAL, the message names the host path
        pkg.HipFeasibility(pkg.Feasibility(pkg.LeastSquares(A.T.copy(), np.ones(30), 1.0), box, 10))
    assert info.value.code == FOS_EINVAL
    # a refused call leaves the set as it was; LeastSquares, a box, LeastSquares again on one handle
    d = _ls_handle(pkg, A, b, 1.0, n)
    before = d.prox(1, x)
    lib = pkg.lib.load()
    assert lib.fos_feas_set_least_squares(d._h, 1, 10, pkg.lib.dptr(A), pkg.lib.dptr(b), 0.0, 1) == FOS_EINVAL      # lambda = 0
    assert lib.fos_feas_set_least_squares(d._h, 1, 10, pkg.lib.dptr(A), pkg.lib.dptr(b), 1.0, 7) == FOS_EINVAL      # an unknown factor
    assert lib.fos_feas_set_least_squares(d._h, 1, 31, pkg.lib.dptr(np.ones((31, 30))), pkg.lib.dptr(np.ones(31)), 1.0, 1) == FOS_EINVAL
    assert d.prox(1, x).tobytes() == before.tobytes()
    d.set_set(1, box)
    assert np.array_equal(d.prox(1, x), np.clip(x, 0.0, 1.0))
    d.set_set(1, pkg.LeastSquares(A, b, 2.0))
    assert np.abs(d.prox(1, x) - RefLeastSquares(A, b, 2.0).project(x)).max() <= TOL * max(1.0, np.abs(x).max())


LASSO_LAM, LASSO_MU = 0.7, 0.5


@pytest.mark.parametrize("algname", ["DR", "GAPA", "FISTA", "Dykstra"])
def test_lasso_iterates_match_oracle_and_callback_path(pkg, oracle, algname):
    """LeastSquares(A, b, 0.7) and NormL1(0.5) in the algorithms: the same iterates as the oracle running the reference objects (<= 1e-11 max(1, |x|_inf)) and as
    the device's own callback path running them (<= 1e-10), two iterations for GAPA (its step-length estimate is ill-conditioned, see
    test_host_callback_set_matches_oracle), 30 otherwise.  Then DR to eps = 1e-9: x* = prox_S1(z) satisfies the lasso's KKT conditions to 1e-6, the bar of the
    whole-solve tests at that eps.  (With the numpy references alone DR ends Optimal at iteration 1160 on this instance, KKT residual 3.4e-10: cap 3000.)"""
    orc = oracle
    A, b = affine_box_instance(m=30, n=100)
    n = A.shape[1]
    ref_o, ref_cb = [(RefLeastSquares(A, b, LASSO_LAM), RefNormL1(LASSO_MU)) for _ in range(2)]
    oalg = ALGS[algname](orc, verbose=0)
    ost = orc.FeasibilityStatus(orc.FeasibilityModel(orc.Feasibility(ref_o[0], ref_o[1], n), oalg), 4, 1e-30, 0, 1)
    d = pkg.HipFeasibility(pkg.Feasibility(pkg.LeastSquares(A, b, LASSO_LAM), pkg.NormL1(LASSO_MU), n))
    dc = pkg.HipFeasibility(pkg.Feasibility(ref_cb[0], ref_cb[1], n))
    for h in (d, dc):
        h.set_alg(ALGS[algname](pkg))
        h.set_iterate(None)
    xo = np.zeros(n)
    nsame = 2 if algname == "GAPA" else 30
    for i in range(1, nsame + 1):
        ost.i = i
        oalg.step(xo, i, ost)
        assert d.step(i, 1, 4, 1e-30)[0] == 1 and dc.step(i, 1, 4, 1e-30)[0] == 1
        z = d.get_iterate()
        assert np.abs(z - xo).max() <= 1e-11 * max(1.0, np.abs(xo).max()), (algname, i)
        assert np.abs(z - dc.get_iterate()).max() <= 1e-10, (algname, i)
    for k in (0, 1):
        assert ref_cb[k].calls == ref_o[k].calls > 0               # the callback path really ran the objects ...
    assert d._callbacks == [] and len(dc._callbacks) == 2          # ... and the device objects have no way to call back
    if algname == "DR":
        done, status, err, checked = d.step(nsame + 1, 3000, 10, 1e-9)
        assert status == "Optimal", (status, err, done)
        xs = d.prox(1, d.get_iterate())
        kkt = lasso_kkt(A, b, LASSO_LAM, LASSO_MU, xs)
        print("DR lasso: Optimal after %d iterations, KKT residual %.2e, %d of %d entries on the support" % (nsame + done, kkt, (np.abs(xs) > 1e-6).sum(), n))
        assert kkt <= 1e-6 and 0 < (np.abs(xs) > 1e-6).sum() < n


def test_error_paths_and_replacement(pkg):
    n = 50
    lib = pkg.lib.load()
    c, f = pkg.lib.SET_CODES, pkg.lib.FN_CODES
    d = pkg.HipFeasibility(pkg.Feasibility(pkg.NormLinf(2.0), pkg.IndBox(0.0, 1.0), n))
    x = np.random.default_rng(4).standard_normal(n)
    before = d.prox(1, x)
    i32p, i64p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)

    def raw(kinds, lens, scal, vec):
        kinds, lens, scal = np.array(kinds, dtype=np.int32), np.array(lens, dtype=np.int64), np.array(scal, dtype=np.float64)
        return lib.fos_feas_set_blocks(d._h, 1, len(kinds), kinds.ctypes.data_as(i32p), lens.ctypes.data_as(i64p), pkg.lib.dptr(scal),
                                       None if vec is None else pkg.lib.dptr(np.asarray(vec, dtype=np.float64)))
    for kinds, scal, vec, blk in (([c["IndFree"], f["NormL1"], f["NormL2"]], [0.0, 0.0, -1.0, 0.0, 1.0, 0.0], None, 2),
                                  ([f["NormL1"], c["IndBallL1"], f["HuberLoss"]], [1.0, 0.0, 1.0, 0.0, 0.0, 1.0], None, 3),
                                  ([f["ElasticNet"], f["SqrNormL2"], f["NormLinf"]], [1.0, np.nan, 1.0, 0.0, 1.0, 0.0], None, 1),
                                  ([f["NormL1"], f["Linear"], f["NormLinf"]], [1.0, 0.0, 0.0, 0.0, 1.0, 0.0], None, 2),            # Linear without its vector
                                  ([f["NormL1"], 31, f["NormLinf"]], [1.0, 0.0, 0.0, 0.0, 1.0, 0.0], None, 2),
                                  ([f["NormL1"], f["NormL1"], 8], [1.0, 0.0, 0.0, 0.0, 1.0, 0.0], None, 3)):
        assert raw(kinds, [10, 20, 20], scal, vec) == FOS_EINVAL and ("block %d" % blk) in lib.fos_last_error().decode(), (kinds, lib.fos_last_error())
    assert d.prox(1, x).tobytes() == before.tobytes()                          # the previous set is still there
    # a function set replaced by a callback and back, on one handle
    ref = RefNormL2(1.5)
    d.set_callback(1, ref)
    y_cb = d.prox(1, x)
    assert ref.calls == 1 and np.array_equal(y_cb, ref.project(x))
    d.set_blocks(1, *_pack(pkg, pkg.NormL2(1.5), n))
    y_dev = d.prox(1, x)
    assert ref.calls == 1 and np.abs(y_dev - y_cb).max() <= 1e-13 * max(np.abs(x).max(), 1.5)
    d.set_callback(1, ref)
    assert np.array_equal(d.prox(1, x), y_cb) and ref.calls == 2
    with pytest.raises(pkg.lib.FosError):
        d.set_stats(1)
