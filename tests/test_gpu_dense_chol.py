"""
direct = true, the Cholesky factor of the stored inverse on the device (csrc/dense_chol.hip): the blocked factorisation and inversion on its own at the edges of
the 64-blocking (fos_dense_spd_inverse), its bad-pivot report, and the reduced and the dense form set up through it -- against the oracle at the tolerances of
tests/test_gpu_direct_reduced.py / tests/test_gpu_direct.py, and against the Newton-Schulz factor on the same input.
"""
import numpy as np
import pytest

import fos_oracle as orc
from test_dense_chol_cpu import FOS_EINVAL, ORDERS, spd_matrix
from test_gpu_direct import _omodel
from test_gpu_direct_reduced import PROBLEMS, _rect_problem

pytestmark = pytest.mark.gpu

NEWTON, CHOLESKY = 0, 1
CASES = dict(PROBLEMS)
CASES["k=321"] = lambda pkg: _rect_problem(pkg, 700, 321, 5)          # five block columns and a ragged sixth


def device_inverse(pkg, K, factor):
    lib = pkg.lib.load()
    k = K.shape[0]
    X = np.zeros((k, k), order="F")
    info = np.full(4, np.nan)
    rc = lib.fos_dense_spd_inverse(0, k, pkg.lib.dptr(np.asfortranarray(K)), pkg.lib.dptr(X), factor, pkg.lib.dptr(info))
    return rc, X, info


@pytest.mark.parametrize("k", ORDERS)
def test_stand_alone_inverse(pkg, k):
    K = spd_matrix(k)
    rc, X, info = device_inverse(pkg, K, CHOLESKY)
    assert rc == 0, pkg.lib.load().fos_last_error()
    resid = float(np.max(np.abs(K @ X - np.eye(k))))
    print("k = %d: cond(K) = %.3e, max |K X - I| = %.3e, info4 = %s" % (k, np.linalg.cond(K), resid, info))
    assert resid <= 1e-12
    assert np.array_equal(X, X.T)
    assert info[0] == -1 and 0 <= info[1] <= 2 and info[2] <= 1e-12 and info[3] == 0          # no bad pivot, polish steps, probe, no fallback
    rc2, X2, _ = device_inverse(pkg, K, CHOLESKY)
    assert rc2 == 0 and np.array_equal(X, X2)                                                  # the same bits from a second call
    rcn, Xn, infon = device_inverse(pkg, K, NEWTON)
    assert rcn == 0 and infon[1] > 0 and infon[3] == 0
    print("        max |X_chol - X_newton| / max |X_newton| = %.3e" % (np.max(np.abs(X - Xn)) / np.max(np.abs(Xn))))
    assert np.max(np.abs(X - Xn)) <= 1e-12 * np.max(np.abs(Xn))


@pytest.mark.parametrize("k,col", [(130, 5), (130, 129), (321, 320)])
def test_bad_pivot_is_an_error_return(pkg, k, col):
    lib = pkg.lib.load()
    K = spd_matrix(k)
    Kbad = K.copy(order="F")
    Kbad[col, col] = -1.0
    rc, _, info = device_inverse(pkg, Kbad, CHOLESKY)
    msg = lib.fos_last_error().decode()
    assert rc == FOS_EINVAL and ("column %d" % col) in msg, msg
    assert info[0] == col
    rc, X, info = device_inverse(pkg, K, CHOLESKY)                                             # the process goes on: the next valid call succeeds
    assert rc == 0 and info[0] == -1 and np.max(np.abs(K @ X - np.eye(k))) <= 1e-12


@pytest.mark.parametrize("which", list(CASES))
def test_reduced_form_through_cholesky(pkg, which):
    prob = CASES[which](pkg)
    rng = np.random.default_rng(9)
    S1 = orc.IndAffineDirect(orc.HSDEMatrixQ(prob.A, prob.b, prob.c))
    handles = []
    for _ in range(2):
        d = pkg.HipHSDE(prob.A, prob.b, prob.c, prob.K1, prob.K2)
        d.enable_direct(prob.A, form="reduced", factor="cholesky")
        handles.append(d)
    dn = pkg.HipHSDE(prob.A, prob.b, prob.c, prob.K1, prob.K2)
    dn.enable_direct(prob.A, form="reduced")
    d = handles[0]
    assert d.direct_mode() == "reduced"
    st, stn = d.direct_stats(), dn.direct_stats()
    print(which, st)
    assert st["form"] == "reduced" and st["k"] == min(prob.A.shape) and st["setup_s"] > 0.0
    assert st["factor"] == "cholesky" and st["fell_back"] == 0 and 0 <= st["ns_steps"] <= 2 and st["invert_s"] > 0.0 and st["probe_resid"] <= 1e-12
    assert stn["factor"] == "newton" and stn["fell_back"] == 0 and stn["ns_steps"] > 0 and stn["invert_s"] > 0.0
    l = d.l
    cond = np.linalg.cond(np.eye(l) + S1.Qd @ S1.Qd.T)
    for scale in (1.0, 1e3):
        x = scale * rng.standard_normal(d.N)
        y = d.prox_affine(x)
        assert d.cgiter() == 0
        ref = np.empty(d.N)
        S1.prox(ref, x)
        yn = dn.prox_affine(x)
        print(which, scale, "rel err", np.linalg.norm(y - ref) / np.linalg.norm(ref), "cond", cond, "vs newton", np.linalg.norm(y - yn) / np.linalg.norm(y))
        assert np.linalg.norm(y - ref) <= 1e-12 * np.linalg.norm(ref) * max(1.0, cond / 1e3)
        assert np.linalg.norm(d.q_apply(y[:l]) - y[l:]) <= 1e-12 * np.linalg.norm(y)
        u = rng.standard_normal(l)
        t = np.concatenate([u, d.q_apply(u)])
        assert abs((x - y) @ t) <= 1e-11 * np.linalg.norm(t) * np.linalg.norm(x)
        assert np.linalg.norm(y - yn) <= 1e-12 * np.linalg.norm(y)
        assert np.array_equal(handles[1].prox_affine(x), y)                                    # two handles, identical bits
    for h in handles + [dn]:
        h.close()


def test_dense_form_through_cholesky(pkg, monkeypatch):
    prob = pkg.workloads.small_lp(seed=21, m=96, n=180)
    monkeypatch.setenv("FOS_DIRECT_MODE", "dense")
    d = pkg.HipHSDE(prob.A, prob.b, prob.c, prob.K1, prob.K2)
    d.enable_direct(prob.A, factor="cholesky")
    st = d.direct_stats()
    print("dense", st)
    assert d.direct_mode() == "dense" and st["form"] == "dense" and st["k"] == d.l
    assert st["factor"] == "cholesky" and st["fell_back"] == 0 and 0 <= st["ns_steps"] <= 2 and st["invert_s"] > 0.0
    S1 = orc.IndAffineDirect(orc.HSDEMatrixQ(prob.A, prob.b, prob.c))
    rng = np.random.default_rng(4)
    l = d.l
    cond = np.linalg.cond(np.eye(l) + S1.Qd @ S1.Qd.T)
    for scale in (1.0, 1e3):
        x = scale * rng.standard_normal(d.N)
        y = d.prox_affine(x)
        assert d.cgiter() == 0
        ref = np.empty(d.N)
        S1.prox(ref, x)
        print("dense", scale, "rel err", np.linalg.norm(y - ref) / np.linalg.norm(ref), "cond", cond)
        assert np.linalg.norm(y - ref) <= 1e-12 * np.linalg.norm(ref) * max(1.0, cond / 1e3)
        assert np.linalg.norm(d.q_apply(y[:l]) - y[l:]) <= 1e-12 * np.linalg.norm(y)
        u = rng.standard_normal(l)
        t = np.concatenate([u, d.q_apply(u)])
        assert abs((x - y) @ t) <= 1e-11 * np.linalg.norm(t) * np.linalg.norm(x)
    d.close()


def test_whole_solve_through_cholesky_matches_oracle(pkg):
    prob = pkg.workloads.small_mixed()
    opts = dict(eps=1e-6, verbose=1, max_iters=3000, checki=50, direct=True)
    out = []
    model = pkg.solve(prob, pkg.DR(direct_form="reduced", direct_factor="cholesky", **opts), out=out)
    assert model.data.direct_mode() == "reduced" and model.data.direct_stats()["factor"] == "cholesky"
    oout = []
    sol = orc.solve(_omodel(prob), orc.DR(**opts), out=oout)
    assert model.status() == sol.status and model.iterations == sol.iterations
    last, olast = model.status_obj.last, sol.status_obj.last
    for key in ("p", "d", "g"):
        assert getattr(last, key) == pytest.approx(olast[key], rel=1e-6, abs=1e-12)
    assert np.max(np.abs(model.getsolution() - sol.x)) <= 1e-9 * max(1.0, np.max(np.abs(sol.x)))


def test_switching_the_factor_on_one_handle(pkg, monkeypatch):
    prob = _rect_problem(pkg, 400, 150, 2)
    x = np.random.default_rng(6).standard_normal(2 * (400 + 150 + 1))
    d = pkg.HipHSDE(prob.A, prob.b, prob.c, prob.K1, prob.K2)
    ys = []
    for factor in ("cholesky", "newton", "cholesky"):
        d.enable_direct(prob.A, form="reduced", factor=factor)
        st = d.direct_stats()
        assert d.direct_mode() == "reduced" and st["factor"] == factor and st["fell_back"] == 0
        assert (st["ns_steps"] > 2) if factor == "newton" else (0 <= st["ns_steps"] <= 2)
        ys.append(d.prox_affine(x))
    assert np.array_equal(ys[0], ys[2])
    for y in ys[1:]:
        assert np.linalg.norm(y - ys[0]) <= 1e-12 * np.linalg.norm(ys[0])
    # the environment picks the factor for callers that did not choose
    monkeypatch.setenv("FOS_DIRECT_FACTOR", "cholesky")
    d2 = pkg.HipHSDE(prob.A, prob.b, prob.c, prob.K1, prob.K2)
    d2.enable_direct(prob.A, form="reduced")
    assert d2.direct_stats()["factor"] == "cholesky" and np.array_equal(d2.prox_affine(x), ys[0])
    monkeypatch.setenv("FOS_DIRECT_FACTOR", "qr")
    with pytest.raises(pkg.lib.FosError) as ei:
        d2.enable_direct(prob.A, form="reduced")
    assert ei.value.code == FOS_EINVAL and "FOS_DIRECT_FACTOR" in str(ei.value)
    d2.close()
    d.close()
