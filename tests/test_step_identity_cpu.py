"""The step-identity checker (tests/step_identity.py) on the oracle: every step of oracle trajectories satisfies it -- to the last bit, the
oracle evaluates the same expressions -- and each of five deliberately wrong steps is rejected.  No GPU."""
import numpy as np
import pytest

import fos_oracle as orc
import step_identity as si

BIG = 10 ** 12
ALGS = {"GAP(0.5,2,2)": (0.5, 2.0, 2.0), "GAP(0.3,1.2,1.7)": (0.3, 1.2, 1.7), "AP": (1.0, 1.0, 1.0)}


@pytest.fixture(scope="module")
def mixed(pkg):
    prob = si.mixed_problem(pkg.workloads)
    assert prob.A.shape == (6320, 14)
    return prob, si.StepIdentity(prob.A, prob.b, prob.c, prob.K1, prob.K2)


@pytest.fixture(scope="module")
def direct_alg(mixed):
    """the oracle's exact affine projection (a dense Cholesky factor of order 6335): built once, shared by the three direct trajectories"""
    alg = orc.GAP(direct=True)
    alg.init(si.oracle_model(mixed[0]))
    return alg


def _trajectory(prob, params, direct, steps, alg=None):
    """(x, sol, x+, i) of every step; sol from CGdata.xinit behind the step, or what the exact projection returned (direct)."""
    alpha, a1, a2 = params
    om = si.oracle_model(prob)
    if alg is None:
        alg = orc.GAP(alpha, a1, a2, direct=direct)
        alg.init(om)
    alg.alpha, alg.alpha1, alg.alpha2 = params
    st = orc.HSDEStatus(om, BIG, 1e-8, 0, 0)
    x = orc.hsde_initialvalue(om)
    out, seen = [], {}
    if direct:                                   # the exact projection keeps no state: record what the step's own call returned
        inner = alg.S1.prox

        def recording(y, xin):
            r = inner(y, xin)
            seen["sol"] = y.copy()
            return r
        alg.S1.prox = recording
    try:
        for k in range(1, steps + 1):
            x0 = x.copy()
            i = None if direct else alg.S1.i
            st.i = k
            alg.step(x, k, st)
            sol = seen["sol"] if direct else alg.S1.cgdata.xinit.copy()
            out.append((x0, sol, x.copy(), i))
    finally:
        if direct:
            del alg.S1.prox                      # (the instance attribute: the class's method is back)
    return out


@pytest.mark.parametrize("direct", [False, True], ids=["cg", "direct"])
@pytest.mark.parametrize("name", list(ALGS))
def test_oracle_trajectories_satisfy_the_identity(mixed, request, name, direct):
    prob, chk = mixed
    alpha, a1, a2 = ALGS[name]
    traj = _trajectory(prob, ALGS[name], direct, 30, request.getfixturevalue("direct_alg") if direct else None)
    moved = 0.0
    for k, (x, sol, xp, i) in enumerate(traj, 1):
        assert i is None or i == k
        res = chk.check(x, sol, xp, alpha, a1, a2, i)
        assert res.ok, (k, str(res))
        assert res.psd_dev == 0.0 and res.ew_worst() == 0.0, (k, str(res))      # the oracle evaluates these very expressions
        moved = max(moved, float(np.linalg.norm(xp - x)))
    assert moved > 1e-3


@pytest.fixture(scope="module")
def asym_step(mixed):
    """step 10 of GAP(0.3, 1.2, 1.7), CG: the step the corrupted variants are made from"""
    prob, chk = mixed
    x, sol, xp, i = _trajectory(prob, ALGS["GAP(0.3,1.2,1.7)"], False, 10)[-1]
    alpha, a1, a2 = ALGS["GAP(0.3,1.2,1.7)"]
    assert chk.check(x, sol, xp, alpha, a1, a2, i).ok
    return x, sol, xp, i


def _finish(t1, t2, x, alpha, a2):
    return alpha * (a2 * t2 + (1 - a2) * t1) + (1 - alpha) * x


def _wrong_swapped(chk, x, sol, xp):
    alpha, a1, a2 = ALGS["GAP(0.3,1.2,1.7)"]
    return chk.reference(x, sol, alpha, a2, a1)[2]              # a1 and alpha2 exchanged


def _wrong_dual_sign(chk, x, sol, xp):
    alpha, a1, a2 = ALGS["GAP(0.3,1.2,1.7)"]
    t1, t2, _ = chk.reference(x, sol, alpha, a1, a2)
    s, ln = chk.psd_segments[1]                                  # the dual copy (first half) of the second PSD cone: x + P(x) for x + P(-x) (cones.jl:80-85)
    seg = np.empty(ln)
    orc.cone_prox(orc.CONE_SDP, seg, t1[s:s + ln])
    seg += t1[s:s + ln]
    assert np.linalg.norm(seg - t2[s:s + ln]) > 1e-3
    t2[s:s + ln] = seg
    return _finish(t1, t2, x, alpha, a2)


def _wrong_nonneg(chk, x, sol, xp):
    alpha, a1, a2 = ALGS["GAP(0.3,1.2,1.7)"]
    t1, t2, _ = chk.reference(x, sol, alpha, a1, a2)
    k = 6 + int(np.argmax(np.abs(t1[6:10])))                     # K2 = [Free 6, NonNeg 4, ...]: primal copy in the first half
    assert t1[k] != 0.0
    t2[k] = min(t1[k], 0.0)
    return _finish(t1, t2, x, alpha, a2)


def _wrong_last_psd_entry(chk, x, sol, xp):
    s, ln = chk.psd_segments[-1]
    k = chk.l + s + ln - 1                                       # primal copy of the last PSD cone, last entry
    out = xp.copy()
    assert out[k] != x[k]
    out[k] = x[k]
    return out


def _wrong_tau_kappa(chk, x, sol, xp):
    out = xp.copy()
    assert out[chk.l - 1] != x[chk.l - 1] or out[2 * chk.l - 1] != x[2 * chk.l - 1]
    out[chk.l - 1], out[2 * chk.l - 1] = x[chk.l - 1], x[2 * chk.l - 1]
    return out


WRONG = {"a1-alpha2-exchanged": (_wrong_swapped, None), "dual-psd-wrong-sign": (_wrong_dual_sign, "psd"), "nonneg-as-nonpos": (_wrong_nonneg, "ew"),
         "last-psd-entry-stale": (_wrong_last_psd_entry, "psd"), "tau-kappa-untouched": (_wrong_tau_kappa, "ew")}


@pytest.mark.parametrize("what", list(WRONG))
def test_wrong_steps_are_rejected(mixed, asym_step, what):
    _, chk = mixed
    x, sol, xp, i = asym_step
    alpha, a1, a2 = ALGS["GAP(0.3,1.2,1.7)"]
    make, where = WRONG[what]
    res = chk.check(x, sol, make(chk, x, sol, xp), alpha, a1, a2, i)
    print(what, "->", res)
    assert not res.ok
    if where == "psd":
        assert not res.psd_ok and res.ew_ok
    elif where == "ew":
        assert not res.ew_ok and res.psd_ok
    else:
        assert not res.psd_ok and not res.ew_ok
    assert res.affine_ok                                         # (x and sol are the true ones)


def test_affine_residual_bites(mixed, asym_step):
    """a sol that belongs to another x fails the residual check of the affine projection"""
    _, chk = mixed
    x, sol, xp, i = asym_step
    alpha, a1, a2 = ALGS["GAP(0.3,1.2,1.7)"]
    bad = sol.copy()
    bad[chk.l + 3] += 1.0
    res = chk.check(x, bad, xp, alpha, a1, a2, i)
    assert not res.affine_ok
    # and the residual itself agrees with the oracle's operator
    M = orc.KKTMatrix(orc.HSDEMatrixQ(mixed[0].A, mixed[0].b, mixed[0].c))
    y = np.empty_like(sol)
    M.mul(y, sol)
    q = np.empty(chk.l)
    orc.HSDEMatrixQ(mixed[0].A, mixed[0].b, mixed[0].c).mul_t(q, x[chk.l:])
    rhs = np.concatenate([x[:chk.l] + q, np.zeros(chk.l)])
    r, allowance = chk.affine_residual(x, sol)
    assert abs(r - np.linalg.norm(y - rhs)) <= allowance
