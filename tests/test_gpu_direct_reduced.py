"""
direct = true, reduced form on the device (HSDE.jl:12-15; csrc/direct_reduced.hip): the exact projection through the inverse of I + A'A or I + A A' alone
(order min(m, n)), kept as tiles of its lower triangle and read once per application.  The cases and tolerances mirror tests/test_gpu_direct.py.
"""
import sys
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp

import fos_oracle as orc
from test_gpu_direct import _omodel, scrambled_block_problem

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tools"))
from direct_reduced_bench import time_projections

pytestmark = pytest.mark.gpu


def _rect_problem(pkg, m, n, seed):
    """a sparse LP-shaped program of the given shape (about 6 entries per column, every row touched)"""
    rng = np.random.default_rng(seed)
    A = sp.random(m, n, density=min(1.0, 6.0 / m), format="csc", random_state=rng, data_rvs=rng.standard_normal) + \
        sp.csc_matrix((rng.standard_normal(m), (np.arange(m), rng.integers(0, n, m))), shape=(m, n))
    A = sp.csc_matrix(A)
    A.sort_indices()
    x0, s0 = np.abs(rng.standard_normal(n)), np.abs(rng.standard_normal(m))
    return pkg.workloads.ConicProblem("rect", A, A @ x0 + s0, rng.standard_normal(n), [("NonNeg", m)], [("NonNeg", n)], x0=x0, y0=np.zeros(m), s0=s0)


PROBLEMS = {
    "small_mixed": lambda pkg: pkg.workloads.small_mixed(),
    "small_lp": lambda pkg: pkg.workloads.small_lp(seed=3, m=31, n=61),
    "tile_lp": lambda pkg: pkg.workloads.small_lp(seed=21, m=96, n=180),
    "block_sdp": lambda pkg: pkg.workloads.c4_block_sdp(nblocks=8, k=16, p=6),
    "scrambled": lambda pkg: scrambled_block_problem(pkg),
    "m<n": lambda pkg: _rect_problem(pkg, 150, 400, 1),
    "n<m": lambda pkg: _rect_problem(pkg, 400, 150, 2),
}


@pytest.mark.parametrize("which", list(PROBLEMS))
def test_reduced_projection_matches_oracle_and_is_exact(pkg, which):
    prob = PROBLEMS[which](pkg)
    d = pkg.HipHSDE(prob.A, prob.b, prob.c, prob.K1, prob.K2)
    d.enable_direct(prob.A, form="reduced")
    assert d.direct_mode() == "reduced"
    st = d.direct_stats()
    assert st["form"] == "reduced" and st["k"] == min(prob.A.shape) and st["ns_steps"] > 0 and st["setup_s"] > 0.0
    S1 = orc.IndAffineDirect(orc.HSDEMatrixQ(prob.A, prob.b, prob.c))
    rng = np.random.default_rng(9)
    l = d.l
    cond = np.linalg.cond(np.eye(l) + S1.Qd @ S1.Qd.T)
    for scale in (1.0, 1e3):
        x = scale * rng.standard_normal(d.N)
        y = d.prox_affine(x)
        assert d.cgiter() == 0
        ref = np.empty(d.N)
        S1.prox(ref, x)
        print(which, scale, "rel err", np.linalg.norm(y - ref) / np.linalg.norm(ref), "cond", cond)
        assert np.linalg.norm(y - ref) <= 1e-12 * np.linalg.norm(ref) * max(1.0, cond / 1e3)
        assert np.linalg.norm(d.q_apply(y[:l]) - y[l:]) <= 1e-12 * np.linalg.norm(y)
        u = rng.standard_normal(l)
        t = np.concatenate([u, d.q_apply(u)])
        assert abs((x - y) @ t) <= 1e-11 * np.linalg.norm(t) * np.linalg.norm(x)
    d.close()


def test_reduced_projection_is_bit_identical(pkg):
    prob = pkg.workloads.small_lp(seed=21, m=96, n=180)
    x = np.random.default_rng(3).standard_normal(2 * (96 + 180 + 1))
    ys = []
    for _ in range(2):
        d = pkg.HipHSDE(prob.A, prob.b, prob.c, prob.K1, prob.K2)
        d.enable_direct(prob.A, form="reduced")
        ys.append(d.prox_affine(x))
        ys.append(d.prox_affine(x))
        d.close()
    for y in ys[1:]:
        assert np.array_equal(y, ys[0])


@pytest.mark.parametrize("algname", ["DR", "GAPA", "FISTA"])
def test_reduced_whole_solve_matches_oracle(pkg, algname):
    prob = pkg.workloads.small_mixed()
    mk = {"DR": lambda M, **o: M.DR(**o), "GAPA": lambda M, **o: M.GAPA(0.8, 0.5, **o), "FISTA": lambda M, **o: M.FISTA(**o)}[algname]
    opts = dict(eps=1e-6, verbose=1, max_iters=3000 if algname != "FISTA" else 300, checki=50, direct=True)
    out = []
    model = pkg.solve(prob, mk(pkg, direct_form="reduced", **opts), out=out)
    assert model.data.direct_mode() == "reduced"
    oout = []
    sol = orc.solve(_omodel(prob), mk(orc, **opts), out=oout)
    assert out[2] == " Iter | pri res | dua res | rel gap | pri obj | dua obj | kap/tau | time" == oout[2]
    assert "cgiter" not in model.history
    assert model.status() == sol.status and model.iterations == sol.iterations
    last, olast = model.status_obj.last, sol.status_obj.last
    for key in ("p", "d", "g"):
        assert getattr(last, key) == pytest.approx(olast[key], rel=1e-6, abs=1e-12)
    assert np.max(np.abs(model.getsolution() - sol.x)) <= 1e-9 * max(1.0, np.max(np.abs(sol.x)))


def test_reduced_agrees_with_the_dense_form(pkg, monkeypatch):
    prob = pkg.workloads.c2_lp(m=300, n=600, scale=25.0)
    x = np.random.default_rng(8).standard_normal(2 * (300 + 600 + 1))
    dr = pkg.HipHSDE(prob.A, prob.b, prob.c, prob.K1, prob.K2)
    dr.enable_direct(prob.A, form="reduced")
    yr = dr.prox_affine(x)
    # the same handle switched to the dense form and back: neither form's inverse survives the other
    monkeypatch.setenv("FOS_DIRECT_MODE", "dense")
    dr.enable_direct(prob.A)
    assert dr.direct_mode() == "dense"
    yd = dr.prox_affine(x)
    monkeypatch.delenv("FOS_DIRECT_MODE")
    dr.disable_direct()
    assert dr.direct_mode() == "off"
    dr.enable_direct(prob.A, form="reduced")
    assert dr.direct_mode() == "reduced"
    assert np.array_equal(dr.prox_affine(x), yr)
    dr.close()
    print("reduced vs dense", np.linalg.norm(yr - yd) / np.linalg.norm(yd))
    assert np.linalg.norm(yr - yd) <= 1e-11 * np.linalg.norm(yd)
    opts = dict(eps=1e-6, verbose=0, max_iters=6000, checki=100, direct=True)
    mr = pkg.solve(prob, pkg.DR(direct_form="reduced", **opts))
    monkeypatch.setenv("FOS_DIRECT_MODE", "dense")
    md = pkg.solve(prob, pkg.DR(**opts))
    assert mr.data.direct_mode() == "reduced" and md.data.direct_mode() == "dense"
    assert mr.status() == md.status()
    assert mr.getobjval() == pytest.approx(md.getobjval(), rel=1e-4, abs=1e-6)


def test_mode_switch_through_the_environment(pkg, monkeypatch):
    prob = pkg.workloads.small_lp(seed=3, m=31, n=61)
    d = pkg.HipHSDE(prob.A, prob.b, prob.c, prob.K1, prob.K2)
    monkeypatch.setenv("FOS_DIRECT_MODE", "reduced")
    d.enable_direct(prob.A)
    assert d.direct_mode() == "reduced"
    d.close()


def test_refusals_leave_a_working_handle(pkg, monkeypatch, fullsize):
    def refused(d, A):
        with pytest.raises(pkg.lib.FosError) as ei:
            d.enable_direct(A, form="reduced")
        assert ei.value.code == -4 and "reduced" in str(ei.value)          # FOS_EUNSUPPORTED
        assert d.direct_mode() == "off"

    prob = pkg.workloads.small_mixed()
    S1 = orc.IndAffineDirect(orc.HSDEMatrixQ(prob.A, prob.b, prob.c))
    x = np.random.default_rng(2).standard_normal(2 * (sum(prob.A.shape) + 1))
    ref = np.empty(x.size)
    S1.prox(ref, x)
    # a forced small cap
    d = pkg.HipHSDE(prob.A, prob.b, prob.c, prob.K1, prob.K2)
    monkeypatch.setenv("FOS_DIRECT_REDUCED_MAX", "10")
    refused(d, prob.A)
    monkeypatch.delenv("FOS_DIRECT_REDUCED_MAX")
    y = None
    for _ in range(400):                                     # the CG path, its tolerance schedule advanced to the floor
        y = d.prox_affine(x)
    assert np.linalg.norm(y - ref) <= 1e-9 * np.linalg.norm(ref)
    d.close()
    # a sharded handle (a one-rank communicator)
    d = pkg.HipHSDE(prob.A, prob.b, prob.c, prob.K1, prob.K2)
    d.comm_init(1, 0, pkg.HipHSDE.comm_unique_id())
    refused(d, prob.A)
    d.close()
    # C5: k = min(m, n) is past the cap
    p5 = fullsize("C5")
    assert min(p5.A.shape) > 46000
    d = pkg.HipHSDE(p5.A, p5.b, p5.c, p5.K1, p5.K2)
    refused(d, p5.A)
    x5 = np.random.default_rng(1).standard_normal(d.N)
    y5 = d.prox_affine(x5)
    assert np.all(np.isfinite(y5)) and d.cgiter() > 0
    d.close()


@pytest.fixture(scope="module")
def c3_reduced(pkg, fullsize):
    prob = fullsize("C3")
    d = pkg.HipHSDE(prob.A, prob.b, prob.c, prob.K1, prob.K2)
    d.enable_direct(prob.A, form="reduced")
    yield prob, d
    d.close()


def test_c3_reduced_certificate(pkg, c3_reduced, fullsize):
    """C3 (m = 50 000, n = 20 000): the oracle-free certificate of the exact projection at 1e-12, two inputs; the default form of the same problem is still cg.
    Measured on one MI355X (one refinement step, the default): see DESIGN.md section 7."""
    prob, d = c3_reduced
    assert d.direct_mode() == "reduced" and d.direct_stats()["k"] == 20000
    print("C3 reduced set-up", d.direct_stats())
    x = np.random.default_rng(1).standard_normal(d.N)
    l = d.l
    for rep in range(2):
        y = d.prox_affine(x)
        assert d.cgiter() == 0
        on_set = np.linalg.norm(d.q_apply(y[:l]) - y[l:])
        in_range = np.linalg.norm((x[:l] - y[:l]) - d.q_apply(y[l:] - x[l:], transpose=True))
        print("C3 certificate", rep, on_set / np.linalg.norm(x), in_range / np.linalg.norm(x))
        assert on_set + in_range <= 1e-12 * np.linalg.norm(x), (rep, on_set, in_range)
        x = x + 1e-3 * np.random.default_rng(2).standard_normal(d.N)
    dd = pkg.HipHSDE(prob.A, prob.b, prob.c, prob.K1, prob.K2)
    dd.enable_direct(prob.A)
    assert dd.direct_mode() == "cg"
    dd.close()


def test_c3_reduced_is_at_least_twice_as_fast_as_cg(pkg, c3_reduced, monkeypatch):
    """per projection, warm, median of 24 projections each, both timed by tools/direct_reduced_bench.time_projections"""
    prob, d = c3_reduced
    tr = float(np.median(time_projections(d, 24)))
    dc = pkg.HipHSDE(prob.A, prob.b, prob.c, prob.K1, prob.K2)
    dc.enable_direct(prob.A)
    assert dc.direct_mode() == "cg"
    tc = float(np.median(time_projections(dc, 24)))
    print("C3 per projection: reduced %.3f ms, cg %.3f ms (%d CG iterations in the last one), ratio %.3f" % (1e3 * tr, 1e3 * tc, dc.cgiter(), tr / tc))
    dc.close()
    assert tr <= 0.5 * tc
