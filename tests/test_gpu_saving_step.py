"""
A saving iteration of the LongstepWrapper that does not close its window leaves the same bits as the plain iteration.

Both run ONE description of the algorithm (step_desc in csrc/step.cpp): the plain step hands everything behind S1 to the solve as gated `post` work, the
saving iteration runs the same launches ungated and takes its two planes in between (long_begin / long_finish).  Taking a plane reads the vectors and
writes only the wrapper's own buffers, so up to the iteration that projects onto the saved planes the two handles must agree in every bit.

LongstepWrapper(alg, longinterval=8, nsave=3): by long_window (wrappers.hpp) iterations 1-4 are plain, 5-7 save planes, iteration 8 saves and projects.
Both handles run the exact projection (enable_direct: no CG stop enters) with FOS_PSD_FUSE=0 and FOS_RELAX_EW=0, so that the plain step runs the plain
relaxation -- the fused forms of GAP / GAPA round differently and a saving iteration never takes them.

The test also passes on the library that kept a second copy of every algorithm for the saving iteration (DESIGN_LOG.md, "The outer iteration"): it pins
behaviour, it did not change any.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LONGINTERVAL, NSAVE = 8, 3
FIELDS = ("p", "d", "g", "ctx", "bty", "kappa", "tau", "norm_axs", "norm_aty", "norm_b", "norm_c", "cgiter", "status", "cg_maxiter_hit")


@pytest.fixture(scope="module")
def problem(pkg):
    return pkg.workloads.small_mixed()


def algorithms(pkg):
    return {"DR": lambda: pkg.DR(direct=True), "GAPA": lambda: pkg.GAPA(0.8, 0.5, direct=True),
            "FISTA": lambda: pkg.FISTA(direct=True), "Dykstra": lambda: pkg.Dykstra(direct=True)}


def bits(v):
    return np.float64(v).tobytes()


@pytest.mark.parametrize("checki", [1, 1000])
@pytest.mark.parametrize("algname", ["DR", "GAPA", "FISTA", "Dykstra"])
def test_saving_iteration_equals_plain_iteration(pkg, problem, monkeypatch, algname, checki):
    monkeypatch.setenv("FOS_PSD_FUSE", "0")
    monkeypatch.setenv("FOS_RELAX_EW", "0")
    handles = []
    try:
        for wrap in (False, True):
            d = pkg.HipHSDE(problem.A, problem.b, problem.c, problem.K1, problem.K2)
            handles.append(d)
            d.enable_direct(problem.A)
            alg = algorithms(pkg)[algname]()
            d.set_alg(pkg.LongstepWrapper(alg, longinterval=LONGINTERVAL, nsave=NSAVE) if wrap else alg)
            d.set_iterate(None)
        plain, saving = handles
        for i in range(1, LONGINTERVAL):                     # 1-4 plain on both, 5-7 saving on the wrapped handle
            (_, ca, ra), (_, cb, rb) = plain.step(i, 1, checki, 1e-30), saving.step(i, 1, checki, 1e-30)
            assert np.array_equal(plain.get_iterate(), saving.get_iterate()), "iterate after step %d" % i
            assert ca == cb == (checki == 1)
            if ca:
                for f in FIELDS:
                    assert bits(getattr(ra, f)) == bits(getattr(rb, f)), "check result of step %d: %s = %r / %r" % (i, f, getattr(ra, f), getattr(rb, f))
        (ya, qa, ta, a12a), (yb, qb, tb, a12b) = plain.get_alg_state(), saving.get_alg_state()
        assert np.array_equal(ya, yb) and np.array_equal(qa, qb) and bits(ta) == bits(tb) and bits(a12a) == bits(a12b)
        saving.step(LONGINTERVAL, 1, checki, 1e-30)          # the window closes: had it never opened, the log would not name this iteration
        assert saving.longstep_log()["iteration"] == LONGINTERVAL
    finally:
        for d in handles:
            d.close()
