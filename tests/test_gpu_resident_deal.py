"""
GPU tests of the streamed resident CG solve (csrc/resident.hip, cg_stream_kernel) at the workgroup tile counts where its DEAL of tiles to
wavefronts changes shape (csrc/fos_internal.hpp, rs_deal): fewer tiles than wavefronts (1, 7), the communication wavefront's share going from
nothing to one tile to its full six (8, 9, 58, 59, 60), C4's own 66 and the LDS cap of 69 -- one 32-column unit on ONE workgroup each -- and a
workgroup of two units with 64-step tiles.

Per operator: the iterate after 1, 2 and 5 iterations against the oracle's merged recurrence and the launch-per-iteration kernels of the same
recurrence, and the solve to the tolerance floor against dense linear algebra, at the tolerances of
test_gpu_resident.py::test_resident_cg_matches_oracle_merged_update_and_dense_solve; equal iteration counts of the two device recurrences; a
warm-started second solve (the start sweep r_0 = rhs - M v, with a v that is not the first one); solves capped at one and at two iterations (the
exchange rounds that carry r.r alone, and the round that stops: no tile is requested ahead of either).
"""
import math
import warnings

import numpy as np
import pytest
import scipy.linalg as sla
import scipy.sparse as sp

import fos_oracle as orc

pytestmark = pytest.mark.gpu


def relerr(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(1e-300, np.linalg.norm(b)))


def _ocg(fn, M, x0, rhs, tol, maxit):
    N = x0.shape[0]
    x = x0.copy()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        it = fn(x, M, rhs, *[np.empty(N) for _ in range(4 if fn is orc.conjugategradient_merged else 3)], tol=tol, max_iters=maxit)
    return x, it


def _dense_solve(Q, rhs, l):
    """[[I, Q'], [Q, -I]] x = rhs by dense linear algebra: the Schur complement (I + Q'Q) x1 = rhs1 + Q' rhs2 (Cholesky), x2 = Q x1 - rhs2, and one
    step of refinement against the full system."""
    Qs = sp.csr_matrix(np.asarray(Q.todense()))
    F = sla.cho_factor(np.eye(l) + (Qs.T @ Qs).toarray())

    def solve(r):
        x1 = sla.cho_solve(F, r[:l] + Qs.T @ r[l:])
        return np.concatenate([x1, Qs @ x1 - r[l:]])

    def mul(x):
        return np.concatenate([x[:l] + Qs.T @ x[l:], Qs @ x[:l] - x[l:]])

    x = solve(rhs)
    return x + solve(rhs - mul(x)), mul


def _decisive_tolerance(M, mul, x0, rhs):
    """A tolerance at which the stopping iteration is not a matter of rounding, from the ORACLE's iterates alone.  CG on this indefinite system does
    not contract monotonically: its spectrum is symmetric about zero, odd iterations may grow the residual, and near such a step the residual of
    iteration k differs between recurrences by factors (the launch-per-iteration kernels and the streamed solve of the parent commit stop one
    iteration apart at 1e-6 on the 60-tile operator, where three recurrences give 0.5e-6, 1.1e-6 and 4.2e-6 at iteration 18 and agree to six
    digits at 16 and at 20).  So: the iteration k in 6 .. 24 whose residual falls furthest below every earlier one, the tolerance halfway (in the
    logarithm) between the two.  Returns (tol, k)."""
    res = []
    for k in range(1, 25):
        xo, _ = _ocg(orc.conjugategradient_merged, M, x0, rhs, 1e-300, k)
        res.append(float(np.linalg.norm(mul(xo) - rhs)))
    best = max(range(6, 25), key=lambda k: min(res[:k - 1]) / res[k - 1])
    return math.sqrt(min(res[:best - 1]) * res[best - 1]), best


# (name, block shapes, tiles of the one workgroup, steps per tile): a ragged last tile everywhere
def _one_unit(tiles):
    return ("tiles-%d" % tiles, [(64 * (tiles - 1) + 40, 32)], tiles, 32)


CASES = [_one_unit(t) for t in (1, 7, 8, 9, 58, 59, 60, 66, 69)] + [("two-units-wide-tiles", [(64 * 9 + 30, 40), (64 * 4, 20)], 14, 64)]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_streamed_deal_matches_merged_update_and_dense_solve(pkg, case, monkeypatch):
    name, shapes, tiles, steps = case
    monkeypatch.setenv("FOS_RESIDENT_GMAX", "1")
    monkeypatch.setenv("FOS_RESIDENT_STREAM", "2")
    rng = np.random.default_rng(5100 + tiles + steps)
    A = sp.block_diag([sp.csc_matrix(rng.standard_normal((r, c)) / math.sqrt(r)) for r, c in shapes], format="csc")
    m, n = A.shape
    b, c = rng.standard_normal(m), rng.standard_normal(n)
    d = pkg.HipHSDE(A, b, c, [("Free", m)], [("Free", n)])
    st = d.resident_stats()
    assert st["qualifies"] == 1 and st["form"] == "streamed" and st["workgroups"] == 1, st
    assert st["max_tiles_per_workgroup"] == tiles and st["steps_per_tile"] == steps, st
    Q = orc.HSDEMatrixQ(A, b, c)
    M = orc.KKTMatrix(Q)
    rhs, x0 = rng.standard_normal(d.N), rng.standard_normal(d.N)
    xs, mul = _dense_solve(Q, rhs, d.l)

    def both(start, tol, maxit):
        d.set_cg_variant("resident")
        assert d.cg_variant_name() == "resident"
        xk, it = d.cg_kkt(start, rhs, tol, maxit)
        d.set_cg_variant("merged_update")
        xm, itm = d.cg_kkt(start, rhs, tol, maxit)
        return xk, it, xm, itm

    # first iterations, the caps at one and two among them: the oracle's merged recurrence (in the envelope of its distance to the reference
    # recurrence) and the launch-per-iteration kernels of the same recurrence
    for k in (1, 2, 5):
        xk, it, xm, itm = both(x0, 1e-300, k)
        xo, ito = _ocg(orc.conjugategradient_merged, M, x0, rhs, 1e-300, k)
        xr, _ = _ocg(orc.conjugategradient, M, x0, rhs, 1e-300, k)
        assert it == ito == itm == k, (name, k, it, itm)
        env = max(1e-14, relerr(xr, xo))
        print("%s k=%d: vs oracle %.3g, vs merged_update %.3g, envelope %.3g" % (name, k, relerr(xk, xo), relerr(xk, xm), env))
        assert relerr(xk, xo) <= 50 * env, (name, k, relerr(xk, xo), env)
        assert relerr(xk, xm) <= 50 * env, (name, k, relerr(xk, xm), env)
    # a tolerance the solve reaches: the same number of iterations in both device recurrences, the oracle's
    tol_d, k_d = _decisive_tolerance(M, mul, x0, rhs)
    xk, it, xm, itm = both(x0, tol_d, 10000)
    print("%s tol %.3g: %d / %d iterations (oracle %d), residual %.3g" % (name, tol_d, it, itm, k_d, np.linalg.norm(mul(xk) - rhs)))
    assert it == itm == k_d, (name, it, itm, k_d)
    assert np.linalg.norm(mul(xk) - rhs) <= tol_d * (1 + 1e-6), name
    # the tolerance floor: the dense solution
    tol = d.N * np.finfo(float).eps
    d.set_cg_variant("resident")
    x, it = d.cg_kkt(x0, rhs, tol, 10000)
    print("%s floor: %d iterations, vs dense %.3g" % (name, it, relerr(x, xs)))
    assert relerr(x, xs) < 1e-11, (name, relerr(x, xs))
    # warm start: a second solve from the loose solution -- the start sweep with another v, the rhs rows read again -- to a tolerance that is
    # again decisive for the oracle started there.  The system's singular values are sqrt(1 + sigma(Q)^2) >= 1, so a residual within tol is an
    # error within tol (twice that: the recursively updated residual drifts from the true one by rounding, orders of magnitude below)
    tol_w, k_w = _decisive_tolerance(M, mul, xk, rhs)
    xw, itw, xwm, itwm = both(xk, tol_w, 10000)
    print("%s warm, tol %.3g: %d / %d iterations (oracle %d), error %.3g" % (name, tol_w, itw, itwm, k_w, np.linalg.norm(xw - xs)))
    assert itw == itwm == k_w, (name, itw, itwm, k_w)
    assert np.linalg.norm(xw - xs) <= 2 * tol_w, (name, np.linalg.norm(xw - xs), tol_w)
    d.set_cg_variant("resident")
    x2, it2 = d.cg_kkt(xk, rhs, tol_w, 10000)
    assert it2 == itw and np.array_equal(xw, x2), name                 # bit-reproducible
    d.close()
