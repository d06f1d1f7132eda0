"""
GPU tests of the streamed resident CG solve's GROUP-MAJOR walk (csrc/resident.hip: rs_sweep, rs_group, res_tile_plain): a wavefront walks its tiles
one column group of eight steps at a time, adds its products per lane over the consecutive tiles of a unit (a segment), reduces the lanes once per
(segment, group, right-hand side) and STORES the column sums; RS_RING chunks of 4 KB are in flight across tile and group boundaries.  The shapes
are the ones at which that walk takes another path, one workgroup each unless said otherwise, a ragged last tile everywhere:

* one unit of 32 columns in 1, 2, 9 and 15 tiles -- wavefronts with 0, 1 and 2 tiles, rings shorter than RS_RING;
* one unit of 8, 20 and 32 columns (1, 3, 4 groups) and of 40 and 64 columns (64-step tiles: 5 and 8 groups);
* five units of 3 tiles and 12 columns each: wavefronts whose two tiles straddle a unit boundary (two segments), column offsets 0 .. 48;
* seven units of 1 tile and 8 columns each: every tile a segment of its own;
* 40 + 20 columns in one workgroup (test_gpu_resident_deal.py's wide-tile shape): segments of different widths in one walk;
* eight units of 32 columns over four workgroups (FOS_RESIDENT_GMAX=4, full groups only): the four sums cross workgroups.

Method and tolerances of test_gpu_resident_deal.py: the iterate after 1, 2 and 5 iterations against the oracle's merged recurrence and against the
launch-per-iteration kernels of the same recurrence (merged_update) within 50 x the envelope (the oracle's own distance between its two
recurrences, at least 1e-14); equal iteration counts of both device recurrences and the oracle at a decisive tolerance; the tolerance floor against
the dense solve below 1e-11; a warm-started second solve; a repeated solve bit for bit (the summation order is fixed: per lane over tiles in tile
order, tile_colsum8's lane order, wavefronts in order).  The plan of every case is asserted through resident_stats().
"""
import math

import numpy as np
import pytest
import scipy.sparse as sp

import fos_oracle as orc
from test_gpu_resident_deal import _decisive_tolerance, _dense_solve, _ocg, relerr

pytestmark = pytest.mark.gpu


def _ragged(tiles, cols):
    """One unit of `cols` columns in `tiles` tiles of 64 rows, the last of 40."""
    return (64 * (tiles - 1) + 40, cols)


# (name, block shapes, FOS_RESIDENT_GMAX, workgroups, units, tiles of the largest workgroup, steps per tile)
CASES = [("32-cols-%d-tiles" % t, [_ragged(t, 32)], 1, 1, 1, t, 32) for t in (1, 2, 9, 15)]
CASES += [("%d-cols" % c, [_ragged(3, c)], 1, 1, 1, 3, 32 if c <= 32 else 64) for c in (8, 20, 32, 40, 64)]
CASES += [("five-units-straddled", [_ragged(3, 12)] * 5, 1, 1, 5, 15, 32),
          ("seven-single-tile-units", [_ragged(1, 8)] * 7, 1, 1, 7, 7, 32),
          ("two-units-wide-tiles", [(64 * 9 + 30, 40), (64 * 4, 20)], 1, 1, 2, 14, 64),
          ("eight-units-four-workgroups", [_ragged(2, 32)] * 8, 4, 4, 8, 4, 32)]


def _instance(shapes, seed):
    """A random block-diagonal problem of the given block shapes with a start and a right-hand side, and its decisive tolerance.  The instance is
    screened BY THE ORACLE ALONE (no device result enters): seeds seed, seed + 1000, ... are drawn until the decisive iteration lies inside the
    window _decisive_tolerance searches (k < 24: at the window's edge the tolerance may sit in the middle of a longer fall) and the tolerance is no
    smaller than 1e-5 of the largest residual norm of the oracle's run -- or the residual falls by 1e3 at the decisive iteration, which leaves a
    factor of 30 on either side of the tolerance (a narrow unit: the Krylov space is exhausted there).  Reason: the recurrences compared here differ by rounding alone, and on
    this indefinite system rounding differences grow with the residual norms the iteration passed through; test_gpu_resident_deal.py records
    factors of 8 between three recurrences at residual 1e-6.  On the first instance drawn for 15 tiles (decisive iteration 24, tolerance 2.8e-7
    after residuals of order 10) the launch-per-iteration kernels, which this change does not touch, stop at 22 where the oracle stops at 24: that
    instance decides nothing."""
    for draw in range(50):
        rng = np.random.default_rng(seed + 1000 * draw)
        A = sp.block_diag([sp.csc_matrix(rng.standard_normal((r, c)) / math.sqrt(r)) for r, c in shapes], format="csc")
        m, n = A.shape
        b, c = rng.standard_normal(m), rng.standard_normal(n)
        Q = orc.HSDEMatrixQ(A, b, c)
        M = orc.KKTMatrix(Q)
        N = 2 * (m + n + 1)
        rhs, x0 = rng.standard_normal(N), rng.standard_normal(N)
        xs, mul = _dense_solve(Q, rhs, m + n + 1)
        tol_d, k_d = _decisive_tolerance(M, mul, x0, rhs)
        res = [float(np.linalg.norm(mul(_ocg(orc.conjugategradient_merged, M, x0, rhs, 1e-300, k)[0]) - rhs)) for k in range(1, k_d + 1)]
        if k_d < 24 and (tol_d >= 1e-5 * max(res) or min(res[:-1]) >= 1e3 * res[-1]):
            return A, b, c, rhs, x0, Q, M, xs, mul, tol_d, k_d
    raise AssertionError("no decisive instance in 50 draws")


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_streamed_group_major_walk_matches_merged_update_and_dense_solve(pkg, case, monkeypatch):
    name, shapes, gmax, workgroups, units, tiles, steps = case
    monkeypatch.setenv("FOS_RESIDENT_GMAX", str(gmax))
    monkeypatch.setenv("FOS_RESIDENT_STREAM", "2")
    A, b, c, rhs, x0, Q, M, xs, mul, tol_d, k_d = _instance(shapes, 7300 + 31 * len(shapes) + tiles + steps + shapes[0][1])
    m, n = A.shape
    d = pkg.HipHSDE(A, b, c, [("Free", m)], [("Free", n)])
    st = d.resident_stats()
    assert st["qualifies"] == 1 and st["form"] == "streamed" and st["workgroups"] == workgroups and st["units"] == units, st
    assert st["max_tiles_per_workgroup"] == tiles and st["steps_per_tile"] == steps, st
    assert rhs.shape[0] == d.N and d.l == m + n + 1

    def both(start, tol, maxit):
        d.set_cg_variant("resident")
        assert d.cg_variant_name() == "resident"
        xk, it = d.cg_kkt(start, rhs, tol, maxit)
        d.set_cg_variant("merged_update")
        xm, itm = d.cg_kkt(start, rhs, tol, maxit)
        return xk, it, xm, itm

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
    # warm start: a second solve from the loose solution, to a tolerance that is again decisive for the oracle started there (a residual within tol
    # is an error within tol: the system's singular values are >= 1; twice that for the drift of the recursively updated residual)
    tol_w, k_w = _decisive_tolerance(M, mul, xk, rhs)
    xw, itw, xwm, itwm = both(xk, tol_w, 10000)
    print("%s warm, tol %.3g: %d / %d iterations (oracle %d), error %.3g" % (name, tol_w, itw, itwm, k_w, np.linalg.norm(xw - xs)))
    assert itw == itwm == k_w, (name, itw, itwm, k_w)
    assert np.linalg.norm(xw - xs) <= 2 * tol_w, (name, np.linalg.norm(xw - xs), tol_w)
    # a repeated solve: the same bits
    d.set_cg_variant("resident")
    x2, it2 = d.cg_kkt(xk, rhs, tol_w, 10000)
    assert it2 == itw and np.array_equal(xw, x2), name
    d.close()
