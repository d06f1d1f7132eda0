"""
GPU tests of the streamed resident CG solve (csrc/resident.hip, cg_stream_kernel) on workgroups of SEVERAL units at the tile counts where the deal
table (csrc/fos_internal.hpp, rs_deal) has its edges, with the compute wavefronts holding [c; b] of their rows in registers for the whole solve
(instances with NT <= 9) -- the rows' epilogue of every sweep, the start's r_0 = rhs - M v and the capped solves all read it.

Block-diagonal operators of four units of 32 columns on TWO workgroups (FOS_RESIDENT_GMAX=2): the first holds two tall units of different heights,
so a segment boundary falls inside a wavefront's tiles, the second two one-tile units (wavefronts without tiles beside the communication wavefront's);
every unit ends on a ragged tile of 40 rows.  Tiles of the first workgroup:

* 66 = 33 + 33: the flagship's shape, 9 9 9 9 8 8 8 + 6 -- the unit boundary inside compute wavefront 3;
* 67 = 34 + 33 and 69 = 35 + 34: the first counts that launch cg_stream_kernel<32, 10>, which reads [c; b] in the sweep (9 9 9 9 9 8 8 + 6, 9 x 7 + 6);
* 9 = 5 + 4 and 15 = 8 + 7: one and two tiles per compute wavefront, 2 and 1 for the communication wavefront.

(The rule hands no compute wavefront 10 tiles at any count up to the LDS cap of 69: no table with a 10-tile wavefront measured faster on the
flagship shape, DESIGN_LOG.md, so there is no such edge to test.)

Method, screening and tolerances are test_gpu_resident_colsum.py's: instances screened by the oracle alone for a decisive tolerance; the iterate after
1, 2 and 5 iterations (capped solves) against the oracle's merged recurrence and the launch-per-iteration kernels of the same recurrence within 50 x
the envelope, and within 1e-9 relative outright; equal iteration counts at the decisive tolerance; the tolerance floor against the dense solve; a
warm-started second solve (the start's rhs - M v with another v; rhs is random on every row, the ragged tiles' rows included); a repeated solve bit
for bit.
"""
import numpy as np
import pytest

import fos_oracle as orc
from test_gpu_resident_colsum import _instance
from test_gpu_resident_deal import _decisive_tolerance, _ocg, relerr

pytestmark = pytest.mark.gpu


def _unit(tiles):
    return (64 * (tiles - 1) + 40, 32)


# (name, tiles of the four units, tiles of the first workgroup)
CASES = [("66-tiles", (33, 33, 1, 1), 66), ("67-tiles", (34, 33, 1, 1), 67), ("69-tiles", (35, 34, 1, 1), 69), ("9-tiles", (5, 4, 1, 1), 9),
         ("15-tiles", (8, 7, 1, 1), 15)]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_streamed_multi_unit_workgroups_match_merged_update_and_dense_solve(pkg, case, monkeypatch):
    name, unit_tiles, tiles = case
    monkeypatch.setenv("FOS_RESIDENT_GMAX", "2")
    monkeypatch.setenv("FOS_RESIDENT_STREAM", "2")
    shapes = [_unit(t) for t in unit_tiles]
    A, b, c, rhs, x0, Q, M, xs, mul, tol_d, k_d = _instance(shapes, 9100 + tiles)
    m, n = A.shape
    d = pkg.HipHSDE(A, b, c, [("Free", m)], [("Free", n)])
    st = d.resident_stats()
    assert st["qualifies"] == 1 and st["form"] == "streamed" and st["workgroups"] == 2 and st["units"] == 4, st
    assert st["max_tiles_per_workgroup"] == tiles and st["steps_per_tile"] == 32, st
    assert st["tiles_per_wave"] == (10 if tiles >= 67 else 9 if tiles > 38 else 3), st            # (NT of the instance: 10 reads [c; b] in the sweep)

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
        assert relerr(xk, xo) <= min(1e-9, 50 * env), (name, k, relerr(xk, xo), env)
        assert relerr(xk, xm) <= min(1e-9, 50 * env), (name, k, relerr(xk, xm), env)
    xk, it, xm, itm = both(x0, tol_d, 10000)
    print("%s tol %.3g: %d / %d iterations (oracle %d), residual %.3g" % (name, tol_d, it, itm, k_d, np.linalg.norm(mul(xk) - rhs)))
    assert it == itm == k_d, (name, it, itm, k_d)
    assert np.linalg.norm(mul(xk) - rhs) <= tol_d * (1 + 1e-6), name
    tol = d.N * np.finfo(float).eps
    d.set_cg_variant("resident")
    x, it = d.cg_kkt(x0, rhs, tol, 10000)
    print("%s floor: %d iterations, vs dense %.3g" % (name, it, relerr(x, xs)))
    assert relerr(x, xs) < 1e-11, (name, relerr(x, xs))
    tol_w, k_w = _decisive_tolerance(M, mul, xk, rhs)
    xw, itw, xwm, itwm = both(xk, tol_w, 10000)
    print("%s warm, tol %.3g: %d / %d iterations (oracle %d), error %.3g" % (name, tol_w, itw, itwm, k_w, np.linalg.norm(xw - xs)))
    assert itw == itwm == k_w, (name, itw, itwm, k_w)
    assert np.linalg.norm(xw - xs) <= 2 * tol_w, (name, np.linalg.norm(xw - xs), tol_w)
    d.set_cg_variant("resident")
    x2, it2 = d.cg_kkt(xk, rhs, tol_w, 10000)
    assert it2 == itw and np.array_equal(xw, x2), name
    d.close()
