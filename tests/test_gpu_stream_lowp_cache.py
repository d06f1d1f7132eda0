"""
GPU tests of WHERE the streamed resident CG solve's fp32 walk reads its float copy from (csrc/resident.hip: rs_request<float, CACHED>; fos_internal.hpp:
rs_lowp_cached; foship.h fos_resident_lowp_cache_stats).  A copy within the budget is read with loads that take the default cache policy, a larger one --
and every copy under FOS_RS_LOWP_CACHE=0 -- with non-temporal loads.  The policy changes where bytes come from and not one operation, so nothing here has
a tolerance: the two arms give the same bits, the same iteration counts and the same count of fp32 sweeps.

The plans are the six streamed plans of test_gpu_stream_lowp.py (FOS_RESIDENT_STREAM=2 with the given FOS_RESIDENT_GMAX) -- many tiles, two units per
workgroup, ragged units, units split over workgroups, 64-step tiles, five tiles per wavefront -- which launch cg_stream_kernel<32, 9>, <32, 3> (three of them),
<64, 3> and <32, 5>, and two more for the instances those six do not reach: <64, 5> (28 tiles of 50 steps in one workgroup) and <32, 10> (68 tiles in one
workgroup).  Which instance a plan launches follows from steps_per_tile and tiles_per_wave (res_kernel, csrc/resident.hip), and every case asserts both, so
all six cached instances and their six non-temporal twins run here.  The switches are read at fos_create, so every arm is a handle of its own.
"""
import os
import zlib
from contextlib import contextmanager

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps

# (name, block shapes, FOS_RESIDENT_GMAX, what the plan must look like: steps_per_tile and tiles_per_wave name the kernel instance <TMAX, NT>)
CASES = [
    ("many-tiles", [(64 * 30 + 10, 32)] * 2, "1", dict(workgroups=1, max_tiles_per_workgroup=62, steps_per_tile=32, tiles_per_wave=9)),
    ("two-units-per-workgroup", [(300, 20)] * 6, "3", dict(workgroups=3, max_tiles_per_workgroup=10, steps_per_tile=32, tiles_per_wave=3)),
    ("ragged-units", [(136, 12)] * 5, "2", dict(workgroups=2, max_tiles_per_workgroup=9, steps_per_tile=32, tiles_per_wave=3)),
    ("units-split-two-ways", [(64 * 17, 30)] * 2, "4", dict(workgroups=4, max_tiles_per_workgroup=9, steps_per_tile=32, tiles_per_wave=3)),
    ("wide-tiles", [(64 * 9 + 30, 50), (64 * 4, 40), (200, 64)], "3", dict(workgroups=3, steps_per_tile=64, tiles_per_wave=3)),
    ("five-tiles-per-wave", [(64 * 17, 30)] * 4, "2", dict(workgroups=2, max_tiles_per_workgroup=34, steps_per_tile=32, tiles_per_wave=5)),
    # beyond the six: the two instances they do not reach
    ("wide-tiles-five-per-wave", [(64 * 27 + 5, 50)], "1", dict(workgroups=1, max_tiles_per_workgroup=28, steps_per_tile=64, tiles_per_wave=5)),
    ("ten-tiles-per-wave", [(64 * 68 - 7, 32)], "1", dict(workgroups=1, max_tiles_per_workgroup=68, steps_per_tile=32, tiles_per_wave=10)),
]
# the arms: what the environment holds at fos_create
DEFAULT, CACHE_OFF, BUDGET_ZERO = (None, None), ("0", None), (None, "0")


@contextmanager
def environment(**kv):
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


class Case:
    """one plan: the problem data once, one handle per (FOS_RS_LOWP, arm), one solve per handle, closed at the end"""

    def __init__(self, pkg, name, shapes, gmax, want):
        self.pkg, self.name, self.gmax, self.want = pkg, name, gmax, want
        rng = np.random.default_rng(zlib.crc32(name.encode()) % 1000 + 11)
        self.A = sp.block_diag([sp.csc_matrix(rng.standard_normal((r, c))) for r, c in shapes], format="csc")
        m, n = self.A.shape
        self.b, self.c = rng.standard_normal(m), rng.standard_normal(n)
        self.N = 2 * (m + n + 1)
        self.rhs, self.x0 = rng.standard_normal(self.N), rng.standard_normal(self.N)
        self.tol = self.N * EPS
        self.handles, self.memo = {}, {}

    def handle(self, lowp, arm):
        key = (lowp, arm)
        if key not in self.handles:
            with environment(FOS_RESIDENT_STREAM="2", FOS_RESIDENT_GMAX=self.gmax, FOS_RS_LOWP=lowp, FOS_RS_LOWP_CACHE=arm[0], FOS_RS_LOWP_CACHE_MB=arm[1]):
                d = self.pkg.HipHSDE(self.A, self.b, self.c, [("Free", self.A.shape[0])], [("Free", self.A.shape[1])])
            st = d.resident_stats()
            assert st["qualifies"] == 1 and st["form"] == "streamed", (self.name, st)
            for k, v in self.want.items():
                assert st[k] == v, (self.name, k, st)
            d.set_cg_variant("resident")
            assert d.N == self.N
            self.handles[key] = d
        return self.handles[key]

    def solve(self, lowp, arm):
        """-> (x, iterations, resident_stats() behind the solve), once per handle"""
        key = (lowp, arm)
        if key not in self.memo:
            d = self.handle(lowp, arm)
            x, it = d.cg_kkt(self.x0, self.rhs, self.tol, 10000)
            self.memo[key] = (x, it, d.resident_stats())
        return self.memo[key]

    def close(self):
        for d in self.handles.values():
            d.close()


@pytest.fixture(scope="module", params=CASES, ids=[c[0] for c in CASES])
def case(request, pkg):
    cs = Case(pkg, *request.param)
    yield cs
    cs.close()


@pytest.mark.parametrize("lowp", ("2", None), ids=("every-sweep-fp32", "by-the-rule"))
def test_cached_and_streamed_copy_give_the_same_bits(case, lowp):
    x1, it1, st1 = case.solve(lowp, DEFAULT)
    x0, it0, st0 = case.solve(lowp, CACHE_OFF)
    print("%s FOS_RS_LOWP=%s: %d / %d iterations, %d / %d fp32 sweeps, lowp_cached %d / %d" %
          (case.name, lowp, it1, it0, st1["lowp_sweeps_last_solve"], st0["lowp_sweeps_last_solve"], st1["lowp_cached"], st0["lowp_cached"]))
    assert st1["lowp_cached"] == 1 and st0["lowp_cached"] == 0, (case.name, st1, st0)
    assert np.all(np.isfinite(x1))
    assert np.array_equal(x1, x0), (case.name, float(np.max(np.abs(x1 - x0))))
    assert it1 == it0, (case.name, it1, it0)
    assert st1["lowp_sweeps_last_solve"] == st0["lowp_sweeps_last_solve"], (case.name, st1, st0)
    if lowp == "2":
        assert st1["lowp_sweeps_last_solve"] == it1 > 0, (case.name, st1, it1)      # every sweep behind the start went through the loads under test


def test_what_the_handle_reports(case):
    d1, d0, dz = case.handle(None, DEFAULT), case.handle(None, CACHE_OFF), case.handle(None, BUDGET_ZERO)
    s1, s0, sz = d1.resident_stats(), d0.resident_stats(), dz.resident_stats()
    nbytes = d1.operator_stats()["lowp_val32_bytes"]
    assert nbytes == 4 * d1.operator_stats()["vals"] > 0
    built_in = case.pkg.host_lowp_cached(nbytes)[1]
    assert (s1["lowp_cached"], s1["lowp_cache_budget_bytes"]) == (1, built_in)
    assert (s0["lowp_cached"], s0["lowp_cache_budget_bytes"]) == (0, built_in)
    assert (sz["lowp_cached"], sz["lowp_cache_budget_bytes"]) == (0, 0)
    # the handle decides by the host rule
    assert case.pkg.host_lowp_cached(nbytes) == (True, built_in)
    assert case.pkg.host_lowp_cached(nbytes, cache=False)[0] is False
    assert case.pkg.host_lowp_cached(nbytes, budget_mb=0) == (False, 0)


def test_no_float_copy_nothing_cached(case):
    d = case.handle("0", DEFAULT)
    assert d.operator_stats()["lowp_val32_bytes"] == 0
    assert d.resident_stats()["lowp_cached"] == 0


def test_the_same_solve_twice_on_one_handle(case):
    d = case.handle("2", DEFAULT)
    xa, ita = d.cg_kkt(case.x0, case.rhs, case.tol, 10000)
    xb, itb = d.cg_kkt(case.x0, case.rhs, case.tol, 10000)
    assert d.resident_stats()["lowp_cached"] == 1
    assert ita == itb and np.array_equal(xa, xb), (case.name, ita, itb)
    x1, it1, _ = case.solve("2", DEFAULT)
    assert ita == it1 and np.array_equal(xa, x1), case.name
