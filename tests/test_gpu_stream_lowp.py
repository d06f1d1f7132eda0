"""
GPU tests of the streamed resident CG solve's FP32 WALK (csrc/resident.hip: rs_walk<float>, rs_lowp_decide; foship.h fos_resident_lowp_stats): sweeps on
small residuals read a float copy of the tile values, by a rule that bounds what that does to the true residual by eta * tol (eta = 0.1).

The plans are those of test_gpu_resident.py's streamed cases (FOS_RESIDENT_STREAM=2 with the given FOS_RESIDENT_GMAX): every kernel instance, units
split over workgroups, ragged tiles, 64-step tiles.  The switches are read at fos_create, so every arm is a handle of its own:
  FOS_RS_LOWP=0   doubles only (the kernel path before the walk existed)      FOS_RS_LOWP=2   every sweep behind the start reads floats, no guard
  default         the rule                                                    FOS_RS_LOWP_ETA  another eta
What needs no tolerance has none: on an A whose entries ARE floats the fp32 walk computes what the fp64 walk computes, bit for bit.  The bounds of the
rule are the rule's own: the true residual of the default run is within eta * tol of the fp64 run's, the iteration counts differ by at most one.
The operator M = [I Q'; Q -I] against which residuals and the direct solution are formed is assembled entry by entry from A, b, c in float64 (sparse
storage of the same entries: the 64-column cases are 9000 x 9000).
"""
import math
import os
import zlib
from contextlib import contextmanager

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

pytestmark = pytest.mark.gpu

ETA, EPS = 0.1, np.finfo(float).eps

# (name, block shapes, FOS_RESIDENT_GMAX, what the plan must look like)
CASES = [
    ("stream-many-tiles", [(64 * 30 + 10, 32)] * 2, "1", dict(workgroups=1, max_tiles_per_workgroup=62, tiles_per_wave=9)),
    ("stream-two-units-per-workgroup", [(300, 20)] * 6, "3", dict(workgroups=3, max_tiles_per_workgroup=10)),
    ("stream-ragged-units", [(136, 12)] * 5, "2", dict(workgroups=2, max_tiles_per_workgroup=9)),
    ("stream-units-split-two-ways", [(64 * 17, 30)] * 2, "4", dict(workgroups=4, max_tiles_per_workgroup=9)),
    ("stream-wide-tiles", [(64 * 9 + 30, 50), (64 * 4, 40), (200, 64)], "3", dict(workgroups=3, steps_per_tile=64)),
    ("stream-five-tiles-per-wave", [(64 * 17, 30)] * 4, "2", dict(workgroups=2, max_tiles_per_workgroup=34, tiles_per_wave=5)),
]


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


def kkt_matrix(A, b, c):
    """M = [I Q'; Q -I], Q = [0 A' c; -A 0 b; -c' -b' 0]   (HSDEAffine.jl:2-20, affinepluslinear.jl:37-49)"""
    m, n = A.shape
    col = lambda v: sp.csr_matrix(np.asarray(v).reshape(-1, 1))
    Q = sp.bmat([[None, A.T, col(c)], [-A, None, col(b)], [-col(c).T, -col(b).T, sp.csr_matrix((1, 1))]], format="csr")
    l = n + m + 1
    return sp.bmat([[sp.identity(l), Q.T], [Q, -sp.identity(l)]], format="csc")


class Case:
    """one plan: the problem data once, the direct solution once, one handle per (A, switches), closed at the end"""

    def __init__(self, pkg, name, shapes, gmax, want):
        self.pkg, self.name, self.gmax, self.want = pkg, name, gmax, want
        rng = np.random.default_rng(zlib.crc32(name.encode()) % 1000 + 11)
        self.A = sp.block_diag([sp.csc_matrix(rng.standard_normal((r, c))) for r, c in shapes], format="csc")        # standard-normal entries
        self.A32 = self.A.copy()
        self.A32.data = self.A32.data.astype(np.float32).astype(np.float64)                                         # the same, every entry a float
        m, n = self.A.shape
        self.b, self.c = rng.standard_normal(m), rng.standard_normal(n)
        self.N = 2 * (m + n + 1)
        self.rhs, self.x0 = rng.standard_normal(self.N), rng.standard_normal(self.N)
        self.tol = self.N * EPS
        self.handles, self.memo = {}, {}

    def handle(self, rounded, lowp=None, eta=None):
        key = (rounded, lowp, eta)
        if key not in self.handles:
            A = self.A32 if rounded else self.A
            with environment(FOS_RESIDENT_STREAM="2", FOS_RESIDENT_GMAX=self.gmax, FOS_RS_LOWP=lowp, FOS_RS_LOWP_ETA=eta):
                d = self.pkg.HipHSDE(A, self.b, self.c, [("Free", A.shape[0])], [("Free", A.shape[1])])
            st = d.resident_stats()
            assert st["qualifies"] == 1 and st["form"] == "streamed", (self.name, st)
            for k, v in self.want.items():
                assert st[k] == v, (self.name, k, st)
            d.set_cg_variant("resident")
            assert d.N == self.N
            self.handles[key] = d
        return self.handles[key]

    def solve(self, rounded, lowp, tol, maxit=10000, eta=None):
        """-> (x, iterations, resident_stats() behind the solve), once per arm"""
        key = (rounded, lowp, eta, tol, maxit)
        if key not in self.memo:
            d = self.handle(rounded, lowp, eta)
            x, it = d.cg_kkt(self.x0, self.rhs, tol, maxit)
            self.memo[key] = (x, it, d.resident_stats())
        return self.memo[key]

    def reference(self):
        if "M" not in self.memo:
            M = kkt_matrix(self.A, self.b, self.c)
            self.memo["M"] = (M, spla.splu(M).solve(self.rhs))
        return self.memo["M"]

    def close(self):
        for d in self.handles.values():
            d.close()


@pytest.fixture(scope="module", params=CASES, ids=[c[0] for c in CASES])
def case(request, pkg):
    cs = Case(pkg, *request.param)
    yield cs
    cs.close()


def relerr(a, b):
    return float(np.linalg.norm(a - b) / max(1e-300, np.linalg.norm(b)))


def test_the_fp32_walk_is_the_fp64_walk_on_float_entries(case):
    """FOS_RS_LOWP=2 against FOS_RS_LOWP=0 on an A of floats: the same bits and the same count, at a loose tolerance and at the floor"""
    assert case.handle(True, 2).operator_stats()["lowp_val32_bytes"] == 4 * case.handle(True, 2).operator_stats()["vals"]
    assert case.handle(True, 0).operator_stats()["lowp_val32_bytes"] == 0
    for tol in (1e-3, case.tol):
        x0, it0, st0 = case.solve(True, 0, tol)
        x2, it2, st2 = case.solve(True, 2, tol)
        print("%s tol %.3g: %d iterations, %d fp32 sweeps" % (case.name, tol, it2, st2["lowp_sweeps_last_solve"]))
        assert st0["lowp_sweeps_last_solve"] == 0 and st2["lowp_sweeps_last_solve"] == it2 > 0
        assert it2 == it0 and np.array_equal(x2, x0), (case.name, tol, it0, it2, relerr(x2, x0))


def test_float_entries_need_no_force(case):
    """the same A at the default switch: delta == 0, every sweep behind the start qualifies, the same bits"""
    for tol in (1e-3, case.tol):
        x0, it0, _ = case.solve(True, 0, tol)
        xd, itd, st = case.solve(True, None, tol)
        assert st["lowp_delta"] == 0.0 and st["lowp_reverted_last_solve"] == 0 and st["lowp_bound_last_solve"] == 0.0, (case.name, st)
        assert st["lowp_sweeps_last_solve"] == itd == it0, (case.name, st, itd, it0)
        assert np.array_equal(xd, x0), (case.name, tol)


def check_rule(case, eta, x0, it0, xd, itd, st):
    """the bounds of the rule for a default-switch run (xd) against the fp64 run (x0) at the floor tolerance.  `eta` is the one in force: the run's own
    bound B is held to eta * tol.  The true residuals are compared within ETA * tol, the default's share, whatever eta is in force: they are formed in
    float64, where rounding alone is eps |M| |x| ~ 1e-12 on these systems -- the fp64 run's true residual sits at 3 to 20 tol for that reason -- and
    the 1e-15 of a hundredth of eta is far below what two summation orders of the same arithmetic differ by.  (The library prices the rule on
    min(tol, l eps) = tol / 2 here, N = 2 l: the bounds asserted are the looser ones of the rule as stated.)"""
    M, xs = case.reference()
    r0, rd = float(np.linalg.norm(case.rhs - M @ x0)), float(np.linalg.norm(case.rhs - M @ xd))
    print("%s eta %.3g: iterations %d (fp64 %d), fp32 sweeps %d, reverted %d, delta %.3g, B %.3g (eta tol %.3g), |rhs - M x| %.4g (fp64 %.4g), relerr %.3g (fp64 %.3g)"
          % (case.name, eta, itd, it0, st["lowp_sweeps_last_solve"], st["lowp_reverted_last_solve"], st["lowp_delta"], st["lowp_bound_last_solve"],
             eta * case.tol, rd, r0, relerr(xd, xs), relerr(x0, xs)))
    assert abs(itd - it0) <= 1, (case.name, itd, it0)
    assert st["lowp_sweeps_last_solve"] > 0, (case.name, st)
    assert st["lowp_bound_last_solve"] <= eta * case.tol, (case.name, st, eta * case.tol)
    assert rd <= r0 + ETA * case.tol, (case.name, rd, r0, ETA * case.tol)
    assert relerr(xd, xs) < 1e-11, (case.name, relerr(xd, xs))


def test_the_rule_on_a_general_matrix(case):
    x0, it0, _ = case.solve(False, 0, case.tol)
    xd, itd, st = case.solve(False, None, case.tol)
    assert st["lowp_delta"] > 0.0
    # delta against the norm it bounds, on the host: |A - fl32(A)|_2 <= delta, and delta is no looser than the Frobenius norm
    dA = (case.A - case.A32).toarray()
    assert np.linalg.norm(dA, 2) <= st["lowp_delta"] <= np.linalg.norm(dA, "fro") * (1 + 1e-6), (case.name, st["lowp_delta"])
    check_rule(case, ETA, x0, it0, xd, itd, st)
    # the same solve twice: the same bits, the same record
    d = case.handle(False, None)
    x2, it2 = d.cg_kkt(case.x0, case.rhs, case.tol, 10000)
    assert it2 == itd and np.array_equal(x2, xd) and d.resident_stats() == st


@pytest.mark.parametrize("cap", [1, 2, 5])
def test_no_switch_where_none_is_due(case, cap):
    """tol = 1e-300: the threshold eta tol / (K delta) is never met -- the doubles' bits"""
    x0, it0, _ = case.solve(False, 0, 1e-300, cap)
    xd, itd, st = case.solve(False, None, 1e-300, cap)
    assert st["lowp_sweeps_last_solve"] == 0 and st["lowp_reverted_last_solve"] == 0, (case.name, st)
    assert itd == it0 == cap and np.array_equal(xd, x0), (case.name, cap)


def test_the_guard_sends_the_solve_back_to_fp64(case):
    """an eta small enough that the bound B crosses eta tol / 2 behind the switch, chosen from the default run's recorded B.  eta moves the switch as well
    as the budget (theta = eta tol / (K delta)), so B shrinks with it and which eta trips the guard depends on where the switch falls among CG's uneven
    steps on the indefinite system: the test walks down from eta = B / tol (the default run's B as the budget) by halves, at most twelve, to the first
    eta whose solve goes back to the doubles, and holds every solve on the way to the rule's bounds."""
    _, _, st3 = case.solve(False, None, case.tol)
    x0, it0, _ = case.solve(False, 0, case.tol)
    for k in range(12):
        eta = "%.6g" % (st3["lowp_bound_last_solve"] / case.tol / 2 ** k)
        print("%s: FOS_RS_LOWP_ETA=%s (the default run's B = %.3g, tol = %.3g)" % (case.name, eta, st3["lowp_bound_last_solve"], case.tol))
        xd, itd, st = case.solve(False, None, case.tol, eta=eta)
        if st["lowp_sweeps_last_solve"] == 0:
            break                                   # (the threshold has fallen below the stop tolerance: no switch any more)
        check_rule(case, float(eta), x0, it0, xd, itd, st)
        if st["lowp_reverted_last_solve"] == 1:
            break
    assert st["lowp_reverted_last_solve"] == 1, (case.name, st)


def floor_call(prob):
    """the projection's call count (AffinePlusLinear.i) from which its CG tolerance max(0.2^sqrt(i), l eps) is the floor l eps (affinepluslinear.jl:108-112)"""
    floor = (prob.m + prob.n + 1) * EPS
    i0 = int(math.ceil((math.log(floor) / math.log(0.2)) ** 2)) + 1
    assert 0.2 ** math.sqrt(i0) <= floor
    return i0


def dr_handle(pkg, prob, lowp):
    with environment(FOS_RESIDENT_STREAM="2", FOS_RS_LOWP=lowp):
        d = pkg.HipHSDE(prob.A, prob.b, prob.c, prob.K1, prob.K2)
    assert d.resident_stats()["form"] == "streamed"
    d.set_cg_variant("resident")
    d.set_alg(pkg.DR())
    d.set_iterate(None)
    return d


def dr_steps(d, count, first=1):
    """-> the CG iterations of each of `count` DR steps and the fp32 sweeps of all of them"""
    totals, sweeps, base = [], 0, d.cg_total()
    for k in range(count):
        done, _, _ = d.step(first + k, 1, 10 ** 6, 1e-8)
        assert done == 1
        totals.append(d.cg_total() - base)
        sweeps += d.resident_stats()["lowp_sweeps_last_solve"]
    return np.diff([0] + totals), sweeps


def test_loose_first_solves_keep_the_doubles(pkg):
    """c4_block_sdp(nblocks=8), streamed, DR, the first 40 steps of a fresh handle, default against FOS_RS_LOWP=0.  Their CG tolerances are 0.2 .. 4e-5 and
    the rule is priced on min(tol, l eps): no residual of these solves gets small enough for the float copy.  No fp32 sweep, the same counts, the same bits."""
    prob = pkg.workloads.c4_block_sdp(nblocks=8)
    runs = []
    for lowp in ("0", None):
        d = dr_handle(pkg, prob, lowp)
        cg, sweeps = dr_steps(d, 40)
        runs.append((d.get_iterate(), cg, sweeps))
        d.close()
    (z0, cg0, s0), (zd, cgd, sd) = runs
    assert s0 == 0 and sd == 0
    assert np.array_equal(cgd, cg0) and np.array_equal(zd, z0)


def test_outer_iterations_take_the_same_steps(pkg):
    """c4_block_sdp(nblocks=8), streamed, DR, 40 steps from the same start, default against FOS_RS_LOWP=0: the iterates agree to 1e-9 relative, the
    project's same-step tolerance, and the CG iterations of every step to one.
    The start is the state an fp64 handle is in after 40 steps at the floor tolerance l eps (iterate, CGdata.xinit and AffinePlusLinear.i, handed to both
    arms): the fp32 sweeps exist only at the floor, and a solver is at the floor only with a warm iterate (outer iteration 267 on for this problem; the
    call count is set there so that the test need not run 267 steps first).  From a COLD iterate at the floor tolerance the count of a step is not a
    property of a build: two fp64 runs that differ in summation order alone (the resident solve against the launch-per-iteration kernels of the same
    recurrence) differ by two or more iterations in 7 of the first 40 such steps, as does the default against FOS_RS_LOWP=0 at every eta from 0.1 down
    to 3e-4 (4 to 6 of 40, none in steps 41 to 80) -- CG's residual on [I Q'; Q -I] falls in pairs of iterations, and those first solves end within
    rounding of the stop test."""
    prob = pkg.workloads.c4_block_sdp(nblocks=8)
    i0 = floor_call(prob)
    w = dr_handle(pkg, prob, "0")
    w.set_affine_state(np.zeros(w.N), i0)
    dr_steps(w, 40)
    z, (xinit, i, _) = w.get_iterate(), w.get_affine_state()
    w.close()
    assert i == i0 + 40
    runs = []
    for lowp in ("0", None):
        d = dr_handle(pkg, prob, lowp)
        d.set_iterate(z)
        d.set_affine_state(xinit, i)
        cg, sweeps = dr_steps(d, 40, 41)
        runs.append((d.get_iterate(), cg, sweeps))
        d.close()
    (z0, cg0, s0), (zd, cgd, sd) = runs
    print("40 DR steps at the floor: CG iterations %d (fp64 %d), fp32 sweeps %d, largest difference of a step's count %d, relative difference of the iterates %.3g"
          % (cgd.sum(), cg0.sum(), sd, np.max(np.abs(cgd - cg0)), relerr(zd, z0)))
    assert s0 == 0 and sd > 0
    assert np.max(np.abs(cgd - cg0)) <= 1, (cg0, cgd)
    assert relerr(zd, z0) <= 1e-9
