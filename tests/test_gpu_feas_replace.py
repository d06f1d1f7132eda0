"""GPU: the sets of the Feasibility form behind one interface (ProxObject, csrc/fos_internal.hpp) and one install path (feas_install, csrc/feas.hip): a slot
defined again with ANY other kind computes what a fresh handle computes, frees what it held, leaves the other slot alone, answers exactly the accessor of the
kind it holds, keeps its set when a definition is refused, and starts a new solve from a clean state.

All objects at n = 96 (not a multiple of 64: L = 128, the padding is in play), the affine kinds at m = 24, built by the case builders of the kinds' own tests.
Comparisons against a fresh handle: np.array_equal where the kind's own test asserts the same bits run to run (test_gpu_sparse_affine.py:52,
test_gpu_affine_factored.py:42, test_gpu_affine_sparse_factored.py:49,104, test_gpu_nspace.py:133, test_gpu_feas_sets.py:62, the element-wise box and the
callback's own arithmetic of test_gpu_feasibility.py:36,348); the dense projector at 1e-11 max(1, |x|_inf) (test_gpu_feasibility.py:33) and the ConeProduct at
5e-12 max(1, |x|_inf) (test_gpu_feasibility.py:230), the bars of their own tests.

Refusals: the duplicated inconsistent row is refused at set-up by the dense projector and the two factored forms; the sparse CG entry accepts it (it finds
the rank at its first projection, test_gpu_sparse_affine.py), so that entry is refused with the argument it does refuse at set-up, a zero row."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

import nspace_cases as nc
from affine_factored_cases import instance
from set_cases import RefBallL2, make_set
from sparse_factored_cases import csc_args, rand

pytestmark = pytest.mark.gpu

N, M = 96, 24
FOS_EINVAL = -1
CONES = [("NonNeg", 30), ("SOC", 20), ("SDP", 6), ("Free", 40)]               # one PSD cone of order 3, one second-order cone
ACCESSORS = ("affine_stats", "affine_factored_stats", "affine_sparse_factored_stats", "nspace_stats", "set_stats")
EXACT, PROJECTOR, CONE = 0.0, 1e-11, 5e-12                                    # the bar against a fresh handle, times max(1, |x|_inf); 0: the same bits


class Objects:
    """name -> (set, the one accessor that describes it or None, bar); the order of the chain; the fixed input; slot 2's box and every fresh handle's prox"""

    def __init__(self, pkg):
        rng = np.random.default_rng(96)
        A, b = instance("gauss", M, N)
        As, bs = rand(M, N, 5)
        At, bt = nc.instance("gauss", 130, N)                                 # a tall A for the normal-equations form
        Ats, bts = nc.tall_sparse(200, N, 3)
        Q, q = nc.quadratic_of(At, bt, 0.3)
        self.A, self.b, self.As, self.bs, self.At, self.bt, self.Ats, self.bts, self.Q, self.q = A, b, As, bs, At, bt, Ats, bts, Q, q
        lo = -0.5 - rng.random(N)
        blocks = [(pkg.IndBallL2(*make_set("IndBallL2", 40, rng)[1]), 40), (pkg.IndSimplex(*make_set("IndSimplex", 30, rng)[1]), 30),
                  (pkg.IndHalfspace(*make_set("IndHalfspace", 26, rng)[1]), 26)]
        self.sets = {
            "box": (pkg.IndBox(-0.5, 0.25), None, EXACT),
            "box_arrays": (pkg.IndBox(lo, lo + 1.0 + rng.random(N)), None, EXACT),
            "affine_projector": (pkg.IndAffine(A, b), None, PROJECTOR),
            "affine_factored": (pkg.IndAffine(A, b, form="factored"), "affine_factored_stats", EXACT),
            "affine_sparse_cg": (pkg.IndAffine(As, bs), "affine_stats", EXACT),
            "affine_sparse_factored": (pkg.IndAffine(As, bs, form="sparse_factored"), "affine_sparse_factored_stats", EXACT),
            "ls_factored": (pkg.LeastSquares(A, b, 0.7), "affine_factored_stats", EXACT),
            "ls_normal": (pkg.LeastSquares(At, bt, 0.7, form="normal"), "nspace_stats", EXACT),
            "ls_sparse_factored": (pkg.LeastSquares(As, bs, 0.7, form="sparse_factored"), "affine_sparse_factored_stats", EXACT),
            "ls_sparse_normal": (pkg.LeastSquares(Ats, bts, 0.7, form="normal"), "nspace_stats", EXACT),
            "quadratic": (pkg.Quadratic(Q, q), "nspace_stats", EXACT),
            "separable_sum": (pkg.SeparableSum(blocks), "set_stats", EXACT),
            "cones": (pkg.ConeProduct(CONES), None, CONE),
            "callback": (RefBallL2(1.5, np.ones(N)), None, EXACT),
        }
        self.order = list(self.sets)
        self.x = 2.0 * rng.standard_normal(N)
        self.box2 = pkg.IndBox(lo - 0.25, lo + 0.75)                          # slot 2 throughout: array bounds
        self.y2 = np.minimum(np.maximum(self.x, lo - 0.25), lo + 0.75)
        self.fresh = {}
        for name, (S, _, _) in self.sets.items():                             # a fresh handle holding only that set (and slot 2's box)
            d = pkg.HipFeasibility(pkg.Feasibility(S, self.box2, N))
            self.fresh[name] = d.prox(1, self.x)
            d.close()

    def handle(self, pkg):
        return pkg.HipFeasibility(pkg.Feasibility(pkg.IndBox(-1.0, 1.0), self.box2, N))

    def define(self, pkg, d, name, which=1):
        S = self.sets[name][0]
        if isinstance(S, pkg.SeparableSum):
            d.set_blocks(which, *S.pack(N))
        else:
            d.set_set(which, S)

    def chain(self):
        return self.order + self.order[::-1]                                  # every object in turn, then a second time round in reverse order

    def same(self, name, y):
        bar = self.sets[name][2]
        err = float(np.abs(y - self.fresh[name]).max())
        print("%s: |chain - fresh handle| = %.2e (bar %.2e)" % (name, err, bar * max(1.0, np.abs(self.x).max())))
        if bar == EXACT:
            assert np.array_equal(y, self.fresh[name]), (name, err)
        else:
            assert err <= bar * max(1.0, np.abs(self.x).max()), (name, err)


@pytest.fixture(scope="module")
def objs(pkg):
    return Objects(pkg)


def test_replacement_chain_computes_what_a_fresh_handle_computes(pkg, objs):
    d = objs.handle(pkg)
    for name in objs.chain():
        objs.define(pkg, d, name)
        objs.same(name, d.prox(1, objs.x))
        assert np.array_equal(d.prox(2, objs.x), objs.y2), name               # slot 2 does not change


def test_accessors_follow_the_kind(pkg, objs):
    d = objs.handle(pkg)
    for name in objs.chain():
        objs.define(pkg, d, name)
        own = objs.sets[name][1]
        for acc in ACCESSORS:
            if acc == own:
                getattr(d, acc)(1)
            else:
                with pytest.raises(pkg.lib.FosError):
                    getattr(d, acc)(1)


def test_newton_schulz_record_follows_the_projector(pkg, objs):
    d = objs.handle(pkg)
    assert d.info()["ns_iters"] == [0, 0]
    for name in objs.chain():
        objs.define(pkg, d, name)
        it, res = d.info()["ns_iters"][0], d.info()["ns_resid"][0]
        if name == "affine_projector":
            assert it > 0 and res <= 1e-10, (it, res)
        else:
            assert it == 0 and res == 0.0, (name, it, res)                    # "0 when the set is not affine": also after the projector was replaced


def test_refusal_keeps_the_set(pkg, objs):
    """every entry that can refuse its arguments: the refused call returns its error and the slot -- holding a set of the SAME entry, so that a build that
    freed or overwrote first would show -- computes the same bits as before the call"""
    lib, dptr = pkg.lib.load(), pkg.lib.dptr
    A, b, As, bs, x = objs.A, objs.b, objs.As, objs.bs, objs.x
    D = A.copy(); D[7] = D[2]                                                 # a duplicated row with an inconsistent right-hand side
    b2 = b.copy(); b2[7] = b[2] + 1.0
    Ds = sp.lil_matrix(As); Ds[7, :] = Ds[2, :]
    bs2 = bs.copy(); bs2[7] = bs[2] + 1.0
    Zs = sp.lil_matrix(As); Zs[4, :] = 0.0                                    # a zero row: what the sparse CG entry refuses at set-up
    bad_q = objs.Q.copy(); bad_q[5, 5] = -2.0                                 # a diagonal that is not positive semidefinite
    keep, (cp, rv, nz) = csc_args(pkg, As)
    keept, (cpt, rvt, nzt) = csc_args(pkg, objs.Ats)
    i32p, i64p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)
    free2 = np.full(2, pkg.lib.SET_CODES["IndFree"], dtype=np.int32)
    short, long_ = np.array([20, 20], dtype=np.int64), np.array([20, 90], dtype=np.int64)
    scal = np.zeros(4)
    d = objs.handle(pkg)

    def by_set(S):
        def call():
            with pytest.raises(pkg.lib.FosError):
                d.set_set(1, S)
        return call

    def by_code(fn):
        def call():
            assert fn() == FOS_EINVAL, lib.fos_last_error()
        return call
    refusals = [
        ("affine_projector", by_set(pkg.IndAffine(D, b2))),
        ("affine_factored", by_set(pkg.IndAffine(D, b2, form="factored"))),
        ("affine_sparse_factored", by_set(pkg.IndAffine(sp.csc_matrix(Ds), bs2, form="sparse_factored"))),
        ("affine_sparse_cg", by_set(pkg.IndAffine(sp.csc_matrix(Zs), bs))),
        ("ls_factored", by_code(lambda: lib.fos_feas_set_least_squares(d._h, 1, M, dptr(A), dptr(b), 0.0, 1))),
        ("ls_normal", by_code(lambda: lib.fos_feas_set_least_squares_normal(d._h, 1, objs.At.shape[0], dptr(objs.At), dptr(objs.bt), 0.0, 1))),
        ("ls_sparse_factored", by_code(lambda: lib.fos_feas_set_least_squares_sparse(d._h, 1, M, cp, rv, nz, dptr(bs), 0.0, pkg.lib.LS_FORM_CODES["sparse_factored"], 1))),
        ("ls_sparse_normal", by_code(lambda: lib.fos_feas_set_least_squares_sparse(d._h, 1, objs.Ats.shape[0], cpt, rvt, nzt, dptr(objs.bts), 0.0, pkg.lib.LS_FORM_CODES["normal"], 1))),
        ("quadratic", by_set(pkg.Quadratic(bad_q, objs.q))),
        ("cones", by_set(pkg.ConeProduct([("NonNeg", 30), ("SOC", 20)]))),                          # lengths summing to 50
        ("cones", by_set(pkg.ConeProduct(CONES + [("SDP", 6)]))),                                    # ... and to 102
        ("separable_sum", by_code(lambda: lib.fos_feas_set_blocks(d._h, 1, 2, free2.ctypes.data_as(i32p), short.ctypes.data_as(i64p), dptr(scal), None))),
        ("separable_sum", by_code(lambda: lib.fos_feas_set_blocks(d._h, 1, 2, free2.ctypes.data_as(i32p), long_.ctypes.data_as(i64p), dptr(scal), None))),
    ]
    for name, refused in refusals:
        objs.define(pkg, d, name)
        before = d.prox(1, x)
        refused()
        assert np.array_equal(d.prox(1, x), before), name
        objs.same(name, before)
    assert keep is not None and keept is not None


def test_a_new_solve_starts_from_a_clean_state(pkg, objs):
    """set_iterate(None) resets every object through its own reset(): 20 GAP iterations with the sparse CG IndAffine (warm multipliers) and the ConeProduct
    (warm PSD bases) after an earlier run on the same handle give the bits of the same run on a fresh handle"""
    def run(d):
        d.set_alg(pkg.GAP())
        d.set_iterate(None)
        done, _, _, _ = d.step(1, 20, 10 ** 9, 1e-30)
        assert done == 20
        return d.get_iterate()
    problem = pkg.Feasibility(objs.sets["affine_sparse_cg"][0], objs.sets["cones"][0], N)
    d = pkg.HipFeasibility(problem)
    first = run(d)
    d.step(21, 7, 10 ** 9, 1e-30)                                             # leave multipliers and bases that the fresh handle does not have
    again = run(d)
    fresh = run(pkg.HipFeasibility(problem))
    print("|again - fresh| = %.2e, |first - fresh| = %.2e" % (np.abs(again - fresh).max(), np.abs(first - fresh).max()))
    assert np.array_equal(again, fresh) and np.array_equal(first, fresh)
