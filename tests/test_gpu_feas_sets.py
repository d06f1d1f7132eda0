"""
GPU: the vector sets of csrc/sets.hip as sets of the Feasibility form (Feasibility.jl:2-6) -- IndBallL2, IndBallL1, IndSimplex, IndHalfspace, IndHyperslab,
IndPoint, IndFree, scalar IndBox, alone and as a SeparableSum -- against the sort-based references of tests/set_cases.py: projections on both sides of every
class boundary, a product of ~300 blocks, oracle-free certificates, iterates and whole solves against the oracle and against the device's own callback path
running the same reference object, the printed search lines of LineSearchWrapper and GAPP, and the error paths.

Tolerance of a projection: 1e-13 max(|x|_inf, |parameter|) per element (tests/test_feas_sets_cpu.py derives it); y = x and y = p cases are compared bit for bit.
"""
import ctypes
import re

import numpy as np
import pytest

from feasibility_cases import ALGS, GAPP, affine_box_instance
from set_cases import INPUTS, KINDS, PASS_CAP, RefBallL2, RefSimplex, make_case, random_separable_sum

pytestmark = pytest.mark.gpu

LENGTHS = [1, 64, 65, 1024, 1025, 16384, 16385, 100003]       # both sides of the wavefront / workgroup / grid class boundaries; no multiple of anything
FOS_EINVAL = -1


def _pack(pkg, S, n):
    return pkg.SeparableSum([(S, n)]).pack(n)


@pytest.mark.parametrize("length", LENGTHS)
@pytest.mark.parametrize("kind", KINDS)
def test_single_block_projection(pkg, kind, length):
    d = pkg.HipFeasibility(pkg.Feasibility(pkg.IndFree(), pkg.IndFree(), length))
    worst = 0.0
    for inp in INPUTS:
        case = make_case(kind, length, inp)
        d.set_blocks(1, *_pack(pkg, case.device_set(pkg), length))              # (replaces the set of the same handle)
        y = d.prox(1, case.x)
        worst = max(worst, case.check(y, inp) / max(case.tol(), 1e-300))
        st = d.set_stats(1)
        assert st["blocks"] == 1 and (st["wave_blocks"], st["workgroup_blocks"], st["grid_blocks"]) == (length <= 1024, 1024 < length <= 16384, length > 16384)
        threshold, scalar = kind in ("IndSimplex", "IndBallL1"), kind in ("IndBallL2", "IndHalfspace", "IndHyperslab")
        assert st["launches"] == (1 if length <= 16384 else 3 + 2 * PASS_CAP if threshold else 3 if scalar else 1)
        assert st["pass_cap"] == PASS_CAP and 0 <= st["last_passes"] <= PASS_CAP and (threshold or st["last_passes"] == 0)
    print("%s, len %d: worst error / tolerance = %.3g" % (kind, length, worst))
    d.close()


def test_separable_sum_of_300_blocks(pkg):
    S, ref, n, layout = random_separable_sum(pkg)
    d = pkg.HipFeasibility(pkg.Feasibility(S, pkg.IndFree(), n))
    st = d.set_stats(1)
    assert st["blocks"] == len(layout) == 300 and st["wave_blocks"] + st["workgroup_blocks"] == 300 and st["workgroup_blocks"] > 0 and st["launches"] == 2
    assert layout[0][0] == layout[-1][0] == "IndFree" and sum(l[0] == "IndFree" for l in layout) > 10
    x = np.random.default_rng(8).standard_normal(n)
    y = d.prox(1, x)
    expect = ref.project(x)
    for kind, start, length, param in layout:
        xs, ys, es = x[start:start + length], y[start:start + length], expect[start:start + length]
        if kind == "IndFree":
            assert np.array_equal(ys, xs), (start, length)                      # no kernel writes outside its block
        else:
            assert np.abs(ys - es).max() <= 1e-13 * max(np.abs(xs).max(), abs(param)), (kind, start, length)
    assert np.array_equal(d.prox(1, x), y)                                      # a fixed summation order: the same bits
    assert 1 <= d.set_stats(1)["last_passes"] <= PASS_CAP


def _in_set(case, y):
    """how far y is outside the set, relative to the tolerance scale"""
    r = case.ref
    if case.kind == "IndBallL2":
        return max(0.0, np.linalg.norm(y - r.c) - r.r) / max(r.r, 1.0)
    if case.kind == "IndBallL1":
        return max(0.0, np.abs(y).sum() - r.r) / max(r.r, 1.0)
    if case.kind == "IndSimplex":
        return max(abs(y.sum() - r.a) / r.a, max(0.0, -y.min()))
    if case.kind in ("IndHalfspace", "IndHyperslab"):
        s = float(r.a @ y)
        return max(0.0, s - r.hi, r.lo - s) / np.linalg.norm(r.a)
    if case.kind == "IndPoint":
        return np.abs(y - r.p).max()
    if case.kind == "IndBox":
        return max(0.0, (y - r.hi).max(), (r.lo - y).max())
    return 0.0


@pytest.mark.parametrize("n", [700, 5000, 40000])
@pytest.mark.parametrize("kind", KINDS)
def test_certificates(pkg, kind, n):
    """Without any reference projection: y = P(x) is in the set to rounding, P(P(x)) = P(x), and <x - y, z - y> <= tol |x| |z| for 20 points z of the set
    (the characterisation of the projection onto a convex set).  tol = 1e-12: y carries at most 1e-13 |x|_inf per element, that is |dy|_2 <= 1e-13 sqrt(n)
    |x|_inf ~ 4.5e-13 |x|_2 for a standard normal x, and the inner product moves by at most |dy| (|x - y| + |z - y|)."""
    case = make_case(kind, n, "gauss", seed=1)
    d = pkg.HipFeasibility(pkg.Feasibility(case.device_set(pkg), pkg.IndFree(), n))
    x = case.x
    y = d.prox(1, x)
    assert _in_set(case, y) <= 1e-12, _in_set(case, y)
    assert np.abs(d.prox(1, y) - y).max() <= case.tol()
    rng = np.random.default_rng(n)
    worst = -np.inf
    for k in range(20):
        z = d.prox(1, (0.1 + k) * rng.standard_normal(n))
        assert _in_set(case, z) <= 1e-12
        viol = float((x - y) @ (z - y)) / (np.linalg.norm(x) * np.linalg.norm(z))
        worst = max(worst, viol)
        assert viol <= 1e-12, (k, viol)
    print("%s, n = %d: max <x - y, z - y> / (|x| |z|) = %.3g" % (kind, n, worst))


def _affine_and(pkg, orc, which):
    """IndAffine(A, b) (30 x 100) against a ball around a point 2 away from the affine set, radius 2.2 (the instance of
    test_host_callback_set_matches_oracle), or against the simplex through the instance's own non-negative solution: both intersections are non-empty"""
    A, b = affine_box_instance(m=30, n=100)
    n = A.shape[1]
    if which == "ball":
        x_ls = np.linalg.lstsq(A, b, rcond=None)[0]
        u = np.random.default_rng(9).standard_normal(n)
        center = x_ls + 2.0 * u / np.linalg.norm(u)
        dev, refs = pkg.IndBallL2(2.2, center), [RefBallL2(2.2, center) for _ in range(2)]
        inside = lambda g: np.linalg.norm(g - center) <= 2.2 * (1 + 1e-6)
    else:
        xs = np.maximum(np.random.default_rng(2).standard_normal(n), 0.0)       # (affine_box_instance's point: A xs = b)
        assert np.allclose(A @ xs, b, rtol=0, atol=1e-12)
        a = float(xs.sum())
        dev, refs = pkg.IndSimplex(a), [RefSimplex(a) for _ in range(2)]
        inside = lambda g: g.min() >= -1e-6 and abs(g.sum() - a) <= 1e-6
    return A, b, n, dev, refs, inside


@pytest.mark.parametrize("which", ["ball", "simplex"])
@pytest.mark.parametrize("algname", ["DR", "GAPA", "FISTA", "Dykstra"])
def test_iterates_match_oracle_and_callback_path(pkg, oracle, algname, which):
    """The device set in the algorithms: the same iterates as the oracle running the reference object (<= 1e-11 max(1, |x|_inf)) and as the device's own
    callback path running it (<= 1e-10), then the whole solve.  (GAPA's step-length estimate is ill-conditioned against a curved set -- see
    test_host_callback_set_matches_oracle: two iterations are compared, then its solve for the result.)"""
    orc = oracle
    A, b, n, dev_set, (ref_o, ref_cb), inside = _affine_and(pkg, orc, which)
    oalg = ALGS[algname](orc, verbose=0)
    ost = orc.FeasibilityStatus(orc.FeasibilityModel(orc.Feasibility(orc.IndAffine(A, b), ref_o, n), oalg), 4, 1e-30, 0, 1)
    d = pkg.HipFeasibility(pkg.Feasibility(pkg.IndAffine(A, b), dev_set, n))
    dc = pkg.HipFeasibility(pkg.Feasibility(pkg.IndAffine(A, b), ref_cb, n))
    for h in (d, dc):
        h.set_alg(ALGS[algname](pkg))
        h.set_iterate(None)
    xo = np.zeros(n)
    nsame = 2 if algname == "GAPA" else 30
    for i in range(1, nsame + 1):
        ost.i = i
        oalg.step(xo, i, ost)
        assert d.step(i, 1, 4, 1e-30)[0] == 1 and dc.step(i, 1, 4, 1e-30)[0] == 1
        z = d.get_iterate()
        assert np.abs(z - xo).max() <= 1e-11 * max(1.0, np.abs(xo).max()), (algname, i)
        assert np.abs(z - dc.get_iterate()).max() <= 1e-10, (algname, i)
    assert ref_cb.calls == ref_o.calls > 0                     # the callback path really ran the object; the device set never did
    if algname in ("DR", "GAPA"):
        done, status, err, checked = d.step(nsame + 1, 3000, 10, 1e-9)
        assert status == "Optimal", (status, err)
        g, _, _ = d.getsol()
        assert np.abs(A @ g - b).max() <= 1e-6 and inside(g)


def _search_lines(lines):
    return [l for l in lines if l.startswith(("test, ", "α", "normtest: "))]


def _same_lines(dev, orc_lines):
    """the same lines in the same order: labels equal, numbers to 1e-7 (the bar of the wrapper tests of the built-in sets)"""
    assert len(dev) == len(orc_lines) > 0
    for ld, lo in zip(dev, orc_lines):
        pd, po = re.split(r"[:,]\s*", ld), re.split(r"[:,]\s*", lo)
        assert pd[0] == po[0] and len(pd) == len(po), (ld, lo)
        assert np.allclose([float(t) for t in pd[1:]], [float(t) for t in po[1:]], rtol=1e-7, atol=1e-11), (ld, lo)


@pytest.mark.parametrize("which", ["ball", "simplex"])
def test_linesearch_and_gapp_print_the_oracles_lines(pkg, oracle, which):
    orc = oracle
    A, b, n, dev_set, (ref_o, ref_o2), _ = _affine_and(pkg, orc, which)
    hp = pkg.Feasibility(pkg.IndAffine(A, b), dev_set, n)
    out, olines = [], []
    pkg.solve_feasibility(hp, pkg.LineSearchWrapper(ALGS["GAP"](pkg, eps=1e-30), lsinterval=5), out=out, checki=5, max_iters=12)
    orc.feasibility_solve(orc.Feasibility(orc.IndAffine(A, b), ref_o, n), orc.LineSearchWrapper(ALGS["GAP"](orc, eps=1e-30, verbose=0), lsinterval=5, out=olines),
                          checki=5, max_iters=12)
    assert len(_search_lines(olines)) == 2 * 33
    _same_lines(_search_lines(out), _search_lines(olines))
    out, olines = [], []
    pkg.solve_feasibility(hp, GAPP(pkg, iproj=4, eps=1e-30), out=out, checki=4, max_iters=9)
    orc.feasibility_solve(orc.Feasibility(orc.IndAffine(A, b), ref_o2, n), GAPP(orc, iproj=4, eps=1e-30, verbose=0, out=olines), checki=4, max_iters=9)
    assert len(_search_lines(olines)) == 2 * 22
    _same_lines(_search_lines(out), _search_lines(olines))


def test_error_paths_and_replacement(pkg):
    n = 50
    lib = pkg.lib.load()
    c = pkg.lib.SET_CODES
    d = pkg.HipFeasibility(pkg.Feasibility(pkg.IndBallL1(2.0), pkg.IndBox(0.0, 1.0), n))
    x = np.random.default_rng(4).standard_normal(n)
    before = d.prox(1, x)
    i32p, i64p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)

    def raw(kinds, lens, scal, vec):
        kinds, lens, scal = np.array(kinds, dtype=np.int32), np.array(lens, dtype=np.int64), np.array(scal, dtype=np.float64)
        return lib.fos_feas_set_blocks(d._h, 1, len(kinds), kinds.ctypes.data_as(i32p), lens.ctypes.data_as(i64p), pkg.lib.dptr(scal),
                                       None if vec is None else pkg.lib.dptr(np.asarray(vec, dtype=np.float64)))
    assert raw([c["IndFree"], c["IndFree"]], [20, 20], [0.0] * 4, None) == FOS_EINVAL                       # lengths not summing to n
    assert raw([c["IndFree"], c["IndFree"]], [20, 40], [0.0] * 4, None) == FOS_EINVAL and "block 2" in lib.fos_last_error().decode()
    assert raw([c["IndFree"], 8], [20, 30], [0.0] * 4, None) == FOS_EINVAL and "block 2" in lib.fos_last_error().decode()      # an unknown kind
    assert raw([c["IndFree"], c["IndHalfspace"]], [20, 30], [0.0] * 4, np.zeros(n)) == FOS_EINVAL and "block 2" in lib.fos_last_error().decode()      # a zero normal
    assert np.array_equal(d.prox(1, x), before)                                 # the previous set is still there
    with pytest.raises(pkg.lib.FosError):
        d.set_stats(2)                                                          # (an IndBox of fos_feas_set_box)
    # a callback set replaced by a block set and back, on one handle
    ref = RefBallL2(1.5, np.ones(n))
    d.set_callback(1, ref)
    y_cb = d.prox(1, x)
    assert ref.calls == 1 and np.array_equal(y_cb, ref.project(x))
    d.set_blocks(1, *_pack(pkg, pkg.IndBallL2(1.5, np.ones(n)), n))
    y_dev = d.prox(1, x)
    assert ref.calls == 1 and np.abs(y_dev - y_cb).max() <= 1e-13 * np.abs(x).max()
    d.set_callback(1, ref)
    assert np.array_equal(d.prox(1, x), y_cb) and ref.calls == 2
    with pytest.raises(pkg.lib.FosError):
        d.set_stats(1)
