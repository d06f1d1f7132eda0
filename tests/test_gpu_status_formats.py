"""
The status epilogue (EpiQStatus: checkstatus, HSDEStatus.jl:27-63) and its siblings EpiQVfromU / EpiQRhs on every storage format of the
operator, against the extended-precision reference of tests/status_reference.py at TWICE its worst-case fp64 allowance and nothing else.

Operators: every shape of test_gpu_parity.shapes() (row blocks in ELL / LDS / LONG form, run-compressed values, dual tiles with deferred
rows, all-zero) as the library stores it by itself, and the four shapes of test_operators_on_forced_window_panels under FOS_WINDOWS = 1
and 2 (window panels of both geometries).  Which sweep a case runs follows from its operator_stats(): no deferred rows -> q1_kernel<.., false>
(or q1_win_kernel<Geo, .., false>), deferred rows -> q1_kernel<.., true> / q1_win_kernel<Geo, .., true> followed by q1_deferred_kernel with
fold_sweep_records.  The worst error / allowance is printed per field and per storage class (test_zz_report).
"""
import json
import os
import subprocess
import sys
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp

import fos_oracle as orc
import status_cases as cases
import status_reference as sref

pytestmark = pytest.mark.gpu

ROW_NAMES = [name for name, _ in cases.row_block_shapes()]
OPERATORS = [(name, None) for name in ROW_NAMES] + [(name, geom) for geom in ("1", "2") for name in cases.WINDOW_NAMES]
OP_IDS = ["%s%s" % (name, "" if geom is None else "-win" + geom) for name, geom in OPERATORS]

WORST = {}            # storage class -> field -> worst |device - reference| / allowance
STATS = {}            # operator id -> operator_stats()


@lru_cache(maxsize=None)
def _matrices(windows):
    return {name: sp.csc_matrix(A) for name, A in (cases.window_shapes() if windows else cases.row_block_shapes())}


def _problem(name, geom, scaled=False):
    A = _matrices(geom is not None)[name]
    b, c = cases.vectors_for(name, A)
    if scaled:
        return cases.scaled_problem(name, A, b, c)
    return A, b, c, None


def _make(pkg, A, b, c, geom, K1=None, K2=None):
    """a handle with the operator stored as FOS_WINDOWS = geom asks (None: the library's own choice)"""
    old = os.environ.pop("FOS_WINDOWS", None)
    try:
        if geom is not None:
            os.environ["FOS_WINDOWS"] = geom
        m, n = A.shape
        return pkg.HipHSDE(A, b, c, K1 or [("Free", m)], K2 or [("Free", n)])
    finally:
        os.environ.pop("FOS_WINDOWS", None)
        if old is not None:
            os.environ["FOS_WINDOWS"] = old


@pytest.fixture(scope="module")
def store(pkg):
    """handles by (operator, geometry, scaled), built on first use and closed with the module"""
    made = {}

    def get(name, geom, scaled=False):
        key = (name, geom, scaled)
        if key not in made:
            A, b, c, z = _problem(name, geom, scaled)
            made[key] = (_make(pkg, A, b, c, geom), A, b, c, z)
        return made[key]
    yield get
    for d, *_ in made.values():
        d.close()


def storage_classes(st, geom):
    out = []
    if st["win_panels"] > 0:
        out.append("window panels, geometry %s%s" % (geom, " + deferred rows" if st["deferred"] > 0 else ""))
    else:
        if st["blocks"] > 0:
            out.append("row blocks")
        if st["tiles"] > 0:
            out.append("dual tiles")
        if st["deferred"] > 0:
            out.append("deferred rows")
    return out or ["empty operator"]


def _got(res):
    return dict(p=res.p, d=res.d, g=res.g, ctx=res.ctx, bty=res.bty, nAxs=res.norm_axs, nATy=res.norm_aty, nb=res.norm_b, nc=res.norm_c,
                tau=res.tau, kappa=res.kappa)


def _record(classes, rat):
    for cl in classes:
        w = WORST.setdefault(cl, {})
        for k, v in rat.items():
            w[k] = max(w.get(k, 0.0), v)


def _compare(pkg, d, A, b, c, z, label, classes):
    """every field within 2 x allowance; the decision at both eps where the reference is clear of its thresholds -> status comparisons skipped"""
    vals, allow = sref.reference(A, b, c, z)
    skipped = 0
    for eps in cases.EPS:
        res = d.check(z, eps)
        rat = sref.ratios(_got(res), vals, allow)
        _record(classes, rat)
        worst = max(rat, key=rat.get)
        print("  %-22s eps=%g  worst error / allowance %.3g (%s)  status %s" % (label, eps, rat[worst], worst, pkg.lib.STATUS_NAMES[res.status]))
        assert rat[worst] <= 2.0, (label, eps, rat)
        if sref.margin(vals, eps) > 2 * sref.relative_allowance(vals, allow, eps):
            assert pkg.lib.STATUS_NAMES[res.status] == sref.decide(vals, eps), (label, eps)
        else:
            skipped += 1
    return skipped


# ---------------------------------------------------------------------------------------------- the status sums, every format


@pytest.mark.parametrize("name,geom", OPERATORS, ids=OP_IDS)
def test_status_fields_and_decision(pkg, store, name, geom):
    """fos_check on unit-scale points with tau in {1e-6, 1, 1e6}, a point supported on one row and one column (a record read at the wrong
    stride shows as an exact zero or a doubled term), tau < 0, tau = 0 (the Inf / NaN pattern of Julia's division), an exactly consistent
    point (p, d at rounding level: the allowance keeps the comparison meaningful) and a problem whose rows, b, c and z are scaled over
    twelve decades: every field of fos_check_result within 2 x allowance of the reference, the status the reference's."""
    d, A, b, c, _ = store(name, geom)
    st = d.operator_stats()
    STATS[OP_IDS[OPERATORS.index((name, geom))]] = st
    classes = storage_classes(st, geom)
    if geom is not None:
        assert st["win_panels"] > 0 and st["blocks"] == 0, st
    print("%s: %s  %s" % (name, classes, {k: v for k, v in st.items() if v}))
    skipped = total = 0
    for label, z in cases.points(name, A, b, c):
        skipped += _compare(pkg, d, A, b, c, z, label, classes)
        total += len(cases.EPS)
    ds, As, bs, cs, zs = store(name, geom, scaled=True)
    assert storage_classes(ds.operator_stats(), geom) == classes          # (row scaling keeps the pattern, hence the format)
    skipped += _compare(pkg, ds, As, bs, cs, zs, "scaled 1e-6..1e6", classes)
    total += len(cases.EPS)
    assert skipped <= 0.05 * total, (skipped, total)


def test_every_storage_class_is_hit(pkg, store):
    seen = dict(tiles_deferred=False, long=False, lds=False, win_panels=False, win_segments=False, win_deferred=False)
    for name, geom in OPERATORS:
        st = store(name, geom)[0].operator_stats()
        seen["tiles_deferred"] |= st["tiles"] > 0 and st["deferred"] > 0
        seen["long"] |= st["long"] > 0
        seen["lds"] |= st["lds"] > 0
        seen["win_panels"] |= st["win_panels"] > 0
        seen["win_segments"] |= st["win_segments"] > 64
        seen["win_deferred"] |= st["win_panels"] > 0 and st["deferred"] > 0
    print("storage classes reached:", seen)
    assert all(seen[k] for k in ("tiles_deferred", "long", "lds", "win_panels", "win_segments")), seen


@pytest.mark.parametrize("name,geom", [("tile-mixed", None), ("tall", "1")], ids=["tile-mixed", "tall-win1"])
def test_constructed_certificates(pkg, store, name, geom):
    """One constructed Optimal, Unbounded, Infeasible and Continue point each on a tile-stored and a window-panel operator, every one at
    least 1e-3 (relative) from each threshold: the device's verdict is the constructed one at both eps."""
    d, A, b, c, _ = store(name, geom)
    st = d.operator_stats()
    assert (st["win_panels"] > 0) if geom else (st["tiles"] > 0 and st["deferred"] > 0), st
    classes = storage_classes(st, geom)
    for want, z in cases.certificates(A, b, c):
        vals, allow = sref.reference(A, b, c, z)
        for eps in cases.EPS:
            assert sref.decide(vals, eps) == want and sref.margin(vals, eps) >= 1e-3
        assert _compare(pkg, d, A, b, c, z, want, classes) == 0
        for eps in cases.EPS:
            assert pkg.lib.STATUS_NAMES[d.check(z, eps).status] == want, (want, eps)


# ---------------------------------------------------------------------------------------------- in the loop, behind a communicator

DOUBLE_FIELDS = ("p", "d", "g", "ctx", "bty", "kappa", "tau", "norm_axs", "norm_aty", "norm_b", "norm_c")


@pytest.mark.parametrize("name,geom", [("tile-mixed", None), ("mixed-lengths", None), ("mid", "1")], ids=["tile-mixed", "mixed-lengths", "mid-win1"])
def test_in_loop_check_equals_stand_alone_check(pkg, name, geom):
    """20 DR iterations with checki = 10: the fos_check_result that fos_step returns at iteration 20 is, bit for bit, fos_check of
    fos_get_checked() -- the same kernels on the same vector -- and lies within 2 x allowance of the reference."""
    A = _matrices(geom is not None)[name]
    m, n = A.shape
    prob = pkg.workloads.from_complementary_pair(name, A, [("Zero", m)], [("NonNeg", n)], np.random.default_rng(cases._seed("loop", name)))
    d = _make(pkg, prob.A, prob.b, prob.c, geom, prob.K1, prob.K2)
    try:
        d.set_alg(pkg.DR())
        d.set_iterate(None)
        eps = 1e-8
        done, checked, res = d.step(1, 10, 10, eps)
        assert done == 10 and checked
        done, checked, res = d.step(11, 10, 10, eps)
        assert done == 10 and checked
        z = d.get_checked()
        alone = d.check(z, eps)
        diff = [k for k in DOUBLE_FIELDS if np.float64(getattr(res, k)).tobytes() != np.float64(getattr(alone, k)).tobytes()]
        print("%s: in-loop vs stand-alone check, fields that differ: %s" % (name, diff or "none"))
        assert not diff, [(k, getattr(res, k), getattr(alone, k)) for k in diff]
        assert res.status == alone.status
        vals, allow = sref.reference(prob.A, prob.b, prob.c, z)
        rat = sref.ratios(_got(res), vals, allow)
        _record(storage_classes(d.operator_stats(), geom), rat)
        assert max(rat.values()) <= 2.0, rat
    finally:
        d.close()


@pytest.mark.parametrize("name", ["tile-mixed", "sparse"])
def test_check_behind_a_one_rank_communicator(pkg, store, name):
    """After comm_init(1, 0, id) the sums go through the local reduce kernel and the all-reduce, and status_finalize_kernel reads the
    reduced buffer (from_reduced) with the replicated entries counted once: same values as the reference, and as the plain handle's,
    at 2 x allowance."""
    d0, A, b, c, _ = store(name, None)
    d1 = _make(pkg, A, b, c, None)
    try:
        d1.comm_init(1, 0, pkg.HipHSDE.comm_unique_id())
        classes = ["one-rank communicator"]
        for label, z in cases.points(name, A, b, c):
            _compare(pkg, d1, A, b, c, z, label, classes)
            vals, allow = sref.reference(A, b, c, z)
            g0, g1 = _got(d0.check(z, 1e-8)), _got(d1.check(z, 1e-8))
            rat = sref.ratios(g1, {k: np.longdouble(v) for k, v in g0.items()}, allow)
            assert max(rat.values()) <= 2.0, (label, rat)
    finally:
        d1.close()


# ---------------------------------------------------------------------------------------------- EpiQVfromU, EpiQRhs


def _vfromu_ratio(A, b, c, y):
    l = sum(A.shape) + 1
    u, v = y[:l], y[l:]
    assert np.all(np.isfinite(y))
    Qu, E = sref.stacked_q_reference(A, b, c, u)
    diff = np.abs(v.astype(np.longdouble) - Qu)
    with np.errstate(divide="ignore", invalid="ignore"):
        rat = np.where(diff == 0, 0.0, diff / E).astype(np.float64)
    return float(rat[:-1].max()), float(rat[-1])


@pytest.mark.parametrize("name,geom", OPERATORS, ids=OP_IDS)
def test_vfromu_to_rounding(pkg, store, name, geom):
    """y = hsdematrix_prox(x) = (u, Q u) (HSDEAffine.jl:105-126): the kernel wrote v = Q u from the u it stored, so whatever the CG solve
    left in u,  |v - Q u|_i <= 2 u (k_i + 3) (|Q||u|)_i  for every row, and the tau row within 2 (l + 8) u sum |[c; b]_i u_i|."""
    d, A, b, c, _ = store(name, geom)
    rng = np.random.default_rng(cases._seed("vfromu", name))
    y = d.hsdematrix_prox(rng.standard_normal(d.N))
    rows, taurow = _vfromu_ratio(A, b, c, y)
    print("%s: EpiQVfromU worst error / allowance: rows %.3g, tau row %.3g (CG iterations %d)" % (name, rows, taurow, d.cgiter()))
    _record(["EpiQVfromU: " + cl for cl in storage_classes(d.operator_stats(), geom)], {"rows": rows, "tau row": taurow})
    assert rows <= 2.0 and taurow <= 2.0


DIRECT_FORMS = [("tile-mixed", "auto", "newton"), ("tile-blockdiag", "auto", "newton"), ("tile-mixed", "reduced", "newton"), ("sparse", "auto", "cholesky"),
                ("sparse", "reduced", "cholesky")]


DIRECT_IDS = ["%s-%s-%s" % t for t in DIRECT_FORMS]


@pytest.fixture(scope="module")
def direct_outputs(pkg):
    """(mode, x, hsdematrix_prox(x), prox_affine(x)) of each direct form: computed once, shared by the three tests below"""
    made = {}

    def get(name, form, factor):
        key = (name, form, factor)
        if key not in made:
            A = _matrices(False)[name]
            b, c = cases.vectors_for(name, A)
            d = _make(pkg, A, b, c, None)
            try:
                d.enable_direct(A, form=form, factor=factor)
                x = np.random.default_rng(cases._seed("direct", name, form)).standard_normal(d.N)
                made[key] = (A, b, c, d.direct_mode(), x, d.hsdematrix_prox(x), d.prox_affine(x))
            finally:
                d.close()
        return made[key]
    return get


@pytest.mark.parametrize("name,form,factor", DIRECT_FORMS, ids=DIRECT_IDS)
def test_vfromu_hsdematrix_prox_with_direct_enabled(direct_outputs, name, form, factor):
    """The bound of test_vfromu_to_rounding on y = hsdematrix_prox(x) with direct = true in each form a small operator admits (dense,
    block, reduced; both factors)."""
    A, b, c, mode, x, y, _ = direct_outputs(name, form, factor)
    rows, taurow = _vfromu_ratio(A, b, c, y)
    print("%s direct form %s (%s): hsdematrix_prox: |v - Q u| worst error / allowance: rows %.3g, tau row %.3g" % (name, mode, factor, rows, taurow))
    assert rows <= 2.0 and taurow <= 2.0, (mode, rows, taurow)


@pytest.mark.parametrize("name,form,factor", DIRECT_FORMS, ids=DIRECT_IDS)
def test_vfromu_prox_affine_with_direct_enabled(direct_outputs, name, form, factor):
    """The same bound on y = prox_affine(x) with direct = true:  |v - Q u|_i <= 2 u (k_i + 3) (|Q||u|)_i.

    The dense and the reduced form find u+ = u + Q w with w = (I + Q Q')^-1 (Q u - v) from a stored inverse; v + w equals Q u+ only as far as
    that inverse solves its system (12 .. 2730 x this allowance when the projection still returned it), so the projection ends with a sweep
    that writes (u+, Q u+).  The block form returns (u^, Q u^)."""
    A, b, c, mode, x, _, y = direct_outputs(name, form, factor)
    rows, taurow = _vfromu_ratio(A, b, c, y)
    print("%s direct form %s (%s): prox_affine: |v - Q u| worst error / allowance: rows %.3g, tau row %.3g" % (name, mode, factor, rows, taurow))
    assert rows <= 2.0 and taurow <= 2.0, (mode, rows, taurow)


RHS_CHILD = r"""
import json, sys
import numpy as np, scipy.sparse as sp
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests", sys.argv[1] + "/oracle"]
import __graft_entry__ as ge
import status_cases as cases
pkg = ge.load_package()
out = {}
for name, A in cases.row_block_shapes():
    if name not in sys.argv[2:]:
        continue
    A = sp.csc_matrix(A)
    b, c = cases.vectors_for(name, A)
    m, n = A.shape
    d = pkg.HipHSDE(A, b, c, [("Free", m)], [("Free", n)])
    x = np.random.default_rng(cases._seed("rhs", name)).standard_normal(d.N)
    d.prox_affine(np.random.default_rng(1).standard_normal(d.N))       # any call: the counter and the warm start leave their first state
    d.reset_affine()
    y = d.prox_affine(x)
    out[name] = dict(y=y.tolist(), cgiter=d.cgiter(), count=d.prox_count())
    d.close()
print("RESULT " + json.dumps(out))
"""
RHS_NAMES = ("tiny-dense", "tile-1chunk", "sparse")


def test_rhs_epilogue_through_the_unfused_prox_affine(pkg, store):
    """EpiQRhs builds [x1 - Q x2; 0] (affinepluslinear.jl:94-95) only where the right-hand side is formed on its own: FOS_FUSED_RHS=0, which
    the library reads once per process -- hence one child process, which is what this test is about.  There the first prox_affine after
    reset_affine() is compared with the oracle's first call at the tolerance of test_prox_affine_sequence (CG iterations within 4,
    ||y - y_oracle|| <= 2 tol + 1e-12, ||M y - rhs|| <= tol (1 + 1e-9)); the distance to this process's fused result (the same system from
    the same start, the right-hand side never formed) is printed.
    The epilogue is isolated no further: its output h->RHS never leaves the device (no C ABI entry reads it, and none is added for a test),
    so it is seen only through the CG solve that consumes it, whose first tolerance is 0.2.  On the SCALED problems of this module the
    oracle's own CG runs into its cap of 1000 iterations on that first call, so the unscaled operators are used."""
    root = Path(__file__).resolve().parent.parent
    env = dict(os.environ, FOS_FUSED_RHS="0")
    env.pop("FOS_WINDOWS", None)
    run = subprocess.run([sys.executable, "-c", RHS_CHILD, str(root)] + list(RHS_NAMES), env=env, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    got = json.loads([ln for ln in run.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert sorted(got) == sorted(RHS_NAMES)
    for name in RHS_NAMES:
        d, A, b, c, _ = store(name, None)
        l = d.l
        x = np.random.default_rng(cases._seed("rhs", name)).standard_normal(d.N)
        Q = orc.HSDEMatrixQ(A, b, c)
        S = orc.AffinePlusLinear(Q, np.zeros(l), np.zeros(l), 1, decreasing_accuracy=True)
        tol = S.tolerance()
        y_ref = np.empty(d.N)
        S.prox(y_ref, x)
        y = np.asarray(got[name]["y"])
        Qd = Q.todense()
        Md = np.block([[np.eye(l), Qd.T], [Qd, -np.eye(l)]])
        rhs = np.concatenate([x[:l] + Qd.T @ x[l:], np.zeros(l)])
        d.reset_affine()
        y_fused = d.prox_affine(x)
        print("%s: unfused prox_affine: CG iterations %d (oracle %d, fused %d), ||y - y_oracle|| = %.3g, ||y - y_fused|| = %.3g, tol = %g" %
              (name, got[name]["cgiter"], S.getcgiter(), d.cgiter(), np.linalg.norm(y - y_ref), np.linalg.norm(y - y_fused), tol))
        assert got[name]["count"] == S.i == 2
        assert abs(got[name]["cgiter"] - S.getcgiter()) <= 4
        assert np.linalg.norm(y - y_ref) <= 2 * tol + 1e-12
        assert np.linalg.norm(Md @ y - rhs) <= tol * (1 + 1e-9)


# ---------------------------------------------------------------------------------------------- report


def test_zz_report():
    """prints the worst error / allowance per storage class and field gathered by the tests above (nothing to report when run alone)"""
    for cl in sorted(WORST):
        print("%-45s %s" % (cl, ", ".join("%s %.3g" % kv for kv in sorted(WORST[cl].items()))))
    for op in sorted(STATS):
        print("%-22s %s" % (op, {k: v for k, v in STATS[op].items() if v}))
    for cl, w in WORST.items():
        assert max(w.values()) <= 2.0, (cl, w)
