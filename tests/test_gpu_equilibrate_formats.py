"""
The status check of an EQUILIBRATED handle (status_check of csrc/step.cpp: the Q_PLAIN_NOTAU sweep of the scaled operator, then eq_status_kernel) on every storage
format of the operator, against the extended-precision reference ON THE CALLER'S DATA at twice the worst-case fp64 allowance of
tests/equilibrate_status.py and nothing else -- the standard test_gpu_status_formats.py sets for a plain handle.

Operators: those of test_gpu_status_formats.py (row blocks in ELL / LDS / LONG form, run-compressed values, dual tiles with deferred rows, all-zero; the
four window shapes under FOS_WINDOWS = 1 and 2), each with equilibrate = 1 and 10; sparse LPs with l = 63, 64, 65 and n + m > 131 072 (the wavefront
and grid-stride edges of eq_status_kernel); a dual-tile and a window operator with SOC and SDP cones on both sides (the block means).  Every case is
checked on the CPU first (test_equilibrate_status_cpu.py): the reference is clear of every threshold, so the status is asserted everywhere.
"""
import os

import numpy as np
import pytest
import scipy.sparse as sp

import equilibrate_status as es
import status_cases as cases
import status_reference as sref
from test_gpu_status_formats import OP_IDS, OPERATORS, _got, _matrices, storage_classes

pytestmark = pytest.mark.gpu

WORST = {}            # storage class -> field -> worst |device - reference| / allowance


def _make(pkg, A, b, c, geom, K1=None, K2=None, equilibrate=0):
    """test_gpu_status_formats._make with the equilibration option"""
    old = os.environ.pop("FOS_WINDOWS", None)
    try:
        if geom is not None:
            os.environ["FOS_WINDOWS"] = geom
        m, n = A.shape
        return pkg.HipHSDE(A, b, c, K1 or [("Free", m)], K2 or [("Free", n)], equilibrate=equilibrate)
    finally:
        os.environ.pop("FOS_WINDOWS", None)
        if old is not None:
            os.environ["FOS_WINDOWS"] = old


def _record(classes, rat):
    for cl in classes:
        w = WORST.setdefault(cl, {})
        for k, v in rat.items():
            w[k] = max(w.get(k, 0.0), v)


def _compare(pkg, d, A, b, c, z, label, classes, want=None):
    """every field within 2 x allowance (non-finite ones as patterns), the status the reference's -- the margin rule of the plain test, which the CPU
    test has shown to hold on every case here, so nothing is skipped"""
    vals, allow = es.reference(A, b, c, z)
    for eps in cases.EPS:
        res = d.check(z, eps)
        rat = sref.ratios(_got(res), vals, allow)
        _record(classes, rat)
        worst = max(rat, key=rat.get)
        print("  %-24s eps=%g  worst error / allowance %.3g (%s)  status %s" % (label, eps, rat[worst], worst, pkg.lib.STATUS_NAMES[res.status]))
        assert rat[worst] <= 2.0, (label, eps, rat)
        assert sref.margin(vals, eps) > 2 * sref.relative_allowance(vals, allow, eps), (label, eps)
        assert pkg.lib.STATUS_NAMES[res.status] == sref.decide(vals, eps), (label, eps)
        if want is not None:
            assert pkg.lib.STATUS_NAMES[res.status] == want, (label, eps)


def _same_format_and_bits(pkg, d, A, b, c, K1, K2, geom, passes, classes):
    """the equilibrated handle IS the plain handle of host_equilibrate's data: the same storage class, bit-identical Q and Q' products"""
    host = pkg.host_equilibrate(A, b, c, K1, K2, passes)
    plain = _make(pkg, host["A"], host["b"], host["c"], geom, K1, K2)
    try:
        assert storage_classes(plain.operator_stats(), geom) == classes
        assert plain.operator_stats() == d.operator_stats()
        got = d.equilibration()
        assert got["passes"] == passes and np.array_equal(got["D"], host["D"]) and np.array_equal(got["E"], host["E"])
        u = np.random.default_rng(cases._seed("q", A.shape)).standard_normal(d.l)
        for transpose in (False, True):
            assert np.array_equal(d.q_apply(u, transpose=transpose), plain.q_apply(u, transpose=transpose)), transpose
    finally:
        plain.close()


def _run(pkg, name, A, b, c, geom, passes, K1=None, K2=None, certificates=False, want_class=None, title=None):
    A = sp.csc_matrix(A)
    handles = {}
    try:
        for label, Ap, bp, cp, z, want in es.point_sets(name, A, b, c, certificates):
            if id(Ap) not in handles:                                # (the operator as it stands, then its scaled problem)
                d = _make(pkg, Ap, bp, cp, geom, K1, K2, equilibrate=passes)
                st = d.operator_stats()
                classes = storage_classes(st, geom)
                if geom is not None:
                    assert st["win_panels"] > 0 and st["blocks"] == 0, st
                if want_class is not None:
                    assert want_class in " ".join(classes), classes
                if not handles:
                    print("%s, %d passes: %s  %s" % (title or name, passes, classes, {k: v for k, v in st.items() if v}))
                    m, n = Ap.shape
                    _same_format_and_bits(pkg, d, Ap, bp, cp, K1 or [("Free", m)], K2 or [("Free", n)], geom, passes, classes)
                handles[id(Ap)] = (d, classes)
            d, classes = handles[id(Ap)]
            _compare(pkg, d, Ap, bp, cp, z, label, classes, want)
    finally:
        for d, _ in handles.values():
            d.close()


@pytest.mark.parametrize("passes", es.PASSES)
@pytest.mark.parametrize("name,geom", OPERATORS, ids=OP_IDS)
def test_status_in_the_callers_units_on_every_format(pkg, name, geom, passes):
    """fos_check of an equilibrated handle on the points of status_cases (tau in {1e-6, 1, 1e6}, one row and one column, tau < 0, tau = 0, consistent),
    its scaled problem, and on the thin operators one constructed point per verdict: every field within 2 x allowance of the reference on the caller's
    data, Inf / NaN where the reference has them, the status the reference's; the handle stores the operator as a plain handle of the scaled data does
    and multiplies to the same bits."""
    A = _matrices(geom is not None)[name]
    b, c = cases.vectors_for(name, A)
    _run(pkg, name, A, b, c, geom, passes, certificates=name in es.CERTIFICATE_OPERATORS)


@pytest.mark.parametrize("passes", es.PASSES)
@pytest.mark.parametrize("m,n", es.EDGE_SHAPES, ids=["l=63", "l=64", "l=65", "two-grid-trips"])
def test_status_at_the_kernels_edges(pkg, m, n, passes):
    """l = n + m + 1 = 63, 64, 65 (a partial, a full, a just-exceeded wavefront) and n + m > 131 072 (the second trip of the grid-stride loop) meet the
    tau = 1e6 and tau = 0 points as well"""
    assert (m + n + 1) in (63, 64, 65) or m + n > 512 * 256
    name, A, b, c = es.edge_problem(pkg, m, n)
    K1 = [("Zero", m // 2), ("NonNeg", m - m // 2)]
    _run(pkg, name, A, b, c, None, passes, K1=K1, K2=[("NonNeg", n)])


@pytest.mark.parametrize("name,geom,want_class", [("tile-mixed", None, "dual tiles"), ("tall", "1", "window panels")], ids=["tile-mixed", "tall-win1"])
def test_status_with_coupling_cones(pkg, name, geom, want_class):
    """SOC and SDP blocks in K1 and K2: the factors are block means (constant on each such cone), the check holds the same bounds"""
    A = _matrices(geom is not None)[name]
    b, c = cases.vectors_for(name, A)
    K1, K2 = es.CONE_VARIANTS[name]
    d = _make(pkg, A, b, c, geom, K1, K2, equilibrate=10)
    try:
        eq = d.equilibration()
        for v, K in ((eq["D"], K1), (eq["E"], K2)):
            at = 0
            for kind, length in K:
                if kind in ("SOC", "SDP"):
                    assert np.all(v[at:at + length] == v[at]), (kind, at)
                at += length
            assert len(np.unique(v)) > 3
    finally:
        d.close()
    _run(pkg, name, A, b, c, geom, 10, K1=K1, K2=K2, want_class=want_class, title=name + " (SOC, SDP)")


@pytest.mark.parametrize("passes", es.PASSES)
def test_every_storage_class_is_hit_by_equilibrated_handles(pkg, passes):
    """the counterpart of test_gpu_status_formats.test_every_storage_class_is_hit: the EQUILIBRATED handles of the operators above reach dual tiles
    with deferred rows, LONG and LDS row blocks, window panels and a panel of more than 64 segments.  (Run-compressed values are not asked for, there
    or here: compression depends on repeated values, which scaling by D and E need not keep.)"""
    seen = dict(tiles_deferred=False, long=False, lds=False, win_panels=False, win_segments=False, win_deferred=False, run=False)
    for name, geom in OPERATORS:
        A = _matrices(geom is not None)[name]
        b, c = cases.vectors_for(name, A)
        d = _make(pkg, A, b, c, geom, equilibrate=passes)
        try:
            assert d.equilibration()["passes"] == passes
            st = d.operator_stats()
        finally:
            d.close()
        seen["tiles_deferred"] |= st["tiles"] > 0 and st["deferred"] > 0
        seen["long"] |= st["long"] > 0
        seen["lds"] |= st["lds"] > 0
        seen["run"] |= st["run"] > 0
        seen["win_panels"] |= st["win_panels"] > 0
        seen["win_segments"] |= st["win_segments"] > 64
        seen["win_deferred"] |= st["win_panels"] > 0 and st["deferred"] > 0
    print("storage classes reached by equilibrated handles, %d passes: %s" % (passes, seen))
    assert all(seen[k] for k in ("tiles_deferred", "long", "lds", "win_panels", "win_segments")), seen


def test_zz_report():
    """prints the worst error / allowance per storage class and field gathered by the tests above (nothing to report when run alone)"""
    for cl in sorted(WORST):
        print("%-45s %s" % (cl, ", ".join("%s %.3g" % kv for kv in sorted(WORST[cl].items()))))
    for cl, w in WORST.items():
        assert max(w.values()) <= 2.0, (cl, w)
