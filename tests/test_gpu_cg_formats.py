"""
The CG kernels (kkt2_kernel / kkt2_win_kernel with the CG epilogue and its three fused sums, cg_update, cg_pupdate, cg_stop_check,
cgm_start / cgm_update, cg_init / cg_init_finalize) on every storage format of the operator, iteration by iteration, against the
extended-precision recurrence of tests/cg_reference.py at the allowance measured there (4 x the worst fp64 evaluation of the reference)
and nothing else.

Operators: every shape of status_cases.row_block_shapes() as the library stores it by itself and the four shapes of
status_cases.window_shapes() under FOS_WINDOWS = 1 and 2; starts: the tamed warm and cold starts (k = 1 .. 4) and the raw one (k = 1) of
tests/cg_cases.py; variants: reference, fused_p, merged_sweep, merged_update, switched on the live handle.  Every element is judged
alike, the deferred rows, the tau element l - 1 and its twin N - 1 included.

fused_p exists for row-block and tile storage only: the window-panel sweeps have no form that closes the previous iteration and builds
p on the fly, so fos_set_cg_variant(FOS_CG_FUSED_P) and fos_set_tuning(fuse_p = 1) refuse it there with FOS_EUNSUPPORTED, and that refusal
is what this file asserts on the window operators.
"""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import cg_cases as cases
import cg_reference as cref

pytestmark = pytest.mark.gpu

VARIANTS = ("reference", "fused_p", "merged_sweep", "merged_update")
OPERATORS = [(name, None) for name in cases.row_names()] + [(name, geom) for geom in ("1", "2") for name in cases.window_names()]
OP_IDS = ["%s%s" % (name, "" if geom is None else "-win" + geom) for name, geom in OPERATORS]
DEFAULT_CHUNK = 8                    # CgState::cg_chunk

WORST = {}            # storage class -> variant -> worst |device - reference| / allowance
STATS = {}            # operator id -> operator_stats()


def _make(pkg, A, b, c, geom):
    """a handle with the operator stored as FOS_WINDOWS = geom asks (None: the library's own choice)"""
    old = os.environ.pop("FOS_WINDOWS", None)
    try:
        if geom is not None:
            os.environ["FOS_WINDOWS"] = geom
        m, n = A.shape
        return pkg.HipHSDE(A, b, c, [("Free", m)], [("Free", n)])
    finally:
        os.environ.pop("FOS_WINDOWS", None)
        if old is not None:
            os.environ["FOS_WINDOWS"] = old


def _operator(name, scaled):
    return cases.scaled_operator(name) if scaled else cases.operators()[name][:3]


@pytest.fixture(scope="module")
def store(pkg):
    """handles by (operator, geometry, scaled), built on first use and closed with the module"""
    made = {}

    def get(name, geom, scaled=True):
        key = (name, geom, scaled)
        if key not in made:
            made[key] = _make(pkg, *_operator(name, scaled), geom)
        return made[key]
    yield get
    for d in made.values():
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


def _classes(d, name, geom):
    st = d.operator_stats()
    STATS[OP_IDS[OPERATORS.index((name, geom))]] = st
    if geom is not None:
        assert st["win_panels"] > 0 and st["blocks"] == 0, st
    return storage_classes(st, geom)


def _record(classes, variant, rat):
    for cl in classes:
        w = WORST.setdefault(cl, {})
        w[variant] = max(w.get(variant, 0.0), rat)


def _variants(pkg, d):
    """the variants the handle's storage admits; on window panels fused_p must be refused (and leaves the handle's variant as it was)"""
    if d.operator_stats()["win_panels"] == 0:
        return VARIANTS
    d.set_cg_variant("reference")
    for ask in (lambda: d.set_cg_variant("fused_p"), lambda: d.set_tuning(fuse_p=1)):
        with pytest.raises(pkg.lib.FosError) as err:
            ask()
        assert err.value.code == -4 and "window" in str(err.value), str(err.value)          # FOS_EUNSUPPORTED
        assert d.cg_variant_name() == "reference"
    return tuple(v for v in VARIANTS if v != "fused_p")


def _alpha0(x1, cs):
    """(alpha_0 recovered from x_1 - x_0, the extended alpha_0): which of the sweep's sums is off when x_1 misses its allowance"""
    ext = cref.extended(cs)
    r0 = ext.r0
    return float(np.sum((np.asarray(x1, dtype=cref.LD) - np.asarray(cs.x0, dtype=cref.LD)) * r0) / np.sum(r0 * r0)), float(ext.alphas[0])


def _judge(bad, classes, variant, what, cs, k, x, it, want_it):
    rat = cref.ratio(x, cs, k)
    _record(classes, variant, rat)
    if it != want_it or not rat <= 1.0:
        a_dev, a_ext = _alpha0(x, cs) if k == 1 else (np.nan, np.nan)
        bad.append("%s %s %s k=%d: iterations %d (want %d), error / allowance %.3g (allowance %.3g = %.3g max|x_k|)%s" %
                   (cs.name, variant, what, k, it, want_it, rat, cref.allowance(cs, k), cref.relative_allowance(cs, k),
                    "" if k != 1 else ", alpha_0 %.17g against %.17g (relative %.3g)" % (a_dev, a_ext, abs(a_dev - a_ext) / abs(a_ext))))
    return rat


def _cases(name):
    return [cases.case(name, start) for start in cases.STARTS]


# ---------------------------------------------------------------------------------------------- iterates, stop rule, bits


@pytest.mark.parametrize("name,geom", OPERATORS, ids=OP_IDS)
def test_iterates_to_rounding(pkg, store, name, geom):
    """cg_kkt(x0, rhs, 1e-300, k): k iterations counted, every element of the result within the allowance of the extended x_k, for every
    variant, start and k; the last solve of each start a second time, bit for bit."""
    bad = []
    for cs in _cases(name):
        d = store(name, geom, scaled=not cs.name.endswith("/raw"))
        classes = _classes(d, name, geom)
        for variant in _variants(pkg, d):
            d.set_cg_variant(variant)
            assert d.cg_variant_name() == variant
            worst = 0.0
            for k in cs.ks:
                x, it = d.cg_kkt(cs.x0, cs.rhs, 1e-300, k)
                worst = max(worst, _judge(bad, classes, variant, "iterates", cs, k, x, it, k))
            x2, it2 = d.cg_kkt(cs.x0, cs.rhs, 1e-300, max(cs.ks))
            if it2 != it or not np.array_equal(x, x2):
                bad.append("%s %s: the same solve twice differs (max %.3g)" % (cs.name, variant, float(np.max(np.abs(x - x2)))))
            print("  %-30s %-13s worst error / allowance %.3g" % (cs.name, variant, worst))
        d.set_cg_variant(None)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("name,geom", OPERATORS, ids=OP_IDS)
def test_stop_rule_is_decisive(pkg, store, name, geom):
    """cg_kkt(x0, rhs, decisive_tol(case, k), 10000) on the tamed starts: the count is k exactly for k = 2, 3 and every variant, the result
    x_k within the allowance."""
    bad = []
    d = store(name, geom)
    classes = _classes(d, name, geom)
    for cs in _cases(name)[:2]:
        for variant in _variants(pkg, d):
            d.set_cg_variant(variant)
            for k in (2, 3):
                x, it = d.cg_kkt(cs.x0, cs.rhs, cref.decisive_tol(cs, k), 10000)
                _judge(bad, classes, variant, "stop rule", cs, k, x, it, k)
    d.set_cg_variant(None)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("name,geom", OPERATORS, ids=OP_IDS)
def test_cg_chunk_changes_no_bit(pkg, store, name, geom):
    """k = 4 under set_tuning(cg_chunk = 1) and 2 -- a following batch's sweep then repeats the closing of the batch before -- and the
    decisive stop at k = 3 likewise: bit-identical to the default batching for every variant (batching changes when launches are enqueued,
    never the arithmetic)."""
    bad = []
    d = store(name, geom)
    cs = cases.case(name, "warm")
    tol3 = cref.decisive_tol(cs, 3)
    try:
        for variant in _variants(pkg, d):
            d.set_cg_variant(variant)
            d.set_tuning(cg_chunk=DEFAULT_CHUNK)
            ref = [d.cg_kkt(cs.x0, cs.rhs, 1e-300, 4), d.cg_kkt(cs.x0, cs.rhs, tol3, 10000)]
            for chunk in (1, 2):
                d.set_tuning(cg_chunk=chunk)
                got = [d.cg_kkt(cs.x0, cs.rhs, 1e-300, 4), d.cg_kkt(cs.x0, cs.rhs, tol3, 10000)]
                for what, (x, it), (xr, itr) in zip(("k = 4", "stop at 3"), got, ref):
                    if it != itr or not np.array_equal(x, xr):
                        bad.append("%s %s cg_chunk=%d %s: iterations %d against %d, max difference %.3g" %
                                   (cs.name, variant, chunk, what, it, itr, float(np.max(np.abs(x - xr)))))
    finally:
        d.set_tuning(cg_chunk=DEFAULT_CHUNK)
        d.set_cg_variant(None)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("env", ["FOS_CG_FUSE_P", "FOS_CG_VARIANT"])
def test_fused_p_from_the_environment_leaves_window_panels_on_the_reference(pkg, monkeypatch, env):
    """FOS_CG_FUSE_P=1 / FOS_CG_VARIANT=1 are read when a handle is created and hold for every handle of the process: a row-block handle then
    runs fused_p, a window-panel handle the reference recurrence -- with right iterates, not the window sweep applied to the previous p."""
    monkeypatch.setenv(env, "1")
    for name, geom, want in (("sparse", None, "fused_p"), ("tall", "1", "reference")):
        cs = cases.case(name, "warm")
        d = _make(pkg, *_operator(name, True), geom)
        bad = []
        try:
            assert d.cg_variant_name() == want
            for k in cs.ks:
                x, it = d.cg_kkt(cs.x0, cs.rhs, 1e-300, k)
                _judge(bad, ["%s=1: %s" % (env, cl) for cl in _classes(d, name, geom)], want, "iterates", cs, k, x, it, k)
            d.set_iterate(None)
            assert d.bench_cg_chain(3, 1, 0) > 0.0                        # (the measurement entry resolves the variant the same way)
        finally:
            d.close()
        assert not bad, "\n".join(bad)


# ---------------------------------------------------------------------------------------------- prox_affine, twice


def _prox_alpha0(name, x, y):
    """alpha_0 of a first call that took one iteration, recovered from y - x = alpha_0 r_0 with r_0 = [0; x2 - Q x1]"""
    A, b, c = cases.scaled_operator(name)
    l = x.shape[0] // 2
    r2 = np.asarray(x[l:], dtype=cref.LD) - cref.q_mul(A, b, c, x[:l], cref.LD)
    return float(np.sum((np.asarray(y[l:], dtype=cref.LD) - np.asarray(x[l:], dtype=cref.LD)) * r2) / np.sum(r2 * r2))


@pytest.mark.parametrize("name,geom", OPERATORS, ids=OP_IDS)
def test_two_prox_affine_calls(pkg, name, geom):
    """Two consecutive prox_affine calls on a fresh handle (tolerances 0.2 and 0.2^sqrt(2); the first start is the input itself, the second
    the shifted warm start of the fused right-hand side), the inputs scaled on the CPU so that the extended recurrence stops decisively
    after 1 .. 3 iterations: cgiter() is that count and the result lies within the allowance of the extended iterate.  The default variant
    on the fresh handle; the others after reset_affine(), which restores the counter's and the warm start's first state."""
    seq = cases.prox_sequence(name)
    d = _make(pkg, *_operator(name, True), geom)
    bad = []
    try:
        classes = _classes(d, name, geom)
        for variant in (None,) + _variants(pkg, d):
            if variant is not None:
                d.set_cg_variant(variant)
                d.reset_affine()
            label = "default (%s)" % d.cg_variant_name() if variant is None else variant
            assert d.prox_count() == 1
            for call, (x, k, yk, allow) in enumerate(seq, 1):
                y = d.prox_affine(x)
                rat = cref.distance(y, yk) / allow
                _record(["prox_affine: " + cl for cl in classes], label.split()[0], rat)
                if d.cgiter() != k or not rat <= 1.0 or d.prox_count() != call + 1:
                    bad.append("%s %s call %d: CG iterations %d (want %d), error / allowance %.3g (allowance %.3g max|y|)%s" %
                               (name, label, call, d.cgiter(), k, rat, allow / float(np.max(np.abs(yk))),
                                ", alpha_0 %.17g (exactly -1 without rounding)" % _prox_alpha0(name, x, y) if call == 1 and k == 1 else ""))
    finally:
        d.close()
    assert not bad, "\n".join(bad)


# ---------------------------------------------------------------------------------------------- repartition


@pytest.mark.parametrize("name,geom", OPERATORS, ids=OP_IDS)
def test_repartitioned_operator_stays_within_allowance(pkg, name, geom):
    """After set_tuning(spmv_workgroups = 8) every iterate of the warm start stays within the allowance (not bitwise: the tau sums regroup).
    On a handle of its own: the partition stays with the handle."""
    cs = cases.case(name, "warm")
    d = _make(pkg, *_operator(name, True), geom)
    bad = []
    try:
        classes = ["repartitioned: " + cl for cl in _classes(d, name, geom)]
        d.set_tuning(spmv_workgroups=8)
        for variant in _variants(pkg, d):
            d.set_cg_variant(variant)
            for k in cs.ks:
                x, it = d.cg_kkt(cs.x0, cs.rhs, 1e-300, k)
                _judge(bad, classes, variant, "8 workgroups", cs, k, x, it, k)
    finally:
        d.close()
    assert not bad, "\n".join(bad)


# ---------------------------------------------------------------------------------------------- the unfused start

UNFUSED = [("sparse", None), ("tile-chunks", None), ("mid", "1")]
UNFUSED_IDS = ["sparse", "tile-chunks", "mid-win1"]
UNFUSED_VARIANTS = ("reference", "merged_update")


def _unfused_runs(cs):
    """(what, tolerance, cap, iterations wanted) of one case"""
    return [("iterates", 1e-300, k, k) for k in cs.ks] + [("stop rule", cref.decisive_tol(cs, k), 10000, k) for k in (2, 3)]


@pytest.mark.parametrize("name,geom", UNFUSED, ids=UNFUSED_IDS)
def test_unfused_start_behind_a_one_rank_communicator(pkg, name, geom):
    """After comm_init(1, 0, id) the reference recurrence starts with kkt_apply_full + cg_init + cg_init_finalize, and every sum of both
    variants goes through the local reduce kernel and the all-reduce (rr_from_reduced): the same iterates and counts, within the allowance."""
    d = _make(pkg, *_operator(name, True), geom)
    bad = []
    try:
        classes = ["one-rank communicator: " + cl for cl in _classes(d, name, geom)]
        d.comm_init(1, 0, pkg.HipHSDE.comm_unique_id())
        assert d.cg_variant_name() == "merged_update"                     # (the default of sharded handles)
        for variant in UNFUSED_VARIANTS:
            d.set_cg_variant(variant)
            assert d.cg_variant_name() == variant
            for cs in _cases(name)[:2]:
                for what, tol, cap, k in _unfused_runs(cs):
                    x, it = d.cg_kkt(cs.x0, cs.rhs, tol, cap)
                    _judge(bad, classes, variant, what, cs, k, x, it, k)
    finally:
        d.close()
    assert not bad, "\n".join(bad)


UNFUSED_CHILD = r"""
import os, sys
import numpy as np
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests", sys.argv[1] + "/oracle"]
import __graft_entry__ as ge
import cg_cases as cases
import cg_reference as cref
pkg = ge.load_package()
name, geom, out = sys.argv[2], sys.argv[3], sys.argv[4]
if geom != "-":
    os.environ["FOS_WINDOWS"] = geom
A, b, c = cases.scaled_operator(name)
d = pkg.HipHSDE(A, b, c, [("Free", A.shape[0])], [("Free", A.shape[1])])
res = {"win_panels": np.int64(d.operator_stats()["win_panels"])}
for variant in sys.argv[5:]:
    d.set_cg_variant(variant)
    for start in cases.TAMED:
        cs = cases.case(name, start)
        runs = [(1e-300, k) for k in cs.ks] + [(cref.decisive_tol(cs, k), 10000) for k in (2, 3)]
        for q, (tol, cap) in enumerate(runs):
            x, it = d.cg_kkt(cs.x0, cs.rhs, tol, cap)
            res["%s|%s|%d|x" % (variant, start, q)] = x
            res["%s|%s|%d|it" % (variant, start, q)] = np.int64(it)
d.close()
np.savez(out, **res)
print("RESULT written")
"""


@pytest.mark.parametrize("name,geom", UNFUSED, ids=UNFUSED_IDS)
def test_unfused_start_in_a_child_process(pkg, store, tmp_path, name, geom):
    """FOS_CG_FUSED_START=0 (read once per process -- hence one fresh child, which is what this test is about): the single-GPU reference
    recurrence starts with kkt_apply_full + cg_init + cg_init_finalize instead of the fused start kernel.  The child's iterates and counts
    are judged here like any other."""
    root = Path(__file__).resolve().parent.parent
    env = dict(os.environ, FOS_CG_FUSED_START="0")
    env.pop("FOS_WINDOWS", None)
    out = tmp_path / "unfused.npz"
    run = subprocess.run([sys.executable, "-c", UNFUSED_CHILD, str(root), name, geom or "-", str(out)] + list(UNFUSED_VARIANTS),
                         env=env, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "RESULT written" in run.stdout, run.stderr[-2000:]
    got = np.load(out)
    assert (int(got["win_panels"]) > 0) == (geom is not None)
    classes = ["FOS_CG_FUSED_START=0: " + cl for cl in _classes(store(name, geom), name, geom)]
    bad = []
    for variant in UNFUSED_VARIANTS:
        for cs in _cases(name)[:2]:
            start = cs.name.split("/")[1]
            for q, (what, tol, cap, k) in enumerate(_unfused_runs(cs)):
                _judge(bad, classes, variant, what, cs, k, got["%s|%s|%d|x" % (variant, start, q)], int(got["%s|%s|%d|it" % (variant, start, q)]), k)
    assert not bad, "\n".join(bad)


# ---------------------------------------------------------------------------------------------- coverage, report


def test_every_storage_class_is_hit(pkg, store):
    seen = dict(tiles_deferred=False, long=False, lds=False, run=False, win_panels=False, win_segments=False)
    for name, geom in OPERATORS:
        st = store(name, geom).operator_stats()
        seen["tiles_deferred"] |= st["tiles"] > 0 and st["deferred"] > 0
        seen["long"] |= st["long"] > 0
        seen["lds"] |= st["lds"] > 0
        seen["run"] |= st["run"] > 0
        seen["win_panels"] |= st["win_panels"] > 0
        seen["win_segments"] |= st["win_segments"] > 64
    print("storage classes reached:", seen)
    assert all(seen.values()), seen


def test_zz_report():
    """prints the worst error / allowance per storage class and variant gathered by the tests above (nothing to report when run alone)"""
    for cl in sorted(WORST):
        print("%-60s %s" % (cl, ", ".join("%s %.3g" % kv for kv in sorted(WORST[cl].items()))))
    for op in sorted(STATS):
        print("%-26s %s" % (op, {k: v for k, v in STATS[op].items() if v}))
    for cl, w in WORST.items():
        assert max(w.values()) <= 1.0, (cl, w)
