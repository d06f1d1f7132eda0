"""
Feasibility form, the vector sets of csrc/sets.hip (Feasibility.jl:2-6 takes any two ProximableFunctions), the parts that need no GPU: the constructors'
validation and the SeparableSum coverage rules, the three entries in every layer, and fos_host_set_project -- the host emulation of the kernels' threshold
search and formulas -- against the sort-based references of tests/set_cases.py.

Tolerance: 1e-13 max(|x|_inf, |parameter|) per element.  A fixed-order sum of L terms differs from an exact one by at most about (log2 L + 2) eps relative
to the sum of magnitudes (5e-15 at L = 2^20); the threshold and the scale factors inherit that bound, so 1e-13 leaves a factor 20.
"""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

from set_cases import INPUTS, KINDS, PASS_CAP, make_case

ROOT = Path(__file__).resolve().parent.parent
LENGTHS = [1, 2, 63, 64, 65, 1023, 1024, 1025, 16383, 16385, 100003]
FOS_EINVAL = -1


def host_project(pkg, case):
    lib = pkg.lib.load()
    S = case.device_set(pkg)
    length = len(case.x)
    if isinstance(S, pkg.IndBox):
        code, scal, vec = pkg.lib.SET_CODES["IndBox"], (S.lo, S.hi), None
    else:
        code, scal, vec = S._block(length)
    scal = np.array(scal, dtype=np.float64)
    y = np.full(length, np.nan)
    passes = ctypes.c_int32(-1)
    rc = lib.fos_host_set_project(code, length, pkg.lib.dptr(scal), None if vec is None else pkg.lib.dptr(vec), pkg.lib.dptr(case.x), pkg.lib.dptr(y),
                                  ctypes.byref(passes))
    assert rc == 0, lib.fos_last_error()
    return y, passes.value


@pytest.mark.parametrize("length", LENGTHS)
@pytest.mark.parametrize("kind", KINDS)
def test_host_emulation_matches_reference(pkg, kind, length):
    worst = 0.0
    for inp in INPUTS:
        case = make_case(kind, length, inp)
        y, passes = host_project(pkg, case)
        worst = max(worst, case.check(y, inp) / max(case.tol(), 1e-300))
        assert 0 <= passes <= PASS_CAP, (inp, passes)
        if kind not in ("IndSimplex", "IndBallL1"):
            assert passes == 0
    print("%s, len %d: worst error / tolerance = %.3g" % (kind, length, worst))


def test_host_emulation_rejects_bad_parameters(pkg):
    lib = pkg.lib.load()
    x, y = np.ones(4), np.zeros(4)
    codes = pkg.lib.SET_CODES

    def call(code, scal, vec, length=4):
        scal = np.array(scal, dtype=np.float64)
        return lib.fos_host_set_project(code, length, pkg.lib.dptr(scal), None if vec is None else pkg.lib.dptr(np.asarray(vec, dtype=np.float64)), pkg.lib.dptr(x),
                                        pkg.lib.dptr(y), None)
    assert call(codes["IndBallL2"], (1.0, 0.0), None) == 0                      # a NULL centre is the origin
    assert call(codes["IndBallL2"], (-1.0, 0.0), None) == FOS_EINVAL
    assert call(codes["IndBallL1"], (np.nan, 0.0), None) == FOS_EINVAL
    assert call(codes["IndSimplex"], (0.0, 0.0), None) == FOS_EINVAL
    assert call(codes["IndHalfspace"], (1.0, 0.0), np.zeros(4)) == FOS_EINVAL and "normal" in lib.fos_last_error().decode()
    assert call(codes["IndHalfspace"], (1.0, 0.0), None) == FOS_EINVAL
    assert call(codes["IndHyperslab"], (1.0, 0.5), np.ones(4)) == FOS_EINVAL
    assert call(codes["IndPoint"], (0.0, 0.0), [1.0, np.inf, 0.0, 0.0]) == FOS_EINVAL
    assert call(codes["IndBox"], (1.0, 0.0), None) == FOS_EINVAL
    assert call(8, (0.0, 0.0), None) == FOS_EINVAL and "unknown kind" in lib.fos_last_error().decode()
    assert call(codes["IndFree"], (0.0, 0.0), None, length=0) == FOS_EINVAL


def test_constructor_validation(pkg):
    bad = [lambda: pkg.IndBallL2(-1.0), lambda: pkg.IndBallL2(np.inf), lambda: pkg.IndBallL2(1.0, [1.0, np.nan]), lambda: pkg.IndBallL1(-0.5),
           lambda: pkg.IndBallL1(np.nan), lambda: pkg.IndSimplex(0.0), lambda: pkg.IndSimplex(-1.0), lambda: pkg.IndSimplex(np.inf),
           lambda: pkg.IndHalfspace(np.zeros(3), 1.0), lambda: pkg.IndHalfspace([1.0, 2.0], np.nan), lambda: pkg.IndHalfspace([1.0, np.inf], 0.0),
           lambda: pkg.IndHyperslab(1.0, [1.0, 2.0], 0.5), lambda: pkg.IndHyperslab(0.0, np.zeros(2), 0.5), lambda: pkg.IndHyperslab(-np.inf, [1.0], 0.5),
           lambda: pkg.IndPoint([np.nan]), lambda: pkg.IndPoint([])]
    for make in bad:
        with pytest.raises(ValueError):
            make()
    assert pkg.IndBallL2().r == 1.0 and pkg.IndBallL2().center is None and pkg.IndBallL1().r == 1.0 and pkg.IndSimplex().a == 1.0
    assert pkg.IndBallL2(0.0).r == 0.0                                          # r = 0 is a set (the centre alone)


def test_separable_sum_coverage_rules(pkg):
    S = pkg.SeparableSum([(pkg.IndFree(), 3), (pkg.IndBallL2(2.0, [1.0, 2.0]), 2), (pkg.IndBox(-1.0, np.inf), 4), (pkg.IndHalfspace([1.0, -1.0, 0.5], 0.25), 3),
                          (pkg.IndHyperslab(-1.0, [2.0], 1.5), 1), (pkg.IndSimplex(3.0), 5), (pkg.IndPoint([7.0, 8.0]), 2), (pkg.IndBallL1(0.5), 1)])
    assert S.n == 21
    kinds, lens, scal, vec = S.pack(21)
    c = pkg.lib.SET_CODES
    assert kinds.dtype == np.int32 and lens.dtype == np.int64
    assert list(kinds) == [c["IndFree"], c["IndBallL2"], c["IndBox"], c["IndHalfspace"], c["IndHyperslab"], c["IndSimplex"], c["IndPoint"], c["IndBallL1"]]
    assert list(lens) == [3, 2, 4, 3, 1, 5, 2, 1]
    assert list(scal) == [0, 0, 2.0, 0, -1.0, np.inf, 0.25, 0, -1.0, 1.5, 3.0, 0, 0, 0, 0.5, 0]
    expect = np.zeros(21)                                                       # each vector at its block's own indices
    expect[3:5], expect[9:12], expect[12], expect[18:20] = [1.0, 2.0], [1.0, -1.0, 0.5], 2.0, [7.0, 8.0]
    assert np.array_equal(vec, expect)
    with pytest.raises(ValueError):
        S.pack(22)                                                              # the blocks must cover 1..n
    for blocks in ([], [(pkg.IndFree(), 0)], [(pkg.IndBallL2(1.0, [1.0, 2.0]), 3)], [(pkg.IndHalfspace([1.0], 0.0), 2)], [(pkg.IndPoint([1.0, 2.0]), 1)],
                   [(pkg.IndBox([0.0, 0.0], 1.0), 2)], [(pkg.IndBox(1.0, 0.0), 2)], [(pkg.ConeProduct([("SOC", 3)]), 3)], [(object(), 2)]):
        with pytest.raises(ValueError):
            pkg.SeparableSum(blocks)
    # a handle checks the sizes BEFORE any device call: these fail the same way with or without a GPU
    for S1 in (pkg.SeparableSum([(pkg.IndFree(), 3)]), pkg.IndBallL2(1.0, np.zeros(3)), pkg.IndPoint(np.zeros(5))):
        with pytest.raises(ValueError):
            pkg.HipFeasibility(pkg.Feasibility(S1, pkg.IndBox(0.0, 1.0), 4))


def test_entries_exist_in_every_layer(pkg):
    lib = pkg.lib.load(check_symbols=True)
    hdr = (ROOT / "include" / "foship.h").read_text()
    jl = (ROOT / "firstordersolvers.jl_amd" / "julia" / "FOSHip.jl").read_text()
    for name in ("fos_feas_set_blocks", "fos_feas_set_stats", "fos_host_set_project"):
        assert getattr(lib, name) is not None
        assert name in pkg.lib.PROTOTYPES and name in pkg.lib.header_symbols()
        assert (":%s, libfoship" % name) in jl
    for name, code in pkg.lib.SET_CODES.items():
        macro = {"IndFree": "FREE", "IndBallL2": "BALL_L2", "IndBallL1": "BALL_L1", "IndSimplex": "SIMPLEX", "IndHalfspace": "HALFSPACE",
                 "IndHyperslab": "HYPERSLAB", "IndPoint": "POINT", "IndBox": "BOX"}[name]
        assert re.search(r"#define\s+FOS_SET_%s\s+%d\b" % (macro, code), hdr), name
        assert re.search(r"const\s+FOS_SET_%s\s*=\s*Int32\(%d\)" % (macro, code), jl), name
    assert re.search(r"#define\s+FOS_ABI_VERSION\s+1\b", hdr)
    P = pkg.lib.PROTOTYPES
    i32p, i64p, dp = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double)
    assert P["fos_feas_set_blocks"][1] == [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, i32p, i64p, dp, dp]
    assert P["fos_feas_set_stats"][1] == [ctypes.c_void_p, ctypes.c_int32, dp]
    assert P["fos_host_set_project"][1] == [ctypes.c_int32, ctypes.c_int64, dp, dp, dp, dp, i32p]
    m = re.search(r"ccall\(\(:fos_feas_set_blocks, libfoship\), Cint,\s*\(([^)]*)\)", jl)
    assert m and [t.strip() for t in m.group(1).split(",")] == ["Ptr{Cvoid}", "Int32", "Int64", "Ptr{Int32}", "Ptr{Int64}", "Ptr{Cdouble}", "Ptr{Cdouble}"]
    for cls in ("IndBallL2", "IndBallL1", "IndSimplex", "IndHalfspace", "IndHyperslab", "IndPoint", "IndFree", "SeparableSum"):
        assert hasattr(pkg, cls)
