"""
Feasibility form, proximable functions that are not indicators (Feasibility.jl:2-6 takes any two ProximableFunctions) -- NormL1, SqrNormL2, ElasticNet, Linear,
NormL2, HuberLoss, NormLinf as block kinds of csrc/sets.hip, LeastSquares on the factored dense form of csrc/affine_dense.hip -- the parts that need no GPU:
fos_host_set_project with the new codes and fos_host_least_squares against the references of tests/prox_fn_cases.py, an oracle-free certificate, the
constructors' validation, SeparableSum.pack with mixed blocks, and every new entry in every layer.

Tolerance of a separable prox: 1e-13 max(|x|_inf, |parameter|) per element, the bound tests/test_feas_sets_cpu.py derives for fixed-order sums of these lengths;
the new formulas add one division or one subtraction to sums of the same kind.
"""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

from affine_factored_cases import SHAPES, TOL, instance
from prox_fn_cases import INPUTS, KINDS, PASS_CAP, REFS, RefLeastSquares, make_case

ROOT = Path(__file__).resolve().parent.parent
LENGTHS = [1, 2, 63, 64, 65, 1023, 1024, 1025, 16383, 16385, 100003]
FOS_EINVAL = -1
MACROS = {"NormL1": "NORM_L1", "SqrNormL2": "SQR_NORM_L2", "ElasticNet": "ELASTIC_NET", "Linear": "LINEAR", "NormL2": "NORM_L2", "HuberLoss": "HUBER",
          "NormLinf": "NORM_LINF"}


def host_prox(pkg, S, x):
    lib = pkg.lib.load()
    code, scal, vec = S._block(len(x))
    scal = np.array(scal, dtype=np.float64)
    y = np.full(len(x), np.nan)
    passes = ctypes.c_int32(-1)
    rc = lib.fos_host_set_project(code, len(x), pkg.lib.dptr(scal), None if vec is None else pkg.lib.dptr(vec), pkg.lib.dptr(x), pkg.lib.dptr(y), ctypes.byref(passes))
    assert rc == 0, lib.fos_last_error()
    return y, passes.value


@pytest.mark.parametrize("length", LENGTHS)
@pytest.mark.parametrize("kind", KINDS)
def test_host_emulation_matches_reference(pkg, kind, length):
    worst = 0.0
    for inp in INPUTS:
        case = make_case(kind, length, inp)
        y, passes = host_prox(pkg, case.device_set(pkg), case.x)
        worst = max(worst, case.check(y, inp) / max(case.tol(), 1e-300))           # (y = x bit for bit and y = 0 exactly are part of the check)
        assert 0 <= passes <= PASS_CAP, (inp, passes)
        if kind != "NormLinf":
            assert passes == 0
    print("%s, len %d: worst error / tolerance = %.3g" % (kind, length, worst))


@pytest.mark.parametrize("n", [700, 5000, 40000])
@pytest.mark.parametrize("kind", KINDS)
def test_certificates(pkg, kind, n):
    """Without any reference prox: y = prox_f(x) iff x - y is a subgradient of f at y, that is f(z) >= f(y) + <x - y, z - y> for every z.  20 random z;
    tol = 1e-12 |x| |z|, the bar and the argument of test_gpu_feas_sets.test_certificates: y carries at most 1e-13 |x|_inf per element, |dy|_2 <= 1e-13 sqrt(n)
    |x|_inf ~ 4.5e-13 |x|_2, and the right-hand side moves by at most |dy| (|x - y| + |z - y|) plus the Lipschitz change of f(y)."""
    case = make_case(kind, n, "gauss", seed=1)
    x, f = case.x, case.ref.value
    y, _ = host_prox(pkg, case.device_set(pkg), x)
    rng = np.random.default_rng(n)
    worst = -np.inf
    for k in range(20):
        z = (0.1 + k) * rng.standard_normal(n)
        viol = (f(y) + float((x - y) @ (z - y)) - f(z)) / (np.linalg.norm(x) * np.linalg.norm(z))
        worst = max(worst, viol)
        assert viol <= 1e-12, (k, viol)
    print("%s, n = %d: max (f(y) + <x - y, z - y> - f(z)) / (|x| |z|) = %.3g" % (kind, n, worst))


def host_least_squares(pkg, A, b, lam, x):
    lib = pkg.lib.load()
    y = np.full(A.shape[1], np.nan)
    rc = lib.fos_host_least_squares(A.shape[0], A.shape[1], pkg.lib.dptr(np.ascontiguousarray(A)), pkg.lib.dptr(b), lam, pkg.lib.dptr(x), pkg.lib.dptr(y))
    return rc, y


@pytest.mark.parametrize("lam", [1e-3, 1.0, 1e3])
@pytest.mark.parametrize("family,m,n", [s for s in SHAPES if s[2] <= 1000])
def test_host_least_squares_matches_the_dense_solve(pkg, family, m, n, lam):
    """the bar of the factored IndAffine's projection (1e-12 max(1, |x|_inf)): the shift only raises the smallest eigenvalue of the matrix that is inverted"""
    A, b = instance(family, m, n)
    x = np.random.default_rng(1).standard_normal(n)
    rc, y = host_least_squares(pkg, A, b, lam, x)
    assert rc == 0, pkg.lib.load().fos_last_error()
    err = np.abs(y - RefLeastSquares(A, b, lam).project(x)).max()
    print("%s (%d, %d) lam %g: |y - dense solve| = %.2e" % (family, m, n, lam, err))
    assert err <= TOL * max(1.0, np.abs(x).max())


def test_host_least_squares_edge_cases(pkg):
    A, b = instance("gauss", 10, 30)
    x = np.random.default_rng(2).standard_normal(30)
    D, bd = A.copy(), b.copy()
    D[7], bd[7] = D[2], b[2] + 1.0                                               # rank deficient, inconsistent: legal here
    Z = A.copy(); Z[4] = 0.0                                                     # a zero row: legal here
    for M, bb in ((D, bd), (Z, b)):
        for lam in (1e-3, 1.0, 1e3):
            rc, y = host_least_squares(pkg, M, bb, lam, x)
            assert rc == 0 and np.abs(y - RefLeastSquares(M, bb, lam).project(x)).max() <= TOL * max(1.0, np.abs(x).max()), lam
    lib = pkg.lib.load()
    assert host_least_squares(pkg, A.T.copy(), np.ones(30), 1.0, np.ones(10))[0] == FOS_EINVAL and "fos_feas_set_callback" in lib.fos_last_error().decode()
    for lam in (0.0, -1.0, np.nan, np.inf):
        assert host_least_squares(pkg, A, b, lam, x)[0] == FOS_EINVAL
    # lambda = 0 is IndAffine: the factored form's own host emulation is unchanged by the shift's code
    y0 = np.empty(30)
    assert lib.fos_host_affine_factored(10, 30, pkg.lib.dptr(A), pkg.lib.dptr(b), 0, pkg.lib.dptr(x), pkg.lib.dptr(y0)) == 0
    assert np.abs(A @ y0 - b).max() <= 1e-12


def test_host_emulation_rejects_bad_parameters(pkg):
    lib = pkg.lib.load()
    x, y = np.ones(4), np.zeros(4)
    c = pkg.lib.FN_CODES

    def call(code, scal, vec):
        scal = np.array(scal, dtype=np.float64)
        return lib.fos_host_set_project(code, 4, pkg.lib.dptr(scal), None if vec is None else pkg.lib.dptr(np.asarray(vec, dtype=np.float64)), pkg.lib.dptr(x),
                                        pkg.lib.dptr(y), None)
    for kind in ("NormL1", "SqrNormL2", "NormL2", "NormLinf"):
        assert call(c[kind], (0.0, 0.0), None) == 0
        for bad in (-1.0, np.nan, np.inf):
            assert call(c[kind], (bad, 0.0), None) == FOS_EINVAL and ("block 1 (%s)" % kind) in lib.fos_last_error().decode(), (kind, bad)
    for bad in ((-1.0, 1.0), (1.0, -1.0), (np.nan, 1.0), (1.0, np.inf)):
        assert call(c["ElasticNet"], bad, None) == FOS_EINVAL and "block 1 (ElasticNet)" in lib.fos_last_error().decode()
    for bad in ((0.0, 1.0), (-1.0, 1.0), (1.0, -1.0), (np.inf, 1.0), (1.0, np.nan)):
        assert call(c["HuberLoss"], bad, None) == FOS_EINVAL and "block 1 (HuberLoss)" in lib.fos_last_error().decode()
    assert call(c["HuberLoss"], (1.0, 0.0), None) == 0
    assert call(c["Linear"], (0.0, 0.0), None) == FOS_EINVAL and "block 1 (Linear)" in lib.fos_last_error().decode()
    assert call(c["Linear"], (0.0, 0.0), [1.0, np.inf, 0.0, 0.0]) == FOS_EINVAL
    assert call(c["Linear"], (0.0, 0.0), np.ones(4)) == 0 and np.array_equal(y, np.zeros(4))
    for code in (8, 31, 39):                                                     # between the sets and the functions, and past them
        assert call(code, (0.0, 0.0), None) == FOS_EINVAL and "unknown kind" in lib.fos_last_error().decode(), code


def test_constructor_validation(pkg):
    A = np.ones((2, 3))
    bad = [lambda: pkg.NormL1(-1.0), lambda: pkg.NormL1(np.nan), lambda: pkg.SqrNormL2(-0.1), lambda: pkg.SqrNormL2(np.inf), lambda: pkg.ElasticNet(-1.0, 1.0),
           lambda: pkg.ElasticNet(1.0, -1.0), lambda: pkg.ElasticNet(1.0, np.nan), lambda: pkg.Linear([1.0, np.nan]), lambda: pkg.Linear([]), lambda: pkg.NormL2(-1.0),
           lambda: pkg.NormL2(np.inf), lambda: pkg.HuberLoss(0.0, 1.0), lambda: pkg.HuberLoss(-1.0, 1.0), lambda: pkg.HuberLoss(1.0, -1.0),
           lambda: pkg.HuberLoss(np.inf, 1.0), lambda: pkg.NormLinf(-1.0), lambda: pkg.NormLinf(np.nan),
           lambda: pkg.LeastSquares(A, np.ones(2), 0.0), lambda: pkg.LeastSquares(A, np.ones(2), -1.0), lambda: pkg.LeastSquares(A, np.ones(2), np.inf),
           lambda: pkg.LeastSquares(A, np.ones(3)), lambda: pkg.LeastSquares(np.ones(3), np.ones(3)), lambda: pkg.LeastSquares(A, np.ones(2), factor="qr"),
           lambda: pkg.LeastSquares(np.array([[1.0, np.nan, 0.0]]), np.ones(1))]
    for make in bad:
        with pytest.raises(ValueError):
            make()
    assert pkg.NormL1().lam == 1.0 and pkg.NormL1(0.0).lam == 0.0 and pkg.HuberLoss(2.0, 0.0).mu == 0.0 and pkg.ElasticNet(0.0, 0.0).scal == (0.0, 0.0)
    ls = pkg.LeastSquares(A, np.ones(2))
    assert ls.lam == 1.0 and ls.A.flags["C_CONTIGUOUS"] and ls.A.dtype == np.float64
    # a handle checks the sizes BEFORE any device call: these fail the same way with or without a GPU
    for S1 in (pkg.Linear(np.zeros(3)), pkg.SeparableSum([(pkg.NormL1(1.0), 3)])):
        with pytest.raises(ValueError):
            pkg.HipFeasibility(pkg.Feasibility(S1, pkg.IndBox(0.0, 1.0), 4))


def test_separable_sum_packs_mixed_set_and_function_blocks(pkg):
    S = pkg.SeparableSum([(pkg.IndFree(), 3), (pkg.NormL1(0.25), 2), (pkg.IndBox(-1.0, np.inf), 4), (pkg.Linear([1.0, -1.0, 0.5]), 3), (pkg.HuberLoss(2.0, 0.5), 1),
                          (pkg.IndSimplex(3.0), 5), (pkg.ElasticNet(0.1, 0.2), 2), (pkg.NormLinf(0.5), 1), (pkg.SqrNormL2(4.0), 2), (pkg.NormL2(1.5), 2),
                          (pkg.IndBallL2(2.0, [1.0, 2.0]), 2)])
    assert S.n == 27
    kinds, lens, scal, vec = S.pack(27)
    c, f = pkg.lib.SET_CODES, pkg.lib.FN_CODES
    assert kinds.dtype == np.int32 and lens.dtype == np.int64
    assert list(kinds) == [c["IndFree"], f["NormL1"], c["IndBox"], f["Linear"], f["HuberLoss"], c["IndSimplex"], f["ElasticNet"], f["NormLinf"], f["SqrNormL2"],
                           f["NormL2"], c["IndBallL2"]]
    assert list(lens) == [3, 2, 4, 3, 1, 5, 2, 1, 2, 2, 2]
    assert list(scal) == [0, 0, 0.25, 0, -1.0, np.inf, 0, 0, 2.0, 0.5, 3.0, 0, 0.1, 0.2, 0.5, 0, 4.0, 0, 1.5, 0, 2.0, 0]
    expect = np.zeros(27)
    expect[9:12], expect[25:27] = [1.0, -1.0, 0.5], [1.0, 2.0]
    assert np.array_equal(vec, expect)
    with pytest.raises(ValueError):
        pkg.SeparableSum([(pkg.Linear([1.0, 2.0]), 3)])                          # the vector's length against the block's
    with pytest.raises(ValueError):
        pkg.SeparableSum([(pkg.LeastSquares(np.ones((1, 2)), np.ones(1)), 2)])   # not separable: S1 or S2 as a whole


def test_codes_and_entries_exist_in_every_layer(pkg):
    lib = pkg.lib.load(check_symbols=True)
    hdr = (ROOT / "include" / "foship.h").read_text()
    jl = (ROOT / "firstordersolvers.jl_amd" / "julia" / "FOSHip.jl").read_text()
    assert pkg.lib.FN_CODES == {k: 32 + i for i, k in enumerate(KINDS)} and set(REFS) == set(KINDS)
    assert pkg.lib.SET_CODES == {"IndFree": 0, "IndBallL2": 1, "IndBallL1": 2, "IndSimplex": 3, "IndHalfspace": 4, "IndHyperslab": 5, "IndPoint": 6, "IndBox": 7}
    for name, code in pkg.lib.FN_CODES.items():
        assert re.search(r"#define\s+FOS_FN_%s\s+%d\b" % (MACROS[name], code), hdr), name
        assert re.search(r"const\s+FOS_FN_%s\s*=\s*Int32\(%d\)" % (MACROS[name], code), jl), name
        assert issubclass(getattr(pkg, name), pkg.IndFree.__mro__[1])             # a _VectorSet: SeparableSum takes it
    assert re.search(r"#define\s+FOS_ABI_VERSION\s+1\b", hdr) and lib.fos_abi_version() == 1
    P = pkg.lib.PROTOTYPES
    dp = ctypes.POINTER(ctypes.c_double)
    for name in ("fos_feas_set_least_squares", "fos_host_least_squares"):
        assert getattr(lib, name) is not None
        assert name in P and name in pkg.lib.header_symbols()
        assert (":%s, libfoship" % name) in jl
    assert P["fos_feas_set_least_squares"][1] == [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, dp, dp, ctypes.c_double, ctypes.c_int32]
    assert P["fos_host_least_squares"][1] == [ctypes.c_int64, ctypes.c_int64, dp, dp, ctypes.c_double, dp, dp]
    m = re.search(r"ccall\(\(:fos_feas_set_least_squares, libfoship\), Cint,\s*\(([^)]*)\)", jl)
    assert m and [t.strip() for t in m.group(1).split(",")] == ["Ptr{Cvoid}", "Int32", "Int64", "Ptr{Cdouble}", "Ptr{Cdouble}", "Cdouble", "Int32"]
    assert hasattr(pkg, "LeastSquares")
