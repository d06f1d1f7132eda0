"""CPU: the dense blocks of a SeparableSum (csrc/dense_blocks.hip) without a device -- fos_host_dense_block runs the library's own set-up (long double, rounded
once) and the kernels' chain y_r = d_r, then fma(G(r, j), x_j, .) for j ascending; the Python mirror packs the arguments of fos_feas_set_blocks2.

The bars are the project's own (dense_block_cases): nspace_cases.bar for Quadratic and LeastSquares against RefQuadratic / RefLeastSquares,
affine_factored_cases.TOL max(1, |x|_inf) for IndAffine against a projection refined in np.longdouble."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

import affine_factored_cases as ac
import dense_block_cases as dc
from dense_block_cases import FOS_EINVAL, KINDS, P

ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.parametrize("p", P)
@pytest.mark.parametrize("kind", KINDS)
def test_host_emulation_meets_the_bar(pkg, kind, p):
    x = dc.input_of(p)
    for tag, blk in dc.blocks_of(kind, p):
        rc, y, G, d = dc.host_block(pkg, blk, x)
        assert rc == 0, dc.last_error(pkg)
        assert np.array_equal(G, G.T), (kind, p, tag, "G is not symmetric bit for bit")
        ref = blk.ref.project(x)
        err, bar = float(np.abs(y - ref).max()), blk.bar(x, ref)
        yL, bound = dc.kernel_bound(G, d, x)
        kerr = float((np.abs(y - yL) / np.maximum(bound, 1e-300)).max().astype(np.float64))
        if kind == "IndAffine":
            print("%s p=%d %s: |y - ref| = %.2e (bar %.2e), range defect %.2e, |A y - b| = %.2e, kernel error / bound %.2f" %
                  (kind, p, tag, err, bar, ac.range_defect(blk.M, x, y), np.abs(blk.M @ y - blk.v).max(), kerr))
        else:
            print("%s p=%d %s: |y - ref| = %.2e (bar %.2e), kernel error / bound %.2f" % (kind, p, tag, err, bar, kerr))
        assert err <= bar, (kind, p, tag, err, bar)
        assert np.all(np.abs(y - yL) <= bound), (kind, p, tag, kerr)


def test_exact_cases(pkg):
    c = pkg.lib.BLK_CODES
    for p in (1, 5, 64, 130):
        x = dc.input_of(p, 1)
        rc, y, G, d = dc.host(pkg, c["Quadratic"], np.zeros((p, p)), np.zeros(p), 0.0, x)
        assert rc == 0 and np.array_equal(G, np.eye(p)) and not d.any()
        assert y.tobytes() == x.tobytes(), p                                      # Q = 0, q = 0: y = x, the same bits
        rc, y0, _, _ = dc.host(pkg, c["Quadratic"], np.zeros((p, p)), None, 0.0, x)      # (no vector: zeros)
        assert rc == 0 and y0.tobytes() == x.tobytes()
        q = dc.input_of(p, 2)
        rc, y, _, d = dc.host(pkg, c["Quadratic"], np.zeros((p, p)), q, 0.0, x)
        assert rc == 0 and np.array_equal(d, -q) and np.array_equal(y, x - q), p  # Q = 0: y = x - q, one rounding
        blk = dc.block("IndAffine", p, m=p)                                       # m = p: the unique solution, whatever x
        rc, y, G, _ = dc.host_block(pkg, blk, x)
        sol = blk.ref.project(x)
        assert rc == 0 and np.abs(y - sol).max() <= ac.TOL * max(1.0, np.abs(x).max()), p
        assert np.abs(G).max() <= 1e-13                                           # I - A^+ A = 0
    # p = 1, by hand
    rc, y, G, d = dc.host(pkg, c["Quadratic"], np.array([[3.0]]), np.array([2.0]), 0.0, np.array([6.0]))
    assert rc == 0 and G[0, 0] == 0.25 and d[0] == -0.5 and y[0] == 1.0           # (6 - 2) / (1 + 3)
    rc, y, G, d = dc.host(pkg, c["LeastSquares"], np.array([[2.0]]), np.array([1.0]), 0.75, np.array([2.0]))
    assert rc == 0 and G[0, 0] == 0.25 and y[0] == (2.0 + 0.75 * 2.0) / 4.0       # (x + lam a b) / (1 + lam a^2)
    rc, y, G, d = dc.host(pkg, c["IndAffine"], np.array([[4.0]]), np.array([2.0]), 0.0, np.array([9.0]))
    assert rc == 0 and G[0, 0] == 0.0 and y[0] == 0.5
    # only the lower triangle of Q is read
    blk = dc.block("Quadratic", 9)
    up = blk.M.copy()
    up[np.triu_indices(9, 1)] = np.nan
    assert np.array_equal(dc.host(pkg, c["Quadratic"], up, blk.v, 0.0, dc.input_of(9))[1], dc.host_block(pkg, blk, dc.input_of(9))[1])


def test_refusals(pkg):
    c = pkg.lib.BLK_CODES
    p = 6
    x = dc.input_of(p)
    q, ls, af = dc.block("Quadratic", p), dc.block("LeastSquares", p), dc.block("IndAffine", p, m=3)

    def refused(what, code, M, v, lam, needle, **shape):
        rc = dc.host(pkg, code, M, v, lam, x if "p" not in shape else np.zeros(shape["p"]), **shape)[0]
        msg = dc.last_error(pkg)
        assert rc == FOS_EINVAL and "block 1" in msg and needle in msg, (what, rc, msg)

    for bad in (np.nan, np.inf):
        M = q.M.copy(); M[4, 2] = bad
        refused("Quadratic entry", c["Quadratic"], M, q.v, 0.0, "not finite")
        M = af.M.copy(); M[1, 5] = bad
        refused("IndAffine entry", c["IndAffine"], M, af.v, 0.0, "not finite")
        M = ls.M.copy(); M[0, 0] = bad
        refused("LeastSquares entry", c["LeastSquares"], M, ls.v, 1.0, "not finite")
        v = q.v.copy(); v[3] = bad
        refused("Quadratic vector", c["Quadratic"], q.M, v, 0.0, "not finite")
        v = af.v.copy(); v[2] = bad
        refused("IndAffine vector", c["IndAffine"], af.M, v, 0.0, "not finite")
        refused("lambda", c["LeastSquares"], ls.M, ls.v, bad, "lambda")
    for lam in (0.0, -1.0):
        refused("lambda", c["LeastSquares"], ls.M, ls.v, lam, "lambda")
    M = q.M.copy(); M[3, 3] = -1.0 - 2.0 * abs(M).max() * p                      # 1 + Q[3, 3] < 0 whatever the earlier columns take away
    refused("pivot", c["Quadratic"], M, q.v, 0.0, "column")
    assert re.search(r"column \d+ of I \+ Q", dc.last_error(pkg))
    M = np.zeros((p, p)); M[0, 0] = -2.0
    refused("pivot 1", c["Quadratic"], M, None, 0.0, "column 1 of I + Q")
    D = af.M.copy(); D[2] = 2.0 * D[0]                                           # a dependent row
    refused("rank", c["IndAffine"], D, af.v, 0.0, "A needs full row rank")
    Z = af.M.copy(); Z[1] = 0.0
    refused("zero row", c["IndAffine"], Z, af.v, 0.0, "A needs full row rank")
    refused("m > p", c["IndAffine"], np.random.default_rng(0).standard_normal((p + 1, p)), np.zeros(p + 1), 0.0, "m <= p")
    refused("order", c["Quadratic"], np.zeros((1025, 1025)), None, 0.0, "1024")
    assert "whole-vector" in dc.last_error(pkg)
    refused("Q not square", c["Quadratic"], q.M, q.v, 0.0, "Quadratic", m=p - 1, p=p)
    rc = pkg.lib.load().fos_host_dense_block(7, p, p, pkg.lib.dptr(q.M), None, 0.0, pkg.lib.dptr(x), pkg.lib.dptr(np.zeros(p)), None, None)
    assert rc == FOS_EINVAL                                                       # a vector kind is no dense block
    # rank-deficient A is accepted by LeastSquares, a wide and a tall A alike
    for m in (1, 3, 40):
        A = np.ones((m, p))
        rc, y, G, _ = dc.host(pkg, c["LeastSquares"], A, np.ones(m), 2.0, x)
        assert rc == 0 and np.array_equal(G, G.T)
    # the dense kinds stay unknown to the entries without matrices
    for code in (48, 49, 50):
        y = np.zeros(p)
        rc = pkg.lib.load().fos_host_set_project(code, p, pkg.lib.dptr(np.zeros(2)), None, pkg.lib.dptr(x), pkg.lib.dptr(y), None)
        assert rc == FOS_EINVAL and "unknown kind" in dc.last_error(pkg), code


def test_a_second_build_gives_the_same_bits(pkg):
    """from order 128 on one matrix is built by several threads, each entry by one of them in the serial order of additions: y, G and d repeat bit for bit"""
    blk = dc.block("LeastSquares", 130)
    a, b = dc.host_block(pkg, blk, dc.input_of(130)), dc.host_block(pkg, blk, dc.input_of(130))
    assert a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes() and a[3].tobytes() == b[3].tobytes()


def _three(pkg, p=5):
    q, af, ls = dc.block("Quadratic", p), dc.block("IndAffine", p, m=2), dc.block("LeastSquares", p, "gauss", 0.5)
    return q, af, ls


def test_python_constructor_pack2_and_sharing(pkg):
    q, af, ls = _three(pkg)
    S = pkg.SeparableSum([(pkg.IndFree(), 3), (q.device_set(pkg), 5), (pkg.NormL1(0.1), 4), (af.device_set(pkg), 5), (ls.device_set(pkg), 5),
                          (pkg.LeastSquares(ls.M, ls.v, 0.5, form="normal"), 5), (pkg.IndAffine(af.M, af.v, form="factored"), 5), (pkg.IndBox(0.0, 1.0), 2)], dense=True)
    assert S.dense and S.n == 34
    kinds, lens, scal, vec, mats, block_mat, block_vec = S.pack2(34)
    assert list(kinds) == [0, 48, 32, 49, 50, 50, 49, 7] and list(lens) == [3, 5, 4, 5, 5, 5, 5, 2]
    assert list(block_mat) == [-1, 0, -1, 1, 2, 2, 1, -1]                         # the same ndarray, kind and lambda: one matrix
    assert [M.shape for M in mats] == [(5, 5), (2, 5), (8, 5)] and mats[0] is q.M and mats[1] is af.M and mats[2] is ls.M
    assert scal[2 * 4] == 0.5 and scal[2 * 2] == 0.1 and scal[2 * 1] == 0.0 and scal[15] == 1.0
    assert [v is None for v in block_vec] == [True, False, True, False, False, False, False, True]
    assert np.array_equal(block_vec[1], q.v) and np.array_equal(block_vec[3], af.v) and np.array_equal(block_vec[4], ls.v) and not vec.any()
    with pytest.raises(ValueError, match="pack2"):
        S.pack(34)
    with pytest.raises(ValueError):
        S.pack2(35)
    # 50 blocks on one Q with 50 different q: one matrix; another lambda on one A: another matrix
    qs = [np.full(5, float(k)) for k in range(50)]
    S = pkg.SeparableSum([(pkg.Quadratic(q.M, v), 5) for v in qs] + [(pkg.LeastSquares(ls.M, ls.v, 0.5), 5), (pkg.LeastSquares(ls.M, ls.v, 0.25), 5)], dense=True)
    _, _, _, _, mats, block_mat, block_vec = S.pack2(260)
    assert len(mats) == 3 and list(block_mat) == [0] * 50 + [1, 2] and all(np.array_equal(block_vec[k], qs[k]) for k in range(50))
    S = pkg.SeparableSum([(pkg.Quadratic(q.M.copy(), q.v), 5), (pkg.Quadratic(q.M.copy(), q.v), 5)], dense=True)      # equal values, other arrays: two matrices
    assert len(S.pack2(10)[4]) == 2
    # a sum without dense blocks packs as before
    S = pkg.SeparableSum([(pkg.IndFree(), 3), (pkg.NormL1(0.1), 4)])
    assert not S.dense and len(S.pack(7)) == 4 and len(S.pack2(7)) == 7 and list(S.pack2(7)[5]) == [-1, -1] and S.pack2(7)[4] == []


def test_python_refusals(pkg):
    blk = dc.block("Quadratic", 5)
    for S in (blk.device_set(pkg), dc.block("LeastSquares", 5).device_set(pkg), dc.block("IndAffine", 5, m=2).device_set(pkg)):
        with pytest.raises(ValueError, match="dense=True"):                         # opt-in: without the keyword the three types are refused as before
            pkg.SeparableSum([(S, 5)])
    import scipy.sparse as sp
    q, af, ls = _three(pkg)
    cases = [
        ("Quadratic(form='cg')", pkg.Quadratic(q.M, q.v, form="cg"), 5),
        ("LeastSquares(form='cg')", pkg.LeastSquares(ls.M, ls.v, 0.5, form="cg"), 5),
        ("LeastSquares(form='sparse_factored')", pkg.LeastSquares(sp.csc_matrix(ls.M[:3]), ls.v[:3], 0.5, form="sparse_factored"), 5),
        ("LeastSquares(form='normal'), sparse", pkg.LeastSquares(sp.csc_matrix(ls.M), ls.v, 0.5, form="normal"), 5),
        ("IndAffine(form='sparse_factored')", pkg.IndAffine(af.M, af.v, form="sparse_factored"), 5),
        ("IndAffine, sparse", pkg.IndAffine(sp.csc_matrix(af.M), af.v), 5),
        ("Quadratic, length", q.device_set(pkg), 6),
        ("LeastSquares, length", ls.device_set(pkg), 4),
        ("IndAffine, length", af.device_set(pkg), 7),
        ("IndAffine, m > p", pkg.IndAffine(np.ones((3, 2)), np.ones(3)), 2),
        ("Quadratic, p > 1024", pkg.Quadratic(np.zeros((1025, 1025)), np.zeros(1025)), 1025),
    ]
    for what, S, length in cases:
        with pytest.raises(ValueError, match="block 2"):
            pkg.SeparableSum([(pkg.IndFree(), 1), (S, length)], dense=True)
        assert what


def test_entries_exist_in_every_layer(pkg):
    lib = pkg.lib.load(check_symbols=True)
    hdr = (ROOT / "include" / "foship.h").read_text()
    jl = (ROOT / "firstordersolvers.jl_amd" / "julia" / "FOSHip.jl").read_text()
    assert pkg.lib.BLK_CODES == {"Quadratic": 48, "IndAffine": 49, "LeastSquares": 50}
    for macro, code in (("FOS_FN_BLK_QUADRATIC", 48), ("FOS_SET_BLK_AFFINE", 49), ("FOS_FN_BLK_LEAST_SQUARES", 50)):
        assert re.search(r"#define\s+%s\s+%d\b" % (macro, code), hdr), macro
        assert re.search(r"const\s+%s\s*=\s*Int32\(%d\)" % (macro, code), jl), macro
    assert re.search(r"#define\s+FOS_ABI_VERSION\s+1\b", hdr) and lib.fos_abi_version() == 1
    P_ = pkg.lib.PROTOTYPES
    vp, i32, i64, dbl = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_double
    i32p, i64p, dp = ctypes.POINTER(i32), ctypes.POINTER(i64), ctypes.POINTER(dbl)
    dpp = ctypes.POINTER(dp)
    for name in ("fos_feas_set_blocks2", "fos_feas_dense_block_stats", "fos_feas_dense_block_get", "fos_host_dense_block"):
        assert getattr(lib, name) is not None and name in P_ and name in pkg.lib.header_symbols()
    assert P_["fos_feas_set_blocks2"][1] == [vp, i32, i64, i32p, i64p, dp, dp, i64, i64p, i64p, dpp, i64p, dpp]
    assert P_["fos_feas_dense_block_stats"][1] == [vp, i32, dp] and P_["fos_feas_dense_block_get"][1] == [vp, i32, i64, dp, dp]
    assert P_["fos_host_dense_block"][1] == [i32, i64, i64, dp, dp, dbl, dp, dp, dp, dp]
    # the Julia wrapper of the entry with two arrays of pointers: bound by address, with the header's thirteen argument types
    m = re.search(r"dlsym\(Libdl\.dlopen\(libfoship\), :fos_feas_set_blocks2\).*?ccall\(fn, Cint,\s*\(([^)]*)\)", jl, flags=re.S)
    assert m and [t.strip() for t in m.group(1).split(",")] == ["Ptr{Cvoid}", "Int32", "Int64", "Ptr{Int32}", "Ptr{Int64}", "Ptr{Cdouble}", "Ptr{Cdouble}", "Int64",
                                                                "Ptr{Int64}", "Ptr{Int64}", "Ptr{Ptr{Cdouble}}", "Ptr{Int64}", "Ptr{Ptr{Cdouble}}"]
    assert "(:fos_feas_dense_block_stats, libfoship)" in jl
