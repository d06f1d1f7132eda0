"""
direct = true, reduced form (HSDE.jl:12-15; csrc/direct_reduced.hip), the parts that need no GPU: the entries exist in every layer, the algebra the kernels
follow is the oracle's projection, and the tile packing / summation order (host emulation, fos_host_reduced_symm) covers the lower triangle exactly once.
"""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp

import fos_oracle as orc

ROOT = Path(__file__).resolve().parent.parent


def test_entries_exist_in_every_layer(pkg):
    lib = pkg.lib.load(check_symbols=True)
    hdr = (ROOT / "include" / "foship.h").read_text()
    jl = (ROOT / "firstordersolvers.jl_amd" / "julia" / "FOSHip.jl").read_text()
    for name in ("fos_enable_direct2", "fos_get_direct_stats"):
        assert getattr(lib, name) is not None
        assert name in pkg.lib.PROTOTYPES and name in pkg.lib.header_symbols()
    assert re.search(r"#define\s+FOS_DIRECT_FORM_AUTO\s+0\b", hdr) and re.search(r"#define\s+FOS_DIRECT_FORM_REDUCED\s+4\b", hdr)
    assert pkg.lib.PROTOTYPES["fos_enable_direct2"][1][-1] is ctypes.c_int32 and len(pkg.lib.PROTOTYPES["fos_enable_direct2"][1]) == 5
    m = re.search(r"ccall\(\(:fos_enable_direct2, libfoship\), Cint, \(([^)]*)\)", jl)
    assert m and [t.strip() for t in m.group(1).split(",")] == ["Ptr{Cvoid}", "Ptr{Int64}", "Ptr{Int64}", "Ptr{Cdouble}", "Int32"]
    assert pkg.HipHSDE.DIRECT_FORMS == {"auto": 0, "reduced": 4}
    assert pkg.DR(direct=True, direct_form="reduced").options["direct_form"] == "reduced"      # travels as a keyword option


def reduced_projection(A, b, c, x):
    """The reduced form restated in numpy: K^-1 explicit (k = min(m, n)), ONE product with two right-hand sides per application of D^-1."""
    A = np.asarray(sp.csc_matrix(A).todense())
    m, n = A.shape
    l = n + m + 1
    h = np.concatenate([c, b])
    Q0 = np.block([[np.zeros((n, n)), A.T], [-A, np.zeros((m, m))]])
    Q = np.block([[Q0, h[:, None]], [-h[None, :], np.zeros((1, 1))]])
    g = -Q0 @ h
    swap = m < n
    Kinv = np.linalg.inv(np.eye(m) + A @ A.T) if swap else np.linalg.inv(np.eye(n) + A.T @ A)

    def dinv(t1):
        tx, ty = t1[:n], t1[n:]
        if not swap:
            Y = Kinv @ np.column_stack([tx, A.T @ ty])
            return np.concatenate([Y[:, 0], ty - A @ Y[:, 1]])
        Y = Kinv @ np.column_stack([ty, A @ tx])
        return np.concatenate([tx - A.T @ Y[:, 1], Y[:, 0]])

    p, q = dinv(h), dinv(g)
    M = np.array([[1 + h @ p, h @ q], [g @ p, g @ q - (1 + h @ h)]])
    u, v = x[:l], x[l:]
    t = Q @ u - v
    d = dinv(t[:-1])
    sigma, w2 = np.linalg.solve(M, np.array([h @ d, g @ d - t[-1]]))
    w = np.concatenate([d - sigma * p - w2 * q, [w2]])
    return np.concatenate([u + Q @ w, v + w])


def _cases(pkg):
    rng = np.random.default_rng(77)
    pm = pkg.workloads.small_mixed()
    yield "small_mixed", pm.A, pm.b, pm.c
    pl = pkg.workloads.small_lp(seed=3, m=31, n=61)
    yield "small_lp 31x61", pl.A, pl.b, pl.c
    yield "lp 61x31", sp.csc_matrix(pl.A.T), pl.c.copy(), pl.b.copy()
    yield "m=1", sp.csc_matrix(rng.standard_normal((1, 7))), rng.standard_normal(1), rng.standard_normal(7)
    yield "n=1", sp.csc_matrix(rng.standard_normal((6, 1))), rng.standard_normal(6), rng.standard_normal(1)
    Ae = rng.standard_normal((9, 5))
    Ae[:, 2] = 0.0
    yield "empty column", sp.csc_matrix(Ae), rng.standard_normal(9), rng.standard_normal(5)
    yield "b=0", sp.csc_matrix(rng.standard_normal((8, 5))), np.zeros(8), rng.standard_normal(5)
    yield "c=0", sp.csc_matrix(rng.standard_normal((5, 8))), rng.standard_normal(5), np.zeros(8)


def test_reduced_algebra_is_the_oracles_projection(pkg):
    rng = np.random.default_rng(5)
    for name, A, b, c in _cases(pkg):
        S1 = orc.IndAffineDirect(orc.HSDEMatrixQ(sp.csc_matrix(A), b, c))
        N = 2 * (A.shape[0] + A.shape[1] + 1)
        for scale in (1.0, 1e3):
            x = scale * rng.standard_normal(N)
            ref = np.empty(N)
            S1.prox(ref, x)
            y = reduced_projection(A, b, c, x)
            assert np.linalg.norm(y - ref) <= 1e-12 * np.linalg.norm(ref), (name, np.linalg.norm(y - ref) / np.linalg.norm(ref))


@pytest.mark.parametrize("k", [1, 63, 64, 65, 200])
def test_tile_packing_and_summation_order(pkg, k):
    """Every entry of the lower triangle sits in exactly one tile slot (the diagonal 64 x 64 blocks whole, nothing of the strict upper triangle outside them), and the
    emulated product -- slots, butterfly, fold in the device's order -- equals X [p q]."""
    lib = pkg.lib.load()
    rng = np.random.default_rng(k)
    B = rng.standard_normal((k, k))
    X = np.asfortranarray(B @ B.T / k + np.eye(k))
    pq = rng.standard_normal((k, 2))
    y = np.zeros((k, 2))
    count = np.zeros((k, k), dtype=np.int32, order="F")
    i32p = ctypes.POINTER(ctypes.c_int32)
    pkg.lib.check(lib.fos_host_reduced_symm(k, pkg.lib.dptr(X), pkg.lib.dptr(pq), pkg.lib.dptr(y), count.ctypes.data_as(i32p)))
    i, j = np.indices((k, k))
    expect = ((i >= j) | (i // 64 == j // 64)).astype(np.int32)
    assert np.array_equal(count, expect)
    ref = X @ pq
    assert np.linalg.norm(y - ref) <= 1e-13 * np.linalg.norm(ref) * max(1.0, np.sqrt(k))
