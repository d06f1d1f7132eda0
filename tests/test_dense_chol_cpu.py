"""
direct = true, the Cholesky factor of the stored inverse (csrc/dense_chol.hip), the parts that need no GPU: the host emulation of the blocked factorisation
and inversion (fos_host_chol_inverse: the kernels' blocking and block order on the CPU), its bad-pivot report, the entries in every layer and the
factor-name helper.
"""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
ORDERS = [1, 2, 63, 64, 65, 128, 130, 321]          # the edges of the 64-blocking: one block, ragged last blocks, several block columns
FOS_EINVAL = -1                                     # include/foship.h

def spd_matrix(k):
    """K = I + B'B, B 2k x k standard normal: lambda_max ~ (sqrt(2k) + sqrt(k))^2 ~ 1.9e3 at k = 321 and cond(K) ~ 31 (printed by the tests), well inside the
    cond <= 1.9e3 at which numpy.linalg.inv itself leaves max |K X - I| ~ 3.5e-13 of the 1e-12 bar"""
    B = np.random.default_rng(1000 + k).standard_normal((2 * k, k))
    return np.asfortranarray(np.eye(k) + B.T @ B)


def host_chol(pkg, K):
    lib = pkg.lib.load()
    k = K.shape[0]
    X = np.zeros((k, k), order="F")
    bad = ctypes.c_int64(-2)
    rc = lib.fos_host_chol_inverse(k, pkg.lib.dptr(np.asfortranarray(K)), pkg.lib.dptr(X), ctypes.byref(bad))
    return rc, X, bad.value


@pytest.mark.parametrize("k", ORDERS)
def test_host_chol_inverse(pkg, k):
    K = spd_matrix(k)
    rc, X, bad = host_chol(pkg, K)
    resid = float(np.max(np.abs(K @ X - np.eye(k))))
    print("k = %d: cond(K) = %.3e, max |K X - I| = %.3e" % (k, np.linalg.cond(K), resid))
    assert rc == 0 and bad == -1
    assert resid <= 1e-12                              # the project's acceptance bar for a stored inverse
    assert np.array_equal(X, X.T)


@pytest.mark.parametrize("k,col", [(130, 5), (130, 129), (321, 320), (64, 0)])
def test_host_chol_reports_the_bad_pivot(pkg, k, col):
    """a negative diagonal entry in block 0 / in the last ragged block: the first failing column is that one (the leading minor before it is still K's)"""
    K = spd_matrix(k)
    K[col, col] = -1.0
    rc, _, bad = host_chol(pkg, K)
    assert rc == FOS_EINVAL and bad == col
    assert ("column %d" % col) in pkg.lib.load().fos_last_error().decode()


def test_host_chol_rejects_non_finite(pkg):
    K = spd_matrix(70)
    K[66, 66] = np.nan
    rc, _, bad = host_chol(pkg, K)
    assert rc == FOS_EINVAL and bad == 66


def test_factor_name_helper(pkg):
    assert pkg.direct_factor_code("newton") == 0 and pkg.direct_factor_code("cholesky") == 1
    for name in ("Cholesky", "ldl", "", None, 1):
        with pytest.raises(ValueError):
            pkg.direct_factor_code(name)
    assert pkg.DR(direct=True, direct_factor="cholesky").options["direct_factor"] == "cholesky"      # travels as a keyword option


def test_entries_exist_in_every_layer(pkg):
    lib = pkg.lib.load(check_symbols=True)
    hdr = (ROOT / "include" / "foship.h").read_text()
    jl = (ROOT / "firstordersolvers.jl_amd" / "julia" / "FOSHip.jl").read_text()
    for name in ("fos_enable_direct3", "fos_get_direct_stats2", "fos_dense_spd_inverse", "fos_host_chol_inverse"):
        assert getattr(lib, name) is not None
        assert name in pkg.lib.PROTOTYPES and name in pkg.lib.header_symbols()
    assert re.search(r"#define\s+FOS_DIRECT_FACTOR_NEWTON\s+0\b", hdr) and re.search(r"#define\s+FOS_DIRECT_FACTOR_CHOLESKY\s+1\b", hdr)
    assert re.search(r"#define\s+FOS_ABI_VERSION\s+1\b", hdr)
    assert pkg.lib.PROTOTYPES["fos_enable_direct3"][1][-2:] == [ctypes.c_int32, ctypes.c_int32] and len(pkg.lib.PROTOTYPES["fos_enable_direct3"][1]) == 6
    m = re.search(r"ccall\(\(:fos_enable_direct3, libfoship\), Cint, \(([^)]*)\)", jl)
    assert m and [t.strip() for t in m.group(1).split(",")] == ["Ptr{Cvoid}", "Ptr{Int64}", "Ptr{Int64}", "Ptr{Cdouble}", "Int32", "Int32"]
    assert ":direct_factor" in jl
