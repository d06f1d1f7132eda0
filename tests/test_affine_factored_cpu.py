"""The factored dense IndAffine (csrc/affine_dense.hip), the parts that need no GPU: fos_host_affine_factored -- the set-up's row scaling, the blocked Cholesky
inverse of A A' accepted by the set-up's probe, and the two passes over A with the kernels' split and summation order -- against the oracle's IndAffine (dense
Cholesky of A A') at the project's tolerance for an exact affine projection, 1e-12 max(1, |x|_inf); its refusals; the entries in every layer."""
import re
from pathlib import Path

import numpy as np
import pytest

from affine_factored_cases import SHAPES, TOL, instance, range_defect

ROOT = Path(__file__).resolve().parent.parent
FOS_EINVAL = -1                                     # include/foship.h


def host_project(pkg, A, b, refine, x):
    lib = pkg.lib.load()
    m, n = A.shape
    y = np.full(n, np.nan)
    rc = lib.fos_host_affine_factored(m, n, pkg.lib.dptr(np.ascontiguousarray(A)), pkg.lib.dptr(b), refine, pkg.lib.dptr(x), pkg.lib.dptr(y))
    return rc, y


@pytest.mark.parametrize("refine", [0, 1])
@pytest.mark.parametrize("family,m,n", SHAPES)
def test_host_emulation_matches_the_oracle(pkg, oracle, family, m, n, refine):
    A, b = instance(family, m, n)
    x = np.random.default_rng(1).standard_normal(n)
    ref = np.empty(n)
    oracle.IndAffine(A, b).prox(ref, x)
    rc, y = host_project(pkg, A, b, refine, x)
    assert rc == 0, pkg.lib.load().fos_last_error().decode()
    scale = max(1.0, np.abs(x).max())
    err, defect = np.abs(y - ref).max(), range_defect(A, x, y)
    print("%s (%d, %d) refine %d: |y - oracle| = %.2e, range defect %.2e (bar %.2e)" % (family, m, n, refine, err, defect, TOL * scale))
    assert err <= TOL * scale
    # y - x = -A'd is formed as a combination of the rows of A: what it misses of the range of A' is the rounding of that sum, far inside the tolerance
    assert defect <= TOL * scale


def test_rank_deficient_and_zero_rows_are_refused(pkg):
    lib = pkg.lib.load()
    A, b = instance("gauss", 10, 30)
    x = np.ones(30)
    D = A.copy(); D[7] = D[2]                                      # a duplicated row
    rc, _ = host_project(pkg, D, b, 0, x)
    assert rc == FOS_EINVAL and "full row rank" in lib.fos_last_error().decode()
    C = A.copy(); C[5] = C[1] + C[3]                               # a row in the span of two others
    rc, _ = host_project(pkg, C, b, 0, x)
    assert rc == FOS_EINVAL and "full row rank" in lib.fos_last_error().decode()
    Z = A.copy(); Z[4] = 0.0
    rc, _ = host_project(pkg, Z, b, 0, x)
    assert rc == FOS_EINVAL and "zero" in lib.fos_last_error().decode()
    N = A.copy(); N[3, 3] = np.nan
    assert host_project(pkg, N, b, 0, x)[0] == FOS_EINVAL
    assert host_project(pkg, A, b, 3, x)[0] == FOS_EINVAL          # refine: 0 .. 2
    assert host_project(pkg, A.T.copy(), np.ones(30), 0, np.ones(10))[0] == FOS_EINVAL      # m > n
    assert host_project(pkg, A, b, 0, x)[0] == 0


def test_python_layer_validates_the_form(pkg):
    A, b = instance("gauss", 7, 9)
    S = pkg.IndAffine(A, b, form="factored", factor="newton", refine=2)
    assert (S.form, S.factor, S.refine, S.sparse) == ("factored", "newton", 2, False)
    import scipy.sparse as sp
    S = pkg.IndAffine(sp.csc_matrix(A), b, form="factored")
    assert isinstance(S.A, np.ndarray) and S.A.flags["C_CONTIGUOUS"] and (S.factor, S.refine) == ("cholesky", 0)
    for kw in (dict(form="projector"), dict(form="factored", refine=3), dict(form="factored", factor="ldl"), dict(form="factored", sparse=True)):
        with pytest.raises(ValueError):
            pkg.IndAffine(A, b, **kw)
    D = pkg.IndAffine(A, b)                                        # form=None: today's selection, to the letter
    assert D.form is None and D.sparse is False and pkg.IndAffine(sp.csc_matrix(A), b).sparse is True
    assert pkg.IndAffine(np.zeros((1, pkg.IndAffine.DENSE_MAX + 1)), np.zeros(1)).sparse is True


def test_entries_exist_in_every_layer(pkg):
    lib = pkg.lib.load(check_symbols=True)
    hdr = (ROOT / "include" / "foship.h").read_text()
    jl = (ROOT / "firstordersolvers.jl_amd" / "julia" / "FOSHip.jl").read_text()
    for name in ("fos_feas_set_affine_factored", "fos_feas_affine_factored_stats", "fos_feas_affine_factored_plan", "fos_host_affine_factored"):
        assert getattr(lib, name) is not None
        assert name in pkg.lib.PROTOTYPES and name in pkg.lib.header_symbols()
    assert re.search(r"#define\s+FOS_ABI_VERSION\s+1\b", hdr)
    assert "ccall((:fos_feas_set_affine_factored, libfoship)" in jl and ":affine_form" in jl
