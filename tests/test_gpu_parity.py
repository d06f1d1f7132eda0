"""
GPU parity tests: the HIP path (through the C ABI, via the ctypes host mirror) against the oracle on the same
seeded inputs.  fp64 everywhere; tolerances are stated per test.  The operator / cone entry points agree to
rounding (different summation order only); anything that runs CG is compared at the accuracy the CG tolerance
of that call allows, and whole solves are compared at convergence (residuals and solution).
"""
import math

import numpy as np
import pytest
import scipy.sparse as sp

import fos_oracle as orc

pytestmark = pytest.mark.gpu


def _codes(cones):
    return [(orc.CONE_CODES[k], l) for k, l in cones]


def omodel(prob):
    return orc.Model(prob.A, prob.b, prob.c, _codes(prob.K1), _codes(prob.K2))


def relerr(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(1e-300, np.linalg.norm(b)))


def random_problem(pkg, rng, m, n, density, K1=None, K2=None):
    A = sp.random(m, n, density=density, format="csc", random_state=rng, data_rvs=rng.standard_normal)
    K1 = K1 or [("Zero", m)]
    K2 = K2 or [("NonNeg", n)]
    return pkg.workloads.from_complementary_pair("rand", A, K1, K2, rng)


def shapes(pkg):
    """Operator test matrices: empty rows/cols, long rows (> NNZ_BLK = 1024 entries), many tiny rows, dense."""
    rng = np.random.default_rng(7)
    out = []
    out.append(("tiny-dense", sp.csc_matrix(rng.standard_normal((3, 2)))))
    out.append(("sparse", sp.random(300, 500, density=0.02, format="csc", random_state=rng, data_rvs=rng.standard_normal)))
    A = sp.random(400, 700, density=0.004, format="lil", random_state=rng, data_rvs=rng.standard_normal)
    A[17, :] = 0
    A[:, 5] = 0
    out.append(("empty-rows-cols", A.tocsc()))
    out.append(("long-rows", sp.csc_matrix(rng.standard_normal((5, 3000)))))           # rows of A: 3000 nnz; rows of A': 5
    out.append(("tall-dense", sp.csc_matrix(rng.standard_normal((2500, 4)))))
    out.append(("identity-like", sp.identity(1500, format="csc") * 2.0))
    out.append(("mixed-lengths", sp.vstack([sp.csc_matrix(rng.standard_normal((2, 1300))),
                                            sp.random(600, 1300, density=0.01, format="csc", random_state=rng,
                                                      data_rvs=rng.standard_normal)]).tocsc()))
    # dual tiles (dense rectangles stored once, column sums by the in-register butterfly, deferred rows)
    out.append(("tile-1chunk", sp.csc_matrix(rng.standard_normal((100, 40)))))
    out.append(("tile-chunks", sp.csc_matrix(rng.standard_normal((70, 300)))))
    out.append(("tile-blockdiag", sp.block_diag([rng.standard_normal((80, 12)) for _ in range(6)], format="csc")))
    out.append(("tile-mixed", sp.vstack([sp.csc_matrix(rng.standard_normal((48, 150))),
                                         sp.random(120, 150, density=0.05, format="csc", random_state=rng, data_rvs=rng.standard_normal),
                                         sp.csc_matrix(rng.standard_normal((20, 150)))]).tocsc()))
    # random mixes of dense rectangles (some tiled, some too small), sparse noise, empty rows / columns
    from test_operator_format import _random_structured
    for seed in (3, 11, 19, 27, 35):
        out.append(("random-structured-%d" % seed, _random_structured(np.random.default_rng(1000 + seed))))
    out.append(("all-zero", sp.csc_matrix((6, 9))))
    return out


@pytest.fixture(scope="module")
def dev_ops(pkg):
    made = []

    def make(A, b=None, c=None, K1=None, K2=None):
        m, n = A.shape
        rng = np.random.default_rng(m * 1000 + n)
        b = rng.standard_normal(m) if b is None else b
        c = rng.standard_normal(n) if c is None else c
        d = pkg.HipHSDE(A, b, c, K1 or [("Free", m)], K2 or [("Free", n)])
        made.append(d)
        return d, b, c
    yield make
    for d in made:
        d.close()


# ---------------------------------------------------------------------------------------------- operators


def test_q_apply_and_transpose(pkg, dev_ops):
    """mul!(Y,Q,B), mul!(Y,transpose(Q),B)  (HSDEAffine.jl:41-65; test/HSDEAffine.jl:26-43).  rtol 1e-13."""
    for name, A in shapes(pkg):
        d, b, c = dev_ops(A)
        Q = orc.HSDEMatrixQ(A, b, c)
        rng = np.random.default_rng(3)
        x = rng.standard_normal(d.l)
        x0 = x.copy()
        y_ref = np.empty(d.l)
        Q.mul(y_ref, x)
        y = d.q_apply(x)
        assert np.array_equal(x, x0)
        assert relerr(y, y_ref) < 1e-13, name
        Q.mul_t(y_ref, x)
        assert relerr(d.q_apply(x, transpose=True), y_ref) < 1e-13, name


def test_kkt_apply(pkg, dev_ops):
    """mul!(y, KKTMatrix(Q), x) == mul!(Y, HSDEMatrix(Q), B)  (affinepluslinear.jl:37-52, HSDEAffine.jl:131-147)."""
    for name, A in shapes(pkg):
        d, b, c = dev_ops(A)
        M = orc.KKTMatrix(orc.HSDEMatrixQ(A, b, c))
        rng = np.random.default_rng(4)
        x = rng.standard_normal(d.N)
        y_ref = np.empty(d.N)
        M.mul(y_ref, x)
        assert relerr(d.kkt_apply(x), y_ref) < 1e-13, name
        H = orc.HSDEMatrix(orc.HSDEMatrixQ(A, b, c))
        H.mul(y_ref, x)
        assert relerr(d.kkt_apply(x), y_ref) < 1e-13, name


def window_panel_shapes(rng):
    """wide, tall, mid, tiny: rows longer than a window's register slots, empty rows and columns, a dense row and column, panels with fewer
    than 64 rows, a panel that touches MORE THAN 64 windows (the record chunks of the walk), a last window cut by the end of the vector."""
    wide = sp.random(150, 420000, density=2.5e-5, format="csc", random_state=rng, data_rvs=rng.standard_normal)   # its rows' panel spans > 64 windows of 6144
    tall_ = sp.random(9000, 300, density=0.01, format="csc", random_state=rng, data_rvs=rng.standard_normal)
    mid = sp.random(5000, 4100, density=0.004, format="csc", random_state=rng, data_rvs=rng.standard_normal).tolil()
    mid[3, :] = rng.standard_normal(4100) * (rng.random(4100) < 0.5)                 # a row with ~2000 entries: far beyond the register slots
    mid[:, 1] = rng.standard_normal((5000, 1))
    return wide, tall_, sp.csc_matrix(mid), sp.random(3, 5, density=0.5, format="csc", random_state=rng)


@pytest.mark.parametrize("geom", ["1", "2"])
def test_operators_on_forced_window_panels(pkg, geom, monkeypatch):
    """The same Q, Q', KKT and status products with the operator forced into window panels (FOS_WINDOWS = 1: 2016-row panels, 2: the tall
    geometry) on the shapes of window_panel_shapes.  The status sums (fos_check) are held against the extended-precision reference of
    tests/status_reference.py at twice its worst-case fp64 allowance."""
    import status_reference as sref
    monkeypatch.setenv("FOS_WINDOWS", geom)
    rng = np.random.default_rng(77)
    for name, A in zip(("wide", "tall", "mid", "tiny"), window_panel_shapes(rng)):
        m, n = A.shape
        b, c = rng.standard_normal(m), rng.standard_normal(n)
        d = pkg.HipHSDE(A, b, c, [("Free", m)], [("Free", n)])
        st = d.operator_stats()
        assert st["win_panels"] > 0 and st["blocks"] == 0, name
        if name == "wide":
            assert st["win_segments"] > 64
        Q = orc.HSDEMatrixQ(A, b, c)
        x = rng.standard_normal(d.l)
        y_ref = np.empty(d.l)
        Q.mul(y_ref, x)
        assert relerr(d.q_apply(x), y_ref) < 1e-13, name
        Q.mul_t(y_ref, x)
        assert relerr(d.q_apply(x, transpose=True), y_ref) < 1e-13, name
        z = rng.standard_normal(d.N)
        z_ref = np.empty(d.N)
        orc.KKTMatrix(Q).mul(z_ref, z)
        assert relerr(d.kkt_apply(z), z_ref) < 1e-13, name
        res = d.check(z, 1e-5)
        vals, allow = sref.reference(A, b, c, z)
        got = dict(p=res.p, d=res.d, g=res.g, ctx=res.ctx, bty=res.bty, nAxs=res.norm_axs, nATy=res.norm_aty, nb=res.norm_b, nc=res.norm_c,
                   tau=res.tau, kappa=res.kappa)
        rat = sref.ratios(got, vals, allow)
        print("window panels FOS_WINDOWS=%s %-5s worst |check - reference| / allowance: %.3g (%s)" % (geom, name, max(rat.values()), max(rat, key=rat.get)))
        assert max(rat.values()) <= 2.0, (name, rat)
        d.close()


def test_cg_kkt_matches_dense_solve_and_oracle_count(pkg, dev_ops):
    """conjugategradient! on the indefinite KKT system (conjugategradients.jl:31-55)."""
    rng = np.random.default_rng(5)
    A = sp.random(100, 200, density=0.05, format="csc", random_state=rng, data_rvs=rng.standard_normal)
    d, b, c = dev_ops(A)
    Q = orc.HSDEMatrixQ(A, b, c)
    M = orc.KKTMatrix(Q)
    rhs = rng.standard_normal(d.N)
    x0 = rng.standard_normal(d.N)
    tol = d.N * np.finfo(float).eps
    x, it = d.cg_kkt(x0, rhs, tol, 10000)
    Qd = Q.todense()
    Md = np.block([[np.eye(d.l), Qd.T], [Qd, -np.eye(d.l)]])
    xs = np.linalg.solve(Md, rhs)
    assert relerr(x, xs) < 1e-12
    xo = x0.copy()
    it_o = orc.conjugategradient(xo, M, rhs, np.empty(d.N), np.empty(d.N), np.empty(d.N), tol=tol, max_iters=10000)
    assert abs(it - it_o) <= 8, (it, it_o)          # ~165 iterations of a chaotic recurrence: see below
    # loose tolerance.  Plain CG on this INDEFINITE system amplifies rounding differences (measured: 1e-16 after one
    # iteration, 1e-12 after 10, 5e-5 after 20 between two summation orders), so stop iterations may differ by a
    # few; both runs must satisfy the reference's stopping rule ||r|| <= tol and be equally close to the solution.
    x, it = d.cg_kkt(x0, rhs, 1e-3, 10000)
    xo = x0.copy()
    it_o = orc.conjugategradient(xo, M, rhs, np.empty(d.N), np.empty(d.N), np.empty(d.N), tol=1e-3, max_iters=10000)
    assert abs(it - it_o) <= 6, (it, it_o)
    assert np.linalg.norm(Md @ x - rhs) <= 1e-3 * (1 + 1e-6)
    assert np.linalg.norm(x - xs) <= 3 * max(np.linalg.norm(xo - xs), 1e-3)
    # the first iterations agree to rounding
    x5, it = d.cg_kkt(x0, rhs, 1e-300, 5)
    xo = x0.copy()
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        orc.conjugategradient(xo, M, rhs, np.empty(d.N), np.empty(d.N), np.empty(d.N), tol=1e-300, max_iters=5)
    assert it == 5 and relerr(x5, xo) < 1e-12
    # max_iters cap (conjugategradients.jl:42): returns max_iters
    x, it = d.cg_kkt(x0, rhs, 1e-300, 7)
    assert it == 7


def test_prox_affine_sequence(pkg, dev_ops):
    """prox!(y, S1::AffinePlusLinear, x): call counter, tolerance schedule, warm start (affinepluslinear.jl:83-126)."""
    rng = np.random.default_rng(6)
    A = sp.random(60, 90, density=0.1, format="csc", random_state=rng, data_rvs=rng.standard_normal)
    d, b, c = dev_ops(A)
    Q = orc.HSDEMatrixQ(A, b, c)
    S = orc.AffinePlusLinear(Q, np.zeros(d.l), np.zeros(d.l), 1, decreasing_accuracy=True)
    Qd = Q.todense()
    Md = np.block([[np.eye(d.l), Qd.T], [Qd, -np.eye(d.l)]])
    for call in range(1, 7):
        x = rng.standard_normal(d.N)
        tol = S.tolerance()
        y_ref = np.empty(d.N)
        S.prox(y_ref, x)
        y = d.prox_affine(x)
        assert d.prox_count() == S.i == call + 1
        exact = np.linalg.solve(Md, np.concatenate([x[:d.l] + Qd.T @ x[d.l:], np.zeros(d.l)]))
        # both are CG iterates stopped at ||r|| <= tol of the same system from the same warm start; plain CG on the
        # indefinite system amplifies rounding (see test_cg_kkt_...), so compare through the stopping rule
        assert abs(d.cgiter() - S.getcgiter()) <= 4
        assert np.linalg.norm(y - y_ref) <= 2 * tol + 1e-12
        assert np.linalg.norm(Md @ y - np.concatenate([x[:d.l] + Qd.T @ x[d.l:], np.zeros(d.l)])) <= tol * (1 + 1e-9)
        assert np.linalg.norm(y - exact) <= 2 * tol + 1e-12
    d.reset_affine()
    assert d.prox_count() == 1


def test_hsdematrix_prox(pkg, dev_ops):
    """prox!(y, HSDEMatrix(Q), x): projection onto {Qu = v} (HSDEAffine.jl:105-126; test/HSDEAffine.jl:71-81)."""
    rng = np.random.default_rng(8)
    A = rng.standard_normal((40, 70))
    d, b, c = dev_ops(sp.csc_matrix(A))
    Q1 = orc.HSDEMatrixQ(A, b, c).todense()
    x = rng.standard_normal(d.N)
    y = d.hsdematrix_prox(x)
    l = d.l
    u = np.linalg.solve(np.eye(l) + Q1.T @ Q1, x[:l] + Q1.T @ x[l:])
    assert relerr(y, np.concatenate([u, Q1 @ u])) < 1e-10      # reference test uses isapprox (rtol 1.5e-8)


# ---------------------------------------------------------------------------------------------- cones


def test_prox_cones_all_kinds(pkg, dev_ops):
    """prox!(y, S2::DualConeProduct, x) (cones.jl:122-142) on every supported cone kind, both sides.
    Elementwise cones: bit exact.  SOC: 1e-14.  PSD (Jacobi vs LAPACK): 1e-12 absolute x ||x||."""
    prob = pkg.workloads.small_mixed()
    d, _, _ = dev_ops(prob.A, prob.b, prob.c, prob.K1 + [], prob.K2 + [])
    S2 = orc.DualConeProduct(orc.ConeProduct.from_lengths(_codes(prob.K1)), orc.ConeProduct.from_lengths(_codes(prob.K2)))
    rng = np.random.default_rng(9)
    for trial in range(5):
        z = rng.standard_normal(d.N) * (10.0 ** (trial - 2))
        ref = np.empty(d.N)
        S2.prox(ref, z)
        out = d.prox_cones(z)
        assert np.linalg.norm(out - ref) <= 1e-12 * np.linalg.norm(z)
    # elementwise-only problem: exact
    K1 = [("Zero", 3), ("NonNeg", 4), ("NonPos", 2), ("Free", 1)]
    K2 = [("NonNeg", 2), ("Free", 2), ("Zero", 1), ("NonPos", 1)]
    A = sp.random(10, 6, density=0.5, format="csc", random_state=rng, data_rvs=rng.standard_normal)
    d2, _, _ = dev_ops(A, None, None, K1, K2)
    S2 = orc.DualConeProduct(orc.ConeProduct.from_lengths(_codes(K1)), orc.ConeProduct.from_lengths(_codes(K2)))
    z = rng.standard_normal(d2.N)
    ref = np.empty(d2.N)
    S2.prox(ref, z)
    assert np.array_equal(d2.prox_cones(z), ref)


def test_soc_cases_and_rotated(pkg, dev_ops):
    rng = np.random.default_rng(10)
    K1 = [("SOC", 1), ("SOC", 2), ("SOC", 5), ("SOC", 70), ("SOC", 300), ("SOCRotated", 2), ("SOCRotated", 9)]
    m = sum(l for _, l in K1)
    K2 = [("SOC", 4), ("SOCRotated", 3)]
    n = 7
    A = sp.random(m, n, density=0.2, format="csc", random_state=rng, data_rvs=rng.standard_normal)
    d, _, _ = dev_ops(A, None, None, K1, K2)
    S2 = orc.DualConeProduct(orc.ConeProduct.from_lengths(_codes(K1)), orc.ConeProduct.from_lengths(_codes(K2)))
    for trial in range(8):
        z = rng.standard_normal(d.N)
        if trial == 1:
            z[:] = 0.0
        if trial == 2:      # inside the cones: head large
            for s in (n, n + 1, n + 3, n + 8):
                z[s] = 50.0
                z[d.l + s] = 50.0
        if trial == 3:      # in the polar cone: head very negative
            for s in (n, n + 1, n + 3, n + 8):
                z[s] = -50.0
                z[d.l + s] = -50.0
        ref = np.empty(d.N)
        S2.prox(ref, z)
        assert np.linalg.norm(d.prox_cones(z) - ref) <= 1e-14 * max(1.0, np.linalg.norm(z)), trial


YS = np.array([[-0.0064709, -0.22443], [-0.22443, -1.02411]])                 # test/testPSD.jl:3-4
PSD_KNOWN = np.array([[0.03909044662082823, -0.00823811392936668],
                      [-0.00823811392936668, 0.00173614084718757]])


@pytest.fixture(params=["wave", "workgroup", "refine"])
def psd64_kernel(request, monkeypatch):
    """Order-64 cones have three kernels (Jacobi with one wavefront per matrix / one workgroup per matrix, and -- warm, behind a
    previous projection -- refinement by matrix products with the Jacobi kernel behind it; the library picks by batch size):
    the PSD tests run all of them."""
    monkeypatch.setenv("FOS_PSD_WAVE", "1" if request.param == "wave" else "0")
    monkeypatch.setenv("FOS_PSD_REFINE", "1" if request.param == "refine" else "0")
    return request.param


def test_psd_known_answer_and_sizes(pkg, dev_ops, psd64_kernel):
    """test/testPSD.jl:14-19 known answer through the GPU PSD kernel; random orders 1..64 (the Jacobi kernels of psd.hip) and 96, 120,
    150 (the sign iteration of psd_sign.hip, which takes every order above 64); degenerate spectra (+-lambda pairs, zero matrix, rank one).
    Matrix by matrix against extended-precision references: test_gpu_psd_edges.py."""
    r2 = math.sqrt(2)
    K1 = [("SDP", 3)]
    d, _, _ = dev_ops(sp.csc_matrix(np.eye(3, 2)), None, None, K1, [("Free", 2)])
    z = np.zeros(d.N)
    xs = np.array([YS[0, 0], r2 * YS[1, 0], YS[1, 1]])
    z[d.l + 2:d.l + 5] = xs                   # s part: primal PSD projection
    z[2:5] = -xs                              # y part: dual = x + P(-x) -> for x = -xs:  -xs + P(xs)
    out = d.prox_cones(z)
    want = np.array([PSD_KNOWN[0, 0], r2 * PSD_KNOWN[1, 0], PSD_KNOWN[1, 1]])
    assert np.allclose(out[d.l + 2:d.l + 5], want, atol=1e-14, rtol=0)
    assert np.allclose(out[2:5], -xs + want, atol=1e-14, rtol=0)

    rng = np.random.default_rng(11)
    for k in (1, 2, 3, 5, 8, 17, 33, 64, 96, 120, 150):
        ln = k * (k + 1) // 2
        d, _, _ = dev_ops(sp.random(ln, 3, density=0.1, format="csc", random_state=rng), None, None, [("SDP", ln)], [("Free", 3)])
        S2 = orc.DualConeProduct(orc.ConeProduct.from_lengths([(orc.CONE_SDP, ln)]), orc.ConeProduct.from_lengths([(orc.CONE_FREE, 3)]))
        cases = [rng.standard_normal(d.N), np.zeros(d.N)]
        # +-lambda pairs: M = [[0,1],[1,0]] pattern embedded (the case plain one-sided Jacobi gets wrong)
        G = np.zeros((k, k))
        for i in range(0, k - 1, 2):
            G[i, i + 1] = G[i + 1, i] = 1.0 + i
        zz = np.zeros(d.N)
        sv = pkg.workloads._svec(G)
        zz[3:3 + ln] = sv
        zz[d.l + 3:d.l + 3 + ln] = sv
        cases.append(zz)
        v = rng.standard_normal(k)
        zz = np.zeros(d.N)
        zz[d.l + 3:d.l + 3 + ln] = pkg.workloads._svec(np.outer(v, v))      # rank one PSD: projection = itself
        zz[3:3 + ln] = pkg.workloads._svec(-np.outer(v, v))
        cases.append(zz)
        for z in cases:
            ref = np.empty(d.N)
            S2.prox(ref, z)
            out = d.prox_cones(z)
            assert np.linalg.norm(out - ref) <= 5e-13 * max(1.0, np.linalg.norm(z)), k


def test_psd_warm_start_drift_and_clustered_spectra(pkg, dev_ops, psd64_kernel):
    """The warm-started Jacobi (previous eigenvector basis, confirming sweep skipped when a sweep's rotations were all tiny):
    slowly drifting matrices as in the solver's steady state, clustered / repeated eigenvalues, eigenvalues straddling zero by
    1e-9, wide dynamic range -- order 64 (register fast path) and 16 (generic path); every call against LAPACK (oracle)."""
    rng = np.random.default_rng(5)
    for k in (64, 16):
        ln = k * (k + 1) // 2
        d, _, _ = dev_ops(sp.random(ln, 3, density=0.1, format="csc", random_state=rng), None, None, [("SDP", ln)], [("Free", 3)])
        S2 = orc.DualConeProduct(orc.ConeProduct.from_lengths([(orc.CONE_SDP, ln)]), orc.ConeProduct.from_lengths([(orc.CONE_FREE, 3)]))
        Q, _ = np.linalg.qr(rng.standard_normal((k, k)))
        sym = lambda B: (B + B.T) / 2
        M0, E = sym(rng.standard_normal((k, k))), sym(rng.standard_normal((k, k)))
        mats = [M0 + t * 1e-4 * E for t in range(6)]                                         # drift
        mats += [M0 + 1e-9 * t * E for t in range(3)]                                        # almost no change: tiny rotations only
        half = k // 2
        mats.append(Q @ np.diag([1.0] * half + [-1.0] * (k - half)) @ Q.T)                    # two clusters
        mats.append(Q @ np.diag(np.concatenate([1 + 1e-9 * rng.standard_normal(half), -1 + 1e-9 * rng.standard_normal(k - half)])) @ Q.T)
        mats.append(Q @ np.diag(1e-9 * rng.standard_normal(k)) @ Q.T + 0.0)                  # everything next to zero
        mats.append(Q @ np.diag(np.concatenate([np.logspace(-8, 8, half), -np.logspace(-8, 8, k - half)])) @ Q.T)
        mats.append(np.eye(k))
        mats.append(-np.eye(k))
        for it, M in enumerate(mats):
            sv = pkg.workloads._svec(sym(M))
            z = np.zeros(d.N)
            z[3:3 + ln] = sv                     # y part (dual copy)
            z[d.l + 3:d.l + 3 + ln] = sv         # s part (primal copy)
            ref = np.empty(d.N)
            S2.prox(ref, z)
            out = d.prox_cones(z)
            assert np.linalg.norm(out - ref) <= 1e-12 * max(1e-300, np.linalg.norm(z)), (k, it)


def test_psd_refinement_path(pkg, dev_ops, monkeypatch):
    """psd64_refine_kernel (warm order-64 projections by matrix products: three per iteration, quadratic convergence) against
    LAPACK (oracle) on sequences built to take each of its paths -- the kernel's own record says which one ran:
    100 (+ 1000 if the extrapolated start was accepted) + 16 rotations + iterations = accepted, otherwise the sweeps of the
    Jacobi kernel it handed the matrix to."""
    monkeypatch.setenv("FOS_PSD_REFINE", "1")
    monkeypatch.setenv("FOS_PSD_WAVE", "0")
    rng = np.random.default_rng(77)
    k, ncone = 64, 3
    ln = k * (k + 1) // 2
    K1 = [("SDP", ln)] * ncone
    d, _, _ = dev_ops(sp.random(ncone * ln, 3, density=0.01, format="csc", random_state=rng), None, None, K1, [("Free", 3)])
    d.psd_debug(True, 0)
    S2 = orc.DualConeProduct(orc.ConeProduct.from_lengths([(orc.CONE_SDP, ln)] * ncone), orc.ConeProduct.from_lengths([(orc.CONE_FREE, 3)]))
    sym = lambda B: (B + B.T) / 2

    def project(mats):
        z = np.zeros(d.N)
        for c_, M in enumerate(mats):
            sv = pkg.workloads._svec(sym(M))
            z[3 + c_ * ln:3 + (c_ + 1) * ln] = sv * (1.0 + 0.25 * c_)       # the dual copy sees a scaled matrix: six different ones
            z[d.l + 3 + c_ * ln:d.l + 3 + (c_ + 1) * ln] = sv
        ref = np.empty(d.N)
        S2.prox(ref, z)
        out = d.prox_cones(z)
        err = np.linalg.norm(out - ref) / max(1e-300, np.linalg.norm(z))
        st = d.psd_sweeps().copy()
        st[st >= 1100] -= 1000
        return err, st

    base = [sym(rng.standard_normal((k, k))) for _ in range(ncone)]
    drift = [sym(rng.standard_normal((k, k))) for _ in range(ncone)]
    err, st = project(base)                                   # cold: no basis yet -> Jacobi
    assert err <= 5e-13 and (st < 100).all() and (st > 0).all(), (err, st)
    # (1) steady drift, 1e-3 relative per call: accepted after 3-5 iterations, no rotation as a rule
    for t in range(1, 6):
        err, st = project([B + 1e-3 * t * D for B, D in zip(base, drift)])
        assert err <= 5e-13, (t, err, st)
        assert (st >= 100).all() and ((st - 100) % 16 <= 8).all(), (t, st)
    # (2) no change at all, then a change at rounding level: one iteration
    cur = [B + 5e-3 * D for B, D in zip(base, drift)]
    err, st = project(cur)
    assert err <= 5e-13 and (st >= 100).all() and ((st - 100) % 16 <= 4).all(), (err, st)
    # (3) two eigenvalues that nearly coincide and are coupled by the change: the rotation path
    Q, _ = np.linalg.qr(rng.standard_normal((k, k)))
    lam = np.linspace(-1.0, 1.0, k)
    lam[20] = lam[21] + 1e-7                                  # same sign pair
    lam[31] = -2e-7; lam[32] = 3e-7                           # a pair straddling zero
    M1 = Q @ np.diag(lam) @ Q.T
    err, st = project([M1] * ncone)                           # a jump: flagged, Jacobi
    assert err <= 5e-13 and (st < 100).all(), (err, st)
    C = np.zeros((k, k))
    C[20, 21] = C[21, 20] = 3e-6
    C[31, 32] = C[32, 31] = 2e-6
    M2 = M1 + Q @ C @ Q.T + 1e-5 * drift[0]
    err, st = project([M2] * ncone)
    assert err <= 5e-13, (err, st)
    assert (st >= 100).all() and ((st - 100) // 16 >= 1).any(), st          # accepted, with rotations
    # (4) exactly repeated eigenvalues (two clusters), then the same matrix again and a small drift: couplings inside a cluster
    #     are at rounding level and must not be chased
    half = k // 2
    M3 = Q @ np.diag([1.0] * half + [-1.0] * (k - half)) @ Q.T
    project([M3] * ncone)
    for t in range(3):
        err, st = project([M3 + 1e-6 * t * drift[1]] * ncone)
        assert err <= 5e-13, (t, err, st)
    # (5) zero matrix, identity, rank one, a jump back: whatever path, the projection is right
    v = rng.standard_normal(k)
    for M in (np.zeros((k, k)), np.eye(k), np.outer(v, v), -np.outer(v, v), base[0], np.zeros((k, k)), base[1]):
        err, st = project([M] * ncone)
        assert err <= 5e-13, (err, st)
    # (6) huge change of scale with the same eigenvectors: the basis still fits
    err, st = project([1e6 * B for B in base])
    err, st = project([1e6 * (B + 1e-4 * D) for B, D in zip(base, drift)])
    assert err <= 5e-13 and (st >= 100).all(), (err, st)
    # (7) stress of the rotation path: MANY near-coincident and crossing pairs at once (ten per matrix, gaps 1e-8 ... 1e-6, coupled by the change at
    #     1e-6 ... 1e-5, some gaps changing sign from call to call) over a sequence of calls -- up to the rotation budget and beyond it (then the
    #     matrix is handed to the Jacobi code): pairs that are still flagged after the rotations of an iteration are left to the next one, and whatever
    #     mixture of paths a call takes, the projection is LAPACK's to 5e-13
    lam0 = np.linspace(-1.0, 1.0, k)
    pairs = [(2 + 6 * q, 3 + 6 * q) for q in range(10)]
    saw_rot = saw_jacobi = False
    for t in range(8):
        mats = []
        for c_ in range(ncone):
            lam = lam0.copy()
            Cc = np.zeros((k, k))
            for q, (i, j) in enumerate(pairs):
                gap = (10.0 ** rng.uniform(-8, -6)) * (1 if (t + q + c_) % 3 else -1)      # crossings between calls
                lam[j] = lam[i] + gap
                Cc[i, j] = Cc[j, i] = 10.0 ** rng.uniform(-6, -5)
            mats.append(Q @ (np.diag(lam) + Cc) @ Q.T + 1e-6 * t * drift[c_])
        err, st = project(mats)
        assert err <= 5e-13, (t, err, st)
        saw_rot |= bool(((st >= 100) & ((st - 100) // 16 >= 1)).any())
        saw_jacobi |= bool((st < 100).any())
    assert saw_rot or saw_jacobi, "the stress sequence took neither the rotation path nor the Jacobi fallback"
    d.psd_debug(False, 0)


# ---------------------------------------------------------------------------------------------- status


def test_check_residuals(pkg, dev_ops):
    """checkstatus values (HSDEStatus.jl:33-38,53-63) on arbitrary points, rtol 1e-12."""
    prob = pkg.workloads.small_mixed()
    d, _, _ = dev_ops(prob.A, prob.b, prob.c, prob.K1, prob.K2)
    mo = omodel(prob)
    rng = np.random.default_rng(12)
    for trial in range(4):
        z = rng.standard_normal(d.N)
        z[d.l - 1] = abs(z[d.l - 1]) + 0.1
        res = d.check(z, 1e-5)
        ref = orc.residuals(mo, z)
        for key in ("p", "d", "g", "ctx", "bty", "kappa", "tau"):
            assert getattr(res, key) == pytest.approx(ref[key], rel=1e-12, abs=1e-14), key
        assert res.norm_axs == pytest.approx(ref["nAxs"], rel=1e-12)
        assert res.norm_aty == pytest.approx(ref["nATy"], rel=1e-12)
        assert pkg.lib.STATUS_NAMES[res.status] == orc.decide_status(ref, 1e-5)
    # an optimal point is reported optimal
    z = np.concatenate([prob.x0, prob.y0, [1.0], prob.c + prob.A.T @ prob.y0, prob.s0, [0.0]])
    res = d.check(z, 1e-8)
    assert pkg.lib.STATUS_NAMES[res.status] == "Optimal"


# ---------------------------------------------------------------------------------------------- iterate-level parity


def _oracle_run(pkg, prob, mk, iters, perturb):
    alg = mk(orc)
    mo = omodel(prob)
    alg.init(mo)
    x = orc.hsde_initialvalue(mo)
    if perturb:
        x[np.abs(x) > 0] *= (1 + 2.220446049250313e-16)       # one ulp on tau and kappa
    st = orc.HSDEStatus(mo, 10 ** 9, 1e-5, 0, 0)
    out = []
    for i in range(1, iters + 1):
        st.i = i
        alg.step(x, i, st)
        out.append((x.copy(), alg.S1.getcgiter(), getattr(alg, "alpha12", None)))
    return out, alg


@pytest.mark.parametrize("algname", ["DR", "GAP", "GAPA", "FISTA", "Dykstra", "AP"])
def test_first_iterations_match_oracle(pkg, algname):
    """Iterate-level parity.  The reference runs plain CG on the INDEFINITE KKT system with a loose, decaying
    tolerance (affinepluslinear.jl:108-118); that iteration amplifies rounding noise: perturbing the oracle's own
    start by ONE ULP moves its iterate by ~5e-9 after the first outer iteration and ~1e-3 after six (where the CG
    stop iteration flips).  So the bar is: the HIP iterates stay as close to the oracle as the oracle stays to its
    one-ulp-perturbed self (factor 50) plus 4 tol_i for every iteration whose CG stop iteration differs, the first
    iteration agrees to 1e-7, and the CG iteration counts agree while the deviation is still below 1e-6."""
    prob = pkg.workloads.small_mixed()
    d = pkg.HipHSDE(prob.A, prob.b, prob.c, prob.K1, prob.K2)
    mk = {"DR": lambda M: M.DR(), "GAP": lambda M: M.GAP(), "GAPA": lambda M: M.GAPA(0.8, 0.5), "FISTA": lambda M: M.FISTA(),
          "Dykstra": lambda M: M.Dykstra(), "AP": lambda M: M.AP()}[algname]
    iters = 25
    ref, alg_o = _oracle_run(pkg, prob, mk, iters, False)
    per, _ = _oracle_run(pkg, prob, mk, iters, True)
    d.set_alg(mk(pkg))
    d.set_iterate(None)
    envelope = kicks = 0.0
    for i in range(1, iters + 1):
        xo, cg_o, a12 = ref[i - 1]
        done, checked, _ = d.step(i, 1, 10 ** 9, 1e-5)
        assert done == 1 and not checked
        z = d.get_iterate()
        dev = np.linalg.norm(z - xo) / max(1.0, np.linalg.norm(xo))
        envelope = max(envelope, np.linalg.norm(per[i - 1][0] - xo) / max(1.0, np.linalg.norm(xo)))
        if d.cgiter() != cg_o:          # a flipped CG stop moves the projection by up to ~2 tol_i (both satisfy ||r|| <= tol_i)
            kicks += 4 * max(0.2 ** math.sqrt(i), d.l * 2.2e-16) / max(1.0, np.linalg.norm(xo))
        assert dev <= 50 * envelope + kicks + 1e-12, (i, dev, envelope, kicks)
        if i == 1:
            assert dev < 1e-7
        if dev < 1e-6 and envelope < 1e-6:
            assert d.cgiter() == cg_o, (i, d.cgiter(), cg_o)
            if algname == "GAPA":
                assert d.alpha12() == pytest.approx(a12, rel=1e-4)
    d.close()


@pytest.mark.parametrize("algname", ["FISTA", "Dykstra", "GAPA"])
def test_algorithm_state_hand_over_mid_solve(pkg, algname):
    """fos_get_alg_state / fos_set_alg_state (FISTAData y, xold, t -- fista.jl:15-25; DykstraData p, q -- dykstra.jl:12-23; GAPAData.alpha12):
    a run handed over mid-solve goes on exactly as the run that was never interrupted -- device -> oracle (the oracle's next steps
    from the device's state equal the device's), oracle -> device, and device -> a second device handle.  With direct = true, so that no
    loosely converged CG sits in the loop: at iteration 30 its tolerance is 1e-4 and a 1e-13 difference (a cold against a warm PSD
    projection) grows to 1e-5 within three steps -- measured on this very test before it ran in direct mode."""
    prob = pkg.workloads.small_mixed()
    mk = {"FISTA": lambda M: M.FISTA(direct=True), "Dykstra": lambda M: M.Dykstra(direct=True), "GAPA": lambda M: M.GAPA(0.8, 0.5, direct=True)}[algname]
    BIG, warm = 10 ** 9, 30
    d = pkg.HipHSDE(prob.A, prob.b, prob.c, prob.K1, prob.K2)
    d.enable_direct(prob.A)
    d.set_alg(mk(pkg))
    d.set_iterate(None)
    d.step(1, warm, BIG, 1e-5)
    z = d.get_iterate()
    a, b, t, a12 = d.get_alg_state()
    if algname == "FISTA":
        assert t > 1.0 and np.linalg.norm(a) > 0 and np.linalg.norm(b) > 0
    # device -> oracle
    mo = omodel(prob)
    alg = mk(orc)
    alg.init(mo)
    if algname == "FISTA":
        alg.y[:], alg.xold[:], alg.t = a, b, t
    elif algname == "Dykstra":
        alg.p[:], alg.q[:] = a, b
    else:
        alg.alpha12 = a12
    st = orc.HSDEStatus(mo, BIG, 1e-5, 0, 0, S1=alg.S1)
    xo = z.copy()
    for i in range(warm + 1, warm + 4):
        st.i = i
        alg.step(xo, i, st)
    # device -> a second handle
    d2 = pkg.HipHSDE(prob.A, prob.b, prob.c, prob.K1, prob.K2)
    d2.enable_direct(prob.A)
    d2.set_alg(mk(pkg))
    d2.set_iterate(z)
    d2.set_alg_state(a, b, t, a12)
    d2.step(warm + 1, 3, BIG, 1e-5)
    d.step(warm + 1, 3, BIG, 1e-5)
    zg, zg2 = d.get_iterate(), d2.get_iterate()
    # the resumed handle repeats the uninterrupted one -- to rounding: the warm-start bases of the PSD kernels are not part of the hand-over
    tol = 1e-10 if algname != "GAPA" else 1e-7                  # (GAPA's step-length estimate amplifies rounding: tests/test_gpu_longstep.py)
    assert relerr(zg, zg2) < tol, relerr(zg, zg2)
    assert relerr(zg, xo) < tol, relerr(zg, xo)
    assert np.linalg.norm(zg - z) > 1e4 * tol * max(1.0, np.linalg.norm(z))     # (the steps moved the iterate: the comparison is not vacuous)
    # without the hand-over the resumed run is a different run
    d3 = pkg.HipHSDE(prob.A, prob.b, prob.c, prob.K1, prob.K2)
    d3.enable_direct(prob.A)
    d3.set_alg(mk(pkg))
    d3.set_iterate(z)
    d3.step(warm + 1, 3, BIG, 1e-5)
    if algname != "GAPA":
        assert relerr(d3.get_iterate(), zg) > 1e3 * tol
    d3.close()
    # oracle -> device: the oracle's state after those three steps installed on the second handle, one more step on both
    d2.set_iterate(xo)
    if algname == "FISTA":
        d2.set_alg_state(alg.y, alg.xold, alg.t, None)
    elif algname == "Dykstra":
        d2.set_alg_state(alg.p, alg.q, None, None)
    else:
        d2.set_alg_state(None, None, None, alg.alpha12)
    st.i = warm + 4
    alg.step(xo, warm + 4, st)
    d2.step(warm + 4, 1, BIG, 1e-5)
    assert relerr(d2.get_iterate(), xo) < tol
    with pytest.raises(pkg.lib.FosError):
        d2.set_alg_state(None, None, 0.5, None)                 # t < 1 cannot be a FISTA state
    d.close()
    d2.close()


# ---------------------------------------------------------------------------------------------- whole solves


def solve_both(pkg, prob, mk, **opts):
    out = []
    model = pkg.solve(prob, mk(pkg, **opts), out=out)
    sol = orc.solve(omodel(prob), mk(orc, **opts), out=[])
    return model, sol, out


def test_readme_nnls_dr_gapa(pkg):
    """test/testDRandGAPA.jl:9-49 on the GPU path (optimum checked against scipy nnls, as in the oracle test)."""
    import scipy.optimize
    prob = pkg.workloads.c1_readme_nnls(seed=2)
    n = prob.meta["n"]
    xs, rnorm = scipy.optimize.nnls(prob.meta["Ad"], prob.meta["bd"])
    opt = rnorm ** 2
    eps = 1e-8
    model, sol, out = solve_both(pkg, prob, lambda M, **o: M.DR(**o), eps=eps, verbose=1)
    assert model.status() == "Optimal" == sol.status
    assert model.getobjval() == pytest.approx(opt, rel=1e-6)
    x = model.getsolution()
    assert abs(min(x[:n].min(), 0.0)) < 10 * eps
    assert np.max(np.abs(x[:n] - sol.x[:n])) < 1e-7
    assert abs(model.iterations - sol.iterations) <= model.options.get("checki", 100)
    # residuals at convergence within 1e-8 of the oracle's (BASELINE.json: "residuals within 1e-8 of reference")
    last, olast = model.status_obj.last, sol.status_obj.last
    for key in ("p", "d", "g"):
        assert abs(getattr(last, key) - olast[key]) < 1e-8
    # printed table (test/testprint.jl:15-19)
    assert out[2] == pkg.HEADER_CG and out[1] == "-" * 81
    assert out[4].startswith("   100|")
    assert any(s.startswith("Found solution i=") for s in out)
    for key in ("p", "d", "g", "ctx", "bty", "κ", "τ", "t", "cgiter"):
        assert key in model.history
    model, sol, _ = solve_both(pkg, prob, lambda M, **o: M.GAPA(**o), eps=1e-4, verbose=0)
    assert model.status() == "Optimal"
    assert abs((model.getobjval() - opt) / opt) < 2e-3
    model, sol, _ = solve_both(pkg, prob, lambda M, **o: M.GAPA(0.5, 0.9, **o), eps=1e-9, verbose=0)
    assert model.status() == "Optimal"
    assert abs((model.getobjval() - opt) / opt) < 1e-6
    assert np.max(np.abs(model.getsolution()[:n] - xs)) < 1e-5


def test_psd_dr_solve(pkg):
    """test/testPSD.jl:22-25: DR(eps=1e-8) through the PSD kernel == projection, atol 1e-8."""
    prob = pkg.workloads.psd2x2_reference_problem()
    model = pkg.solve(prob, pkg.DR(eps=1e-8, verbose=0))
    assert model.status() == "Optimal"
    v = model.getsolution()[1:]
    Y = np.array([[v[0], v[1] / math.sqrt(2)], [v[1] / math.sqrt(2), v[2]]])
    assert np.allclose(Y, PSD_KNOWN, atol=1e-8, rtol=0)


@pytest.mark.parametrize("algname", ["DR", "GAPA", "FISTA"])
def test_mixed_cone_solve_matches_oracle(pkg, algname):
    """Whole solves on a problem with every cone kind: same status, iteration count within one check interval, same
    solution (to the accuracy eps gives the oracle itself), residuals p/d/g within 1e-8 of the oracle's at
    convergence (BASELINE.json north_star)."""
    prob = pkg.workloads.small_mixed()
    mk = {"DR": lambda M, **o: M.DR(**o), "GAPA": lambda M, **o: M.GAPA(0.8, 0.5, **o), "FISTA": lambda M, **o: M.FISTA(**o)}[algname]
    opts = dict(eps=1e-6, verbose=0, max_iters=3000 if algname != "FISTA" else 300, checki=50)
    model, sol, _ = solve_both(pkg, prob, mk, **opts)
    assert model.status() == sol.status
    assert abs(model.iterations - sol.iterations) <= 50
    last, olast = model.status_obj.last, sol.status_obj.last
    if sol.status == "Optimal":
        ref_err = np.max(np.abs(sol.x - prob.x0))
        assert np.max(np.abs(model.getsolution() - prob.x0)) <= 3 * ref_err + 1e-9
        assert model.getobjval() == pytest.approx(sol.obj_val, abs=1e-4)
        for key in ("p", "d", "g"):
            assert abs(getattr(last, key) - olast[key]) < 1e-8 * 1e2      # eps = 1e-6 here: both are below eps (1+norm)
    else:
        for key in ("p", "d", "g"):
            assert getattr(last, key) == pytest.approx(olast[key], rel=0.5)


@pytest.mark.parametrize("algname", ["DR", "GAPA"])
def test_tile_stored_lp_solve_matches_oracle(pkg, algname):
    """Whole solves on a dense LP whose operator is partly stored as dual tiles (96 x 180: the first 64 rows as three 64-column
    chunks, the other 32 rows in ordinary blocks, so every column of A is a deferred row WITH an own partial and the 64 tile
    rows are deferred across chunks): status, iteration count, solution and residuals against the oracle."""
    prob = pkg.workloads.small_lp(seed=21, m=96, n=180)
    dev = pkg.HipHSDE(prob.A, prob.b, prob.c, prob.K1, prob.K2)
    st = dev.operator_stats()
    dev.close()
    assert st["tiles"] == 3 and st["deferred"] == 64 + 180, st
    mk = {"DR": lambda M, **o: M.DR(**o), "GAPA": lambda M, **o: M.GAPA(0.8, 0.5, **o)}[algname]
    # (this LP converges slowly: both runs stop at max_iters with the reference's :Continue -> :Indeterminate; what is compared
    # is the whole 1500-iteration trajectory's end point)
    model, sol, _ = solve_both(pkg, prob, mk, eps=1e-6, verbose=0, max_iters=1500, checki=50)
    assert model.status() == sol.status
    assert model.iterations == sol.iterations
    assert np.max(np.abs(model.getsolution() - sol.x)) <= 1e-4 * max(1.0, np.max(np.abs(sol.x)))
    assert model.getobjval() == pytest.approx(sol.obj_val, rel=1e-4, abs=1e-6)
    last, olast = model.status_obj.last, sol.status_obj.last
    for key in ("p", "d", "g"):
        assert getattr(last, key) == pytest.approx(olast[key], rel=1e-3)


def test_max_iters_forced_check_and_history(pkg):
    """solverwrapper.jl:31-34: forced check on the guess when the last iteration was not a check iteration."""
    prob = pkg.workloads.c1_readme_nnls(seed=2)
    model = pkg.solve(prob, pkg.GAP(0.5, 2.0, 2.0, max_iters=150, verbose=0, debug=2))
    assert model.iterations == 150
    assert [i for i, _ in model.history["p"]] == [100, 150]
    assert model.history["x"][0][1].shape == (prob.n,)
    assert model.status() in ("Indeterminate", "Optimal")


def test_infeasible_and_unbounded_detection(pkg):
    """The :Unbounded / :Infeasible branches of checkstatus (HSDEStatus.jl:58-63) through the GPU residual kernel:
    same verdict at the same check as the oracle.  (The reference's tests are literal -- e.g. ||A'y|| rather than
    ||A'y - r|| -- and are reproduced as they are.)"""
    rng = np.random.default_rng(0)
    m, n = 8, 12
    Ad = rng.standard_normal((m, n))
    y = rng.standard_normal(m)
    Ad = Ad * np.sign(Ad.T @ y)[None, :]                    # A'y >= 0
    b = -np.abs(rng.standard_normal(m)) * np.sign(y)        # b'y < 0  -> {Ax = b, x >= 0} is infeasible (Farkas)
    inf = pkg.workloads.ConicProblem("inf", sp.csc_matrix(Ad), b, rng.standard_normal(n), [("Zero", m)], [("NonNeg", n)])
    A2 = rng.standard_normal((m, n))
    dd = rng.standard_normal(n)
    A2 = A2 - np.outer(np.maximum(A2 @ dd, 0) + 0.1, dd) / (dd @ dd)     # A2 d <= -0.1, c'd < 0: unbounded ray
    unb = pkg.workloads.ConicProblem("unb", sp.csc_matrix(A2), np.abs(rng.standard_normal(m)) + 1, -dd, [("NonNeg", m)], [("Free", n)])
    for prob in (inf, unb):
        model, sol, _ = solve_both(pkg, prob, lambda M, **o: M.DR(**o), eps=1e-6, verbose=0, max_iters=5000, checki=20)
        assert model.status() == sol.status, prob.name
        assert model.status() in ("Unbounded", "Infeasible")
        assert model.iterations == sol.iterations


def test_bad_inputs_fail_loudly(pkg):
    A = sp.csc_matrix(np.eye(3))
    with pytest.raises(pkg.lib.FosError):          # gap in the cone ranges (cones.jl:69)
        pkg.HipHSDE(A, np.zeros(3), np.zeros(3), [("Zero", 2)], [("Free", 3)])
    with pytest.raises(pkg.lib.FosError):          # SDP length not triangular
        pkg.HipHSDE(sp.csc_matrix(np.eye(4)), np.zeros(4), np.zeros(4), [("SDP", 4)], [("Free", 4)])
    with pytest.raises(pkg.lib.FosError):          # an exponential cone has exactly 3 entries
        pkg.HipHSDE(sp.csc_matrix(np.eye(4)), np.zeros(4), np.zeros(4), [("ExpPrimal", 4)], [("Free", 4)])
    with pytest.raises(ValueError):
        pkg.HipHSDE(A, np.zeros(3), np.zeros(3), [("Zero", [1, 3, 2])], [("Free", 3)])


def test_rccl_reduction_path_single_rank(pkg):
    """The sharded code path (local reduce kernel -> in-stream RCCL all-reduce -> finalize from the reduced buffer)
    with a 1-rank communicator must reproduce the single-GPU path bit for bit (same summation order)."""
    prob = pkg.workloads.small_mixed()
    outs = []
    for use_comm in (False, True):
        d = pkg.HipHSDE(prob.A, prob.b, prob.c, prob.K1, prob.K2)
        if use_comm:
            d.comm_init(1, 0, pkg.HipHSDE.comm_unique_id())
        else:
            d.set_cg_variant("merged_update")        # the recurrence sharded handles run by default
        assert d.cg_variant_name() == "merged_update"
        d.set_alg(pkg.GAPA(0.8, 0.5))
        d.set_iterate(None)
        done, checked, res = d.step(1, 30, 30, 1e-6)
        assert done == 30 and checked
        outs.append((d.get_iterate(), d.cgiter(), res.p, res.d, res.g, d.alpha12()))
        d.close()
    assert np.array_equal(outs[0][0], outs[1][0])
    assert outs[0][1:] == outs[1][1:]


def test_exponential_cones(pkg, dev_ops):
    """IndExpPrimal / IndExpDual (conemap :ExpPrimal, :ExpDual; cones.jl:12-13) on both sides of the product, primal and
    Moreau-dual copies.  PARITY UNPINNED upstream (no reference test); checked against the oracle's restatement of the
    SCS-derived algorithm to 1e-9 (the bisection/Newton iteration counts may differ by rounding) and through
    cone membership + Moreau orthogonality."""
    rng = np.random.default_rng(21)
    K1 = [("ExpPrimal", 3), ("ExpDual", 3), ("ExpPrimal", 3), ("NonNeg", 2), ("ExpDual", 3)]
    K2 = [("ExpDual", 3), ("ExpPrimal", 3)]
    m, n = 14, 6
    A = sp.random(m, n, density=0.4, format="csc", random_state=rng, data_rvs=rng.standard_normal)
    d, _, _ = dev_ops(A, None, None, K1, K2)
    S2 = orc.DualConeProduct(orc.ConeProduct.from_lengths(_codes(K1)), orc.ConeProduct.from_lengths(_codes(K2)))
    for trial in range(40):
        z = rng.standard_normal(d.N) * 10.0 ** rng.uniform(-1.5, 1.5)
        ref = np.empty(d.N)
        S2.prox(ref, z)
        out = d.prox_cones(z)
        assert np.linalg.norm(out - ref) <= 1e-9 * max(1.0, np.linalg.norm(z)), trial
    # closed-form cases: a point inside the cone is fixed, a point in the polar cone maps to 0
    z = np.zeros(d.N)
    z[d.l + n:d.l + n + 3] = [0.5, 1.0, 3.0]          # s part of the first K1 cone (ExpPrimal): 1*exp(0.5) <= 3
    out = d.prox_cones(z)
    assert np.array_equal(out[d.l + n:d.l + n + 3], [0.5, 1.0, 3.0])
