"""
GPU: dense Quadratic, IndAffine and LeastSquares blocks of a SeparableSum (csrc/dense_blocks.hip) through a handle: every order at which the kernels change path
(the packing steps 1, 2, 4, ... 32 of the wavefront class, the class boundary 64 / 65, the LDS threshold, the cap 1024), mixed with the vector kinds, shared
matrices, whole solves and refusals on a live handle.

Bounds.  With the G and d the device holds (fos_feas_dense_block_get) and y_L = G x + d in np.longdouble, |y - y_L| <= (p + 1) 2^-53 (|G||x| + |d|) elementwise:
the bound of a dot product of length p plus one addition, whatever the order.  Device against host emulation may use twice that.  The library's emulation runs
the kernels' chain (acc = d_r, then one fused multiply-add per j ascending, in every class), so device and emulation are also compared bit for bit.
Against the references the bars are the project's own (dense_block_cases).
"""
import numpy as np
import pytest
import scipy.linalg

import affine_factored_cases as ac
import dense_block_cases as dc
import nspace_cases as nc
import set_cases as sc
from dense_block_cases import FOS_EINVAL, KINDS, P
from feasibility_cases import ALGS
from set_cases import RefBox

pytestmark = pytest.mark.gpu


def _handle(pkg, S, n, S2=None):
    return pkg.HipFeasibility(pkg.Feasibility(S, pkg.IndFree() if S2 is None else S2, n))


def _single(kind, p):
    return dc.block(kind, p, m=max(1, p // 2)) if kind == "IndAffine" else dc.block(kind, p, "gauss", 1.0)


@pytest.mark.parametrize("p", P)
@pytest.mark.parametrize("kind", KINDS)
def test_single_block_every_order(pkg, kind, p):
    blk, x = _single(kind, p), dc.input_of(p)
    d = _handle(pkg, pkg.SeparableSum([(blk.device_set(pkg), p)], dense=True), p)
    y = d.prox(1, x)
    rc, yh, Gh, dh = dc.host_block(pkg, blk, x)
    assert rc == 0
    G, dv = d.dense_block_get(1, 0, p)
    assert np.array_equal(G, Gh) and np.array_equal(dv, dh) and np.array_equal(G, G.T)      # the same set-up code
    yL, bound = dc.kernel_bound(G, dv, x)
    kerr = float((np.abs(y - yL) / np.maximum(bound, 1e-300)).max())
    ref = blk.ref.project(x)
    err, bar = float(np.abs(y - ref).max()), blk.bar(x, ref)
    print("%s p=%d: kernel error / bound %.3f, |device - emulation| = %.2e, |y - ref| = %.2e (bar %.2e)" % (kind, p, kerr, np.abs(y - yh).max(), err, bar))
    assert np.all(np.abs(y - yL) <= bound), (kind, p, kerr)
    assert np.all(np.abs(y - yh) <= 2.0 * bound), (kind, p)
    assert y.tobytes() == yh.tobytes(), (kind, p, "device and emulation run one chain: the same bits")
    assert err <= bar, (kind, p, err, bar)
    assert d.prox(1, x).tobytes() == y.tobytes()
    st, ss = d.dense_block_stats(1), d.set_stats(1)
    wave = p <= dc.WAVE_MAX
    assert (st["dense_blocks"], st["matrices"], st["wave_blocks"], st["workgroup_blocks"], st["launches"], st["largest_order"]) == (1, 1, int(wave), int(not wave), 1, p), st
    in_lds = p <= 200                                                             # 8 (p + p (p + 1) / 2) bytes fit the CU's 160 KiB up to order 200
    assert st["matrix_bytes"] == (4 * p * (p + 1) if in_lds else 8 * p * p) and st["lds_blocks"] == int(in_lds), st      # the triangle in LDS, the square above
    assert (ss["blocks"], ss["wave_blocks"], ss["workgroup_blocks"], ss["grid_blocks"], ss["launches"]) == (1, 0, 0, 0, 1), ss


def _mixed(pkg, seed=3):
    """~200 blocks: vector kinds of set_cases.random_separable_sum's list with lengths 1..1500, dense blocks of the orders of P up to 257 in between, IndFree
    first, last and between dense neighbours; n is not a multiple of 64 -> (SeparableSum, [(tag, reference, start, length, tolerance parameter | Block)], n)"""
    rng = np.random.default_rng(seed)
    orders = [p for p in P if p <= 257]
    dev, layout, pos = [], [], 0

    def add(S, ref, length, what):
        nonlocal pos
        dev.append((S, length)); layout.append((what, ref, pos, length)); pos += length

    def free(length):
        add(pkg.IndFree(), sc.RefFree(), length, "IndFree")

    def dense():
        p = orders[int(rng.integers(len(orders)))]
        kind = KINDS[int(rng.integers(3))]
        add(_single(kind, p).device_set(pkg), _single(kind, p), p, "dense")
    free(3)
    for i in range(115):
        r = rng.random()
        if r < 0.45:
            kind = sc.KINDS[int(rng.integers(len(sc.KINDS)))]
            length = int(rng.integers(1, 1501)) if rng.random() < 0.2 else int(rng.integers(1, 130))
            ref, args, param = sc.make_set(kind, length, rng, variant=i)
            add(getattr(pkg, kind)(*args), ref, length, ("vector", kind, param))
        elif r < 0.75:
            dense()
        else:                                                                     # two dense neighbours with nothing between, then IndFree between two more
            dense(); dense(); free(int(rng.integers(1, 9))); dense()
    free(1 + (62 - pos) % 64)                                                     # n = 63 mod 64
    return pkg.SeparableSum(dev, dense=True), layout, pos


def test_mixed_sum(pkg):
    S, layout, n = _mixed(pkg)
    assert n % 64 == 63 and 150 <= len(layout) <= 260
    x = np.random.default_rng(9).standard_normal(n)
    d = _handle(pkg, S, n)
    y = d.prox(1, x)
    assert d.prox(1, x).tobytes() == y.tobytes()                                  # two calls, the same bits
    ndense = 0
    for what, ref, start, length in layout:
        xb, yb = x[start:start + length], y[start:start + length]
        if what == "IndFree":
            assert yb.tobytes() == xb.tobytes(), ("IndFree at", start)            # nobody wrote outside its own block
        elif what == "dense":
            ndense += 1
            r = ref.ref.project(xb)
            assert np.abs(yb - r).max() <= ref.bar(xb, r), (ref.kind, ref.p, start)
            assert yb.tobytes() == dc.host_block(pkg, ref, xb)[1].tobytes(), (ref.kind, ref.p, start)
        else:
            _, kind, param = what
            assert np.abs(yb - ref.project(xb)).max() <= 1e-13 * max(float(np.abs(xb).max()), abs(param)), (kind, start, length)
    st, ss = d.dense_block_stats(1), d.set_stats(1)
    nvec = len(layout) - ndense
    print("mixed sum: %d blocks, %d dense on %d matrices (%d wavefront, %d workgroup class), n = %d, launches %d" %
          (len(layout), ndense, st["matrices"], st["wave_blocks"], st["workgroup_blocks"], n, ss["launches"]))
    assert st["dense_blocks"] == ndense and st["wave_blocks"] + st["workgroup_blocks"] == ndense and st["wave_blocks"] > 0 and st["workgroup_blocks"] > 0
    assert st["launches"] == 2 and st["matrices"] < ndense                        # (the same instance drawn twice names one ndarray)
    assert ss["blocks"] == len(layout) and ss["wave_blocks"] + ss["workgroup_blocks"] + ss["grid_blocks"] == nvec and ss["grid_blocks"] == 0
    assert ss["launches"] == (ss["wave_blocks"] > 0) + (ss["workgroup_blocks"] > 0) + st["launches"]


@pytest.mark.parametrize("p", [24, 200])
def test_shared_matrix(pkg, p):
    blk = dc.block("Quadratic", p, "gauss", 1.0)
    rng = np.random.default_rng(p)
    qs = [rng.standard_normal(p) for _ in range(50)]
    x = rng.standard_normal(50 * p + 5)
    shared = _handle(pkg, pkg.SeparableSum([(pkg.Quadratic(blk.M, v), p) for v in qs] + [(pkg.IndFree(), 5)], dense=True), 50 * p + 5)
    private = _handle(pkg, pkg.SeparableSum([(pkg.Quadratic(blk.M.copy(), v), p) for v in qs] + [(pkg.IndFree(), 5)], dense=True), 50 * p + 5)
    ys, yp = shared.prox(1, x), private.prox(1, x)
    s, t = shared.dense_block_stats(1), private.dense_block_stats(1)
    print("order %d: shared %s; private %s" % (p, s, t))
    assert (s["dense_blocks"], s["matrices"], s["matrix_bytes"]) == (50, 1, 4 * p * (p + 1)) and (t["dense_blocks"], t["matrices"], t["matrix_bytes"]) == (50, 50, 200 * p * (p + 1))
    assert s["lds_blocks"] == 50 and t["lds_blocks"] == 50                        # order <= 64: always; order 200: 8 (200 + 200 * 201 / 2) = 162 400 bytes <= 160 KiB
    assert ys.tobytes() == yp.tobytes()                                           # sharing changes traffic, never bits
    assert ys[-5:].tobytes() == x[-5:].tobytes()
    for k in (0, 7, 49):
        ref = nc.RefQuadratic(blk.M, qs[k]).project(x[k * p:(k + 1) * p])
        assert np.abs(ys[k * p:(k + 1) * p] - ref).max() <= blk.bar(x[k * p:(k + 1) * p], ref), k


def test_box_qp_by_blocks_under_dr(pkg):
    """Feasibility(SeparableSum(40 x Quadratic of order 16), IndBox(0, 1), 640) under DR against the whole-vector Quadratic(blockdiag(Q), q) handle and the handle's
    own callback path on the reference objects: a DR step is nonexpansive and each reflected prox doubles its error, so after k steps the iterates differ by at most
    2 k sqrt(n) (the sum of the two sets' elementwise bars) in the 2-norm"""
    nb, p, n, steps = 40, 16, 640, 50
    Qs, qs = zip(*[nc.quadratic_of(*nc.instance("gauss", p + 1 + k, p), 0.05) for k in range(nb)])
    Q, q = scipy.linalg.block_diag(*Qs), np.concatenate(qs)
    refs = sc.RefSeparableSum([(nc.RefQuadratic(Qs[k], qs[k]), p) for k in range(nb)])
    blocks = _handle(pkg, pkg.SeparableSum([(pkg.Quadratic(Qs[k], qs[k]), p) for k in range(nb)], dense=True), n, pkg.IndBox(0.0, 1.0))
    whole = _handle(pkg, pkg.Quadratic(Q, q), n, pkg.IndBox(0.0, 1.0))
    callback = _handle(pkg, refs, n, RefBox(0.0, 1.0))
    for h in (blocks, whole, callback):
        h.set_alg(ALGS["DR"](pkg))
        h.set_iterate(None)
    cond = max(nc.scaled_cond(np.eye(p) + Qk) for Qk in Qs)
    worst, xmax = 0.0, 1.0
    for i in range(1, steps + 1):
        for h in (blocks, whole, callback):
            assert h.step(i, 1, 10 ** 9, 1e-30)[0] == 1
        z = blocks.get_iterate()
        xmax = max(xmax, float(np.abs(z).max()))
        bars = nc.TOL * max(1.0, cond / 1e3) * xmax + 1e-13 * xmax                # the Quadratic's bar at the largest iterate so far, the box's
        dev = max(np.linalg.norm(z - whole.get_iterate()), np.linalg.norm(z - callback.get_iterate()))
        worst = max(worst, dev / (2.0 * i * np.sqrt(n) * bars))
        assert dev <= 2.0 * i * np.sqrt(n) * bars, (i, dev)
    assert blocks._callbacks == [] and len(callback._callbacks) == 2
    res = {}
    for name, h in (("blocks", blocks), ("whole", whole)):
        done, status, err, _ = h.step(steps + 1, 5000, 10, 1e-9)
        xs = np.clip(h.prox(1, h.get_iterate()), 0.0, 1.0)
        res[name] = (status, steps + done, nc.box_qp_residual(Q, q, 0.0, 1.0, xs))
    print("DR block box QP: worst deviation / bound %.2e; blocks %s, whole-vector %s" % (worst, res["blocks"], res["whole"]))
    # the existing box-QP test prints this residual and holds the status; here the whole-vector handle on the same problem, the same eps, sets the level
    assert res["blocks"][0] == "Optimal" and res["whole"][0] == "Optimal"
    assert res["blocks"][2] <= 10.0 * max(res["whole"][2], 1e-9)


def _affine_problem(pkg):
    nb, m, p, tail = 60, 3, 8, 21
    n = nb * p + tail
    rng = np.random.default_rng(4)
    As = [rng.standard_normal((m, p)) for _ in range(nb)]
    bs = [A @ np.maximum(rng.standard_normal(p), 0.0) for A in As]
    S = pkg.SeparableSum([(pkg.IndAffine(As[k], bs[k]), p) for k in range(nb)] + [(pkg.IndFree(), tail)], dense=True)
    A = np.hstack([scipy.linalg.block_diag(*As), np.zeros((nb * m, tail))])
    return S, As, bs, A, np.concatenate(bs), n, p


def test_block_affine_feasibility_under_gapa(pkg):
    S, As, bs, A, b, n, p = _affine_problem(pkg)
    out = {}
    for name, S1 in (("blocks", S), ("whole", pkg.IndAffine(A, b))):
        d = _handle(pkg, S1, n, pkg.IndBox(0.0, np.inf))
        d.set_alg(ALGS["GAPA"](pkg))
        d.set_iterate(None)
        done, status, err, _ = d.step(1, 20000, 10, 1e-8)
        out[name] = (status, done)
        if name == "blocks":
            sol, _, _ = d.getsol()
            y = d.prox(1, sol)
    print("GAPA on 60 IndAffine 3 x 8 blocks: %s; whole-vector IndAffine: %s" % (out["blocks"], out["whole"]))
    assert out["blocks"][0] == "Optimal" and out["blocks"] == out["whole"]
    worst = max(np.abs(As[k] @ y[k * p:(k + 1) * p] - bs[k]).max() for k in range(len(As)))
    assert worst <= ac.TOL * max(1.0, np.abs(sol).max()), worst
    print("|A sol - b| = %.2e at sol = P_S2(P_S1(x))" % np.abs(A @ sol - b).max())
    assert sol.min() >= 0.0


def test_wrappers_see_only_the_prox(pkg):
    S, _, _, _, _, n, _ = _affine_problem(pkg)
    d = _handle(pkg, S, n, pkg.IndBox(0.0, np.inf))
    d.set_alg(pkg.LineSearchWrapper(pkg.GAP(0.8, 1.5, 1.6), lsinterval=10))
    d.set_iterate(None)
    assert d.step(1, 30, 10 ** 9, 1e-30)[0] == 30
    it, normres, tests, alpha = d.linesearch_log()
    assert it == 30 and np.isfinite(normres) and np.all(np.isfinite(tests)) and np.isfinite(alpha)
    d.set_alg(pkg.GAPP(0.8, 1.5, 1.6, iproj=10))
    d.set_iterate(None)
    assert d.step(1, 30, 10 ** 9, 1e-30)[0] == 30
    it, tests, alpha = d.gapp_log()
    assert it == 30 and np.all(np.isfinite(tests)) and np.isfinite(alpha) and np.all(np.isfinite(d.get_iterate()))


def test_replacement_and_refusals_on_a_live_handle(pkg):
    c = pkg.lib.BLK_CODES
    q, af, ls = dc.block("Quadratic", 6), dc.block("IndAffine", 6, m=3), dc.block("LeastSquares", 6)
    n = 20
    S = pkg.SeparableSum([(pkg.IndFree(), 1), (q.device_set(pkg), 6), (af.device_set(pkg), 6), (ls.device_set(pkg), 6), (pkg.NormL1(0.1), 1)], dense=True)
    x = np.random.default_rng(1).standard_normal(n)
    d = _handle(pkg, S, n)
    first = d.prox(1, x)
    d.set_set(1, pkg.IndBox(-0.1, 0.1))
    assert np.array_equal(d.prox(1, x), np.clip(x, -0.1, 0.1))
    with pytest.raises(pkg.lib.FosError, match="dense"):
        d.dense_block_stats(1)                                                    # a box
    d.set_blocks(1, *pkg.SeparableSum([(pkg.IndFree(), n)]).pack(n))
    with pytest.raises(pkg.lib.FosError, match="dense"):
        d.dense_block_stats(1)                                                    # a sum without dense blocks
    d.set_blocks2(1, *S.pack2(n))
    assert d.prox(1, x).tobytes() == first.tobytes() and d.dense_block_stats(1)["dense_blocks"] == 3

    kinds, lens, scal = [0, c["Quadratic"], c["IndAffine"], c["LeastSquares"], 32], [1, 6, 6, 6, 1], [0.0, 0, 0, 0, 0, 0, 1.0, 0, 0.1, 0]
    mats, bm, bv = [q.M, af.M, ls.M], [-1, 0, 1, 2, -1], [None, q.v, af.v, ls.v, None]

    def call(kinds=kinds, lens=lens, scal=scal, mats=mats, rows=None, cols=None, bm=bm, bv=bv):
        rows = [M.shape[0] for M in mats] if rows is None else rows
        cols = [M.shape[1] for M in mats] if cols is None else cols
        return dc.set_blocks2_raw(pkg, d, 1, kinds, lens, scal, None, mats, rows, cols, bm, bv)
    assert call() == 0 and d.prox(1, x).tobytes() == first.tobytes()              # the raw call itself is sound

    def poke(M, i, j, v):
        M = np.array(M); M[i, j] = v
        return M
    dep = np.array(af.M); dep[2] = -3.0 * dep[1]
    lam_bad = lambda v: scal[:6] + [v] + scal[7:]
    refusals = [
        ("block 2", "not finite", dict(mats=[poke(q.M, 3, 1, np.nan), af.M, ls.M])),
        ("block 3", "not finite", dict(mats=[q.M, poke(af.M, 0, 0, np.inf), ls.M])),
        ("block 4", "not finite", dict(bv=[None, q.v, af.v, poke(ls.v[None, :], 0, 2, np.nan)[0], None])),
        ("block 2", "column 1 of I + Q", dict(mats=[poke(q.M, 0, 0, -2.0), af.M, ls.M])),
        ("block 3", "A needs full row rank", dict(mats=[q.M, dep, ls.M])),
        ("block 3", "m <= p", dict(mats=[q.M, np.ones((7, 6)), ls.M], bv=[None, q.v, np.ones(7), ls.v, None])),
        ("block 2", "Q is 6 x 6, the block has 5", dict(lens=[2, 5, 6, 6, 1])),
        ("block 4", "A has 6 columns, the block has 5", dict(lens=[2, 6, 6, 5, 1])),
        ("block 2", "Q is 5 x 6", dict(rows=[5, 3, 9])),
        ("block 4", "lambda", dict(scal=lam_bad(0.0))),
        ("block 4", "lambda", dict(scal=lam_bad(np.inf))),
        ("block 4", "lambda", dict(scal=lam_bad(np.nan))),
        ("block 3", "out of range", dict(bm=[-1, 0, 3, 2, -1])),
        ("block 2", "needs a matrix", dict(bm=[-1, -1, 1, 2, -1])),
        ("block 5", "takes no matrix", dict(bm=[-1, 0, 1, 2, 0])),
        ("block 1", "unknown kind", dict(kinds=[8] + kinds[1:])),
        ("block 5", "unknown kind", dict(kinds=kinds[:4] + [51])),
    ]
    for block, needle, kw in refusals:
        rc = call(**kw)
        msg = dc.last_error(pkg)
        assert rc == FOS_EINVAL and block in msg and needle in msg, (block, needle, rc, msg)
        assert d.prox(1, x).tobytes() == first.tobytes(), (block, needle)        # the set held before: the same bits
    # a block longer than 1024 names the whole-vector forms
    big = pkg.HipFeasibility(pkg.Feasibility(pkg.IndFree(), pkg.IndFree(), 1025))
    rc = dc.set_blocks2_raw(pkg, big, 1, [c["Quadratic"]], [1025], [0.0, 0.0], None, [np.zeros((1025, 1025))], [1025], [1025], [0], [None])
    assert rc == FOS_EINVAL and "block 1" in dc.last_error(pkg) and "whole-vector" in dc.last_error(pkg)
    # the entry without matrices does not know the dense kinds
    for code in c.values():
        with pytest.raises(pkg.lib.FosError, match="unknown kind"):
            d.set_blocks(1, np.array([0, code, 0], dtype=np.int32), np.array([1, 6, 13], dtype=np.int64), np.zeros(6), None)
        assert d.prox(1, x).tobytes() == first.tobytes()
    # nmat = 0 behaves as fos_feas_set_blocks
    assert dc.set_blocks2_raw(pkg, d, 1, [0, 32], [10, 10], [0, 0, 0.5, 0], None, [], [], [], [-1, -1], [None, None]) == 0
    assert np.array_equal(d.prox(1, x)[:10], x[:10]) and d.set_stats(1)["launches"] == 1
