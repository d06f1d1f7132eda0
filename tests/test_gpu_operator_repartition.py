"""fos_set_tuning(spmv_workgroups) on a window-panel operator: another number of persistent workgroups walks the same panels, so no row sum may
change by a bit -- the assertion test_gpu_edge_cases.py makes for re-partitioned tile operators, with its exception: the two tau rows are sums of
one partial record per workgroup, another grid adds the same products in another order, and they are held to rtol = 1e-13 (atol = 0) as there.
Strict bit identity of the tau rows does not hold on window panels (the grid the handle is built with and a grid of 8 differ in the last bits).

Shapes: "tiny", the smallest of status_cases.window_shapes() (every request ends at its few panels), and "wide", the one with far more panels
than 8 (a workgroup then walks several panels, and 7 against 8 is the multiple-of-8 edge of the set-up's own grid), under FOS_WINDOWS = 1 and 2;
and the row-sharded "mixed" rows problem of test_gpu_peer_mailbox.py on one rank without a transport, whose n rows of A' are deferred rows: the
consumers of a sweep's sums must go on reading the deferred-row kernel's records after a re-partitioning.
"""
import numpy as np
import pytest
import scipy.sparse as sp

import status_cases as cases

pytestmark = pytest.mark.gpu


def _handle(pkg, name):
    if name == "rows-mixed":
        import test_gpu_peer_mailbox as pm
        p = pm._rows_problem(pkg, "mixed")
        return pkg.HipHSDE(p.A, p.b, p.c, p.K1, p.K2, row_sharded=True)
    A = sp.csc_matrix(dict(cases.window_shapes())[name])
    m, n = A.shape
    b, c = cases.vectors_for(name, A)
    return pkg.HipHSDE(A, b, c, [("Free", m)], [("Free", n)])


@pytest.mark.parametrize("geom", ["1", "2"])
@pytest.mark.parametrize("name", ["tiny", "wide", "rows-mixed"])
def test_window_panel_operator_survives_repartitioning(pkg, monkeypatch, name, geom):
    monkeypatch.setenv("FOS_WINDOWS", geom)
    d = _handle(pkg, name)
    st = d.operator_stats()
    panels = st["win_panels"]
    assert panels > 0 and (st["deferred"] > 0) == (name == "rows-mixed")
    l, N = d.l, d.N
    rng = np.random.default_rng(cases._seed("repartition", name))
    x, z = rng.standard_normal(l), rng.standard_normal(N)

    def products():
        return d.q_apply(x), d.q_apply(x, transpose=True), d.kkt_apply(z)

    ref = products()
    for wg in (1, 7, 8, panels, 16384):
        d.set_tuning(spmv_workgroups=wg)
        got = products()
        for what, r, g, tau_rows in (("q", ref[0], got[0], [l - 1]), ("qt", ref[1], got[1], [l - 1]), ("kkt", ref[2], got[2], [l - 1, N - 1])):
            rows = np.ones(r.size, dtype=bool)
            rows[tau_rows] = False            # sums of per-workgroup partial sums: grouping may change the last bits
            rel = float(np.max(np.abs(g[~rows] - r[~rows]) / np.abs(r[~rows])))
            print("%s FOS_WINDOWS=%s %d panels, %5d workgroups, %-3s: rows differing %d, tau rows |difference| / |value| %.3g"
                  % (name, geom, panels, wg, what, int(np.count_nonzero(g[rows] != r[rows])), rel))
            assert np.array_equal(g[rows], r[rows]), (wg, what)
            assert np.allclose(g[~rows], r[~rows], rtol=1e-13, atol=0), (wg, what, rel)
    d.close()
