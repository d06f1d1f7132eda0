"""SHA-256 digests of the raw fp64 output of the cone projections, for comparing two builds of the library bit for bit (a change that is meant to leave
the cone kernels and their launches alone gives the same line).  Public Python API only, so the same file runs against any build:

    python tools/cone_digest.py                                   # the library of this tree
    FOSHIP_LIB=/path/to/other/libfoship.so python tools/cone_digest.py

One JSON line:
  hsde_all     fos_prox_cones four times in a row (slowly moving input) on a handle with every cone kind on both sides and SDP orders 2, 6, 64 and 65
  hsde_psd64   the same on 8 x PSD(64) only: the refinement kernel from the second call on
  feas_mixed   fos_feas_prox four times on a ConeProduct of every kind (SDP orders 6, 64 and 2)
  dr_steps     the iterate after 12 fos_step calls of DR on 8 x PSD(64) (c4_block_sdp), with fos_psd_fused_steps beside it.  The CG solves in the steps
               end on a host-observed stop, so this one may differ between two runs of ONE build; the fused-step count may not.
"""
import hashlib
import json
import sys

sys.path.insert(0, '.')
import numpy as np
import scipy.sparse as sp

import __graft_entry__ as ge

pkg = ge.load_package()

tri = lambda k: k * (k + 1) // 2
ALL_K1 = [("NonNeg", 7), ("SOC", 6), ("SDP", tri(6)), ("Free", 3), ("SOCRotated", 5), ("SDP", tri(64)), ("NonPos", 4), ("SOC", 1), ("SDP", tri(2)),
          ("ExpPrimal", 3), ("SDP", tri(65)), ("ExpDual", 3), ("Zero", 2)]
ALL_K2 = [("Free", 2), ("SOC", 4), ("NonNeg", 3), ("SDP", tri(6)), ("ExpPrimal", 3), ("Zero", 1)]
FEAS_MIXED = [("NonNeg", 7), ("SOC", 6), ("SDP", 21), ("Free", 3), ("SOCRotated", 5), ("SDP", 2080), ("NonPos", 4), ("SOC", 1), ("SDP", 3),
              ("ExpPrimal", 3), ("ExpDual", 3), ("Zero", 2)]


def digest(arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    return h.hexdigest()


def four_projections(project, size, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(size)
    outs = []
    for _ in range(4):
        outs.append(np.array(project(x), copy=True))
        x = x + 1e-3 * rng.standard_normal(size)
    return digest(outs)


def hsde_handle(K1, K2, seed):
    m, n = sum(l for _, l in K1), sum(l for _, l in K2)
    A = sp.random(m, n, density=0.02, format="csc", random_state=np.random.RandomState(seed))
    return pkg.HipHSDE(A, np.zeros(m), np.zeros(n), K1, K2)


out = {}
d = hsde_handle(ALL_K1, ALL_K2, 1)
out["hsde_all"] = four_projections(d.prox_cones, d.N, 31)
d.close()

prob = pkg.workloads.c4_block_sdp(nblocks=8, k=64, p=4)
d = pkg.HipHSDE(prob.A, prob.b, prob.c, prob.K1, prob.K2)
out["hsde_psd64"] = four_projections(d.prox_cones, d.N, 32)
d.close()

n = sum(l for _, l in FEAS_MIXED)
f = pkg.HipFeasibility(pkg.Feasibility(pkg.ConeProduct(FEAS_MIXED), pkg.IndBox(-np.inf, np.inf), n))
out["feas_mixed"] = four_projections(lambda x: f.prox(1, x), n, 33)
f.close()

d = pkg.HipHSDE(prob.A, prob.b, prob.c, prob.K1, prob.K2)
d.set_alg(pkg.DR())
d.set_iterate(None)
for i in range(1, 13):
    d.step(i, 1, 10 ** 12, 1e-12)
out["dr_steps"] = digest([d.get_iterate()])
out["dr_fused_steps"] = int(d.psd_fused_steps())
d.close()

print(json.dumps(out))
