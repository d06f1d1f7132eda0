"""The PSD projection kernels (csrc/psd.hip: psd_kernel in its 256-, 512- and 1024-thread forms, psd64_wave_kernel, psd64_refine_kernel; csrc/psd_sign.hip) on
every path launch_cones_psd picks, matrix by matrix against the long-double references of psd_cases.py (the tolerance and its derivation are there, the figures
in profiles/psd_edges_allowance.txt).  Every round fills each cone copy with another case -- a dual copy takes the next case of the list -- and checks every
matrix on its own, the Free(3) guard blocks between the cones, that the input is untouched, and the kernel's own record (fos_psd_stats): a matrix that
reports Jacobi sweeps converged before PSD_MAX_SWEEPS = 40 (an order-1 or an all-zero matrix runs no sweep and reports 0).

    pytest -m gpu -s tests/test_gpu_psd_edges.py     prints worst error / tolerance per kernel path and order
"""
import numpy as np
import pytest
import scipy.sparse as sp

import psd_cases as pc

pytestmark = pytest.mark.gpu

VARIANTS = {                                   # what is set before fos_create, and the kernel it selects (launch_cones_psd)
    "default": ({}, "psd_kernel<true,true,512>"),
    "narrow": ({"FOS_PSD_NARROW": "1"}, "psd_kernel<true,true,256>"),
    "threads1024": ({"FOS_PSD_THREADS": "1024"}, "psd_kernel<true,true,1024>"),
    "wave": ({"FOS_PSD_WAVE": "1", "FOS_PSD_REFINE": "0"}, "psd64_wave_kernel"),
    "workgroup": ({"FOS_PSD_WAVE": "0", "FOS_PSD_REFINE": "0"}, "psd_kernel<true,true,256>, all 64"),
    "refine": ({"FOS_PSD_WAVE": "0", "FOS_PSD_REFINE": "1"}, "psd64_refine_kernel"),
}


def device_cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


class Handle:
    def __init__(self, pkg, monkeypatch, name, variant="default"):
        for key in ("FOS_PSD_NARROW", "FOS_PSD_WIDE", "FOS_PSD_THREADS", "FOS_PSD_WAVE", "FOS_PSD_REFINE", "FOS_PSD_COLD", "FOS_PSD_SIGN_MIN"):
            monkeypatch.delenv(key, raising=False)
        for key, val in VARIANTS[variant][0].items():
            monkeypatch.setenv(key, val)
        self.name, self.variant, self.path = name, variant, VARIANTS[variant][1]
        self.cus = device_cus()
        if name == "feas":
            self.layout = pc.Layout(pc.handle_cones("mixed")[0])
            self.dev = pkg.HipFeasibility(pkg.Feasibility(pkg.ConeProduct(self.layout.K1), pkg.IndFree(), self.layout.m))
            self.project = lambda z: self.dev.prox(1, z)
            self.records = None
            self.path = "Feasibility ConeProduct (the kernel launch_cones_psd picks)"
        else:
            self.layout = pc.Layout(*pc.handle_cones(name, self.cus))
            m, n = self.layout.m, self.layout.n
            rng = np.random.default_rng(41)
            A = sp.random(m, n, density=min(1.0, 40.0 / m), format="csc", random_state=rng, data_rvs=rng.standard_normal)
            self.dev = pkg.HipHSDE(A, rng.standard_normal(m), rng.standard_normal(n), self.layout.K1, self.layout.K2)
            assert self.dev.N == self.layout.N
            self.project = self.dev.prox_cones
            self.dev.psd_debug(True, 0)
            self.records = self.dev.psd_sweeps
        self.worst, self.sweeps = {}, {}

    def close(self):
        self.dev.close()

    def run(self, z, used, scale=0, label=None):
        """one projection: input untouched, guards, every matrix on its own against its reference, the records.  -> y"""
        lay = self.layout
        z0 = z.copy()
        y = self.project(z)
        assert np.array_equal(z, z0, equal_nan=True), (self.name, "the input was written to")
        lay.check_guards(z, y, self.name)
        rec = self.records() if self.records else None
        if rec is not None:
            assert len(rec) == 2 * len({s.cone for s in lay.sdp if s.k <= 64})
        for slot, case in used:
            r = int(rec[lay.record_index(slot)]) if rec is not None and slot.k <= 64 else None
            refined = r is not None and r >= 100
            what = "%s/%s %s copy at %d, record %s" % (self.name, self.variant, "dual" if slot.dual else "primal", slot.at, r)
            ratio = case.check(y[slot.at:slot.at + slot.length], dual=slot.dual, refined=refined, scale=scale, what=what, exact=slot.k <= 64)
            if r is not None and not refined:
                if slot.k >= 2 and case.norm > 0.0:
                    assert 0 < r < 40, (what, case.label(), "Jacobi sweeps")
                else:
                    assert r == 0, (what, case.label(), "a matrix without a sweep to run")
            if slot.k > 64:
                path = "psd_sign, padded order %d" % ((slot.k + 63) // 64 * 64)
            elif self.variant == "refine":
                path = self.path + (": extrapolated basis accepted" if r >= 1100 else ": previous basis accepted" if refined else ": Jacobi (cold / handed back)")
            else:
                path = self.path
            key = (path + (", " + label if label else ""), slot.k)
            self.worst[key] = max(self.worst.get(key, 0.0), ratio)
            if r is not None and not refined:
                self.sweeps[key] = max(self.sweeps.get(key, 0), r)
        return y

    def idempotent(self, y, used):
        """P(P(x)) within the tolerance of P(x), matrix by matrix"""
        y2 = self.project(y)
        self.layout.check_guards(y, y2, self.name)
        rec = self.records() if self.records else None
        for slot, case in used:
            seg = slice(slot.at, slot.at + slot.length)
            refined = rec is not None and slot.k <= 64 and rec[self.layout.record_index(slot)] >= 100
            err = float(np.abs(y2[seg] - y[seg]).max())
            assert err <= case.tol(refined), (self.name, self.variant, case.label(), "P(P(x)) - P(x)", err, case.tol(refined))

    def report(self):
        print("\nhandle %s (%s): worst error / tolerance per path and order; most Jacobi sweeps" % (self.name, self.variant))
        for (path, k) in sorted(self.worst):
            print("  %-58s order %3d   %.4f   %s" % (path, k, self.worst[(path, k)], self.sweeps.get((path, k), "")))
        assert all(r <= 1.0 for r in self.worst.values())


@pytest.fixture
def make(pkg, monkeypatch):
    made = []

    def build(name, variant="default"):
        made.append(Handle(pkg, monkeypatch, name, variant))
        return made[-1]
    yield build
    for h in made:
        h.close()


def every_case_rounds(h):
    """round 1 cold inside the warm kernel, round 2 the same matrices (warm), round 3 unrelated ones (the basis comes from another matrix), then every
    case of the list on both copies of every cone -- the same tolerance throughout: accuracy does not depend on the start"""
    lay = h.layout
    z, used = lay.fill(0)
    y = h.run(z, used)
    h.run(z, used)
    h.idempotent(y, used)
    h.run(*lay.fill(0, seed=7))
    for rnd in range(1, len(pc.NAMES)):
        z, used = lay.fill(rnd)
        y = h.run(z, used)
    h.idempotent(y, used)


@pytest.mark.parametrize("variant", ["default", "narrow", "threads1024"])
def test_mixed_orders_in_one_batch(make, variant):
    """orders 1 .. 64 in K1 and 5, 64 in K2 in ONE launch: per-cone k, ld, tpp and the basis stride kmax^2; the order-64 members run jacobi64_regs<8>
    with the eight-wavefront MFMA products (512 threads), jacobi64_regs<4> (256) and jacobi64<1024, 32> (1024)"""
    h = make("mixed", variant)
    assert len({s.cone for s in h.layout.sdp}) <= h.cus              # (few enough cones for the wide form)
    every_case_rounds(h)
    h.report()


def test_more_cones_than_compute_units(make):
    """cus + 3 cones of orders 1 .. 9 and one of order 64: the 256-thread form by count alone"""
    h = make("many")
    assert len({s.cone for s in h.layout.sdp}) == h.cus + 4 > h.cus
    h.path = "psd_kernel<true,true,256> by count (%d cones, %d CUs)" % (h.cus + 4, h.cus)
    lay = h.layout
    z, used = lay.fill(0)
    y = h.run(z, used)
    h.run(z, used)
    h.idempotent(y, used)
    h.run(*lay.fill(0, seed=7))
    for rnd in (5, 10):
        h.run(*lay.fill(rnd))
    h.report()


@pytest.mark.parametrize("variant", ["wave", "workgroup"])
def test_order_64_jacobi_kernels(make, variant):
    h = make("all64", variant)
    every_case_rounds(h)
    h.report()


def test_order_64_refinement(make):
    """the sequence of test_psd_refinement_path -- cold, steady drift, no change, a jump -- and the record says which state each matrix was in: Jacobi
    (cold, or handed back after a jump), accepted from the previous basis, accepted from the extrapolated basis; the per-matrix tolerance (with the
    refinement's own term for an accepted matrix) holds in all three"""
    h = make("all64", "refine")
    lay = h.layout

    def drift(t):
        z = np.random.default_rng([36, t]).standard_normal(lay.N)
        used = [(s, pc.drift_case(64, 2 * s.cone + (1 if s.dual else 0), t)) for s in lay.sdp]
        for s, case in used:
            z[s.at:s.at + s.length] = case.x
        return z, used

    seen = {"jacobi": 0, "accepted": 0, "extrapolated": 0, "handed back": 0}

    def count(after_warm):
        rec = h.records()
        seen["jacobi"] += int((rec < 100).sum())
        seen["accepted"] += int(((rec >= 100) & (rec < 1100)).sum())
        seen["extrapolated"] += int((rec >= 1100).sum())
        if after_warm:
            seen["handed back"] += int((rec < 100).sum())

    h.run(*drift(0)); count(False)                                    # cold
    assert seen["jacobi"] == 2 * 4
    for t in range(1, 5):                                             # steady drift
        z, used = drift(t)
        y = h.run(z, used); count(False)
    h.run(z, used); count(False)                                      # no change
    h.idempotent(y, used)
    h.run(*lay.fill(0)); count(True)                                  # a jump: unrelated matrices
    every_case_rounds(h)
    print("\nrefinement records over the drift sequence:", seen)
    assert seen["accepted"] > 0 and seen["extrapolated"] > 0 and seen["handed back"] > 0, seen
    h.report()
    assert len({p for p, _ in h.worst}) == 3


def test_sign_iteration_orders(make):
    """orders 65, 128, 129, 200 (padded 128, 128, 192, 256) beside a 5 and a 64 in one handle; one round with the order-129 matrix scaled by 1e6 and the
    order-5 matrix by 1e-6"""
    h = make("sign")
    lay = h.layout
    every_case_rounds(h)
    z, used = lay.fill(3)
    scaled = []
    for s, case in used:
        f = {129: 1e6, 5: 1e-6}.get(s.k)
        if f is not None:
            key = ("scaled", s.k, case.name, f)
            if key not in pc.Case._cache:
                c2 = pc.Case.get(s.k, case.name)
                c3 = object.__new__(pc.Case)
                c3.__dict__.update(c2.__dict__)
                c3.x = c2.x * f                                        # rounded once more: within the reference term of the tolerance (0.5 U)
                c3.p_ref = c2.p_ref * pc.LD(f)
                c3.norm, c3.unresolved, c3.name = c2.norm * f, c2.unresolved * f, c2.name + " x %g" % f
                pc.Case._cache[key] = c3
            case = pc.Case._cache[key]
            z[s.at:s.at + s.length] = case.x
        scaled.append((s, case))
    h.run(z, scaled, label="mixed scales 1e6 / 1e-6")
    h.report()
    assert {65, 128, 129, 200} <= {k for _, k in h.worst}


def test_feasibility_cone_product(make):
    """the same kernels through feas_objects.hip: primal copies only"""
    h = make("feas")
    every_case_rounds(h)
    h.report()


@pytest.mark.parametrize("name", ["mixed", "sign"])
def test_homogeneity(make, name):
    """P(2^s x) = 2^s P(x) at s = +-100, +-400 (the squares stay normal numbers): against the base reference scaled exactly, same tolerance"""
    h = make(name)
    for base in pc.HOMOGENEITY_BASE:
        for s in [0] + pc.HOMOGENEITY_SCALES:
            z, used = h.layout.fill(0, scale=s, names=[base])
            h.run(z, used, scale=s, label="scaled by 2^%+d" % s)
    h.report()


@pytest.mark.parametrize("name,variant", [("mixed", "default"), ("sign", "default"), ("all64", "refine")])
def test_nan_and_inf_stay_in_their_cone(make, name, variant):
    """a NaN in one matrix and an Inf in another: the call returns, and every other cone and every guard block has the bits of the same round without
    them (two handles with the same history: the kernels are deterministic).  Nothing is asked of the poisoned matrices themselves."""
    clean, dirty = make(name, variant), make(name, variant)
    lay = clean.layout
    z0, used0 = lay.fill(0)
    for h in (clean, dirty):
        h.run(z0, used0)
    z, used = lay.fill(2)
    zp = z.copy()
    cones = sorted({s.cone for s in lay.sdp})
    nan_at = {"mixed": 4, "sign": 2, "all64": 2}[name]                 # (orders 3, 128 -- batched with the order-65 cone -- and 64)
    hit = {cones[nan_at]: np.nan, cones[-1]: np.inf}                   # both copies of two cones; the Inf in the last cone (order 64, 200, 64)
    for s in lay.sdp:
        if s.cone in hit:
            zp[s.at + s.length // 2] = hit[s.cone]
    y = clean.run(z, used)
    yp = dirty.project(zp)
    lay.check_guards(zp, yp, name)
    for s in lay.sdp:
        if s.cone not in hit:
            seg = slice(s.at, s.at + s.length)
            assert np.array_equal(yp[seg], y[seg]), (name, "cone at %d changed beside a NaN / Inf" % s.at)
