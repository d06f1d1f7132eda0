"""
The one-launch step (relaxation + PSD(64) projection + final pass: psd64_refine_kernel with PsdFuse::on, step_once in step.cpp) at small
shapes and on every path it has, each step checked against its own definition (tests/step_identity.py: the iterate before, the affine
projection and the iterate after, reference cone projection by LAPACK).  fos_psd_fused_steps says whether a step took the fused launch,
the kernel's per-matrix record (fos_psd_stats) which path each matrix took:

    < 100            Jacobi sweeps: the in-place fallback (or the cold first projection)
    100 ... 1099     accepted from the previous basis      (+ 16 per rotation, + iterations)
    >= 1100          accepted from the extrapolated basis

Problems: `one` (two matrices, l = 2084: below the tail workgroups' 16 x 256 entries, no multiple of 256), `mixed` (every elementwise cone
on both sides, between and behind three PSD cones), `wps2` (CUs / 2 + 2 blocks: the smallest batch that takes psd64_refine_kernel<2>).
"""
import numpy as np
import pytest

import fos_oracle as orc
import step_identity as si

pytestmark = pytest.mark.gpu

BIG = 10 ** 12
EPS_STATUS = 1e-12
ALGS = {"DR": (0.5, 2.0, 2.0), "GAP": (0.3, 1.2, 1.7), "AP": (1.0, 1.0, 1.0)}
CHECKED_STEPS = (16, 32)                       # sequence (a): steps taken WITH a status check (they cannot be fused)


def _make_alg(pkg, name):
    return {"DR": pkg.DR(), "GAP": pkg.GAP(0.3, 1.2, 1.7), "AP": pkg.AP()}[name]


@pytest.fixture(scope="module")
def problems(pkg):
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    out = {"one": si.one_problem(pkg.workloads), "mixed": si.mixed_problem(pkg.workloads),
           "wps2": pkg.workloads.c4_block_sdp(nblocks=cus // 2 + 2, k=64, p=4)}
    assert 2 * len(out["wps2"].K1) > cus       # two workgroups per CU: psd64_refine_kernel<2>
    assert 2 * len(out["mixed"].K1) <= cus
    return {k: (p, si.StepIdentity(p.A, p.b, p.c, p.K1, p.K2)) for k, p in out.items()}


@pytest.fixture(scope="module")
def oracle_direct(problems):
    """the oracle's exact affine projection (a dense Cholesky factor), built once per problem and shared"""
    made = {}

    def get(name):
        if name not in made:
            alg = orc.GAP(direct=True)
            alg.init(si.oracle_model(problems[name][0]))
            made[name] = alg
        return made[name]
    return get


def classify(rec):
    """per matrix: 'fallback' | 'accept' | 'extrapolated', and whether columns were rotated"""
    rec = np.asarray(rec)
    kind = np.where(rec < 100, "fallback", np.where(rec >= 1100, "extrapolated", "accept"))
    rot = (rec >= 100) & (((rec % 1000) - 100) // 16 >= 1)
    return kind, rot


class Driver:
    """a handle, the checker of its problem and what the steps showed"""

    def __init__(self, pkg, prob, chk, algname, direct, label):
        self.d = pkg.HipHSDE(prob.A, prob.b, prob.c, prob.K1, prob.K2)
        self.prob, self.chk, self.params, self.direct, self.label = prob, chk, ALGS[algname], direct, label
        self.d.set_alg(_make_alg(pkg, algname))
        if direct:
            self.d.enable_direct(prob.A)
            assert self.d.direct_mode() in ("dense", "block", "reduced")       # an exact projection: the fused kernel writes no shift
        self.d.set_iterate(None)
        self.d.psd_debug(True, 0)
        self.seen = {"fallback": [], "accept": [], "extrapolated": [], "rotations": []}       # under the fused launch: (sequence, step)
        self.prev_rec = None                                                                  # the records of the step before (single steps only)

    def close(self):
        self.d.close()

    def step(self, i, seq, checki=BIG):
        """one step through the checker; returns (records, rise of the fused counter)"""
        d = self.d
        x = d.get_iterate()
        pi = d.get_affine_state()[1]
        f0 = d.psd_fused_steps()
        done, checked, _ = d.step(i, 1, checki, EPS_STATUS)
        assert done == 1 and checked == (i % checki == 0)
        xp = d.get_iterate()
        sol = d.get_affine_state()[0]
        rec = d.psd_sweeps().copy()
        rise = d.psd_fused_steps() - f0
        alpha, a1, a2 = self.params
        res = self.chk.check(x, sol, xp, alpha, a1, a2, None if self.direct else pi)
        kind, rot = classify(rec)
        if self.prev_rec is not None:
            # a matrix that fell back leaves record 1 behind: its next projection starts from the Jacobi basis, never from an extrapolated one
            # (it may be accepted from that basis or fall back again; the step after THAT acceptance may extrapolate: two continuation bases exist)
            after = rec[self.prev_rec < 100]
            assert (after < 1100).all(), (self.label, seq, i, "extrapolated right after a fallback", after)
        self.prev_rec = rec
        print("%s %s step %d: fused %d, records min %d max %d, CG %d; %s" % (self.label, seq, i, rise, rec.min(), rec.max(), d.cgiter(), res))
        assert res.ew_ok, (self.label, seq, i, "elementwise / (tau, kappa) entries", res.ew_worst())
        assert res.psd_ok, (self.label, seq, i, "PSD entries", res.psd_dev, res.psd_bound)
        assert res.affine_ok, (self.label, seq, i, "affine projection", res.affine_res, res.affine_bound)
        if rise:
            for k in ("fallback", "accept", "extrapolated"):
                if (kind == k).any():
                    self.seen[k].append((seq, i))
            if rot.any():
                self.seen["rotations"].append((seq, i))
        return rec, rise


def _unit(rng, n):
    v = rng.standard_normal(n)
    return v / np.linalg.norm(v)


def _sequences(drv, rng, single_to, resume_at, drift_to, recover=12, settle=3):
    """(a) steps 1 .. single_to one at a time [then one multi-step call up to resume_at - 1], (b) steady drift to drift_to, (c) a jump,
    (d) smaller jumps.  Returns the next step index."""
    d = drv.d
    # ---- (a)
    first_fused = None
    for i in range(1, single_to + 1):
        checki = i if i in CHECKED_STEPS else BIG
        rec, rise = drv.step(i, "a", checki)
        if i == 1:
            assert rise == 0 and (rec < 100).all() and (rec > 0).all(), rec         # the cold projection: Jacobi, not fused (no basis yet)
        if checki != BIG:
            assert rise == 0, (drv.label, i, "a step with a status check went through the fused launch")
        elif first_fused is not None:
            assert rise == 1, (drv.label, i, rise)
        elif rise:
            assert rise == 1
            first_fused = i
    assert first_fused == 2, first_fused                                          # one projection leaves a basis: the second step is the first fused one
    i = single_to + 1
    if resume_at > i:
        f0 = d.psd_fused_steps()
        done, _, _ = d.step(i, resume_at - i, BIG, EPS_STATUS)
        assert done == resume_at - i and d.psd_fused_steps() - f0 == done
        i = resume_at
        drv.prev_rec = None
    # ---- (b)
    all_extrapolated = False
    while i <= drift_to:
        rec, rise = drv.step(i, "b", BIG)
        assert rise == 1
        all_extrapolated |= bool((rec >= 1100).all())
        i += 1
    assert all_extrapolated, "no step of the steady drift had every matrix accepted from the extrapolated basis"
    # ---- (c) a jump: a fresh random vector of the same norm; the bases stay
    x = d.get_iterate()
    d.set_iterate(np.linalg.norm(x) * _unit(rng, x.size))
    rec, rise = drv.step(i, "c", BIG)
    i += 1
    assert rise == 1
    fell = rec < 100
    assert fell.any(), rec                                                        # the in-place Jacobi fallback inside the fused launch
    # The steps behind the jump go through the checker like every other, and Driver.step holds them to "no extrapolation right after a fallback".
    # A matrix may fall back AGAIN there, for several steps -- the iterate still moves by a large fraction of ||x|| per step and the refinement
    # has seven iterations and twelve rotations: on `one`, DR, the step behind the jump gave Jacobi records (9, 9) once more; on `wps2`,
    # GAP(0.3, 1.2, 1.7), 258 of 260 matrices were accepted again six to eight steps behind the jump and two were still Jacobi's after thirteen.
    # So: at least two more steps, then on until every matrix that fell back has been accepted again (`recover` steps at the most); the first
    # acceptance of each is from the previous basis (100 <= record < 1100), and at least one matrix gets there.
    pending, taken = fell.copy(), 0
    for n in range(recover):
        if n >= 2 and not pending.any():
            break
        rec, rise = drv.step(i, "c+", BIG)
        i += 1
        taken += 1
        assert rise == 1
        now = pending & (rec >= 100)
        assert (rec[now] < 1100).all(), (drv.label, rec[now])
        pending &= ~now
    assert (fell & ~pending).any(), (drv.label, "no matrix that fell back was accepted again", recover, rec[pending])
    print("%s (c) %d of %d matrices fell back at the jump; %d still not accepted again %d steps later" % (drv.label, fell.sum(), fell.size, pending.sum(), taken))
    # ---- (d) smaller jumps
    for k in (6, 4, 3, 2):
        for _ in range(settle):                                                   # (the drift is steady again)
            drv.step(i, "d-settle", BIG)
            i += 1
        x = d.get_iterate()
        d.set_iterate(x + 10.0 ** -k * np.linalg.norm(x) * _unit(rng, x.size))
        rec, rise = drv.step(i, "d", BIG)
        i += 1
        assert rise == 1
        kind, rot = classify(rec)
        print("%s (d) perturbation 1e-%d: extrapolated %d, accepted from the previous basis %d, fallback %d, with rotations %d"
              % (drv.label, k, (kind == "extrapolated").sum(), (kind == "accept").sum(), (kind == "fallback").sum(), rot.sum()))
    print("%s paths seen under the fused launch: %s" % (drv.label, {k: len(v) for k, v in drv.seen.items()}))
    if drv.seen["rotations"]:
        print("%s rotations inside a fused step at %s" % (drv.label, drv.seen["rotations"]))
    return i


def _whole_step_vs_oracle(drv, oalg, i):
    """direct = true on both sides: the state handed over, one step each, relative 1e-9 (as the full-size same-step tests)"""
    d = drv.d
    z = d.get_iterate()
    oalg.alpha, oalg.alpha1, oalg.alpha2 = drv.params
    st = orc.NoStatus()
    xo = z.copy()
    oalg.step(xo, i, st)
    _, rise = drv.step(i, "oracle-step", BIG)
    assert rise == 1
    zg = d.get_iterate()
    dev = float(np.linalg.norm(zg - xo) / max(1.0, np.linalg.norm(xo)))
    print("%s whole step against the oracle (direct): rel. dev. %.2e" % (drv.label, dev))
    assert dev <= 1e-9, dev
    assert np.linalg.norm(zg - z) > 1e3 * 1e-9 * max(1.0, np.linalg.norm(z))      # (the step moved the iterate)


@pytest.mark.parametrize("direct", [False, True], ids=["cg", "direct"])
@pytest.mark.parametrize("algname", ["DR", "GAP", "AP"])
@pytest.mark.parametrize("pname", ["one", "mixed"])
def test_fused_step_paths(pkg, problems, oracle_direct, pname, algname, direct):
    """sequences (a)-(d) at one workgroup per CU"""
    prob, chk = problems[pname]
    drv = Driver(pkg, prob, chk, algname, direct, "%s/%s/%s" % (pname, algname, "direct" if direct else "cg"))
    try:
        rng = np.random.default_rng([21, len(pname), len(algname), int(direct)])
        i = _sequences(drv, rng, 40, 41, 60)
        if direct:
            _whole_step_vs_oracle(drv, oracle_direct(pname), i)
        if pname == "mixed":
            for k in ("extrapolated", "accept", "fallback"):
                assert drv.seen[k], (drv.label, "never seen under the fused launch", k)
    finally:
        drv.close()


@pytest.mark.parametrize("algname", ["DR", "GAP"])
def test_fused_step_paths_two_workgroups_per_cu(pkg, problems, algname):
    """sequences (a)-(d) at more matrices than CUs (psd64_refine_kernel<2>: the rotation path borrows M's LDS array): steps 1-12 singly, then
    on from step 200"""
    prob, chk = problems["wps2"]
    drv = Driver(pkg, prob, chk, algname, False, "wps2/%s/cg" % algname)
    try:
        rng = np.random.default_rng([22, len(algname)])
        _sequences(drv, rng, 12, 200, 203, recover=8, settle=1)
        for k in ("extrapolated", "accept", "fallback"):
            assert drv.seen[k], (drv.label, "never seen under the fused launch", k)
    finally:
        drv.close()


def test_no_extrapolation_when_switched_off(pkg, problems, monkeypatch):
    """(e) FOS_PSD_EXTRAPOLATE=0 at fos_create: fused steps all the same, every start from the previous basis"""
    monkeypatch.setenv("FOS_PSD_EXTRAPOLATE", "0")
    prob, chk = problems["mixed"]
    drv = Driver(pkg, prob, chk, "DR", False, "mixed/DR/no-extrapolation")
    monkeypatch.delenv("FOS_PSD_EXTRAPOLATE")
    try:
        for i in range(1, 21):
            rec, rise = drv.step(i, "e", BIG)
            assert rise == (1 if i >= 2 else 0)
            assert (rec < 1100).all(), (i, rec)
        assert drv.seen["accept"]
    finally:
        drv.close()


@pytest.mark.parametrize("relax_ew", ["1", "0"], ids=["relax-ew", "plain-relax"])
@pytest.mark.parametrize("algname", ["DR", "GAP"])
def test_checker_on_the_unfused_path(pkg, problems, monkeypatch, algname, relax_ew):
    """(g) FOS_PSD_FUSE=0 at fos_create: the counter stays 0 and the same bounds hold for relax_ew_kernel (FOS_RELAX_EW=0: the plain
    relaxation and the elementwise kernel), the PSD projection and gap_final_kernel as separate launches"""
    monkeypatch.setenv("FOS_PSD_FUSE", "0")
    monkeypatch.setenv("FOS_RELAX_EW", relax_ew)
    prob, chk = problems["mixed"]
    drv = Driver(pkg, prob, chk, algname, False, "mixed/%s/unfused/relax_ew=%s" % (algname, relax_ew))
    monkeypatch.delenv("FOS_PSD_FUSE")
    monkeypatch.delenv("FOS_RELAX_EW")
    try:
        for i in range(1, 21):
            rec, rise = drv.step(i, "g", BIG)
            assert rise == 0
        assert drv.d.psd_fused_steps() == 0
    finally:
        drv.close()
    # the switches are per handle: a handle created now, in the same process, fuses again
    drv = Driver(pkg, prob, chk, algname, False, "mixed/%s/fused-again" % algname)
    try:
        for i in range(1, 4):
            drv.step(i, "g'", BIG)
        assert drv.d.psd_fused_steps() == 2
    finally:
        drv.close()


@pytest.mark.parametrize("at_floor", [False, True], ids=["small-counter", "tolerance-floor"])
@pytest.mark.parametrize("algname", ["DR", "GAP"])
@pytest.mark.parametrize("pname", ["one", "mixed"])
def test_fused_shift_feeds_the_next_cg_start(pkg, problems, pname, algname, at_floor):
    """(f) two handles with the same history take the same two iterations: one in ONE fos_step call -- the second CG solve starts from the shift
    the fused kernel wrote -- the other in two calls (fos_step clears shift_ready: the start comes from shift_part2_kernel).  Both solve the same
    system to tol_{i+1} and ||M^-1|| <= 1:  ||dx+|| <= |alpha a1| (|alpha2| + |1 - alpha2|) 2 tol_{i+1} + the PSD term of the checker."""
    prob, chk = problems[pname]
    alpha, a1, a2 = ALGS[algname]
    runs = [Driver(pkg, prob, chk, algname, False, "%s/%s/shift-%s" % (pname, algname, w)) for w in ("one-call", "two-calls")]
    try:
        warm = 5
        for drv in runs:
            done, _, _ = drv.d.step(1, warm, BIG, EPS_STATUS)
            assert done == warm
        assert np.array_equal(runs[0].d.get_iterate(), runs[1].d.get_iterate())           # the same history, to the bit
        if at_floor:
            for drv in runs:
                drv.d.set_affine_state(drv.d.get_affine_state()[0], 400)
        i = warm + 1
        pi = runs[0].d.get_affine_state()[1]
        assert pi == (400 if at_floor else i)
        f0 = runs[0].d.psd_fused_steps()
        done, _, _ = runs[0].d.step(i, 2, BIG, EPS_STATUS)
        assert done == 2 and runs[0].d.psd_fused_steps() - f0 == 2
        _, r1 = runs[1].step(i, "f", BIG)
        x_mid, sol_mid = runs[1].d.get_iterate(), None
        _, r2 = runs[1].step(i + 1, "f", BIG)
        assert r1 == 1 and r2 == 1
        xa, xb = runs[0].d.get_iterate(), runs[1].d.get_iterate()
        sol_mid = runs[1].d.get_affine_state()[0]
        tol = chk.tolerance(pi + 1)
        t1 = a1 * sol_mid + (1 - a1) * x_mid
        psd_term = chk.psd_bound(t1, chk.entry_bound(x_mid, sol_mid, alpha, a1, a2), alpha, a2)
        bound = abs(alpha * a1) * (abs(a2) + abs(1 - a2)) * 2 * tol + psd_term
        diff = float(np.linalg.norm(xa - xb))
        print("%s/%s shift pair at call counter %d: bit-identical %s, ||dx+|| %.3e (bound %.3e, tol %.3e)"
              % (pname, algname, pi, np.array_equal(xa, xb), diff, bound, tol))
        assert diff <= bound, (diff, bound)
        assert np.linalg.norm(xb - x_mid) > 1e3 * bound or not at_floor                  # (at the floor a wrong shift is O(||x||) against the bound)
    finally:
        for drv in runs:
            drv.close()
