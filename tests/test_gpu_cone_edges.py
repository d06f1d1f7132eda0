"""cones_soc_kernel and cones_exp_kernel (csrc/vecops.hip) at their edges, element by element against the certified extended-precision references of
tests/golden/cone_edges.npz (cone_cases.py; tolerances and classes are explained there, the figures are in profiles/cone_edges_allowance.txt).

Four handles.  HSDE A: every SOC and rotated SOC length between Free(3) guard blocks, 21 cones for the SOC kernel (four to a workgroup: one past a multiple)
and 33 for the Exp kernel (32 to a workgroup: one past a multiple).  HSDE B: 20 and 32, on the multiples.  HSDE C: one SOCRotated(2), a one-cone launch with
no tail.  A Feasibility handle whose set is the ConeProduct of A's K1 list: the same kernels through feas_objects.hip, primal copies only.  Every round
fills each cone copy with another input; a dual copy takes the next input of the list, so the two parts of a cone never hold the same numbers.

    pytest -m gpu -s tests/test_gpu_cone_edges.py     prints worst error / tolerance per kind and length
"""
import numpy as np
import pytest
import scipy.sparse as sp

import cone_cases as cc
import fos_oracle as orc

pytestmark = pytest.mark.gpu


def _codes(cones):
    return [(orc.CONE_CODES[k], l) for k, l in cones]


class Handle:
    def __init__(self, pkg, name):
        self.name = name
        if name == "feas":
            self.layout = cc.Layout(cc.HANDLES["A"][0])
            self.dev = pkg.HipFeasibility(pkg.Feasibility(pkg.ConeProduct(self.layout.K1), pkg.IndFree(), self.layout.m))
            self.project = lambda z: self.dev.prox(1, z)
        else:
            self.layout = cc.Layout(*cc.HANDLES[name])
            m, n = self.layout.m, self.layout.n
            rng = np.random.default_rng(23)
            A = sp.random(m, n, density=min(1.0, 40.0 / m), format="csc", random_state=rng, data_rvs=rng.standard_normal)
            self.dev = pkg.HipHSDE(A, rng.standard_normal(m), rng.standard_normal(n), self.layout.K1, self.layout.K2)
            assert self.dev.N == self.layout.N
            self.project = self.dev.prox_cones


@pytest.fixture(scope="module")
def handles(pkg):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Handle(pkg, name)
        return made[name]
    yield get
    for h in made.values():
        h.dev.close()


_oracle_cache = {}


def oracle_slot(slot, case):
    """the oracle's restatement of this copy: prox! or proxDual! (x + P(-x)) of the slot's cone -- the arithmetic path the kernel takes"""
    key = (slot.kind, slot.dual, id(case))
    if key not in _oracle_cache:
        y = np.empty_like(case.x)
        with np.errstate(invalid="ignore"):                               # (inf - inf in the Inf cases)
            (orc.cone_prox_dual if slot.dual else orc.cone_prox)(orc.CONE_CODES[slot.kind], y, case.x)
        _oracle_cache[key] = y
    return _oracle_cache[key]


def check_round(h, z, y, used, worst):
    h.layout.check_guards(z, y, h.name)
    for slot, case in used:
        got = y[slot.at:slot.at + slot.length]
        what = "%s %s copy at %d" % (h.name, "dual" if slot.dual else "primal", slot.at)
        if slot.kind in cc.KINDS:
            if case.finite:
                key, r = "%-11s %5d" % (slot.kind, slot.length), case.check(got, what=what, dual=slot.dual)
            else:
                case.check_pattern(got, oracle_slot(slot, case), what=what)
                continue
        else:
            key, r = "Exp %s" % case.cls, case.check(got, oracle_slot(slot, case), what=what)
        worst[key] = max(worst.get(key, 0.0), r)


def report(title, worst):
    print("\n%s: worst error / tolerance" % title)
    for key in sorted(worst):
        print("  %-20s %.3f" % (key, worst[key]))


@pytest.mark.parametrize("name", ["A", "B", "feas"])
def test_every_case_on_every_copy(handles, name):
    """per element against the certified references on the primal and the dual copy of every cone (for a self-dual cone the dual copy's reference is the
    exact P(x); the kernel reaches it as x + P(-x)); bit identities; the NaN / Inf patterns of the oracle; guard blocks untouched; the same bits twice"""
    h = handles(name)
    lay, worst = h.layout, {}
    exp_rounds = max(-(-len(cc.exp_triples(op)) // max(1, sum(1 for s in lay.slots if getattr(s, "op", None) == op))) for op in "PD")
    for rnd in range(lay.rounds()):
        z, used = lay.fill(rnd, exp=rnd < exp_rounds)
        z0 = z.copy()
        y = h.project(z)
        assert np.array_equal(z, z0, equal_nan=True)
        check_round(h, z, y, used, worst)
        if rnd < 2 or rnd == lay.rounds() - 1:
            assert np.array_equal(h.project(z), y, equal_nan=True), (name, rnd, "the same call gave other bits")
    report("handle " + name, worst)
    assert all(r <= 1.0 for r in worst.values())


def test_one_cone_launch_without_a_tail(handles):
    """HSDE C: one SOCRotated(2), both copies, every input"""
    h = handles("C")
    worst = {}
    for rnd in range(len(cc.NAMES["SOCRotated"])):
        z, used = h.layout.fill(rnd)
        assert len(used) == 2
        check_round(h, z, h.project(z), used, worst)
    report("handle C", worst)


@pytest.mark.parametrize("name", ["A", "feas"])
def test_homogeneity(handles, name):
    """P(2^k z) = 2^k P(z): powers of two commute with every operation of the kernel, so bit for bit at k = +-100 and +-480 (the squares stay normal
    numbers); at k = +-600 a plain sum of squares overflows or vanishes and the rescaled norm must give 2^k x the k = 0 reference within the tolerance"""
    h = handles(name)
    worst = {}
    for base in cc.HOMOGENEITY_BASE:
        rnd = cc.NAMES["SOC"].index(base)
        assert cc.NAMES["SOCRotated"].index(base) == rnd
        z, used = h.layout.fill(rnd, exp=False)
        for _, case in used:
            head = 2 if case.kind == "SOCRotated" else 1                  # what the kernel squares: the tail and the rotated second entry
            sq = np.append(case.x[head:], case.x[0] - case.x[1] if head == 2 else 1.0)
            assert not np.any((sq != 0.0) & (np.abs(sq) <= 2.0 ** -30)), case.label()
        y0 = h.project(z)
        for k in cc.HOMOGENEITY_BITS + cc.HOMOGENEITY_RANGE:
            zk, _ = h.layout.fill(rnd, scale=k, exp=False)
            yk = h.project(zk)
            h.layout.check_guards(zk, yk, name)
            for slot, case in used:
                seg = slice(slot.at, slot.at + slot.length)
                if k in cc.HOMOGENEITY_BITS:
                    assert np.array_equal(yk[seg], np.ldexp(y0[seg], k)), (name, case.label(), k, "dual" if slot.dual else "primal")
                else:
                    key = "%-11s %5d 2^%+d" % (slot.kind, slot.length, k)
                    r = case.check(yk[seg], scale=k, what=name, dual=slot.dual)
                    worst[key] = max(worst.get(key, 0.0), r)
    report("handle %s, rescaled norm" % name, worst)
