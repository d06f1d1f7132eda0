"""
CPU: the rule that decides where the streamed CG solve's fp32 walk reads its float copy from (csrc/fos_internal.hpp: rs_lowp_cached, rs_lowp_cache_budget)
through its host entry fos_host_lowp_cached -- without a handle or a GPU.  A copy is read with the cached policy when it exists, FOS_RS_LOWP_CACHE is not 0
and it is no larger than the budget: the built-in one, or FOS_RS_LOWP_CACHE_MB MiB.
"""
import pytest

MIB = 1 << 20
BUILT_IN = 138 * MIB          # RS_LOWP_CACHE_BUDGET_BYTES, stated here a second time on purpose: changing the budget is a decision, not a side effect


def sizes_around(budget):
    return sorted({0, 1, 4, MIB, budget // 2, budget - 1, budget, budget + 1, budget + MIB, 2 * budget + 1, 138412032, 1 << 40} - {-1})


def test_built_in_budget(pkg):
    assert pkg.host_lowp_cached(1)[1] == BUILT_IN
    assert pkg.host_lowp_cached(1, cache=False)[1] == BUILT_IN


@pytest.mark.parametrize("cache", (True, False))
@pytest.mark.parametrize("budget_mb", (None, 0, 1, 132, 133, 256, 1 << 20))
def test_rule_over_sizes(pkg, cache, budget_mb):
    budget = BUILT_IN if budget_mb is None else budget_mb * MIB
    for nbytes in sizes_around(budget):
        cached, got_budget = pkg.host_lowp_cached(nbytes, cache=cache, budget_mb=budget_mb)
        assert got_budget == budget, (nbytes, cache, budget_mb)
        assert cached == (cache and 0 < nbytes <= budget), (nbytes, cache, budget_mb)


def test_edges_of_the_built_in_budget(pkg):
    assert pkg.host_lowp_cached(0) == (False, BUILT_IN)                   # no copy
    assert pkg.host_lowp_cached(BUILT_IN) == (True, BUILT_IN)
    assert pkg.host_lowp_cached(BUILT_IN + 1) == (False, BUILT_IN)
    assert pkg.host_lowp_cached(138412032) == (True, BUILT_IN)            # the flagship's copy: 512 blocks x 66 tiles x 64 x 32 floats
    assert pkg.host_lowp_cached(138412032, cache=False) == (False, BUILT_IN)
    assert pkg.host_lowp_cached(138412032, budget_mb=0) == (False, 0)
    assert pkg.host_lowp_cached(138412032, budget_mb=132) == (True, 132 * MIB)
    assert pkg.host_lowp_cached(138412032, budget_mb=131) == (False, 131 * MIB)


def test_bad_arguments(pkg):
    with pytest.raises(Exception):
        pkg.host_lowp_cached(-1)
