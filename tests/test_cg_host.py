"""
CPU: the two pure rules of the CG solve (csrc/cg.cpp) through their host entries -- fos_host_cg_windows, the windows of sequence numbers a solve reserves,
and fos_host_cg_variant, the decision table behind fos_get_cg_variant -- without a handle or a GPU.
"""
import itertools

import pytest

W21, W32 = 1 << 21, 1 << 32
MAXITS = (0, 1, 1021, 1022, 1023, 1000, 10000, 2 ** 31 - 1)
EPOCHS = (0, 1, W21 - 2, W21 - 1, W21, 3 * W21 - 3, W32 - 2049)


def windows_rule(cg_epoch, maxit):
    """The rule as cg.cpp states it: sequence numbers seq_base + 1 .. seq_base + 2 maxit + 3 in windows of 2048, as many as maxit can use (at most 2^20); the
    run starts behind the last window used, and where it would run through an epoch that is 0 mod 2^21 it starts AT that epoch instead.  uint32 arithmetic."""
    nwin = min((2 * max(maxit, 0) + 4 + 2047) // 2048, 1 << 20)
    first = (cg_epoch + 1) % W32
    off = first % W21
    if off != 0 and off + nwin - 1 > W21 - 1:
        first = (first + W21 - off) % W32
    return first, (first + nwin - 1) % W32


@pytest.mark.parametrize("maxit", MAXITS)
@pytest.mark.parametrize("cg_epoch", EPOCHS)
def test_cg_windows(pkg, cg_epoch, maxit):
    first, last = pkg.host_cg_windows(cg_epoch, maxit)
    assert (first, last) == windows_rule(cg_epoch, maxit)
    nwin = (last - first) % W32 + 1                                   # the new cg_epoch is the run's last window
    assert nwin == min(-(-(2 * maxit + 4) // 2048), 1 << 20)
    ahead = (first - cg_epoch) % W32                                  # the first epoch lies behind the old cg_epoch ...
    assert 1 <= ahead <= W21
    assert first > cg_epoch or cg_epoch + ahead >= W32                # ... greater, or wrapped only as uint32 does
    off = first % W21                                                 # epochs first + 1 .. last: none is 0 mod 2^21
    assert off + nwin - 1 <= W21 - 1
    assert 0 <= first < W32 and 0 <= last < W32


def test_cg_windows_consecutive_solves_never_share_a_window(pkg):
    """a sequence of solves across the 2^21 boundary: every run starts behind the one before"""
    epoch, seen_last = W21 - 20, W21 - 20
    for maxit in (1000, 10000, 1, 1000, 10000, 10000, 1000):
        first, epoch = pkg.host_cg_windows(epoch, maxit)
        assert first > seen_last and epoch >= first
        seen_last = epoch


# ---- the variant table
FLAGS = ("fuse_p", "sharded", "mailboxes", "fold", "row_sharded", "qualifies", "all_qualify", "window_panels", "resident_default")
CACHE = (dict(cache_resident=False, l=100000), dict(cache_resident=True, l=32767), dict(cache_resident=True, l=32768))
PLAN = (dict(plan_streamed=False, plan_workgroups=256, cus=256), dict(plan_streamed=True, plan_workgroups=127, cus=256),
        dict(plan_streamed=True, plan_workgroups=128, cus=256))
REQUESTS = (None, "reference", "fused_p", "merged_sweep", "merged_update", "resident")


def resident_allowed(f):
    return f["qualifies"] and not f["row_sharded"] and (not f["sharded"] or (f["mailboxes"] and f["fold"] and f["all_qualify"]))


def forbidden(v, f):
    return ((v == "resident" and not resident_allowed(f)) or (v == "fused_p" and f["window_panels"]) or (v == "merged_sweep" and f["sharded"])
            or (v == "merged_update" and f["mailboxes"] and not f["fold"]))


def test_cg_variant_table(pkg):
    assert pkg.CG_VARIANT_FLAGS[:2] == ("fuse_p", "sharded") and len(pkg.CG_VARIANT_FLAGS) == 11
    rows = 0
    for bits in itertools.product((False, True), repeat=len(FLAGS)):
        f = dict(zip(FLAGS, bits))
        for cache, plan, request in itertools.product(CACHE, PLAN, REQUESTS):
            v = pkg.host_cg_variant(request, **f, **cache, **plan)
            rows += 1
            where = (request, f, cache, plan)
            assert not forbidden(v, f), where
            if request is not None and not forbidden(request, f):
                assert v == request, where                               # an explicit request that violates nothing is returned as asked
            if request is None and not f["resident_default"]:
                assert v != "resident", where
    assert rows == 2 ** len(FLAGS) * 9 * 6


def test_cg_variant_named_rows(pkg):
    """the defaults DESIGN.md names"""
    one = dict(resident_default=True)
    # one GPU, streamed plan filling at least half the chip
    assert pkg.host_cg_variant(None, l=200000, qualifies=True, all_qualify=True, plan_streamed=True, plan_workgroups=128, cus=256, **one) == "resident"
    assert pkg.host_cg_variant(None, l=200000, qualifies=True, all_qualify=True, plan_streamed=True, plan_workgroups=127, cus=256, **one) == "reference"
    assert pkg.host_cg_variant(None, l=200000, qualifies=True, all_qualify=True, plan_streamed=False, plan_workgroups=256, cus=256, **one) == "reference"
    # one GPU, cache-resident, l >= 32768, no plan
    assert pkg.host_cg_variant(None, l=32768, cache_resident=True, **one) == "merged_update"
    # one GPU otherwise
    assert pkg.host_cg_variant(None, l=32767, cache_resident=True, **one) == "reference"
    assert pkg.host_cg_variant(None, l=10 ** 6, **one) == "reference"
    assert pkg.host_cg_variant(None, l=10 ** 6, fuse_p=True, **one) == "fused_p"
    # sharded through RCCL or a host collective
    assert pkg.host_cg_variant(None, l=1000, sharded=True, **one) == "merged_update"
    assert pkg.host_cg_variant(None, l=1000, sharded=True, qualifies=True, all_qualify=True, plan_streamed=True, plan_workgroups=256, cus=256, **one) == "merged_update"
    # sharded, all shards qualifying, folded mailboxes
    assert pkg.host_cg_variant(None, l=1000, sharded=True, mailboxes=True, fold=True, qualifies=True, all_qualify=True, **one) == "resident"
    assert pkg.host_cg_variant(None, l=1000, sharded=True, mailboxes=True, fold=True, qualifies=True, all_qualify=False, **one) == "merged_update"
    assert pkg.host_cg_variant(None, l=1000, sharded=True, mailboxes=True, fold=True, qualifies=True, all_qualify=True) == "merged_update"   # FOS_RESIDENT_DEFAULT=0
    # unfolded mailboxes: the reference recurrence, its two exchanges between the kernels
    assert pkg.host_cg_variant(None, l=1000, sharded=True, mailboxes=True, fold=False, qualifies=True, all_qualify=True, **one) == "reference"


def test_cg_host_entries_refuse_bad_arguments(pkg):
    with pytest.raises(pkg.lib.FosError):
        pkg.host_cg_windows(-1, 10)
    with pytest.raises(pkg.lib.FosError):
        pkg.host_cg_windows(W32, 10)
    with pytest.raises(pkg.lib.FosError):
        pkg.host_cg_windows(0, 2 ** 31)
