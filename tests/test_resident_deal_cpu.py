"""CPU test of the streamed resident solve's DEAL: which of a workgroup's tiles each of its eight wavefronts walks (csrc/fos_internal.hpp: rs_deal,
rs_split; carried to cg_stream_kernel in the plan), no GPU needed.

The deal is restated here from its description -- the communication wavefront takes min(nblk % 7, 3) tiles, and up to RS_NTC = 6 (32-step tiles) where
that leaves it two tiles lighter than the heaviest compute wavefront; the rest goes to the seven compute wavefronts evenly, the earlier ones first --
and checked against what the library makes (`fos_debug_resident_deal`) for every workgroup tile count from 1 to 69: every tile walked exactly once,
compute wavefronts within the NT of the kernel instance the planner picks, the communication wavefront within RS_NTC, slot order = tile order (the
rows' p and s sit in LDS by tile number: what the planner's LDS formula counts), the LDS bytes equal to the launch's and within a CU's 160 KiB.
"""
import ctypes as C

import pytest

RS_NCOMP, RS_NTC, RS_NTC_BASE, RS_COMM_LEAD, RS_GMAX, RS_WPU_MAX = 7, 6, 3, 2, 256, 4
D2, F64 = 16, 8
LDS_CU = 160 * 1024
# cg_stream_kernel's static arrays: s_gcol[64] (d2), s_red[16][4], s_ctl[6], s_halves[16 * 8] (uint32), s_cnt, s_failed, s_tau[9]
STATIC_LDS = 64 * D2 + 16 * 4 * F64 + 6 * F64 + 16 * 8 * 4 + 2 * 4 + 9 * F64


def deal(nblk, steps=32):
    """Tiles per wavefront: seven compute wavefronts, then the communication wavefront."""
    ntc = RS_NTC_BASE if steps > 32 else RS_NTC
    kc = min(nblk % RS_NCOMP, RS_NTC_BASE)
    for k in range(ntc, kc, -1):
        if k <= -(-(nblk - k) // RS_NCOMP) - RS_COMM_LEAD:
            kc = k
            break
    per, rem = divmod(nblk - kc, RS_NCOMP)
    return [per + (1 if w < rem else 0) for w in range(RS_NCOMP)] + [kc]


def previous_deal(nblk):
    per, r = divmod(nblk, RS_NCOMP)
    kc = min(r, RS_NTC_BASE)
    return [per + (1 if w < r - kc else 0) for w in range(RS_NCOMP)] + [kc]


def instance_nt(nblk, steps):
    """NT of the kernel instance for a workgroup of nblk tiles (csr_build.cpp, stream_plan; resident.hip, res_kernel)."""
    nt = max(previous_deal(nblk)[:RS_NCOMP])
    if steps > 32:
        return 3 if nt <= 3 else 5
    return 3 if nt <= 3 else 5 if nt <= 5 else 9 if nt <= 9 else 10


def native_deal(pkg, nblk, steps):
    lib = pkg.lib.load()
    lib.fos_debug_resident_deal.restype = C.c_int
    lib.fos_debug_resident_deal.argtypes = [C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int64)]
    cnt = (C.c_int32 * 8)()
    lds = C.c_int64(0)
    assert lib.fos_debug_resident_deal(nblk, steps, cnt, C.byref(lds)) == 0
    return list(cnt), lds.value


@pytest.mark.parametrize("steps", [32, 64])
def test_deal_for_every_workgroup_tile_count(pkg, steps):
    # (64-step tiles: five per compute wavefront at most -- the planner takes no workgroup beyond 5 x 7 + 3 tiles)
    for nblk in range(1, 70 if steps <= 32 else 39):
        cnt, lds = native_deal(pkg, nblk, steps)
        assert cnt == deal(nblk, steps), (nblk, cnt)
        # every tile exactly once, slot order = tile order: wavefront w's tiles follow those of the wavefronts in front of it, slot = tile number
        slots, t0 = [], 0
        for w in range(RS_NCOMP + 1):
            slots += list(range(t0, t0 + cnt[w]))
            t0 += cnt[w]
        assert slots == list(range(nblk)), (nblk, cnt)
        assert max(cnt[:RS_NCOMP]) <= instance_nt(nblk, steps), (nblk, cnt)
        assert cnt[RS_NCOMP] <= (RS_NTC if steps <= 32 else RS_NTC_BASE), (nblk, cnt)
        # never more per compute wavefront than the previous deal gave, and the previous deal itself up to 8 tiles
        assert max(cnt[:RS_NCOMP]) <= max(previous_deal(nblk)[:RS_NCOMP]), (nblk, cnt)
        if nblk <= 8:
            assert cnt == previous_deal(nblk), (nblk, cnt)
        # the LDS of the launch: column sums per wavefront, the records, the sibling workgroups' column sums, p and s per tile slot
        want = (RS_NCOMP + 1) * 64 * D2 + 4 * RS_GMAX * F64 + (RS_WPU_MAX - 1) * 64 * 2 * F64 + nblk * 128 * D2
        assert lds == want, (nblk, lds, want)
        assert lds + STATIC_LDS <= LDS_CU, (nblk, lds)


def test_c4_deal(pkg):
    """C4's 66 tiles per workgroup: the three compute wavefronts that ended their sweeps last walk one tile fewer, the communication wavefront six."""
    assert native_deal(pkg, 66, 32)[0] == [9, 9, 9, 9, 8, 8, 8, 6]
    assert native_deal(pkg, 69, 32)[0] == [9, 9, 9, 9, 9, 9, 9, 6]
    assert native_deal(pkg, 8, 32)[0] == [1, 1, 1, 1, 1, 1, 1, 1]
    assert native_deal(pkg, 5, 32)[0] == [1, 1, 0, 0, 0, 0, 0, 3]
