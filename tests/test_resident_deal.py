"""CPU test of the streamed resident solve's deal TABLE (csrc/fos_internal.hpp: rs_deal, rs_split, rs_deal_ok; csrc/csr_build.cpp: stream_plan), no GPU
needed: what any table must promise the kernel, whatever rule made it.

For every workgroup tile count from 1 to 69 and both step classes (tiles of at most 32 steps, and 64-step tiles, which the planner takes up to
5 x 7 + 3 = 38 per workgroup) the eight counts (`fos_debug_resident_deal`: seven compute wavefronts, then the communication wavefront) are checked
against properties, and against the kernel instance the PLANNER selects for a one-unit operator of that many tiles (`fos_host_resident_plan`):

* the counts sum to the tile count;
* each count is at most 10 (four bits, RS_NT_MAX) and at most the NT of the selected instance cg_stream_kernel<TMAX, NT>;
* the communication wavefront's count is at most rs_ntc (6 for 32 steps, 3 for 64) and, where it is above min(tiles mod 7, 3), at least
  RS_COMM_LEAD = 2 below the heaviest compute wavefront;
* a compute wavefront with 0 tiles is followed only by compute wavefronts with 0 tiles (the rows' p and s sit in LDS by tile number: consecutive slots);
* workgroups of at most 8 tiles and all 64-step workgroups get the deal they had before the table could be forced or re-ruled: the expected tables
  are the literals below.

The rule itself for 9 .. 69 tiles of 32 steps did not change either (no candidate table measured faster on the 66-tile flagship shape, DESIGN_LOG.md):
the three counts the log quotes are pinned.
"""
import ctypes as C

import pytest

from test_resident_plan_limits import block_structure, host_plan

RS_NCOMP, RS_NTC, RS_NTC_BASE, RS_COMM_LEAD, RS_NT_MAX = 7, 6, 3, 2, 10

# tiles -> counts, both step classes alike up to 8 tiles
SMALL = {
    1: [0, 0, 0, 0, 0, 0, 0, 1],
    2: [0, 0, 0, 0, 0, 0, 0, 2],
    3: [0, 0, 0, 0, 0, 0, 0, 3],
    4: [1, 0, 0, 0, 0, 0, 0, 3],
    5: [1, 1, 0, 0, 0, 0, 0, 3],
    6: [1, 1, 1, 0, 0, 0, 0, 3],
    7: [1, 1, 1, 1, 1, 1, 1, 0],
    8: [1, 1, 1, 1, 1, 1, 1, 1],
}
# 64-step tiles, 9 .. 38 per workgroup
WIDE = {
    9: [1, 1, 1, 1, 1, 1, 1, 2],
    10: [1, 1, 1, 1, 1, 1, 1, 3],
    11: [2, 1, 1, 1, 1, 1, 1, 3],
    12: [2, 2, 1, 1, 1, 1, 1, 3],
    13: [2, 2, 2, 1, 1, 1, 1, 3],
    14: [2, 2, 2, 2, 2, 2, 2, 0],
    15: [2, 2, 2, 2, 2, 2, 2, 1],
    16: [2, 2, 2, 2, 2, 2, 2, 2],
    17: [2, 2, 2, 2, 2, 2, 2, 3],
    18: [3, 2, 2, 2, 2, 2, 2, 3],
    19: [3, 3, 2, 2, 2, 2, 2, 3],
    20: [3, 3, 3, 2, 2, 2, 2, 3],
    21: [3, 3, 3, 3, 3, 3, 2, 1],
    22: [3, 3, 3, 3, 3, 3, 3, 1],
    23: [3, 3, 3, 3, 3, 3, 3, 2],
    24: [3, 3, 3, 3, 3, 3, 3, 3],
    25: [4, 3, 3, 3, 3, 3, 3, 3],
    26: [4, 4, 3, 3, 3, 3, 3, 3],
    27: [4, 4, 4, 3, 3, 3, 3, 3],
    28: [4, 4, 4, 4, 4, 3, 3, 2],
    29: [4, 4, 4, 4, 4, 4, 3, 2],
    30: [4, 4, 4, 4, 4, 4, 4, 2],
    31: [4, 4, 4, 4, 4, 4, 4, 3],
    32: [5, 4, 4, 4, 4, 4, 4, 3],
    33: [5, 5, 4, 4, 4, 4, 4, 3],
    34: [5, 5, 5, 4, 4, 4, 4, 3],
    35: [5, 5, 5, 5, 4, 4, 4, 3],
    36: [5, 5, 5, 5, 5, 4, 4, 3],
    37: [5, 5, 5, 5, 5, 5, 4, 3],
    38: [5, 5, 5, 5, 5, 5, 5, 3],
}


def native_deal(pkg, nblk, steps):
    lib = pkg.lib.load()
    lib.fos_debug_resident_deal.restype = C.c_int
    lib.fos_debug_resident_deal.argtypes = [C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int64)]
    cnt = (C.c_int32 * 8)()
    assert lib.fos_debug_resident_deal(nblk, steps, cnt, None) == 0
    return list(cnt)


def planned_nt(pkg, nblk, steps, monkeypatch):
    """NT of the instance the planner selects for ONE unit of nblk tiles on one workgroup (32 columns, or 40: 64-step tiles), streamed form forced."""
    monkeypatch.setenv("FOS_RESIDENT_STREAM", "2")
    m, n, colptr, rowval = block_structure([(64 * (nblk - 1) + 40, 32 if steps <= 32 else 40)])
    P = host_plan(pkg, m, n, colptr, rowval, 1)
    assert P["form"] == 2 and P["G"] == 1 and int(P["wg"][0, 1]) == nblk and P["tmax"] == (32 if steps <= 32 else 64), (nblk, steps, P)
    nt = P["nt"]
    assert nt in ((3, 5, 9, 10) if steps <= 32 else (3, 5)), (nblk, steps, nt)          # (the instances res_kernel can launch)
    return nt


@pytest.mark.parametrize("steps", [32, 64])
def test_table_keeps_the_kernels_promises(pkg, steps, monkeypatch):
    ntc = RS_NTC if steps <= 32 else RS_NTC_BASE
    for nblk in range(1, 70 if steps <= 32 else 39):
        cnt = native_deal(pkg, nblk, steps)
        comp, comm = cnt[:RS_NCOMP], cnt[RS_NCOMP]
        assert len(cnt) == 8 and min(cnt) >= 0 and sum(cnt) == nblk, (nblk, cnt)
        nt = planned_nt(pkg, nblk, steps, monkeypatch)
        assert max(cnt) <= RS_NT_MAX and max(comp) <= nt, (nblk, cnt, nt)
        assert comm <= ntc, (nblk, cnt)
        if comm > min(nblk % RS_NCOMP, RS_NTC_BASE):
            assert comm <= max(comp) - RS_COMM_LEAD, (nblk, cnt)
        if 0 in comp:
            assert not any(comp[comp.index(0):]), (nblk, cnt)
        if nblk <= 8:
            assert cnt == SMALL[nblk], (nblk, cnt)
        elif steps > 32:
            assert cnt == WIDE[nblk], (nblk, cnt)


def test_flagship_table_is_the_measured_one(pkg):
    """66 tiles (two units of the flagship block SDP per workgroup), and the two counts the GPU tests take as the rule's edges."""
    assert native_deal(pkg, 66, 32) == [9, 9, 9, 9, 8, 8, 8, 6]
    assert native_deal(pkg, 67, 32) == [9, 9, 9, 9, 9, 8, 8, 6]
    assert native_deal(pkg, 69, 32) == [9, 9, 9, 9, 9, 9, 9, 6]
