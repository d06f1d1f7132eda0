"""CPU tests of the resident CG solve's plans against the limits of the kernels that run them (csrc/resident.hip), no GPU needed.

`fos_host_resident_plan` exports the plan `build_resident_plan` (csrc/csr_build.cpp) makes for an operator.  This module restates, from the
kernel source and not from the planner, what each kernel instance indexes, holds in LDS and numbers, and checks every plan the planner accepts:

* the STREAMED form (cg_stream_kernel<TMAX, NT>): G <= RS_GMAX records; a workgroup's tiles split over RS_NCOMP compute wavefronts of at most NT
  tiles and one communication wavefront of at most RS_NTC (rs_split); each tile walked in passes of 32 steps, each pass in whole groups of 8
  steps from the unit's offset in the workgroup (rs_sweep / res_tile_plain) -- inside s_gcol[64] and the wavefront's 64 column sums; a unit over
  at most RS_WPU_MAX workgroups, its column records at stride tmax;
* the REGISTER form (cg_resident_kernel<TMAX, RPT, LB>): tile ti of a workgroup in (wavefront ti % nw, slot ti / nw), nw * RPT slots and
  nw + ncomm wavefronts within the instance's NSLOT and LB; G <= RES_GMAX, a unit over at most RES_WPU_MAX workgroups; whole groups of 8 steps
  inside s_gcol[TMAX];
* both: the launch's dynamic LDS plus the kernel's static arrays within the 160 KiB of a gfx950 CU; the tiles partition the rows of A, the
  units partition its columns.

Fuzzed over random block-diagonal structures, with named structures at the edges (units that end past column 64 of their workgroup, workgroups
of 69..73 tiles, the whole of C4).
"""
import ctypes as C

import numpy as np
import pytest

# ---- the kernels' constants (csrc/resident.hip, csrc/fos_internal.hpp, csrc/dev_common.hpp)
RS_GMAX, RS_WPU_MAX, RS_NCOMP, RS_NTC = 256, 4, 7, 3
RES_GMAX, RES_WPU_MAX = 512, 16
D2, F64 = 16, 8
PEER_MAX_RANKS, RC_COUNT = 16, 6
LDS_CU = 160 * 1024
TILE_GROUP = 8


def _static_lds(tmax_gcol):
    # s_gcol[TMAX] (d2), s_red[16][4], s_ctl[RC_COUNT], s_halves[PEER_MAX_RANKS * 8] (uint32), s_cnt, s_failed
    return tmax_gcol * D2 + 16 * 4 * F64 + RC_COUNT * F64 + PEER_MAX_RANKS * 8 * 4 + 2 * 4


def _stream_instance(tmax, nt):
    """(TMAX, NT) of the cg_stream_kernel instance launch_cg_resident picks."""
    if tmax > 32:
        return 64, (3 if nt <= 3 else 5)
    return 32, (3 if nt <= 3 else 5 if nt <= 5 else 9 if nt <= 9 else 10)


def _rs_split(nblk, w):
    per, r = divmod(nblk, RS_NCOMP)
    kc = min(r, RS_NTC)
    rem = r - kc
    if w < RS_NCOMP:
        return w * per + min(w, rem), per + (1 if w < rem else 0)
    return nblk - kc, kc


def _walk(coff, steps, tmax_k):
    """The column offsets a tile's walk touches in rs_sweep: per pass hf, res_tile_plain<32> from coff + 32 hf over whole groups of 8 steps."""
    spans = []
    for hf in range(tmax_k // 32):
        rem = steps - 32 * hf
        if rem > 0:
            spans.append((coff + 32 * hf, coff + 32 * hf + min(32, -(-rem // TILE_GROUP) * TILE_GROUP)))
    return spans


def host_plan(pkg, m, n, colptr, rowval, gmax):
    lib = pkg.lib.load()
    i64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
    nz = np.ones(len(rowval), dtype=np.float64)
    info = np.zeros(8, dtype=np.int64)
    rc = lib.fos_host_resident_plan(m, n, i64(colptr), i64(rowval), pkg.lib.dptr(nz), int(gmax), i64(info), None, 0, None, 0)
    assert rc == 0, lib.fos_last_error()
    if info[0] == 0:
        return dict(form=0, why=lib.fos_last_error().decode())
    G, ntiles = int(info[1]), int(info[7])
    wg = np.zeros((G, 7), dtype=np.int32)
    tiles = np.zeros((ntiles, 5), dtype=np.int64)
    rc = lib.fos_host_resident_plan(m, n, i64(colptr), i64(rowval), pkg.lib.dptr(nz), int(gmax), i64(info),
                                    wg.ctypes.data_as(C.POINTER(C.c_int32)), G, i64(tiles), ntiles)
    assert rc == 0
    return dict(form=int(info[0]), G=G, nt=int(info[2]), tmax=int(info[3]), nw=int(info[4]), rpt=int(info[5]), ncomm=int(info[6]), wg=wg, tiles=tiles)


def block_structure(shapes):
    """CSC arrays (1-based, as the C ABI takes them) of a block-diagonal A of dense blocks of the given (rows, columns)."""
    rows = np.array([r for r, _ in shapes], dtype=np.int64)
    cols = np.array([c for _, c in shapes], dtype=np.int64)
    roff = np.concatenate([[0], np.cumsum(rows)])
    col_rows = np.repeat(rows, cols)                        # entries per column
    col_r0 = np.repeat(roff[:-1], cols)                     # first row per column
    colptr = np.concatenate([[0], np.cumsum(col_rows)])
    rowval = np.repeat(col_r0 - colptr[:-1], col_rows) + np.arange(colptr[-1], dtype=np.int64)
    return int(roff[-1]), int(cols.sum()), np.ascontiguousarray(colptr + 1), np.ascontiguousarray(rowval + 1)


def violations(P, m, n):
    """What of plan P the kernels cannot run as planned (empty: the plan fits)."""
    bad = []
    G, wg, tiles = P["G"], P["wg"], P["tiles"]
    if P["tmax"] not in (32, 64):
        bad.append("tmax %d" % P["tmax"])
    if (wg[:, 1] < 1).any():
        bad.append("a workgroup without tiles")
    starts = np.concatenate([[0], np.cumsum(wg[:, 1])])
    if P["form"] == 2:
        TMAX, NT = _stream_instance(P["tmax"], P["nt"])
        if G > RS_GMAX:
            bad.append("G %d > RS_GMAX" % G)
        lds = (RS_NCOMP + 1) * 64 * D2 + 4 * RS_GMAX * F64 + (RS_WPU_MAX - 1) * 64 * 2 * F64 + int(wg[:, 1].max()) * 128 * D2
        if lds + _static_lds(64) > LDS_CU:
            bad.append("LDS %d + %d static > %d" % (lds, _static_lds(64), LDS_CU))
    else:
        TMAX = 32 if P["tmax"] <= 32 else 64
        rpt, nw, ncomm = P["rpt"], P["nw"], P["ncomm"]
        RPT, LB = (1, 768) if (TMAX == 32 and rpt == 1) else (2, 512) if (TMAX == 32 and rpt == 2) else (3, 512) if TMAX == 32 else (1, 512)
        NSLOT = LB // 64 * RPT
        if G > RES_GMAX:
            bad.append("G %d > RES_GMAX" % G)
        if rpt > RPT or nw * RPT > NSLOT or 64 * (nw + ncomm) > LB or nw < 1 or ncomm < 1:
            bad.append("wavefronts %d + %d, %d per wavefront in <%d, %d, %d>" % (nw, ncomm, rpt, TMAX, RPT, LB))
        lds = NSLOT * 64 * 4 * D2 + NSLOT * TMAX * D2 + (RES_WPU_MAX - 1) * TMAX * 2 * F64 + 4 * RES_GMAX * F64
        if lds + _static_lds(TMAX) > LDS_CU:
            bad.append("LDS %d + %d static > %d" % (lds, _static_lds(TMAX), LDS_CU))
    for q in range(G):
        blk0, nblk, c0, tc, wg0, wpu, idx = (int(v) for v in wg[q])
        if not (0 <= wg0 <= q < wg0 + wpu <= G and wg0 + idx == q):
            bad.append("wg %d: unit workgroups %d + %d, number %d" % (q, wg0, wpu, idx))
        if wpu > (RS_WPU_MAX if P["form"] == 2 else RES_WPU_MAX):
            bad.append("wg %d: a unit over %d workgroups" % (q, wpu))
        if tc < 1 or tc > 64:
            bad.append("wg %d: %d columns" % (q, tc))
        if wpu > 1 and tc > P["tmax"]:
            bad.append("wg %d: %d columns of a split unit at record stride %d" % (q, tc, P["tmax"]))
        if P["form"] == 2:
            walkers = [_rs_split(nblk, w) for w in range(RS_NCOMP + 1)]
            if sorted(t for t0, cnt in walkers for t in range(t0, t0 + cnt)) != list(range(nblk)):
                bad.append("wg %d: rs_split does not cover its %d tiles once" % (q, nblk))
            if max(cnt for _, cnt in walkers[:RS_NCOMP]) > NT or walkers[RS_NCOMP][1] > RS_NTC:
                bad.append("wg %d: %d tiles, more per wavefront than NT %d" % (q, nblk, NT))
        elif nblk > P["nw"] * P["rpt"]:
            bad.append("wg %d: %d tiles, %d wavefronts x %d" % (q, nblk, P["nw"], P["rpt"]))
        for k in range(starts[q], starts[q] + nblk):
            tc0, tcols, steps, nrows, row0 = (int(v) for v in tiles[k])
            coff = tc0 - c0
            if steps < 1 or steps > TMAX:
                bad.append("wg %d tile %d: %d steps in a TMAX %d kernel" % (q, k, steps, TMAX))
            if P["form"] == 2:
                for a, b in _walk(coff, steps, TMAX):
                    if a < 0 or b > 64:
                        bad.append("wg %d tile %d: walks columns [%d, %d) of 64" % (q, k, a, b))
            else:
                if coff != 0:
                    bad.append("wg %d tile %d: starts at column %d of its unit" % (q, k, coff))
                if -(-steps // TILE_GROUP) * TILE_GROUP > TMAX:
                    bad.append("wg %d tile %d: walks %d of s_gcol[%d]" % (q, k, steps, TMAX))
            if coff < 0 or tcols < 1 or tcols > steps or coff + tcols > tc:
                bad.append("wg %d tile %d: columns [%d, %d) in %d steps, the workgroup's %d" % (q, k, coff, coff + tcols, steps, tc))
            if not (1 <= nrows <= 64):
                bad.append("wg %d tile %d: %d rows" % (q, k, nrows))
    # the tiles partition the rows of A (rows n .. n + m of S), the units (first workgroups) partition its columns
    rows = np.zeros(m, dtype=np.int64)
    for tc0, tcols, steps, nrows, row0 in tiles:
        if row0 < n or row0 + nrows > n + m:
            bad.append("tile rows [%d, %d) outside A" % (row0, row0 + nrows))
        else:
            rows[row0 - n:row0 - n + nrows] += 1
    if not (rows == 1).all():
        bad.append("%d rows of A not in exactly one tile" % int((rows != 1).sum()))
    cols = np.zeros(n, dtype=np.int64)
    for blk0, nblk, c0, tc, wg0, wpu, idx in wg:
        if idx == 0:
            cols[c0:c0 + tc] += 1
    if not (cols == 1).all():
        bad.append("%d columns of A not in exactly one unit" % int((cols != 1).sum()))
    return bad


def check(pkg, shapes, gmax, what):
    m, n, colptr, rowval = block_structure(shapes)
    P = host_plan(pkg, m, n, colptr, rowval, gmax)
    if P["form"] == 0:
        assert P["why"], what
        return P
    bad = violations(P, m, n)
    assert not bad, (what, bad[:5])
    return P


# (name, block shapes, gmax): the units of one streamed workgroup end past column 64 (42 + 24, 50 + 16, 54 + 16, 30 + 32 + 8 in the second pass)
OVERRUNS = [("3x21", [(100, 21)] * 3, 1), ("6x10", [(70, 10)] * 6, 1), ("7x9", [(70, 9)] * 7, 1), ("30+33", [(100, 30), (100, 33)], 1),
            ("3x21-two-workgroups", [(100, 21)] * 6, 2)]


@pytest.mark.parametrize("case", OVERRUNS, ids=[c[0] for c in OVERRUNS])
@pytest.mark.parametrize("stream", ["2", None])
def test_units_past_column_64_are_refused(pkg, case, stream, monkeypatch):
    name, shapes, gmax = case
    if stream:
        monkeypatch.setenv("FOS_RESIDENT_STREAM", stream)
    else:
        monkeypatch.delenv("FOS_RESIDENT_STREAM", raising=False)
    P = check(pkg, shapes, gmax, name)
    if P["form"] == 0:
        assert "column 64" in P["why"], (name, P["why"])


def test_a_unit_at_the_edge_of_column_64_is_planned(pkg, monkeypatch):
    """32 + 24 + 8 columns: the last unit's walk ends exactly on column 64 -- the planner still takes it."""
    monkeypatch.setenv("FOS_RESIDENT_STREAM", "2")
    P = check(pkg, [(100, 32), (100, 24), (100, 8)], 1, "32+24+8")
    assert P["form"] == 2 and P["G"] == 1


@pytest.mark.parametrize("tiles,fits", [(62, True), (69, True), (70, False), (73, False)])
@pytest.mark.parametrize("stream", ["2", None])
def test_streamed_workgroup_tiles_within_lds(pkg, tiles, fits, stream, monkeypatch):
    """One 32-column unit of 64-row tiles on one workgroup: 19456 + 2048 tiles bytes of dynamic LDS + 2104 static -- 69 tiles fit the 160 KiB of a
    CU, 70 .. 73 (the planner's nt_cap * 7 + 3) do not and must be refused, with a reason that says so."""
    if stream:
        monkeypatch.setenv("FOS_RESIDENT_STREAM", stream)
    else:
        monkeypatch.delenv("FOS_RESIDENT_STREAM", raising=False)
    P = check(pkg, [(64 * tiles, 32)], 1, tiles)
    if fits:
        assert P["form"] == 2 and int(P["wg"][0, 1]) == tiles, P
    else:
        assert P["form"] == 0 and "LDS" in P["why"], P


def test_c4_plan_unchanged(pkg, monkeypatch):
    """The whole of C4 (512 blocks of 2080 x 32): the streamed form, 256 workgroups of two units, 66 tiles in nine per compute wavefront -- what
    test_c4_shard_plans asserts -- and within every limit."""
    monkeypatch.delenv("FOS_RESIDENT_STREAM", raising=False)
    P = check(pkg, [(2080, 32)] * 512, 256, "C4")
    assert P["form"] == 2 and P["G"] == 256 and P["nt"] == 9 and int(P["wg"][:, 1].max()) == 66


def _gpu_random_structure(seed):
    """The structure test_gpu_resident.py::test_resident_forms_on_random_block_structures[seed] builds (the same draws)."""
    rng = np.random.default_rng(9000 + seed)
    nb = int(rng.integers(1, 13))
    wide = rng.random() < 0.3
    shapes = [(int(rng.integers(20, 1400)), int(rng.integers(8, 65 if wide else 33))) for _ in range(nb)]
    gmax = rng.choice(["", "1", "2", "3", "5", "8", "40"])
    stream = rng.random() < 0.5
    return shapes, (int(gmax) if gmax else 256), stream


@pytest.mark.parametrize("seed", range(36))
def test_gpu_random_structures_fit_the_kernels(pkg, seed, monkeypatch):
    shapes, gmax, stream = _gpu_random_structure(seed)
    if stream:
        monkeypatch.setenv("FOS_RESIDENT_STREAM", "2")
    else:
        monkeypatch.delenv("FOS_RESIDENT_STREAM", raising=False)
    check(pkg, shapes, gmax, (seed, shapes, gmax, stream))


@pytest.mark.parametrize("chunk", range(8))
def test_random_block_structures_fit_the_kernels(pkg, chunk, monkeypatch):
    """Random block-diagonal structures: 1 .. 600 blocks of 64 .. 4500 rows and 1 .. 64 columns (at most about 400 000 entries), gmax in
    {1, 2, 3, 5, 8, 40, 256}, the streamed form forced and left to the planner: every plan the planner makes fits the kernels."""
    rng = np.random.default_rng(4400 + chunk)
    planned = {1: 0, 2: 0}
    for trial in range(320):
        nb = int(np.exp(rng.uniform(0, np.log(600))))
        narrow = rng.random() < 0.5
        shapes = []
        for _ in range(nb):
            r = int(np.exp(rng.uniform(np.log(64), np.log(4500))))
            c = int(rng.integers(1, 33 if narrow else 65))
            shapes.append((r, c))
        budget = 400_000 / max(1, sum(r * c for r, c in shapes))
        if budget < 1:
            shapes = [(max(64, int(r * budget)), c) for r, c in shapes]
        gmax = int(rng.choice([1, 2, 3, 5, 8, 40, 256]))
        if rng.random() < 0.5:
            monkeypatch.setenv("FOS_RESIDENT_STREAM", "2")
        else:
            monkeypatch.delenv("FOS_RESIDENT_STREAM", raising=False)
        P = check(pkg, shapes, gmax, (chunk, trial, nb, gmax))
        if P["form"]:
            planned[P["form"]] += 1
    assert planned[1] > 0 and planned[2] > 0, planned
