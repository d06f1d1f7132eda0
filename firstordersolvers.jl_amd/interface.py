"""
Host-side mirror of the reference's solver interface for the HSDE hot path.

Same names, argument meaning and behaviour as the Julia reference (paths under the reference checkout):

  GAP / DR / AP / GAPA / FISTA / Dykstra constructors   src/solvers/gap.jl:13, solvers.jl:10-11, gapa.jl:15,
                                                        fista.jl:11, dykstra.jl:9
  FOSMathProgModel + loadproblem! / optimize! / status / getobjval / getsolution / numvar / numconstr
                                                        src/types.jl:30-60, src/FOSSolverInterface.jl:5-69
  solve! option handling, iterate                       src/solverwrapper.jl:2-41
  HSDEStatus printing, history keys                     src/problemforms/HSDE/HSDEStatus.jl:73-91,125-139
  HSDE_populatesolution                                 src/problemforms/HSDE/HSDE.jl:49-61

Every numerical operation is a call into libfoship.so (HIP, gfx950) through `_lib`; nothing here computes on
the CPU beyond scalar bookkeeping, and there is no fallback when the library or a GPU is missing.
"""
from __future__ import annotations

import ctypes as C
import time

import math

import numpy as np
import scipy.sparse as sp

from . import _lib

HEADER_CG = " Iter | pri res | dua res | rel gap | pri obj | dua obj | kap/tau | cg  | time"       # HSDEStatus.jl:79-81
HEADER_DIRECT = " Iter | pri res | dua res | rel gap | pri obj | dua obj | kap/tau | time"


# ---------------------------------------------------------------------------------------------- algorithms

class FOSAlgorithm:
    """abstract type FOSAlgorithm (src/types.jl:13)."""
    direct = False
    options: dict

    def _alg_args(self):
        raise NotImplementedError


class GAP(FOSAlgorithm):
    """GAP(alpha=0.8, alpha1=1.8, alpha2=1.8; direct=false, kwargs...)   gap.jl:6-13"""

    def __init__(self, alpha=0.8, alpha1=1.8, alpha2=1.8, direct=False, **kwargs):
        self.alpha, self.alpha1, self.alpha2, self.direct, self.options = alpha, alpha1, alpha2, direct, kwargs

    def _alg_args(self):
        return (_lib.ALG_GAP, self.alpha, self.alpha1, self.alpha2, 0.0)


def DR(alpha=0.5, **kwargs):
    """DR(alpha=0.5) = GAP(alpha, 2.0, 2.0)   solvers.jl:10"""
    return GAP(alpha, 2.0, 2.0, **kwargs)


def AP(alpha=1, **kwargs):
    """AP(alpha=1) = GAP(alpha, 1.0, 1.0)   solvers.jl:11"""
    return GAP(alpha, 1.0, 1.0, **kwargs)


class GAPA(FOSAlgorithm):
    """GAPA(alpha=1.0, beta=0.0; direct=false, kwargs...)   gapa.jl:9-15"""

    def __init__(self, alpha=1.0, beta=0.0, direct=False, **kwargs):
        self.alpha, self.beta, self.direct, self.options = alpha, beta, direct, kwargs

    def _alg_args(self):
        return (_lib.ALG_GAPA, self.alpha, 0.0, 0.0, self.beta)


class FISTA(FOSAlgorithm):
    """FISTA(alpha=1.0; direct=false, kwargs...)   fista.jl:6-11"""

    def __init__(self, alpha=1.0, direct=False, **kwargs):
        self.alpha, self.direct, self.options = alpha, direct, kwargs

    def _alg_args(self):
        return (_lib.ALG_FISTA, self.alpha, 0.0, 0.0, 0.0)


class GAPP(FOSAlgorithm):
    """GAPP(alpha=0.8, alpha1=1.8, alpha2=1.8; direct=true, iproj=100, kwargs...)   gapproj.jl:5-13, the last row of the reference's
    solver table (README.md:32-40): GAP whose every iproj-th iteration is a 21-point projected search.  On the HSDE path
    (fos_set_gapp) and on the Feasibility form (fos_feas_set_gapp); `direct` defaults to true as in the reference (dense, l <= 46 000)."""

    def __init__(self, alpha=0.8, alpha1=1.8, alpha2=1.8, direct=True, iproj=100, **kwargs):
        self.alpha, self.alpha1, self.alpha2, self.direct, self.iproj, self.options = alpha, alpha1, alpha2, direct, int(iproj), kwargs

    def _alg_args(self):
        return (_lib.ALG_GAP, self.alpha, self.alpha1, self.alpha2, 0.0)         # + fos_set_gapp(iproj)


class Dykstra(FOSAlgorithm):
    """Dykstra(; direct=false, kwargs...)   dykstra.jl:5-9"""

    def __init__(self, direct=False, **kwargs):
        self.direct, self.options = direct, kwargs

    def _alg_args(self):
        return (_lib.ALG_DYKSTRA, 0.0, 0.0, 0.0, 0.0)


# ---------------------------------------------------------------------------------------------- device handle

def _ieee_div(a, b):
    """a / b as Julia evaluates it (Inf / NaN instead of an exception when tau is still 0 at an early check)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.float64(a) / np.float64(b))


def _julia_specials(s):
    """@printf shows Inf / NaN where Python's % formatting writes inf / nan."""
    return s.replace("inf", "Inf").replace("nan", "NaN")


def julia_float(x):
    """How Julia's println shows a Float64 (shortest round-trip digits; exponent form outside 1e-4 <= |x| < 1e6)."""
    x = float(x)
    if math.isnan(x):
        return "NaN"
    if math.isinf(x):
        return "Inf" if x > 0 else "-Inf"
    if x == 0.0:
        return "-0.0" if math.copysign(1.0, x) < 0 else "0.0"
    mant, ex = np.format_float_scientific(x, unique=True, trim="0").split("e")
    ex = int(ex)
    if -4 <= ex < 6:
        return np.format_float_positional(x, unique=True, trim="0")
    return "%se%d" % (mant + "0" if mant.endswith(".") else mant, ex)


class LineSearchWrapper(FOSAlgorithm):
    """LineSearchWrapper(alg; lsinterval=100, kwargs...)   wrappers/linesearch.jl:3-24 -- around GAP (AP, DR) or GAPA, the
    algorithms with support_linesearch == Val{:Fast}.  Every lsinterval-th iteration is a 31-point search of the step length
    along S2!(S1!(x)) - x, run on the device (fos_set_linesearch); the reference's println output of a search is reproduced
    from fos_linesearch_log."""

    def __init__(self, alg, lsinterval=100, **kwargs):
        if not isinstance(alg, (GAP, GAPA)):                 # linesearch.jl:20-22 (an @error in the reference)
            raise ValueError("Algorithm %s does not support line search" % type(alg).__name__)
        self.alg, self.lsinterval = alg, int(lsinterval)
        self.options = {**alg.options, **kwargs}            # merge(alg.options, kwargs)
        self.direct = alg.direct

    def _alg_args(self):
        return self.alg._alg_args()


class LongstepWrapper(FOSAlgorithm):
    """LongstepWrapper(alg; longinterval=100, nsave=10, kwargs...)   wrappers/longstep.jl:5-24 -- around GAP (AP, DR), GAPA, FISTA or Dykstra
    (support_longstep).  The last nsave + 1 iterations of every longinterval save the half-planes of their two projections (addprojeq /
    addprojineq); the iterate is then projected onto the saved planes (projectonnormals!, saveplanes.jl:13-35).  All on the device
    (fos_set_longstep): the planes never leave it, the projection's small dual QP is solved by the library."""

    def __init__(self, alg, longinterval=100, nsave=10, **kwargs):
        if not isinstance(alg, (GAP, GAPA, FISTA, Dykstra)) or isinstance(alg, GAPP):      # longstep.jl:28 (an @error in the reference)
            raise ValueError("Algorithm %s does not support longstep" % type(alg).__name__)
        self.alg, self.longinterval, self.nsave = alg, int(longinterval), int(nsave)
        self.options = {**kwargs, **alg.options}            # [kwargs..., alg.options...]: the wrapped algorithm's options win  longstep.jl:23
        self.direct = alg.direct

    def _alg_args(self):
        return self.alg._alg_args()


def _normalize_cones(cones, total, what):
    """(name, length) or (name, 1-based index range/list) tuples -> (types int32, starts int64 1-based, lens int64).
    Index lists must be contiguous: toRanges, src/cones.jl:44-56."""
    types, starts, lens = [], [], []
    run = 1
    for name, spec in cones:
        if name not in _lib.CONE_CODES:
            raise KeyError("Cone type %s not supported" % name)          # FOSSolverInterface.jl:37-42
        if isinstance(spec, (int, np.integer)):
            s, ln = run, int(spec)
        else:
            idx = np.asarray(list(spec), dtype=np.int64)
            if idx.size == 0 or not np.array_equal(idx, np.arange(idx[0], idx[-1] + 1)):
                raise ValueError("Invalid range in input")               # cones.jl:50
            s, ln = int(idx[0]), int(idx.size)
        types.append(_lib.CONE_CODES[name])
        starts.append(s)
        lens.append(ln)
        run = s + ln
    return (np.asarray(types, dtype=np.int32), np.asarray(starts, dtype=np.int64), np.asarray(lens, dtype=np.int64))


DIRECT_FACTOR_NAMES = ("newton", "cholesky")                     # FOS_DIRECT_FACTOR_*


def direct_factor_code(factor):
    """FOS_DIRECT_FACTOR_* of the name of a factor of direct = true ("newton" | "cholesky"); needs no GPU"""
    if factor not in DIRECT_FACTOR_NAMES:
        raise ValueError("direct factor must be one of %s, not %r" % (sorted(DIRECT_FACTOR_NAMES), factor))
    return DIRECT_FACTOR_NAMES.index(factor)


EQUILIBRATE_DEFAULT_PASSES = 10


def equilibrate_passes(equilibrate):
    """the `equilibrate` option -> passes of fos_create3: False / None / 0 = off, True = 10 passes, an int = that many"""
    if equilibrate is None or equilibrate is False:
        return 0
    if equilibrate is True:
        return EQUILIBRATE_DEFAULT_PASSES
    if not isinstance(equilibrate, (int, np.integer)):
        raise TypeError("equilibrate must be a bool or a number of passes, not %r" % (equilibrate,))
    return int(equilibrate)


class _KeepAlive(tuple):
    """a tuple of ctypes arguments that also holds the numpy arrays behind its pointers"""


def _problem_args(A, b, c, K1, K2):
    """(m, n, the leading arguments of fos_create* / fos_host_equilibrate, nnz); the tuple keeps the arrays the pointers refer to alive"""
    A = sp.csc_matrix(A)                       # loadproblem! sparsifies dense input, FOSSolverInterface.jl:27-29
    A.sort_indices()
    m, n = A.shape
    b = _lib.as_f64(b, m)
    c = _lib.as_f64(c, n)
    colptr = np.ascontiguousarray(A.indptr, dtype=np.int64) + 1          # Julia 1-based
    rowval = np.ascontiguousarray(A.indices, dtype=np.int64) + 1
    nzval = np.ascontiguousarray(A.data, dtype=np.float64)
    k1t, k1s, k1l = _normalize_cones(K1, m, "K1")
    k2t, k2s, k2l = _normalize_cones(K2, n, "K2")
    i64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
    i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    args = _KeepAlive((m, n, i64(colptr), i64(rowval), _lib.dptr(nzval), _lib.dptr(b), _lib.dptr(c),
                       len(k1t), i32(k1t), i64(k1s), i64(k1l), len(k2t), i32(k2t), i64(k2s), i64(k2l)))
    args.keep = (colptr, rowval, nzval, b, c, k1t, k1s, k1l, k2t, k2s, k2l)
    return m, n, args, int(A.nnz)


def host_equilibrate(A, b, c, K1, K2, passes=EQUILIBRATE_DEFAULT_PASSES):
    """fos_host_equilibrate: the scaling fos_create3 computes, on the host (no GPU).  Returns dict(passes, D, E, sigma, rho, gamma, A, b, c) with
    A = D A E (CSC, the pattern of the input), b = sigma D b, c = rho E c."""
    lib = _lib.load()
    m, n, args, nnz = _problem_args(A, b, c, K1, K2)
    D, E, scal, nz, bo, co = np.empty(m), np.empty(n), np.empty(3), np.empty(nnz), np.empty(m), np.empty(n)
    _lib.check(lib.fos_host_equilibrate(*args, int(passes), _lib.dptr(D), _lib.dptr(E), _lib.dptr(scal), _lib.dptr(nz), _lib.dptr(bo), _lib.dptr(co)))
    colptr, rowval = args.keep[0], args.keep[1]
    As = sp.csc_matrix((nz, (rowval - 1).astype(np.int64), (colptr - 1).astype(np.int64)), shape=(m, n))
    return dict(passes=int(passes), D=D, E=E, sigma=float(scal[0]), rho=float(scal[1]), gamma=float(scal[2]), A=As, b=bo, c=co)


CG_VARIANT_NAMES = ("reference", "fused_p", "merged_sweep", "merged_update", "resident")
# foship.h FOS_CGV_*, in bit order
CG_VARIANT_FLAGS = ("fuse_p", "sharded", "mailboxes", "fold", "row_sharded", "qualifies", "all_qualify", "cache_resident", "window_panels", "plan_streamed",
                    "resident_default")


def host_cg_variant(request=None, l=0, plan_workgroups=0, cus=256, **flags):
    """fos_host_cg_variant: the recurrence a handle with these properties would run (the rule behind cg_variant_name(), no GPU).  request: a name of
    CG_VARIANT_NAMES or None (the default); flags: CG_VARIANT_FLAGS by keyword, False where not given."""
    bits = sum(1 << CG_VARIANT_FLAGS.index(k) for k, on in flags.items() if on)
    v = C.c_int32(0)
    _lib.check(_lib.load().fos_host_cg_variant(-1 if request is None else CG_VARIANT_NAMES.index(request), bits, int(l), int(plan_workgroups), int(cus), C.byref(v)))
    return CG_VARIANT_NAMES[v.value]


def host_lowp_cached(val32_bytes, cache=True, budget_mb=None):
    """fos_host_lowp_cached: (whether a streamed plan with a float copy of `val32_bytes` reads it with the cached policy, the budget in bytes) -- the rule
    behind resident_stats()["lowp_cached"], no GPU.  cache: FOS_RS_LOWP_CACHE; budget_mb: FOS_RS_LOWP_CACHE_MB (MiB) or None for the built-in budget."""
    cached, budget = C.c_int32(0), C.c_int64(0)
    _lib.check(_lib.load().fos_host_lowp_cached(int(val32_bytes), 1 if cache else 0, -1 if budget_mb is None else int(budget_mb), C.byref(cached), C.byref(budget)))
    return bool(cached.value), budget.value


def host_cg_windows(cg_epoch, maxit):
    """fos_host_cg_windows: (first window, last window = the new cg_epoch) of a solve with the cap `maxit` behind `cg_epoch` (no GPU)."""
    first, last = C.c_int64(0), C.c_int64(0)
    _lib.check(_lib.load().fos_host_cg_windows(int(cg_epoch), int(maxit), C.byref(first), C.byref(last)))
    return first.value, last.value


class _WrapperLogs:
    """The last search / projection of the three wrappers, for both handles: `_log_prefix` names the form's entries (fos_ / fos_feas_)."""

    def _wrapper_log(self, name, count):
        out = np.zeros(count)
        _lib.check(getattr(self._lib, self._log_prefix + name)(self._h, _lib.dptr(out)))
        return out

    def longstep_log(self):
        """last projection onto the saved planes: dict(iteration, active inequalities, KKT violation of the small dual, step length, rows, supports tried)"""
        out = self._wrapper_log("longstep_log", 8)
        return dict(iteration=int(out[0]), active=int(out[1]), violation=float(out[2]), step=float(out[3]), rows=int(out[4]), tried=int(out[5]), failed=bool(out[6]),
                    given_up=int(out[7]))

    def gapp_log(self):
        """(iteration, [21 test norms], alpha_best) of GAPP's last search."""
        out = self._wrapper_log("gapp_log", 23)
        return int(out[22]), out[0:21].copy(), float(out[21])

    def linesearch_log(self):
        """(iteration, ||res||, [31 test residuals], alpha_best) of the last search."""
        out = self._wrapper_log("linesearch_log", 34)
        return int(out[33]), float(out[0]), out[1:32].copy(), float(out[32])


class HipHSDE(_WrapperLogs):
    """Owns one fos_handle: the device-resident S1 (AffinePlusLinear over HSDEMatrixQ), S2 (DualConeProduct),
    iterate and algorithm data.  == what init_algorithm!/get_sets_and_status build (FOSSolverInterface.jl:76-79)."""
    _log_prefix = "fos_"

    def __init__(self, A, b, c, K1, K2, device=0, row_sharded=False, equilibrate=0):
        """row_sharded: this rank holds the rows of A of its K1 cones and all columns (sharding.shard_rows);
        follow with comm_init on every rank.
        equilibrate: passes (0..50; True = 10) of the opt-in scaling of fos_create3 -- the handle then solves D A E, sigma D b, rho E c; iterates and check
        results stay in the caller's units, the fine-grained operators speak the scaled problem (include/foship.h)."""
        self._lib = _lib.load()
        m, n, args, self.nnz = _problem_args(A, b, c, K1, K2)
        self.m, self.n, self.l, self.N = m, n, m + n + 1, 2 * (m + n + 1)
        h = C.c_void_p()
        _lib.check(self._lib.fos_create3(*args, device, 1 if row_sharded else 0, equilibrate_passes(equilibrate), C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._lib.fos_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def equilibration(self):
        """fos_get_equilibration: dict(passes, D, E, sigma, rho, gamma); a plain handle reports 0 passes and ones"""
        p = C.c_int32(0)
        D, E, scal = np.empty(self.m), np.empty(self.n), np.empty(3)
        _lib.check(self._lib.fos_get_equilibration(self._h, C.byref(p), _lib.dptr(D), _lib.dptr(E), _lib.dptr(scal)))
        return dict(passes=int(p.value), D=D, E=E, sigma=float(scal[0]), rho=float(scal[1]), gamma=float(scal[2]))

    # -- algorithm / state
    def set_alg(self, alg: FOSAlgorithm):
        code, a, a1, a2, beta = alg._alg_args()
        _lib.check(self._lib.fos_set_alg(self._h, code, a, a1, a2, beta))
        if isinstance(alg, LineSearchWrapper):
            self.set_linesearch(alg.lsinterval)
        if isinstance(alg, GAPP):
            _lib.check(self._lib.fos_set_gapp(self._h, alg.iproj))
        if isinstance(alg, LongstepWrapper):
            self.set_longstep(alg.longinterval, alg.nsave)

    def set_longstep(self, longinterval, nsave):
        """LongstepWrapper around the current algorithm (longinterval 0: off); fos_set_longstep."""
        _lib.check(self._lib.fos_set_longstep(self._h, int(longinterval), int(nsave)))

    def set_linesearch(self, lsinterval):
        """LineSearchWrapper around the current algorithm (0: off); fos_set_linesearch."""
        _lib.check(self._lib.fos_set_linesearch(self._h, int(lsinterval)))

    def reset_affine(self):
        _lib.check(self._lib.fos_reset_affine(self._h))

    def set_iterate(self, z=None):
        if z is None:
            _lib.check(self._lib.fos_set_iterate(self._h, None))
        else:
            z = _lib.as_f64(z, self.N)
            _lib.check(self._lib.fos_set_iterate(self._h, _lib.dptr(z)))

    def get_iterate(self):
        z = np.empty(self.N)
        _lib.check(self._lib.fos_get_iterate(self._h, _lib.dptr(z)))
        return z

    def get_checked(self):
        z = np.empty(self.N)
        _lib.check(self._lib.fos_get_checked(self._h, _lib.dptr(z)))
        return z

    def step(self, i_first, count, checki, eps):
        done = C.c_int64(0)
        checked = C.c_int32(0)
        res = _lib.CheckResult()
        _lib.check(self._lib.fos_step(self._h, i_first, count, checki, eps, C.byref(done), C.byref(checked), C.byref(res)))
        return done.value, bool(checked.value), res

    def getsol(self, force_check=False, eps=1e-5):
        z = np.empty(self.N)
        res = _lib.CheckResult()
        _lib.check(self._lib.fos_getsol(self._h, _lib.dptr(z), 1 if force_check else 0, eps, C.byref(res)))
        return z, (res if force_check else None)

    def get_affine_state(self):
        """(xinit, i, firstrun): CGdata.xinit, AffinePlusLinear.i, CGdata.firstrun."""
        z = np.empty(self.N)
        i = C.c_int64(0)
        fr = C.c_int32(0)
        _lib.check(self._lib.fos_get_affine_state(self._h, _lib.dptr(z), C.byref(i), C.byref(fr)))
        return z, i.value, bool(fr.value)

    def set_affine_state(self, xinit, i):
        xinit = _lib.as_f64(xinit, self.N)
        _lib.check(self._lib.fos_set_affine_state(self._h, _lib.dptr(xinit), int(i)))

    def get_alg_state(self):
        """(a, b, t, alpha12): FISTAData.y / .xold / .t (fista.jl:15-25), DykstraData.p / .q (dykstra.jl:12-23), GAPAData.alpha12."""
        a, b, sc = np.empty(self.N), np.empty(self.N), np.zeros(2)
        _lib.check(self._lib.fos_get_alg_state(self._h, _lib.dptr(a), _lib.dptr(b), _lib.dptr(sc)))
        return a, b, float(sc[0]), float(sc[1])

    def set_alg_state(self, a=None, b=None, t=None, alpha12=None):
        """installs what is given (fos_set_alg_state); t / alpha12 default to the handle's current values"""
        sc = None
        if t is not None or alpha12 is not None:
            cur = np.zeros(2)
            _lib.check(self._lib.fos_get_alg_state(self._h, None, None, _lib.dptr(cur)))
            sc = np.array([cur[0] if t is None else float(t), cur[1] if alpha12 is None else float(alpha12)])
        a = None if a is None else _lib.as_f64(a, self.N)
        b = None if b is None else _lib.as_f64(b, self.N)
        _lib.check(self._lib.fos_set_alg_state(self._h, None if a is None else _lib.dptr(a), None if b is None else _lib.dptr(b),
                                               None if sc is None else _lib.dptr(sc)))

    def cgiter(self):
        v = C.c_int64(0)
        _lib.check(self._lib.fos_get_cgiter(self._h, C.byref(v)))
        return v.value

    def alpha12(self):
        v = C.c_double(0)
        _lib.check(self._lib.fos_get_alpha12(self._h, C.byref(v)))
        return v.value

    def prox_count(self):
        v = C.c_int64(0)
        _lib.check(self._lib.fos_get_prox_count(self._h, C.byref(v)))
        return v.value

    # -- fine grained operators (each: host -> device -> host)
    def q_apply(self, x, transpose=False):
        x = _lib.as_f64(x, self.l)
        y = np.empty(self.l)
        _lib.check(self._lib.fos_q_apply(self._h, _lib.dptr(y), _lib.dptr(x), 1 if transpose else 0))
        return y

    def kkt_apply(self, x):
        x = _lib.as_f64(x, self.N)
        y = np.empty(self.N)
        _lib.check(self._lib.fos_kkt_apply(self._h, _lib.dptr(y), _lib.dptr(x)))
        return y

    def cg_kkt(self, x0, rhs, tol, max_iters=10000):
        x = _lib.as_f64(x0, self.N).copy()
        rhs = _lib.as_f64(rhs, self.N)
        it = C.c_int64(0)
        _lib.check(self._lib.fos_cg_kkt(self._h, _lib.dptr(x), _lib.dptr(rhs), tol, max_iters, C.byref(it)))
        return x, it.value

    def prox_affine(self, x):
        x = _lib.as_f64(x, self.N)
        y = np.empty(self.N)
        _lib.check(self._lib.fos_prox_affine(self._h, _lib.dptr(y), _lib.dptr(x)))
        return y

    def hsdematrix_prox(self, x):
        x = _lib.as_f64(x, self.N)
        y = np.empty(self.N)
        _lib.check(self._lib.fos_hsdematrix_prox(self._h, _lib.dptr(y), _lib.dptr(x)))
        return y

    def prox_cones(self, x):
        x = _lib.as_f64(x, self.N)
        y = np.empty(self.N)
        _lib.check(self._lib.fos_prox_cones(self._h, _lib.dptr(y), _lib.dptr(x)))
        return y

    def check(self, z, eps=1e-5):
        z = _lib.as_f64(z, self.N)
        res = _lib.CheckResult()
        _lib.check(self._lib.fos_check(self._h, _lib.dptr(z), eps, C.byref(res)))
        return res

    # -- measurement
    def profile(self, enable):
        """False/0: off; True/1: events around every KKT launch; N > 1: around every N-th (sampling)."""
        _lib.check(self._lib.fos_profile(self._h, int(enable)))

    def profile_read(self):
        n = C.c_int64(0)
        ms = C.c_double(0)
        by = C.c_double(0)
        _lib.check(self._lib.fos_profile_read(self._h, C.byref(n), C.byref(ms), C.byref(by)))
        return n.value, ms.value, by.value

    def bench_kkt(self, reps):
        ms = C.c_double(0)
        _lib.check(self._lib.fos_bench_kkt(self._h, reps, C.byref(ms)))
        return ms.value

    def cg_total(self):
        v = C.c_int64(0)
        _lib.check(self._lib.fos_get_cg_total(self._h, C.byref(v)))
        return v.value

    def operator_stats(self):
        """Format statistics of the device operator (fos_operator_stats)."""
        st = (C.c_int64 * 12)()
        _lib.check(self._lib.fos_operator_stats(self._h, st))
        keys = ("blocks", "ell", "lds", "long", "run", "vals", "cols", "waves", "tiles", "slots", "deferred", "tile_vals")
        out = dict(zip(keys, list(st)))
        ws = (C.c_int64 * 4)()
        _lib.check(self._lib.fos_window_stats(self._h, ws))
        out.update(zip(("win_panels", "win_segments", "win_slices", "win_vals"), list(ws)))
        out["lowp_val32_bytes"] = int(self._lowp_stats()[4])      # the float copy of the tile values (streamed resident plan, fos_resident_lowp_stats)
        return out

    def sync(self):
        _lib.check(self._lib.fos_sync(self._h))

    DIRECT_FORMS = {"auto": 0, "reduced": 4}                      # FOS_DIRECT_FORM_*

    def enable_direct(self, A, form="auto", factor="newton"):
        """direct = true (HSDE.jl:12-15): exact affine projection through a one-time factorisation (fos_enable_direct3).  form="auto": the first of
        block / dense / cg that applies; form="reduced": the inverse of I + A'A or I + A A' (order min(m, n) <= 46 000) as packed lower-triangle tiles.
        factor: how the stored inverse of the dense and the reduced form is built -- "newton" (Newton-Schulz) or "cholesky" (blocked Cholesky, opt-in)."""
        if form not in self.DIRECT_FORMS:
            raise ValueError("direct form must be one of %s, not %r" % (sorted(self.DIRECT_FORMS), form))
        factor_code = direct_factor_code(factor)
        A = sp.csc_matrix(A)
        A.sort_indices()
        colptr = (A.indptr.astype(np.int64) + 1)
        rowval = (A.indices.astype(np.int64) + 1)
        nz = np.ascontiguousarray(A.data, dtype=np.float64)
        i64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
        _lib.check(self._lib.fos_enable_direct3(self._h, i64(colptr), i64(rowval), _lib.dptr(nz), self.DIRECT_FORMS[form], factor_code))

    def disable_direct(self):
        _lib.check(self._lib.fos_disable_direct(self._h))

    def direct_mode(self):
        """'off' | 'dense' | 'block' | 'cg' | 'reduced': the form S1 = IndAffine([Q -I], 0) runs in (fos_get_direct_mode)"""
        v = C.c_int32(0)
        _lib.check(self._lib.fos_get_direct_mode(self._h, C.byref(v)))
        return ("off", "dense", "block", "cg", "reduced")[v.value]

    def direct_stats(self):
        """the last set-up of direct = true (fos_get_direct_stats2): form, order of the stored inverse, set-up seconds, Newton-Schulz steps (Cholesky factor: its
        polish steps), the factor that built the inverse, the seconds of the inversion stage alone, the last probe residual, whether Cholesky fell back"""
        out = np.zeros(8)
        _lib.check(self._lib.fos_get_direct_stats2(self._h, _lib.dptr(out)))
        return {"form": ("off", "dense", "block", "cg", "reduced")[int(out[0])], "k": int(out[1]), "setup_s": float(out[2]), "ns_steps": int(out[3]),
                "factor": DIRECT_FACTOR_NAMES[int(out[4])], "invert_s": float(out[5]), "probe_resid": float(out[6]), "fell_back": int(out[7])}

    def set_tuning(self, spmv_workgroups=0, cg_chunk=0, fuse_p=-1):
        """fuse_p: -1 keeps the library's choice, 0 / 1 force the three- / two-launch CG iteration (1 on an operator stored in window panels:
        FosError(FOS_EUNSUPPORTED), nothing changes)."""
        _lib.check(self._lib.fos_set_tuning(self._h, spmv_workgroups, cg_chunk, fuse_p))

    def set_cg_variant(self, variant):
        """which CG recurrence the affine projection runs: 'reference' | 'fused_p' | 'merged_sweep' | 'merged_update' | 'resident' | None (default).
        'resident' (one launch per solve, operator and vectors in registers) raises FosError(FOS_EUNSUPPORTED) when the operator does not qualify,
        'fused_p' when the operator is stored in window panels (their sweeps cannot build p on the fly)."""
        codes = {None: -1, "default": -1, "reference": _lib.CG_REFERENCE, "fused_p": _lib.CG_FUSED_P,
                 "merged_sweep": _lib.CG_MERGED_SWEEP, "merged_update": _lib.CG_MERGED_UPDATE, "resident": _lib.CG_RESIDENT}
        _lib.check(self._lib.fos_set_cg_variant(self._h, codes[variant] if not isinstance(variant, int) else variant))

    def cg_variant_name(self):
        v = C.c_int32(0)
        _lib.check(self._lib.fos_get_cg_variant(self._h, C.byref(v)))
        return CG_VARIANT_NAMES[v.value]

    def resident_stats(self):
        """The plan of the resident CG solve (foship.h fos_resident_stats)."""
        st = (C.c_int64 * 8)()
        _lib.check(self._lib.fos_resident_stats(self._h, st))
        keys = ("qualifies", "workgroups", "waves_per_workgroup", "tiles_per_wave", "units", "max_tiles_per_workgroup", "steps_per_tile", "all_ranks_qualify")
        out = {k: int(st[i]) for i, k in enumerate(keys)}
        out["form"] = "streamed" if out["tiles_per_wave"] < 0 else "registers"        # streamed: tiles re-read every iteration (resident.hip, cg_stream_kernel)
        out["tiles_per_wave"] = abs(out["tiles_per_wave"])
        # the streamed form's fp32 walk (foship.h fos_resident_lowp_stats): its bound of |A - fl32(A)|_2 and the last solve's record
        lp = self._lowp_stats()
        out.update(lowp_delta=lp[0], lowp_sweeps_last_solve=int(lp[1]), lowp_reverted_last_solve=int(lp[2]), lowp_bound_last_solve=lp[3])
        # where the float copy is read from (foship.h fos_resident_lowp_cache_stats): 1 = with the cached policy, and the budget the rule was held to
        lc = (C.c_int64 * 2)()
        _lib.check(self._lib.fos_resident_lowp_cache_stats(self._h, lc))
        out.update(lowp_cached=int(lc[0]), lowp_cache_budget_bytes=int(lc[1]))
        return out

    def _lowp_stats(self):
        lp = np.zeros(8)
        _lib.check(self._lib.fos_resident_lowp_stats(self._h, _lib.dptr(lp)))
        return [float(v) for v in lp]

    def debug_set(self, what, value):
        _lib.check(self._lib.fos_debug_set(self._h, int(what), int(value)))

    def profile_read_classes(self):
        """{'kkt' | 'psd' | 'cgvec': (launch groups, summed ms), 'other': (sampled outer iterations, summed ms of every other launch
        group in them)} of the bracketed launches since the last read."""
        n = (C.c_int64 * 5)()
        ms = (C.c_double * 5)()
        _lib.check(self._lib.fos_profile_read_classes(self._h, n, ms))
        return {k: (n[i], ms[i]) for i, k in enumerate(("kkt", "psd", "cgvec", "other", "resident"))}

    def psd_debug(self, collect_stats=True, phase_limit=0):
        _lib.check(self._lib.fos_psd_debug(self._h, 1 if collect_stats else 0, int(phase_limit)))

    def psd_sweeps(self):
        """Jacobi sweeps of the last PSD projection per (cone, copy) matrix (after psd_debug(True))."""
        n = C.c_int64(0)
        _lib.check(self._lib.fos_psd_stats(self._h, None, 0, C.byref(n)))
        out = np.zeros(max(1, n.value), dtype=np.int32)
        _lib.check(self._lib.fos_psd_stats(self._h, out.ctypes.data_as(C.POINTER(C.c_int32)), n.value, C.byref(n)))
        return out[:n.value]

    def psd_fused_steps(self):
        """Steps taken so far with relaxation, PSD(64) projection and the step's last pass in one launch (fos_psd_fused_steps)."""
        v = C.c_int64(0)
        _lib.check(self._lib.fos_psd_fused_steps(self._h, C.byref(v)))
        return v.value

    def bench_cg_chain(self, iters, reps=5, use_graph=False):
        """ms per CG iteration of a chain that never converges (fos_bench_cg_chain)."""
        ms = C.c_double(0)
        _lib.check(self._lib.fos_bench_cg_chain(self._h, iters, reps, 1 if use_graph else 0, C.byref(ms)))
        return ms.value

    # -- sharding; the host side hands over an ncclUniqueId obtained on rank 0
    @staticmethod
    def comm_unique_id():
        buf = (C.c_ubyte * 128)()
        _lib.check(_lib.load().fos_comm_get_unique_id(buf))
        return bytes(buf)

    def comm_init(self, nranks, rank, unique_id: bytes):
        buf = (C.c_ubyte * 128).from_buffer_copy(unique_id)
        _lib.check(self._lib.fos_comm_init(self._h, nranks, rank, buf))

    def comm_init_host(self, nranks, rank, allreduce_sum):
        """Sharding over the caller's own collective (fos_comm_init_host): `allreduce_sum(a)` must replace the float64 numpy
        array `a` by its sum over the ranks, in place, blocking -- e.g. torch.distributed.all_reduce(torch.from_numpy(a)) on
        any backend, or MPI's Allreduce."""
        def _cb(user, buf, count):
            try:
                allreduce_sum(np.ctypeslib.as_array(buf, shape=(count,)))
                return 0
            except Exception:           # noqa: BLE001 -- reported through the ABI's error code
                import traceback
                traceback.print_exc()
                return 1
        self._host_cb = _lib.ALLREDUCE_FN(_cb)          # keep the trampoline alive as long as the handle
        _lib.check(self._lib.fos_comm_init_host(self._h, nranks, rank, C.cast(self._host_cb, C.c_void_p), None))

    # -- peer mailboxes: the sharded sums without a collective call (include/foship.h, fos_peer_*)
    def peer_export(self) -> bytes:
        buf = (C.c_ubyte * 64)()
        _lib.check(self._lib.fos_peer_export(self._h, buf))
        return bytes(buf)

    def peer_open(self, nranks, rank, handles, timeout_s=0.0):
        """handles: the peer_export() bytes of every rank, in rank order."""
        blob = b"".join(handles)
        assert len(blob) == 64 * nranks
        buf = (C.c_ubyte * len(blob)).from_buffer_copy(blob)
        _lib.check(self._lib.fos_peer_open(self._h, nranks, rank, buf, float(timeout_s)))

    def peer_open_host(self, nranks, rank, shm_name, timeout_s=0.0):
        """host-pinned mailboxes (fos_peer_open_host): `shm_name` = "/something-unique-to-the-job", the same on every rank of the node;
        replaces peer_export + peer_open, then peer_selftest / peer_enable as usual."""
        _lib.check(self._lib.fos_peer_open_host(self._h, nranks, rank, shm_name.encode(), float(timeout_s)))

    def peer_close(self):
        """drop the open mailboxes (device or host) so that another transport can be opened on this handle"""
        _lib.check(self._lib.fos_peer_close(self._h))

    def peer_vec_export(self) -> bytes:
        """row-sharded handles: the exchange buffer of the n-vector A'y (after peer_open)"""
        buf = (C.c_ubyte * 64)()
        _lib.check(self._lib.fos_peer_vec_export(self._h, buf))
        return bytes(buf)

    def peer_vec_open(self, handles):
        blob = b"".join(handles)
        buf = (C.c_ubyte * len(blob)).from_buffer_copy(blob)
        _lib.check(self._lib.fos_peer_vec_open(self._h, buf))

    def peer_selftest(self, rounds=32) -> bool:
        ok = C.c_int32(0)
        _lib.check(self._lib.fos_peer_selftest(self._h, rounds, C.byref(ok)))
        return bool(ok.value)

    def exchange_bench(self, rounds=200) -> float:
        """microseconds per exchange of four doubles on the handle's transport (collective; foship.h fos_exchange_bench)."""
        us = C.c_double(0.0)
        _lib.check(self._lib.fos_exchange_bench(self._h, int(rounds), C.byref(us)))
        return float(us.value)

    def peer_enable(self, on=True):
        _lib.check(self._lib.fos_peer_enable(self._h, 1 if on else 0))


# ---------------------------------------------------------------------------------------------- status

class HSDEStatus:
    """HSDEStatus (HSDEStatus.jl:2-16): fields the outer loop reads/writes + printing + history."""

    def __init__(self, model, checki, eps, verbose, debug, out=None):
        self.model = model
        self.i = 0
        self.status = "Continue"
        self.checki, self.eps, self.verbose, self.debug = checki, eps, verbose, debug
        self.checked = False
        self.direct = False
        self.init_time = time.perf_counter_ns()
        self._out = out

    def _println(self, s):
        if self._out is None:
            print(s)
        else:
            self._out.append(s)

    def printstatusheader(self):                                   # HSDEStatus.jl:73-83
        if self.verbose > 0:
            self._println("Time to initialize: %ss" % (self.model.init_duration / 1e9))
            width = 76 + (0 if self.direct else 5)
            self._println("-" * width)
            self._println(HEADER_DIRECT if self.direct else HEADER_CG)
            self._println("-" * width)

    def record(self, res, z=None):
        """What checkstatus does once the residual scalars are known (HSDEStatus.jl:39-65)."""
        t = time.perf_counter_ns() - self.init_time
        i, h = self.i, self.model.history
        if self.debug > 0:                                         # savedata :125-139
            for key, val in (("p", res.p), ("d", res.d), ("g", res.g), ("ctx", res.ctx), ("bty", res.bty),
                             ("κ", res.kappa), ("τ", res.tau), ("t", t)):
                h.setdefault(key, []).append((i, val))
            if self.debug > 1 and z is not None:
                m, n = self.model.m, self.model.n
                nu = n + m + 1
                h.setdefault("x", []).append((i, z[0:n].copy()))
                h.setdefault("y", []).append((i, z[n:n + m].copy()))
                h.setdefault("s", []).append((i, z[nu + n:nu + n + m].copy()))
        if self.verbose > 0 and not self.direct:                   # :43-47
            h.setdefault("cgiter", []).append((i, int(res.cgiter)))
            self._println(_julia_specials("%6d|% 9.2e % 9.2e % 9.2e % 9.2e % 9.2e % 9.2e % 4d % .1es" %
                          (i, res.p, res.d, res.g, res.ctx, -res.bty, _ieee_div(res.kappa, res.tau), res.cgiter, t / 1e9)))
        elif self.verbose > 0:                                     # :48-50 (direct: no cg column, no :cgiter history)
            self._println(_julia_specials("%6d|% 9.2e % 9.2e % 9.2e % 9.2e % 9.2e % 9.2e % .1es" %
                          (i, res.p, res.d, res.g, res.ctx, -res.bty, _ieee_div(res.kappa, res.tau), t / 1e9)))
        if res.cg_maxiter_hit:
            import warnings
            warnings.warn("CG reached max iterations, result may be inaccurate")     # conjugategradients.jl:53
        if isinstance(self.model.alg, LongstepWrapper):            # (the reference's QP solver throws where no projection exists; here the step stands and the host is told)
            gu = self.model.data.longstep_log()["given_up"]
            if gu > getattr(self, "_long_given_up", 0):
                import warnings
                warnings.warn("LongstepWrapper: %d projection(s) onto the saved planes found no KKT point of the small dual within its budget "
                              "(inconsistent or dependent planes); those iterations kept the wrapped algorithm's iterate" % (gu - getattr(self, "_long_given_up", 0)))
            self._long_given_up = gu
        self.status = _lib.STATUS_NAMES[res.status]
        if self.status == "Optimal" and self.verbose > 0:
            self._println("Found solution i=%d" % i)               # :55-57
        self.checked = True
        self.last = res


class Solution:                                                    # src/types.jl:6-11
    def __init__(self, x, y, s, status):
        self.x, self.y, self.s, self.status = x, y, s, status


# ---------------------------------------------------------------------------------------------- model

class FOSMathProgModel:
    """FOSMathProgModel (src/types.jl:30-60) with the MathProgBase methods of src/FOSSolverInterface.jl."""

    def __init__(self, alg: FOSAlgorithm, device=0, **kwargs):
        self.alg = alg
        self.options = dict(alg.options)
        self.options.update(kwargs)
        self.device = device
        self.input_numconstr = 0
        self.input_numvar = 0
        self.solve_stat = "NotSolved"
        self.obj_val = 0.0
        self.primal_sol = np.zeros(0)
        self.dual_sol = np.zeros(0)
        self.slack = np.zeros(0)
        self.history = {}
        self.init_duration = 1
        self.data = None
        self.out = None            # list collecting printed lines (None -> stdout)

    # loadproblem!(model, c, A, b, constr_cones, var_cones)        FOSSolverInterface.jl:27-64
    def loadproblem(self, c, A, b, constr_cones, var_cones):
        t1 = time.perf_counter_ns()
        A = sp.csc_matrix(A)
        self.input_numconstr, self.input_numvar = A.shape
        self.m, self.n = A.shape
        self.A, self.b, self.c = A, _lib.as_f64(b, A.shape[0]), _lib.as_f64(c, A.shape[1])
        self.K1, self.K2 = list(constr_cones), list(var_cones)
        if self.data is not None:
            self.data.close()
        self.data = HipHSDE(A, self.b, self.c, self.K1, self.K2, device=self.device,     # init_algorithm!  :58
                            equilibrate=self.options.get("equilibrate", 0))              # device-side key, like cg_variant: True = 10 passes, an int = that many
        self.data.set_alg(self.alg)
        if "cg_variant" in self.options:                           # device-side key (the reference ignores unknown option keys):
            self.data.set_cg_variant(self.options["cg_variant"])   # which CG recurrence the affine projection runs (foship.h FOS_CG_*)
        if self.alg.direct:                                        # HSDE(model, direct=alg.direct)   HSDE.jl:12-15
            self.data.enable_direct(A, form=self.options.get("direct_form", "auto"),     # device-side keys, like cg_variant
                                    factor=self.options.get("direct_factor", "newton"))
        self.init_duration = time.perf_counter_ns() - t1
        return self

    def numvar(self):
        return self.input_numvar

    def numconstr(self):
        return self.input_numconstr

    @staticmethod
    def supportedcones():                                          # FOSSolverInterface.jl:69
        return ["Free", "Zero", "NonNeg", "NonPos", "SOC", "SDP", "ExpPrimal", "ExpDual"]

    # optimize!(m)                                                 FOSSolverInterface.jl:8-21
    def optimize(self):
        self.history = {}
        sol = self._solve()
        self.solve_stat = sol.status
        self.primal_sol, self.dual_sol, self.slack = sol.x, sol.y, sol.s
        self.obj_val = float(np.dot(self.c, self.primal_sol))
        return self

    def status(self):
        return self.solve_stat

    def getobjval(self):
        return self.obj_val

    def getsolution(self):
        return self.primal_sol.copy()

    # solve!(model) + iterate                                      solverwrapper.jl:2-41
    def _solve(self):
        opts = self.options
        max_iters = opts.get("max_iters", 10000)
        verbose = opts.get("verbose", 1)
        debug = opts.get("debug", 1)
        eps = opts.get("eps", 1e-5)
        checki = opts.get("checki", 100)
        dev = self.data                                            # model.data persists across optimize! calls, as in the
        dev.set_iterate(opts.get("initx", None))                   # reference (alpha12 / t / y / S1 counters carry over); :10
        status = HSDEStatus(self, checki, eps, verbose, debug, out=self.out)
        # HSDE.jl:27 -- the table drops its cg column when S1 runs no CG; beyond the sizes the exact forms cover, direct = true is the same
        # projection by CG at its tolerance floor (fos_enable_direct): the column stays, the iterations are real
        status.direct = bool(self.alg.direct) and self.data.direct_mode() in ("dense", "block", "reduced")
        self.status_obj = status
        t1 = time.time()
        status.printstatusheader()
        i = 0
        ls = self.alg.lsinterval if isinstance(self.alg, LineSearchWrapper) else 0
        gp = self.alg.iproj if isinstance(self.alg, GAPP) else 0
        while i < max_iters:                                       # for i = 1:max_iters   :23
            count = min(max_iters - i, checki - (i % checki))
            if ls > 0:
                count = min(count, ls - (i % ls))                  # stop at every line-search iteration: its output is printed
            if gp > 0:
                count = min(count, gp - (i % gp))
            done, checked, res = dev.step(i + 1, count, checki, eps)
            i += done
            status.i = i
            if gp > 0 and i % gp == 0:                             # what gapproj.jl:51,57 print (unconditionally)
                _, tests, abest = dev.gapp_log()
                for nt in tests:
                    status._println("normtest: %s" % julia_float(nt))
                status._println("\u03b1best: %s" % julia_float(abest))
            if ls > 0 and i % ls == 0:                             # what linesearch.jl:51,63,69 print
                _, normres, tests, abest = dev.linesearch_log()
                status._println("test, %s" % julia_float(normres))
                a = 0.1
                for tr in tests:
                    a = a * 1.8
                    status._println("\u03b1: %s, %s" % (julia_float(a), julia_float(tr)))
                status._println("\u03b1: %s" % julia_float(abest))
            if checked:
                z = dev.get_checked() if debug > 1 else None      # debug=2 stores x,y,s of the checked point
                status.record(res, z)
                if status.status != "Continue":                    # :26
                    break
            else:
                status.checked = False
        guess, res = dev.getsol(force_check=not status.checked, eps=eps)       # :31-34
        if not status.checked:
            status.record(res, guess)
        if verbose > 0:                                            # :35-39
            status._println("Time for iterations: ")
            status._println("%s s" % (time.time() - t1))
        self.iterations = i
        self.guess = guess
        # HSDE_populatesolution                                    HSDE.jl:49-61
        m, n = self.m, self.n
        l = m + n + 1
        tau = guess[l - 1]
        endstatus = status.status if status.status != "Continue" else "Indeterminate"
        with np.errstate(divide="ignore", invalid="ignore"):
            return Solution(guess[0:n] / tau, guess[n:n + m] / tau, guess[l + n:l + n + m] / tau, endstatus)


def solve(problem, alg, device=0, out=None):
    """Convenience: ConicModel(alg) -> loadproblem! -> optimize!  for a workloads.ConicProblem."""
    model = FOSMathProgModel(alg, device=device)
    model.out = out
    model.loadproblem(problem.c, problem.A, problem.b, problem.K1, problem.K2)
    model.optimize()
    return model


# ---------------------------------------------------------------------------------------------- Feasibility form
# src/problemforms/Feasibility/Feasibility.jl, FeasibilityStatus.jl.  The reference takes any two
# ProximalOperators objects; the device path takes the two set types below (the ones test/testfeasibility.jl uses).

class IndAffine:
    """ProximalOperators.IndAffine(A, b): {x : A x = b}, A m x n of full row rank.  A dense A (n <= 46 000) becomes a dense projector on the
    device (fos_feas_set_affine); a scipy.sparse A stays sparse at any n (fos_feas_set_affine_sparse: warm-started CG on the row-scaled normal
    equations, ended by the recomputed residual) -- `sparse=True / False` forces either form.
    form="factored" (opt-in; form=None keeps the selection above to the letter): the dense A is kept once on the device with the inverse of A A'
    (order m <= 46 000, any n) and a projection is two passes over A (fos_feas_set_affine_factored); factor = "cholesky" | "newton" builds the
    inverse, refine = 0..2 refinement steps follow every projection.  A scipy.sparse A is densified.
    form="sparse_factored" (opt-in): A stays sparse (CSC on the host, two CSR matrices on the device) with the dense inverse of A A' (order m <= 46 000, any n);
    a projection is two segmented sparse passes and three products of order m, a fixed number of launches whatever cond(A A')
    (fos_feas_set_affine_sparse_factored); factor and refine as for form="factored"."""

    DENSE_MAX = 46000
    FACTORED_MAX = 46000

    def __init__(self, A, b, sparse=None, form=None, factor="cholesky", refine=0):
        if form not in (None, "factored", "sparse_factored"):
            raise ValueError("IndAffine: form must be None, 'factored' or 'sparse_factored', not %r" % (form,))
        self.form, self.factor, self.refine = form, factor, int(refine)
        if form is not None:
            if form == "factored" and sparse:
                raise ValueError("IndAffine: form='factored' keeps a dense A (sparse=True asks for the sparse form)")
            if form == "sparse_factored" and sparse is not None and not sparse:
                raise ValueError("IndAffine: form='sparse_factored' keeps a sparse A (sparse=False asks for a dense form)")
            direct_factor_code(factor)
            if not 0 <= self.refine <= 2:
                raise ValueError("IndAffine: refine must be 0, 1 or 2, not %r" % (refine,))
            self.sparse = form == "sparse_factored"
        else:
            self.sparse = bool(sp.issparse(A) or np.shape(A)[1] > self.DENSE_MAX) if sparse is None else bool(sparse)
        if self.sparse:
            self.A = sp.csc_matrix(A, dtype=np.float64)
            self.A.sum_duplicates(); self.A.sort_indices()
        else:
            self.A = np.ascontiguousarray(A.toarray() if sp.issparse(A) else np.asarray(A, dtype=np.float64))
        self.b = np.ascontiguousarray(np.asarray(b, dtype=np.float64))
        if self.A.ndim != 2 or self.b.shape != (self.A.shape[0],):
            raise ValueError("IndAffine(A, b): A must be m x n and b of length m")
        if form is not None and self.A.shape[0] > self.FACTORED_MAX:
            raise ValueError("IndAffine(form=%r): m = %d, the inverse of A A' is supported up to m = %d" % (form, self.A.shape[0], self.FACTORED_MAX))


class IndBox:
    """ProximalOperators.IndBox(lo, hi): {x : lo <= x <= hi}, scalar or array bounds (+-inf allowed)."""

    def __init__(self, lo, hi):
        self.arrays = np.ndim(lo) > 0 or np.ndim(hi) > 0
        if self.arrays:
            self.lo, self.hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
        else:
            self.lo, self.hi = float(lo), float(hi)


class ConeProduct:
    """FirstOrderSolvers.ConeProduct (src/cones.jl:31-94) as a set of the Feasibility form: cones = [(name, length), ...] with the
    names of `conemap` (cones.jl:4-14: Free, Zero, NonNeg, NonPos, SOC, SOCRotated, SDP, ExpPrimal, ExpDual), in order, contiguous."""

    def __init__(self, cones):
        self.cones = [(str(k), int(l)) for k, l in cones]
        for k, _ in self.cones:
            if k not in _lib.CONE_CODES:
                raise ValueError("unknown cone %r (supportedcones: %s)" % (k, ", ".join(_lib.CONE_CODES)))


# Convex vector sets projected by the kernels of csrc/sets.hip (fos_feas_set_blocks).  Parameter holders like IndBox: validation, no arithmetic.
# ProximalOperators.jl's definitions: the projection of each is stated in its docstring.

def _finite_scalar(name, v):
    v = float(v)
    if not np.isfinite(v):
        raise ValueError("%s must be finite, got %r" % (name, v))
    return v


def _finite_vector(name, v):
    v = np.ascontiguousarray(np.asarray(v, dtype=np.float64))
    if v.ndim != 1 or v.size < 1 or not np.all(np.isfinite(v)):
        raise ValueError("%s must be a non-empty vector of finite numbers" % name)
    return v


class _VectorSet:
    """One block of a SeparableSum: `kind` (a key of _lib.SET_CODES), the two scalars and the vector fos_feas_set_blocks takes for it."""
    kind, scal, vec = "IndFree", (0.0, 0.0), None

    def _block(self, length):
        if self.vec is not None and self.vec.shape[0] != length:
            raise ValueError("%s: its vector has %d entries, the block has %d" % (self.kind, self.vec.shape[0], length))
        return _lib.SET_CODES[self.kind], self.scal, self.vec


class IndBallL2(_VectorSet):
    """{x : |x - c|_2 <= r}.  d = x - c: y = x if |d| <= r, else c + d (r / |d|)."""
    kind = "IndBallL2"

    def __init__(self, r=1.0, center=None):
        self.r = _finite_scalar("IndBallL2: r", r)
        if self.r < 0.0:
            raise ValueError("IndBallL2: r >= 0 is required")
        self.center = self.vec = None if center is None else _finite_vector("IndBallL2: center", center)
        self.scal = (self.r, 0.0)


class IndBallL1(_VectorSet):
    """{x : |x|_1 <= r}.  y = x if |x|_1 <= r, else sign(x) max(|x| - tau, 0) with sum max(|x_i| - tau, 0) = r."""
    kind = "IndBallL1"

    def __init__(self, r=1.0):
        self.r = _finite_scalar("IndBallL1: r", r)
        if self.r < 0.0:
            raise ValueError("IndBallL1: r >= 0 is required")
        self.scal = (self.r, 0.0)


class IndSimplex(_VectorSet):
    """{x : x >= 0, sum x = a}.  y = max(x - tau, 0) with sum max(x_i - tau, 0) = a (always thresholded; tau may be negative)."""
    kind = "IndSimplex"

    def __init__(self, a=1.0):
        self.a = _finite_scalar("IndSimplex: a", a)
        if not self.a > 0.0:
            raise ValueError("IndSimplex: a > 0 is required")
        self.scal = (self.a, 0.0)


class IndHalfspace(_VectorSet):
    """{x : <a, x> <= b}.  y = x - max(0, (<a, x> - b) / <a, a>) a."""
    kind = "IndHalfspace"

    def __init__(self, a, b):
        self.a = self.vec = _finite_vector("IndHalfspace: a", a)
        if not np.any(self.a != 0.0):
            raise ValueError("IndHalfspace: the normal vector is zero")
        self.b = _finite_scalar("IndHalfspace: b", b)
        self.scal = (self.b, 0.0)


class IndHyperslab(_VectorSet):
    """{x : lo <= <a, x> <= hi}.  The halfspace's projection, towards whichever side is violated."""
    kind = "IndHyperslab"

    def __init__(self, lo, a, hi):
        self.a = self.vec = _finite_vector("IndHyperslab: a", a)
        if not np.any(self.a != 0.0):
            raise ValueError("IndHyperslab: the normal vector is zero")
        self.lo, self.hi = _finite_scalar("IndHyperslab: lo", lo), _finite_scalar("IndHyperslab: hi", hi)
        if self.lo > self.hi:
            raise ValueError("IndHyperslab: lo <= hi is required")
        self.scal = (self.lo, self.hi)


class IndPoint(_VectorSet):
    """{p}.  y = p."""
    kind = "IndPoint"

    def __init__(self, p):
        self.p = self.vec = _finite_vector("IndPoint: p", p)


class IndFree(_VectorSet):
    """R^k.  y = x."""
    kind = "IndFree"


# Proximable functions that are not indicators, on the same kernels (kind codes _lib.FN_CODES, from 32): the block's "projection" is prox_f(x), step 1.

def _nonneg_scalar(name, v):
    v = _finite_scalar(name, v)
    if v < 0.0:
        raise ValueError("%s >= 0 is required" % name)
    return v


class _ProxFunction(_VectorSet):
    """One block of a SeparableSum that is a function: `kind` is a key of _lib.FN_CODES."""

    def _block(self, length):
        if self.vec is not None and self.vec.shape[0] != length:
            raise ValueError("%s: its vector has %d entries, the block has %d" % (self.kind, self.vec.shape[0], length))
        return _lib.FN_CODES[self.kind], self.scal, self.vec


class NormL1(_ProxFunction):
    """f(x) = lam |x|_1.  y = sign(x) max(|x| - lam, 0)."""
    kind = "NormL1"

    def __init__(self, lam=1.0):
        self.lam = _nonneg_scalar("NormL1: lam", lam)
        self.scal = (self.lam, 0.0)


class SqrNormL2(_ProxFunction):
    """f(x) = lam/2 |x|_2^2.  y = x / (1 + lam)."""
    kind = "SqrNormL2"

    def __init__(self, lam=1.0):
        self.lam = _nonneg_scalar("SqrNormL2: lam", lam)
        self.scal = (self.lam, 0.0)


class ElasticNet(_ProxFunction):
    """f(x) = mu |x|_1 + lam/2 |x|_2^2.  y = sign(x) max(|x| - mu, 0) / (1 + lam)."""
    kind = "ElasticNet"

    def __init__(self, mu=1.0, lam=1.0):
        self.mu, self.lam = _nonneg_scalar("ElasticNet: mu", mu), _nonneg_scalar("ElasticNet: lam", lam)
        self.scal = (self.mu, self.lam)


class Linear(_ProxFunction):
    """f(x) = <c, x>.  y = x - c."""
    kind = "Linear"

    def __init__(self, c):
        self.c = self.vec = _finite_vector("Linear: c", c)


class NormL2(_ProxFunction):
    """f(x) = lam |x|_2.  y = max(0, 1 - lam / |x|) x; zeros when |x| <= lam."""
    kind = "NormL2"

    def __init__(self, lam=1.0):
        self.lam = _nonneg_scalar("NormL2: lam", lam)
        self.scal = (self.lam, 0.0)


class HuberLoss(_ProxFunction):
    """f(x) = mu/2 |x|^2 if |x|_2 <= rho, else rho mu (|x| - rho/2).  y = x / (1 + mu) if |x| <= rho (1 + mu), else (1 - rho mu / |x|) x."""
    kind = "HuberLoss"

    def __init__(self, rho=1.0, mu=1.0):
        self.rho, self.mu = _finite_scalar("HuberLoss: rho", rho), _nonneg_scalar("HuberLoss: mu", mu)
        if not self.rho > 0.0:
            raise ValueError("HuberLoss: rho > 0 is required")
        self.scal = (self.rho, self.mu)


class NormLinf(_ProxFunction):
    """f(x) = lam |x|_inf.  y = x - P(x), P the projection onto {|.|_1 <= lam}: zeros when |x|_1 <= lam, else sign(x) min(|x|, tau) with IndBallL1(lam)'s tau."""
    kind = "NormLinf"

    def __init__(self, lam=1.0):
        self.lam = _nonneg_scalar("NormLinf: lam", lam)
        self.scal = (self.lam, 0.0)


def _cg_tol(name, tol, form):
    """the relative stop of form="cg": a number in [0, 1); any other form takes none"""
    tol = _finite_scalar(name + ": tol", tol)
    if not 0.0 <= tol < 1.0:
        raise ValueError("%s: tol must be in [0, 1)" % name)
    if tol != 0.0 and form != "cg":
        raise ValueError("%s: tol belongs to form='cg'" % name)
    return tol


class LeastSquares:
    """f(x) = lam/2 |A x - b|^2 with a dense A (m x n, 1 <= m <= n, m <= 46 000; rank-deficient and zero rows allowed), lam > 0.  The prox
    y = x - A'(A A' + I/lam)^-1 (A x - b) runs on the factored form of IndAffine with the diagonal of A A' shifted (fos_feas_set_least_squares): two passes
    over A per prox, a fixed number of launches.  factor = "cholesky" | "newton" builds the inverse.  m > n, m > 46 000 or a sparse A: pass an object with
    a prox(y, x) method instead (the host-callback path), or opt in to one of the forms below (form=None keeps all of the above to the letter).
    form="normal": the normal-equations form in the n-space, y = (I + lam A'A)^-1 (x + lam A'b), for a dense or scipy-sparse A of ANY m with n <= 46 000
    (fos_feas_set_least_squares_normal / _sparse): I + lam A'A and its inverse are kept as packed triangles, a prox is three tile products, six launches.
    form="sparse_factored": a scipy-sparse A with m <= min(n, 46 000) stays sparse, with the dense inverse of A A' + I/lam (fos_feas_set_least_squares_sparse): the
    sparse factored IndAffine with a shifted diagonal; zero and dependent rows are accepted.
    form="cg": a scipy-sparse A (a dense A is converted) of ANY m and n, nothing dense kept: y = (I + lam A'A)^-1 (x + lam A'b) by warm-started Jacobi-preconditioned
    CG on the device (fos_feas_set_least_squares_cg), three launches per iteration, ended on the recomputed residual at max(tol |x + lam A'b|, its rounding level)."""

    MAX_M = 46000
    MAX_N = 46000

    def __init__(self, A, b, lam=1.0, factor="cholesky", form=None, tol=0.0):
        self.lam = _finite_scalar("LeastSquares: lam", lam)
        if not self.lam > 0.0:
            raise ValueError("LeastSquares: lam > 0 is required")
        direct_factor_code(factor)
        self.factor = factor
        if form not in (None, "normal", "sparse_factored", "cg"):
            raise ValueError("LeastSquares: form must be None, 'normal', 'sparse_factored' or 'cg', not %r" % (form,))
        self.form = form
        self.tol = _cg_tol("LeastSquares", tol, form)
        if form == "cg" and not sp.issparse(A):
            A = sp.csc_matrix(np.atleast_2d(np.asarray(A, dtype=np.float64)))
        self.sparse = form is not None and bool(sp.issparse(A))
        if form == "sparse_factored" and not self.sparse:
            raise ValueError("LeastSquares: form='sparse_factored' keeps a scipy.sparse A")
        if self.sparse:
            self.A = sp.csc_matrix(A, dtype=np.float64)
            self.A.sum_duplicates(); self.A.sort_indices()
            self.b = np.ascontiguousarray(np.asarray(b, dtype=np.float64))
            m, n = self.A.shape
            if m < 1 or n < 1 or self.b.shape != (m,):
                raise ValueError("LeastSquares(A, b): A must be m x n and b of length m")
            if not (np.all(np.isfinite(self.A.data)) and np.all(np.isfinite(self.b))):
                raise ValueError("LeastSquares(A, b): A and b must be finite")
            if form == "normal" and n > self.MAX_N:
                raise ValueError("LeastSquares(form='normal'): n = %d, the inverse of I + lam A'A is supported up to n = %d" % (n, self.MAX_N))
            if form == "sparse_factored" and (m > n or m > self.MAX_M):
                raise ValueError("LeastSquares(form='sparse_factored'): m = %d, n = %d: 1 <= m <= min(n, %d) is required" % (m, n, self.MAX_M))
            return
        if sp.issparse(A):
            raise ValueError("LeastSquares: A must be dense (a sparse A: an object with a prox(y, x) method, evaluated on the host)")
        self.A = np.ascontiguousarray(np.asarray(A, dtype=np.float64))
        self.b = np.ascontiguousarray(np.asarray(b, dtype=np.float64))
        if self.A.ndim != 2 or self.A.shape[0] < 1 or self.b.shape != (self.A.shape[0],):
            raise ValueError("LeastSquares(A, b): A must be m x n and b of length m")
        if not (np.all(np.isfinite(self.A)) and np.all(np.isfinite(self.b))):
            raise ValueError("LeastSquares(A, b): A and b must be finite")
        if form == "normal" and self.A.shape[1] > self.MAX_N:
            raise ValueError("LeastSquares(form='normal'): n = %d, the inverse of I + lam A'A is supported up to n = %d" % (self.A.shape[1], self.MAX_N))


class Quadratic:
    """ProximalOperators.Quadratic(Q, q): f(x) = 1/2 x'Qx + q'x with a dense symmetric positive semidefinite Q of order n <= 46 000.  The prox
    y = (I + Q)^-1 (x - q) runs in the n-space (fos_feas_set_quadratic): I + Q, scaled to a unit diagonal, and its inverse are kept as packed triangles and a prox is
    three tile products, six launches.  ONLY THE LOWER TRIANGLE of Q is read (Q[i, j], i >= j): there is no symmetry test.  factor = "cholesky" | "newton" builds
    the inverse; a Q that is not positive semidefinite is refused at set-up with the column of the failed pivot.  Feasibility(Quadratic(Q, q), IndBox(lo, hi), n)
    under DR is the box-constrained QP.
    form="cg": a scipy-sparse Q (a dense Q is converted) of ANY order, nothing dense kept: y = (I + Q)^-1 (x - q) by warm-started Jacobi-preconditioned CG on the device
    (fos_feas_set_quadratic_sparse), two launches per iteration, ended on the recomputed residual at max(tol |x - q|, its rounding level).  Only the entries i >= j are
    read; a Q that is not positive semidefinite is refused at set-up (1 + Q[i, i] <= 0) or by the prox that meets p'(I + Q)p <= 0."""

    MAX_N = 46000

    def __init__(self, Q, q, factor="cholesky", form=None, tol=0.0):
        direct_factor_code(factor)
        self.factor = factor
        if form not in (None, "cg"):
            raise ValueError("Quadratic: form must be None or 'cg', not %r" % (form,))
        self.form = form
        self.tol = _cg_tol("Quadratic", tol, form)
        if form == "cg":
            self.Q = sp.csc_matrix(Q if sp.issparse(Q) else np.atleast_2d(np.asarray(Q, dtype=np.float64)), dtype=np.float64)
            self.Q.sum_duplicates(); self.Q.sort_indices()
            self.q = np.ascontiguousarray(np.asarray(q, dtype=np.float64))
            if self.Q.shape[0] < 1 or self.Q.shape[0] != self.Q.shape[1] or self.q.shape != (self.Q.shape[0],):
                raise ValueError("Quadratic(Q, q): Q must be n x n and q of length n")
            if not (np.all(np.isfinite(self.Q.data)) and np.all(np.isfinite(self.q))):
                raise ValueError("Quadratic(Q, q): Q and q must be finite")
            return
        if sp.issparse(Q):
            raise ValueError("Quadratic: Q must be dense")
        self.Q = np.ascontiguousarray(np.asarray(Q, dtype=np.float64))
        self.q = np.ascontiguousarray(np.asarray(q, dtype=np.float64))
        if self.Q.ndim != 2 or self.Q.shape[0] < 1 or self.Q.shape[0] != self.Q.shape[1] or self.q.shape != (self.Q.shape[0],):
            raise ValueError("Quadratic(Q, q): Q must be n x n and q of length n")
        if self.Q.shape[0] > self.MAX_N:
            raise ValueError("Quadratic: n = %d, the inverse of I + Q is supported up to n = %d" % (self.Q.shape[0], self.MAX_N))
        if not (np.all(np.isfinite(np.tril(self.Q))) and np.all(np.isfinite(self.q))):
            raise ValueError("Quadratic(Q, q): Q and q must be finite")


class SeparableSum:
    """The analogue of ProximalOperators.SlicedSeparableSum over index ranges, in the style of ConeProduct: blocks = [(set, length), ...], contiguous, in
    order, together covering 1..n.  A set is one of IndBallL2, IndBallL1, IndSimplex, IndHalfspace, IndHyperslab, IndPoint, IndFree, an IndBox with
    scalar bounds (cones stay in ConeProduct), or one of the functions NormL1, SqrNormL2, ElasticNet, Linear, NormL2, HuberLoss, NormLinf, whose block
    is their prox; sets and functions mix freely.  A bare set or function used as S1 or S2 is the one-block case of length n.
    Dense blocks: a dense Quadratic(Q, q) (form=None), LeastSquares(A, b, lam) (form=None | "normal") or IndAffine(A, b) (form=None | "factored") of order
    length == p <= 1024 is a block like any other (csrc/dense_blocks.hip: y = G x + d with G built once per distinct matrix).  Blocks built on the SAME ndarray
    (Quadratic(Q, q_t) for many q_t) share one matrix on the device.  A sum with a dense block is packed by pack2 and set by fos_feas_set_blocks2.
    Dense blocks are opt-in, SeparableSum(blocks, dense=True): without the keyword the three types are refused as before (form=None keeps every earlier refusal)."""

    DENSE_MAX = 1024

    @staticmethod
    def _dense_block(S, length, k):
        """the dense block S of `length` entries as (kind code, matrix, vector, lambda), or None when S is no Quadratic / LeastSquares / IndAffine"""
        if isinstance(S, Quadratic):
            name, M, v, lam, forms = "Quadratic", S.Q, S.q, 0.0, (None,)
        elif isinstance(S, LeastSquares):
            name, M, v, lam, forms = "LeastSquares", S.A, S.b, S.lam, (None, "normal")
        elif isinstance(S, IndAffine):
            name, M, v, lam, forms = "IndAffine", S.A, S.b, 0.0, (None, "factored")
        else:
            return None
        if S.form not in forms:
            raise ValueError("SeparableSum: block %d: %s(form=%r) is no dense block (form must be one of %s)" % (k, name, S.form, ", ".join(repr(f) for f in forms)))
        if sp.issparse(M) or getattr(S, "sparse", False):
            raise ValueError("SeparableSum: block %d: a %s block takes a dense matrix, not a sparse one" % (k, name))
        if M.shape[1] != length:
            raise ValueError("SeparableSum: block %d: the matrix of %s has %d columns, the block has %d entries" % (k, name, M.shape[1], length))
        if length > SeparableSum.DENSE_MAX:
            raise ValueError("SeparableSum: block %d: a dense %s block holds at most %d entries, not %d (use the whole-vector form)" % (k, name, SeparableSum.DENSE_MAX, length))
        if name == "IndAffine" and M.shape[0] > length:
            raise ValueError("SeparableSum: block %d: IndAffine needs m <= p, A is %d x %d" % (k, M.shape[0], M.shape[1]))
        return _lib.BLK_CODES[name], M, v, lam

    def __init__(self, blocks, dense=False):
        self.blocks = []
        self.dense = False
        if not dense:                                                   # opt-in: without it a Quadratic / LeastSquares / IndAffine is refused as it always was
            for k, (S, _) in enumerate(blocks):
                if isinstance(S, (Quadratic, LeastSquares, IndAffine)):
                    raise ValueError("SeparableSum: block %d is %s: not one of the vector sets or functions of the device path (a dense one of order <= %d is a "
                                     "block of SeparableSum(blocks, dense=True))" % (k + 1, type(S).__name__, self.DENSE_MAX))
        for S, length in blocks:
            length = int(length)
            if length < 1:
                raise ValueError("SeparableSum: block %d has length %d < 1" % (len(self.blocks) + 1, length))
            if self._dense_block(S, length, len(self.blocks) + 1) is not None:
                self.dense = True
            elif isinstance(S, IndBox):
                if S.arrays:
                    raise ValueError("SeparableSum: block %d: an IndBox inside a SeparableSum takes scalar bounds" % (len(self.blocks) + 1))
                if not S.lo <= S.hi:
                    raise ValueError("SeparableSum: block %d: IndBox needs lo <= hi" % (len(self.blocks) + 1))
            elif not isinstance(S, _VectorSet):
                raise ValueError("SeparableSum: block %d is %s: not one of the vector sets or functions of the device path" % (len(self.blocks) + 1, type(S).__name__))
            else:
                S._block(length)                                       # (the length of its vector)
            self.blocks.append((S, length))
        if not self.blocks:
            raise ValueError("SeparableSum: at least one block is required")
        self.n = sum(l for _, l in self.blocks)

    def pack(self, n):
        """-> (kind[nblocks] int32, len[nblocks] int64, scal[2 nblocks], vec[n]): the arguments of fos_feas_set_blocks"""
        if self.dense:
            raise ValueError("SeparableSum: the sum holds a dense block: pack2 returns the arguments of fos_feas_set_blocks2")
        return self._pack(n)[:4]

    def pack2(self, n):
        """-> (kind, len, scal, vec, mats, block_mat, block_vec): the arguments of fos_feas_set_blocks2.  mats: the distinct matrices (float64, C order), found by
        identity of the ndarray plus kind and lambda; block_mat[nblocks] int64: the block's index into mats, -1 for a vector kind; block_vec[nblocks]: q or b, None."""
        return self._pack(n)

    def _pack(self, n):
        if self.n != n:
            raise ValueError("SeparableSum: the blocks cover %d entries, the problem has n = %d" % (self.n, n))
        kinds, lens = np.zeros(len(self.blocks), dtype=np.int32), np.zeros(len(self.blocks), dtype=np.int64)
        scal, vec = np.zeros(2 * len(self.blocks)), np.zeros(n)
        mats, seen, block_mat, block_vec = [], {}, np.full(len(self.blocks), -1, dtype=np.int64), [None] * len(self.blocks)
        pos = 0
        for i, (S, length) in enumerate(self.blocks):
            dense = self._dense_block(S, length, i + 1)
            if dense is not None:
                kinds[i], M, block_vec[i], scal[2 * i] = dense
                key = (id(M), int(kinds[i]), float(scal[2 * i]))
                if key not in seen:
                    seen[key] = len(mats)
                    mats.append(M)
                block_mat[i] = seen[key]
            elif isinstance(S, IndBox):
                kinds[i], scal[2 * i], scal[2 * i + 1] = _lib.SET_CODES["IndBox"], S.lo, S.hi
            else:
                kinds[i], (scal[2 * i], scal[2 * i + 1]), v = S._block(length)
                if v is not None:
                    vec[pos:pos + length] = v
            lens[i] = length
            pos += length
        return kinds, lens, scal, vec, mats, block_mat, block_vec


PROX_FN = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_int64, C.POINTER(C.c_double), C.POINTER(C.c_double))     # fos_prox_fn


class Feasibility:
    """struct Feasibility{T1,T2}(S1, S2, n)   Feasibility.jl:2-6.  S1, S2: IndAffine, IndBox, ConeProduct, a vector set (IndBallL2, IndBallL1,
    IndSimplex, IndHalfspace, IndHyperslab, IndPoint, IndFree), a separable function (NormL1, SqrNormL2, ElasticNet, Linear, NormL2, HuberLoss,
    NormLinf) or a SeparableSum of them, LeastSquares(A, b, lam) with a dense A, Quadratic(Q, q), LeastSquares(form="normal" | "sparse_factored") for a tall or sparse A, Quadratic / LeastSquares(form="cg") for a sparse Q / A of any size (all device resident: Feasibility(LeastSquares(A, b, lam), NormL1(mu), n)
    under DR is the lasso, with no host round trip), or any
    object with a `prox(y, x)` method filling y = prox_S(x) in place (the ProximableFunction protocol; evaluated on the host)."""

    def __init__(self, S1, S2, n):
        self.S1, self.S2, self.n = S1, S2, int(n)


class FeasibilitySolution:
    """mutable struct FeasibilitySolution   Feasibility.jl:8-11"""

    def __init__(self, x, status):
        self.x, self.status = x, status


def _csc_one_based(A):
    """the arrays of a scipy CSC matrix as the sparse fos_feas_set_* entries take them (Julia's SparseMatrixCSC{Float64,Int64}: 1-based), and the int64 pointer cast"""
    i64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
    colptr = np.ascontiguousarray(A.indptr, dtype=np.int64) + 1
    rowval = np.ascontiguousarray(A.indices, dtype=np.int64) + 1
    return i64, colptr, rowval, np.ascontiguousarray(A.data, dtype=np.float64)


class HipFeasibility(_WrapperLogs):
    """The device handle of a Feasibility problem (fos_feas_*): both sets, the algorithm's vectors and the status state."""
    _log_prefix = "fos_feas_"

    def __init__(self, problem: Feasibility, device=0):
        self.n = problem.n
        packed = {}                                                     # the vector sets are checked against n before any device call
        for which, S in ((1, problem.S1), (2, problem.S2)):
            if isinstance(S, _VectorSet):
                S = SeparableSum([(S, self.n)])
            if isinstance(S, SeparableSum):
                packed[which] = S.pack2(self.n) if S.dense else S.pack(self.n)
        self._lib = _lib.load()
        h = C.c_void_p()
        _lib.check(self._lib.fos_feas_create(self.n, device, C.byref(h)))
        self._h = h
        self._callbacks = []
        self.callback_error = None
        for which, S in ((1, problem.S1), (2, problem.S2)):
            if which in packed:                                         # before the `prox` test: these never become callbacks
                (self.set_blocks2 if len(packed[which]) > 4 else self.set_blocks)(which, *packed[which])
            else:
                self.set_set(which, S)

    def set_set(self, which, S):
        """set `which` (1 | 2) becomes S: an IndAffine, LeastSquares, Quadratic (any form), IndBox, ConeProduct or an object with a prox(y, x) method; replaces what was there"""
        if isinstance(S, Quadratic) and S.form == "cg":
            if S.Q.shape[0] != self.n:
                raise ValueError("Quadratic: Q has order %d, the problem has n = %d" % (S.Q.shape[0], self.n))
            i64, colptr, rowval, nzval = _csc_one_based(S.Q)
            _lib.check(self._lib.fos_feas_set_quadratic_sparse(self._h, which, i64(colptr), i64(rowval), _lib.dptr(nzval), _lib.dptr(S.q), S.tol))
        elif isinstance(S, Quadratic):
            if S.Q.shape[0] != self.n:
                raise ValueError("Quadratic: Q has order %d, the problem has n = %d" % (S.Q.shape[0], self.n))
            _lib.check(self._lib.fos_feas_set_quadratic(self._h, which, _lib.dptr(S.Q), _lib.dptr(S.q), direct_factor_code(S.factor)))
        elif isinstance(S, LeastSquares) and S.form is not None:
            if S.A.shape[1] != self.n:
                raise ValueError("LeastSquares: A has %d columns, the problem has n = %d" % (S.A.shape[1], self.n))
            if S.form == "cg":
                i64, colptr, rowval, nzval = _csc_one_based(S.A)
                _lib.check(self._lib.fos_feas_set_least_squares_cg(self._h, which, S.A.shape[0], i64(colptr), i64(rowval), _lib.dptr(nzval), _lib.dptr(S.b), S.lam, S.tol))
            elif S.sparse:
                i64, colptr, rowval, nzval = _csc_one_based(S.A)
                _lib.check(self._lib.fos_feas_set_least_squares_sparse(self._h, which, S.A.shape[0], i64(colptr), i64(rowval), _lib.dptr(nzval), _lib.dptr(S.b), S.lam,
                                                                       _lib.LS_FORM_CODES[S.form], direct_factor_code(S.factor)))
            else:
                _lib.check(self._lib.fos_feas_set_least_squares_normal(self._h, which, S.A.shape[0], _lib.dptr(S.A), _lib.dptr(S.b), S.lam, direct_factor_code(S.factor)))
        elif isinstance(S, LeastSquares):
            if S.A.shape[1] != self.n:
                raise ValueError("LeastSquares: A has %d columns, the problem has n = %d" % (S.A.shape[1], self.n))
            _lib.check(self._lib.fos_feas_set_least_squares(self._h, which, S.A.shape[0], _lib.dptr(S.A), _lib.dptr(S.b), S.lam, direct_factor_code(S.factor)))
        elif isinstance(S, IndAffine):
            if S.A.shape[1] != self.n:
                raise ValueError("IndAffine: A has %d columns, the problem has n = %d" % (S.A.shape[1], self.n))
            if S.form == "factored":
                _lib.check(self._lib.fos_feas_set_affine_factored(self._h, which, S.A.shape[0], _lib.dptr(S.A), _lib.dptr(S.b), direct_factor_code(S.factor), S.refine))
            elif S.sparse:
                i64, colptr, rowval, nzval = _csc_one_based(S.A)
                if S.form == "sparse_factored":
                    _lib.check(self._lib.fos_feas_set_affine_sparse_factored(self._h, which, S.A.shape[0], i64(colptr), i64(rowval), _lib.dptr(nzval), _lib.dptr(S.b),
                                                                             direct_factor_code(S.factor), S.refine))
                else:
                    _lib.check(self._lib.fos_feas_set_affine_sparse(self._h, which, S.A.shape[0], i64(colptr), i64(rowval), _lib.dptr(nzval), _lib.dptr(S.b)))
            else:
                _lib.check(self._lib.fos_feas_set_affine(self._h, which, S.A.shape[0], _lib.dptr(S.A), _lib.dptr(S.b)))
        elif isinstance(S, IndBox) and S.arrays:
            lo = np.ascontiguousarray(np.broadcast_to(S.lo, (self.n,)), dtype=np.float64)
            hi = np.ascontiguousarray(np.broadcast_to(S.hi, (self.n,)), dtype=np.float64)
            _lib.check(self._lib.fos_feas_set_box_arrays(self._h, which, _lib.dptr(lo), _lib.dptr(hi)))
        elif isinstance(S, IndBox):
            _lib.check(self._lib.fos_feas_set_box(self._h, which, S.lo, S.hi))
        elif isinstance(S, ConeProduct):
            types = np.ascontiguousarray([_lib.CONE_CODES[k] for k, _ in S.cones], dtype=np.int32)
            lens = np.ascontiguousarray([l for _, l in S.cones], dtype=np.int64)
            _lib.check(self._lib.fos_feas_set_cones(self._h, which, len(S.cones), types.ctypes.data_as(C.POINTER(C.c_int32)),
                                                    lens.ctypes.data_as(C.POINTER(C.c_int64))))
        elif callable(getattr(S, "prox", None)):                    # any other ProximableFunction: prox!(y, S, x) as a host callback
            self.set_callback(which, S)
        else:
            raise _lib.FosError(-4, "Feasibility: set %d must be IndAffine, IndBox, ConeProduct or an object with a prox(y, x) method "
                                    "(evaluated on the host through fos_feas_set_callback), got %s" % (which, type(S).__name__))

    def set_blocks(self, which, kinds, lens, scal, vec):
        """fos_feas_set_blocks with raw arrays (SeparableSum.pack): replaces set `which`"""
        kinds, lens = np.ascontiguousarray(kinds, dtype=np.int32), np.ascontiguousarray(lens, dtype=np.int64)
        scal = np.ascontiguousarray(scal, dtype=np.float64)
        vec = None if vec is None else np.ascontiguousarray(vec, dtype=np.float64)
        _lib.check(self._lib.fos_feas_set_blocks(self._h, which, len(kinds), kinds.ctypes.data_as(C.POINTER(C.c_int32)), lens.ctypes.data_as(C.POINTER(C.c_int64)),
                                                 _lib.dptr(scal), None if vec is None else _lib.dptr(vec)))

    def set_blocks2(self, which, kinds, lens, scal, vec, mats, block_mat, block_vec):
        """fos_feas_set_blocks2 with raw arrays (SeparableSum.pack2): a separable sum that may hold dense blocks replaces set `which`"""
        kinds, lens = np.ascontiguousarray(kinds, dtype=np.int32), np.ascontiguousarray(lens, dtype=np.int64)
        scal = np.ascontiguousarray(scal, dtype=np.float64)
        vec = None if vec is None else np.ascontiguousarray(vec, dtype=np.float64)
        mats = [np.ascontiguousarray(M, dtype=np.float64) for M in mats]
        for M in mats:
            if M.ndim != 2:
                raise ValueError("set_blocks2: every matrix must be two-dimensional")
        rows = np.ascontiguousarray([M.shape[0] for M in mats], dtype=np.int64)
        cols = np.ascontiguousarray([M.shape[1] for M in mats], dtype=np.int64)
        block_mat = np.ascontiguousarray(block_mat, dtype=np.int64)
        vecs = [None if v is None else np.ascontiguousarray(v, dtype=np.float64) for v in block_vec]
        if block_mat.shape[0] != len(kinds) or len(vecs) != len(kinds):
            raise ValueError("set_blocks2: block_mat and block_vec have one entry per block")
        dpp = C.POINTER(C.c_double)
        mat_ptrs = (dpp * max(len(mats), 1))(*[_lib.dptr(M) for M in mats])
        vec_ptrs = (dpp * max(len(vecs), 1))(*[C.cast(None, dpp) if v is None else _lib.dptr(v) for v in vecs])
        i64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
        _lib.check(self._lib.fos_feas_set_blocks2(self._h, which, len(kinds), kinds.ctypes.data_as(C.POINTER(C.c_int32)), i64(lens), _lib.dptr(scal),
                                                  None if vec is None else _lib.dptr(vec), len(mats), i64(rows), i64(cols), mat_ptrs, i64(block_mat), vec_ptrs))

    def dense_block_stats(self, which):
        """the counters of the dense blocks of a separable sum (fos_feas_dense_block_stats)"""
        o = np.zeros(8)
        _lib.check(self._lib.fos_feas_dense_block_stats(self._h, which, _lib.dptr(o)))
        return {"dense_blocks": int(o[0]), "matrices": int(o[1]), "wave_blocks": int(o[2]), "workgroup_blocks": int(o[3]), "launches": int(o[4]),
                "matrix_bytes": int(o[5]), "largest_order": int(o[6]), "lds_blocks": int(o[7])}

    def dense_block_get(self, which, block, p):
        """test entry: the G (p x p) and d (p) the device holds for the 0-based block `block` (fos_feas_dense_block_get)"""
        G, d = np.zeros((p, p)), np.zeros(p)
        _lib.check(self._lib.fos_feas_dense_block_get(self._h, which, block, _lib.dptr(G), _lib.dptr(d)))
        return G, d

    def set_callback(self, which, S):
        """fos_feas_set_callback: set `which` becomes the object S, its prox(y, x) evaluated on the host"""
        cb = PROX_FN(self._make_prox_callback(S))
        self._callbacks.append(cb)                                      # (the library keeps the pointer: it must outlive the handle)
        _lib.check(self._lib.fos_feas_set_callback(self._h, which, C.cast(cb, C.c_void_p), None))

    def set_stats(self, which):
        """the counters of a set defined by fos_feas_set_blocks (fos_feas_set_stats)"""
        o = np.zeros(8)
        _lib.check(self._lib.fos_feas_set_stats(self._h, which, _lib.dptr(o)))
        return {"blocks": int(o[0]), "wave_blocks": int(o[1]), "workgroup_blocks": int(o[2]), "grid_blocks": int(o[3]), "launches": int(o[4]),
                "last_passes": int(o[5]), "pass_cap": int(o[6]), "candidates": int(o[7])}

    def _make_prox_callback(self, S):
        n = self.n

        def call(ctx, nn, xp, yp):
            try:
                x = np.ctypeslib.as_array(xp, shape=(n,))
                y = np.ctypeslib.as_array(yp, shape=(n,))
                S.prox(y, x)                                            # prox!(y, S, x): fills y in place
                return 0
            except Exception as exc:  # noqa: BLE001  (an exception must not unwind through the C frames)
                self.callback_error = exc
                return 1
        return call

    def _check(self, rc):
        """_lib.check, with the exception a prox callback raised (if that is what stopped the call) as the cause"""
        try:
            _lib.check(rc)
        except _lib.FosError as err:
            exc, self.callback_error = self.callback_error, None
            if exc is not None:
                raise err from exc
            raise

    def close(self):
        if getattr(self, "_h", None):
            self._lib.fos_feas_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_alg(self, alg: FOSAlgorithm):
        if isinstance(alg, GAPP):
            _lib.check(self._lib.fos_feas_set_gapp(self._h, alg.alpha, alg.alpha1, alg.alpha2, alg.iproj))
            return
        _lib.check(self._lib.fos_feas_set_alg(self._h, *alg._alg_args()))
        if isinstance(alg, LineSearchWrapper):                          # the wrapped algorithm's arguments, then the search
            _lib.check(self._lib.fos_feas_set_linesearch(self._h, alg.lsinterval))
        if isinstance(alg, LongstepWrapper):
            _lib.check(self._lib.fos_feas_set_longstep(self._h, alg.longinterval, alg.nsave))

    def set_iterate(self, x0=None):
        if x0 is None:
            _lib.check(self._lib.fos_feas_set_iterate(self._h, None))
        else:
            x0 = np.ascontiguousarray(x0, dtype=np.float64)
            assert x0.shape == (self.n,)
            _lib.check(self._lib.fos_feas_set_iterate(self._h, _lib.dptr(x0)))

    def step(self, i_first, count, checki, eps):
        """-> (iterations run, status name, err of the last check or nan, checked flag of the last iteration)"""
        done, st, err, chk = C.c_int64(0), C.c_int32(0), C.c_double(float("nan")), C.c_int32(0)
        self._check(self._lib.fos_feas_step(self._h, i_first, count, checki, eps, C.byref(done), C.byref(st), C.byref(err), C.byref(chk)))
        return done.value, _lib.STATUS_NAMES[st.value], err.value, bool(chk.value)

    def getsol(self, force_check=False, eps=1e-5):
        sol = np.empty(self.n)
        st, err = C.c_int32(0), C.c_double(float("nan"))
        self._check(self._lib.fos_feas_getsol(self._h, _lib.dptr(sol), 1 if force_check else 0, eps, C.byref(st), C.byref(err)))
        return sol, _lib.STATUS_NAMES[st.value], err.value

    def get_iterate(self):
        x = np.empty(self.n)
        _lib.check(self._lib.fos_feas_get_iterate(self._h, _lib.dptr(x)))
        return x

    def prox(self, which, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.empty(self.n)
        self._check(self._lib.fos_feas_prox(self._h, which, _lib.dptr(x), _lib.dptr(y)))
        return y

    def info(self):
        a12 = C.c_double(0.0)
        its = (C.c_int32 * 2)()
        res = (C.c_double * 2)()
        _lib.check(self._lib.fos_feas_info(self._h, C.byref(a12), its, res))
        return {"alpha12": a12.value, "ns_iters": list(its), "ns_resid": list(res)}

    def affine_stats(self, which):
        """the sparse IndAffine's counters (fos_feas_affine_stats)"""
        o = np.zeros(8)
        _lib.check(self._lib.fos_feas_affine_stats(self._h, which, _lib.dptr(o)))
        return {"projections": int(o[0]), "cg_iterations": int(o[1]), "last_cg_iterations": int(o[2]), "last_restarts": int(o[3]), "last_residual": o[4],
                "last_rounding_level": o[5], "nnz": int(o[6]), "lanes_per_row": (int(o[7]) // 1000, int(o[7]) % 1000)}

    def affine_factored_stats(self, which):
        """the factored IndAffine's (or LeastSquares') set-up record and the split of its two passes (fos_feas_affine_factored_stats, fos_feas_affine_factored_plan)"""
        o, p = np.zeros(8), np.zeros(6, dtype=np.int64)
        _lib.check(self._lib.fos_feas_affine_factored_stats(self._h, which, _lib.dptr(o)))
        _lib.check(self._lib.fos_feas_affine_factored_plan(self._h, which, p.ctypes.data_as(C.POINTER(C.c_int64))))
        return {"m": int(o[0]), "n": int(o[1]), "refine": int(o[2]), "factor": DIRECT_FACTOR_NAMES[int(o[3])], "fell_back": int(o[4]), "probe_resid": float(o[5]),
                "launches": int(o[6]), "bytes": int(o[7]), "ld": int(p[0]), "gram_order": int(p[1]), "span_cols": int(p[2]), "spans": int(p[3]),
                "rows_per_block": int(p[4]), "row_blocks": int(p[5])}

    def nspace_stats(self, which):
        """the set-up record of a Quadratic or a LeastSquares(form="normal") (fos_feas_nspace_stats)"""
        o = np.zeros(8)
        _lib.check(self._lib.fos_feas_nspace_stats(self._h, which, _lib.dptr(o)))
        return {"n": int(o[0]), "m": int(o[1]), "factor": DIRECT_FACTOR_NAMES[int(o[2])], "fell_back": int(o[3]), "probe_resid": float(o[4]), "launches": int(o[5]),
                "bytes": int(o[6]), "tiles": int(o[7])}

    def nspace_cg_stats(self, which):
        """the CG record of a Quadratic(form="cg") or a LeastSquares(form="cg") (fos_feas_nspace_cg_stats)"""
        o = np.zeros(8)
        _lib.check(self._lib.fos_feas_nspace_cg_stats(self._h, which, _lib.dptr(o)))
        return {"calls": int(o[0]), "iters_total": int(o[1]), "last_iters": int(o[2]), "last_restarts": int(o[3]), "last_resid": float(o[4]),
                "last_level": float(o[5]), "stored": int(o[6]), "launches_per_iter": int(o[7])}

    def affine_sparse_factored_stats(self, which):
        """the sparse factored IndAffine's (or sparse wide LeastSquares') set-up record and the segment tables of its two passes (fos_feas_affine_sparse_factored_stats, ..._plan)"""
        o, p = np.zeros(8), np.zeros(8, dtype=np.int64)
        _lib.check(self._lib.fos_feas_affine_sparse_factored_stats(self._h, which, _lib.dptr(o)))
        _lib.check(self._lib.fos_feas_affine_sparse_factored_plan(self._h, which, p.ctypes.data_as(C.POINTER(C.c_int64))))
        return {"m": int(o[0]), "n": int(o[1]), "refine": int(o[2]), "factor": DIRECT_FACTOR_NAMES[int(o[3])], "fell_back": int(o[4]), "probe_resid": float(o[5]),
                "launches": int(o[6]), "bytes": int(o[7]), "nnz": int(p[0]), "gram_order": int(p[1]), "seg": int(p[2]), "items_rows": int(p[3]),
                "folded_rows": int(p[4]), "items_cols": int(p[5]), "folded_cols": int(p[6]), "segments": int(p[7])}


class FeasibilityModel:
    """mutable struct FeasibilityModel   Feasibility.jl:15-50: problem + algorithm + merged options, solve_stat, history."""

    def __init__(self, problem: Feasibility, alg: FOSAlgorithm, device=0, **kwargs):
        self.S1, self.S2, self.n, self.alg = problem.S1, problem.S2, problem.n, alg
        self.options = dict(alg.options)
        self.options.update(kwargs)                                    # kwargs of solve! override the algorithm's   :37-41
        self.solve_stat = "NotSolved"
        self.obj_val = 0.0
        self.enditr = -1
        self.history = {}
        self.out = None
        t1 = time.perf_counter_ns()
        self.dev = HipFeasibility(problem, device=device)              # init_algorithm!   :46
        self.dev.set_alg(alg)
        self.init_duration = time.perf_counter_ns() - t1

    def _println(self, s):
        if self.out is not None:
            self.out.append(s)
        else:
            print(s)

    def solve(self):
        """solve!(model)   solverwrapper.jl:2-41 with FeasibilityStatus (FeasibilityStatus.jl:32-91)."""
        o = self.options
        max_iters, verbose, debug = o.get("max_iters", 10000), o.get("verbose", 1), o.get("debug", 1)
        eps, checki = o.get("eps", 1e-5), o.get("checki", 100)
        dev = self.dev
        dev.set_iterate(o.get("initx"))
        t0 = time.perf_counter_ns()
        if verbose > 0:                                                # printstatusheader :74-84 (direct = true: no cg column)
            self._println("Time to initialize: %ss" % julia_float(self.init_duration / 1e9))
            self._println("-" * 22)
            self._println(" Iter | res | time")
            self._println("-" * 22)
        i, status, checked, err = 0, "Continue", False, float("nan")
        ls = self.alg.lsinterval if isinstance(self.alg, LineSearchWrapper) else 0
        gp = self.alg.iproj if isinstance(self.alg, GAPP) else 0
        while i < max_iters and status == "Continue":
            nxt = min(max_iters, (i // checki + 1) * checki) if checki > 0 else max_iters
            if ls > 0:
                nxt = min(nxt, (i // ls + 1) * ls)                     # stop at every line-search iteration: its output is printed
            if gp > 0:
                nxt = min(nxt, (i // gp + 1) * gp)
            done, status, err, checked = dev.step(i + 1, nxt - i, checki, eps)
            i += done
            if gp > 0 and i % gp == 0:                                 # what gapproj.jl:51,57 print (unconditionally)
                _, tests, abest = dev.gapp_log()
                for nt in tests:
                    self._println("normtest: %s" % julia_float(nt))
                self._println("\u03b1best: %s" % julia_float(abest))
            if ls > 0 and i % ls == 0:                                 # what linesearch.jl:51,63,69 print
                _, normres, tests, abest = dev.linesearch_log()
                self._println("test, %s" % julia_float(normres))
                a = 0.1
                for tr in tests:
                    a = a * 1.8
                    self._println("\u03b1: %s, %s" % (julia_float(a), julia_float(tr)))
                self._println("\u03b1: %s" % julia_float(abest))
            if checked:
                t = time.perf_counter_ns() - t0
                if debug > 0:                                          # savedata :95-103
                    self.history.setdefault("err", []).append((i, err))
                    self.history.setdefault("t", []).append((i, t))
                if verbose > 0:                                        # printstatusiter :86-88
                    self._println("%6d|%s % .1es" % (i, _jl_e9(err), t / 1e9))
                    if status == "Optimal":
                        self._println("Found solution i=%d" % i)
        guess, st2, err2 = dev.getsol(force_check=not checked, eps=eps)            # solverwrapper.jl:30-34
        if not checked:
            status, err = st2, err2
            if debug > 0:
                self.history.setdefault("err", []).append((i, err))
            if verbose > 0:
                self._println("%6d|%s % .1es" % (i, _jl_e9(err), (time.perf_counter_ns() - t0) / 1e9))
                if status == "Optimal":
                    self._println("Found solution i=%d" % i)
        if verbose > 0:                                                # solverwrapper.jl:35-39
            self._println("Time for iterations: ")
            self._println("%s s" % julia_float((time.perf_counter_ns() - t0) / 1e9))
        self.enditr = i
        endstatus = "Indeterminate" if status == "Continue" else status            # populate_solution :61-68
        self.solve_stat = endstatus
        sol = FeasibilitySolution(guess, endstatus)
        sol.iterations, sol.err = i, err
        return sol


def _jl_e9(v):
    """@printf("% 9.2e", v)"""
    return "% 9.2e" % v


def solve_feasibility(problem: Feasibility, alg: FOSAlgorithm, device=0, out=None, **kwargs):
    """solve!(problem::Feasibility, alg; kwargs...) -> (solution, model)   Feasibility.jl:52-56"""
    model = FeasibilityModel(problem, alg, device=device, **kwargs)
    model.out = out
    return model.solve(), model
