# FOSHip.jl -- thin Julia shim that routes FirstOrderSolvers.jl's HSDE hot path to libfoship.so (MI355X / HIP).
#
# STATUS: written against the reference sources but NOT EXECUTED -- the build container has no Julia binary
# (SURVEY.md section 8(c)).  The same C ABI is exercised end to end by the Python mirror
# (firstordersolvers.jl_amd/interface.py, tests/test_gpu_parity.py); this file is the binding a maintainer adds.
#
# How it plugs in (reference files in brackets):
#   * `include("FOSHip.jl")` at the end of src/FirstOrderSolvers.jl (after solvers/*.jl are loaded).
#   * The user passes `gpu=true` with any solver:  solve!(problem, DR(eps=1e-8, gpu=true)).  Keyword arguments are
#     captured in `alg.options` and splatted into `model.options` [FOSSolverInterface.jl:5, types.jl:57]; unknown keys
#     are ignored by the reference, so nothing else changes.
#   * `init_algorithm!` [gap.jl:23, gapa.jl:27, fista.jl:20, dykstra.jl:19] is intercepted for FOSMathProgModel when
#     `gpu=true`: it returns a `HipData` (a FOSSolverData) instead of GAPData/GAPAData/...; everything downstream
#     dispatches on that data type:  `iterate` [solverwrapper.jl:20-41], `Base.step`, `getsol`, `getcgiter`.
#   * FOSMathProgModel, loadproblem!, optimize!, status/getobjval/getsolution, model.history, the printed table and
#     HSDE_populatesolution stay the reference's own code.
module FOSHip

using ..FirstOrderSolvers
import ..FirstOrderSolvers: FOSAlgorithm, FOSSolverData, FOSMathProgModel, HSDEStatus, GAP, GAPA, FISTA, Dykstra,
                            init_algorithm!, getsol, getcgiter, iterate, printstatusheader, printstatusiter,
                            savedata, ConeProduct
import ProximalOperators
using SparseArrays, Printf

const libfoship = get(ENV, "FOSHIP_LIB", "libfoship.so")

# ---- mirror of include/foship.h ------------------------------------------------------------------------------
const FOS_ALG_GAP, FOS_ALG_GAPA, FOS_ALG_FISTA, FOS_ALG_DYKSTRA = Cint(0), Cint(1), Cint(2), Cint(3)
const STATUS_SYMBOLS = (:Continue, :Optimal, :Unbounded, :Infeasible)        # FOS_STATUS_*

struct CheckResult            # struct fos_check_result
    p::Cdouble; d::Cdouble; g::Cdouble; ctx::Cdouble; bty::Cdouble
    kappa::Cdouble; tau::Cdouble; norm_axs::Cdouble; norm_aty::Cdouble; norm_b::Cdouble; norm_c::Cdouble
    cgiter::Int64; status::Int32; cg_maxiter_hit::Int32
end

function check(code::Cint)
    code == 0 && return
    msg = unsafe_string(ccall((:fos_last_error, libfoship), Cstring, ()))
    error("libfoship error $code: $msg")
end

# cone codes: keys of conemap [cones.jl:4-14]
conecode(::ProximalOperators.IndFree) = Int32(0)
conecode(::ProximalOperators.IndZero) = Int32(1)
conecode(::ProximalOperators.IndNonnegative) = Int32(2)
conecode(::ProximalOperators.IndNonpositive) = Int32(3)
conecode(::ProximalOperators.IndSOC) = Int32(4)
conecode(::ProximalOperators.IndRotatedSOC) = Int32(5)
conecode(::ProximalOperators.IndPSD) = Int32(6)
conecode(::ProximalOperators.IndExpPrimal) = Int32(7)
conecode(::ProximalOperators.IndExpDual) = Int32(8)

function conearrays(K::ConeProduct)
    N = length(K.cones)
    types = Int32[conecode(K.cones[i]) for i in 1:N]
    starts = Int64[first(K.ranges[i]) for i in 1:N]
    lens = Int64[length(K.ranges[i]) for i in 1:N]
    return types, starts, lens
end

# ---- the device-resident solver data ---------------------------------------------------------------------------
mutable struct HipData <: FOSSolverData
    handle::Ptr{Cvoid}
    m::Int
    n::Int
    cgiter::Int64
    lsinterval::Int64                     # > 0: LineSearchWrapper around the algorithm [wrappers/linesearch.jl]
    gappinterval::Int64                   # > 0: GAPP, its search interval [solvers/gapproj.jl]
    # equilibrate: the option of the same name (device-side key, like cg_variant) -- false / 0: the problem as given [HSDE.jl:7-29]; true: 10 passes of the opt-in
    # scaling of fos_create3, an integer 1..50: that many.  Iterates and check results stay in the caller's units (include/foship.h).
    function HipData(model::FOSMathProgModel, device::Integer; equilibrate=get(model.options, :equilibrate, false))
        A = model.A                       # SparseMatrixCSC{Float64,Int}: colptr/rowval are Int64 and 1-based, as the ABI wants
        m, n = size(A)
        b = convert(Vector{Float64}, vec(model.b))
        c = convert(Vector{Float64}, vec(model.c))
        t1, s1, l1 = conearrays(model.K1)
        t2, s2, l2 = conearrays(model.K2)
        h = Ref{Ptr{Cvoid}}(C_NULL)
        passes = equilibrate === true ? Int32(10) : (equilibrate === false ? Int32(0) : Int32(equilibrate))
        GC.@preserve A b c t1 s1 l1 t2 s2 l2 begin
            if passes == 0
                check(ccall((:fos_create, libfoship), Cint,
                            (Int64, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                             Int64, Ptr{Int32}, Ptr{Int64}, Ptr{Int64}, Int64, Ptr{Int32}, Ptr{Int64}, Ptr{Int64},
                             Cint, Ref{Ptr{Cvoid}}),
                            m, n, A.colptr, A.rowval, A.nzval, b, c,
                            length(t1), t1, s1, l1, length(t2), t2, s2, l2, Cint(device), h))
            else
                check(ccall((:fos_create3, libfoship), Cint,
                            (Int64, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                             Int64, Ptr{Int32}, Ptr{Int64}, Ptr{Int64}, Int64, Ptr{Int32}, Ptr{Int64}, Ptr{Int64},
                             Cint, Int32, Int32, Ref{Ptr{Cvoid}}),
                            m, n, A.colptr, A.rowval, A.nzval, b, c,
                            length(t1), t1, s1, l1, length(t2), t2, s2, l2, Cint(device), Int32(0), passes, h))
            end
        end
        d = new(h[], m, n, 0, 0, 0)
        finalizer(x -> (x.handle != C_NULL && ccall((:fos_destroy, libfoship), Cint, (Ptr{Cvoid},), x.handle); x.handle = C_NULL), d)
        return d
    end
end

algargs(a::GAP) = (FOS_ALG_GAP, a.α, a.α1, a.α2, 0.0)              # gap.jl:6-13
algargs(a::GAPA) = (FOS_ALG_GAPA, a.α, 0.0, 0.0, a.β)              # gapa.jl:9-15
algargs(a::FISTA) = (FOS_ALG_FISTA, a.α, 0.0, 0.0, 0.0)            # fista.jl:6-11
algargs(a::Dykstra) = (FOS_ALG_DYKSTRA, 0.0, 0.0, 0.0, 0.0)        # dykstra.jl:5-9
algargs(a::FirstOrderSolvers.GAPP) = (FOS_ALG_GAP, a.α, a.α1, a.α2, 0.0)   # gapproj.jl:5-13: GAP + fos_set_gapp(iproj)

set_alg!(d::HipData, alg) = check(ccall((:fos_set_alg, libfoship), Cint, (Ptr{Cvoid}, Cint, Cdouble, Cdouble, Cdouble, Cdouble),
                                        d.handle, algargs(alg)...))

usegpu(model::FOSMathProgModel) = get(model.options, :gpu, false) === true

# ---- init_algorithm!: return HipData when gpu=true, otherwise fall through to the reference method --------------
for T in (:GAP, :GAPA, :FISTA, :Dykstra, :(FirstOrderSolvers.GAPP))
    @eval function init_algorithm!(alg::$T, model::FOSMathProgModel)
        if usegpu(model)
            # the reference's closure [HSDE.jl:24-27], built directly: get_sets_and_status would also construct the host-side
            # AffinePlusLinear (5 N-vectors of CG state) and DualConeProduct, which the device path never touches.
            # m, n as DualConeProduct's constructor takes them [cones.jl:121]
            sm, sn = model.K1.ranges[end][end], model.K2.ranges[end][end]
            dmode = Ref{Int32}(0)          # fos_get_direct_mode, read below: 1 dense inverse, 2 block form, 4 reduced form (no CG: the table drops its cg column), 3 CG at its floor
            status_generator = (mo, checki, eps, verbose, debug) ->
                HSDEStatus(sm, sn, 0, mo, :Continue, checki, eps, verbose, false, alg.direct && dmode[] in (1, 2, 4), time_ns(), model.init_duration, debug)
            data = HipData(model, get(model.options, :device, 0))
            set_alg!(data, alg)
            if haskey(model.options, :cg_variant)      # device-side key: which CG recurrence the affine projection runs (FOS_CG_* of foship.h)
                check(ccall((:fos_set_cg_variant, libfoship), Cint, (Ptr{Cvoid}, Int32), data.handle, Int32(model.options[:cg_variant])))
            end
            if alg isa FirstOrderSolvers.GAPP            # "projected GAP": every iproj-th iteration is a 21-point search on the device
                check(ccall((:fos_set_gapp, libfoship), Cint, (Ptr{Cvoid}, Int64), data.handle, Int64(alg.iproj)))
                data.gappinterval = alg.iproj
            end
            if alg.direct            # HSDE.jl:12-15: S1 = IndAffine([Q -I], 0) -> exact projection, (I + Q Q')^-1 formed once on the device
                A = model.A
                # the option direct_form = :reduced asks for the reduced form (FOS_DIRECT_FORM_REDUCED = 4: the inverse of I + A'A or I + A A' only, min(m, n) <= 46 000)
                form = get(model.options, :direct_form, :auto) == :reduced ? Int32(4) : Int32(0)
                # the option direct_factor = :cholesky builds the stored inverse by a blocked Cholesky factorisation (FOS_DIRECT_FACTOR_CHOLESKY = 1) instead of Newton-Schulz (0)
                dfac = get(model.options, :direct_factor, :newton)
                dfac in (:newton, :cholesky) || error("direct_factor must be :newton or :cholesky, not $(repr(dfac))")
                if dfac == :cholesky
                    GC.@preserve A check(ccall((:fos_enable_direct3, libfoship), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}, Ptr{Cdouble}, Int32, Int32),
                                               data.handle, A.colptr, A.rowval, A.nzval, form, Int32(1)))
                else                 # no factor chosen: the older entry (the environment's FOS_DIRECT_FACTOR still applies there)
                    GC.@preserve A check(ccall((:fos_enable_direct2, libfoship), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}, Ptr{Cdouble}, Int32),
                                               data.handle, A.colptr, A.rowval, A.nzval, form))
                end
                check(ccall((:fos_get_direct_mode, libfoship), Cint, (Ptr{Cvoid}, Ref{Int32}), data.handle, dmode))
            end
            return data, status_generator
        end
        return invoke(init_algorithm!, Tuple{$T,FirstOrderSolvers.AbstractFOSModel}, alg, model)
    end
end

# ---- LineSearchWrapper(GAP / GAPA) [wrappers/linesearch.jl]: the wrapped algorithm's handle with the search switched on; the
#      search itself (tmp1 = x; x = S2!(S1!(x)); 31 trial step lengths; x = tmp1 + alpha_best res) runs on the device.
function init_algorithm!(ls::LineSearchWrapper, model::FOSMathProgModel)
    if usegpu(model)
        data, status_generator = init_algorithm!(ls.alg, model)          # errors for algorithms other than GAP / GAPA below
        check(ccall((:fos_set_linesearch, libfoship), Cint, (Ptr{Cvoid}, Int64), data.handle, ls.lsinterval))
        data.lsinterval = ls.lsinterval
        return data, status_generator
    end
    return invoke(init_algorithm!, Tuple{LineSearchWrapper,FirstOrderSolvers.AbstractFOSModel}, ls, model)
end

# ---- LongstepWrapper(GAP / GAPA / FISTA / Dykstra) [wrappers/longstep.jl, saveplanes.jl]: the wrapped algorithm's handle with the plane saving and the
#      projection onto the saved planes switched on (fos_set_longstep); planes and projection stay on the device, `iterate` is the wrapped algorithm's.
import ..FirstOrderSolvers: LongstepWrapper
function init_algorithm!(long::LongstepWrapper, model::FOSMathProgModel)
    if usegpu(model)
        !FirstOrderSolvers.support_longstep(long.alg) && @error "Algorithm alg does not support longstep"        # longstep.jl:28
        data, status_generator = init_algorithm!(long.alg, model)
        check(ccall((:fos_set_longstep, libfoship), Cint, (Ptr{Cvoid}, Int64, Int64), data.handle, Int64(long.longinterval), Int64(long.nsave)))
        return data, status_generator
    end
    return invoke(init_algorithm!, Tuple{LongstepWrapper,FirstOrderSolvers.AbstractFOSModel}, long, model)
end
iterate(long::LongstepWrapper, data::HipData, status::HSDEStatus, x, max_iters) = iterate(long.alg, data, status, x, max_iters)
getsol(long::LongstepWrapper, data::HipData, x) = getsol(long.alg, data, x)

# what linesearch.jl:51,63,69 print during a search, from the device's record of the last one
function print_gapp(data::HipData)                       # gapproj.jl:51,57
    log = Vector{Float64}(undef, 23)
    check(ccall((:fos_gapp_log, libfoship), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), data.handle, log))
    for k = 1:21
        println("normtest: $(log[k])")
    end
    println("αbest: $(log[22])")
end
function print_linesearch(data::HipData)
    log = Vector{Float64}(undef, 34)
    check(ccall((:fos_linesearch_log, libfoship), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), data.handle, log))
    println("test, $(log[1])")
    α = 0.1
    for k = 0:30
        α = α * 1.8
        println("α: $α, $(log[2+k])")
    end
    println("α: $(log[33])")
end

getcgiter(d::HipData) = d.cgiter                                              # defaults.jl:25-30

# ---- what checkstatus does once the device has produced the scalars [HSDEStatus.jl:39-65] ----------------------
function record!(stat::HSDEStatus, data::HipData, r::CheckResult)
    t = time_ns() - stat.init_time
    i, model = stat.i, stat.model
    data.cgiter = r.cgiter
    if stat.debug > 0           # savedata [HSDEStatus.jl:125-139]; debug=2 vectors need fos_get_checked (below)
        x = y = s = Float64[]
        if stat.debug > 1
            z = Vector{Float64}(undef, 2 * (data.m + data.n + 1))
            check(ccall((:fos_get_checked, libfoship), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), data.handle, z))
            nu = data.n + data.m + 1
            x, y, s = z[1:data.n], z[data.n+1:data.n+data.m], z[nu+data.n+1:nu+data.n+data.m]
        end
        savedata(i, r.p, r.d, r.g, r.ctx, r.bty, r.kappa, r.tau, x, y, s, t, model, stat.debug)
    end
    if stat.verbose > 0 && !stat.direct                                        # HSDEStatus.jl:43-47
        push!(model.history, :cgiter, i, r.cgiter)
        printstatusiter(i, r.p, r.d, r.g, r.ctx, r.bty, r.kappa / r.tau, r.cgiter, t)
    elseif stat.verbose > 0                                                    # :48-50
        printstatusiter(i, r.p, r.d, r.g, r.ctx, r.bty, r.kappa / r.tau, t)
    end
    r.cg_maxiter_hit != 0 && @warn "CG reached max iterations, result may be inaccurate"   # conjugategradients.jl:53
    stat.status = STATUS_SYMBOLS[r.status+1]
    if stat.status == :Optimal && stat.verbose > 0
        println("Found solution i=$i")
    end
    stat.checked = true
    return
end

# ---- iterate [solverwrapper.jl:20-41], device resident: the host sees one ccall per check interval ---------------
function iterate(alg::FOSAlgorithm, data::HipData, status::HSDEStatus, x, max_iters)
    t1 = time()
    printstatusheader(status)
    check(ccall((:fos_set_iterate, libfoship), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), data.handle, x))     # initx / z0
    i = 0
    done, checked, res = Ref{Int64}(0), Ref{Int32}(0), Ref{CheckResult}()
    while i < max_iters
        count = min(max_iters - i, status.checki - (i % status.checki))
        ls = data.lsinterval
        ls > 0 && (count = min(count, ls - (i % ls)))                 # stop at every line-search iteration: its output is printed
        gp = data.gappinterval
        gp > 0 && (count = min(count, gp - (i % gp)))
        check(ccall((:fos_step, libfoship), Cint,
                    (Ptr{Cvoid}, Int64, Int64, Int64, Cdouble, Ref{Int64}, Ref{Int32}, Ref{CheckResult}),
                    data.handle, i + 1, count, status.checki, status.eps, done, checked, res))
        i += done[]
        status.i = i
        ls > 0 && i % ls == 0 && print_linesearch(data)
        gp > 0 && i % gp == 0 && print_gapp(data)
        if checked[] != 0
            record!(status, data, res[])
            status.status != :Continue && break
        else
            status.checked = false
        end
    end
    guess = Vector{Float64}(undef, length(x))
    force = status.checked ? Int32(0) : Int32(1)                                   # solverwrapper.jl:31-34
    check(ccall((:fos_getsol, libfoship), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Int32, Cdouble, Ref{CheckResult}),
                data.handle, guess, force, status.eps, res))
    force != 0 && record!(status, data, res[])
    if status.verbose > 0
        println("Time for iterations: ")
        println("$(time() - t1) s")
    end
    return guess
end

# ---- single-step entry points for callers written against step/getsol (one upload, one ccall, one download per
#      iteration: correct but PCIe bound -- `iterate` above is the path to use).  The host vector is uploaded on EVERY call, so
#      a caller that edits x between steps is honoured.  LineSearchWrapper and LongstepWrapper run on the device through `iterate` (above).
function Base.step(alg::FOSAlgorithm, data::HipData, x, i, status::HSDEStatus, longstep = nothing)
    longstep === nothing || error("longstep/linesearch wrappers are not available with gpu=true")
    check(ccall((:fos_set_iterate, libfoship), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), data.handle, x))
    done, checked, res = Ref{Int64}(0), Ref{Int32}(0), Ref{CheckResult}()
    check(ccall((:fos_step, libfoship), Cint,
                (Ptr{Cvoid}, Int64, Int64, Int64, Cdouble, Ref{Int64}, Ref{Int32}, Ref{CheckResult}),
                data.handle, i, 1, status.checki, status.eps, done, checked, res))
    if checked[] != 0
        record!(status, data, res[])
    else
        status.checked = false
    end
    check(ccall((:fos_get_iterate, libfoship), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), data.handle, x))
    return
end

function getsol(alg::FOSAlgorithm, data::HipData, x)
    guess = Vector{Float64}(undef, length(x))
    res = Ref{CheckResult}()
    check(ccall((:fos_getsol, libfoship), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Int32, Cdouble, Ref{CheckResult}),
                data.handle, guess, Int32(0), 0.0, res))
    return guess
end

# ---- checkpoint / resume of a device-resident run: the iterate, S1's persistent state (CGdata.xinit, AffinePlusLinear.i:
#      affinepluslinear.jl:58-69,114) and the algorithm's *Data struct (FISTAData.y/.xold/.t fista.jl:15-25, DykstraData.p/.q
#      dykstra.jl:12-23, GAPAData.alpha12 gapa.jl:29) -- everything `iterate` would need to go on from iteration i + 1 elsewhere
function checkpoint(data::HipData, N::Integer)
    x, xinit, a, b = (Vector{Float64}(undef, N) for _ in 1:4)
    i, firstrun, scal = Ref{Int64}(0), Ref{Int32}(0), zeros(2)
    check(ccall((:fos_get_iterate, libfoship), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), data.handle, x))
    check(ccall((:fos_get_affine_state, libfoship), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ref{Int64}, Ref{Int32}), data.handle, xinit, i, firstrun))
    check(ccall((:fos_get_alg_state, libfoship), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}), data.handle, a, b, scal))
    return (x = x, xinit = xinit, i = i[], firstrun = firstrun[] != 0, a = a, b = b, t = scal[1], alpha12 = scal[2])
end
function restore!(data::HipData, cp)
    check(ccall((:fos_set_iterate, libfoship), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), data.handle, cp.x))
    cp.firstrun || check(ccall((:fos_set_affine_state, libfoship), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Int64), data.handle, cp.xinit, Int64(cp.i)))
    check(ccall((:fos_set_alg_state, libfoship), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}), data.handle, cp.a, cp.b, [cp.t, cp.alpha12]))
    return data
end

# ---- Feasibility form [problemforms/Feasibility/Feasibility.jl, FeasibilityStatus.jl]: solve!(Feasibility(S1, S2, n), alg; gpu=true)
#      with S1, S2 among ProximalOperators.IndAffine (dense A), IndBox -- the sets of test/testfeasibility.jl -- and
#      FirstOrderSolvers.ConeProduct on the device, as are IndBallL2, IndBallL1, IndSimplex, IndHalfspace, IndHyperslab, IndPoint and IndFree,
#      the functions NormL1, SqrNormL2, ElasticNet, Linear, NormL2, HuberLoss, NormLinf (fos_feas_set_blocks) and LeastSquares over a dense A
#      (fos_feas_set_least_squares), a tall or sparse LeastSquares and a dense Quadratic in the n-space (fos_feas_set_least_squares_normal, _sparse,
#      fos_feas_set_quadratic); any other ProximableFunction through a host callback (fos_feas_set_callback).
#      init_algorithm! returns a HipFeasData; iterate dispatches on it; FeasibilityModel, populate_solution and the printed table
#      stay the reference's own code.
import ..FirstOrderSolvers: FeasibilityModel, FeasibilityStatus

# fos_prox_fn: int32 fn(void* ctx, int64 n, const double* x, double* y) -- ctx is the set (boxed in a Ref), y = prox_S(x)
function prox_trampoline(ctx::Ptr{Cvoid}, n::Int64, x::Ptr{Cdouble}, y::Ptr{Cdouble})::Int32
    try
        S = unsafe_pointer_to_objref(ctx)[]
        ProximalOperators.prox!(unsafe_wrap(Array, y, n), S, unsafe_wrap(Array, x, n))
        return Int32(0)
    catch
        return Int32(1)                                     # (an exception must not unwind through the C frames)
    end
end
const PROX_TRAMPOLINE = Ref{Ptr{Cvoid}}(C_NULL)             # @cfunction pointers are made at run time (__init__)

# Vector sets with kernels of their own (csrc/sets.hip, fos_feas_set_blocks) [Feasibility.jl:2-6 takes any two ProximableFunctions]: kind codes of
# include/foship.h, and the (kind, scalar 1, scalar 2, vector | nothing) of the ProximalOperators types that map onto one block of length n
const FOS_SET_FREE = Int32(0)
const FOS_SET_BALL_L2 = Int32(1)
const FOS_SET_BALL_L1 = Int32(2)
const FOS_SET_SIMPLEX = Int32(3)
const FOS_SET_HALFSPACE = Int32(4)
const FOS_SET_HYPERSLAB = Int32(5)
const FOS_SET_POINT = Int32(6)
const FOS_SET_BOX = Int32(7)
# proximable functions that are not indicators: further kinds of the same entry (prox with step 1)
const FOS_FN_NORM_L1 = Int32(32)
const FOS_FN_SQR_NORM_L2 = Int32(33)
const FOS_FN_ELASTIC_NET = Int32(34)
const FOS_FN_LINEAR = Int32(35)
const FOS_FN_NORM_L2 = Int32(36)
const FOS_FN_HUBER = Int32(37)
const FOS_FN_NORM_LINF = Int32(38)
vectorset_block(S) = nothing
vectorset_block(S::ProximalOperators.NormL1{<:Real}) = (FOS_FN_NORM_L1, Float64(S.lambda), 0.0, nothing)
vectorset_block(S::ProximalOperators.SqrNormL2{<:Real}) = (FOS_FN_SQR_NORM_L2, Float64(S.lambda), 0.0, nothing)
vectorset_block(S::ProximalOperators.ElasticNet) = (FOS_FN_ELASTIC_NET, Float64(S.mu), Float64(S.lambda), nothing)
vectorset_block(S::ProximalOperators.Linear) = (FOS_FN_LINEAR, 0.0, 0.0, Vector{Float64}(vec(S.c)))
vectorset_block(S::ProximalOperators.NormL2) = (FOS_FN_NORM_L2, Float64(S.lambda), 0.0, nothing)
vectorset_block(S::ProximalOperators.HuberLoss) = (FOS_FN_HUBER, Float64(S.rho), Float64(S.mu), nothing)
vectorset_block(S::ProximalOperators.Conjugate{<:ProximalOperators.IndBallL1}) = (FOS_FN_NORM_LINF, Float64(S.f.r), 0.0, nothing)      # NormLinf(lambda)
vectorset_block(S::ProximalOperators.IndFree) = (FOS_SET_FREE, 0.0, 0.0, nothing)
vectorset_block(S::ProximalOperators.IndBallL2) = (FOS_SET_BALL_L2, Float64(S.r), 0.0, nothing)
vectorset_block(S::ProximalOperators.IndBallL1) = (FOS_SET_BALL_L1, Float64(S.r), 0.0, nothing)
vectorset_block(S::ProximalOperators.IndSimplex) = (FOS_SET_SIMPLEX, Float64(S.a), 0.0, nothing)
vectorset_block(S::ProximalOperators.IndHalfspace) = (FOS_SET_HALFSPACE, Float64(S.b), 0.0, Vector{Float64}(vec(S.a)))
vectorset_block(S::ProximalOperators.IndHyperslab) = (FOS_SET_HYPERSLAB, Float64(S.low), Float64(S.upp), Vector{Float64}(vec(S.a)))
vectorset_block(S::ProximalOperators.IndPoint) = (FOS_SET_POINT, 0.0, 0.0, Vector{Float64}(vec(S.p)))
# blocks = [(kind, s1, s2, vector | nothing, length), ...]: contiguous, in order, covering 1..n
function feas_set_blocks!(handle::Ptr{Cvoid}, which::Integer, n::Integer, blocks)
    kinds = Int32[b[1] for b in blocks]
    lens = Int64[b[5] for b in blocks]
    scal = Float64[]
    v = zeros(Float64, n)
    pos = 0
    for b in blocks
        push!(scal, b[2], b[3])
        b[4] === nothing || (v[pos+1:pos+b[5]] .= b[4])
        pos += b[5]
    end
    GC.@preserve kinds lens scal v check(ccall((:fos_feas_set_blocks, libfoship), Cint,
                                               (Ptr{Cvoid}, Int32, Int64, Ptr{Int32}, Ptr{Int64}, Ptr{Cdouble}, Ptr{Cdouble}),
                                               handle, Int32(which), Int64(length(blocks)), kinds, lens, scal, v))
end
# Dense blocks of a separable sum (csrc/dense_blocks.hip, fos_feas_set_blocks2): a block of p <= 1024 entries with a dense matrix of its own, y = G x + d
const FOS_FN_BLK_QUADRATIC = Int32(48)
const FOS_SET_BLK_AFFINE = Int32(49)
const FOS_FN_BLK_LEAST_SQUARES = Int32(50)
import Libdl
# blocks as for feas_set_blocks!, a dense block being (kind, lambda | 0.0, 0.0, q | b | nothing, length) with block_mat[i] its 1-based index into
# mats (0 for a vector kind).  mats: Matrix{Float64} as Julia holds them; the library takes ROW-major m x p, so the transposed copy is passed.
# (The entry takes two arrays of pointers, const double* const*: it is bound through its address, with the argument types of include/foship.h.)
function feas_set_blocks2!(handle::Ptr{Cvoid}, which::Integer, n::Integer, blocks, mats, block_mat)
    kinds = Int32[b[1] for b in blocks]
    lens = Int64[b[5] for b in blocks]
    scal = Float64[]
    v = zeros(Float64, n)
    dense(b) = b[1] == FOS_FN_BLK_QUADRATIC || b[1] == FOS_SET_BLK_AFFINE || b[1] == FOS_FN_BLK_LEAST_SQUARES
    pos = 0
    for b in blocks
        push!(scal, b[2], b[3])
        (dense(b) || b[4] === nothing) || (v[pos+1:pos+b[5]] .= b[4])
        pos += b[5]
    end
    rowmajor = [Matrix{Float64}(transpose(M)) for M in mats]              # column-major p x m = ROW-major m x p
    rows = Int64[size(M, 1) for M in mats]
    cols = Int64[size(M, 2) for M in mats]
    bvecs = [dense(b) && b[4] !== nothing ? Vector{Float64}(vec(b[4])) : nothing for b in blocks]
    bmat = Int64[Int64(k) - 1 for k in block_mat]
    fn = Libdl.dlsym(Libdl.dlopen(libfoship), :fos_feas_set_blocks2)
    GC.@preserve kinds lens scal v rowmajor rows cols bvecs bmat begin
        matp = Ptr{Cdouble}[pointer(M) for M in rowmajor]
        vecp = Ptr{Cdouble}[w === nothing ? Ptr{Cdouble}(C_NULL) : pointer(w) for w in bvecs]
        check(ccall(fn, Cint,
                    (Ptr{Cvoid}, Int32, Int64, Ptr{Int32}, Ptr{Int64}, Ptr{Cdouble}, Ptr{Cdouble}, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Ptr{Cdouble}}, Ptr{Int64}, Ptr{Ptr{Cdouble}}),
                    handle, Int32(which), Int64(length(blocks)), kinds, lens, scal, v, Int64(length(mats)), rows, cols, matp, bmat, vecp))
    end
end
function feas_dense_block_stats(handle::Ptr{Cvoid}, which::Integer)
    out = zeros(Float64, 8)
    check(ccall((:fos_feas_dense_block_stats, libfoship), Cint, (Ptr{Cvoid}, Int32, Ptr{Cdouble}), handle, Int32(which), out))
    return (dense_blocks = Int(out[1]), matrices = Int(out[2]), wave_blocks = Int(out[3]), workgroup_blocks = Int(out[4]), launches = Int(out[5]),
            matrix_bytes = Int(out[6]), largest_order = Int(out[7]), lds_blocks = Int(out[8]))
end
function feas_set_stats(handle::Ptr{Cvoid}, which::Integer)
    out = zeros(Float64, 8)
    check(ccall((:fos_feas_set_stats, libfoship), Cint, (Ptr{Cvoid}, Int32, Ptr{Cdouble}), handle, Int32(which), out))
    return (blocks = Int(out[1]), wave_blocks = Int(out[2]), workgroup_blocks = Int(out[3]), grid_blocks = Int(out[4]), launches = Int(out[5]),
            last_passes = Int(out[6]), pass_cap = Int(out[7]), candidates = Int(out[8]))
end
function feas_affine_factored_stats(handle::Ptr{Cvoid}, which::Integer)
    out, plan = zeros(Float64, 8), zeros(Int64, 6)
    check(ccall((:fos_feas_affine_factored_stats, libfoship), Cint, (Ptr{Cvoid}, Int32, Ptr{Cdouble}), handle, Int32(which), out))
    check(ccall((:fos_feas_affine_factored_plan, libfoship), Cint, (Ptr{Cvoid}, Int32, Ptr{Int64}), handle, Int32(which), plan))
    return (m = Int(out[1]), n = Int(out[2]), refine = Int(out[3]), factor = out[4] == 1 ? :cholesky : :newton, fell_back = out[5] != 0, probe_resid = out[6],
            launches = Int(out[7]), bytes = Int(out[8]), ld = plan[1], gram_order = plan[2], span_cols = plan[3], spans = plan[4], rows_per_block = plan[5], row_blocks = plan[6])
end
function feas_affine_sparse_factored_stats(handle::Ptr{Cvoid}, which::Integer)
    out, plan = zeros(Float64, 8), zeros(Int64, 8)
    check(ccall((:fos_feas_affine_sparse_factored_stats, libfoship), Cint, (Ptr{Cvoid}, Int32, Ptr{Cdouble}), handle, Int32(which), out))
    check(ccall((:fos_feas_affine_sparse_factored_plan, libfoship), Cint, (Ptr{Cvoid}, Int32, Ptr{Int64}), handle, Int32(which), plan))
    return (m = Int(out[1]), n = Int(out[2]), refine = Int(out[3]), factor = out[4] == 1 ? :cholesky : :newton, fell_back = out[5] != 0, probe_resid = out[6],
            launches = Int(out[7]), bytes = Int(out[8]), nnz = plan[1], gram_order = plan[2], seg = plan[3], items_rows = plan[4], folded_rows = plan[5],
            items_cols = plan[6], folded_cols = plan[7], segments = plan[8])
end
# LeastSquares(A, b, lambda) over a dense A (1 <= m <= n, m <= 46 000): the factored form with the diagonal of A A' shifted by 1 / lambda
function feas_set_least_squares!(handle::Ptr{Cvoid}, which::Integer, A::AbstractMatrix, b::AbstractVector, lambda::Real, factor::Symbol = :cholesky)
    At = Matrix{Float64}(transpose(A))                      # the C ABI takes A row-major = column-major A'
    bv = Vector{Float64}(b)
    GC.@preserve At bv check(ccall((:fos_feas_set_least_squares, libfoship), Cint, (Ptr{Cvoid}, Int32, Int64, Ptr{Cdouble}, Ptr{Cdouble}, Cdouble, Int32),
                                   handle, Int32(which), Int64(size(A, 1)), At, bv, Float64(lambda), factor == :newton ? Int32(0) : Int32(1)))
end
# test entry: the host emulation of the LeastSquares prox (no GPU needed)
function host_least_squares(A::Matrix{Float64}, b::Vector{Float64}, lambda::Real, x::Vector{Float64})
    At = Matrix{Float64}(transpose(A))
    y = similar(x)
    check(ccall((:fos_host_least_squares, libfoship), Cint, (Int64, Int64, Ptr{Cdouble}, Ptr{Cdouble}, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}),
                Int64(size(A, 1)), Int64(size(A, 2)), At, b, Float64(lambda), x, y))
    return y
end
# The n-space forms (csrc/nspace.hip): y = M^-1 (x + c) with M and its inverse kept as packed triangles, three tile products per prox, n <= 46 000.
# Quadratic(Q, q): M = I + Q (only the lower triangle of Q is read: the transposed copy's lower triangle is the caller's upper one, the same matrix when Q is symmetric)
const FOS_LS_FORM_SPARSE_FACTORED = Int32(0)
const FOS_LS_FORM_NORMAL = Int32(1)
function feas_set_quadratic!(handle::Ptr{Cvoid}, which::Integer, Q::AbstractMatrix, q::AbstractVector, factor::Symbol = :cholesky)
    Qt = Matrix{Float64}(transpose(Q))                      # row-major for the C ABI
    qv = Vector{Float64}(q)
    GC.@preserve Qt qv check(ccall((:fos_feas_set_quadratic, libfoship), Cint, (Ptr{Cvoid}, Int32, Ptr{Cdouble}, Ptr{Cdouble}, Int32),
                                   handle, Int32(which), Qt, qv, factor == :newton ? Int32(0) : Int32(1)))
end
# LeastSquares(A, b, lambda) in the normal-equations form, M = I + lambda A'A: a dense A of any m (the tall A that fos_feas_set_least_squares refuses)
function feas_set_least_squares_normal!(handle::Ptr{Cvoid}, which::Integer, A::AbstractMatrix, b::AbstractVector, lambda::Real, factor::Symbol = :cholesky)
    At = Matrix{Float64}(transpose(A))
    bv = Vector{Float64}(b)
    GC.@preserve At bv check(ccall((:fos_feas_set_least_squares_normal, libfoship), Cint, (Ptr{Cvoid}, Int32, Int64, Ptr{Cdouble}, Ptr{Cdouble}, Cdouble, Int32),
                                   handle, Int32(which), Int64(size(A, 1)), At, bv, Float64(lambda), factor == :newton ? Int32(0) : Int32(1)))
end
# ... over a sparse A: form = :normal (any m, n <= 46 000) or :sparse_factored (m <= min(n, 46 000): the sparse factored IndAffine with a shifted diagonal)
function feas_set_least_squares_sparse!(handle::Ptr{Cvoid}, which::Integer, A::SparseArrays.SparseMatrixCSC, b::AbstractVector, lambda::Real, form::Symbol,
                                        factor::Symbol = :cholesky)
    As = SparseArrays.SparseMatrixCSC{Float64,Int64}(A)
    bv = Vector{Float64}(b)
    GC.@preserve As bv check(ccall((:fos_feas_set_least_squares_sparse, libfoship), Cint,
                                   (Ptr{Cvoid}, Int32, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Cdouble}, Ptr{Cdouble}, Cdouble, Int32, Int32),
                                   handle, Int32(which), Int64(size(As, 1)), As.colptr, As.rowval, As.nzval, bv, Float64(lambda),
                                   form == :normal ? FOS_LS_FORM_NORMAL : FOS_LS_FORM_SPARSE_FACTORED, factor == :newton ? Int32(0) : Int32(1)))
end
function feas_nspace_stats(handle::Ptr{Cvoid}, which::Integer)
    out = zeros(Float64, 8)
    check(ccall((:fos_feas_nspace_stats, libfoship), Cint, (Ptr{Cvoid}, Int32, Ptr{Cdouble}), handle, Int32(which), out))
    return (n = Int(out[1]), m = Int(out[2]), factor = out[3] == 1 ? :cholesky : :newton, fell_back = out[4] != 0, probe_resid = out[5], launches = Int(out[6]),
            bytes = Int(out[7]), tiles = Int(out[8]))
end
# test entries: the host emulations of the n-space forms and of the one-right-hand-side tile product (no GPU needed)
function host_quadratic(Q::Matrix{Float64}, q::Vector{Float64}, x::Vector{Float64})
    Qt = Matrix{Float64}(transpose(Q))
    y = similar(x)
    check(ccall((:fos_host_quadratic, libfoship), Cint, (Int64, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}), Int64(length(x)), Qt, q, x, y))
    return y
end
function host_least_squares_normal(A::Matrix{Float64}, b::Vector{Float64}, lambda::Real, x::Vector{Float64})
    At = Matrix{Float64}(transpose(A))
    y = similar(x)
    check(ccall((:fos_host_least_squares_normal, libfoship), Cint, (Int64, Int64, Ptr{Cdouble}, Ptr{Cdouble}, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}),
                Int64(size(A, 1)), Int64(size(A, 2)), At, b, Float64(lambda), x, y))
    return y
end
function host_least_squares_sparse(A::SparseArrays.SparseMatrixCSC{Float64,Int64}, b::Vector{Float64}, lambda::Real, form::Symbol, x::Vector{Float64})
    y = similar(x)
    check(ccall((:fos_host_least_squares_sparse, libfoship), Cint,
                (Int64, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Cdouble}, Ptr{Cdouble}, Cdouble, Int32, Ptr{Cdouble}, Ptr{Cdouble}),
                Int64(size(A, 1)), Int64(size(A, 2)), A.colptr, A.rowval, A.nzval, b, Float64(lambda),
                form == :normal ? FOS_LS_FORM_NORMAL : FOS_LS_FORM_SPARSE_FACTORED, x, y))
    return y
end
function host_symv_packed(X::Matrix{Float64}, v::Vector{Float64})
    y = similar(v)
    count = zeros(Int32, size(X))
    check(ccall((:fos_host_symv_packed, libfoship), Cint, (Int64, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Int32}), Int64(length(v)), X, v, y, count))
    return y, count
end
# The n-space forms by conjugate gradients (csrc/nspace_cg.hip): a SPARSE Q or A of any size, nothing dense kept; warm-started Jacobi-preconditioned CG ended on the
# recomputed residual at max(tol |x + c|, its rounding level).  Quadratic: only the entries i >= j of Q are read.
function feas_set_quadratic_sparse!(handle::Ptr{Cvoid}, which::Integer, Q::SparseArrays.SparseMatrixCSC, q::AbstractVector, tol::Real = 0.0)
    Qs = SparseArrays.SparseMatrixCSC{Float64,Int64}(Q)
    qv = Vector{Float64}(q)
    GC.@preserve Qs qv check(ccall((:fos_feas_set_quadratic_sparse, libfoship), Cint, (Ptr{Cvoid}, Int32, Ptr{Int64}, Ptr{Int64}, Ptr{Cdouble}, Ptr{Cdouble}, Cdouble),
                                   handle, Int32(which), Qs.colptr, Qs.rowval, Qs.nzval, qv, Float64(tol)))
end
function feas_set_least_squares_cg!(handle::Ptr{Cvoid}, which::Integer, A::SparseArrays.SparseMatrixCSC, b::AbstractVector, lambda::Real, tol::Real = 0.0)
    As = SparseArrays.SparseMatrixCSC{Float64,Int64}(A)
    bv = Vector{Float64}(b)
    GC.@preserve As bv check(ccall((:fos_feas_set_least_squares_cg, libfoship), Cint,
                                   (Ptr{Cvoid}, Int32, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Cdouble}, Ptr{Cdouble}, Cdouble, Cdouble),
                                   handle, Int32(which), Int64(size(As, 1)), As.colptr, As.rowval, As.nzval, bv, Float64(lambda), Float64(tol)))
end
function feas_nspace_cg_stats(handle::Ptr{Cvoid}, which::Integer)
    out = zeros(Float64, 8)
    check(ccall((:fos_feas_nspace_cg_stats, libfoship), Cint, (Ptr{Cvoid}, Int32, Ptr{Cdouble}), handle, Int32(which), out))
    return (calls = Int(out[1]), iters_total = Int(out[2]), last_iters = Int(out[3]), last_restarts = Int(out[4]), last_resid = out[5], last_level = out[6],
            stored = Int(out[7]), launches_per_iter = Int(out[8]))
end
# test entries: the host emulations of the cg forms (no GPU needed) -> y and the CG iterations taken
function host_quadratic_cg(Q::SparseArrays.SparseMatrixCSC{Float64,Int64}, q::Vector{Float64}, tol::Real, x::Vector{Float64})
    y = similar(x)
    iters = Ref{Int32}(0)
    check(ccall((:fos_host_quadratic_cg, libfoship), Cint, (Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Cdouble}, Ptr{Cdouble}, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}, Ref{Int32}),
                Int64(length(x)), Q.colptr, Q.rowval, Q.nzval, q, Float64(tol), x, y, iters))
    return y, Int(iters[])
end
function host_least_squares_cg(A::SparseArrays.SparseMatrixCSC{Float64,Int64}, b::Vector{Float64}, lambda::Real, tol::Real, x::Vector{Float64})
    y = similar(x)
    iters = Ref{Int32}(0)
    check(ccall((:fos_host_least_squares_cg, libfoship), Cint,
                (Int64, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Cdouble}, Ptr{Cdouble}, Cdouble, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}, Ref{Int32}),
                Int64(size(A, 1)), Int64(size(A, 2)), A.colptr, A.rowval, A.nzval, b, Float64(lambda), Float64(tol), x, y, iters))
    return y, Int(iters[])
end
# test entry: the host emulation of the sparse factored IndAffine (no GPU needed)
function host_affine_sparse_factored(A::SparseArrays.SparseMatrixCSC{Float64,Int64}, b::Vector{Float64}, refine::Integer, x::Vector{Float64})
    y = similar(x)
    check(ccall((:fos_host_affine_sparse_factored, libfoship), Cint, (Int64, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Cdouble}, Ptr{Cdouble}, Int32, Ptr{Cdouble}, Ptr{Cdouble}),
                Int64(size(A, 1)), Int64(size(A, 2)), A.colptr, A.rowval, A.nzval, b, Int32(refine), x, y))
    return y
end
# test entry: the host emulation of one block's projection (no GPU needed)
function host_set_project(kind::Integer, scal::NTuple{2,Float64}, v::Union{Nothing,Vector{Float64}}, x::Vector{Float64})
    y = similar(x)
    passes = Ref{Int32}(0)
    sc = [scal[1], scal[2]]
    check(ccall((:fos_host_set_project, libfoship), Cint, (Int32, Int64, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ref{Int32}),
                Int32(kind), Int64(length(x)), sc, v === nothing ? C_NULL : pointer(v), x, y, passes))
    return y, Int(passes[])
end

mutable struct HipFeasData <: FOSSolverData
    handle::Ptr{Cvoid}
    lsinterval::Int64                     # > 0: LineSearchWrapper around the algorithm
    gappinterval::Int64                   # > 0: GAPP, its search interval
    sets::Vector{Base.RefValue{Any}}      # callback sets, kept alive as long as the handle
    function HipFeasData(model::FeasibilityModel, device::Integer)
        h = Ref{Ptr{Cvoid}}(C_NULL)
        check(ccall((:fos_feas_create, libfoship), Cint, (Int64, Int32, Ref{Ptr{Cvoid}}), Int64(model.n), Int32(device), h))
        d = new(h[], 0, 0, Base.RefValue{Any}[])
        finalizer(x -> ccall((:fos_feas_destroy, libfoship), Cint, (Ptr{Cvoid},), x.handle), d)
        for (which, S) in ((Int32(1), model.S1), (Int32(2), model.S2))
            if S isa ProximalOperators.IndBox && (S.lb isa AbstractArray || S.ub isa AbstractArray)
                lo = S.lb isa AbstractArray ? Vector{Float64}(vec(S.lb)) : fill(Float64(S.lb), model.n)
                hi = S.ub isa AbstractArray ? Vector{Float64}(vec(S.ub)) : fill(Float64(S.ub), model.n)
                GC.@preserve lo hi check(ccall((:fos_feas_set_box_arrays, libfoship), Cint, (Ptr{Cvoid}, Int32, Ptr{Cdouble}, Ptr{Cdouble}), d.handle, which, lo, hi))
            elseif S isa ProximalOperators.IndBox
                check(ccall((:fos_feas_set_box, libfoship), Cint, (Ptr{Cvoid}, Int32, Cdouble, Cdouble), d.handle, which, Float64(S.lb), Float64(S.ub)))
            elseif S isa ConeProduct                        # the reference's own cone stack [cones.jl:31-94]
                types, _, lens = conearrays(S)
                GC.@preserve types lens check(ccall((:fos_feas_set_cones, libfoship), Cint, (Ptr{Cvoid}, Int32, Int64, Ptr{Int32}, Ptr{Int64}),
                                                    d.handle, which, Int64(length(types)), types, lens))
            elseif S isa ProximalOperators.IndAffine && S.A isa AbstractMatrix && get(model.options, :affine_form, nothing) == :sparse_factored
                # solve!(...; affine_form = :sparse_factored [, affine_factor, affine_refine]): A stays sparse (the arrays of the SparseMatrixCSC as they are; a dense A is
                # converted) with the dense inverse of A A' (m <= 46 000, any n), a projection is two segmented sparse passes, a fixed number of launches
                As = SparseArrays.SparseMatrixCSC{Float64,Int64}(S.A)
                b = Vector{Float64}(S.b)
                factor = get(model.options, :affine_factor, :cholesky) == :newton ? Int32(0) : Int32(1)      # FOS_DIRECT_FACTOR_*
                GC.@preserve As b check(ccall((:fos_feas_set_affine_sparse_factored, libfoship), Cint,
                                              (Ptr{Cvoid}, Int32, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Cdouble}, Ptr{Cdouble}, Int32, Int32),
                                              d.handle, which, Int64(size(As, 1)), As.colptr, As.rowval, As.nzval, b, factor, Int32(get(model.options, :affine_refine, 0))))
            elseif S isa ProximalOperators.IndAffine && S.A isa AbstractMatrix && get(model.options, :affine_form, nothing) == :factored
                # solve!(...; affine_form = :factored [, affine_factor = :cholesky | :newton, affine_refine = 0..2]): A (a sparse one densified) kept once with the
                # inverse of A A' (m <= 46 000, any n), a projection is two passes over A
                At = Matrix{Float64}(transpose(S.A))
                b = Vector{Float64}(S.b)
                factor = get(model.options, :affine_factor, :cholesky) == :newton ? Int32(0) : Int32(1)      # FOS_DIRECT_FACTOR_*
                GC.@preserve At b check(ccall((:fos_feas_set_affine_factored, libfoship), Cint, (Ptr{Cvoid}, Int32, Int64, Ptr{Cdouble}, Ptr{Cdouble}, Int32, Int32),
                                              d.handle, which, Int64(size(S.A, 1)), At, b, factor, Int32(get(model.options, :affine_refine, 0))))
            elseif S isa ProximalOperators.IndAffine && S.A isa AbstractMatrix && !(S.A isa SparseArrays.AbstractSparseMatrix)
                At = Matrix{Float64}(transpose(S.A))        # IndAffine(A, b), dense: the C ABI takes A row-major = column-major A'
                b = Vector{Float64}(S.b)
                GC.@preserve At b check(ccall((:fos_feas_set_affine, libfoship), Cint, (Ptr{Cvoid}, Int32, Int64, Ptr{Cdouble}, Ptr{Cdouble}),
                                              d.handle, which, Int64(size(S.A, 1)), At, b))
            elseif S isa ProximalOperators.IndAffine && S.A isa SparseArrays.SparseMatrixCSC
                # IndAffine(A, b) over a sparse A stays sparse on the device (any n): the arrays of the SparseMatrixCSC as they are (1-based)
                As = SparseArrays.SparseMatrixCSC{Float64,Int64}(S.A)
                b = Vector{Float64}(S.b)
                GC.@preserve As b check(ccall((:fos_feas_set_affine_sparse, libfoship), Cint,
                                              (Ptr{Cvoid}, Int32, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Cdouble}, Ptr{Cdouble}),
                                              d.handle, which, Int64(size(As, 1)), As.colptr, As.rowval, As.nzval, b))
            elseif S isa ProximalOperators.LeastSquares && hasproperty(S, :A) && S.A isa Matrix && hasproperty(S, :lambda) && size(S.A, 1) <= min(size(S.A, 2), 46000)
                feas_set_least_squares!(d.handle, which, S.A, S.b, S.lambda, get(model.options, :affine_factor, :cholesky))
            elseif S isa ProximalOperators.LeastSquares && hasproperty(S, :A) && S.A isa Matrix && hasproperty(S, :lambda) && size(S.A, 2) <= 46000
                # a tall dense A (or m > 46 000): the normal-equations form in the n-space
                feas_set_least_squares_normal!(d.handle, which, S.A, S.b, S.lambda, get(model.options, :affine_factor, :cholesky))
            elseif S isa ProximalOperators.LeastSquares && hasproperty(S, :A) && S.A isa SparseArrays.SparseMatrixCSC && hasproperty(S, :lambda) &&
                   (size(S.A, 1) <= min(size(S.A, 2), 46000) || size(S.A, 2) <= 46000)
                # a sparse A: wide, it stays sparse with the dense inverse of A A' + I/lambda; tall, the normal-equations form
                feas_set_least_squares_sparse!(d.handle, which, S.A, S.b, S.lambda, size(S.A, 1) <= min(size(S.A, 2), 46000) ? :sparse_factored : :normal,
                                               get(model.options, :affine_factor, :cholesky))
            elseif S isa ProximalOperators.Quadratic && hasproperty(S, :Q) && S.Q isa Matrix && size(S.Q, 1) <= 46000
                feas_set_quadratic!(d.handle, which, S.Q, S.q, get(model.options, :affine_factor, :cholesky))      # a dense Q: the n-space form
            elseif S isa ProximalOperators.Quadratic && hasproperty(S, :Q) && S.Q isa SparseArrays.SparseMatrixCSC
                feas_set_quadratic_sparse!(d.handle, which, S.Q, S.q, get(model.options, :cg_tol, 0.0))      # a sparse Q of any order: CG in the n-space
            elseif S isa ProximalOperators.LeastSquares && hasproperty(S, :A) && S.A isa SparseArrays.SparseMatrixCSC && hasproperty(S, :lambda)
                # a sparse A beyond both kept-inverse forms (n > 46 000 and m > min(n, 46 000)): CG in the n-space, nothing dense
                feas_set_least_squares_cg!(d.handle, which, S.A, S.b, S.lambda, get(model.options, :cg_tol, 0.0))
            elseif vectorset_block(S) !== nothing           # a ball, simplex, halfspace, hyperslab, point, the free set or a separable function: one block of length n
                feas_set_blocks!(d.handle, which, model.n, [(vectorset_block(S)..., Int64(model.n))])
            else                                            # any other ProximableFunction: prox!(y, S, x) on host vectors [Feasibility.jl:2-6]
                push!(d.sets, Ref{Any}(S))                  # (rooted: the library keeps a pointer to it)
                check(ccall((:fos_feas_set_callback, libfoship), Cint, (Ptr{Cvoid}, Int32, Ptr{Cvoid}, Ptr{Cvoid}),
                            d.handle, which, PROX_TRAMPOLINE[], pointer_from_objref(d.sets[end])))
            end
        end
        return d
    end
end

getcgiter(::HipFeasData) = 0

for T in (:GAP, :GAPA, :FISTA, :Dykstra)
    @eval function init_algorithm!(alg::$T, model::FeasibilityModel)
        if get(model.options, :gpu, false) === true
            data = HipFeasData(model, get(model.options, :device, 0))
            check(ccall((:fos_feas_set_alg, libfoship), Cint, (Ptr{Cvoid}, Cint, Cdouble, Cdouble, Cdouble, Cdouble), data.handle, algargs(alg)...))
            status_generator = (mo, checki, eps, verbose, debug) ->            # Feasibility.jl:76-78
                FeasibilityStatus(mo.n, 0, mo, fill(NaN, mo.n), Array{Array{Float64,1},1}(), :Continue, checki, eps, verbose, false, true,
                                  time_ns(), mo.init_duration, debug)
            return data, status_generator
        end
        return invoke(init_algorithm!, Tuple{$T,FirstOrderSolvers.AbstractFOSModel}, alg, model)
    end
end

# LineSearchWrapper(GAP / GAPA) on the Feasibility form (test/testfeasibility.jl:36-44): the wrapped algorithm's handle with the
# search switched on; what linesearch.jl prints during a search comes from fos_feas_linesearch_log
function init_algorithm!(long::LongstepWrapper, model::FeasibilityModel)      # [wrappers/longstep.jl] on the Feasibility form: fos_feas_set_longstep
    if usegpu(model)
        !FirstOrderSolvers.support_longstep(long.alg) && @error "Algorithm alg does not support longstep"
        data, status_generator = init_algorithm!(long.alg, model)
        check(ccall((:fos_feas_set_longstep, libfoship), Cint, (Ptr{Cvoid}, Int64, Int64), data.handle, Int64(long.longinterval), Int64(long.nsave)))
        return data, status_generator
    end
    return invoke(init_algorithm!, Tuple{LongstepWrapper,FirstOrderSolvers.AbstractFOSModel}, long, model)
end
iterate(long::LongstepWrapper, data::HipFeasData, status::FeasibilityStatus, x, max_iters) = iterate(long.alg, data, status, x, max_iters)
getsol(long::LongstepWrapper, data::HipFeasData, x) = getsol(long.alg, data, x)
function init_algorithm!(ls::LineSearchWrapper, model::FeasibilityModel)
    if get(model.options, :gpu, false) === true
        data, status_generator = init_algorithm!(ls.alg, model)
        check(ccall((:fos_feas_set_linesearch, libfoship), Cint, (Ptr{Cvoid}, Int64), data.handle, ls.lsinterval))
        data.lsinterval = ls.lsinterval
        return data, status_generator
    end
    return invoke(init_algorithm!, Tuple{LineSearchWrapper,FirstOrderSolvers.AbstractFOSModel}, ls, model)
end
function print_linesearch(data::HipFeasData)
    log = Vector{Float64}(undef, 34)
    check(ccall((:fos_feas_linesearch_log, libfoship), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), data.handle, log))
    println("test, $(log[1])")
    α = 0.1
    for k = 0:30
        α = α * 1.8
        println("α: $α, $(log[2+k])")
    end
    println("α: $(log[33])")
end

# GAPP ("projected GAP", solvers/gapproj.jl) on the Feasibility form: every iproj-th iteration is a 21-point search on the device
import ..FirstOrderSolvers: GAPP
function init_algorithm!(alg::GAPP, model::FeasibilityModel)
    if get(model.options, :gpu, false) === true
        data = HipFeasData(model, get(model.options, :device, 0))
        check(ccall((:fos_feas_set_gapp, libfoship), Cint, (Ptr{Cvoid}, Cdouble, Cdouble, Cdouble, Int64), data.handle, alg.α, alg.α1, alg.α2, Int64(alg.iproj)))
        data.gappinterval = alg.iproj
        status_generator = (mo, checki, eps, verbose, debug) ->
            FeasibilityStatus(mo.n, 0, mo, fill(NaN, mo.n), Array{Array{Float64,1},1}(), :Continue, checki, eps, verbose, false, true,
                              time_ns(), mo.init_duration, debug)
        return data, status_generator
    end
    return invoke(init_algorithm!, Tuple{GAPP,FirstOrderSolvers.AbstractFOSModel}, alg, model)
end
function print_gapp(data::HipFeasData)                       # gapproj.jl:51,57
    log = Vector{Float64}(undef, 23)
    check(ccall((:fos_feas_gapp_log, libfoship), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), data.handle, log))
    for k = 1:21
        println("normtest: $(log[k])")
    end
    println("αbest: $(log[22])")
end

function iterate(alg::FOSAlgorithm, data::HipFeasData, status::FeasibilityStatus, x, max_iters)
    t1 = time()
    printstatusheader(status)
    check(ccall((:fos_feas_set_iterate, libfoship), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), data.handle, x))
    i = 0
    done, st, err, checked = Ref{Int64}(0), Ref{Int32}(0), Ref{Cdouble}(NaN), Ref{Int32}(0)
    report = function ()
        t = time_ns() - status.init_time
        status.debug > 0 && savedata(status.i, err[], x, t, status.model, status.extra, min(status.debug, 1))     # FeasibilityStatus.jl:42-45
        status.verbose > 0 && printstatusiter(status.i, err[], t)                                              # :46-54 (direct: no cg column)
        status.status = STATUS_SYMBOLS[st[] + 1]
        status.verbose > 0 && status.status == :Optimal && println("Found solution i=$(status.i)")
        status.checked = true
    end
    while i < max_iters
        count = min(max_iters - i, status.checki - (i % status.checki))
        ls = data.lsinterval
        ls > 0 && (count = min(count, ls - (i % ls)))
        gp = data.gappinterval
        gp > 0 && (count = min(count, gp - (i % gp)))
        check(ccall((:fos_feas_step, libfoship), Cint,
                    (Ptr{Cvoid}, Int64, Int64, Int64, Cdouble, Ref{Int64}, Ref{Int32}, Ref{Cdouble}, Ref{Int32}),
                    data.handle, i + 1, count, status.checki, status.eps, done, st, err, checked))
        i += done[]
        status.i = i
        ls > 0 && i % ls == 0 && print_linesearch(data)
        gp > 0 && i % gp == 0 && print_gapp(data)
        if checked[] != 0
            report()
            status.status != :Continue && break
        else
            status.checked = false
        end
    end
    guess = Vector{Float64}(undef, length(x))
    force = status.checked ? Int32(0) : Int32(1)                                   # solverwrapper.jl:31-34
    check(ccall((:fos_feas_getsol, libfoship), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Int32, Cdouble, Ref{Int32}, Ref{Cdouble}),
                data.handle, guess, force, status.eps, st, err))
    force != 0 && report()
    if status.verbose > 0
        println("Time for iterations: ")
        println("$(time() - t1) s")
    end
    return guess
end

function __init__()
    PROX_TRAMPOLINE[] = @cfunction(prox_trampoline, Int32, (Ptr{Cvoid}, Int64, Ptr{Cdouble}, Ptr{Cdouble}))
end

end # module
