"""
firstordersolvers.jl_amd -- MI355X-native hot path of FirstOrderSolvers.jl.

Host-side mirror of the reference's solver interface (GAP/DR/AP/GAPA/FISTA constructors,
FOSMathProgModel with loadproblem/optimize/status/getobjval/getsolution, model.history) over the
C-ABI shared library `csrc/libfoship.so` (hand-written HIP kernels for gfx950).  There is no CPU
fallback: every compute call goes through the library and fails loudly if it is missing.
"""
from . import _lib as lib          # noqa: F401
from . import workloads            # noqa: F401
from .interface import (AP, DR, FISTA, GAP, GAPA, GAPP, Dykstra, FOSAlgorithm, FOSMathProgModel, HipHSDE, HSDEStatus,  # noqa: F401
                        LineSearchWrapper, LongstepWrapper, Solution, solve, HEADER_CG, HEADER_DIRECT,
                        ConeProduct, Feasibility, FeasibilityModel, FeasibilitySolution, HipFeasibility, IndAffine, IndBox, IndBallL2, IndBallL1, IndSimplex, IndHalfspace,
                        IndHyperslab, IndPoint, IndFree, SeparableSum, NormL1, SqrNormL2, ElasticNet, Linear, NormL2, HuberLoss, NormLinf, LeastSquares, Quadratic, solve_feasibility, direct_factor_code, DIRECT_FACTOR_NAMES,
                        host_equilibrate, equilibrate_passes, host_cg_variant, host_cg_windows, host_lowp_cached, CG_VARIANT_FLAGS, CG_VARIANT_NAMES)
from . import sharding             # noqa: F401
