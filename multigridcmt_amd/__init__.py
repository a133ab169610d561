"""multigridcmt_amd — the geometric-multigrid V-cycle path of AndyMN/MultigridCMT on AMD MI355X.

Host side: the reference's three classes with unchanged signatures.  Device side: hand-written HIP
kernels for gfx950 behind the C-ABI of include/mgcmt_hip.h (libmgcmt_hip.so, bound with ctypes).
"""
from .operators import (StructuredOperator, UnrecognisedOperator, identity_operator, laplacian_operator,
                        potential_operator, potential_well_operator, recognise, recognise_27_point, recognise_five_point, recognise_nine_point,
                        recognise_potential, recognise_seven_point, tensor_mass_operator, variable_mass_operator)
from .plan import Plan, get_plan, release_plans
from .processor import MGCMTProcessor
from .solver import MGCMTSolver
from .stencil_maker import MGCMTStencilMaker

__all__ = ["MGCMTSolver", "MGCMTStencilMaker", "MGCMTProcessor", "StructuredOperator", "UnrecognisedOperator",
           "laplacian_operator", "identity_operator", "potential_well_operator", "potential_operator", "recognise",
           "recognise_potential", "variable_mass_operator", "recognise_five_point", "recognise_seven_point",
           "tensor_mass_operator", "recognise_nine_point", "recognise_27_point", "Plan", "get_plan", "release_plans"]
