// gfx950 code objects of the FMPC problem types with time-varying input / inequality dimensions shipped with the library (a
// translation unit of their own, so that fmpc_models.hip compiles to what it compiled to before they existed).
#include <nmpc_amd/hip/fmpc_ops.hpp>
#include <nmpc_amd/models/FmpcVerticalMotion.hpp>

using nmpc_amd::FmpcProblemVerticalMotion;

NMPC_AMD_REGISTER_FMPC_PROBLEM(FmpcProblemVerticalMotion)
