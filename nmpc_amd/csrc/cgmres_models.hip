// gfx950 code objects of the C/GMRES problem types shipped with the library: the two problems of the reference's C/GMRES tests
// (nmpc_cgmres/tests/src/SemiactiveDamperProblem.h, CartPoleProblem.h), the cart-pole with and without its input bound.
#include <nmpc_amd/hip/cgmres_kernels.hpp>
#include <nmpc_amd/models/CgmresCartPole.hpp>
#include <nmpc_amd/models/CgmresSemiactiveDamper.hpp>

using nmpc_amd::CgmresProblemCartPole;
using nmpc_amd::CgmresProblemCartPoleWithInputBound;
using nmpc_amd::CgmresProblemSemiactiveDamper;

NMPC_AMD_REGISTER_CGMRES_PROBLEM(CgmresProblemSemiactiveDamper)
NMPC_AMD_REGISTER_CGMRES_PROBLEM(CgmresProblemCartPole)
NMPC_AMD_REGISTER_CGMRES_PROBLEM(CgmresProblemCartPoleWithInputBound)
