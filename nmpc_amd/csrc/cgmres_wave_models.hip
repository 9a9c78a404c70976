// gfx950 code objects of the wave kernels (one wavefront per controller, include/nmpc_amd/hip/cgmres_wave_kernels.hpp) of the
// C/GMRES problem types shipped with the library.  A translation unit of its own: the lane kernels of cgmres_models.hip stay as
// they are, and tests/test_cgmres_isa.py counts their instantiations per object.
#include <nmpc_amd/hip/cgmres_wave_kernels.hpp>
#include <nmpc_amd/models/CgmresCartPole.hpp>
#include <nmpc_amd/models/CgmresSemiactiveDamper.hpp>

using nmpc_amd::CgmresProblemCartPole;
using nmpc_amd::CgmresProblemCartPoleWithInputBound;
using nmpc_amd::CgmresProblemSemiactiveDamper;

NMPC_AMD_REGISTER_CGMRES_WAVE_PROBLEM(CgmresProblemSemiactiveDamper)
NMPC_AMD_REGISTER_CGMRES_WAVE_PROBLEM(CgmresProblemCartPole)
NMPC_AMD_REGISTER_CGMRES_WAVE_PROBLEM(CgmresProblemCartPoleWithInputBound)
