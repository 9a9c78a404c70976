// Problem functor API of the MI355X C/GMRES solver.
//
// Keeps the interface of the reference's abstract class nmpc_cgmres::CgmresProblem
// (nmpc_cgmres/include/nmpc_cgmres/CgmresProblem.h:14-72) method for method — same names, same argument order, same
// meaning — so a user problem carries over by
//   * deriving from nmpc_amd::CgmresProblem<StateDim, InputDim, ConstraintDim> instead of nmpc_cgmres::CgmresProblem
//     (dim_x_ / dim_u_ / dim_c_ / dim_uc_ become compile-time constants; dim_uc_ = InputDim + ConstraintDim),
//   * marking the four methods NMPC_HD (host + device, non-virtual: the solver is instantiated on the concrete type),
//   * replacing Eigen::Ref<> arguments by plain arrays: x, lmd, dotx, dotlmd, DphiDx [dim_x_], u, DhDu [dim_uc_],
//     xu [dim_x_ + dim_uc_] (the state followed by the inputs and the constraint multipliers),
//   * keeping every member trivially copyable (the problem object IS the parameter block the solver copies to the device:
//     no Eigen vectors, no std::function — a constant per-instance reference replaces the reference's RefFunc),
//   * turning x_initial_ / u_initial_ into the static functions initialState / initialInput, and giving the class a kName.
//
// Methods a problem must provide (CgmresProblem.h:29-55):
//
//   void stateEquation(double t, const double * x, const double * u, double * dotx) const;
//   void costateEquation(double t, const double * lmd, const double * xu, double * dotlmd) const;
//   void calcDphiDx(double t, const double * x, double * DphiDx) const;
//   void calcDhDu(double t, const double * x, const double * u, const double * lmd, double * DhDu) const;
//   static void initialState(double * x);   // x_initial_
//   static void initialInput(double * u);   // u_initial_ (inputs followed by the constraint multipliers)
//
// and is made known to the C-ABI with NMPC_AMD_REGISTER_CGMRES_PROBLEM(ProblemType) in one HIP translation unit
// (nmpc_amd/csrc/cgmres_models.hip shows the shipped ones).  dumpData (CgmresProblem.h:58-61) is the Python mirror's
// CgmresSolverBatch.dump.
#pragma once

#include <nmpc_amd/linalg.hpp>

namespace nmpc_amd
{
/** \brief C/GMRES problem.
    \tparam StateDim state dimension
    \tparam InputDim input dimension
    \tparam ConstraintDim equality-constraint dimension (one Lagrange multiplier per row, appended to the input) */
template<int StateDim, int InputDim, int ConstraintDim>
class CgmresProblem
{
  static_assert(StateDim > 0 && InputDim > 0 && ConstraintDim >= 0, "[C/GMRES] dimensions must be fixed and positive");

public:
  static constexpr int dim_x_ = StateDim;
  static constexpr int dim_u_ = InputDim;
  static constexpr int dim_c_ = ConstraintDim;
  static constexpr int dim_uc_ = InputDim + ConstraintDim;
};
} // namespace nmpc_amd
