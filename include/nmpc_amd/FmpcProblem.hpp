// Problem functor API of the MI355X FMPC solver.
//
// Keeps the interface of the reference's abstract class nmpc_fmpc::FmpcProblem<StateDim, InputDim, IneqDim>
// (nmpc_fmpc/include/nmpc_fmpc/FmpcProblem.h:15-132), which is nmpc_ddp::DDPProblem<StateDim, InputDim> plus the inequality
// constraints g(t, x, u) <= 0 and their first derivatives.  A user problem carries over as described in DDPProblem.hpp
// (derive from nmpc_amd::FmpcProblem, NMPC_HD non-virtual methods, plain references instead of Eigen::Ref, trivially copyable
// members).  In addition to the DDPProblem methods a problem provides (FmpcProblem.h:94-109):
//
//   IneqDimVector ineqConst(double t, const StateDimVector & x, const InputDimVector & u) const;
//   void calcIneqConstDeriv(double t, const StateDimVector & x, const InputDimVector & u,
//                           IneqStateDimMatrix & ineq_const_deriv_x, IneqInputDimMatrix & ineq_const_deriv_u) const;
//
// The second-order overload of calcStateEqDeriv is private and throws in the reference (FmpcProblem.h:113-131): it does not
// exist here.
//
// Time-varying dimensions (the reference's Eigen::Dynamic InputDim / IneqDim, FmpcSolver.hpp:201-218, :310-345): pass
// nmpc_amd::Dynamic for InputDim and / or IneqDim together with a capacity (MaxInputDim, MaxIneqDim), and shadow
// `int inputDim(double t) const` / `int ineqDim(double t) const`.  The solver then sizes every step i of the horizon with
// inputDim(t0 + i dt) and ineqDim(t0 + i dt) and hands every callback its arguments already sized: u (m(t)), s / nu (g(t)),
// state_eq_deriv_u (n x m(t)), ineq_const_deriv_x (g(t) x n), ineq_const_deriv_u (g(t) x m(t)), running_cost_deriv_u /
// _uu / _xu (m(t), m(t) x m(t), n x m(t)); ineqConst returns g(t) rows.  The active inputs and rows are the LEADING ones of
// the capacity-sized arrays.  models/FmpcVerticalMotion.hpp is an example.
#pragma once

#include <nmpc_amd/DDPProblem.hpp>

namespace nmpc_amd
{
/** \brief Fast MPC problem.
    \tparam StateDim state dimension
    \tparam InputDim input dimension (fixed, or nmpc_amd::Dynamic)
    \tparam IneqDim inequality dimension (fixed, or nmpc_amd::Dynamic)
    \tparam MaxInputDim capacity of the input dimension when InputDim is Dynamic (ignored otherwise)
    \tparam MaxIneqDim capacity of the inequality dimension when IneqDim is Dynamic (ignored otherwise) */
template<int StateDim, int InputDim, int IneqDim, int MaxInputDim = InputDim, int MaxIneqDim = IneqDim>
class FmpcProblem : public DDPProblem<StateDim, InputDim, MaxInputDim>
{
  static_assert(IneqDim >= 0 || IneqDim == Dynamic, "[FMPC] Template param IneqDim should be non-negative or nmpc_amd::Dynamic.");
  static_assert(IneqDim != Dynamic || MaxIneqDim >= 0, "[FMPC] Dynamic inequality dimension needs MaxIneqDim.");

public:
  static constexpr bool kDynamicIneq = (IneqDim == Dynamic);
  static constexpr int kIneqDimMax = kDynamicIneq ? MaxIneqDim : IneqDim;
  //! capacity of the inequality dimension (= IneqDim when it is fixed)
  static constexpr int kIneqDim = kIneqDimMax;

  /** \brief Type of vector of inequality dimension. */
  using IneqDimVector = Matrix<double, kIneqDimMax, 1, kDynamicIneq, false>;
  /** \brief Type of matrix of inequality x state dimension. */
  using IneqStateDimMatrix = Matrix<double, kIneqDimMax, StateDim, kDynamicIneq, false>;
  /** \brief Type of matrix of inequality x input dimension. */
  using IneqInputDimMatrix =
      Matrix<double, kIneqDimMax, DDPProblem<StateDim, InputDim, MaxInputDim>::kInputDimMax, kDynamicIneq, (InputDim == Dynamic)>;

  /** \brief Constructor.
      \param dt discretization timestep [sec] */
  NMPC_HD explicit FmpcProblem(double dt) : DDPProblem<StateDim, InputDim, MaxInputDim>(dt) {}

  /** \brief Gets the inequality dimension (capacity when the dimension is dynamic; the reference throws there,
      FmpcProblem.h:63-74 — device code cannot, so callers must use ineqDim(t)). */
  NMPC_HD static constexpr int ineqDim()
  {
    return kIneqDimMax;
  }

  /** \brief Gets the inequality dimension at time t (FmpcProblem.h:76-87).  Must be shadowed by the problem if IneqDim is
      Dynamic. */
  NMPC_HD int ineqDim(double) const
  {
    return kIneqDimMax;
  }
};
} // namespace nmpc_amd
