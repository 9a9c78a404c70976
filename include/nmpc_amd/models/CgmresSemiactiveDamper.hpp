// Semi-active damper problem for the MI355X C/GMRES solver.
//
// The system of the reference's C/GMRES test (nmpc_cgmres/tests/src/SemiactiveDamperProblem.h:10-118; Ohtsuka's textbook
// example), restated from its equations: a unit mass on a spring, x = (position, velocity), a damper whose coefficient u0
// the controller sets within [0, u_max]:
//
//   x0' = x1,   x1' = a x0 + b x1 u0                       (a = b = -1, u_max = 1)
//
// The bound is the equality (u0 - u_max/2)^2 + u1^2 = u_max^2/4 with a dummy input u1 and multiplier mu (dim (2, 2, 1)).
// Running cost 1/2 (q1 x0^2 + q2 x1^2 + r1 u0^2) - r2 u1, terminal cost 1/2 (sf1 x0^2 + sf2 x1^2).
//
// The costate equation is -dH/dx of H = running cost + lmd . x' + mu (bound):
//   lmd0' = -(q1 x0 + a lmd1),   lmd1' = -(q2 x1 + lmd0 + b lmd1 u0)
// with the damper coefficient u0.  The reference's costateEquation reads its inputs as xu.tail(dim_u_)
// (SemiactiveDamperProblem.h:52-67), i.e. (u1, mu), and so multiplies b lmd1 by the dummy input u1 instead; this class
// follows the Hamiltonian, so its closed loops differ from the reference's in that term.
#pragma once

#include <nmpc_amd/CgmresProblem.hpp>

namespace nmpc_amd
{
class CgmresProblemSemiactiveDamper : public CgmresProblem<2, 2, 1>
{
public:
  static constexpr const char * kName = "cgmres_semiactive_damper";

  // the parameter block (all doubles, in this order)
  double a = -1; //!< state_eq_param_(0)
  double b = -1; //!< state_eq_param_(1)
  double u_max = 1; //!< state_eq_param_(2)
  double q1 = 1, q2 = 10, r1 = 1, r2 = 1e-1; //!< obj_weight_
  double sf1 = 1, sf2 = 10; //!< terminal_obj_weight_

  NMPC_HD static void initialState(double * x)
  {
    x[0] = 2;
    x[1] = 0;
  }

  NMPC_HD static void initialInput(double * u)
  {
    u[0] = 0.01;
    u[1] = 0.9;
    u[2] = 0.03;
  }

  NMPC_HD void stateEquation(double, // t
                             const double * x,
                             const double * u,
                             double * dotx) const
  {
    dotx[0] = x[1];
    dotx[1] = a * x[0] + b * x[1] * u[0];
  }

  NMPC_HD void costateEquation(double, // t
                               const double * lmd,
                               const double * xu,
                               double * dotlmd) const
  {
    const double * x = xu;
    const double u0 = xu[2];
    dotlmd[0] = -(q1 * x[0] + a * lmd[1]);
    dotlmd[1] = -(q2 * x[1] + lmd[0] + b * lmd[1] * u0);
  }

  NMPC_HD void calcDphiDx(double, // t
                          const double * x,
                          double * DphiDx) const
  {
    DphiDx[0] = sf1 * x[0];
    DphiDx[1] = sf2 * x[1];
  }

  NMPC_HD void calcDhDu(double, // t
                        const double * x,
                        const double * u,
                        const double * lmd,
                        double * DhDu) const
  {
    const double mu = u[2];
    const double d0 = u[0] - u_max / 2.0;
    DhDu[0] = r1 * u[0] + b * lmd[1] * x[1] + mu * (2 * u[0] - u_max);
    DhDu[1] = -r2 + 2 * mu * u[1];
    DhDu[2] = d0 * d0 + u[1] * u[1] - u_max * u_max / 4.0;
  }
};
} // namespace nmpc_amd
