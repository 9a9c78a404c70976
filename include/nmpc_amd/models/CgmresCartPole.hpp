// Cart-pole swing-up problems for the MI355X C/GMRES solver.
//
// The system of the reference's C/GMRES test (nmpc_cgmres/tests/src/CartPoleProblem.h:11-210), restated from its equations
// of motion rather than from that file's code: a cart of mass m1 on a rail, a pole of mass m2 and length l, the pole
// upright at theta = 0 (hanging down at theta = pi, the reference's x_initial_), horizontal force f on the cart.  With
// s = sin(theta), c = cos(theta), D = m1 + m2 s^2:
//
//   p''     = (f - m2 l theta'^2 s + m2 g s c) / D
//   theta'' = (f c - m2 l theta'^2 s c + g (m1 + m2) s) / (l D)
//
// Running cost 1/2 sum_i q_i (x_i - ref_i)^2 + 1/2 r1 f^2, terminal cost 1/2 sum_i sf_i (x_i - ref_i)^2.  The costate
// equation is -dH/dx of the Hamiltonian H = running cost + lmd . f(x, u), DhDu is dH/d(u, mu).
//
// Two registered types, as the reference's constructor flag with_input_bound selects (CartPoleProblem.h:19-42):
//   * cgmres_cartpole (4, 1, 0): the force alone,
//   * cgmres_cartpole_with_input_bound (4, 2, 1): |f| <= f_max as the equality f^2 + f_dummy^2 = f_max^2 with a dummy input,
//     multiplier mu, and the term -r2 f_dummy in the running cost.
// The reference state is a constant member of the problem object (a per-instance target when set_problem is given one object
// per instance); the reference's default RefFunc returns zero (CartPoleProblem.h:58-63).  Time-varying references are not
// offered.
#pragma once

#include <nmpc_amd/CgmresProblem.hpp>

namespace nmpc_amd
{
template<bool kInputBound>
class CgmresProblemCartPoleT : public CgmresProblem<4, kInputBound ? 2 : 1, kInputBound ? 1 : 0>
{
public:
  static constexpr const char * kName = kInputBound ? "cgmres_cartpole_with_input_bound" : "cgmres_cartpole";

  // the parameter block (all doubles, in this order: the C-ABI's default_params and the Python mirror rely on it)
  double m1 = 1.0; //!< cart mass (state_eq_param_(0))
  double m2 = 1.0; //!< pole mass (state_eq_param_(1))
  double l = 1.0; //!< pole length (state_eq_param_(2))
  double f_max = 100.0; //!< force bound of the bounded variant (state_eq_param_(3))
  double q[4] = {10, 100, 1, 10}; //!< running state weights (obj_weight_(0..3))
  double r1 = 10; //!< running force weight (obj_weight_(4))
  double r2 = 0.01; //!< dummy-input weight of the bounded variant (obj_weight_(5))
  double sf[4] = {100, 300, 1, 10}; //!< terminal weights (terminal_obj_weight_)
  double ref[4] = {0, 0, 0, 0}; //!< constant reference state
  double g = 9.80665; //!< gravity

  NMPC_HD static void initialState(double * x)
  {
    x[0] = 0;
    x[1] = M_PI;
    x[2] = 0;
    x[3] = 0;
  }

  NMPC_HD static void initialInput(double * u)
  {
    u[0] = 0;
    if(kInputBound)
    {
      u[1] = 1.0;
      u[2] = 0.01;
    }
  }

  NMPC_HD void stateEquation(double, // t
                             const double * x,
                             const double * u,
                             double * dotx) const
  {
    double s, c;
    sincos(x[1], s, c);
    const double D = m1 + m2 * (s * s);
    const double w2 = x[3] * x[3];
    dotx[0] = x[2];
    dotx[1] = x[3];
    dotx[2] = (u[0] - m2 * l * w2 * s + m2 * g * s * c) / D;
    dotx[3] = (u[0] * c - m2 * l * w2 * s * c + g * (m1 + m2) * s) / (l * D);
  }

  NMPC_HD void costateEquation(double, // t
                               const double * lmd,
                               const double * xu,
                               double * dotlmd) const
  {
    const double * x = xu;
    const double f = xu[4];
    double s, c;
    sincos(x[1], s, c);
    const double D = m1 + m2 * (s * s);
    const double dD = 2 * m2 * s * c; // dD/dtheta
    const double w = x[3], w2 = w * w;
    const double c2s2 = c * c - s * s; // cos(2 theta)
    // numerators of p'' and l theta'' and their theta derivatives
    const double Na = f - m2 * l * w2 * s + m2 * g * s * c;
    const double dNa = -m2 * l * w2 * c + m2 * g * c2s2;
    const double Nb = f * c - m2 * l * w2 * s * c + g * (m1 + m2) * s;
    const double dNb = -f * s - m2 * l * w2 * c2s2 + g * (m1 + m2) * c;
    const double dpdd_dtheta = (dNa * D - Na * dD) / (D * D);
    const double dthdd_dtheta = (dNb * D - Nb * dD) / (l * D * D);
    const double dpdd_dw = -2 * m2 * l * w * s / D;
    const double dthdd_dw = -2 * m2 * w * s * c / D;
    dotlmd[0] = -(q[0] * (x[0] - ref[0]));
    dotlmd[1] = -(q[1] * (x[1] - ref[1]) + lmd[2] * dpdd_dtheta + lmd[3] * dthdd_dtheta);
    dotlmd[2] = -(q[2] * (x[2] - ref[2]) + lmd[0]);
    dotlmd[3] = -(q[3] * (x[3] - ref[3]) + lmd[1] + lmd[2] * dpdd_dw + lmd[3] * dthdd_dw);
  }

  NMPC_HD void calcDphiDx(double, // t
                          const double * x,
                          double * DphiDx) const
  {
    for(int i = 0; i < 4; i++)
    {
      DphiDx[i] = sf[i] * (x[i] - ref[i]);
    }
  }

  NMPC_HD void calcDhDu(double, // t
                        const double * x,
                        const double * u,
                        const double * lmd,
                        double * DhDu) const
  {
    double s, c;
    sincos(x[1], s, c);
    const double D = m1 + m2 * (s * s);
    DhDu[0] = r1 * u[0] + lmd[2] / D + lmd[3] * c / (l * D);
    if(kInputBound)
    {
      const double f = u[0], fd = u[1], mu = u[2];
      DhDu[0] += 2 * mu * f;
      DhDu[1] = -r2 + 2 * mu * fd;
      DhDu[2] = f * f + fd * fd - f_max * f_max;
    }
  }
};

using CgmresProblemCartPole = CgmresProblemCartPoleT<false>;
using CgmresProblemCartPoleWithInputBound = CgmresProblemCartPoleT<true>;
} // namespace nmpc_amd
