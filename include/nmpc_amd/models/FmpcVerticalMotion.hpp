// Vertical motion with a time-varying number of contacts for the MI355X FMPC solver: the FMPC counterpart of
// models/VerticalMotion.hpp (the reference's DDPProblemVerticalMotion, nmpc_ddp/tests/src/TestDDPVerticalMotion.cpp:31-234)
// with unilateral contact forces.  State [z, vz]; input: one vertical contact force per contact; inequality rows
// f_min - f_j <= 0 and f_j - f_max <= 0 per contact, so g(t) = 2 m(t).  Contacts: 1, then 2 in (double_support_begin_,
// double_support_end_), then 0 in (flight_begin_, flight_end_), then 1 again.  The schedule is part of the problem object, so
// per-instance objects may switch at different times.
// The loops over the contacts run to the capacity with a guard on the run-time size: unrolled, every index is a compile-time
// constant and the small arrays stay in registers (a loop bounded by u.size() indexes them at run time, which puts them in scratch).
#pragma once

#include <nmpc_amd/FmpcProblem.hpp>

namespace nmpc_amd
{
class FmpcProblemVerticalMotion : public FmpcProblem<2, Dynamic, Dynamic, 2, 4>
{
public:
  static constexpr const char * kName = "fmpc_vertical";
  static constexpr double g_ = 9.80665; // [m/s^2]

  NMPC_HD explicit FmpcProblemVerticalMotion(double dt = 0.01) : FmpcProblem(dt) {}

  /** Number of contacts at time t.  The comparisons are offset by 1e-6 s (as in VerticalMotion.hpp): a last-bit difference in
      t0 + i dt never moves a step across a switch time. */
  NMPC_HD int inputDim(double t) const
  {
    t += 1e-6;
    if(double_support_begin_ < t && t < double_support_end_)
    {
      return 2;
    }
    if(flight_begin_ < t && t < flight_end_)
    {
      return 0;
    }
    return 1;
  }

  NMPC_HD int ineqDim(double t) const
  {
    return 2 * inputDim(t);
  }

  NMPC_HD double refPos(double t) const
  {
    t += 1e-6;
    return (t < ref_switch_t_) ? 1.0 : 0.0; // [m]
  }

  NMPC_HD StateDimVector stateEq(double t, const StateDimVector & x, const InputDimVector & u) const
  {
    return stateEq(t, x, u, dt_);
  }

  NMPC_HD StateDimVector stateEq(double, // t
                                 const StateDimVector & x,
                                 const InputDimVector & u,
                                 double dt) const
  {
    double force = 0;
    NMPC_UNROLL
    for(int j = 0; j < kInputDimMax; j++)
    {
      if(j < u.size())
      {
        force += u[j];
      }
    }
    StateDimVector x_next;
    x_next[0] = x[0] + dt * x[1];
    x_next[1] = x[1] + dt * (force / mass_ - g_);
    return x_next;
  }

  NMPC_HD double runningCost(double t, const StateDimVector & x, const InputDimVector & u) const
  {
    const double e0 = x[0] - refPos(t);
    const double e1 = x[1];
    double uu = 0;
    NMPC_UNROLL
    for(int j = 0; j < kInputDimMax; j++)
    {
      if(j < u.size())
      {
        uu += u[j] * u[j];
      }
    }
    return 0.5 * (running_x_[0] * (e0 * e0) + running_x_[1] * (e1 * e1)) + 0.5 * running_u_ * uu;
  }

  NMPC_HD double terminalCost(double t, const StateDimVector & x) const
  {
    const double e0 = x[0] - refPos(t);
    const double e1 = x[1];
    return 0.5 * (terminal_x_[0] * (e0 * e0) + terminal_x_[1] * (e1 * e1));
  }

  NMPC_HD IneqDimVector ineqConst(double t, const StateDimVector &, const InputDimVector & u) const
  {
    IneqDimVector g(ineqDim(t));
    NMPC_UNROLL
    for(int j = 0; j < kInputDimMax; j++)
    {
      if(j < u.size())
      {
        g[2 * j] = f_min_ - u[j];
        g[2 * j + 1] = u[j] - f_max_;
      }
    }
    return g;
  }

  NMPC_HD void calcStateEqDeriv(double, // t
                                const StateDimVector &, // x
                                const InputDimVector & u,
                                StateStateDimMatrix & state_eq_deriv_x,
                                StateInputDimMatrix & state_eq_deriv_u) const
  {
    state_eq_deriv_x.setZero();
    state_eq_deriv_x(0, 1) = 1;
    state_eq_deriv_x *= dt_;
    state_eq_deriv_x.addToDiagonal(1.0);
    NMPC_UNROLL
    for(int j = 0; j < kInputDimMax; j++)
    {
      if(j < u.size())
      {
        state_eq_deriv_u(0, j) = 0;
        state_eq_deriv_u(1, j) = (1.0 / mass_) * dt_;
      }
    }
  }

  NMPC_HD void calcRunningCostDeriv(double t,
                                    const StateDimVector & x,
                                    const InputDimVector & u,
                                    StateDimVector & running_cost_deriv_x,
                                    InputDimVector & running_cost_deriv_u,
                                    StateStateDimMatrix & running_cost_deriv_xx,
                                    InputInputDimMatrix & running_cost_deriv_uu,
                                    StateInputDimMatrix & running_cost_deriv_xu) const
  {
    running_cost_deriv_x[0] = running_x_[0] * (x[0] - refPos(t));
    running_cost_deriv_x[1] = running_x_[1] * x[1];
    running_cost_deriv_xx.setZero();
    running_cost_deriv_xx(0, 0) = running_x_[0];
    running_cost_deriv_xx(1, 1) = running_x_[1];
    NMPC_UNROLL
    for(int j = 0; j < kInputDimMax; j++)
    {
      if(j < u.size())
      {
        running_cost_deriv_u[j] = running_u_ * u[j];
        running_cost_deriv_xu(0, j) = 0;
        running_cost_deriv_xu(1, j) = 0;
        NMPC_UNROLL
        for(int k = 0; k < kInputDimMax; k++)
        {
          if(k < u.size())
          {
            running_cost_deriv_uu(k, j) = (j == k) ? running_u_ : 0.0;
          }
        }
      }
    }
  }

  NMPC_HD void calcTerminalCostDeriv(double t,
                                     const StateDimVector & x,
                                     StateDimVector & terminal_cost_deriv_x,
                                     StateStateDimMatrix & terminal_cost_deriv_xx) const
  {
    terminal_cost_deriv_x[0] = terminal_x_[0] * (x[0] - refPos(t));
    terminal_cost_deriv_x[1] = terminal_x_[1] * x[1];
    terminal_cost_deriv_xx.setZero();
    terminal_cost_deriv_xx(0, 0) = terminal_x_[0];
    terminal_cost_deriv_xx(1, 1) = terminal_x_[1];
  }

  NMPC_HD void calcIneqConstDeriv(double, // t
                                  const StateDimVector &, // x
                                  const InputDimVector & u,
                                  IneqStateDimMatrix & ineq_const_deriv_x,
                                  IneqInputDimMatrix & ineq_const_deriv_u) const
  {
    NMPC_UNROLL
    for(int r = 0; r < kIneqDimMax; r++)
    {
      if(r < ineq_const_deriv_x.rows())
      {
        ineq_const_deriv_x(r, 0) = 0;
        ineq_const_deriv_x(r, 1) = 0;
        NMPC_UNROLL
        for(int j = 0; j < kInputDimMax; j++)
        {
          if(j < u.size())
          {
            ineq_const_deriv_u(r, j) = (r == 2 * j) ? -1.0 : ((r == 2 * j + 1) ? 1.0 : 0.0);
          }
        }
      }
    }
  }

public:
  double running_x_[2] = {1.0, 1e-3};
  double running_u_ = 1e-3;
  double terminal_x_[2] = {1.0, 1e-3};
  double mass_ = 1.0; // [kg]
  double f_min_ = 0.0; // [N] per contact
  double f_max_ = 30.0; // [N] per contact
  double ref_switch_t_ = 8.0; // [sec] reference height drops from 1 m to 0 m here
  double double_support_begin_ = 2.0, double_support_end_ = 3.0; // [sec] two contacts
  double flight_begin_ = 4.5, flight_end_ = 5.0; // [sec] no contact
};
} // namespace nmpc_amd
