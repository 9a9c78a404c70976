// Test-only DDP problem whose backward pass hands the BoxQP of every timestep a chosen H, g and C (tests/test_gpu_boxqp_known_answers.py).
//
//   stateEq(t, x, u) = x                       (Fx = I, Fu = 0: the input does not move the state)
//   runningCost      = 1/2 u'Hu + g'u + u'Cx   (Luu = H, Lu = Hu + g + Cx, Lxu = C', Lx = C'u, Lxx = 0)
//   terminalCost     = 1/2 x'x
//
// With x0 = 0 and u_init = 0 the state stays 0, and since Fu = 0 the Q terms of the reference's backward pass (DDPSolver.hpp:421-441)
// are Qu = g, Quu_F = H and Qux = C at every timestep, exactly, with no lambda under reg_type 2 (which adds lambda to Vxx, where Fu = 0
// multiplies it away).  Every timestep therefore solves the same box QP: the last from a zero start, the earlier ones warm-started from
// k of the next timestep (DDPSolver.hpp:452-467).  For a Dynamic input dimension the timestep's m takes the leading m x m block of H,
// the first m entries of g and the first m rows of C; inputDim(t) reads a per-timestep table of the problem object.
//
// Not part of the library: the probe library (nmpc_amd/build.py: build_test_models) and the host checker include it.
#pragma once

#include <nmpc_amd/DDPProblem.hpp>

namespace nmpc_amd
{
namespace test
{
template<class Real, int N, int M, int MaxM = M>
class BoxQPProbe : public DDPProblemT<Real, N, M, MaxM>
{
  using Base = DDPProblemT<Real, N, M, MaxM>;

public:
  using typename Base::InputDimVector;
  using typename Base::InputInputDimMatrix;
  using typename Base::StateDimVector;
  using typename Base::StateInputDimMatrix;
  using typename Base::StateStateDimMatrix;
  static constexpr int MM = Base::kInputDimMax;
  //! length of the inputDim table: timestep i of a solve from t0 = 0 reads m_steps_[min(i, kSteps - 1)]
  static constexpr int kSteps = 16;

  NMPC_HD explicit BoxQPProbe(Real dt = Real(0.1)) : Base(dt)
  {
    for(int a = 0; a < MM; a++)
    {
      for(int b = 0; b < MM; b++)
      {
        H_[a + b * MM] = a == b ? Real(1) : Real(0);
      }
      g_[a] = 0;
      for(int c = 0; c < N; c++)
      {
        C_[a + c * MM] = 0;
      }
    }
    for(int i = 0; i < kSteps; i++)
    {
      m_steps_[i] = MM;
    }
  }

  NMPC_HD int inputDim(Real t) const
  {
    int i = static_cast<int>(t / this->dt_ + Real(0.5));
    i = i < 0 ? 0 : (i >= kSteps ? kSteps - 1 : i);
    return m_steps_[i];
  }

  NMPC_HD StateDimVector stateEq(Real, const StateDimVector & x, const InputDimVector &) const
  {
    return x;
  }

  NMPC_HD Real runningCost(Real, const StateDimVector & x, const InputDimVector & u) const
  {
    Real c = 0;
    for(int a = 0; a < u.size(); a++)
    {
      Real hu = 0, cx = 0;
      for(int b = 0; b < u.size(); b++)
      {
        hu += H_[a + b * MM] * u[b];
      }
      for(int j = 0; j < N; j++)
      {
        cx += C_[a + j * MM] * x[j];
      }
      c += u[a] * (Real(0.5) * hu + g_[a] + cx);
    }
    return c;
  }

  NMPC_HD Real terminalCost(Real, const StateDimVector & x) const
  {
    Real c = 0;
    for(int j = 0; j < N; j++)
    {
      c += x[j] * x[j];
    }
    return Real(0.5) * c;
  }

  NMPC_HD void calcStateEqDeriv(Real,
                                const StateDimVector &,
                                const InputDimVector &,
                                StateStateDimMatrix & state_eq_deriv_x,
                                StateInputDimMatrix & state_eq_deriv_u) const
  {
    state_eq_deriv_x.setIdentity();
    state_eq_deriv_u.setZero();
  }

  NMPC_HD void calcRunningCostDeriv(Real,
                                    const StateDimVector & x,
                                    const InputDimVector & u,
                                    StateDimVector & running_cost_deriv_x,
                                    InputDimVector & running_cost_deriv_u,
                                    StateStateDimMatrix & running_cost_deriv_xx,
                                    InputInputDimMatrix & running_cost_deriv_uu,
                                    StateInputDimMatrix & running_cost_deriv_xu) const
  {
    const int m = u.size();
    running_cost_deriv_xx.setZero();
    for(int j = 0; j < N; j++)
    {
      Real s = 0;
      for(int a = 0; a < m; a++)
      {
        s += C_[a + j * MM] * u[a];
        running_cost_deriv_xu(j, a) = C_[a + j * MM];
      }
      running_cost_deriv_x[j] = s;
    }
    for(int a = 0; a < m; a++)
    {
      Real s = g_[a];
      for(int b = 0; b < m; b++)
      {
        s += H_[a + b * MM] * u[b];
        running_cost_deriv_uu(a, b) = H_[a + b * MM];
      }
      for(int j = 0; j < N; j++)
      {
        s += C_[a + j * MM] * x[j];
      }
      running_cost_deriv_u[a] = s;
    }
  }

  NMPC_HD void calcTerminalCostDeriv(Real,
                                     const StateDimVector & x,
                                     StateDimVector & terminal_cost_deriv_x,
                                     StateStateDimMatrix & terminal_cost_deriv_xx) const
  {
    terminal_cost_deriv_x = x;
    terminal_cost_deriv_xx.setIdentity();
  }

  // the problem object's memory image (tests/test_gpu_boxqp_known_answers.py mirrors it): dt_ (Base), then
  Real H_[MM * MM]; //!< column-major, leading dimension MM
  Real g_[MM];
  Real C_[MM * N]; //!< m x n, column-major, leading dimension MM
  int m_steps_[kSteps]; //!< inputDim of timestep i (read for a Dynamic input dimension only)
};
} // namespace test
} // namespace nmpc_amd
