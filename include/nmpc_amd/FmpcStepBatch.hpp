// Host-side C++ mirror of the batched FMPC iteration on caller-supplied linearisations: one FmpcSolver::procOnce of the reference
// (nmpc_fmpc/include/nmpc_fmpc/FmpcSolver.hpp:365-493, enable_line_search = false) per step() for a BATCH of instances whose
// Jacobians, cost derivatives and function values the caller supplies, on one MI355X.  The solver owns the variable: linearise at
// variable(), call step(), repeat until every status is Succeeded.
//
// Plain C++17 (no HIP runtime, no Eigen): everything numeric happens behind the C-ABI of <nmpc_hip_fmpc_step.h> in
// libnmpc_hip_ddp.so.  Matrix blocks are column-major (Eigen's order) unless config().row_major is set.
#pragma once

#include <stdexcept>
#include <string>
#include <vector>

#include <nmpc_hip_fmpc_step.h>

namespace nmpc_amd
{
/** \brief Batched interior-point iteration of FMPC on caller-supplied linearisations. */
class FmpcStepBatch
{
public:
  static constexpr int MaxDim = 16; // NMPC_HIP_FMPC_STEP_MAX_DIM
  static constexpr int MaxIneq = 32; // NMPC_HIP_FMPC_STEP_MAX_INEQ
  static_assert(MaxDim == NMPC_HIP_FMPC_STEP_MAX_DIM && MaxIneq == NMPC_HIP_FMPC_STEP_MAX_INEQ, "mirror and header disagree");

  /** The linearisation of every step and instance at the current variable, in the layouts of nmpc_hip_fmpc_step.h: A, Lxx
      [B][T][n*n]; B, Lxu [B][T][n*m]; C [B][T][g*n]; D [B][T][g*m]; Luu [B][T][m*m]; Lx, f [B][T][n]; Lu [B][T][m]; g [B][T][g];
      Lx_T [B][n]; Lxx_T [B][n*n]; current_x [B][n]. */
  struct Linearisation
  {
    std::vector<double> A, B, C, D, Lx, Lu, Lxx, Luu, Lxu, f, g, Lx_T, Lxx_T, current_x;
  };

  /** FmpcSolver::Variable (FmpcSolver.h:117-158): x, lambda [B][T+1][n]; u [B][T][m]; s, nu [B][T][g]. */
  struct Variable
  {
    std::vector<double> x, u, lambda, s, nu;
  };

  /** What an iteration leaves per instance (status: FmpcSolver::Status, 6 = IterationContinued), the gains k [B][T][m],
      K [B][T][m*n], s [B][T+1][n], P [B][T+1][n*n], and the delta. */
  struct Result
  {
    std::vector<int> status;
    std::vector<double> kkt_error, barrier_eps, alpha_s_max, alpha_nu_max;
    std::vector<double> k, K, s, P;
    Variable delta;
  };

  FmpcStepBatch(int state_dim, int input_dim, int ineq_dim, int horizon_steps, int batch, int device = 0)
  : n_(state_dim), m_(input_dim), g_(ineq_dim), T_(horizon_steps), batch_(batch)
  {
    check(nmpc_hip_fmpc_step_create(state_dim, input_dim, ineq_dim, horizon_steps, batch, device, &h_));
    check(nmpc_hip_fmpc_step_get_config(h_, &config_));
  }

  ~FmpcStepBatch()
  {
    nmpc_hip_fmpc_step_destroy(h_);
  }

  FmpcStepBatch(const FmpcStepBatch &) = delete;
  FmpcStepBatch & operator=(const FmpcStepBatch &) = delete;

  /** The configuration; pushed to the library by the next step(). */
  nmpc_hip_fmpc_step_config & config()
  {
    return config_;
  }

  /** inputDim(t) and ineqDim(t) of every step, shared by the batch; an empty vector = the capacity everywhere. */
  void setStepDims(const std::vector<int> & input_dims, const std::vector<int> & ineq_dims)
  {
    const size_t T = T_;
    if((!input_dims.empty() && input_dims.size() != T) || (!ineq_dims.empty() && ineq_dims.size() != T))
    {
      throw std::invalid_argument("[FmpcStep] the dimensions must hold horizon_steps entries");
    }
    check(nmpc_hip_fmpc_step_set_step_dims(h_, input_dims.empty() ? nullptr : input_dims.data(),
                                           ineq_dims.empty() ? nullptr : ineq_dims.data()));
  }

  /** variable_ of every instance; barrier_eps [B], or empty to keep the solver's (1e-4 after construction). */
  void setVariable(const Variable & v, const std::vector<double> & barrier_eps = {})
  {
    const size_t B = batch_, T = T_, n = n_, m = m_, g = g_;
    if(v.x.size() != B * (T + 1) * n || v.lambda.size() != B * (T + 1) * n || v.u.size() != B * T * m || v.s.size() != B * T * g
       || v.nu.size() != B * T * g || (!barrier_eps.empty() && barrier_eps.size() != B))
    {
      throw std::invalid_argument("[FmpcStep] a variable array has the wrong size");
    }
    check(nmpc_hip_fmpc_step_set_variable(h_, v.x.data(), ptr(v.u), v.lambda.data(), ptr(v.s), ptr(v.nu), ptr(barrier_eps), 0));
  }

  /** One procOnce of every instance on the linearisation at the solver's variable. */
  Result step(const Linearisation & l)
  {
    const size_t B = batch_, S = B * T_, n = n_, m = m_, g = g_;
    if(l.A.size() != S * n * n || l.B.size() != S * n * m || l.C.size() != S * g * n || l.D.size() != S * g * m || l.Lx.size() != S * n
       || l.Lu.size() != S * m || l.Lxx.size() != S * n * n || l.Luu.size() != S * m * m || l.Lxu.size() != S * n * m || l.f.size() != S * n
       || l.g.size() != S * g || l.Lx_T.size() != B * n || l.Lxx_T.size() != B * n * n || l.current_x.size() != B * n)
    {
      throw std::invalid_argument("[FmpcStep] a linearisation array has the wrong size");
    }
    check(nmpc_hip_fmpc_step_set_config(h_, &config_));
    check(nmpc_hip_fmpc_step_set_linearisation(h_, l.A.data(), ptr(l.B), ptr(l.C), ptr(l.D), l.Lx.data(), ptr(l.Lu), l.Lxx.data(), ptr(l.Luu),
                                               ptr(l.Lxu), l.f.data(), ptr(l.g), l.Lx_T.data(), l.Lxx_T.data(), l.current_x.data(), 0));
    check(nmpc_hip_fmpc_step_step(h_));
    return result();
  }

  /** Device arrays (layouts of nmpc_hip_fmpc_step.h), read in place; asynchronous on `stream` (a hipStream_t; nullptr = the
      solver's own).  The arrays are read in the order of `stream`: pass the stream that writes them, or have that work completed
      before the call when the solver's own stream (non-blocking: it waits for no other stream) is used.  Read the fields with
      result() after synchronize(). */
  void stepDevice(const double * d_A,
                  const double * d_B,
                  const double * d_C,
                  const double * d_D,
                  const double * d_Lx,
                  const double * d_Lu,
                  const double * d_Lxx,
                  const double * d_Luu,
                  const double * d_Lxu,
                  const double * d_f,
                  const double * d_g,
                  const double * d_Lx_T,
                  const double * d_Lxx_T,
                  const double * d_current_x,
                  void * stream = nullptr)
  {
    check(nmpc_hip_fmpc_step_set_config(h_, &config_));
    check(nmpc_hip_fmpc_step_set_linearisation(h_, d_A, d_B, d_C, d_D, d_Lx, d_Lu, d_Lxx, d_Luu, d_Lxu, d_f, d_g, d_Lx_T, d_Lxx_T,
                                               d_current_x, 1));
    check(nmpc_hip_fmpc_step_step_device(h_, stream));
  }
  void synchronize()
  {
    check(nmpc_hip_fmpc_step_synchronize(h_));
  }

  Result result() const
  {
    Result r;
    r.status = get<int>(NMPC_HIP_FMPC_STEP_FIELD_STATUS);
    r.kkt_error = get<double>(NMPC_HIP_FMPC_STEP_FIELD_KKT_ERROR);
    r.barrier_eps = get<double>(NMPC_HIP_FMPC_STEP_FIELD_BARRIER_EPS);
    r.alpha_s_max = get<double>(NMPC_HIP_FMPC_STEP_FIELD_ALPHA_S_MAX);
    r.alpha_nu_max = get<double>(NMPC_HIP_FMPC_STEP_FIELD_ALPHA_NU_MAX);
    r.k = get<double>(NMPC_HIP_FMPC_STEP_FIELD_K_FF);
    r.K = get<double>(NMPC_HIP_FMPC_STEP_FIELD_K_FB);
    r.s = get<double>(NMPC_HIP_FMPC_STEP_FIELD_S);
    r.P = get<double>(NMPC_HIP_FMPC_STEP_FIELD_P);
    r.delta.x = get<double>(NMPC_HIP_FMPC_STEP_FIELD_DELTA_X);
    r.delta.u = get<double>(NMPC_HIP_FMPC_STEP_FIELD_DELTA_U);
    r.delta.lambda = get<double>(NMPC_HIP_FMPC_STEP_FIELD_DELTA_LAMBDA);
    r.delta.s = get<double>(NMPC_HIP_FMPC_STEP_FIELD_DELTA_S);
    r.delta.nu = get<double>(NMPC_HIP_FMPC_STEP_FIELD_DELTA_NU);
    return r;
  }

  /** The variable the solver holds. */
  Variable variable() const
  {
    Variable v;
    v.x = get<double>(NMPC_HIP_FMPC_STEP_FIELD_VAR_X);
    v.u = get<double>(NMPC_HIP_FMPC_STEP_FIELD_VAR_U);
    v.lambda = get<double>(NMPC_HIP_FMPC_STEP_FIELD_VAR_LAMBDA);
    v.s = get<double>(NMPC_HIP_FMPC_STEP_FIELD_VAR_S);
    v.nu = get<double>(NMPC_HIP_FMPC_STEP_FIELD_VAR_NU);
    return v;
  }

  std::string kernelName() const
  {
    const char * name = nullptr;
    check(nmpc_hip_fmpc_step_kernel_name(h_, &name));
    return name;
  }
  float lastMs() const
  {
    float ms = 0;
    check(nmpc_hip_fmpc_step_last_ms(h_, &ms));
    return ms;
  }
  int batch() const
  {
    return batch_;
  }

protected:
  static void check(int rc)
  {
    if(rc == NMPC_HIP_OK)
    {
      return;
    }
    const std::string msg = nmpc_hip_fmpc_step_last_error();
    if(rc == NMPC_HIP_ERR_INVALID_ARGUMENT)
    {
      throw std::invalid_argument(msg);
    }
    throw std::runtime_error(msg);
  }

  static const double * ptr(const std::vector<double> & v)
  {
    return v.empty() ? nullptr : v.data();
  }

  template<class T>
  std::vector<T> get(int field) const
  {
    size_t bytes = 0;
    check(nmpc_hip_fmpc_step_field_bytes(h_, field, &bytes));
    std::vector<T> out(bytes / sizeof(T));
    check(nmpc_hip_fmpc_step_get(h_, field, out.data(), bytes, 0));
    return out;
  }

  int n_ = 0, m_ = 0, g_ = 0, T_ = 0, batch_ = 0;
  nmpc_hip_fmpc_step_config config_;
  nmpc_hip_fmpc_step_handle h_ = nullptr;
};
} // namespace nmpc_amd
