// Host-side C++ mirror of the batched Riccati backward pass: the reference's DDPSolver::backwardPass (nmpc_ddp/include/nmpc_ddp/
// DDPSolver.hpp:342-534) with its lambda retry loop (:188-214) and BoxQP feed-forward (:450-497) for a BATCH of instances whose
// Derivative blocks the caller supplies, on one MI355X.
//
// Plain C++17 (no HIP runtime, no Eigen): everything numeric happens behind the C-ABI of <nmpc_hip_riccati.h> in libnmpc_hip_ddp.so.
// Matrix blocks are column-major (Eigen's order) unless config().row_major is set.
#pragma once

#include <stdexcept>
#include <string>
#include <vector>

#include <nmpc_hip_riccati.h>

namespace nmpc_amd
{
/** \brief Batched backward pass of DDP / iLQR on caller-supplied derivatives. */
class RiccatiBatch
{
public:
  static constexpr int MaxDim = 16; // NMPC_HIP_RICCATI_MAX_DIM
  static_assert(MaxDim == NMPC_HIP_RICCATI_MAX_DIM, "mirror and header disagree");

  /** The Derivative blocks of every step and instance (DDPSolver.hpp:371-380) and the terminal pair (:346-347), in the layouts of
      nmpc_hip_riccati.h: Fx, Lxx [B][T][n*n]; Fu, Lxu [B][T][n*m]; Luu [B][T][m*m]; Lx [B][T][n]; Lu [B][T][m]; Vx_T [B][n];
      Vxx_T [B][n*n]. */
  struct Derivatives
  {
    std::vector<double> Fx, Fu, Lx, Lu, Lxx, Luu, Lxu, Vx_T, Vxx_T;
  };

  /** What a pass leaves: k [B][T][m], K [B][T][m*n], dV [B][2], Vx0 [B][n], Vxx0 [B][n*n], and per instance the status
      (nmpc_hip_riccati_status), the passes started, lambda_ and dlambda_ after the retries and the step the last failed pass
      stopped at; per step BoxQP::retval_ and the free mask. */
  struct Result
  {
    std::vector<double> k, K, dV, Vx0, Vxx0, lambda, dlambda;
    std::vector<int> status, n_backward, fail_step, qp_retval;
    std::vector<unsigned> free_mask;
  };

  RiccatiBatch(int state_dim, int input_dim, int horizon_steps, int batch, int device = 0)
  : n_(state_dim), m_(input_dim), T_(horizon_steps), batch_(batch)
  {
    check(nmpc_hip_riccati_create(state_dim, input_dim, horizon_steps, batch, device, &h_));
    check(nmpc_hip_riccati_get_config(h_, &config_));
  }

  ~RiccatiBatch()
  {
    nmpc_hip_riccati_destroy(h_);
  }

  RiccatiBatch(const RiccatiBatch &) = delete;
  RiccatiBatch & operator=(const RiccatiBatch &) = delete;

  /** The configuration; pushed to the library by the next backward(). */
  nmpc_hip_riccati_config & config()
  {
    return config_;
  }

  /** Fu.cols() of every step (:381), shared by the batch; an empty vector = input_dim everywhere. */
  void setInputDims(const std::vector<int> & dims)
  {
    if(!dims.empty() && dims.size() != static_cast<size_t>(T_))
    {
      throw std::invalid_argument("[Riccati] dims must hold horizon_steps entries");
    }
    check(nmpc_hip_riccati_set_input_dims(h_, dims.empty() ? nullptr : dims.data()));
  }

  /** lambda_ and dlambda_ per instance; empty vectors = the config's scalars. */
  void setLambda(const std::vector<double> & lambda, const std::vector<double> & dlambda)
  {
    const size_t B = batch_;
    if((!lambda.empty() && lambda.size() != B) || (!dlambda.empty() && dlambda.size() != B))
    {
      throw std::invalid_argument("[Riccati] lambda and dlambda must hold batch entries");
    }
    check(nmpc_hip_riccati_set_lambda(h_, lambda.empty() ? nullptr : lambda.data(), dlambda.empty() ? nullptr : dlambda.data(), 0));
  }

  /** u_list and the input limits for with_input_constraint (:470-472): U [B][T][m]; lower, upper [m], or [B][T][m] with
      limits_per_step. */
  void setInputs(const std::vector<double> & U, const std::vector<double> & lower, const std::vector<double> & upper, bool limits_per_step = false)
  {
    const size_t S = static_cast<size_t>(batch_) * T_ * m_, lim = limits_per_step ? S : static_cast<size_t>(m_);
    if(U.size() != S || lower.size() != lim || upper.size() != lim)
    {
      throw std::invalid_argument("[Riccati] U must hold batch * T * m entries, lower and upper m (or batch * T * m)");
    }
    check(nmpc_hip_riccati_set_inputs(h_, U.data(), lower.data(), upper.data(), limits_per_step ? 1 : 0, 0));
  }

  /** The retry loop around backwardPass (:188-214) for every instance. */
  Result backward(const Derivatives & d)
  {
    const size_t B = batch_, S = B * T_, n = n_, m = m_;
    if(d.Fx.size() != S * n * n || d.Fu.size() != S * n * m || d.Lx.size() != S * n || d.Lu.size() != S * m || d.Lxx.size() != S * n * n
       || d.Luu.size() != S * m * m || d.Lxu.size() != S * n * m || d.Vx_T.size() != B * n || d.Vxx_T.size() != B * n * n)
    {
      throw std::invalid_argument("[Riccati] a derivative array has the wrong size");
    }
    check(nmpc_hip_riccati_set_config(h_, &config_));
    check(nmpc_hip_riccati_set_derivatives(h_, d.Fx.data(), d.Fu.data(), d.Lx.data(), d.Lu.data(), d.Lxx.data(), d.Luu.data(), d.Lxu.data(),
                                           d.Vx_T.data(), d.Vxx_T.data(), 0));
    check(nmpc_hip_riccati_solve(h_));
    return result();
  }

  /** Device arrays (layouts of nmpc_hip_riccati.h), read in place; asynchronous on `stream` (a hipStream_t; nullptr = the solver's
      own).  Read the fields with result() after synchronize(). */
  void backwardDevice(const double * d_Fx,
                      const double * d_Fu,
                      const double * d_Lx,
                      const double * d_Lu,
                      const double * d_Lxx,
                      const double * d_Luu,
                      const double * d_Lxu,
                      const double * d_Vx_T,
                      const double * d_Vxx_T,
                      void * stream = nullptr)
  {
    check(nmpc_hip_riccati_set_config(h_, &config_));
    check(nmpc_hip_riccati_set_derivatives(h_, d_Fx, d_Fu, d_Lx, d_Lu, d_Lxx, d_Luu, d_Lxu, d_Vx_T, d_Vxx_T, 1));
    check(nmpc_hip_riccati_solve_device(h_, stream));
  }
  void synchronize()
  {
    check(nmpc_hip_riccati_synchronize(h_));
  }

  Result result() const
  {
    Result r;
    r.k = get<double>(NMPC_HIP_RICCATI_FIELD_K_FF);
    r.K = get<double>(NMPC_HIP_RICCATI_FIELD_K_FB);
    r.dV = get<double>(NMPC_HIP_RICCATI_FIELD_DV);
    r.Vx0 = get<double>(NMPC_HIP_RICCATI_FIELD_VX0);
    r.Vxx0 = get<double>(NMPC_HIP_RICCATI_FIELD_VXX0);
    r.lambda = get<double>(NMPC_HIP_RICCATI_FIELD_LAMBDA);
    r.dlambda = get<double>(NMPC_HIP_RICCATI_FIELD_DLAMBDA);
    r.status = get<int>(NMPC_HIP_RICCATI_FIELD_STATUS);
    r.n_backward = get<int>(NMPC_HIP_RICCATI_FIELD_N_BACKWARD);
    r.fail_step = get<int>(NMPC_HIP_RICCATI_FIELD_FAIL_STEP);
    r.qp_retval = get<int>(NMPC_HIP_RICCATI_FIELD_QP_RETVAL);
    r.free_mask = get<unsigned>(NMPC_HIP_RICCATI_FIELD_FREE_MASK);
    return r;
  }

  std::string kernelName() const
  {
    const char * name = nullptr;
    check(nmpc_hip_riccati_kernel_name(h_, &name));
    return name;
  }
  float lastMs() const
  {
    float ms = 0;
    check(nmpc_hip_riccati_last_ms(h_, &ms));
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
    const std::string msg = nmpc_hip_riccati_last_error();
    if(rc == NMPC_HIP_ERR_INVALID_ARGUMENT)
    {
      throw std::invalid_argument(msg);
    }
    throw std::runtime_error(msg);
  }

  template<class T>
  std::vector<T> get(int field) const
  {
    size_t bytes = 0;
    check(nmpc_hip_riccati_field_bytes(h_, field, &bytes));
    std::vector<T> out(bytes / sizeof(T));
    check(nmpc_hip_riccati_get(h_, field, out.data(), bytes, 0));
    return out;
  }

  int n_ = 0, m_ = 0, T_ = 0, batch_ = 0;
  nmpc_hip_riccati_config config_;
  nmpc_hip_riccati_handle h_ = nullptr;
};
} // namespace nmpc_amd
