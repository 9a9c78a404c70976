// Host-side C++ mirror of the reference's nmpc_cgmres::CgmresSolver (nmpc_cgmres/include/nmpc_cgmres/CgmresSolver.h:25-132) for a
// BATCH of independent solvers of one problem type on one MI355X.  Same public members (the C/GMRES parameters sim_duration_ ...
// dump_step_, the variables x_, u_, u_list_, delta_u_vec_) and methods (setup, run, calcControlInput), with a leading batch index
// where the reference has one solver.  ODE solvers are named by the enum of <nmpc_hip_cgmres.h> instead of OdeSolver objects.
//
// Plain C++17 (no HIP, no Eigen): everything numeric happens behind the C-ABI of <nmpc_hip_cgmres.h> in libnmpc_hip_ddp.so.  The
// problem TYPE must have been compiled into a gfx950 code object and registered (NMPC_AMD_REGISTER_CGMRES_PROBLEM,
// <nmpc_amd/hip/cgmres_kernels.hpp>); the problem OBJECT is copied to the device at every setup / run / calcControlInput, so
// mutating it in between behaves as with the reference's shared_ptr.
#pragma once

#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include <nmpc_amd/CgmresProblem.hpp>
#include <nmpc_hip_cgmres.h>

namespace nmpc_amd
{
/** \brief Batched C/GMRES solver.
    \tparam Problem problem class derived from nmpc_amd::CgmresProblem with a `static constexpr const char * kName` */
template<class Problem>
class CgmresSolverBatch
{
public:
  static constexpr int dim_x = Problem::dim_x_, dim_uc = Problem::dim_uc_;
  using StateVector = std::vector<double>; //!< dim_x_ entries
  using InputVector = std::vector<double>; //!< dim_uc_ entries

  /** CgmresSolver(problem, ode_solver, sim_ode_solver) (CgmresSolver.h:30-40) for `batch` instances; sim_ode_solver -1 = the same as
      ode_solver.  Every instance starts from Problem::initialState / initialInput. */
  CgmresSolverBatch(std::shared_ptr<Problem> problem, int batch, int horizon_divide_num = 25, int ode_solver = NMPC_HIP_CGMRES_ODE_EULER,
                    int sim_ode_solver = -1, int device = 0)
  : problem_(std::move(problem)), batch_(batch), x_initial_(batch, StateVector(dim_x)), u_initial_(batch, InputVector(dim_uc))
  {
    check(nmpc_hip_cgmres_create(Problem::kName, horizon_divide_num, batch, device, &h_));
    nmpc_hip_cgmres_config c;
    check(nmpc_hip_cgmres_get_config(h_, &c));
    sim_duration_ = c.sim_duration;
    steady_horizon_duration_ = c.steady_horizon_duration;
    horizon_divide_num_ = c.horizon_divide_num;
    horizon_increase_ratio_ = c.horizon_increase_ratio;
    dt_ = c.dt;
    eq_zeta_ = c.eq_zeta;
    k_max_ = c.k_max;
    finite_diff_delta_ = c.finite_diff_delta;
    dump_step_ = c.dump_step;
    ode_solver_ = ode_solver;
    sim_ode_solver_ = sim_ode_solver;
    for(int b = 0; b < batch; b++)
    {
      Problem::initialState(x_initial_[b].data());
      Problem::initialInput(u_initial_[b].data());
    }
  }

  ~CgmresSolverBatch()
  {
    nmpc_hip_cgmres_destroy(h_);
  }

  CgmresSolverBatch(const CgmresSolverBatch &) = delete;
  CgmresSolverBatch & operator=(const CgmresSolverBatch &) = delete;

  /** CgmresSolver::setup (CgmresSolver.cpp:8-64) for every instance, from x_initial_ / u_initial_. */
  void setup()
  {
    push();
    check(nmpc_hip_cgmres_setup(h_));
  }

  /** CgmresSolver::run (CgmresSolver.cpp:66-107) for every instance; the logs stay on the device (nmpc_hip_cgmres_get). */
  void run()
  {
    push();
    check(nmpc_hip_cgmres_run(h_));
  }

  /** CgmresSolver::calcControlInput for every instance: t [B], x / next_x [B][dim_x] (row-major), u out [B][dim_uc]. */
  void calcControlInput(const double * t, const double * x, const double * next_x, double * u)
  {
    pushConfig();
    check(nmpc_hip_cgmres_control_input(h_, t, x, next_x, u));
  }

  /** Same with device arrays, asynchronous on `stream` (a hipStream_t; nullptr = the solver's own stream). */
  void calcControlInputDevice(const double * d_t, const double * d_x, const double * d_next_x, double * d_u, void * stream = nullptr)
  {
    check(nmpc_hip_cgmres_control_input_device(h_, d_t, d_x, d_next_x, d_u, stream));
  }

  /** "lane" (default) or "wave" (one wavefront per instance, the tick in LDS; <nmpc_hip_cgmres.h>): the kernel family of run and
      calcControlInput.  Same bits either way.  Throws std::invalid_argument when the problem type has no wave kernels or the shape
      (horizon_divide_num_, k_max_) exceeds their LDS budget. */
  void setKernel(const char * kernel)
  {
    if(kernel && std::string(kernel) == "wave") // the handle has to know k_max_ to judge the shape; "lane" takes every config
    {
      pushConfig();
    }
    check(nmpc_hip_cgmres_set_kernel(h_, kernel));
    pushConfig();
  }

  /** The kernel symbol run() launches next: "cgmres_run_kernel" or "cgmres_wave_run_kernel". */
  std::string kernelName() const
  {
    const char * name = nullptr;
    check(nmpc_hip_cgmres_kernel_name(h_, &name));
    return name;
  }

  void synchronize()
  {
    check(nmpc_hip_cgmres_synchronize(h_));
  }

  /** x_ / u_ of every instance ([B][dim]), u_list_ / delta_u_vec_ ([B][horizon_divide_num * dim_uc]), per-instance status. */
  std::vector<double> x() const
  {
    return get<double>(NMPC_HIP_CGMRES_FIELD_X);
  }
  std::vector<double> u() const
  {
    return get<double>(NMPC_HIP_CGMRES_FIELD_U);
  }
  std::vector<double> uList() const
  {
    return get<double>(NMPC_HIP_CGMRES_FIELD_U_LIST);
  }
  std::vector<double> deltaUVec() const
  {
    return get<double>(NMPC_HIP_CGMRES_FIELD_DELTA_U);
  }
  std::vector<int> status() const
  {
    return get<int>(NMPC_HIP_CGMRES_FIELD_STATUS);
  }

  nmpc_hip_cgmres_handle handle() const
  {
    return h_;
  }

public:
  std::shared_ptr<Problem> problem_;

  //////// parameters of C/GMRES method (CgmresSolver.h:72-86) ////////
  double sim_duration_;
  double steady_horizon_duration_;
  int horizon_divide_num_; //!< fixed at construction
  double horizon_increase_ratio_;
  double dt_;
  double eq_zeta_;
  int k_max_;
  double finite_diff_delta_;
  int dump_step_;
  int ode_solver_;
  int sim_ode_solver_;

  //! x_initial_ / u_initial_ of every instance (CgmresProblem.h:68-69): setup() and run() start from them
  int batch_;
  std::vector<StateVector> x_initial_;
  std::vector<InputVector> u_initial_;

private:
  static void check(int rc)
  {
    if(rc == NMPC_HIP_OK)
    {
      return;
    }
    const std::string msg = nmpc_hip_cgmres_last_error();
    if(rc == NMPC_HIP_ERR_INVALID_ARGUMENT || rc == NMPC_HIP_ERR_UNKNOWN_MODEL)
    {
      throw std::invalid_argument(msg);
    }
    throw std::runtime_error("[nmpc_hip_cgmres " + std::to_string(rc) + "] " + msg);
  }

  void pushConfig()
  {
    nmpc_hip_cgmres_config c;
    check(nmpc_hip_cgmres_get_config(h_, &c));
    c.sim_duration = sim_duration_;
    c.steady_horizon_duration = steady_horizon_duration_;
    c.horizon_divide_num = horizon_divide_num_;
    c.horizon_increase_ratio = horizon_increase_ratio_;
    c.dt = dt_;
    c.eq_zeta = eq_zeta_;
    c.k_max = k_max_;
    c.finite_diff_delta = finite_diff_delta_;
    c.dump_step = dump_step_;
    c.ode_solver = ode_solver_;
    c.sim_ode_solver = sim_ode_solver_;
    check(nmpc_hip_cgmres_set_config(h_, &c));
  }

  void push()
  {
    pushConfig();
    check(nmpc_hip_cgmres_set_problem(h_, problem_.get(), sizeof(Problem), 0));
    std::vector<double> x(static_cast<size_t>(batch_) * dim_x), u(static_cast<size_t>(batch_) * dim_uc);
    for(int b = 0; b < batch_; b++)
    {
      for(int a = 0; a < dim_x; a++)
      {
        x[static_cast<size_t>(b) * dim_x + a] = x_initial_.at(b).at(a);
      }
      for(int j = 0; j < dim_uc; j++)
      {
        u[static_cast<size_t>(b) * dim_uc + j] = u_initial_.at(b).at(j);
      }
    }
    check(nmpc_hip_cgmres_set_initial(h_, x.data(), u.data()));
  }

  template<class T>
  std::vector<T> get(int field) const
  {
    size_t bytes = 0;
    check(nmpc_hip_cgmres_field_bytes(h_, field, &bytes));
    std::vector<T> out(bytes / sizeof(T));
    check(nmpc_hip_cgmres_get(h_, field, out.data(), bytes));
    return out;
  }

  nmpc_hip_cgmres_handle h_ = nullptr;
};
} // namespace nmpc_amd
