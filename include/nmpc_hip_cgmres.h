/* C-ABI of the MI355X-native batched C/GMRES solver (part of libnmpc_hip_ddp.so).
 *
 * Boundary for the reference's nmpc_cgmres::CgmresSolver (nmpc_cgmres/include/nmpc_cgmres/CgmresSolver.h:25-132,
 * src/CgmresSolver.cpp:8-202): B independent solvers of one problem type, each with its own state, input list and GMRES warm
 * start, one lane of a gfx950 wavefront each.  The reference has no FFI layer; each entry point cites the member it replaces.
 * Plain pointers and sizes only.  Every function returns 0 (NMPC_HIP_OK) or a negative nmpc_hip_status (nmpc_hip_ddp.h);
 * nothing throws across this boundary.  There is no CPU fallback: without a gfx950 device create() reports
 * NMPC_HIP_ERR_NO_DEVICE.
 *
 * Layouts at this boundary (row-major in the order written, doubles unless noted; NX / NUC = dim_x_ / dim_uc_ of the problem
 * type, N = horizon_divide_num, B = batch, L = logged ticks of the last run):
 *   X          [B][NX]          x_                                  (CgmresSolver.h:90)
 *   U          [B][NUC]         u_                                  (CgmresSolver.h:91)
 *   U_LIST     [B][N][NUC]      u_list_, column i as row i          (CgmresSolver.h:99)
 *   DELTA_U    [B][N][NUC]      delta_u_vec_                        (CgmresSolver.h:110)
 *   STATUS     [B] int          nmpc_hip_cgmres_instance_status
 *   ERR        [B]              |DhDu_vec_| of the last tick (after setup: |DhDu| at the end of its Newton loop)
 *   LOG_T      [L]              time column of cgmres_{x,u,err}.dat (CgmresSolver.cpp:92-98)
 *   LOG_X      [B][L][NX]       x_ after the tick
 *   LOG_U      [B][L][NUC]      u_ after the tick
 *   LOG_ERR    [B][L]           |DhDu_vec_| at (t, x) of the tick
 *   LOG_ITERS  [B][L] int       GMRES iterations of the tick
 *   LOG_REORTH [B][L] int       1 if the GMRES re-orthogonalisation fired in the tick
 * On the device the same data is kept [element][instance]; the conversion happens inside set / get.
 */
#ifndef NMPC_HIP_CGMRES_H
#define NMPC_HIP_CGMRES_H

#include <stddef.h>

#include "nmpc_hip_ddp.h" /* nmpc_hip_status */

#ifdef __cplusplus
extern "C"
{
#endif

  /** OdeSolver subclasses (OdeSolver.h:32-80). */
  typedef enum
  {
    NMPC_HIP_CGMRES_ODE_EULER = 0,
    NMPC_HIP_CGMRES_ODE_RUNGE_KUTTA = 1
  } nmpc_hip_cgmres_ode_solver;

  /** Per-instance status (the reference prints "failed to converge u in setup." and goes on, CgmresSolver.cpp:42-45). */
  typedef enum
  {
    NMPC_HIP_CGMRES_UNINITIALIZED = 0,
    NMPC_HIP_CGMRES_SUCCEEDED = 1, /* setup converged to |DhDu| <= 1e-6 */
    NMPC_HIP_CGMRES_SETUP_NOT_CONVERGED = 2, /* setup ended above 1e-6; the ticks still run, as in the reference */
    NMPC_HIP_CGMRES_NON_FINITE = 3 /* a state or input became NaN / Inf: the instance stopped updating */
  } nmpc_hip_cgmres_instance_status;

  /** The parameters of C/GMRES method (CgmresSolver.h:72-86) and the two ODE solvers of the constructor (CgmresSolver.h:30-40). */
  typedef struct
  {
    double sim_duration; /* :73 */
    double steady_horizon_duration; /* :75 */
    int horizon_divide_num; /* :76 (fixed at create(); set_config rejects a different value) */
    double horizon_increase_ratio; /* :77 */
    double dt; /* :79 */
    double eq_zeta; /* :81 */
    int k_max; /* :82; 1 .. 16 */
    double finite_diff_delta; /* :84 */
    int dump_step; /* :86; 0 = no logs (throughput runs) */
    int ode_solver; /* nmpc_hip_cgmres_ode_solver inside the horizon (ode_solver_) */
    int sim_ode_solver; /* of the simulation in run() (sim_ode_solver_); -1 = the same as ode_solver, as the constructor does */
    int ticks_per_launch; /* run(): ticks per kernel launch; 0 = automatic (a few tenths of a second of work per launch) */
  } nmpc_hip_cgmres_config;

  typedef enum
  {
    NMPC_HIP_CGMRES_FIELD_X = 0,
    NMPC_HIP_CGMRES_FIELD_U = 1,
    NMPC_HIP_CGMRES_FIELD_U_LIST = 2,
    NMPC_HIP_CGMRES_FIELD_DELTA_U = 3,
    NMPC_HIP_CGMRES_FIELD_STATUS = 4, /* int */
    NMPC_HIP_CGMRES_FIELD_ERR = 5,
    NMPC_HIP_CGMRES_FIELD_LOG_T = 6,
    NMPC_HIP_CGMRES_FIELD_LOG_X = 7,
    NMPC_HIP_CGMRES_FIELD_LOG_U = 8,
    NMPC_HIP_CGMRES_FIELD_LOG_ERR = 9,
    NMPC_HIP_CGMRES_FIELD_LOG_ITERS = 10, /* int */
    NMPC_HIP_CGMRES_FIELD_LOG_REORTH = 11 /* int */
  } nmpc_hip_cgmres_field;

  typedef struct nmpc_hip_cgmres_solver * nmpc_hip_cgmres_handle;

  /** Fill cfg with the reference defaults (CgmresSolver.h:72-86): sim_duration 10, steady_horizon_duration 1, horizon_divide_num
      25, horizon_increase_ratio 0.5, dt 1e-3, eq_zeta 1000, k_max 5, finite_diff_delta 0.002, dump_step 5; Euler inside the horizon
      and the same solver for the simulation. */
  int nmpc_hip_cgmres_default_config(nmpc_hip_cgmres_config * cfg);

  /** Registered C/GMRES problem types (NMPC_AMD_REGISTER_CGMRES_PROBLEM). */
  int nmpc_hip_cgmres_model_count(void);
  int nmpc_hip_cgmres_model_name(int index, const char ** name);
  /** dim_x_, dim_u_, dim_c_ (dim_uc_ = dim_u_ + dim_c_), the size of the problem object, and x_initial_ [NX] / u_initial_ [NUC]
      (each may be NULL). */
  int nmpc_hip_cgmres_model_info(const char * model,
                                 int * dim_x,
                                 int * dim_u,
                                 int * dim_c,
                                 size_t * param_bytes,
                                 double * x_initial,
                                 double * u_initial);
  /** Copy the default-constructed problem object (a trivially-copyable blob of param_bytes) to out. */
  int nmpc_hip_cgmres_model_default_params(const char * model, void * out, size_t bytes);

  /** CgmresSolver(problem, ode_solver, sim_ode_solver) (CgmresSolver.h:30-40) for `batch` instances with horizon_divide_num on
      HIP device `device`.  Every instance starts from the problem type's x_initial_ / u_initial_ and the default problem object. */
  int nmpc_hip_cgmres_create(const char * model, int horizon_divide_num, int batch, int device, nmpc_hip_cgmres_handle * out);
  int nmpc_hip_cgmres_destroy(nmpc_hip_cgmres_handle h);

  /** Kernel family of run / control_input / control_input_device: "lane" (the default: one lane per instance, every list in HBM; a
      throughput kernel for very large batches) or "wave" (one wavefront per instance, the whole tick in LDS; the low-latency kernel
      for 1 .. a few thousand instances that have to tick inside dt).  Both read and write the same handle state and give the same
      bits, so the kernel may be changed between calls.  "wave" is refused with NMPC_HIP_ERR_INVALID_ARGUMENT (the message names the
      bytes) when the problem type has no wave registration (NMPC_AMD_REGISTER_CGMRES_WAVE_PROBLEM,
      <nmpc_amd/hip/cgmres_wave_kernels.hpp>) or the shape needs more than 64 KiB of LDS; while "wave" is set, a set_config that raises
      k_max past that budget is refused the same way and leaves the config as it was.  A NULL or unknown name is an invalid argument. */
  int nmpc_hip_cgmres_set_kernel(nmpc_hip_cgmres_handle h, const char * kernel);
  /** The kernel symbol run launches next, without template arguments: "cgmres_run_kernel" or "cgmres_wave_run_kernel". */
  int nmpc_hip_cgmres_kernel_name(nmpc_hip_cgmres_handle h, const char ** name);
  /** LDS bytes of one workgroup of the wave kernels for a registered problem type: with n = N * dim_uc, K = k_max,
      8 * (4 n + 3 ((2 N + 1) dim_x + N) + (K + 3) n + K * K + 3 K + 1)  (layout: <nmpc_amd/hip/cgmres_wave_kernels.hpp>).  Needs no
      device. */
  int nmpc_hip_cgmres_wave_lds_bytes(const char * model, int horizon_divide_num, int k_max, size_t * bytes);

  int nmpc_hip_cgmres_set_config(nmpc_hip_cgmres_handle h, const nmpc_hip_cgmres_config * cfg);
  int nmpc_hip_cgmres_get_config(nmpc_hip_cgmres_handle h, nmpc_hip_cgmres_config * cfg);

  /** The problem object(s) (CgmresSolver.h:65): one blob of param_bytes shared by every instance (per_instance = 0) or `batch`
      blobs back to back (per_instance = 1). */
  int nmpc_hip_cgmres_set_problem(nmpc_hip_cgmres_handle h, const void * params, size_t bytes, int per_instance);

  /** x_initial_ [B][NX] and u_initial_ [B][NUC] of every instance (HOST arrays; either may be NULL to keep it).  Setup starts from
      them; run() too (it calls setup first, CgmresSolver.cpp:80). */
  int nmpc_hip_cgmres_set_initial(nmpc_hip_cgmres_handle h, const double * x, const double * u);

  /** CgmresSolver::setup (CgmresSolver.cpp:8-64) for every instance: x_ and u_ from the initial values, u_ by the Newton / GMRES
      loop, u_list_ filled with it, delta_u_vec_ zeroed.  Synchronous. */
  int nmpc_hip_cgmres_setup(nmpc_hip_cgmres_handle h);

  /** CgmresSolver::run (CgmresSolver.cpp:66-107) for every instance: setup, then the ticks t = 0, dt, ... while t <= sim_duration
      (t accumulated in fp64 as there), each simulating next_x with sim_ode_solver, calling calcControlInput and logging every
      dump_step-th tick.  Synchronous. */
  int nmpc_hip_cgmres_run(nmpc_hip_cgmres_handle h);

  /** CgmresSolver::calcControlInput(t, x, next_x, u) (CgmresSolver.cpp:109-143) for every instance: HOST arrays t [B],
      x / next_x [B][NX], u out [B][NUC].  Needs setup.  Synchronous. */
  int nmpc_hip_cgmres_control_input(nmpc_hip_cgmres_handle h, const double * t, const double * x, const double * next_x, double * u);
  /** Same with DEVICE arrays of the same layouts, asynchronous on `stream` (hipStream_t; NULL = the solver's own stream). */
  int nmpc_hip_cgmres_control_input_device(nmpc_hip_cgmres_handle h,
                                           const double * d_t,
                                           const double * d_x,
                                           const double * d_next_x,
                                           double * d_u,
                                           void * stream);
  int nmpc_hip_cgmres_synchronize(nmpc_hip_cgmres_handle h);

  /** Copy one field (layouts above) to HOST memory; bytes must equal nmpc_hip_cgmres_field_bytes. */
  int nmpc_hip_cgmres_get(nmpc_hip_cgmres_handle h, int field, void * out, size_t bytes);
  int nmpc_hip_cgmres_field_bytes(nmpc_hip_cgmres_handle h, int field, size_t * bytes);

  /** Diagnostic: Gmres::solve (Gmres.h:42-125, make_triangular_ = true) on `batch` dense systems A x = b on `device`: HOST arrays
      A [batch][n][n], b [batch][n], x [batch][n] (the initial guess in, the solution out), iters / reorth [batch] int out (may be
      NULL).  1 <= n <= 512; k_max is clamped to n as there. */
  int nmpc_hip_cgmres_dense_gmres(int device,
                                  int batch,
                                  int n,
                                  const double * A,
                                  const double * b,
                                  double * x,
                                  int k_max,
                                  int apply_reorth,
                                  double eps,
                                  int * iters,
                                  int * reorth);

  /** Diagnostic: the four problem functions at n_points points with the handle's problem objects (point p uses instance p % B's):
      HOST arrays t [P], x [P][NX], u [P][NUC], lmd [P][NX] in; dotx, dotlmd, DphiDx [P][NX], DhDu [P][NUC] out.
      costateEquation gets xu = (x, u). */
  int nmpc_hip_cgmres_model_eval(nmpc_hip_cgmres_handle h,
                                 int n_points,
                                 const double * t,
                                 const double * x,
                                 const double * u,
                                 const double * lmd,
                                 double * dotx,
                                 double * dotlmd,
                                 double * dphidx,
                                 double * dhdu);

  /** Time of the last setup / run / control_input [ms] (HIP events around the launches). */
  int nmpc_hip_cgmres_last_ms(nmpc_hip_cgmres_handle h, float * ms);

  /** Text of the last error raised on this thread. */
  const char * nmpc_hip_cgmres_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* NMPC_HIP_CGMRES_H */
