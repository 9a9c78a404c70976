/* C-ABI of the MI355X-native batched Riccati backward pass on caller-supplied derivatives (part of libnmpc_hip_ddp.so).
 *
 * Boundary for the model-free part of the reference's DDP solver: DDPSolver::backwardPass (nmpc_ddp/include/nmpc_ddp/DDPSolver.hpp:
 * 342-534) with the lambda retry loop of procOnce (:188-214) and the BoxQP feed-forward (:450-497, BoxQP.h:141-347).  B independent
 * instances of one run-time shape (state dimension n, input capacity m, T steps) are solved in one launch on a gfx950 device, one
 * wavefront per instance (riccati_wave_kernel, include/nmpc_amd/hip/riccati_kernels.hpp).  The caller supplies the Derivative blocks
 * of every step (DDPSolver.h: Fx, Fu, Lx, Lu, Lxx, Luu, Lxu) and the terminal Vx, Vxx; no problem class is compiled in.  Plain
 * pointers and sizes only.  Every function returns 0 (NMPC_HIP_OK) or a negative nmpc_hip_status (nmpc_hip_ddp.h); nothing throws
 * across this boundary.  Arguments are validated before the device is probed.  There is no CPU fallback: without a gfx950 device
 * create() reports NMPC_HIP_ERR_NO_DEVICE.  Everything is fp64, compiled without FMA contraction.
 *
 * Layouts at this boundary (doubles unless noted; B = batch):
 *   Fx, Lxx        [B][T][n*n]      Fu, Lxu   [B][T][n*m]      Luu   [B][T][m*m]
 *   Lx             [B][T][n]        Lu, U     [B][T][m]
 *   lower, upper   [m] (limits_per_step = 0) or [B][T][m] (limits_per_step = 1)
 *   Vx_T           [B][n]           Vxx_T     [B][n*n]
 * A matrix block has the handle's capacities (Fu is n x m even at a step with fewer inputs).  row_major = 0 stores a block
 * column-major (entry (r, c) at r + rows * c: Eigen, and the rest of this C-ABI); row_major = 1 stores it [rows][cols] (entry (r, c)
 * at r * cols + c: a contiguous numpy or torch [B, T, rows, cols] array).  The flag covers every matrix, input and output.  At a step
 * with input dimension m_i < m (set_input_dims) only the leading m_i columns and rows of a block are read, outputs beyond m_i are
 * written as exactly 0, and a step with m_i = 0 takes the branch of DDPSolver.hpp:513-517.
 *
 * Fields of get():
 *   K_FF        [B][T][m]      k                                      (:509, :471)
 *   K_FB        [B][T][m*n]    K, an m x n block                      (:510, :482-496)
 *   DV          [B][2]         dV_                                    (:522)
 *   VX0         [B][n]         Vx after step 0                        (:523)
 *   VXX0        [B][n*n]       Vxx after step 0, symmetrised          (:524-526)
 *   STATUS      [B] int        nmpc_hip_riccati_status
 *   N_BACKWARD  [B] int        passes started
 *   LAMBDA, DLAMBDA  [B]       lambda_, dlambda_ after the retries: what the caller carries into its next iteration
 *   FAIL_STEP   [B] int        step at which the last failed pass stopped; -1 if none failed
 *   QP_RETVAL   [B][T] int     BoxQP::retval_ of each step (0 without with_input_constraint)
 *   FREE_MASK   [B][T] uint32  bit j set = variable j is free (BoxQP::free_idxs_)
 * The gains of an instance whose status is negative are unspecified.
 */
#ifndef NMPC_HIP_RICCATI_H
#define NMPC_HIP_RICCATI_H

#include <stddef.h>

#include "nmpc_hip_ddp.h" /* nmpc_hip_status */

#define NMPC_HIP_RICCATI_MAX_DIM 16

#ifdef __cplusplus
extern "C"
{
#endif

  /** The members of DDPSolver::Configuration that steer the backward pass (DDPSolver.h:47-110), and this boundary's own switches. */
  typedef struct
  {
    int reg_type; /* 1: Quu_F diagonal (:438-441), 2: Vxx diagonal (:422-425) */
    double lambda; /* initial_lambda: used when set_lambda gave no per-instance array */
    double dlambda; /* initial_dlambda: likewise */
    double lambda_factor;
    double lambda_min;
    double lambda_max;
    int with_input_constraint; /* run the BoxQP feed-forward (:450-497); needs set_inputs */
    int retry; /* 1: the loop of :191-209 on the device; 0: one pass */
    int row_major; /* storage order of every matrix block, see above */
  } nmpc_hip_riccati_config;

  typedef enum
  {
    NMPC_HIP_RICCATI_FIELD_K_FF = 0,
    NMPC_HIP_RICCATI_FIELD_K_FB = 1,
    NMPC_HIP_RICCATI_FIELD_DV = 2,
    NMPC_HIP_RICCATI_FIELD_VX0 = 3,
    NMPC_HIP_RICCATI_FIELD_VXX0 = 4,
    NMPC_HIP_RICCATI_FIELD_STATUS = 5, /* int */
    NMPC_HIP_RICCATI_FIELD_N_BACKWARD = 6, /* int */
    NMPC_HIP_RICCATI_FIELD_LAMBDA = 7,
    NMPC_HIP_RICCATI_FIELD_DLAMBDA = 8,
    NMPC_HIP_RICCATI_FIELD_FAIL_STEP = 9, /* int */
    NMPC_HIP_RICCATI_FIELD_QP_RETVAL = 10, /* int */
    NMPC_HIP_RICCATI_FIELD_FREE_MASK = 11 /* uint32 */
  } nmpc_hip_riccati_field;

  typedef enum
  {
    NMPC_HIP_RICCATI_OK = 1, /* a pass succeeded */
    NMPC_HIP_RICCATI_LAMBDA_MAX = -1, /* lambda passed lambda_max (:196-204) */
    NMPC_HIP_RICCATI_PASS_FAILED = -2 /* retry = 0 and the pass failed */
  } nmpc_hip_riccati_status;

  typedef struct nmpc_hip_riccati_solver * nmpc_hip_riccati_handle;

  /** The reference's defaults (DDPSolver.h:47-110): reg_type 1, initial_lambda 1e-4, initial_dlambda 1, lambda_factor 1.6,
      lambda_min 1e-6, lambda_max 1e10, with_input_constraint 0; retry 1, row_major 0. */
  int nmpc_hip_riccati_default_config(nmpc_hip_riccati_config * cfg);

  /** `batch` instances of shape (state_dim, input_dim, horizon_steps) on HIP device `device`; 1 <= state_dim <= 16,
      0 <= input_dim <= 16, horizon_steps >= 1, batch >= 1.  The handle owns the output buffers; the staging copies of host inputs
      are allocated by the first call that needs them.  An allocation that fails is NMPC_HIP_ERR_RUNTIME. */
  int nmpc_hip_riccati_create(int state_dim, int input_dim, int horizon_steps, int batch, int device, nmpc_hip_riccati_handle * out);
  int nmpc_hip_riccati_destroy(nmpc_hip_riccati_handle h);

  /** reg_type other than 1 or 2, a lambda_factor / lambda_min / lambda_max that is not finite, is NMPC_HIP_ERR_INVALID_ARGUMENT. */
  int nmpc_hip_riccati_set_config(nmpc_hip_riccati_handle h, const nmpc_hip_riccati_config * cfg);
  int nmpc_hip_riccati_get_config(nmpc_hip_riccati_handle h, nmpc_hip_riccati_config * cfg);

  /** Fu.cols() of every step (:381): HOST array dims[T], each 0 .. input_dim, shared by the batch; NULL = input_dim everywhere. */
  int nmpc_hip_riccati_set_input_dims(nmpc_hip_riccati_handle h, const int * dims);

  /** derivative_list_ (:371-380) and last_Vx_, last_Vxx_ (:346-347) of every instance: HOST (on_device = 0) or DEVICE
      (on_device = 1) arrays in the layouts above, in the storage order of the CURRENT config's row_major.  Host arrays are copied;
      device arrays are read in place by the solves and must stay valid until synchronize.  Arrays of a block with no entries
      (input_dim = 0) may be NULL. */
  int nmpc_hip_riccati_set_derivatives(nmpc_hip_riccati_handle h,
                                       const double * Fx,
                                       const double * Fu,
                                       const double * Lx,
                                       const double * Lu,
                                       const double * Lxx,
                                       const double * Luu,
                                       const double * Lxu,
                                       const double * Vx_T,
                                       const double * Vxx_T,
                                       int on_device);

  /** control_data_.u_list and input_limits_func_ (:470-472) for with_input_constraint: the QP bounds of step i are lower - u_i and
      upper - u_i.  limits_per_step = 0: lower, upper are [m], shared; 1: [B][T][m].  Same copying rule as set_derivatives. */
  int nmpc_hip_riccati_set_inputs(nmpc_hip_riccati_handle h,
                                  const double * U,
                                  const double * lower,
                                  const double * upper,
                                  int limits_per_step,
                                  int on_device);

  /** lambda_ and dlambda_ per instance ([B] each); NULL = the config's scalar for all.  Same copying rule. */
  int nmpc_hip_riccati_set_lambda(nmpc_hip_riccati_handle h, const double * lambda, const double * dlambda, int on_device);

  /** The retry loop around backwardPass (:188-214) for every instance; synchronous.  NMPC_HIP_ERR_NOT_SOLVED without
      set_derivatives, or with with_input_constraint and no set_inputs. */
  int nmpc_hip_riccati_solve(nmpc_hip_riccati_handle h);
  /** The same, asynchronous on `stream` (hipStream_t; NULL = the handle's own stream). */
  int nmpc_hip_riccati_solve_device(nmpc_hip_riccati_handle h, void * stream);
  /** Wait for the last solve_device. */
  int nmpc_hip_riccati_synchronize(nmpc_hip_riccati_handle h);

  /** Copy one field of the last solve to HOST (on_device = 0) or DEVICE (on_device = 1) memory; bytes must equal
      nmpc_hip_riccati_field_bytes.  on_device = 0 waits for the solve; on_device = 1 enqueues the copy behind it on the solve's
      stream and returns.  NMPC_HIP_ERR_NOT_SOLVED before a solve. */
  int nmpc_hip_riccati_get(nmpc_hip_riccati_handle h, int field, void * out, size_t bytes, int on_device);
  int nmpc_hip_riccati_field_bytes(nmpc_hip_riccati_handle h, int field, size_t * bytes);

  /** "riccati_wave_kernel". */
  int nmpc_hip_riccati_kernel_name(nmpc_hip_riccati_handle h, const char ** name);
  /** Device time of the last solve [ms] (HIP events around its launch; after solve_device: once it has finished). */
  int nmpc_hip_riccati_last_ms(nmpc_hip_riccati_handle h, float * ms);
  /** Text of the last error raised on this thread. */
  const char * nmpc_hip_riccati_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* NMPC_HIP_RICCATI_H */
