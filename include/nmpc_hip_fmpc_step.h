/* C-ABI of the MI355X-native batched FMPC iteration on caller-supplied linearisations (part of libnmpc_hip_ddp.so).
 *
 * Boundary for the model-free part of the reference's interior-point solver: one FmpcSolver::procOnce (nmpc_fmpc/include/nmpc_fmpc/
 * FmpcSolver.hpp:365-493 and what it calls) with enable_line_search = false, the reference's default.  B independent instances of one
 * run-time shape (state dimension n, input capacity m, inequality capacity g, T steps) take one iteration per step() on a gfx950
 * device, one wavefront per instance (fmpc_step_wave_kernel, include/nmpc_amd/hip/fmpc_step_kernels.hpp).  The caller supplies the
 * Jacobians A, B, C, D, the cost derivatives and the two function values stateEq(t, x, u) and ineqConst(t, x, u) of every step at the
 * CURRENT variable; no problem class is compiled in.  The handle owns the variable (x, u, lambda, s, nu and barrier_eps): a step()
 * without a set_variable in between continues from the variable the step before left.  The merit line search needs model evaluations
 * at trial points and is the caller's to run (apply_update = 0 returns the delta and the two step lengths and leaves the variable).
 *
 * Plain pointers and sizes only.  Every function returns 0 (NMPC_HIP_OK) or a negative nmpc_hip_status (nmpc_hip_ddp.h); nothing
 * throws across this boundary.  Arguments are validated before the device is probed.  There is no CPU fallback: without a gfx950
 * device create() reports NMPC_HIP_ERR_NO_DEVICE.  Everything is fp64, compiled without FMA contraction.
 *
 * Layouts at this boundary (doubles unless noted; B = batch):
 *   A, Lxx     [B][T][n*n]     B, Lxu   [B][T][n*m]     C   [B][T][g*n]     D   [B][T][g*m]     Luu   [B][T][m*m]
 *   Lx, f      [B][T][n]       Lu       [B][T][m]       g   [B][T][g]
 *   Lx_T       [B][n]          Lxx_T    [B][n*n]        current_x   [B][n]
 *   x, lambda  [B][T+1][n]     u        [B][T][m]       s, nu   [B][T][g]       barrier_eps   [B]
 * A matrix block has the handle's capacities (B is n x m even at a step with fewer inputs, C is g x n).  row_major = 0 stores a block
 * column-major (entry (r, c) at r + rows * c: Eigen, and the rest of this C-ABI); row_major = 1 stores it [rows][cols] (a contiguous
 * numpy or torch [B, T, rows, cols] array).  The flag covers every matrix, input and output.  At a step with dimensions m_i < m or
 * g_i < g (set_step_dims) only the leading m_i and g_i rows and columns of a block and entries of a vector are read, outputs beyond
 * them are written as exactly 0, variable entries beyond them are left alone, and a step with m_i = 0 takes FmpcSolver.hpp:620-624.
 *
 * Fields of get():
 *   STATUS        [B] int         FmpcSolver::Status of this procOnce (FmpcSolver.h:92-114); 6 = IterationContinued
 *   KKT_ERROR     [B]             calcKktError(0.0)                                 (:496-521)
 *   BARRIER_EPS   [B]             barrier_eps_ after the call                       (:378-399)
 *   ALPHA_S_MAX, ALPHA_NU_MAX [B] the fraction-to-boundary step lengths             (:713-750)
 *   K_FF          [B][T][m]       k                                                 (:599)
 *   K_FB          [B][T][m*n]     K, an m x n block                                 (:600)
 *   S             [B][T+1][n]     s                                                 (:633)
 *   P             [B][T+1][n*n]   P, symmetrised                                    (:634-637)
 *   DELTA_X, DELTA_LAMBDA [B][T+1][n]   DELTA_U [B][T][m]   DELTA_S, DELTA_NU [B][T][g]     (:668-696)
 *   VAR_X, VAR_LAMBDA     [B][T+1][n]   VAR_U   [B][T][m]   VAR_S, VAR_NU     [B][T][g]     the variable after the call
 * An instance whose status is Succeeded or an error keeps its variable bit for bit; its gains, delta and step lengths are those the
 * iteration had computed when it stopped (unspecified beyond that point).  Two things happen BEFORE the iteration and are therefore
 * exceptions to this, whatever the status and whatever apply_update says: with init_complementary_variable = 1, s and nu (and
 * barrier_eps = 1e-4) of every instance are overwritten from g (:172-188); with update_barrier_eps = 1, barrier_eps of every instance
 * is rewritten (:378-399).  x, u and lambda of such an instance are never touched.
 *
 * Ordering of DEVICE arrays (on_device = 1).  The handle works on a stream of its own, created non-blocking: it waits for no other
 * stream, the null stream included.  This library adds no ordering against the work that produces a device array:
 *   - set_variable copies on the handle's stream, and step() launches there.  The work that writes the arrays must have COMPLETED
 *     (hipStreamSynchronize of the producing stream, or hipDeviceSynchronize) before set_variable, and for the arrays of
 *     set_linearisation before step().
 *   - step_device(h, stream) with the caller's stream launches there: the arrays of set_linearisation are read in stream order, so work
 *     queued on that stream before the call is seen and needs no wait.  With stream = NULL it is the handle's stream, as for step().
 *   - the arrays must stay valid and unwritten until the step has finished (step() returns, or synchronize).
 *   - get(on_device = 1) enqueues its copy on the stream of the last step; order a consumer on another stream behind synchronize.
 * The Python mirror drains torch's current stream before either call when it is handed device tensors.
 */
#ifndef NMPC_HIP_FMPC_STEP_H
#define NMPC_HIP_FMPC_STEP_H

#include <stddef.h>

#include "nmpc_hip_ddp.h" /* nmpc_hip_status */

#define NMPC_HIP_FMPC_STEP_MAX_DIM 16
#define NMPC_HIP_FMPC_STEP_MAX_INEQ 32

#ifdef __cplusplus
extern "C"
{
#endif

  /** The members of FmpcSolver::Configuration that steer procOnce (FmpcSolver.h:57-89), the problem's dt, and this boundary's own
      switches. */
  typedef struct
  {
    double dt; /* problem_->dt(): the weight of the running cost derivatives */
    double kkt_error_thre;
    int check_nan;
    int init_complementary_variable; /* 1: s and nu are set from g before the iteration (:172-188); clear it after the first call */
    int update_barrier_eps;
    int break_if_llt_fails;
    int apply_update; /* 0: return the delta and the step lengths, leave the variable alone */
    int row_major; /* storage order of every matrix block, see above */
  } nmpc_hip_fmpc_step_config;

  typedef enum
  {
    NMPC_HIP_FMPC_STEP_FIELD_STATUS = 0, /* int */
    NMPC_HIP_FMPC_STEP_FIELD_KKT_ERROR = 1,
    NMPC_HIP_FMPC_STEP_FIELD_BARRIER_EPS = 2,
    NMPC_HIP_FMPC_STEP_FIELD_ALPHA_S_MAX = 3,
    NMPC_HIP_FMPC_STEP_FIELD_ALPHA_NU_MAX = 4,
    NMPC_HIP_FMPC_STEP_FIELD_K_FF = 5,
    NMPC_HIP_FMPC_STEP_FIELD_K_FB = 6,
    NMPC_HIP_FMPC_STEP_FIELD_S = 7,
    NMPC_HIP_FMPC_STEP_FIELD_P = 8,
    NMPC_HIP_FMPC_STEP_FIELD_DELTA_X = 9,
    NMPC_HIP_FMPC_STEP_FIELD_DELTA_U = 10,
    NMPC_HIP_FMPC_STEP_FIELD_DELTA_LAMBDA = 11,
    NMPC_HIP_FMPC_STEP_FIELD_DELTA_S = 12,
    NMPC_HIP_FMPC_STEP_FIELD_DELTA_NU = 13,
    NMPC_HIP_FMPC_STEP_FIELD_VAR_X = 14,
    NMPC_HIP_FMPC_STEP_FIELD_VAR_U = 15,
    NMPC_HIP_FMPC_STEP_FIELD_VAR_LAMBDA = 16,
    NMPC_HIP_FMPC_STEP_FIELD_VAR_S = 17,
    NMPC_HIP_FMPC_STEP_FIELD_VAR_NU = 18
  } nmpc_hip_fmpc_step_field;

  /** FmpcSolver::Status (FmpcSolver.h:92-114). */
  typedef enum
  {
    NMPC_HIP_FMPC_STEP_UNINITIALIZED = 0,
    NMPC_HIP_FMPC_STEP_SUCCEEDED = 1,
    NMPC_HIP_FMPC_STEP_ERROR_IN_FORWARD = 2,
    NMPC_HIP_FMPC_STEP_ERROR_IN_BACKWARD = 3,
    NMPC_HIP_FMPC_STEP_ERROR_IN_UPDATE = 4,
    NMPC_HIP_FMPC_STEP_MAX_ITERATION_REACHED = 5,
    NMPC_HIP_FMPC_STEP_ITERATION_CONTINUED = 6
  } nmpc_hip_fmpc_step_status;

  typedef struct nmpc_hip_fmpc_step_solver * nmpc_hip_fmpc_step_handle;

  /** The reference's defaults (FmpcSolver.h:57-89): kkt_error_thre 1e-4, check_nan 1, init_complementary_variable 0,
      update_barrier_eps 1, break_if_llt_fails 0; dt 0.01, apply_update 1, row_major 0. */
  int nmpc_hip_fmpc_step_default_config(nmpc_hip_fmpc_step_config * cfg);

  /** `batch` instances of shape (state_dim, input_dim, ineq_dim, horizon_steps) on HIP device `device`; 1 <= state_dim <= 16,
      0 <= input_dim <= 16, 0 <= ineq_dim <= 32, horizon_steps >= 1, batch >= 1.  The handle owns the variable, the output buffers and
      the residual workspace; barrier_eps starts at 1e-4 (FmpcSolver.h:414).  The staging copies of host inputs are allocated by the
      first call that needs them.  An allocation that fails is NMPC_HIP_ERR_RUNTIME. */
  int nmpc_hip_fmpc_step_create(int state_dim,
                                int input_dim,
                                int ineq_dim,
                                int horizon_steps,
                                int batch,
                                int device,
                                nmpc_hip_fmpc_step_handle * out);
  int nmpc_hip_fmpc_step_destroy(nmpc_hip_fmpc_step_handle h);

  /** A dt or kkt_error_thre that is NaN is NMPC_HIP_ERR_INVALID_ARGUMENT. */
  int nmpc_hip_fmpc_step_set_config(nmpc_hip_fmpc_step_handle h, const nmpc_hip_fmpc_step_config * cfg);
  int nmpc_hip_fmpc_step_get_config(nmpc_hip_fmpc_step_handle h, nmpc_hip_fmpc_step_config * cfg);

  /** inputDim(t) and ineqDim(t) of every step: HOST arrays [T], each 0 .. input_dim (0 .. ineq_dim), shared by the batch; NULL = the
      capacity everywhere. */
  int nmpc_hip_fmpc_step_set_step_dims(nmpc_hip_fmpc_step_handle h, const int * input_dims, const int * ineq_dims);

  /** The linearisation at the current variable: HOST (on_device = 0) or DEVICE (on_device = 1) arrays in the layouts above, in the
      storage order of the CURRENT config's row_major.  Host arrays are copied; device arrays are read in place by step() and must stay
      valid until synchronize, and what writes them is ordered before the step by the caller ("Ordering of DEVICE arrays" above).
      Arrays of a block with no entries (input_dim = 0 or ineq_dim = 0) may be NULL. */
  int nmpc_hip_fmpc_step_set_linearisation(nmpc_hip_fmpc_step_handle h,
                                           const double * A,
                                           const double * B,
                                           const double * C,
                                           const double * D,
                                           const double * Lx,
                                           const double * Lu,
                                           const double * Lxx,
                                           const double * Luu,
                                           const double * Lxu,
                                           const double * f,
                                           const double * g,
                                           const double * Lx_T,
                                           const double * Lxx_T,
                                           const double * current_x,
                                           int on_device);

  /** variable_ (FmpcSolver.h:117-158) of every instance, copied into the handle from HOST or DEVICE arrays; barrier_eps ([B]) may
      be NULL: the handle's values stay.  DEVICE arrays are copied on the handle's stream: what writes them must have completed. */
  int nmpc_hip_fmpc_step_set_variable(nmpc_hip_fmpc_step_handle h,
                                      const double * x,
                                      const double * u,
                                      const double * lambda,
                                      const double * s,
                                      const double * nu,
                                      const double * barrier_eps,
                                      int on_device);

  /** One procOnce of every instance; synchronous.  NMPC_HIP_ERR_NOT_SOLVED without set_linearisation and set_variable;
      NMPC_HIP_ERR_INVALID_ARGUMENT with update_barrier_eps and no inequality at any step (the reference divides 0 by 0 there). */
  int nmpc_hip_fmpc_step_step(nmpc_hip_fmpc_step_handle h);
  /** The same, asynchronous on `stream` (hipStream_t; NULL = the handle's own stream). */
  int nmpc_hip_fmpc_step_step_device(nmpc_hip_fmpc_step_handle h, void * stream);
  /** Wait for the last step_device. */
  int nmpc_hip_fmpc_step_synchronize(nmpc_hip_fmpc_step_handle h);

  /** Copy one field to HOST (on_device = 0) or DEVICE (on_device = 1) memory; bytes must equal nmpc_hip_fmpc_step_field_bytes.
      on_device = 0 waits for the step; on_device = 1 enqueues the copy behind it on the step's stream and returns.  The VAR fields
      can be read once set_variable has been called; every other field is NMPC_HIP_ERR_NOT_SOLVED before a step. */
  int nmpc_hip_fmpc_step_get(nmpc_hip_fmpc_step_handle h, int field, void * out, size_t bytes, int on_device);
  int nmpc_hip_fmpc_step_field_bytes(nmpc_hip_fmpc_step_handle h, int field, size_t * bytes);

  /** "fmpc_step_wave_kernel". */
  int nmpc_hip_fmpc_step_kernel_name(nmpc_hip_fmpc_step_handle h, const char ** name);
  /** Device time of the last step [ms] (HIP events around its launch; after step_device: once it has finished). */
  int nmpc_hip_fmpc_step_last_ms(nmpc_hip_fmpc_step_handle h, float * ms);
  /** Text of the last error raised on this thread. */
  const char * nmpc_hip_fmpc_step_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* NMPC_HIP_FMPC_STEP_H */
