/* C-ABI of the MI355X-native batched BoxQP solver (part of libnmpc_hip_ddp.so).
 *
 * Boundary for the reference's nmpc_ddp::BoxQP<VarDim> (nmpc_ddp/include/nmpc_ddp/BoxQP.h:18-397), the projected-Newton solver of
 *   min_x 1/2 x'Hx + g'x   s.t.  lower <= x <= upper
 * (Tassa, Mansard, Todorov, ICRA 2014): B independent QPs of one size n = var_dim, solved in one launch on a gfx950 device.  The
 * reference has no FFI layer; each entry point cites the member it replaces.  Plain pointers and sizes only.  Every function
 * returns 0 (NMPC_HIP_OK) or a negative nmpc_hip_status (nmpc_hip_ddp.h); nothing throws across this boundary.  Arguments are
 * validated before the device is probed.  There is no CPU fallback: without a gfx950 device create() reports
 * NMPC_HIP_ERR_NO_DEVICE.  Everything is fp64.
 *
 * Layouts at this boundary (row-major in the order written, doubles unless noted; n = var_dim, B = batch):
 *   H                 [B][n][n]   H[b][i][j] = H(i, j).  The contract is a SYMMETRIC H.  As in the reference, the factorisation
 *                                 reads the LOWER triangle (i >= j) of the free block only (Eigen::LLT, BoxQP.h:229) while every
 *                                 product H x (objective, gradient, right-hand side; BoxQP.h:149, 184, 273, 297) reads the full
 *                                 matrix.
 *   g, lower, upper   [B][n]
 *   initial_x         [B][n]      NULL = zeros (the four-argument overload, BoxQP.h:126-132)
 *   X                 [B][n]      the returned x                                     (BoxQP.h:346)
 *   RETVAL            [B] int     retval_, the codes of BoxQP.h:375-383              (BoxQP.h:372)
 *   ITER              [B] int     iter at the exit of the main loop                  (BoxQP.h:166-168)
 *   FACTORIZATION_NUM [B] int     factorization_num                                  (BoxQP.h:162, 240)
 *   FREE_MASK         [B] uint64  bit j set <=> j is in free_idxs_                   (BoxQP.h:389)
 *   OBJ               [B]         obj of the returned x                              (BoxQP.h:149, 329)
 *   FACTOR            [B][n][n]   llt_free_ (BoxQP.h:386, read by DDPSolver.hpp:473-497): with nf = popcount(FREE_MASK),
 *                                 FACTOR[b][r][c], c <= r < nf, is L(r, c) of H[free, free] = L L' in free_idxs_ order; every other
 *                                 entry is 0.  Defined where FREE_MASK != 0 and RETVAL != -1.
 *   TRACE             [B][trace_capacity][6]  8-byte words: the scalar members of TraceData (BoxQP.h:58-82), row r = the entry
 *                                 with iter == r of traceDataList() (row 0 the initial entry, BoxQP.h:154-158).  Columns: 0 iter,
 *                                 1 obj, 2 factorization_num, 3 step_num (doubles), 4 clamped_flag as the BIT PATTERN of a uint64
 *                                 mask (bit j = clamped_flag[j]; not a converted value: n may be 64), 5 grad_norm of BoxQP.h:244-248
 *                                 (the sum of squares of the free gradient that the reference compares with grad_thre^2).  As in
 *                                 the reference the entry of the iteration that leaves the loop before BoxQP.h:320 has only iter
 *                                 set.  Rows beyond ITER, and rows at or beyond trace_capacity, are not written.
 * On the device the lane kernel keeps its data [element][instance]; the conversion happens inside solve / get.
 *
 * Kernels.  "lane" (boxqp_lane_kernel): one QP per lane of a wavefront, var_dim <= 16.  "wave" (boxqp_wave_kernel): one
 * wavefront per QP, lane j owning variable j, var_dim <= 64.  The automatic choice is a pure function of (var_dim, batch):
 *   lane  if var_dim <= NMPC_HIP_BOXQP_AUTO_LANE_MAX_DIM (3) and batch >= NMPC_HIP_BOXQP_AUTO_LANE_MIN_BATCH (65536),
 *   wave  otherwise.
 * That is the measured crossover (scripts/boxqp_throughput.py): a lane-per-QP kernel needs 64 QPs to fill one
 * wavefront and tens of thousands to fill the chip, and its iterates live in HBM; the wave kernel was the faster one at every
 * measured shape but var_dim 1, 2, 3 at batch 65536 (var_dim 4 there: a tie).
 */
#ifndef NMPC_HIP_BOXQP_H
#define NMPC_HIP_BOXQP_H

#include <stddef.h>

#include "nmpc_hip_ddp.h" /* nmpc_hip_status */

#define NMPC_HIP_BOXQP_MAX_DIM 64
#define NMPC_HIP_BOXQP_LANE_MAX_DIM 16
#define NMPC_HIP_BOXQP_AUTO_LANE_MAX_DIM 3
#define NMPC_HIP_BOXQP_AUTO_LANE_MIN_BATCH 65536
#define NMPC_HIP_BOXQP_TRACE_COLUMNS 6

#ifdef __cplusplus
extern "C"
{
#endif

  /** BoxQP::Configuration (BoxQP.h:33-55) without print_level (the mirrors keep it), plus the trace capacity. */
  typedef struct
  {
    int max_iter; /* :39 */
    double grad_thre; /* :42 */
    double rel_improve_thre; /* :45 */
    double step_factor; /* :48 */
    double min_step; /* :51 */
    double armijo_param; /* :54 */
    int trace_capacity; /* rows of TRACE per QP; 0 = no trace */
  } nmpc_hip_boxqp_config;

  typedef enum
  {
    NMPC_HIP_BOXQP_FIELD_X = 0,
    NMPC_HIP_BOXQP_FIELD_RETVAL = 1, /* int */
    NMPC_HIP_BOXQP_FIELD_ITER = 2, /* int */
    NMPC_HIP_BOXQP_FIELD_FACTORIZATION_NUM = 3, /* int */
    NMPC_HIP_BOXQP_FIELD_FREE_MASK = 4, /* uint64 */
    NMPC_HIP_BOXQP_FIELD_OBJ = 5,
    NMPC_HIP_BOXQP_FIELD_FACTOR = 6,
    NMPC_HIP_BOXQP_FIELD_TRACE = 7
  } nmpc_hip_boxqp_field;

  /** retval_ (BoxQP.h:375-383). */
  typedef enum
  {
    NMPC_HIP_BOXQP_RET_SEARCH_DIR_GRAD_POSITIVE = -2, /* "Gradient of search direction is positive" */
    NMPC_HIP_BOXQP_RET_NOT_POSITIVE_DEFINITE = -1, /* "Hessian is not positive definite" */
    NMPC_HIP_BOXQP_RET_NOT_FINISHED = 0, /* "Computation is not finished" */
    NMPC_HIP_BOXQP_RET_MAX_ITER = 1, /* "Maximum main iterations exceeded" */
    NMPC_HIP_BOXQP_RET_MAX_LINE_SEARCH = 2, /* "Maximum line-search iterations exceeded" */
    NMPC_HIP_BOXQP_RET_NO_BOUNDS = 3, /* "No bounds, returning Newton point" */
    NMPC_HIP_BOXQP_RET_SMALL_IMPROVEMENT = 4, /* "Improvement smaller than tolerance" */
    NMPC_HIP_BOXQP_RET_SMALL_GRADIENT = 5, /* "Gradient norm smaller than tolerance" */
    NMPC_HIP_BOXQP_RET_ALL_CLAMPED = 6 /* "All dimensions are clamped" */
  } nmpc_hip_boxqp_retval;

  typedef struct nmpc_hip_boxqp_solver * nmpc_hip_boxqp_handle;

  /** Fill cfg with the reference defaults (BoxQP.h:33-55): max_iter 500, grad_thre 1e-8, rel_improve_thre 1e-8, step_factor 0.6,
      min_step 1e-22, armijo_param 0.1; trace_capacity 0. */
  int nmpc_hip_boxqp_default_config(nmpc_hip_boxqp_config * cfg);

  /** BoxQP(var_dim) (BoxQP.h:101-118) for `batch` QPs on HIP device `device`; 1 <= var_dim <= 64, batch >= 1.  An allocation that
      fails, here or in a later call, is NMPC_HIP_ERR_RUNTIME with the byte count in the message. */
  int nmpc_hip_boxqp_create(int var_dim, int batch, int device, nmpc_hip_boxqp_handle * out);
  int nmpc_hip_boxqp_destroy(nmpc_hip_boxqp_handle h);

  /** config() (BoxQP.h:350-359). */
  int nmpc_hip_boxqp_set_config(nmpc_hip_boxqp_handle h, const nmpc_hip_boxqp_config * cfg);
  int nmpc_hip_boxqp_get_config(nmpc_hip_boxqp_handle h, nmpc_hip_boxqp_config * cfg);

  /** solve(H, g, lower, upper, initial_x) (BoxQP.h:141-347) for every QP: HOST arrays in the layouts above; initial_x may be NULL
      (BoxQP.h:126-132).  Synchronous. */
  int nmpc_hip_boxqp_solve(nmpc_hip_boxqp_handle h,
                           const double * H,
                           const double * g,
                           const double * lower,
                           const double * upper,
                           const double * initial_x);
  /** The same solve (BoxQP.h:141-347) with DEVICE arrays of the same layouts, asynchronous on `stream` (hipStream_t; NULL = the
      handle's own stream).  The arrays must stay valid until the solve has finished. */
  int nmpc_hip_boxqp_solve_device(nmpc_hip_boxqp_handle h,
                                  const double * d_H,
                                  const double * d_g,
                                  const double * d_lower,
                                  const double * d_upper,
                                  const double * d_initial_x,
                                  void * stream);
  /** Wait for the last solve_device. */
  int nmpc_hip_boxqp_synchronize(nmpc_hip_boxqp_handle h);

  /** Copy one field of the last solve (layouts above; the members BoxQP.h:346, 372, 386, 389 and traceDataList(), BoxQP.h:362) to
      HOST (on_device = 0) or DEVICE (on_device = 1) memory; bytes must equal nmpc_hip_boxqp_field_bytes.  Waits for the solve. */
  int nmpc_hip_boxqp_get(nmpc_hip_boxqp_handle h, int field, void * out, size_t bytes, int on_device);
  int nmpc_hip_boxqp_field_bytes(nmpc_hip_boxqp_handle h, int field, size_t * bytes);

  /** The kernel the next solve launches: "boxqp_lane_kernel" or "boxqp_wave_kernel". */
  int nmpc_hip_boxqp_kernel_name(nmpc_hip_boxqp_handle h, const char ** name);
  /** Pin the kernel: "lane" (var_dim <= 16 only), "wave", or NULL for the automatic choice described above. */
  int nmpc_hip_boxqp_set_kernel(nmpc_hip_boxqp_handle h, const char * kernel);

  /** Device time of the last solve [ms] (HIP events around its launches; after solve_device: once it has finished). */
  int nmpc_hip_boxqp_last_solve_ms(nmpc_hip_boxqp_handle h, float * ms);

  /** Text of the last error raised on this thread. */
  const char * nmpc_hip_boxqp_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* NMPC_HIP_BOXQP_H */
