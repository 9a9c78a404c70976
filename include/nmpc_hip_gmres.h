/* C-ABI of the MI355X-native batched GMRES solver (part of libnmpc_hip_ddp.so).
 *
 * Boundary for the reference's nmpc_cgmres::Gmres (nmpc_cgmres/include/nmpc_cgmres/Gmres.h:21-204), the dense-matrix overload of
 * solve() (Gmres.h:42-51): B independent systems A x = b of one size n, solved in one launch on a gfx950 device, one wavefront per
 * system (gmres_wave_kernel, include/nmpc_amd/hip/gmres_kernels.hpp).  Both variants of the reference exist: the Givens
 * ("triangular", make_triangular_ = true, Gmres.h:135-168) and the Householder least-squares one (make_triangular_ = false,
 * Gmres.h:169-176).  The reference has no FFI layer; each entry point cites the lines it replaces.  Plain pointers and sizes only.
 * Every function returns 0 (NMPC_HIP_OK) or a negative nmpc_hip_status (nmpc_hip_ddp.h); nothing throws across this boundary.
 * Arguments are validated before the device is probed.  There is no CPU fallback: without a gfx950 device create() reports
 * NMPC_HIP_ERR_NO_DEVICE.  Everything is fp64, compiled without FMA contraction.
 *
 * Layouts at this boundary (row-major in the order written, doubles unless noted; B = batch, k_max = the configured k_max clamped
 * to n as in Gmres.h:73):
 *   A         [B][n][n]            a_col_major = 0: A[b][i][j] = A(i, j), the reference's (i, j) at i * n + j;
 *                                  a_col_major = 1: A[b][j][i] = A(i, j), the transposed image the kernel reads
 *   b, x0     [B][n]               x0 NULL = zeros
 *   X         [B][n]               x                                                   (Gmres.h:188-191)
 *   ITERS     [B] int              the final k                                         (Gmres.h:94-98)
 *   REORTH    [B] int              iterations whose re-orthogonalisation fired         (Gmres.h:120)
 *   ERR_LIST  [B][k_max+1]         err_list_ (Gmres.h:88, 178); entries beyond ITERS are NaN
 *   H         [B][k_max+1][k_max]  H_ as the reference leaves it (Gmres.h:87): rotated in the triangular variant, the raw
 *                                  Hessenberg matrix in the Householder variant; zero where the reference never wrote
 *   G         [B][k_max+1]         g_ (Gmres.h:83-84, 161-164)
 *   BASIS     [B][k_max+1][n]      basis_ (Gmres.h:80, 133): rows 0 .. ITERS; rows beyond are not written.  Readable only with
 *                                  keep_basis = 1 (NMPC_HIP_ERR_INVALID_ARGUMENT otherwise)
 *   STATUS    [B] int              nmpc_hip_gmres_status
 * The reference has no breakdown guard and neither has this solver: nu == 0 (Gmres.h:150-154) gives NaN there and NaN here, and
 * the system reports NMPC_HIP_GMRES_NON_FINITE.
 */
#ifndef NMPC_HIP_GMRES_H
#define NMPC_HIP_GMRES_H

#include <stddef.h>

#include "nmpc_hip_ddp.h" /* nmpc_hip_status */

/* the bound of the dense-GMRES diagnostic (nmpc_hip_cgmres_dense_gmres); the reference's own test stops at 500 */
#define NMPC_HIP_GMRES_MAX_DIM 512
/* Householder variant: the clamped k_max may not exceed this.  Its working copy of the (k + 1) x k least-squares problem, with the
   right-hand side as one more column, lives in LDS: (K + 1)^2 doubles = 133 128 bytes at K = 128, beside 15.4 KB of vectors
   (two of n <= 512, the reflector, y, g and the Givens arrays): 148.5 KB of the 160 KB a gfx950 workgroup may use.  K = 144 would
   need 168 KB.  The reference's test uses the variant up to n = 100. */
#define NMPC_HIP_GMRES_HOUSEHOLDER_MAX_K 128

#ifdef __cplusplus
extern "C"
{
#endif

  /** The arguments and members of Gmres that steer a solve (Gmres.h:45-46, 195-196). */
  typedef struct
  {
    int k_max; /* :45, clamped to n at :73 */
    double eps; /* :46 */
    int make_triangular; /* :195 */
    int apply_reorth; /* :196 */
    int keep_basis; /* 1: BASIS may be read after a solve */
  } nmpc_hip_gmres_config;

  typedef enum
  {
    NMPC_HIP_GMRES_FIELD_X = 0,
    NMPC_HIP_GMRES_FIELD_ITERS = 1, /* int */
    NMPC_HIP_GMRES_FIELD_REORTH = 2, /* int */
    NMPC_HIP_GMRES_FIELD_ERR_LIST = 3,
    NMPC_HIP_GMRES_FIELD_H = 4,
    NMPC_HIP_GMRES_FIELD_G = 5,
    NMPC_HIP_GMRES_FIELD_BASIS = 6,
    NMPC_HIP_GMRES_FIELD_STATUS = 7 /* int */
  } nmpc_hip_gmres_field;

  typedef enum
  {
    NMPC_HIP_GMRES_CONVERGED = 1, /* left the loop of Gmres.h:94 with rho <= eps * b_norm */
    NMPC_HIP_GMRES_K_MAX = 2, /* left it at k == k_max */
    NMPC_HIP_GMRES_NON_FINITE = 3 /* rho or an entry of x is not finite */
  } nmpc_hip_gmres_status;

  typedef struct nmpc_hip_gmres_solver * nmpc_hip_gmres_handle;

  /** The reference's defaults: k_max 100, eps 1e-10 (Gmres.h:45-46), make_triangular 1, apply_reorth 1 (:195-196); keep_basis 0. */
  int nmpc_hip_gmres_default_config(nmpc_hip_gmres_config * cfg);

  /** Gmres() (Gmres.h:31) for `batch` systems of size n on HIP device `device`; 1 <= n <= 512, batch >= 1, k_max_capacity >= 1.
      The handle owns every device buffer, sized for a k_max of min(k_max_capacity, n).  An allocation that fails is
      NMPC_HIP_ERR_RUNTIME with the byte count in the message. */
  int nmpc_hip_gmres_create(int n, int batch, int k_max_capacity, int device, nmpc_hip_gmres_handle * out);
  int nmpc_hip_gmres_destroy(nmpc_hip_gmres_handle h);

  /** The arguments k_max, eps (Gmres.h:45-46) and the members make_triangular_, apply_reorth_ (:195-196) of the next solves.
      k_max (clamped to n) above the capacity, or above NMPC_HIP_GMRES_HOUSEHOLDER_MAX_K with make_triangular = 0, is
      NMPC_HIP_ERR_INVALID_ARGUMENT. */
  int nmpc_hip_gmres_set_config(nmpc_hip_gmres_handle h, const nmpc_hip_gmres_config * cfg);
  int nmpc_hip_gmres_get_config(nmpc_hip_gmres_handle h, nmpc_hip_gmres_config * cfg);

  /** The arguments A, b, x of solve() (Gmres.h:42-44) for every system, HOST (on_device = 0) or DEVICE (on_device = 1) arrays in
      the layouts above; x0 may be NULL (zeros).  b and x0 are copied.  A row-major A is transposed into the handle's image by the
      ingest kernel; with on_device = 1 and a_col_major = 1 nothing is copied and d_A must stay valid until the next set_system.
      Returns once the copies have finished. */
  int nmpc_hip_gmres_set_system(nmpc_hip_gmres_handle h, const double * A, const double * b, const double * x0, int on_device, int a_col_major);

  /** solve() (Gmres.h:67-192) for every system from the handle's current x; synchronous.  A second solve without a new set_system
      continues from the x of the first: restarted GMRES, as a caller of the reference loops solve(). */
  int nmpc_hip_gmres_solve(nmpc_hip_gmres_handle h);
  /** The same solve (Gmres.h:67-192), asynchronous on `stream` (hipStream_t; NULL = the handle's own stream). */
  int nmpc_hip_gmres_solve_device(nmpc_hip_gmres_handle h, void * stream);
  /** Wait for the last solve_device. */
  int nmpc_hip_gmres_synchronize(nmpc_hip_gmres_handle h);

  /** Copy one field of the last solve (layouts above; x and the members H_, g_, err_list_, basis_ of Gmres.h:198-203) to HOST
      (on_device = 0) or DEVICE (on_device = 1) memory; bytes must equal nmpc_hip_gmres_field_bytes.  Waits for the solve. */
  int nmpc_hip_gmres_get(nmpc_hip_gmres_handle h, int field, void * out, size_t bytes, int on_device);
  int nmpc_hip_gmres_field_bytes(nmpc_hip_gmres_handle h, int field, size_t * bytes);

  /** "gmres_wave_kernel". */
  int nmpc_hip_gmres_kernel_name(nmpc_hip_gmres_handle h, const char ** name);
  /** Device time of the last solve [ms] (HIP events around its launches; after solve_device: once it has finished). */
  int nmpc_hip_gmres_last_ms(nmpc_hip_gmres_handle h, float * ms);
  /** Text of the last error raised on this thread. */
  const char * nmpc_hip_gmres_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* NMPC_HIP_GMRES_H */
