// Device kernel of the batched FMPC iteration on caller-supplied linearisations (include/nmpc_hip_fmpc_step.h): one
// FmpcSolver::procOnce of the reference (FmpcSolver.hpp:365-493, with calcKktError :496-521, backwardPass :524-665, forwardPass
// :668-708 and updateVariables :713-831 without the line search) for B independent instances of run-time size (n, m, g, T).  fp64
// only, no FMA contraction.
//
//   fmpc_step_wave_kernel   one wavefront (one 64-thread workgroup) per instance.
//
//   Residuals, barrier sums, KKT error, ds / dnu, step lengths and the update are parallel over (step, component), strided over the
//   wave, and reduced by butterflies.
//
//   Backward sweep: the matrices of a step are 16-row tiles in LDS with leading dimension 17; a tile holds as many columns as the
//   handle's n (or m) asks for and C, D take one tile per 16 inequality rows, so the LDS request follows the shape (ldsBytes).  The
//   triple products (A'PA, A'PB, B'PB; C'SC, C'SD, D'SD with S = diag(nu / s), contraction up to 32; K'GK) run on
//   v_mfma_f64_16x16x4_f64 with the contraction index and the stored rows and columns masked by n and the step's m_i, g_i.  The
//   pivoted LDLT of G is cooperative (lane l owns row l; the pivot search is a wave argmax in which the lowest index wins a tie); the
//   n columns of K and the column of k are solved one per lane, in place in LDS.  The full-pivot LU fallback is a wave-uniform
//   branch that lane 0 runs serially; it is reached only after an exactly zero pivot.
//
//   Forward sweep: lane r owns row r of dlambda, du and dx+.  P, K, A, B of a step are staged in LDS from registers that were
//   requested one step ahead.
//
// Memory traffic: the record of the next step is requested into registers right after the current one has been staged.  What a step
// stores (the gains of the backward sweep, the delta of the forward sweep) is issued at the top of the NEXT step together with that
// step's loads: a wave with a store in flight can only wait for everything, so stores and loads share one wait.
//
// Ordering: the lanes of the one wavefront hand data to each other through LDS and, between the phases, through HBM (the residuals,
// the gains, the delta).  A wavefront's memory instructions are issued in order and performed in order at its CU's vector cache, so a
// compiler fence between the phases is all that is needed.  P and K are, in addition, read back by the lane that
// stored them.
//
// Statement order follows the reference; sums are ordered as the lanes need them: MFMA accumulation (k ascending in groups of four)
// and butterflies in the reductions over the horizon.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace nmpc_amd
{
namespace hip
{
namespace fmpc_step
{
constexpr int kMaxDim = 16;
constexpr int kMaxIneq = 32;
constexpr int kLd = 17; // leading dimension of every tile
constexpr int kWave = 64;
constexpr int kNTiles = 8; // tiles with n columns, without those of C
constexpr int kMTiles = 5; // tiles with m columns, without those of D
constexpr int kNVecs = 6;
constexpr int kMVecs = 6;
constexpr int kGVecs = 3;

// FmpcSolver::Status (FmpcSolver.h:92-114)
constexpr int kSucceeded = 1;
constexpr int kErrorInForward = 2;
constexpr int kErrorInBackward = 3;
constexpr int kErrorInUpdate = 4;
constexpr int kIterationContinued = 6;

typedef double v4d __attribute__((ext_vector_type(4)));

/** The handle's sizes and nmpc_hip_fmpc_step_config as the kernel reads them. */
struct Params
{
  int n, m, g, T; // m, g: the handle's capacities
  int row_major;
  int check_nan;
  int init_complementary_variable;
  int update_barrier_eps;
  int break_if_llt_fails;
  int apply_update;
  int total_ineq_dim; // sum of the steps' inequality dimensions
  size_t B;
  double dt;
  double kkt_error_thre;
};

/** Inputs, the variable and the outputs in the boundary layout (nmpc_hip_fmpc_step.h). */
struct Buffers
{
  const double *A, *Bm, *C, *D, *Lx, *Lu, *Lxx, *Luu, *Lxu, *f, *gv; // [B][T][block]
  const double *LxT, *LxxT, *cur_x; // [B][block]
  const int *mdims, *gdims; // [T] or null
  double *x, *u, *lam, *s, *nu, *eps; // the variable: read, and written by the update
  double * out_d; // the real results and the residual workspace, placed by OutputLayout
  int * out_i; // status
};

/** Where the results are in the handle's result allocation (offsets in elements), from the shape alone. */
struct OutputLayout
{
  size_t kkt, alpha_s, alpha_nu, k, K, gs, P, dx, du, dlam, ds, dnu;
  size_t xbar, gbar, lxbar, lubar; // workspace: the residuals of (2.23c), (2.23d), (2.25b) with the terminal (2.25a), (2.25c)
  size_t doubles;
  __host__ __device__ OutputLayout(size_t B, size_t T, size_t n, size_t m, size_t g)
  {
    kkt = 0;
    alpha_s = kkt + B;
    alpha_nu = alpha_s + B;
    k = alpha_nu + B;
    K = k + B * T * m;
    gs = K + B * T * m * n;
    P = gs + B * (T + 1) * n;
    dx = P + B * (T + 1) * n * n;
    du = dx + B * (T + 1) * n;
    dlam = du + B * T * m;
    ds = dlam + B * (T + 1) * n;
    dnu = ds + B * T * g;
    xbar = dnu + B * T * g;
    gbar = xbar + B * T * n;
    lxbar = gbar + B * T * g;
    lubar = lxbar + B * (T + 1) * n;
    doubles = lubar + B * T * m;
  }
};

__host__ __device__ constexpr int ineqTiles(int g)
{
  return (g + 15) / 16;
}

/** Dynamic LDS of one workgroup [bytes]: the tiles of n and of m columns (C, S C and D, S D take one tile each per 16 inequality
    rows), the vectors, and 16 doubles of integers (the transpositions of the LDLT and the column permutation of the LU). */
__host__ __device__ constexpr size_t ldsBytes(int n, int m, int g)
{
  return static_cast<size_t>((kNTiles + 2 * ineqTiles(g)) * kLd * n + (kMTiles + 2 * ineqTiles(g)) * kLd * m + kNVecs * n + kMVecs * m
                             + kGVecs * g + 16)
         * sizeof(double);
}
static_assert(ldsBytes(kMaxDim, kMaxDim, kMaxIneq) < 64 * 1024, "fmpc_step_wave_kernel: the largest shape must fit 64 KB of LDS");

__device__ __forceinline__ double bcastLane(double v, int lane)
{
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
  return __hiloint2double(hi, lo);
}

/** Sum over the 64 lanes by a butterfly; every lane gets the same bits. */
__device__ __forceinline__ double waveSum(double v)
{
#pragma unroll
  for(int s = 32; s >= 1; s >>= 1)
  {
    v += __shfl_xor(v, s, 64);
  }
  return bcastLane(v, 0);
}

/** std::min over the 64 lanes by a butterfly. */
__device__ __forceinline__ double waveMin(double v)
{
#pragma unroll
  for(int s = 32; s >= 1; s >>= 1)
  {
    const double o = __shfl_xor(v, s, 64);
    v = (o < v) ? o : v;
  }
  return bcastLane(v, 0);
}

/** A compiler fence: see "Ordering" at the top of the file. */
__device__ __forceinline__ void fence()
{
  asm volatile("" ::: "memory");
}

__device__ __forceinline__ bool notFinite(double v)
{
  return !(fabs(v) <= 1.7976931348623157e308); // NaN or Inf
}

/** The record of one step of the backward sweep in registers, as the loads return it: entry (r = lane % 16, c = 4 q + lane / 16)
    of each block; C and D one tile per 16 rows. */
struct Record
{
  double a[4], b[4], lxx[4], lxu[4], luu[4];
  double c0[4], c1[4], d0[4], d1[4];
  double xbar, lxbar, lubar, gbar, s, nu;
};

/** The record of one step of the forward sweep. */
struct FwdRecord
{
  double P[4], K[4], a[4], b[4];
  double gs, k, xbar;
};

struct Wave
{
  const Buffers & bf;
  const Params & p;
  double * lds;
  const size_t b;
  mutable int lane, lj, lk;
  int n, mc, gc; // state dimension, input capacity, inequality capacity

  /** Hides where the lane indices come from, so that an address is computed where it is used and not kept in a register over the
      step loop (riccati_kernels.hpp has the figures).  The dimensions are left alone here: they sit in scalar registers. */
  __device__ __forceinline__ void launder() const
  {
    asm volatile("" : "+v"(lane), "+v"(lj), "+v"(lk));
  }

  // tiles of n columns
  enum
  {
    tA,
    tP,
    tPA, // P A
    tF, // dt Lxx, then Qxx_tilde, then F
    tK, // m x n
    tHt, // m x n: H^T
    tGK, // m x n: G K
    tPn, // the new P before it is symmetrised
    tC // g x n, one tile per 16 rows; then S C likewise
  };
  // tiles of m columns
  enum
  {
    uB, // n x m
    uPB, // n x m
    uG,
    uL, // the LDLT of G
    uLU, // the LU of G
    uD // g x m, one tile per 16 rows; then S D likewise
  };
  enum
  {
    vXbar,
    vLxbar,
    vLxt, // Lx_tilde
    vS, // s of the recursion
    vV, // P x_bar - s
    vDx
  };
  enum
  {
    vLubar,
    vLut, // Lu_tilde
    vKff,
    vRhs,
    vDu,
    vY // the LU's back substitution
  };
  enum
  {
    vGbar,
    vNus, // nu / s
    vTsub // tilde_sub
  };

  __device__ __forceinline__ int gt() const
  {
    return ineqTiles(gc);
  }
  __device__ __forceinline__ double * nTile(int t) const
  {
    return lds + t * (kLd * n);
  }
  __device__ __forceinline__ double * cTile(int jt) const
  {
    return nTile(tC + jt);
  }
  __device__ __forceinline__ double * scTile(int jt) const
  {
    return nTile(tC + gt() + jt);
  }
  __device__ __forceinline__ double * mBase() const
  {
    return lds + (kNTiles + 2 * gt()) * (kLd * n);
  }
  __device__ __forceinline__ double * mTile(int u) const
  {
    return mBase() + u * (kLd * mc);
  }
  __device__ __forceinline__ double * dTile(int jt) const
  {
    return mTile(uD + jt);
  }
  __device__ __forceinline__ double * sdTile(int jt) const
  {
    return mTile(uD + gt() + jt);
  }
  __device__ __forceinline__ double * vBase() const
  {
    return mBase() + (kMTiles + 2 * gt()) * (kLd * mc);
  }
  __device__ __forceinline__ double * nVec(int v) const
  {
    return vBase() + v * n;
  }
  __device__ __forceinline__ double * mVec(int v) const
  {
    return vBase() + kNVecs * n + v * mc;
  }
  __device__ __forceinline__ double * gVec(int v) const
  {
    return vBase() + kNVecs * n + kMVecs * mc + v * gc;
  }
  __device__ __forceinline__ int * ints() const // [0, 16): transpositions, [16, 32): column permutation
  {
    return reinterpret_cast<int *>(vBase() + kNVecs * n + kMVecs * mc + kGVecs * gc);
  }
  __device__ __forceinline__ int mAt(int i) const
  {
    return bf.mdims ? bf.mdims[i] : mc;
  }
  __device__ __forceinline__ int gAt(int i) const
  {
    return bf.gdims ? bf.gdims[i] : gc;
  }
  /** Index of entry (r, c) of a rows_cap x cols_cap block at the boundary. */
  __device__ __forceinline__ int at(int r, int c, int rows_cap, int cols_cap) const
  {
    return p.row_major ? r * cols_cap + c : r + rows_cap * c;
  }

  // ===================================================================================================
  // matrix products
  // ===================================================================================================
  /** acc + op(A) * Bm over k < kdim in the MFMA D layout: acc[r] = D(i = lane / 16 + 4 r, j = lane % 16); op(A) = A^T with kTransA.
      D has rows_d rows and cols_d columns; operands outside them (and k >= kdim) are fed as zeros from an in-bounds address. */
  template<bool kTransA>
  __device__ __forceinline__ v4d mma(v4d acc, const double * A, const double * Bm, int rows_d, int kdim, int cols_d) const
  {
    for(int k0 = 0; k0 < kdim; k0 += 4)
    {
      const int k = k0 + lk;
      const bool av = k < kdim && lj < rows_d;
      const bool bv = k < kdim && lj < cols_d;
      const double a = A[av ? (kTransA ? k + kLd * lj : lj + kLd * k) : 0];
      const double bb = Bm[bv ? k + kLd * lj : 0];
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av ? a : 0.0, bv ? bb : 0.0, acc, 0, 0, 0);
    }
    return acc;
  }
  __device__ __forceinline__ void store(double * dst, v4d acc, int rows, int cols) const
  {
#pragma unroll
    for(int r = 0; r < 4; r++)
    {
      const int i = lk + 4 * r;
      if(i < rows && lj < cols)
      {
        dst[i + kLd * lj] = acc[r];
      }
    }
  }
  /** rows x cols of dst <- (dst + acc1) + acc2. */
  __device__ __forceinline__ void storeSum2(double * dst, v4d acc1, v4d acc2, int rows, int cols) const
  {
#pragma unroll
    for(int r = 0; r < 4; r++)
    {
      const int i = lk + 4 * r;
      if(i < rows && lj < cols)
      {
        dst[i + kLd * lj] = (dst[i + kLd * lj] + acc1[r]) + acc2[r];
      }
    }
  }

  // ===================================================================================================
  // Eigen::LDLT, its solve, and the full-pivot LU
  // ===================================================================================================
  /** In-place LDLT of the m x m matrix in tile uL with symmetric pivoting on the largest |diagonal| (the first index wins a tie),
      lower triangle only; lane l owns row l.  false where Eigen's info() is NumericalIssue. */
  __device__ __forceinline__ bool ldlt(int m) const
  {
    double * L = mTile(uL);
    int * tr = ints();
    const int l = lane;
    if(m <= 1)
    {
      if(l == 0)
      {
        tr[0] = 0;
      }
      fence();
      return true;
    }
    bool ret = true, found_zero_pivot = false;
    for(int k = 0; k < m; k++)
    {
      fence();
      // the largest |diagonal| of the remaining block; a NaN wins only where the serial scan starts from it
      double v = -1.0;
      if(l >= k && l < m)
      {
        const double d = fabs(L[l + kLd * l]);
        v = (d != d) ? ((l == k) ? __builtin_huge_val() : -1.0) : d;
      }
      int idx = l;
#pragma unroll
      for(int s = 8; s >= 1; s >>= 1)
      {
        const double ov = __shfl_xor(v, s, 64);
        const int oi = __shfl_xor(idx, s, 64);
        if(ov > v || (ov == v && oi < idx))
        {
          v = ov;
          idx = oi;
        }
      }
      const int pv = __builtin_amdgcn_readlane(idx, 0);
      if(l == 0)
      {
        tr[k] = pv;
      }
      if(pv != k && l < m) // symmetric swap of rows / columns k and pv
      {
        int i0, i1;
        bool any = true;
        if(l < k)
        {
          i0 = k + kLd * l;
          i1 = pv + kLd * l;
        }
        else if(l == k)
        {
          i0 = k + kLd * k;
          i1 = pv + kLd * pv;
        }
        else if(l < pv)
        {
          i0 = l + kLd * k;
          i1 = pv + kLd * l;
        }
        else if(l > pv)
        {
          i0 = l + kLd * k;
          i1 = l + kLd * pv;
        }
        else
        {
          i0 = i1 = 0;
          any = false;
        }
        if(any)
        {
          const double t0 = L[i0], t1 = L[i1];
          L[i0] = t1;
          L[i1] = t0;
        }
      }
      fence();
      if(k > 0 && l >= k && l < m)
      {
        double s = 0;
        for(int j = 0; j < k; j++)
        {
          s += L[l + kLd * j] * (L[j + kLd * j] * L[k + kLd * j]);
        }
        L[l + kLd * k] -= s;
      }
      fence();
      const double akk = bcastLane(L[k + kLd * k], 0); // the same in every lane: the branches below are wave-uniform
      const bool pivot_is_valid = fabs(akk) > 0.0;
      if(k == 0 && !pivot_is_valid)
      {
        // the entire diagonal is zero: success iff the strictly lower part is zero too
        bool nz = false;
        if(l < m)
        {
          tr[l] = l;
          for(int j = 0; j < l; j++)
          {
            nz = nz || !(L[l + kLd * j] == 0.0);
          }
        }
        fence();
        return __ballot(nz) == 0;
      }
      const bool below = l > k && l < m;
      if(pivot_is_valid)
      {
        if(below)
        {
          L[l + kLd * k] /= akk;
        }
      }
      else if(__ballot(below && !(L[l + kLd * k] == 0.0)) != 0)
      {
        ret = false;
      }
      if(found_zero_pivot && pivot_is_valid)
      {
        ret = false;
      }
      else if(!pivot_is_valid)
      {
        found_zero_pivot = true;
      }
    }
    fence();
    return ret;
  }

  /** x <- -G^-1 x through the LDLT in tile uL, in the order of Eigen's solve (D's pseudo-inverse); one lane, in place in LDS. */
  __device__ __forceinline__ void ldltSolveColumn(double * x, int m) const
  {
    const double * L = mTile(uL);
    const int * tr = ints();
    for(int k = 0; k < m; k++)
    {
      const int t = tr[k];
      const double a = x[k], c = x[t];
      x[k] = c;
      x[t] = a;
    }
    for(int i = 0; i < m; i++)
    {
      double s = x[i];
      for(int j = 0; j < i; j++)
      {
        s -= L[i + kLd * j] * x[j];
      }
      x[i] = s;
    }
    for(int i = 0; i < m; i++)
    {
      const double d = L[i + kLd * i];
      x[i] = (fabs(d) > 2.2250738585072014e-308) ? x[i] / d : 0.0;
    }
    for(int i = m - 1; i >= 0; i--)
    {
      double s = x[i];
      for(int j = i + 1; j < m; j++)
      {
        s -= L[j + kLd * i] * x[j];
      }
      x[i] = s;
    }
    for(int k = m - 1; k >= 0; k--)
    {
      const int t = tr[k];
      const double a = x[k], c = x[t];
      x[k] = c;
      x[t] = a;
    }
    for(int i = 0; i < m; i++)
    {
      x[i] = -1 * x[i];
    }
  }

  /** b <- -G^-1 b for c right-hand sides (column q at b + ld q) by full-pivot Gaussian elimination of tile uG in tile uLU;
      rank-deficient directions get 0.  Serial: the calling lane does everything. */
  __device__ __forceinline__ void luSolve(double * bb, int ld, int c, int m) const
  {
    double * a = mTile(uLU);
    const double * G = mTile(uG);
    int * colperm = ints() + 16;
    double * y = mVec(vY);
    for(int j = 0; j < m; j++)
    {
      colperm[j] = j;
      for(int i = 0; i < m; i++)
      {
        a[i + kLd * j] = G[i + kLd * j];
      }
    }
    int rank = 0;
    for(int k = 0; k < m; k++)
    {
      int pr = k, pc = k;
      double big = 0;
      for(int j = k; j < m; j++)
      {
        for(int i = k; i < m; i++)
        {
          if(fabs(a[i + kLd * j]) > big)
          {
            big = fabs(a[i + kLd * j]);
            pr = i;
            pc = j;
          }
        }
      }
      if(big == 0.0)
      {
        break;
      }
      rank++;
      for(int j = 0; j < m; j++)
      {
        const double t0 = a[k + kLd * j], t1 = a[pr + kLd * j];
        a[k + kLd * j] = t1;
        a[pr + kLd * j] = t0;
      }
      for(int q = 0; q < c; q++)
      {
        const double t0 = bb[k + ld * q], t1 = bb[pr + ld * q];
        bb[k + ld * q] = t1;
        bb[pr + ld * q] = t0;
      }
      for(int i = 0; i < m; i++)
      {
        const double t0 = a[i + kLd * k], t1 = a[i + kLd * pc];
        a[i + kLd * k] = t1;
        a[i + kLd * pc] = t0;
      }
      {
        const int t0 = colperm[k], t1 = colperm[pc];
        colperm[k] = t1;
        colperm[pc] = t0;
      }
      for(int i = k + 1; i < m; i++)
      {
        const double f = a[i + kLd * k] / a[k + kLd * k];
        for(int j = k + 1; j < m; j++)
        {
          a[i + kLd * j] -= f * a[k + kLd * j];
        }
        for(int q = 0; q < c; q++)
        {
          bb[i + ld * q] -= f * bb[k + ld * q];
        }
      }
    }
    for(int q = 0; q < c; q++)
    {
      for(int i = m - 1; i >= 0; i--)
      {
        if(i >= rank)
        {
          y[i] = 0;
          continue;
        }
        double s = bb[i + ld * q];
        for(int j = i + 1; j < rank; j++)
        {
          s -= a[i + kLd * j] * y[j];
        }
        y[i] = s / a[i + kLd * i];
      }
      for(int i = 0; i < m; i++)
      {
        bb[colperm[i] + ld * q] = -1 * y[i];
      }
    }
  }

  // ===================================================================================================
  // the phases over (step, component)
  // ===================================================================================================
  /** s, nu <- the initial complementarity variables    FmpcSolver.hpp:172-188 */
  __device__ __forceinline__ void initComplementary() const
  {
    const int T = p.T;
    for(int idx = lane; idx < T * gc; idx += kWave)
    {
      const int i = idx / gc, j = idx - i * gc;
      if(j < gAt(i))
      {
        const size_t e = (b * T + i) * gc + j;
        const double a = -1 * bf.gv[e];
        const double s = (1.0 + 1e-2) * ((a < 1e-2) ? 1e-2 : a);
        const double c = 1e-4 * (1.0 / s);
        bf.s[e] = s;
        bf.nu[e] = (1.0 + 1e-2) * ((c < 1e-2) ? 1e-2 : c);
      }
    }
    fence();
  }

  /** barrier_eps by (19.19)    :378-399 */
  __device__ __forceinline__ double barrierEps() const
  {
    const int T = p.T;
    double acc = 0;
    for(int idx = lane; idx < T * gc; idx += kWave)
    {
      const int i = idx / gc, j = idx - i * gc;
      if(j < gAt(i))
      {
        const size_t e = (b * T + i) * gc + j;
        acc += bf.s[e] * bf.nu[e];
      }
    }
    double s_nu_ave = waveSum(acc);
    s_nu_ave /= p.total_ineq_dim;
    const double v = 0.5 * s_nu_ave;
    return (v < 1e-8) ? 1e-8 : ((1e6 < v) ? 1e6 : v); // std::clamp
  }

  /** The residuals into the workspace, and calcKktError(0.0)    :422-434, :496-521 */
  __device__ __forceinline__ double residuals() const
  {
    const int T = p.T;
    const OutputLayout o(p.B, T, n, mc, gc);
    const double dt = p.dt;
    double acc = 0;
    for(int idx = lane; idx < T * n; idx += kWave)
    {
      const int i = idx / n, r = idx - i * n;
      const size_t st = b * T + i;
      const int gi = gAt(i);
      const double * lamn = bf.lam + (b * (T + 1) + i + 1) * n;
      const double xbar = bf.f[st * n + r] - bf.x[(b * (T + 1) + i + 1) * n + r];
      const double * A = bf.A + st * (n * n);
      double s1 = 0;
      for(int k = 0; k < n; k++)
      {
        s1 += A[at(k, r, n, n)] * lamn[k];
      }
      double s2 = 0;
      for(int j = 0; j < gi; j++)
      {
        s2 += bf.C[st * (gc * n) + at(j, r, gc, n)] * bf.nu[st * gc + j];
      }
      const double lxbar = ((-1 * bf.lam[(b * (T + 1) + i) * n + r] + dt * bf.Lx[st * n + r]) + s1) + s2;
      bf.out_d[o.xbar + st * n + r] = xbar;
      bf.out_d[o.lxbar + (b * (T + 1) + i) * n + r] = lxbar;
      acc += xbar * xbar + lxbar * lxbar;
    }
    for(int idx = lane; idx < T * mc; idx += kWave)
    {
      const int i = idx / mc, r = idx - i * mc;
      const size_t st = b * T + i;
      const int gi = gAt(i);
      double lubar = 0;
      if(r < mAt(i))
      {
        const double * lamn = bf.lam + (b * (T + 1) + i + 1) * n;
        double s1 = 0;
        for(int k = 0; k < n; k++)
        {
          s1 += bf.Bm[st * (n * mc) + at(k, r, n, mc)] * lamn[k];
        }
        double s2 = 0;
        for(int j = 0; j < gi; j++)
        {
          s2 += bf.D[st * (gc * mc) + at(j, r, gc, mc)] * bf.nu[st * gc + j];
        }
        lubar = (dt * bf.Lu[st * mc + r] + s1) + s2;
      }
      bf.out_d[o.lubar + st * mc + r] = lubar;
      acc += lubar * lubar;
    }
    for(int idx = lane; idx < T * gc; idx += kWave)
    {
      const int i = idx / gc, j = idx - i * gc;
      const size_t e = (b * T + i) * gc + j;
      double gbar = 0;
      if(j < gAt(i))
      {
        const double s = bf.s[e], nu = bf.nu[e];
        gbar = bf.gv[e] + s;
        const double comp = s * nu - 0.0;
        const double cpos = (comp < 0) ? 0.0 : comp;
        acc += cpos * cpos;
      }
      bf.out_d[o.gbar + e] = gbar;
      acc += gbar * gbar;
    }
    if(lane < n)
    {
      const double lxbarT = bf.LxT[b * n + lane] - bf.lam[(b * (T + 1) + T) * n + lane];
      bf.out_d[o.lxbar + (b * (T + 1) + T) * n + lane] = lxbarT;
      const double e0 = bf.cur_x[b * n + lane] - bf.x[b * (T + 1) * n + lane];
      acc += lxbarT * lxbarT + e0 * e0;
    }
    fence();
    return sqrt(waveSum(acc));
  }

  // ===================================================================================================
  // backwardPass    :524-665
  // ===================================================================================================
  __device__ __forceinline__ void loadRecord(Record & rec, int i, int m, int gi) const
  {
    const int T = p.T;
    const size_t st = b * T + i;
    const OutputLayout o(p.B, T, n, mc, gc);
    const double * A = bf.A + st * (n * n);
    const double * Lxx = bf.Lxx + st * (n * n);
    const double * Bm = bf.Bm + st * (n * mc);
    const double * Lxu = bf.Lxu + st * (n * mc);
    const double * Luu = bf.Luu + st * (mc * mc);
    const double * Cm = bf.C + st * (gc * n);
    const double * Dm = bf.D + st * (gc * mc);
#pragma unroll
    for(int q = 0; q < 4; q++)
    {
      const int c = 4 * q + lk;
      rec.a[q] = rec.lxx[q] = rec.b[q] = rec.lxu[q] = rec.luu[q] = 0.0;
      if(lj < n && c < n)
      {
        rec.a[q] = A[at(lj, c, n, n)];
        rec.lxx[q] = Lxx[at(lj, c, n, n)];
      }
      if(lj < n && c < m)
      {
        rec.b[q] = Bm[at(lj, c, n, mc)];
        rec.lxu[q] = Lxu[at(lj, c, n, mc)];
      }
      if(lj < m && c < m)
      {
        rec.luu[q] = Luu[at(lj, c, mc, mc)];
      }
      auto tile = [&](int jt, double & cv, double & dv) {
        const int row = 16 * jt + lj;
        cv = dv = 0.0;
        if(row < gi && c < n)
        {
          cv = Cm[at(row, c, gc, n)];
        }
        if(row < gi && c < m)
        {
          dv = Dm[at(row, c, gc, mc)];
        }
      };
      tile(0, rec.c0[q], rec.d0[q]);
      tile(1, rec.c1[q], rec.d1[q]);
    }
    rec.xbar = rec.lxbar = rec.lubar = rec.gbar = rec.s = rec.nu = 0.0;
    if(lane < n)
    {
      rec.xbar = bf.out_d[o.xbar + st * n + lane];
      rec.lxbar = bf.out_d[o.lxbar + (b * (T + 1) + i) * n + lane];
    }
    if(lane < m)
    {
      rec.lubar = bf.out_d[o.lubar + st * mc + lane];
    }
    if(lane < gi)
    {
      rec.gbar = bf.out_d[o.gbar + st * gc + lane];
      rec.s = bf.s[st * gc + lane];
      rec.nu = bf.nu[st * gc + lane];
    }
  }

  /** The record into LDS: A, B, C, D, the dt-weighted cost blocks where the products are added to them, S C and S D, the residuals,
      nu / s and tilde_sub.  true where an entry is NaN or Inf. */
  __device__ __forceinline__ bool stageRecord(const Record & rec, int m, int gi, double eps) const
  {
    bool bad = false;
    const double dt = p.dt;
    double nus = 0;
    if(lane < n)
    {
      nVec(vXbar)[lane] = rec.xbar;
      nVec(vLxbar)[lane] = rec.lxbar;
      bad = bad || notFinite(rec.xbar) || notFinite(rec.lxbar);
    }
    if(lane < m)
    {
      mVec(vLubar)[lane] = rec.lubar;
      bad = bad || notFinite(rec.lubar);
    }
    if(lane < gi)
    {
      nus = rec.nu / rec.s;
      gVec(vGbar)[lane] = rec.gbar;
      gVec(vNus)[lane] = nus;
      gVec(vTsub)[lane] = (nus * rec.gbar - rec.nu) + eps * (1.0 / rec.s);
      bad = bad || notFinite(rec.gbar);
    }
#pragma unroll
    for(int q = 0; q < 4; q++)
    {
      const int c = 4 * q + lk;
      if(lj < n && c < n)
      {
        nTile(tA)[lj + kLd * c] = rec.a[q];
        nTile(tF)[lj + kLd * c] = dt * rec.lxx[q];
        bad = bad || notFinite(rec.a[q]) || notFinite(rec.lxx[q]);
      }
      if(lj < n && c < m)
      {
        mTile(uB)[lj + kLd * c] = rec.b[q];
        nTile(tHt)[c + kLd * lj] = dt * rec.lxu[q]; // H^T(c, lj) starts as dt Lxu(lj, c)
        bad = bad || notFinite(rec.b[q]) || notFinite(rec.lxu[q]);
      }
      if(lj < m && c < m)
      {
        mTile(uG)[lj + kLd * c] = dt * rec.luu[q];
        bad = bad || notFinite(rec.luu[q]);
      }
      auto tile = [&](int jt, double cv, double dv) {
        const int row = 16 * jt + lj;
        const double w = bcastLaneVar(nus, row);
        if(row < gi && c < n)
        {
          cTile(jt)[lj + kLd * c] = cv;
          scTile(jt)[lj + kLd * c] = w * cv;
          bad = bad || notFinite(cv);
        }
        if(row < gi && c < m)
        {
          dTile(jt)[lj + kLd * c] = dv;
          sdTile(jt)[lj + kLd * c] = w * dv;
          bad = bad || notFinite(dv);
        }
      };
      tile(0, rec.c0[q], rec.d0[q]);
      tile(1, rec.c1[q], rec.d1[q]);
    }
    return bad;
  }

  /** v of lane `src` (src < 64, different per lane). */
  __device__ __forceinline__ double bcastLaneVar(double v, int src) const
  {
    return __shfl(v, src & 63, 64);
  }

  /** s and P of step i (and k, K where has_gain) from LDS to HBM; gains beyond the step's input dimension are written as 0.  true
      where a value is NaN or Inf. */
  __device__ __forceinline__ bool flushGains(int i, int m, bool has_gain) const
  {
    const int T = p.T;
    const OutputLayout o(p.B, T, n, mc, gc);
    bool bad = false;
    if(lane < n)
    {
      const double v = nVec(vS)[lane];
      bf.out_d[o.gs + (b * (T + 1) + i) * n + lane] = v;
      bad = bad || notFinite(v);
    }
    double * Po = bf.out_d + o.P + (b * (T + 1) + i) * (n * n);
    double * Ko = bf.out_d + o.K + (b * T + i) * (mc * n);
#pragma unroll
    for(int q = 0; q < 4; q++)
    {
      const int c = 4 * q + lk;
      if(lj < n && c < n)
      {
        const double v = nTile(tP)[lj + kLd * c];
        Po[at(lj, c, n, n)] = v;
        bad = bad || notFinite(v);
      }
      if(has_gain && lj < mc && c < n)
      {
        const double v = (lj < m) ? nTile(tK)[lj + kLd * c] : 0.0;
        Ko[at(lj, c, mc, n)] = v;
        bad = bad || notFinite(v);
      }
    }
    if(has_gain && lane < mc)
    {
      const double v = (lane < m) ? mVec(vKff)[lane] : 0.0;
      bf.out_d[o.k + (b * T + i) * mc + lane] = v;
      bad = bad || notFinite(v);
    }
    return bad;
  }

  /** 0: done; kErrorInBackward otherwise. */
  __device__ __forceinline__ int backwardPass(double eps) const
  {
    const int T = p.T;
    bool bad = false;
    // s = -Lx_bar_T, P = Lxx_T    (2.34)
    {
      const OutputLayout o(p.B, T, n, mc, gc);
      const double * V = bf.LxxT + b * (n * n);
#pragma unroll
      for(int q = 0; q < 4; q++)
      {
        const int c = 4 * q + lk;
        if(lj < n && c < n)
        {
          nTile(tP)[lj + kLd * c] = V[at(lj, c, n, n)];
        }
      }
      if(lane < n)
      {
        nVec(vS)[lane] = -1 * bf.out_d[o.lxbar + (b * (T + 1) + T) * n + lane];
        bad = bad || notFinite(bf.LxT[b * n + lane]);
      }
    }
    Record rec;
    int m = mAt(T - 1), gi = gAt(T - 1);
    loadRecord(rec, T - 1, m, gi);
    int m_prev = 0; // input dimension of step i + 1, whose gains are still in LDS
    for(int i = T - 1; i >= 0; i--)
    {
      launder();
      fence();
      bad = stageRecord(rec, m, gi, eps) || bad;
      fence();
      bad = flushGains(i + 1, m_prev, i + 1 < T) || bad;
      const int m_next = (i > 0) ? mAt(i - 1) : 0;
      const int g_next = (i > 0) ? gAt(i - 1) : 0;
      if(i > 0)
      {
        loadRecord(rec, i - 1, m_next, g_next);
      }

      launder();
      const v4d zero = {0, 0, 0, 0};
      const int g0 = (gi < 16) ? gi : 16, g1 = gi - 16; // rows of the two inequality tiles
      // ---- pre-process    :568-586
      store(nTile(tPA), mma<false>(zero, nTile(tP), nTile(tA), n, n, n), n, n);
      if(m > 0)
      {
        store(mTile(uPB), mma<false>(zero, nTile(tP), mTile(uB), n, n, m), n, m);
      }
      if(lane < n)
      {
        double s = 0;
        for(int k = 0; k < n; k++)
        {
          s += nTile(tP)[lane + kLd * k] * nVec(vXbar)[k];
        }
        nVec(vV)[lane] = s - nVec(vS)[lane]; // P x_bar - s
        double t = 0;
        for(int j = 0; j < gi; j++)
        {
          t += cTile(j >> 4)[(j & 15) + kLd * lane] * gVec(vTsub)[j];
        }
        nVec(vLxt)[lane] = nVec(vLxbar)[lane] + t; // (2.28f)
      }
      if(lane < m)
      {
        double t = 0;
        for(int j = 0; j < gi; j++)
        {
          t += dTile(j >> 4)[(j & 15) + kLd * lane] * gVec(vTsub)[j];
        }
        mVec(vLut)[lane] = mVec(vLubar)[lane] + t; // (2.28g)
      }
      fence();
      {
        v4d qc = zero; // C' S C    (2.28c)
        if(gi > 0)
        {
          qc = mma<true>(qc, cTile(0), scTile(0), n, g0, n);
        }
        if(g1 > 0)
        {
          qc = mma<true>(qc, cTile(1), scTile(1), n, g1, n);
        }
        storeSum2(nTile(tF), qc, mma<true>(zero, nTile(tA), nTile(tPA), n, n, n), n, n); // (2.35b)
      }
      if(m > 0)
      {
        v4d hc = zero, gcc = zero; // D' S C (the transpose of (2.28d)), D' S D (2.28e)
        if(gi > 0)
        {
          hc = mma<true>(hc, dTile(0), scTile(0), m, g0, n);
          gcc = mma<true>(gcc, dTile(0), sdTile(0), m, g0, m);
        }
        if(g1 > 0)
        {
          hc = mma<true>(hc, dTile(1), scTile(1), m, g1, n);
          gcc = mma<true>(gcc, dTile(1), sdTile(1), m, g1, m);
        }
        storeSum2(nTile(tHt), hc, mma<true>(zero, mTile(uB), nTile(tPA), m, n, n), m, n); // (2.35c), transposed
        storeSum2(mTile(uG), gcc, mma<true>(zero, mTile(uB), mTile(uPB), m, n, m), m, m); // (2.35d)
        if(lane < m)
        {
          double s = 0;
          for(int k = 0; k < n; k++)
          {
            s += mTile(uB)[k + kLd * lane] * nVec(vV)[k];
          }
          mVec(vRhs)[lane] = s + mVec(vLut)[lane];
        }
      }
      fence();

      launder();
      // ---- gains    :588-627
      if(m > 0)
      {
#pragma unroll
        for(int q = 0; q < 4; q++)
        {
          const int c = 4 * q + lk;
          if(lj < m && c < m)
          {
            mTile(uL)[lj + kLd * c] = mTile(uG)[lj + kLd * c];
          }
          if(lj < m && c < n)
          {
            nTile(tK)[lj + kLd * c] = nTile(tHt)[lj + kLd * c];
          }
        }
        if(lane < m)
        {
          mVec(vKff)[lane] = mVec(vRhs)[lane];
        }
        fence();
        if(ldlt(m))
        {
          if(lane < n)
          {
            ldltSolveColumn(nTile(tK) + kLd * lane, m);
          }
          else if(lane == n)
          {
            ldltSolveColumn(mVec(vKff), m);
          }
        }
        else if(p.break_if_llt_fails)
        {
          return kErrorInBackward;
        }
        else if(lane == 0)
        {
          luSolve(nTile(tK), kLd, n, m);
          luSolve(mVec(vKff), kLd, 1, m);
        }
        fence();
        store(nTile(tGK), mma<false>(zero, mTile(uG), nTile(tK), m, m, n), m, n);
      }
      // ---- post-process    :629-640
      if(lane < n)
      {
        double s1 = 0;
        for(int k = 0; k < n; k++)
        {
          s1 += nTile(tA)[k + kLd * lane] * (-1 * nVec(vV)[k]); // A' (s - P x_bar)
        }
        double s2 = 0;
        for(int a = 0; a < m; a++)
        {
          s2 += nTile(tHt)[a + kLd * lane] * mVec(vKff)[a];
        }
        const double t = s1 - nVec(vLxt)[lane];
        nVec(vS)[lane] = (m > 0) ? t - s2 : t;
      }
      fence();
      {
        v4d kgk = zero;
        if(m > 0)
        {
          kgk = mma<true>(kgk, nTile(tK), nTile(tGK), n, m, n);
        }
#pragma unroll
        for(int r = 0; r < 4; r++)
        {
          const int row = lk + 4 * r;
          if(row < n && lj < n)
          {
            const int e = row + kLd * lj;
            nTile(tPn)[e] = (m > 0) ? nTile(tF)[e] - kgk[r] : nTile(tF)[e];
          }
        }
      }
      fence();
#pragma unroll
      for(int q = 0; q < 4; q++)
      {
        const int c = 4 * q + lk;
        if(lj < n && c < n)
        {
          nTile(tP)[lj + kLd * c] = 0.5 * (nTile(tPn)[lj + kLd * c] + nTile(tPn)[c + kLd * lj]);
        }
      }
      fence();
      m_prev = m;
      m = m_next;
      gi = g_next;
    }
    bad = flushGains(0, m_prev, true) || bad;
    fence();
    if(p.check_nan && __ballot(bad) != 0)
    {
      return kErrorInBackward;
    }
    return 0;
  }

  // ===================================================================================================
  // forwardPass    :668-708
  // ===================================================================================================
  __device__ __forceinline__ void loadFwd(FwdRecord & rec, int i, int m) const
  {
    const int T = p.T;
    const OutputLayout o(p.B, T, n, mc, gc);
    const bool inner = i < T;
    const size_t st = b * T + (inner ? i : T - 1);
    const double * Po = bf.out_d + o.P + (b * (T + 1) + i) * (n * n);
    const double * Ko = bf.out_d + o.K + st * (mc * n);
    const double * A = bf.A + st * (n * n);
    const double * Bm = bf.Bm + st * (n * mc);
#pragma unroll
    for(int q = 0; q < 4; q++)
    {
      const int c = 4 * q + lk;
      rec.P[q] = rec.K[q] = rec.a[q] = rec.b[q] = 0.0;
      if(lj < n && c < n)
      {
        rec.P[q] = Po[at(lj, c, n, n)];
        if(inner)
        {
          rec.a[q] = A[at(lj, c, n, n)];
        }
      }
      if(inner && lj < m && c < n)
      {
        rec.K[q] = Ko[at(lj, c, mc, n)];
      }
      if(inner && lj < n && c < m)
      {
        rec.b[q] = Bm[at(lj, c, n, mc)];
      }
    }
    rec.gs = rec.k = rec.xbar = 0.0;
    if(lane < n)
    {
      rec.gs = bf.out_d[o.gs + (b * (T + 1) + i) * n + lane];
      if(inner)
      {
        rec.xbar = bf.out_d[o.xbar + st * n + lane];
      }
    }
    if(inner && lane < m)
    {
      rec.k = bf.out_d[o.k + st * mc + lane];
    }
  }

  /** 0: done; kErrorInForward otherwise. */
  __device__ __forceinline__ int forwardPass() const
  {
    const int T = p.T;
    const OutputLayout o(p.B, T, n, mc, gc);
    bool bad = false;
    double dx = 0; // row `lane` of delta x_i
    if(lane < n)
    {
      dx = bf.cur_x[b * n + lane] - bf.x[b * (T + 1) * n + lane];
    }
    FwdRecord rec;
    int m = mAt(0);
    loadFwd(rec, 0, m);
    double dlam_prev = 0, du_prev = 0; // of step i - 1, stored at the top of step i
    for(int i = 0; i <= T; i++)
    {
      launder();
      fence();
      const bool inner = i < T;
#pragma unroll
      for(int q = 0; q < 4; q++)
      {
        const int c = 4 * q + lk;
        if(lj < n && c < n)
        {
          nTile(tP)[lj + kLd * c] = rec.P[q];
          nTile(tA)[lj + kLd * c] = rec.a[q];
        }
        if(lj < m && c < n)
        {
          nTile(tK)[lj + kLd * c] = rec.K[q];
        }
        if(lj < n && c < m)
        {
          mTile(uB)[lj + kLd * c] = rec.b[q];
        }
      }
      if(lane < n)
      {
        nVec(vDx)[lane] = dx;
      }
      const double gs_i = rec.gs, k_i = rec.k, xbar_i = rec.xbar;
      fence();
      // the stores of step i - 1 and of delta x_i, together with the loads of step i + 1
      if(lane < n)
      {
        bf.out_d[o.dx + (b * (T + 1) + i) * n + lane] = dx;
        if(i > 0)
        {
          bf.out_d[o.dlam + (b * (T + 1) + i - 1) * n + lane] = dlam_prev;
        }
      }
      if(i > 0 && lane < mc)
      {
        bf.out_d[o.du + (b * T + i - 1) * mc + lane] = du_prev;
      }
      const int m_next = (i + 1 < T) ? mAt(i + 1) : 0;
      if(inner)
      {
        loadFwd(rec, i + 1, m_next);
      }

      launder();
      double dlam = 0, du = 0;
      if(lane < n)
      {
        double s = 0;
        for(int k = 0; k < n; k++)
        {
          s += nTile(tP)[lane + kLd * k] * nVec(vDx)[k];
        }
        dlam = s - gs_i; // (2.33)
      }
      if(inner && lane < m)
      {
        double s = 0;
        for(int k = 0; k < n; k++)
        {
          s += nTile(tK)[lane + kLd * k] * nVec(vDx)[k];
        }
        du = s + k_i; // (2.36)
        mVec(vDu)[lane] = du;
      }
      fence();
      bad = bad || notFinite(dx) || notFinite(dlam) || notFinite(du);
      if(inner && lane < n)
      {
        double s1 = 0;
        for(int k = 0; k < n; k++)
        {
          s1 += nTile(tA)[lane + kLd * k] * nVec(vDx)[k];
        }
        double s2 = 0;
        for(int a = 0; a < m; a++)
        {
          s2 += mTile(uB)[lane + kLd * a] * mVec(vDu)[a];
        }
        dx = ((m > 0) ? s1 + s2 : s1) + xbar_i; // (2.26b)
      }
      dlam_prev = dlam;
      du_prev = du;
      m = m_next;
    }
    if(lane < n)
    {
      bf.out_d[o.dlam + (b * (T + 1) + T) * n + lane] = dlam_prev;
    }
    fence();
    return (__ballot(bad) != 0) ? kErrorInForward : 0;
  }

  /** ds, dnu (2.27) and the fraction-to-boundary rule (19.9)    :686-696, :713-738.  nan: a delta entry is NaN or Inf. */
  __device__ __forceinline__ void slackStep(double eps, double & alpha_s_max, double & alpha_nu_max, bool & nan, bool fwd_bad) const
  {
    const int T = p.T;
    const OutputLayout o(p.B, T, n, mc, gc);
    double a_s = 1.0, a_nu = 1.0;
    bool bad = false;
    for(int idx = lane; idx < T * gc; idx += kWave)
    {
      const int i = idx / gc, j = idx - i * gc;
      const size_t st = b * T + i;
      const size_t e = st * gc + j;
      double ds = 0, dnu = 0;
      if(j < gAt(i))
      {
        const int mi = mAt(i);
        const double * dxi = bf.out_d + o.dx + (b * (T + 1) + i) * n;
        const double * dui = bf.out_d + o.du + st * mc;
        double s1 = 0;
        for(int k = 0; k < n; k++)
        {
          s1 += bf.C[st * (gc * n) + at(j, k, gc, n)] * dxi[k];
        }
        double s2 = 0;
        for(int a = 0; a < mi; a++)
        {
          s2 += bf.D[st * (gc * mc) + at(j, a, gc, mc)] * dui[a];
        }
        const double s = bf.s[e], nu = bf.nu[e];
        ds = -1 * ((s1 + s2) + bf.out_d[o.gbar + e]);
        dnu = (-1 * (nu * (ds + s) - eps)) / s;
        bad = bad || notFinite(ds) || notFinite(dnu);
        if(ds < 0)
        {
          const double c = ((-1 * 0.995) * s) / ds;
          a_s = (c < a_s) ? c : a_s;
        }
        if(dnu < 0)
        {
          const double c = ((-1 * 0.995) * nu) / dnu;
          a_nu = (c < a_nu) ? c : a_nu;
        }
      }
      bf.out_d[o.ds + e] = ds;
      bf.out_d[o.dnu + e] = dnu;
    }
    fence();
    alpha_s_max = waveMin(a_s);
    alpha_nu_max = waveMin(a_nu);
    nan = fwd_bad || __ballot(bad) != 0;
  }

  /** variable += alpha delta    :802-831 */
  __device__ __forceinline__ void update(double alpha_s, double alpha_nu) const
  {
    const int T = p.T;
    const OutputLayout o(p.B, T, n, mc, gc);
    const double lowest = -1.7976931348623157e308; // std::numeric_limits<double>::lowest()
    for(int idx = lane; idx < (T + 1) * n; idx += kWave)
    {
      const size_t e = b * (T + 1) * n + idx;
      bf.x[e] += alpha_s * bf.out_d[o.dx + e];
      bf.lam[e] += alpha_nu * bf.out_d[o.dlam + e];
    }
    for(int idx = lane; idx < T * mc; idx += kWave)
    {
      const int i = idx / mc, r = idx - i * mc;
      if(r < mAt(i))
      {
        const size_t e = b * T * mc + idx;
        bf.u[e] += alpha_s * bf.out_d[o.du + e];
      }
    }
    for(int idx = lane; idx < T * gc; idx += kWave)
    {
      const int i = idx / gc, j = idx - i * gc;
      if(j < gAt(i))
      {
        const size_t e = b * T * gc + idx;
        double s = bf.s[e] + alpha_s * bf.out_d[o.ds + e];
        double nu = bf.nu[e] + alpha_nu * bf.out_d[o.dnu + e];
        // :813-829: where a step has a negative entry the reference takes max(., lowest()) of every entry of that step, which
        // returns each entry as it is (a NaN included); restated on the negative entry alone
        if(s < 0)
        {
          s = (s < lowest) ? lowest : s;
        }
        if(nu < 0)
        {
          nu = (nu < lowest) ? lowest : nu;
        }
        bf.s[e] = s;
        bf.nu[e] = nu;
      }
    }
  }

  // ===================================================================================================
  // procOnce    :365-493
  // ===================================================================================================
  __device__ __forceinline__ void run() const
  {
    const OutputLayout o(p.B, p.T, n, mc, gc);
    double eps = bf.eps[b];
    if(p.init_complementary_variable)
    {
      initComplementary();
      eps = 1e-4;
    }
    if(p.update_barrier_eps)
    {
      eps = barrierEps();
    }
    const double kkt_error = residuals();
    int status = 0;
    double alpha_s = 1.0, alpha_nu = 1.0;
    if(kkt_error <= p.kkt_error_thre)
    {
      status = kSucceeded;
    }
    if(status == 0)
    {
      status = backwardPass(eps);
    }
    if(status == 0)
    {
      const int fwd = forwardPass();
      bool nan = false;
      slackStep(eps, alpha_s, alpha_nu, nan, fwd != 0);
      if(p.check_nan && nan)
      {
        status = kErrorInForward;
      }
      else if(!(alpha_s > 0.0 && alpha_s <= 1.0 && alpha_nu > 0.0 && alpha_nu <= 1.0))
      {
        status = kErrorInUpdate;
      }
      else
      {
        if(p.apply_update)
        {
          update(alpha_s, alpha_nu);
        }
        status = kIterationContinued;
      }
    }
    if(lane == 0)
    {
      bf.eps[b] = eps;
      bf.out_d[o.kkt + b] = kkt_error;
      bf.out_d[o.alpha_s + b] = alpha_s;
      bf.out_d[o.alpha_nu + b] = alpha_nu;
      bf.out_i[b] = status;
    }
  }
};

__global__ void __launch_bounds__(kWave) fmpc_step_wave_kernel(Buffers bf, Params p)
{
  extern __shared__ __attribute__((aligned(16))) double lds_fmpc_step[];
  const int lane = threadIdx.x;
  const Wave w{bf, p, lds_fmpc_step, blockIdx.x, lane, lane & 15, lane >> 4, p.n, p.m, p.g};
  w.run();
}
} // namespace fmpc_step
} // namespace hip
} // namespace nmpc_amd
