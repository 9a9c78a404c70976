// Device kernel of the batched Riccati backward pass on caller-supplied derivatives (include/nmpc_hip_riccati.h): the reference's
// DDPSolver::backwardPass (DDPSolver.hpp:342-534) with the lambda retry loop of procOnce (:188-214) and the BoxQP feed-forward
// (:450-497, BoxQP.h:141-347), for B independent instances of run-time size (n, m, T).  fp64 only, no FMA contraction.
//
//   riccati_wave_kernel   one wavefront (one 64-thread workgroup) per instance.  The matrices of a step are 16-row tiles in LDS with
//                         leading dimension 17; a tile holds as many columns as the handle's n (or m) asks for, so the LDS request
//                         follows the shape (ldsBytes).  The five triple products of a step run on v_mfma_f64_16x16x4_f64 with
//                         the contraction index and the stored rows and columns masked by n and the step's input dimension m_i.
//                         The m_i x m_i factorisation is cooperative (lane l owns row l, right-looking, over the set bits of the
//                         free mask); the unconstrained pass is the case "every variable free".  In the BoxQP lane j owns variable
//                         j and the clamped set is a ballot, so every branch is wave-uniform.  The n columns of K and the column
//                         of k are solved one per lane, in place in LDS.
//
// Memory traffic: the record of step i - 1 (seven blocks, and u / limits when constrained) is requested into registers right after
// step i's record has been staged, before step i's products and factorisation.  The gains of a step stay in LDS (tile K, vector k)
// until the top of the NEXT step and are written to HBM there, right behind the one wait of that step (the wait for the staged
// record): a wave with a store in flight can only wait for everything, so stores and loads are issued together and
// have a whole step to drain before the next wait.
//
// Statement order follows the reference; sums are ordered as the lanes need them: MFMA accumulation (k ascending in groups of
// four), butterflies in the QP's scalar reductions and in dV.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace nmpc_amd
{
namespace hip
{
namespace riccati
{
constexpr int kMaxDim = 16;
constexpr int kLd = 17; // leading dimension of every tile
constexpr int kWave = 64;
constexpr int kNTiles = 10; // tiles with n columns
constexpr int kMTiles = 7; // tiles with m columns

constexpr int kStatusOk = 1;
constexpr int kStatusLambdaMax = -1;
constexpr int kStatusPassFailed = -2;

typedef double v4d __attribute__((ext_vector_type(4)));

/** The handle's sizes and nmpc_hip_riccati_config as the kernel reads them. */
struct Params
{
  int n, m, T; // m: the handle's input capacity
  int reg_type;
  int with_input_constraint;
  int retry;
  int row_major;
  int limits_per_step;
  size_t B;
  double lambda, dlambda; // used where lam_in / dlam_in are null
  double lambda_factor, lambda_min, lambda_max;
};

/** Inputs and outputs in the boundary layout (nmpc_hip_riccati.h). */
struct Buffers
{
  const double *Fx, *Fu, *Lx, *Lu, *Lxx, *Luu, *Lxu; // [B][T][block]
  const double *VxT, *VxxT; // [B][block]
  const double *U, *lower, *upper; // [B][T][m]; limits [m] or [B][T][m]
  const double *lam_in, *dlam_in; // [B] or null
  const int * dims; // [T] or null
  double * out_d; // the real results, placed by OutputLayout
  int * out_i; // the 32-bit results, likewise
};

/** Where the results are in the handle's two result allocations (offsets in elements), from the shape alone: the kernel holds two
    pointers instead of twelve. */
struct OutputLayout
{
  size_t k, K, dV, Vx0, Vxx0, lam, dlam, doubles;
  size_t qp_retval, free_mask, status, n_backward, fail_step, ints;
  __host__ __device__ OutputLayout(size_t B, size_t T, size_t n, size_t m)
  {
    k = 0;
    K = k + B * T * m;
    dV = K + B * T * m * n;
    Vx0 = dV + B * 2;
    Vxx0 = Vx0 + B * n;
    lam = Vxx0 + B * n * n;
    dlam = lam + B;
    doubles = dlam + B;
    qp_retval = 0;
    free_mask = qp_retval + B * T;
    status = free_mask + B * T;
    n_backward = status + B;
    fail_step = n_backward + B;
    ints = fail_step + B;
  }
};

/** BoxQP::Configuration defaults (BoxQP.h:33-55), as DDPSolver constructs its QP (:469). */
constexpr int kQpMaxIter = 500;
constexpr double kQpGradThre = 1e-8;
constexpr double kQpRelImproveThre = 1e-8;
constexpr double kQpStepFactor = 0.6;
constexpr double kQpMinStep = 1e-22;
constexpr double kQpArmijo = 0.1;

/** Dynamic LDS of one workgroup [bytes]: ten tiles of n columns, seven of m columns, three vectors of n and three of m. */
__host__ __device__ constexpr size_t ldsBytes(int n, int m)
{
  return static_cast<size_t>((kNTiles * kLd + 3) * n + (kMTiles * kLd + 3) * m) * sizeof(double);
}

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

/** The lanes of the one wavefront hand data to each other through LDS.  The LDS executes one wave's instructions in order, so a
    compiler fence is all that is needed, and loads and stores to HBM stay in flight. */
__device__ __forceinline__ void fence()
{
  asm volatile("" ::: "memory");
}

/** The record of one step in registers, as the loads return it: entry (r = lane % 16, c = 4 q + lane / 16) of each block. */
struct Record
{
  double fx[4], fu[4], lxx[4], lxu[4], luu[4];
  double lx, lu, u, lo, up;
};

struct QpResult
{
  int retval;
  unsigned free_mask;
  double x;
};

struct Wave
{
  const Buffers & bf;
  const Params & p;
  double * lds;
  const size_t b;
  mutable int lane, lj, lk;
  mutable int n, mc; // state dimension, input capacity

  /** Hides where the lane indices and the dimensions come from.  Every LDS and HBM address of a step is built from them and none
      changes from step to step: left alone, the compiler computes some two hundred addresses once, in front of the step loop, and
      keeps them in registers (296 VGPRs and 157 SGPRs moved to VGPR lanes, against 128 and 41 with this).  Called at the top of a
      step and between its phases, so that an address is computed where it is used. */
  __device__ void launder() const
  {
    asm volatile("" : "+v"(lane), "+v"(lj), "+v"(lk), "+s"(n), "+s"(mc));
  }

  // tiles of n columns
  enum
  {
    tFx,
    tLxx,
    tVxx,
    tP, // Fx^T Vxx
    tP2, // Fu^T Vxx / Fu^T Vxx_reg    m x n
    tQxx,
    tQux, // m x n
    tQuxR, // m x n
    tK, // m x n
    tVnew // Vxx_reg, then the new Vxx before it is symmetrised
  };
  // tiles of m columns
  enum
  {
    uFu, // n x m
    uLxu, // n x m
    uLuu,
    uQuu,
    uH, // Quu_F
    uF, // the factor of the free block
    uKtQuu // n x m
  };
  enum
  {
    vLx,
    vVx,
    vQx
  };
  enum
  {
    vLu,
    vQu,
    vKff
  };

  __device__ double * nTile(int t) const
  {
    return lds + t * (kLd * n);
  }
  __device__ double * mTile(int u) const
  {
    return lds + kNTiles * (kLd * n) + u * (kLd * mc);
  }
  __device__ double * nVec(int v) const
  {
    return lds + kNTiles * (kLd * n) + kMTiles * (kLd * mc) + v * n;
  }
  __device__ double * mVec(int v) const
  {
    return lds + kNTiles * (kLd * n) + kMTiles * (kLd * mc) + 3 * n + v * mc;
  }
  __device__ int dimAt(int i) const
  {
    return bf.dims ? bf.dims[i] : mc;
  }

  // ===================================================================================================
  // records
  // ===================================================================================================
  /** Entry (r, c) of a rows_cap x cols_cap block, of which rows x cols are read. */
  __device__ double blockEntry(const double * base, int r, int c, int rows, int cols, int rows_cap, int cols_cap) const
  {
    double v = 0.0;
    if(r < rows && c < cols)
    {
      v = base[p.row_major ? r * cols_cap + c : r + rows_cap * c];
    }
    return v;
  }

  __device__ void loadRecord(Record & rec, int i, int m) const
  {
    const size_t s = b * p.T + i;
    const double * Fx = bf.Fx + s * (n * n);
    const double * Fu = bf.Fu + s * (n * mc);
    const double * Lxx = bf.Lxx + s * (n * n);
    const double * Lxu = bf.Lxu + s * (n * mc);
    const double * Luu = bf.Luu + s * (mc * mc);
#pragma unroll
    for(int q = 0; q < 4; q++)
    {
      const int c = 4 * q + lk;
      rec.fx[q] = rec.lxx[q] = rec.fu[q] = rec.lxu[q] = rec.luu[q] = 0.0;
      if(4 * q < n)
      {
        rec.fx[q] = blockEntry(Fx, lj, c, n, n, n, n);
        rec.lxx[q] = blockEntry(Lxx, lj, c, n, n, n, n);
      }
      if(4 * q < m)
      {
        rec.fu[q] = blockEntry(Fu, lj, c, n, m, n, mc);
        rec.lxu[q] = blockEntry(Lxu, lj, c, n, m, n, mc);
        rec.luu[q] = blockEntry(Luu, lj, c, m, m, mc, mc);
      }
    }
    rec.lx = rec.lu = rec.u = rec.lo = rec.up = 0.0;
    if(lane < n)
    {
      rec.lx = bf.Lx[s * n + lane];
    }
    if(lane < m)
    {
      rec.lu = bf.Lu[s * mc + lane];
      if(p.with_input_constraint)
      {
        const size_t at = p.limits_per_step ? s * mc + lane : static_cast<size_t>(lane);
        rec.u = bf.U[s * mc + lane];
        rec.lo = bf.lower[at];
        rec.up = bf.upper[at];
      }
    }
  }

  __device__ void stageRecord(const Record & rec, int m) const
  {
#pragma unroll
    for(int q = 0; q < 4; q++)
    {
      const int c = 4 * q + lk;
      if(lj < n && c < n)
      {
        nTile(tFx)[lj + kLd * c] = rec.fx[q];
        nTile(tLxx)[lj + kLd * c] = rec.lxx[q];
      }
      if(lj < n && c < m)
      {
        mTile(uFu)[lj + kLd * c] = rec.fu[q];
        mTile(uLxu)[lj + kLd * c] = rec.lxu[q];
      }
      if(lj < m && c < m)
      {
        mTile(uLuu)[lj + kLd * c] = rec.luu[q];
      }
    }
    if(lane < n)
    {
      nVec(vLx)[lane] = rec.lx;
    }
    if(lane < m)
    {
      mVec(vLu)[lane] = rec.lu;
    }
  }

  /** k and K of step i from LDS to HBM; rows beyond the step's input dimension are written as 0. */
  __device__ void flushGains(int i, int m) const
  {
    const size_t s = b * p.T + i;
    const OutputLayout at(p.B, p.T, n, mc);
    if(lane < mc)
    {
      bf.out_d[at.k + s * mc + lane] = (lane < m) ? mVec(vKff)[lane] : 0.0;
    }
    double * Ko = bf.out_d + at.K + s * (mc * n);
#pragma unroll
    for(int q = 0; q < 4; q++)
    {
      const int c = 4 * q + lk; // K(a = lj, c)
      if(lj < mc && c < n)
      {
        const double v = (lj < m) ? nTile(tK)[lj + kLd * c] : 0.0;
        Ko[p.row_major ? lj * n + c : lj + mc * c] = v;
      }
    }
  }

  // ===================================================================================================
  // matrix products
  // ===================================================================================================
  /** op(A) * Bm over k < kdim in the MFMA D layout: acc[r] = D(i = lane / 16 + 4 r, j = lane % 16); op(A) = A^T with kTransA.
      D has rows_d rows and cols_d columns; operands outside them (and k >= kdim) are fed as zeros from an in-bounds address. */
  template<bool kTransA>
  __device__ v4d mma(const double * A, const double * Bm, int rows_d, int kdim, int cols_d) const
  {
    v4d acc = {0, 0, 0, 0};
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
  /** rows x cols of dst <- add + acc ("L + product"); with kAddT the entry (j, i) of add. */
  template<bool kAddT>
  __device__ void storeSum(double * dst, const double * add, v4d acc, int rows, int cols) const
  {
#pragma unroll
    for(int r = 0; r < 4; r++)
    {
      const int i = lk + 4 * r;
      if(i < rows && lj < cols)
      {
        dst[i + kLd * lj] = add[kAddT ? lj + kLd * i : i + kLd * lj] + acc[r];
      }
    }
  }
  __device__ void store(double * dst, v4d acc, int rows, int cols) const
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

  // ===================================================================================================
  // factorisation and solves
  // ===================================================================================================
  /** Lower Cholesky factor of H[free, free] into F (unpacked: entry (i, j) of the factor at (i, j), i and j free), right-looking
      over the set bits of `free_mask`; lane l owns row l.  false iff a pivot is <= 0 (a NaN pivot passes). */
  __device__ bool factorFree(unsigned free_mask) const
  {
    const double * H = mTile(uH);
    double * F = mTile(uF);
    const int l = lane;
    const bool is_free = (l < 32) && ((free_mask >> (l & 31)) & 1u);
    fence();
    for(unsigned mj = free_mask; mj; mj &= mj - 1)
    {
      const int j = __builtin_ctz(mj);
      if(is_free && l >= j)
      {
        F[l + kLd * j] = H[l + kLd * j];
      }
    }
    bool positive = true;
    for(unsigned mk = free_mask; mk; mk &= mk - 1)
    {
      const int k = __builtin_ctz(mk);
      const bool below = is_free && l >= k;
      double lik = below ? F[l + kLd * k] : 0.0;
      const double d = bcastLane(lik, k);
      if(d <= 0)
      {
        positive = false;
        break;
      }
      const double s = sqrt(d);
      lik = (l == k) ? s : lik / s;
      if(below)
      {
        F[l + kLd * k] = lik;
      }
      for(unsigned mj = mk & (mk - 1); mj; mj &= mj - 1) // the free j > k
      {
        const int j = __builtin_ctz(mj);
        const double ljk = bcastLane(lik, j);
        if(is_free && l >= j)
        {
          F[l + kLd * j] -= lik * ljk;
        }
      }
    }
    fence();
    return positive;
  }

  /** col[free] <- -(L L^T)^-1 src[free], col[clamped] <- 0: forward then backward substitution in the order of Eigen's llt.solve,
      one lane, in place in LDS. */
  __device__ void solveColumn(double * col, const double * src, unsigned free_mask, int m) const
  {
    const double * F = mTile(uF);
    for(int a = 0; a < m; a++)
    {
      col[a] = src[a];
    }
    for(unsigned mi = free_mask; mi; mi &= mi - 1)
    {
      const int i = __builtin_ctz(mi);
      double s = col[i];
      for(unsigned mj = free_mask & ((1u << i) - 1u); mj; mj &= mj - 1)
      {
        const int j = __builtin_ctz(mj);
        s -= F[i + kLd * j] * col[j];
      }
      col[i] = s / F[i + kLd * i];
    }
    for(unsigned mi = free_mask; mi;)
    {
      const int i = 31 - __builtin_clz(mi);
      mi &= ~(1u << i);
      double s = col[i];
      for(unsigned mj = free_mask & ~((2u << i) - 1u); mj; mj &= mj - 1)
      {
        const int j = __builtin_ctz(mj);
        s -= F[j + kLd * i] * col[j];
      }
      col[i] = s / F[i + kLd * i];
    }
    for(int a = 0; a < m; a++)
    {
      col[a] = ((free_mask >> a) & 1u) ? -1 * col[a] : 0.0;
    }
  }

  // ===================================================================================================
  // BoxQP    BoxQP.h:141-347, after boxqp_wave_kernel: H = tile uH, lane j owns variable j
  // ===================================================================================================
  __device__ QpResult boxQp(int m, double g, double lower, double upper, double x_init) const
  {
    const double * H = mTile(uH);
    const double * F = mTile(uF);
    const int l = lane;
    const bool is_live = l < m;
    const int row = is_live ? l : 0;
    const unsigned live = (1u << m) - 1u; // m <= 16

    auto Hv = [&](double v) {
      double s = 0;
      for(int j = 0; j < m; j++)
      {
        s += H[row + kLd * j] * bcastLane(v, j);
      }
      return s;
    };
    auto objective = [&](double v) {
      const double hv = Hv(v);
      const double vg = waveSum(is_live ? v * g : 0.0);
      const double vhv = waveSum(is_live ? v * hv : 0.0);
      return vg + 0.5 * vhv;
    };

    double x = is_live ? fmax(fmin(x_init, upper), lower) : 0.0; // BoxQP.h:148
    double obj = objective(x);
    double old_obj = obj;
    int retval = 0;
    unsigned clamped = 0, old_clamped = 0, free_mask = 0;
    bool is_free = false;
    for(int iter = 1;; iter++)
    {
      if(iter > 1 && (old_obj - obj) < kQpRelImproveThre * fabs(old_obj)) // BoxQP.h:176-181
      {
        retval = 4;
        break;
      }
      old_obj = obj;

      const double hx = Hv(x); // BoxQP.h:184-206
      const double grad = is_live ? g + hx : 0.0;
      old_clamped = clamped;
      clamped = static_cast<unsigned>(__ballot(is_live && ((x == lower && grad > 0) || (x == upper && grad < 0))));
      free_mask = ~clamped & live;
      is_free = (l < 32) && ((free_mask >> (l & 31)) & 1u);
      if(free_mask == 0) // BoxQP.h:209-213
      {
        retval = 6;
        break;
      }

      if(iter == 1 || clamped != old_clamped) // BoxQP.h:216-241
      {
        if(!factorFree(free_mask))
        {
          retval = -1;
          break;
        }
      }

      const double grad_norm = waveSum(is_free ? grad * grad : 0.0); // BoxQP.h:244-253
      if(grad_norm < kQpGradThre * kQpGradThre)
      {
        retval = 5;
        break;
      }

      // Newton direction on the free dimensions    BoxQP.h:256-279
      double r = 0;
      for(unsigned mj = clamped; mj; mj &= mj - 1)
      {
        const int j = __builtin_ctz(mj);
        r += H[row + kLd * j] * bcastLane(x, j);
      }
      r = g + r;
      const double diag = F[row + kLd * row]; // L(l, l); meaningful in the free lanes only
      for(unsigned mk = free_mask; mk; mk &= mk - 1) // L y = rhs, column-oriented
      {
        const int k = __builtin_ctz(mk);
        if(l == k)
        {
          r = r / diag;
        }
        const double yk = bcastLane(r, k);
        if(is_free && l > k)
        {
          r -= F[l + kLd * k] * yk;
        }
      }
      for(unsigned mk = free_mask; mk;) // L' z = y, column-oriented (descending k): row k of L across the lanes
      {
        const int k = 31 - __builtin_clz(mk);
        mk &= ~(1u << k);
        if(l == k)
        {
          r = r / diag;
        }
        const double zk = bcastLane(r, k);
        if(is_free && l < k)
        {
          r -= F[k + kLd * l] * zk;
        }
      }
      const double dir = is_free ? -1 * r - x : 0.0;

      const double sdg = waveSum(dir * grad); // BoxQP.h:282-291
      if(sdg > 1e-10)
      {
        retval = -2;
        break;
      }

      // Armijo line search with projection    BoxQP.h:294-309
      double step = 1;
      double cand = is_live ? fmax(fmin(x + step * dir, upper), lower) : 0.0;
      double obj_cand = objective(cand);
      while((obj_cand - old_obj) / (step * sdg) < kQpArmijo)
      {
        step = step * kQpStepFactor;
        cand = is_live ? fmax(fmin(x + step * dir, upper), lower) : 0.0;
        obj_cand = objective(cand);
        if(step < kQpMinStep)
        {
          retval = 2; // leaves only the inner loop (BoxQP.h:304-308)
          break;
        }
      }

      x = cand; // BoxQP.h:328-329
      obj = obj_cand;
      if(iter == kQpMaxIter) // BoxQP.h:332-336
      {
        retval = 1;
        break;
      }
    }
    QpResult out;
    out.retval = retval;
    out.free_mask = free_mask;
    out.x = x;
    return out;
  }

  // ===================================================================================================
  // backwardPass    DDPSolver.hpp:342-534
  // ===================================================================================================
  /** One pass at `lambda`; returns the step at which it failed, or -1.  dV is valid after a pass that succeeded. */
  __device__ int backwardPass(double lambda, double & dV0, double & dV1) const
  {
    const int T = p.T;
    // Vx = last_Vx_, Vxx = last_Vxx_    :346-347
    {
      const double * V = bf.VxxT + b * (n * n);
#pragma unroll
      for(int q = 0; q < 4; q++)
      {
        const int c = 4 * q + lk;
        if(lj < n && c < n)
        {
          nTile(tVxx)[lj + kLd * c] = V[p.row_major ? lj * n + c : lj + n * c];
        }
      }
      if(lane < n)
      {
        nVec(vVx)[lane] = bf.VxT[b * n + lane];
      }
    }
    dV0 = 0;
    dV1 = 0;
    Record rec;
    int m = dimAt(T - 1);
    loadRecord(rec, T - 1, m);
    int m_prev = 0; // input dimension of step i + 1, whose gains are still in LDS
    for(int i = T - 1; i >= 0; i--)
    {
      launder();
      stageRecord(rec, m);
      const double u_i = rec.u, lo_i = rec.lo, up_i = rec.up;
      fence();
      if(i < T - 1)
      {
        flushGains(i + 1, m_prev);
      }
      const int m_next = (i > 0) ? dimAt(i - 1) : 0;
      if(i > 0)
      {
        loadRecord(rec, i - 1, m_next);
      }

      launder();
      // ---- Q terms    :386-408
      store(nTile(tP), mma<true>(nTile(tFx), nTile(tVxx), n, n, n), n, n);
      if(m > 0)
      {
        store(nTile(tP2), mma<true>(mTile(uFu), nTile(tVxx), m, n, n), m, n);
      }
      fence();
      storeSum<false>(nTile(tQxx), nTile(tLxx), mma<false>(nTile(tP), nTile(tFx), n, n, n), n, n);
      if(m > 0)
      {
        storeSum<true>(nTile(tQux), mTile(uLxu), mma<false>(nTile(tP2), nTile(tFx), m, n, n), m, n);
        storeSum<false>(mTile(uQuu), mTile(uLuu), mma<false>(nTile(tP2), mTile(uFu), m, n, m), m, m);
      }
      if(lane < n) // Qx    :388
      {
        double s = 0;
        for(int k = 0; k < n; k++)
        {
          s += nTile(tFx)[k + kLd * lane] * nVec(vVx)[k];
        }
        nVec(vQx)[lane] = nVec(vLx)[lane] + s;
      }
      if(lane < m) // Qu    :386
      {
        double s = 0;
        for(int k = 0; k < n; k++)
        {
          s += mTile(uFu)[k + kLd * lane] * nVec(vVx)[k];
        }
        mVec(vQu)[lane] = mVec(vLu)[lane] + s;
      }
      fence();

      unsigned free_mask = 0;
      if(m > 0)
      {
        // ---- regularisation    :421-441
        if(p.reg_type == 2)
        {
#pragma unroll
          for(int q = 0; q < 4; q++)
          {
            const int c = 4 * q + lk;
            if(lj < n && c < n)
            {
              const double v = nTile(tVxx)[lj + kLd * c];
              nTile(tVnew)[lj + kLd * c] = (lj == c) ? v + lambda : v;
            }
          }
          fence();
          store(nTile(tP2), mma<true>(mTile(uFu), nTile(tVnew), m, n, n), m, n);
          fence();
          storeSum<true>(nTile(tQuxR), mTile(uLxu), mma<false>(nTile(tP2), nTile(tFx), m, n, n), m, n);
          storeSum<false>(mTile(uH), mTile(uLuu), mma<false>(nTile(tP2), mTile(uFu), m, n, m), m, m);
        }
        else
        {
          // Vxx_reg = Vxx: the products of :427 and :433 are those of :390 and :399, bit for bit
#pragma unroll
          for(int q = 0; q < 4; q++)
          {
            const int c = 4 * q + lk;
            if(lj < m && c < n)
            {
              nTile(tQuxR)[lj + kLd * c] = nTile(tQux)[lj + kLd * c];
            }
            if(lj < m && c < m)
            {
              const double v = mTile(uQuu)[lj + kLd * c];
              mTile(uH)[lj + kLd * c] = (lj == c) ? v + lambda : v; // :438-441
            }
          }
        }
        fence();

        launder();
        // ---- gains    :448-517
        if(p.with_input_constraint)
        {
          const bool warm = (i != T - 1) && (m_prev == m); // :452-467
          const double x_init = (warm && lane < m) ? mVec(vKff)[lane] : 0.0;
          const double g = (lane < m) ? mVec(vQu)[lane] : 0.0;
          const QpResult qp = boxQp(m, g, lo_i - u_i, up_i - u_i, x_init); // :469-472
          if(lane == 0)
          {
            const OutputLayout at(p.B, p.T, n, mc);
            bf.out_i[at.qp_retval + b * T + i] = qp.retval;
            bf.out_i[at.free_mask + b * T + i] = static_cast<int>(qp.free_mask);
          }
          if(qp.retval < 0) // :473-480
          {
            return i;
          }
          free_mask = qp.free_mask;
          fence();
          if(lane < m)
          {
            mVec(vKff)[lane] = qp.x;
          }
          if(lane < n) // :482-496
          {
            solveColumn(nTile(tK) + kLd * lane, nTile(tQuxR) + kLd * lane, free_mask, m);
          }
        }
        else
        {
          free_mask = (1u << m) - 1u;
          if(!factorFree(free_mask)) // :500-508
          {
            return i;
          }
          if(lane < n) // :509-510
          {
            solveColumn(nTile(tK) + kLd * lane, nTile(tQuxR) + kLd * lane, free_mask, m);
          }
          else if(lane == n)
          {
            solveColumn(mVec(vKff), mVec(vQu), free_mask, m);
          }
        }
        fence();

        // ---- cost-to-go    :522
        {
          double kQu = 0, kQuuk = 0;
          if(lane < m)
          {
            double s = 0;
            for(int q = 0; q < m; q++)
            {
              s += mTile(uQuu)[lane + kLd * q] * mVec(vKff)[q];
            }
            kQu = mVec(vKff)[lane] * mVec(vQu)[lane];
            kQuuk = mVec(vKff)[lane] * s;
          }
          dV0 += waveSum(kQu);
          dV1 += 0.5 * waveSum(kQuuk);
        }
        store(mTile(uKtQuu), mma<true>(nTile(tK), mTile(uQuu), n, m, m), n, m);
        fence();
      }
      launder();
      // Vx    :523
      if(lane < n)
      {
        double s1 = 0, s2 = 0, s3 = 0;
        for(int a = 0; a < m; a++)
        {
          s1 += mTile(uKtQuu)[lane + kLd * a] * mVec(vKff)[a];
          s2 += nTile(tK)[a + kLd * lane] * mVec(vQu)[a];
          s3 += nTile(tQux)[a + kLd * lane] * mVec(vKff)[a];
        }
        nVec(vVx)[lane] = ((nVec(vQx)[lane] + s1) + s2) + s3;
      }
      // Vxx    :524-526
      {
        const v4d t1 = mma<false>(mTile(uKtQuu), nTile(tK), n, m, n);
        const v4d t2 = mma<true>(nTile(tK), nTile(tQux), n, m, n);
        const v4d t3 = mma<true>(nTile(tQux), nTile(tK), n, m, n);
#pragma unroll
        for(int r = 0; r < 4; r++)
        {
          const int row = lk + 4 * r;
          if(row < n && lj < n)
          {
            const int at = row + kLd * lj;
            nTile(tVnew)[at] = ((nTile(tQxx)[at] + t1[r]) + t2[r]) + t3[r];
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
          nTile(tVxx)[lj + kLd * c] = 0.5 * (nTile(tVnew)[lj + kLd * c] + nTile(tVnew)[c + kLd * lj]);
        }
      }
      fence();
      m_prev = m;
      m = m_next;
    }
    flushGains(0, m_prev);
    return -1;
  }

  // ===================================================================================================
  // the retry loop    DDPSolver.hpp:188-214
  // ===================================================================================================
  __device__ void run() const
  {
    double lambda = bf.lam_in ? bf.lam_in[b] : p.lambda;
    double dlambda = bf.dlam_in ? bf.dlam_in[b] : p.dlambda;
    double dV0 = 0, dV1 = 0;
    int status = 0, n_backward = 0, fail_step = -1;
    for(;;)
    {
      n_backward++;
      const int failed_at = backwardPass(lambda, dV0, dV1);
      if(failed_at < 0)
      {
        status = kStatusOk;
        break;
      }
      fail_step = failed_at;
      if(!p.retry)
      {
        status = kStatusPassFailed;
        break;
      }
      dlambda = fmax(dlambda * p.lambda_factor, p.lambda_factor); // :194-195
      lambda = fmax(lambda * dlambda, p.lambda_min);
      if(lambda > p.lambda_max) // :196-204
      {
        status = kStatusLambdaMax;
        break;
      }
    }
    fence();
    const OutputLayout at(p.B, p.T, n, mc);
    if(lane < n)
    {
      bf.out_d[at.Vx0 + b * n + lane] = nVec(vVx)[lane];
    }
    {
      double * V = bf.out_d + at.Vxx0 + b * (n * n);
#pragma unroll
      for(int q = 0; q < 4; q++)
      {
        const int c = 4 * q + lk;
        if(lj < n && c < n)
        {
          V[p.row_major ? lj * n + c : lj + n * c] = nTile(tVxx)[lj + kLd * c];
        }
      }
    }
    if(lane == 0)
    {
      bf.out_d[at.dV + b * 2 + 0] = dV0;
      bf.out_d[at.dV + b * 2 + 1] = dV1;
      bf.out_d[at.lam + b] = lambda;
      bf.out_d[at.dlam + b] = dlambda;
      bf.out_i[at.status + b] = status;
      bf.out_i[at.n_backward + b] = n_backward;
      bf.out_i[at.fail_step + b] = fail_step;
    }
  }
};

__global__ void __launch_bounds__(kWave) riccati_wave_kernel(Buffers bf, Params p)
{
  extern __shared__ __attribute__((aligned(16))) double lds_riccati[];
  const int lane = threadIdx.x;
  const Wave w{bf, p, lds_riccati, blockIdx.x, lane, lane & 15, lane >> 4, p.n, p.m};
  w.run();
}
} // namespace riccati
} // namespace hip
} // namespace nmpc_amd
