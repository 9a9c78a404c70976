// Batched dense GMRES for gfx950: one wavefront per system (the reference's nmpc_cgmres::Gmres::solve, Gmres.h:67-192, both the
// Givens and the Householder variant).  Shares nothing with cgmres_kernels.hpp, whose lane-per-system kernel stays the diagnostic.
//
// Work layout.  A workgroup is one wavefront of 64 lanes and owns one system.  Lane l owns rows l, l + 64, ... of it: its entries of
// r, of A v and of every basis vector.  A is read as its transposed image At[j][i] = A(i, j), so the 64 lanes' reads of column j
// over their rows are one contiguous segment.  Basis vectors are rows of [k_max + 1][n] in HBM and are only ever read by the lane
// that wrote them; the vector being orthogonalised (w) and a copy of the newest basis vector (v, broadcast-read by the product)
// live in LDS, as do the current column of H, g, the Givens pairs, the diagonal of R and y.  H itself is written column by column
// to the handle's [k_max + 1][k_max] array in HBM (entry (i, .) by lane i % 64, which is also the lane that reads it back in the
// back substitution).  The Householder variant adds its (k + 1) x (k + 1) working copy [H | g] in LDS.  Nothing indexed at run time
// lives in registers, so the kernel needs no scratch.  Every branch is wave-uniform.
//
// Order of the arithmetic (tests/cpp/gmres_checker.cpp restates it operation for operation, sum order "wave"; the translation
// unit is compiled with -ffp-contract=off):
//   * entry i of A v: acc = 0, then acc = acc + At[j][i] * v[j] for j ascending, on the lane that owns row i;
//   * a dot product or squared norm: each lane's partial p = 0, p = p + a[i] * b[i] over its rows i ascending, then the butterfly
//     p = p + p(lane ^ m) for m = 32, 16, 8, 4, 2, 1 (every lane ends with the same bits: + is commutative);
//   * modified Gram-Schmidt, the re-orthogonalisation test, the rotations, nu, c_k, s_k: the statements of Gmres.h:94-168 in their
//     order (pow(x, 2) as x * x); normalized() divides by sqrt(squared norm) where that is > 0 and leaves the vector otherwise;
//   * back substitution by columns: for i = k - 1 .. 0: y[i] = y[i] / R(i, i), then y[j] = y[j] - y[i] * R(j, i) for j < i;
//   * x[i] = x[i] + y[j] * basis[j][i] for j ascending;
//   * Householder variant, per iteration, on W = [H(0..k, 0..k-1) | g(0..k)]: for column j = 0 .. k - 1: alpha = W(j, j),
//     ss = sum of W(i, j)^2 for i = j + 1 .. k ascending (every lane computes it, sequentially); if ss != 0: nrm = sqrt(alpha * alpha
//     + ss), beta = alpha >= 0 ? -nrm : nrm, tau = (beta - alpha) / beta, u[i] = W(i, j) / (alpha - beta); every later column c
//     (one lane per column, the right-hand side included): d = W(j, c), d = d + u[i] * W(i, c) ascending, d = tau * d,
//     W(j, c) -= d, W(i, c) -= d * u[i]; W(j, j) = beta.  Then the back substitution above on R = W(0..k-1, 0..k-1), and
//     rho = || g - H y || (Gmres.h:175): t[i] = g[i] - s[i], s[i] = 0 + H(i, j) * y[j] for j ascending, and the norm as above.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>

namespace nmpc_amd
{
namespace hip
{
namespace gmres
{
constexpr int kMaxDim = 512;
constexpr int kHouseholderMaxK = 128;
constexpr int kWave = 64;
constexpr int kTile = 32; // ingest transpose tile

enum Status
{
  kConverged = 1,
  kKMax = 2,
  kNonFinite = 3
};

struct Params
{
  int n;
  int k_max; // already clamped to n
  double eps;
  int make_triangular;
  int apply_reorth;
};

struct Buffers
{
  const double * At; // [B][n][n], At[j][i] = A(i, j)
  const double * b; // [B][n]
  double * x; // [B][n] in: initial guess, out: solution
  double * basis; // [B][k_max + 1][n]
  double * H; // [B][k_max + 1][k_max], zeroed before the launch
  double * g; // [B][k_max + 1]
  double * err; // [B][k_max + 1]
  int * iters; // [B]
  int * reorth; // [B]
  int * status; // [B]
};

/** Doubles of LDS of one workgroup: w, v [n]; hcol, g, u [K + 1]; cs, sn, diag, y [K]; Householder: W [(K + 1)^2]. */
inline size_t waveLdsBytes(int n, int k_max, bool make_triangular)
{
  const size_t K = static_cast<size_t>(k_max);
  return (2 * static_cast<size_t>(n) + 3 * (K + 1) + 4 * K + (make_triangular ? 0 : (K + 1) * (K + 1))) * sizeof(double);
}

/** At[b][j][i] = A[b][i][j] through a padded LDS tile; grid (ceil(n / 32), ceil(n / 32), B), block (32, 8). */
__global__ __launch_bounds__(kTile * 8) void gmres_ingest_kernel(const double * __restrict__ A, double * __restrict__ At, int n)
{
  __shared__ double tile[kTile][kTile + 1];
  const size_t base = static_cast<size_t>(blockIdx.z) * n * n;
  const int i0 = blockIdx.y * kTile, j0 = blockIdx.x * kTile;
  for(int r = threadIdx.y; r < kTile; r += 8)
  {
    const int i = i0 + r, j = j0 + threadIdx.x;
    if(i < n && j < n)
    {
      tile[r][threadIdx.x] = A[base + static_cast<size_t>(i) * n + j];
    }
  }
  __syncthreads();
  for(int r = threadIdx.y; r < kTile; r += 8)
  {
    const int j = j0 + r, i = i0 + threadIdx.x;
    if(i < n && j < n)
    {
      At[base + static_cast<size_t>(j) * n + i] = tile[threadIdx.x][r];
    }
  }
}

/** The butterfly of a wavefront's 64 partials; every lane returns the same bits. */
__device__ inline double waveSum(double p)
{
  for(int m = kWave / 2; m >= 1; m >>= 1)
  {
    p = p + __shfl_xor(p, m, kWave);
  }
  return p;
}

/** Partial over this lane's rows of a[i] * b[i], then the butterfly.  a and b may be LDS or HBM; each lane touches its own rows. */
__device__ inline double waveDot(const double * a, const double * b, int n, int lane)
{
  double p = 0.0;
  for(int i = lane; i < n; i += kWave)
  {
    p = p + a[i] * b[i];
  }
  return waveSum(p);
}

/** w[own rows] = sum over j ascending of At[j][i] * v[j]; v is read by every lane (LDS broadcast).  NS = ceil(n / 64) stripes of rows
    per lane, each with its own accumulator (the stripe index is a compile-time constant after unrolling, so they are registers), so
    that NS loads per column and kColumns columns (16 loads in all where NS divides 16) are in flight at once; a row beyond n reads
    row n - 1 and is dropped. */
template<int NS>
__device__ inline void waveMatVecStripes(const double * __restrict__ At, const double * v, double * w, int n, int lane)
{
  constexpr int kColumns = NS >= 5 ? 2 : (NS >= 3 ? 4 : (NS == 2 ? 8 : 16));
  double acc[NS];
  int row[NS];
#pragma unroll
  for(int s = 0; s < NS; s++)
  {
    acc[s] = 0.0;
    row[s] = min(lane + kWave * s, n - 1);
  }
#pragma unroll kColumns
  for(int j = 0; j < n; j++)
  {
    const double vj = v[j];
    const double * col = At + static_cast<size_t>(j) * n;
#pragma unroll
    for(int s = 0; s < NS; s++)
    {
      acc[s] = acc[s] + col[row[s]] * vj;
    }
  }
#pragma unroll
  for(int s = 0; s < NS; s++)
  {
    if(lane + kWave * s < n)
    {
      w[lane + kWave * s] = acc[s];
    }
  }
}

__device__ inline void waveMatVec(const double * __restrict__ At, const double * v, double * w, int n, int lane)
{
  switch((n + kWave - 1) / kWave) // wave-uniform
  {
    case 1:
      return waveMatVecStripes<1>(At, v, w, n, lane);
    case 2:
      return waveMatVecStripes<2>(At, v, w, n, lane);
    case 3:
      return waveMatVecStripes<3>(At, v, w, n, lane);
    case 4:
      return waveMatVecStripes<4>(At, v, w, n, lane);
    case 5:
      return waveMatVecStripes<5>(At, v, w, n, lane);
    case 6:
      return waveMatVecStripes<6>(At, v, w, n, lane);
    case 7:
      return waveMatVecStripes<7>(At, v, w, n, lane);
    default:
      return waveMatVecStripes<8>(At, v, w, n, lane);
  }
}

/** The loop of Gmres.h:104-110 (accumulate = false: hcol[j] = h) or :123-128 (true: hcol[j] += h) over basis vectors 0 .. k - 1:
    h = <w, q_j>, w = w - h * q_j.  The lane's NS entries of w stay in registers for the whole loop and q_{j+1} is loaded while the
    butterfly of q_j runs; the partial of a dot product still runs over the lane's rows ascending.  Every lane stores the same h. */
template<int NS>
__device__ inline void waveOrthogonaliseStripes(double * w, const double * __restrict__ V, int k, double * hcol, bool accumulate, int n, int lane)
{
  double wv[NS], qv[NS], qn[NS];
  int row[NS];
  bool own[NS];
#pragma unroll
  for(int s = 0; s < NS; s++)
  {
    own[s] = lane + kWave * s < n;
    row[s] = min(lane + kWave * s, n - 1);
    wv[s] = w[row[s]];
    qn[s] = V[row[s]];
  }
  for(int j = 0; j < k; j++)
  {
#pragma unroll
    for(int s = 0; s < NS; s++)
    {
      qv[s] = qn[s];
    }
    if(j + 1 < k)
    {
      const double * q = V + static_cast<size_t>(j + 1) * n;
#pragma unroll
      for(int s = 0; s < NS; s++)
      {
        qn[s] = q[row[s]];
      }
    }
    double p = 0.0;
#pragma unroll
    for(int s = 0; s < NS; s++)
    {
      p = own[s] ? p + wv[s] * qv[s] : p;
    }
    const double h = waveSum(p);
#pragma unroll
    for(int s = 0; s < NS; s++)
    {
      wv[s] = wv[s] - h * qv[s];
    }
    hcol[j] = accumulate ? hcol[j] + h : h;
  }
#pragma unroll
  for(int s = 0; s < NS; s++)
  {
    if(own[s])
    {
      w[lane + kWave * s] = wv[s];
    }
  }
}

__device__ inline void waveOrthogonalise(double * w, const double * __restrict__ V, int k, double * hcol, bool accumulate, int n, int lane)
{
  switch((n + kWave - 1) / kWave) // wave-uniform
  {
    case 1:
      return waveOrthogonaliseStripes<1>(w, V, k, hcol, accumulate, n, lane);
    case 2:
      return waveOrthogonaliseStripes<2>(w, V, k, hcol, accumulate, n, lane);
    case 3:
      return waveOrthogonaliseStripes<3>(w, V, k, hcol, accumulate, n, lane);
    case 4:
      return waveOrthogonaliseStripes<4>(w, V, k, hcol, accumulate, n, lane);
    case 5:
      return waveOrthogonaliseStripes<5>(w, V, k, hcol, accumulate, n, lane);
    case 6:
      return waveOrthogonaliseStripes<6>(w, V, k, hcol, accumulate, n, lane);
    case 7:
      return waveOrthogonaliseStripes<7>(w, V, k, hcol, accumulate, n, lane);
    default:
      return waveOrthogonaliseStripes<8>(w, V, k, hcol, accumulate, n, lane);
  }
}

__global__ __launch_bounds__(kWave) void gmres_wave_kernel(Buffers buf, Params p)
{
  extern __shared__ __align__(16) double gmres_lds[];
  const int lane = threadIdx.x;
  const size_t sys = blockIdx.x;
  const int n = p.n, K = p.k_max;
  const int LD = K + 1; // row stride of W
  double * w = gmres_lds;
  double * v = w + n;
  double * hcol = v + n; // [K + 1] the column of H being built
  double * g = hcol + (K + 1); // [K + 1]
  double * u = g + (K + 1); // [K + 1] Householder reflector
  double * cs = u + (K + 1); // [K]
  double * sn = cs + K; // [K]
  double * diag = sn + K; // [K] R(i, i) of the triangular variant
  double * y = diag + K; // [K]
  double * W = y + K; // [(K + 1)^2], Householder variant only

  const double * At = buf.At + sys * n * n;
  const double * b = buf.b + sys * n;
  double * x = buf.x + sys * n;
  double * V = buf.basis + sys * (K + 1) * n;
  double * H = buf.H + sys * (K + 1) * K;
  double * err = buf.err + sys * (K + 1);

  // 1. r = b - A x (Gmres.h:79)
  for(int i = lane; i < n; i += kWave)
  {
    v[i] = x[i];
  }
  __syncthreads();
  waveMatVec(At, v, w, n, lane);
  for(int i = lane; i < n; i += kWave)
  {
    w[i] = b[i] - w[i];
  }
  const double rr = waveDot(w, w, n, lane);
  double rho = sqrt(rr); // :81
  const double b_norm = sqrt(waveDot(b, b, n, lane)); // :86
  __syncthreads(); // every lane has read v
  {
    // basis_.push_back(r.normalized()) (:80)
    const bool scale = rr > 0.0;
    for(int i = lane; i < n; i += kWave)
    {
      const double e = scale ? w[i] / rho : w[i];
      V[i] = e;
      v[i] = e;
    }
  }
  for(int i = lane; i <= K; i += kWave)
  {
    g[i] = i == 0 ? rho : 0.0; // :83-84
    err[i] = i == 0 ? rho : __builtin_nan(""); // :88
  }
  __syncthreads();

  int k = 0, fired = 0;
  while(rho > p.eps * b_norm && k < K) // :94
  {
    k++;
    // (b) Avk = A v_k; new_basis = Avk minus its components along the basis (:102-110)
    waveMatVec(At, v, w, n, lane);
    const double avk_norm = sqrt(waveDot(w, w, n, lane)); // :119 (Avk is not kept: its norm is taken here)
    waveOrthogonalise(w, V, k, hcol, false, n, lane);
    // (c)
    double zz = waveDot(w, w, n, lane);
    const double new_basis_norm = sqrt(zz); // :113
    hcol[k] = new_basis_norm;
    // (d)
    if(p.apply_reorth && avk_norm + 1e-3 * new_basis_norm == avk_norm) // :120
    {
      fired++;
      waveOrthogonalise(w, V, k, hcol, true, n, lane);
      zz = waveDot(w, w, n, lane);
    }
    __syncthreads(); // every lane has read v; hcol is complete
    // (e) basis_.push_back(new_basis.normalized()) (:133)
    {
      const bool scale = zz > 0.0;
      const double nrm = sqrt(zz);
      double * q = V + static_cast<size_t>(k) * n;
      for(int i = lane; i < n; i += kWave)
      {
        const double e = scale ? w[i] / nrm : w[i];
        q[i] = e;
        v[i] = e;
      }
    }
    if(p.make_triangular)
    {
      // (f) i. the earlier rotations on the new column (:139-147); every lane runs the chain on the same values
      double t = hcol[0];
      for(int i = 0; i < k - 1; i++)
      {
        const double h1 = hcol[i + 1], c = cs[i], s = sn[i];
        hcol[i] = c * t - s * h1;
        t = s * t + c * h1;
      }
      // ii., iii. (:150-158)
      const double hk = hcol[k];
      const double nu = sqrt(t * t + hk * hk);
      const double c_k = t / nu, s_k = -hk / nu;
      const double rkk = c_k * t - s_k * hk;
      // iv. (:161-164)
      const double g0 = g[k - 1], g1 = g[k];
      __syncthreads(); // reads above before the (same-valued) writes below
      cs[k - 1] = c_k;
      sn[k - 1] = s_k;
      hcol[k - 1] = rkk;
      hcol[k] = 0.0;
      diag[k - 1] = rkk;
      g[k - 1] = c_k * g0 - s_k * g1;
      const double gk = s_k * g0 + c_k * g1;
      g[k] = gk;
      rho = fabs(gk); // (g) :167
      __syncthreads();
      for(int i = lane; i <= k; i += kWave)
      {
        H[static_cast<size_t>(i) * K + (k - 1)] = hcol[i];
      }
    }
    else
    {
      for(int i = lane; i <= k; i += kWave)
      {
        H[static_cast<size_t>(i) * K + (k - 1)] = hcol[i];
      }
      __syncthreads(); // H in HBM is read across lanes below
      // (f) y_k = argmin || g - H y || by Householder QR (:172) on W = [H | g]
      for(int e = lane; e < (k + 1) * (k + 1); e += kWave)
      {
        const int i = e / (k + 1), c = e - i * (k + 1);
        W[i * LD + c] = c < k ? H[static_cast<size_t>(i) * K + c] : g[i];
      }
      __syncthreads();
      for(int j = 0; j < k; j++)
      {
        const double alpha = W[j * LD + j];
        double ss = 0.0;
        for(int i = j + 1; i <= k; i++)
        {
          const double e = W[i * LD + j];
          ss = ss + e * e;
        }
        if(ss != 0.0)
        {
          const double nrm = sqrt(alpha * alpha + ss);
          const double beta = alpha >= 0.0 ? -nrm : nrm;
          const double tau = (beta - alpha) / beta;
          const double den = alpha - beta;
          for(int i = j + 1 + lane; i <= k; i += kWave)
          {
            u[i] = W[i * LD + j] / den;
          }
          __syncthreads();
          for(int c = j + 1 + lane; c <= k; c += kWave)
          {
            double d = W[j * LD + c];
            for(int i = j + 1; i <= k; i++)
            {
              d = d + u[i] * W[i * LD + c];
            }
            d = tau * d;
            W[j * LD + c] = W[j * LD + c] - d;
            for(int i = j + 1; i <= k; i++)
            {
              W[i * LD + c] = W[i * LD + c] - d * u[i];
            }
          }
          __syncthreads(); // the reads of column j and of u are done
          W[j * LD + j] = beta;
        }
        __syncthreads();
      }
      for(int i = lane; i < k; i += kWave)
      {
        y[i] = W[i * LD + k];
      }
      __syncthreads();
      for(int i = k - 1; i >= 0; i--)
      {
        const double yi = y[i] / W[i * LD + i];
        __syncthreads();
        y[i] = yi;
        for(int j = lane; j < i; j += kWave)
        {
          y[j] = y[j] - yi * W[j * LD + i];
        }
        __syncthreads();
      }
      // (g) rho = || g - H y || (:175)
      double pt = 0.0;
      for(int i = lane; i <= k; i += kWave)
      {
        double s = 0.0;
        for(int j = 0; j < k; j++)
        {
          s = s + H[static_cast<size_t>(i) * K + j] * y[j];
        }
        const double t = g[i] - s;
        pt = pt + t * t;
      }
      rho = sqrt(waveSum(pt));
    }
    if(lane == 0)
    {
      err[k] = rho; // :178
    }
    __syncthreads();
  }

  if(p.make_triangular)
  {
    // 3. y_k = R^{-1} g (:184); R(j, i) is read by the lane that wrote it
    for(int i = lane; i < k; i += kWave)
    {
      y[i] = g[i];
    }
    __syncthreads();
    for(int i = k - 1; i >= 0; i--)
    {
      const double yi = y[i] / diag[i];
      __syncthreads();
      y[i] = yi;
      for(int j = lane; j < i; j += kWave)
      {
        y[j] = y[j] - yi * H[static_cast<size_t>(j) * K + i];
      }
      __syncthreads();
    }
  }
  // 4. x += y_k(i) * basis_[i] (:188-191)
  bool finite = isfinite(rho);
  for(int i = lane; i < n; i += kWave)
  {
    double xi = x[i];
    for(int j = 0; j < k; j++)
    {
      xi = xi + y[j] * V[static_cast<size_t>(j) * n + i];
    }
    x[i] = xi;
    finite = finite && isfinite(xi);
  }
  const bool all_finite = __all(finite);
  for(int i = lane; i <= K; i += kWave)
  {
    buf.g[sys * (K + 1) + i] = g[i];
  }
  if(lane == 0)
  {
    buf.iters[sys] = k;
    buf.reorth[sys] = fired;
    buf.status[sys] = !all_finite ? kNonFinite : (rho > p.eps * b_norm ? kKMax : kConverged);
  }
}
} // namespace gmres
} // namespace hip
} // namespace nmpc_amd
