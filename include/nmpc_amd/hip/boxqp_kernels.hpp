// Device kernels of the batched BoxQP solver (include/nmpc_hip_boxqp.h): the reference's BoxQP<VarDim>::solve (BoxQP.h:141-347)
// for B independent QPs of one run-time size n.  fp64 only.
//
//   boxqp_lane_kernel   one QP per lane, n <= 16.  Inputs, iterates, the factor and the results live in HBM addressed
//                       [element][instance], so the 64 lanes of a wavefront load and store 64 consecutive doubles; nothing is kept
//                       in a run-time-indexed register array.  boxqp_ingest_kernel converts the inputs from the boundary layout
//                       [instance][element], boxqp_egress_kernel converts X and FACTOR back when they are asked for.  No workgroup
//                       barrier: a lane leaves the main loop at its own iteration.
//   boxqp_wave_kernel   one wavefront (one 64-thread workgroup) per QP, n <= 64.  Lane j owns variable j: x_j, g_j, its limits,
//                       grad_j, its search direction and its clamped flag.  The clamped set is a wave ballot, so every branch on
//                       the active set, on the objective and on the exits is wave-uniform.  H and the factor are in LDS,
//                       column-major, lanes over rows: every access of a fixed column is contiguous.  A lane reads and writes only
//                       its own row of either matrix and gets the other lanes' values by v_readlane broadcasts, with ONE
//                       exception: the back substitution L'z = y, column-oriented, reads row k of L across the lanes — hence the
//                       factor's odd leading dimension (a stride of n doubles would put every lane on one bank for even n) and the
//                       wave-level synchronisation after the factorisation.
//
// Both kernels run the same algorithm in the same order, statement for statement after BoxQP.h; they differ where the wave kernel
// sums across lanes (objective, free gradient norm, search_dir . grad: a butterfly instead of the reference's left-to-right sum).
// The Cholesky factorisation of the free block is right-looking over the set bits of the free mask and works on the UNPACKED
// matrix (entry (i, j) of the factor at (i, j) of the workspace, i and j free); it is packed into free_idxs_ order when FACTOR is
// written.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace nmpc_amd
{
namespace hip
{
namespace boxqp
{
constexpr int kMaxDim = 64;
constexpr int kLaneMaxDim = 16;
constexpr int kTraceColumns = 6;
constexpr int kLaneBlock = 64; // lane kernel: one wavefront per workgroup (no LDS, no barrier)

/** BoxQP::Configuration (BoxQP.h:33-55) as the kernels read it. */
struct Params
{
  int max_iter;
  double grad_thre;
  double rel_improve_thre;
  double step_factor;
  double min_step;
  double armijo_param;
  int trace_capacity;
};

/** Results in the boundary layout (nmpc_hip_boxqp.h), written by both kernels. */
struct Results
{
  int * retval; // [B]
  int * iter; // [B]
  int * factorization_num; // [B]
  unsigned long long * free_mask; // [B]
  double * obj; // [B]
  double * trace; // [B][trace_capacity][6]
};

/** Leading dimension of the wave kernel's factor in LDS: odd, so that the lanes' reads of one ROW fall on distinct banks. */
__host__ __device__ inline int waveFactorLd(int n)
{
  return n | 1;
}

/** Dynamic LDS of one workgroup of the wave kernel: H [n][n] and the factor [n][ld]. */
__host__ __device__ inline size_t waveLdsBytes(int n)
{
  return (static_cast<size_t>(n) * n + static_cast<size_t>(waveFactorLd(n)) * n) * sizeof(double);
}

__device__ __forceinline__ unsigned long long bitsAbove(int k)
{
  return ~((2ull << k) - 1ull); // bits k + 1 .. 63 (k = 63: 2 << 63 wraps to 0, so none)
}

__device__ __forceinline__ void writeTraceRow(const Results & out, const Params & p, size_t b, int row, double obj, int factorization_num,
                                              int step_num, unsigned long long clamped, double grad_norm)
{
  if(row < p.trace_capacity)
  {
    double * t = out.trace + (b * p.trace_capacity + row) * kTraceColumns;
    t[0] = row;
    t[1] = obj;
    t[2] = factorization_num;
    t[3] = step_num;
    t[4] = __longlong_as_double(static_cast<long long>(clamped)); // the mask's bits, not its value
    t[5] = grad_norm;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// layout conversion for the lane kernel
// ---------------------------------------------------------------------------------------------------------------------------
/** dst[e'][b] = src[b][e] for e < E; with rows > 0 the E = rows * rows entries are a row-major matrix that is stored column-major
    (e = i * rows + j -> e' = i + j * rows).  src == nullptr stores zeros (initial_x = NULL). */
__global__ void boxqp_ingest_kernel(const double * __restrict__ src, double * __restrict__ dst, size_t B, int E, int rows)
{
  const size_t t = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if(t >= B * static_cast<size_t>(E))
  {
    return;
  }
  const size_t b = t % B;
  const int e = static_cast<int>(t / B);
  const int ed = rows > 0 ? (e / rows) + (e % rows) * rows : e;
  dst[static_cast<size_t>(ed) * B + b] = src ? src[b * E + e] : 0.0;
}

/** dst[b][e] = src[e][b]: the transposing store of X and FACTOR (both already in the boundary's element order). */
__global__ void boxqp_egress_kernel(const double * __restrict__ src, double * __restrict__ dst, size_t B, int E)
{
  const size_t t = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if(t >= B * static_cast<size_t>(E))
  {
    return;
  }
  const size_t b = t % B;
  const size_t e = t / B;
  dst[b * E + e] = src[e * B + b];
}

// ---------------------------------------------------------------------------------------------------------------------------
// lane kernel
// ---------------------------------------------------------------------------------------------------------------------------
/** Inputs and workspace of the lane kernel, all [element][instance] (H and fac column-major: element i + j * n). */
struct LaneBuffers
{
  const double * H; // [n*n][B]
  const double * g; // [n][B]
  const double * lower;
  const double * upper;
  const double * x0;
  double * x; // [n][B]  the iterate, and the result
  double * grad; // [n][B]
  double * dir; // [n][B]  right-hand side, then the search direction
  double * cand; // [n][B]
  double * fac; // [n*n][B]  unpacked factor
  double * factor_out; // [n*n][B]  FACTOR in the boundary's element order (r * n + c)
};

__global__ void __launch_bounds__(kLaneBlock) boxqp_lane_kernel(LaneBuffers bf, Results out, Params p, int n, size_t B)
{
  const size_t b = static_cast<size_t>(blockIdx.x) * kLaneBlock + threadIdx.x;
  if(b >= B)
  {
    return;
  }
  const double * H = bf.H + b;
  const double * g = bf.g + b;
  const double * lower = bf.lower + b;
  const double * upper = bf.upper + b;
  double * x = bf.x + b;
  double * grad = bf.grad + b;
  double * dir = bf.dir + b;
  double * cand = bf.cand + b;
  double * fac = bf.fac + b;
  const unsigned long long live = n == 64 ? ~0ull : ((1ull << n) - 1ull);
  // element e of an [element][instance] array
#define BOXQP_AT(ptr, e) (ptr)[static_cast<size_t>(e) * B]

  // v.dot(g) + 0.5 * v.dot(H * v)    BoxQP.h:149, 297
  auto objective = [&](const double * v) {
    double vg = 0, vhv = 0;
    for(int i = 0; i < n; i++)
    {
      double hv = 0;
      for(int j = 0; j < n; j++)
      {
        hv += BOXQP_AT(H, i + j * n) * BOXQP_AT(v, j);
      }
      vg += BOXQP_AT(v, i) * BOXQP_AT(g, i);
      vhv += BOXQP_AT(v, i) * hv;
    }
    return vg + 0.5 * vhv;
  };

  for(int i = 0; i < n; i++)
  {
    BOXQP_AT(x, i) = fmax(fmin(BOXQP_AT(bf.x0 + b, i), BOXQP_AT(upper, i)), BOXQP_AT(lower, i)); // BoxQP.h:148
  }
  double obj = objective(x);
  double old_obj = obj;
  writeTraceRow(out, p, b, 0, obj, 0, 0, 0ull, 0.0); // BoxQP.h:154-158

  int retval = 0;
  int factorization_num = 0;
  unsigned long long clamped = 0, old_clamped = 0, free_mask = 0;
  int iter = 1;
  for(;; iter++)
  {
    // relative improvement    BoxQP.h:176-181
    if(iter > 1 && (old_obj - obj) < p.rel_improve_thre * fabs(old_obj))
    {
      retval = 4;
      break;
    }
    old_obj = obj;

    // gradient, clamped and free sets (exact == compare)    BoxQP.h:184-206
    old_clamped = clamped;
    clamped = 0;
    for(int i = 0; i < n; i++)
    {
      double hx = 0;
      for(int j = 0; j < n; j++)
      {
        hx += BOXQP_AT(H, i + j * n) * BOXQP_AT(x, j);
      }
      const double gi = BOXQP_AT(g, i) + hx;
      BOXQP_AT(grad, i) = gi;
      const double xi = BOXQP_AT(x, i);
      if((xi == BOXQP_AT(lower, i) && gi > 0) || (xi == BOXQP_AT(upper, i) && gi < 0))
      {
        clamped |= 1ull << i;
      }
    }
    free_mask = ~clamped & live;
    if(free_mask == 0) // BoxQP.h:209-213
    {
      retval = 6;
      break;
    }

    // factorise the free block iff the clamped set changed    BoxQP.h:216-241
    if(iter == 1 || clamped != old_clamped)
    {
      for(unsigned long long mj = free_mask; mj; mj &= mj - 1)
      {
        const int j = __builtin_ctzll(mj);
        for(unsigned long long mi = mj; mi; mi &= mi - 1) // rows i >= j: the lower triangle
        {
          const int i = __builtin_ctzll(mi);
          BOXQP_AT(fac, i + j * n) = BOXQP_AT(H, i + j * n);
        }
      }
      bool positive = true;
      for(unsigned long long mk = free_mask; mk; mk &= mk - 1)
      {
        const int k = __builtin_ctzll(mk);
        const double d = BOXQP_AT(fac, k + k * n);
        if(!(d > 0))
        {
          positive = false;
          break;
        }
        const double s = sqrt(d);
        BOXQP_AT(fac, k + k * n) = s;
        const unsigned long long below = free_mask & bitsAbove(k);
        for(unsigned long long mi = below; mi; mi &= mi - 1)
        {
          const int i = __builtin_ctzll(mi);
          BOXQP_AT(fac, i + k * n) = BOXQP_AT(fac, i + k * n) / s;
        }
        for(unsigned long long mj = below; mj; mj &= mj - 1)
        {
          const int j = __builtin_ctzll(mj);
          const double ljk = BOXQP_AT(fac, j + k * n);
          for(unsigned long long mi = mj; mi; mi &= mi - 1)
          {
            const int i = __builtin_ctzll(mi);
            BOXQP_AT(fac, i + j * n) -= BOXQP_AT(fac, i + k * n) * ljk;
          }
        }
      }
      if(!positive)
      {
        retval = -1;
        break;
      }
      factorization_num++;
    }

    // free gradient norm    BoxQP.h:244-253
    double grad_norm = 0;
    for(unsigned long long mi = free_mask; mi; mi &= mi - 1)
    {
      const double gi = BOXQP_AT(grad, __builtin_ctzll(mi));
      grad_norm += gi * gi;
    }
    if(grad_norm < p.grad_thre * p.grad_thre)
    {
      retval = 5;
      break;
    }

    // Newton direction on the free dimensions    BoxQP.h:256-279
    for(unsigned long long mi = free_mask; mi; mi &= mi - 1)
    {
      const int i = __builtin_ctzll(mi);
      double s = 0;
      for(unsigned long long mj = clamped; mj; mj &= mj - 1)
      {
        const int j = __builtin_ctzll(mj);
        s += BOXQP_AT(H, i + j * n) * BOXQP_AT(x, j);
      }
      BOXQP_AT(dir, i) = BOXQP_AT(g, i) + s;
    }
    for(unsigned long long mk = free_mask; mk; mk &= mk - 1) // L y = rhs, column-oriented
    {
      const int k = __builtin_ctzll(mk);
      const double yk = BOXQP_AT(dir, k) / BOXQP_AT(fac, k + k * n);
      BOXQP_AT(dir, k) = yk;
      for(unsigned long long mi = free_mask & bitsAbove(k); mi; mi &= mi - 1)
      {
        const int i = __builtin_ctzll(mi);
        BOXQP_AT(dir, i) -= BOXQP_AT(fac, i + k * n) * yk;
      }
    }
    for(unsigned long long mk = free_mask; mk;) // L' z = y, column-oriented (descending k)
    {
      const int k = 63 - __builtin_clzll(mk);
      mk &= ~(1ull << k);
      const double zk = BOXQP_AT(dir, k) / BOXQP_AT(fac, k + k * n);
      BOXQP_AT(dir, k) = zk;
      for(unsigned long long mi = mk; mi; mi &= mi - 1) // the free i < k
      {
        const int i = __builtin_ctzll(mi);
        BOXQP_AT(dir, i) -= BOXQP_AT(fac, k + i * n) * zk;
      }
    }
    double sdg = 0; // search_dir.dot(grad)    BoxQP.h:282
    for(int i = 0; i < n; i++)
    {
      const double sd = ((free_mask >> i) & 1ull) ? -1 * BOXQP_AT(dir, i) - BOXQP_AT(x, i) : 0.0;
      BOXQP_AT(dir, i) = sd;
      sdg += sd * BOXQP_AT(grad, i);
    }
    if(sdg > 1e-10) // BoxQP.h:283-291
    {
      retval = -2;
      break;
    }

    // Armijo line search with projection    BoxQP.h:294-309
    double step = 1;
    int step_num = 0;
    for(int i = 0; i < n; i++)
    {
      BOXQP_AT(cand, i) = fmax(fmin(BOXQP_AT(x, i) + step * BOXQP_AT(dir, i), BOXQP_AT(upper, i)), BOXQP_AT(lower, i));
    }
    double obj_cand = objective(cand);
    // (0 / 0 or x / 0 at the Newton point: the comparison is false and the step is taken, as in the reference)
    while((obj_cand - old_obj) / (step * sdg) < p.armijo_param)
    {
      step = step * p.step_factor;
      step_num++;
      for(int i = 0; i < n; i++)
      {
        BOXQP_AT(cand, i) = fmax(fmin(BOXQP_AT(x, i) + step * BOXQP_AT(dir, i), BOXQP_AT(upper, i)), BOXQP_AT(lower, i));
      }
      obj_cand = objective(cand);
      if(step < p.min_step)
      {
        retval = 2; // leaves only the inner loop (BoxQP.h:304-308)
        break;
      }
    }

    writeTraceRow(out, p, b, iter, obj, factorization_num, step_num, clamped, grad_norm); // BoxQP.h:320-325

    // accept    BoxQP.h:328-329
    for(int i = 0; i < n; i++)
    {
      BOXQP_AT(x, i) = BOXQP_AT(cand, i);
    }
    obj = obj_cand;
    if(iter == p.max_iter) // BoxQP.h:332-336
    {
      retval = 1;
      break;
    }
  }
  if(retval != 1)
  {
    writeTraceRow(out, p, b, iter, 0.0, 0, 0, 0ull, 0.0); // the entry of the iteration that left the loop: iter only (BoxQP.h:171-173)
  }

  out.retval[b] = retval;
  out.iter[b] = iter;
  out.factorization_num[b] = factorization_num;
  out.free_mask[b] = free_mask;
  out.obj[b] = obj;
  // FACTOR: the factor packed in free_idxs_ order, zeros elsewhere
  double * fo = bf.factor_out + b;
  for(int e = 0; e < n * n; e++)
  {
    BOXQP_AT(fo, e) = 0.0;
  }
  if(factorization_num > 0)
  {
    int r = 0;
    for(unsigned long long mi = free_mask; mi; mi &= mi - 1, r++)
    {
      const int i = __builtin_ctzll(mi);
      int c = 0;
      for(unsigned long long mj = free_mask; c <= r; mj &= mj - 1, c++)
      {
        BOXQP_AT(fo, r * n + c) = BOXQP_AT(fac, i + __builtin_ctzll(mj) * n);
      }
    }
  }
#undef BOXQP_AT
}

// ---------------------------------------------------------------------------------------------------------------------------
// wave kernel
// ---------------------------------------------------------------------------------------------------------------------------
/** v of lane `lane` (wave-uniform) in every lane: two v_readlane_b32. */
__device__ __forceinline__ double bcastLane(double v, int lane)
{
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
  return __hiloint2double(hi, lo);
}

/** Sum over the 64 lanes by a butterfly; every lane gets the same bits (each level adds the same two numbers in both partners,
    and fp addition is commutative), read back from lane 0 so that the compiler knows the value is uniform. */
__device__ __forceinline__ double waveSum(double v)
{
#pragma unroll
  for(int s = 32; s >= 1; s >>= 1)
  {
    v += __shfl_xor(v, s, 64);
  }
  return bcastLane(v, 0);
}

/** The lanes of the one wavefront of this workgroup hand data to each other through LDS: the writes have to be complete and the
    compiler must not move LDS accesses across this point.  (A 64-thread workgroup: the barrier costs no waiting.) */
__device__ __forceinline__ void waveLdsSync()
{
  __syncthreads();
}

/** Inputs in the BOUNDARY layout (the wave kernel needs no ingest); X and FACTOR are written in it too. */
struct WaveBuffers
{
  const double * H; // [B][n][n]
  const double * g; // [B][n]
  const double * lower;
  const double * upper;
  const double * x0; // [B][n] or nullptr = zeros
  double * x; // [B][n]
  double * factor; // [B][n][n]
};

__global__ void __launch_bounds__(64) boxqp_wave_kernel(WaveBuffers bf, Results out, Params p, int n)
{
  extern __shared__ __attribute__((aligned(16))) double lds_boxqp[];
  const size_t b = blockIdx.x;
  const int l = threadIdx.x;
  const int ld = waveFactorLd(n);
  double * Hs = lds_boxqp; // H(i, j) at [i + j * n]
  double * F = lds_boxqp + n * n; // factor (i, j) at [i + j * ld]
  const bool is_live = l < n; // lanes l >= n own no variable: they add 0 to every sum and vote false in every ballot
  const int row = is_live ? l : 0; // (an in-bounds LDS address for the idle lanes; what they read is never used)
  const unsigned long long live = n == 64 ? ~0ull : ((1ull << n) - 1ull);

  // H into LDS.  The boundary layout has row i contiguous: the lanes read it along j (coalesced, 8-byte loads: the rows of an odd n
  // are only 8-byte aligned) and store it transposed.  Every later access of Hs is a lane's own row.
  {
    const double * Hb = bf.H + b * n * n;
    for(int i = 0; i < n; i++)
    {
      if(is_live)
      {
        Hs[i + l * n] = Hb[i * n + l];
      }
    }
  }
  const double g = is_live ? bf.g[b * n + l] : 0.0;
  const double lower = is_live ? bf.lower[b * n + l] : 0.0;
  const double upper = is_live ? bf.upper[b * n + l] : 0.0;
  const double x_init = (is_live && bf.x0) ? bf.x0[b * n + l] : 0.0;
  waveLdsSync(); // Hs written along columns by other lanes than those that read its rows

  // (H v)_l, the reference's order: column by column, j ascending    BoxQP.h:149, 184, 297
  auto Hv = [&](double v) {
    double s = 0;
    for(int j = 0; j < n; j++)
    {
      s += Hs[row + j * n] * bcastLane(v, j);
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
  if(l == 0)
  {
    writeTraceRow(out, p, b, 0, obj, 0, 0, 0ull, 0.0); // BoxQP.h:154-158
  }

  int retval = 0;
  int factorization_num = 0;
  unsigned long long clamped = 0, old_clamped = 0, free_mask = 0;
  bool is_free = false;
  double diag = 1.0; // L(l, l) of the current factor
  int iter = 1;
  for(;; iter++)
  {
    // relative improvement    BoxQP.h:176-181
    if(iter > 1 && (old_obj - obj) < p.rel_improve_thre * fabs(old_obj))
    {
      retval = 4;
      break;
    }
    old_obj = obj;

    // gradient, clamped and free sets (exact == compare)    BoxQP.h:184-206
    const double hx = Hv(x);
    const double grad = is_live ? g + hx : 0.0;
    old_clamped = clamped;
    clamped = __ballot(is_live && ((x == lower && grad > 0) || (x == upper && grad < 0)));
    free_mask = ~clamped & live;
    is_free = (free_mask >> l) & 1ull;
    if(free_mask == 0) // all clamped among the LIVE lanes    BoxQP.h:209-213
    {
      retval = 6;
      break;
    }

    // factorise the free block iff the clamped set changed    BoxQP.h:216-241
    if(iter == 1 || clamped != old_clamped)
    {
      waveLdsSync(); // the last back substitution read rows of F across the lanes
      for(unsigned long long mj = free_mask; mj; mj &= mj - 1)
      {
        const int j = __builtin_ctzll(mj);
        if(is_free && l >= j) // the lower triangle
        {
          F[l + j * ld] = Hs[l + j * n];
        }
      }
      bool positive = true;
      for(unsigned long long mk = free_mask; mk; mk &= mk - 1)
      {
        const int k = __builtin_ctzll(mk);
        const bool below = is_free && l >= k;
        double lik = below ? F[l + k * ld] : 0.0;
        const double d = bcastLane(lik, k);
        if(!(d > 0))
        {
          positive = false;
          break;
        }
        const double s = sqrt(d);
        lik = (l == k) ? s : lik / s;
        if(below)
        {
          F[l + k * ld] = lik;
        }
        if(l == k)
        {
          diag = s;
        }
        for(unsigned long long mj = mk & (mk - 1); mj; mj &= mj - 1) // the free j > k
        {
          const int j = __builtin_ctzll(mj);
          const double ljk = bcastLane(lik, j);
          if(is_free && l >= j)
          {
            F[l + j * ld] -= lik * ljk;
          }
        }
      }
      waveLdsSync(); // F complete before a lane reads another lane's row
      if(!positive)
      {
        retval = -1;
        break;
      }
      factorization_num++;
    }

    // free gradient norm    BoxQP.h:244-253
    const double grad_norm = waveSum(is_free ? grad * grad : 0.0);
    if(grad_norm < p.grad_thre * p.grad_thre)
    {
      retval = 5;
      break;
    }

    // Newton direction on the free dimensions    BoxQP.h:256-279
    double r = 0;
    for(unsigned long long mj = clamped; mj; mj &= mj - 1)
    {
      const int j = __builtin_ctzll(mj);
      r += Hs[row + j * n] * bcastLane(x, j);
    }
    r = g + r;
    for(unsigned long long mk = free_mask; mk; mk &= mk - 1) // L y = rhs, column-oriented
    {
      const int k = __builtin_ctzll(mk);
      if(l == k)
      {
        r = r / diag;
      }
      const double yk = bcastLane(r, k);
      if(is_free && l > k)
      {
        r -= F[l + k * ld] * yk;
      }
    }
    for(unsigned long long mk = free_mask; mk;) // L' z = y, column-oriented (descending k): row k of L across the lanes
    {
      const int k = 63 - __builtin_clzll(mk);
      mk &= ~(1ull << k);
      if(l == k)
      {
        r = r / diag;
      }
      const double zk = bcastLane(r, k);
      if(is_free && l < k)
      {
        r -= F[k + l * ld] * zk;
      }
    }
    const double dir = is_free ? -1 * r - x : 0.0;

    // descent check    BoxQP.h:282-291
    const double sdg = waveSum(dir * grad);
    if(sdg > 1e-10)
    {
      retval = -2;
      break;
    }

    // Armijo line search with projection    BoxQP.h:294-309
    double step = 1;
    int step_num = 0;
    double cand = is_live ? fmax(fmin(x + step * dir, upper), lower) : 0.0;
    double obj_cand = objective(cand);
    // (0 / 0 or x / 0 at the Newton point: the comparison is false and the step is taken, as in the reference)
    while((obj_cand - old_obj) / (step * sdg) < p.armijo_param)
    {
      step = step * p.step_factor;
      step_num++;
      cand = is_live ? fmax(fmin(x + step * dir, upper), lower) : 0.0;
      obj_cand = objective(cand);
      if(step < p.min_step)
      {
        retval = 2; // leaves only the inner loop (BoxQP.h:304-308)
        break;
      }
    }

    if(l == 0)
    {
      writeTraceRow(out, p, b, iter, obj, factorization_num, step_num, clamped, grad_norm); // BoxQP.h:320-325
    }

    // accept    BoxQP.h:328-329
    x = cand;
    obj = obj_cand;
    if(iter == p.max_iter) // BoxQP.h:332-336
    {
      retval = 1;
      break;
    }
  }

  if(l == 0)
  {
    if(retval != 1)
    {
      writeTraceRow(out, p, b, iter, 0.0, 0, 0, 0ull, 0.0); // the entry of the iteration that left the loop: iter only (BoxQP.h:171-173)
    }
    out.retval[b] = retval;
    out.iter[b] = iter;
    out.factorization_num[b] = factorization_num;
    out.free_mask[b] = free_mask;
    out.obj[b] = obj;
  }
  if(is_live)
  {
    bf.x[b * n + l] = x;
  }
  // FACTOR: lane r writes row r of the packed factor — row src of F, where src is the r-th free index — and zeros elsewhere
  const int nf = factorization_num > 0 ? __popcll(free_mask) : 0;
  int src = 0;
  {
    int r = 0;
    for(unsigned long long mi = free_mask; mi; mi &= mi - 1, r++)
    {
      if(r == l)
      {
        src = __builtin_ctzll(mi);
      }
    }
  }
  if(is_live)
  {
    double * fo = bf.factor + (b * n + l) * n;
    unsigned long long mj = free_mask;
    for(int c = 0; c < n; c++)
    {
      double v = 0.0;
      if(l < nf && c <= l)
      {
        v = F[src + __builtin_ctzll(mj) * ld];
        mj &= mj - 1;
      }
      fo[c] = v;
    }
  }
}
} // namespace boxqp
} // namespace hip
} // namespace nmpc_amd
