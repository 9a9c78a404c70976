// gfx950 "wave" kernels of the batched C/GMRES solver: one wavefront (one 64-thread workgroup) per controller, the whole tick in
// LDS.  The second kernel family beside the lane kernels of cgmres_kernels.hpp (one lane per controller, every list in HBM); it
// reads and writes the same handle arrays and returns the same bits, so a caller may switch kernels between calls.
//
// Why: the lane kernel's tick is the memory-latency chain of one lane (about eight horizon evaluations of 2 N dependent model
// steps, each storing and reloading the lists through HBM) and takes as long for 64 controllers as for 16 384.  Here nothing inside
// a tick goes to HBM.
//
// Lane roles inside a tick (every phase ends in a workgroup barrier; the workgroup is one wavefront):
//   chain lanes       the forward ODE steps and backward costate steps of a horizon evaluation are sequential and stay on ONE
//                     lane.  The three evaluations at the start of a tick do not depend on each other (DhDu at (t, x), DhDu at
//                     (t + delta, x_with_delta) and the A delta_u of GMRES's initial residual): lanes 0, 1, 2 run them in lockstep,
//                     each into its own chain slot (state list, costate list, per-step times).  Inside the Arnoldi loop lane 0
//                     runs the one evaluation of the step.  The dependent chain of a tick is 1 + k evaluations instead of 3 + k.
//   calcDhDu          the N calcDhDu of an evaluation need only (x_i, u_i, lmd_{i+1}, tau_i), all in LDS after the chain: one lane
//                     per (evaluation, step), off the chain.
//   element loops     the right-hand side, the Gram-Schmidt updates, the normalisation, x += V y and U += dt du: element e on lane
//                     e % 64.
//   ordered scalars   every sum (dot products, norms, the sum of squares behind err) accumulates from 0 over e = 0 .. n - 1 as
//                     cgmres_kernels.hpp's dot() writes it, and EVERY lane does so from LDS (same-address reads are a broadcast),
//                     as every lane does the Givens updates and the triangular solve: all 64 lanes hold the same bits, the loop
//                     conditions of GMRES are wave-uniform without a broadcast, and no reduction reorders a sum.
//
// Bits: the ODE steps (Lane::odeStep / stateStep), loadU and the problem functions are the lane kernel's own device functions,
// called with the same arguments; this translation unit is compiled with -ffp-contract=off like the lane kernels' (nmpc_amd/build.py).
// Element-wise operations carry no order; the sums, tau += step / tau -= step, t += dt, the Givens updates, the triangular solve
// and the accumulation of x += V y over i keep the lane kernel's order.
//
// LDS of one workgroup, in doubles (n = N dim_uc, K = the configured k_max, NX = dim_x):
//   U, DhDu, DhDu_with_delta, delta_u                                4 n
//   3 chain slots: x list (N + 1) NX, costate list N NX, times N     3 ((2 N + 1) NX + N)
//   GMRES workspace b, w, V [K + 1], R [K][K], g [K + 1], c, s [K]   (K + 3) n + K K + 3 K + 1   (gmresWorkspaceElems(n, K))
// waveLdsBytes() = 8 * the sum: 13 024 B for the bounded cart-pole at N = 25, k_max = 5, 21 736 B at k_max = 16.  A shape above
// 64 KiB is refused by the C-ABI (nmpc_hip_cgmres_set_kernel / set_config); no raised LDS limit is requested.
#pragma once

#include <nmpc_amd/hip/cgmres_kernels.hpp>

namespace nmpc_amd
{
namespace hip
{
namespace cgmres
{
constexpr size_t kWaveMaxLdsBytes = 65536;

/** Doubles of one chain slot: the state list, the costate list and the per-step times of one horizon evaluation. */
NMPC_HD size_t waveChainElems(int N, int nx)
{
  return static_cast<size_t>(2 * static_cast<size_t>(N) + 1) * nx + static_cast<size_t>(N);
}

/** LDS bytes of one workgroup of the wave kernels (formula above). */
NMPC_HD size_t waveLdsBytes(int N, int nx, int nuc, int k_max)
{
  const size_t n = static_cast<size_t>(N) * nuc;
  return sizeof(double) * (4 * n + 3 * waveChainElems(N, nx) + gmresWorkspaceElems(static_cast<int>(n), k_max));
}

#ifdef __HIPCC__
/** One controller on one wavefront.  Every member function is called by all 64 lanes (wave-uniform control flow). */
template<class P>
struct Wave
{
  static constexpr int NX = P::dim_x_, NUC = P::dim_uc_;
  const Lane<P> & ln; //!< the lane kernel's device functions on this controller's problem object
  double * lds;
  int lane;

  __device__ int n() const
  {
    return ln.bf.N * NUC;
  }
  __device__ Vec vec(size_t off) const
  {
    return Vec{lds + off, 1};
  }
  __device__ Vec U() const
  {
    return vec(0);
  }
  __device__ Vec D() const
  {
    return vec(n());
  }
  __device__ Vec Dw() const
  {
    return vec(2 * static_cast<size_t>(n()));
  }
  __device__ Vec du() const
  {
    return vec(3 * static_cast<size_t>(n()));
  }
  __device__ double * slot(int c) const
  {
    return lds + 4 * static_cast<size_t>(n()) + c * waveChainElems(ln.bf.N, NX);
  }
  __device__ GmresWs ws() const
  {
    return GmresWs{lds + 4 * static_cast<size_t>(n()) + 3 * waveChainElems(ln.bf.N, NX), 1, n(), ln.bf.k_max};
  }

  /** Input column i of U (use_v false) or of U + delta v (use_v true).  use_v may differ between lanes: both are Lane::loadU's
      results and the lane keeps the one it needs, so that lanes evaluating different lists stay in lockstep. */
  __device__ void inputAt(const Vec & v, bool use_v, double delta, int i, double * u) const
  {
    double up[NUC], uv[NUC];
    ln.loadU(U(), nullptr, delta, i, up);
    ln.loadU(U(), &v, delta, i, uv);
    NMPC_UNROLL
    for(int j = 0; j < NUC; j++)
    {
      u[j] = use_v ? uv[j] : up[j];
    }
  }

  /** The sequential part of CgmresSolver::calcDhDuList at (t, x0) for the input list U (+ delta v when use_v), on the calling lane
      alone: the state list, the costate each calcDhDu needs and its time go to the chain slot. */
  __device__ void chain(double * sl, double t, const double * x0, const Vec & v, bool use_v, double delta) const
  {
    const CgmresBuffers & bf = ln.bf;
    const int N = bf.N;
    const double horizon_duration = bf.steady_horizon_duration * (1.0 - exp(-bf.horizon_increase_ratio * t));
    const double step = horizon_duration / N;
    double * xl = sl;
    double * ll = sl + static_cast<size_t>(N + 1) * NX;
    double * taus = ll + static_cast<size_t>(N) * NX;
    double x[NX];
    NMPC_UNROLL
    for(int a = 0; a < NX; a++)
    {
      x[a] = x0[a];
      xl[a] = x[a];
    }
    double tau = t;
    for(int i = 0; i < N; i++)
    {
      double u[NUC], xn[NX];
      inputAt(v, use_v, delta, i, u);
      ln.stateStep(bf.horizon_solver, tau, x, u, step, xn);
      NMPC_UNROLL
      for(int a = 0; a < NX; a++)
      {
        x[a] = xn[a];
        xl[(i + 1) * NX + a] = x[a];
      }
      tau += step;
    }
    double lmd[NX];
    ln.prob.calcDphiDx(tau, x, lmd);
    const P & p = ln.prob;
    for(int i = N - 1; i >= 0; i--)
    {
      double xu[NX + NUC], lmd_prev[NX];
      NMPC_UNROLL
      for(int a = 0; a < NX; a++)
      {
        xu[a] = xl[i * NX + a];
        ll[i * NX + a] = lmd[a];
      }
      inputAt(v, use_v, delta, i, xu + NX);
      Lane<P>::template odeStep<NX>(
          bf.horizon_solver, [&p](double tt, const double * y, const double * a, double * dy) { p.costateEquation(tt, y, a, dy); }, tau,
          lmd, xu, -step, lmd_prev);
      tau -= step;
      taus[i] = tau;
      NMPC_UNROLL
      for(int a = 0; a < NX; a++)
      {
        lmd[a] = lmd_prev[a];
      }
    }
  }

  /** calcDhDu of step i of the evaluation in chain slot sl; sub, when given, turns the result into eqAmulFunc's (. - sub) / delta. */
  __device__ void dhduStep(const double * sl, int i, const Vec & v, bool use_v, double delta, const Vec & out, const Vec * sub) const
  {
    const int N = ln.bf.N;
    const double * xl = sl;
    const double * ll = sl + static_cast<size_t>(N + 1) * NX;
    const double * taus = ll + static_cast<size_t>(N) * NX;
    double xu[NX + NUC], lmd[NX], dhdu[NUC];
    NMPC_UNROLL
    for(int a = 0; a < NX; a++)
    {
      xu[a] = xl[i * NX + a];
      lmd[a] = ll[i * NX + a];
    }
    inputAt(v, use_v, delta, i, xu + NX);
    ln.prob.calcDhDu(taus[i], xu, xu + NX, lmd, dhdu);
    NMPC_UNROLL
    for(int j = 0; j < NUC; j++)
    {
      out[i * NUC + j] = sub ? (dhdu[j] - (*sub)[i * NUC + j]) / delta : dhdu[j];
    }
  }

  /** Element-wise v / |v| (z = v . v, summed in order by the caller), a zero vector unchanged; out may be v. */
  __device__ void normalizedInto(const Vec & v, double z, const Vec & out) const
  {
    const int nn = n();
    if(z > 0)
    {
      const double nrm = sqrt(z);
      for(int e = lane; e < nn; e += kBlock)
      {
        out[e] = v[e] / nrm;
      }
    }
    else
    {
      for(int e = lane; e < nn; e += kBlock)
      {
        out[e] = v[e];
      }
    }
    __syncthreads();
  }

  /** One pass of modified Gram-Schmidt of w against v_0 .. v_{k-1}; add = the re-orthogonalisation's R += h. */
  __device__ void gramSchmidt(const GmresWs & W, int k, int col, bool add) const
  {
    const int nn = n();
    const Vec w = W.w(), R = W.R();
    for(int j = 0; j < k; j++)
    {
      const Vec vj = W.V(j);
      const double h = dot(w, vj, nn);
      R[col + j] = add ? R[col + j] + h : h;
      __syncthreads(); // every lane has read w
      for(int e = lane; e < nn; e += kBlock)
      {
        w[e] = w[e] - h * vj[e];
      }
      __syncthreads();
    }
  }

  /** CgmresSolver::calcControlInput(t, x, next_x, u) on the LDS-resident U and delta_u (Lane::controlInput with gmresSolve written
      out for 64 lanes).  x, next_x and the results are the same in every lane. */
  __device__ void controlInput(double t, const double * x, const double * next_x, double * u, double & err, int & iters, int & reorth) const
  {
    const CgmresBuffers & bf = ln.bf;
    const int nn = n(), N = bf.N;
    const double delta = bf.finite_diff_delta;
    const Vec Uv = U(), Dv = D(), Dwv = Dw(), duv = du();
    const GmresWs W = ws();
    const Vec rhs = W.b(), w = W.w(), R = W.R(), g = W.g(), cs = W.c(), sn = W.s();
    const double t_wd = t + delta;
    const double a0 = 1 - delta / bf.dt, a1 = delta / bf.dt;
    double x_wd[NX];
    NMPC_UNROLL
    for(int a = 0; a < NX; a++)
    {
      x_wd[a] = a0 * x[a] + a1 * next_x[a];
    }
    // 1.1, 1.2 and the A delta_u of GMRES's step 1: three independent evaluations, lanes 0, 1, 2
    if(lane < 3)
    {
      double x0[NX];
      NMPC_UNROLL
      for(int a = 0; a < NX; a++)
      {
        x0[a] = lane == 0 ? x[a] : x_wd[a];
      }
      chain(slot(lane), lane == 0 ? t : t_wd, x0, duv, lane == 2, delta);
    }
    __syncthreads();
    for(int task = lane; task < 3 * N; task += kBlock)
    {
      const int c = task / N, i = task - c * N;
      dhduStep(slot(c), i, duv, c == 2, delta, c == 0 ? Dv : (c == 1 ? Dwv : w), nullptr);
    }
    __syncthreads();
    // 2.1 b = ((1 - zeta delta) DhDu - DhDu_with_delta) / delta; w = A delta_u; v_1 = b - w (unnormalised)
    const double zd = 1 - bf.eq_zeta * delta;
    const Vec v0 = W.V(0);
    for(int e = lane; e < nn; e += kBlock)
    {
      const double d = Dv[e], dw = Dwv[e];
      const double be = (zd * d - dw) / delta;
      const double we = (w[e] - dw) / delta;
      rhs[e] = be;
      v0[e] = be - we;
    }
    double sq = 0;
    for(int e = 0; e < nn; e++)
    {
      const double d = Dv[e];
      sq += d * d;
    }
    err = sqrt(sq);
    __syncthreads();
    // 2.2 gmresSolve (cgmres_kernels.hpp) from its step 1 on
    int k_max = bf.k_max < nn ? bf.k_max : nn;
    k_max = k_max < W.K ? k_max : W.K;
    const double z0 = dot(v0, v0, nn);
    double rho = sqrt(z0);
    __syncthreads(); // every lane has read v_1
    normalizedInto(v0, z0, v0);
    for(int i = 0; i <= k_max; i++)
    {
      g[i] = 0;
    }
    g[0] = rho;
    const double b_norm = sqrt(dot(rhs, rhs, nn));
    int k = 0;
    reorth = 0;
    while(rho > 1e-10 * b_norm && k < k_max)
    {
      k++;
      // (b) w = A v_k: eqAmulFunc
      const Vec vk = W.V(k - 1);
      if(lane == 0)
      {
        chain(slot(0), t_wd, x_wd, vk, true, delta);
      }
      __syncthreads();
      for(int i = lane; i < N; i += kBlock)
      {
        dhduStep(slot(0), i, vk, true, delta, w, &Dwv);
      }
      __syncthreads();
      const int col = (k - 1) * W.K;
      const double Avk_norm = sqrt(dot(w, w, nn));
      gramSchmidt(W, k, col, false);
      // (c)
      double z = dot(w, w, nn);
      const double new_basis_norm = sqrt(z);
      const double h_sub = new_basis_norm;
      // (d)
      if(Avk_norm + 1e-3 * new_basis_norm == Avk_norm)
      {
        reorth = 1;
        gramSchmidt(W, k, col, true);
        z = dot(w, w, nn);
      }
      // (e)
      normalizedInto(w, z, W.V(k));
      // (f), (g): every lane, the same values
      for(int i = 0; i < k - 1; i++)
      {
        const double h0 = R[col + i], h1 = R[col + i + 1];
        const double c = cs[i], s = sn[i];
        R[col + i] = c * h0 - s * h1;
        R[col + i + 1] = s * h0 + c * h1;
      }
      const double hd = R[col + k - 1];
      const double nu = sqrt(hd * hd + h_sub * h_sub);
      const double c_k = hd / nu, s_k = -h_sub / nu;
      cs[k - 1] = c_k;
      sn[k - 1] = s_k;
      R[col + k - 1] = c_k * hd - s_k * h_sub;
      const double g0 = g[k - 1], g1 = g[k];
      g[k - 1] = c_k * g0 - s_k * g1;
      g[k] = s_k * g0 + c_k * g1;
      rho = fabs(g[k]);
    }
    // 3. y = R^-1 g
    for(int i = k - 1; i >= 0; i--)
    {
      const double yi = g[i] / R[i * W.K + i];
      g[i] = yi;
      for(int j = 0; j < i; j++)
      {
        g[j] = g[j] - yi * R[i * W.K + j];
      }
    }
    __syncthreads();
    // 4. delta_u += V y (the accumulation over i in order), 2.3 U += dt delta_u
    for(int e = lane; e < nn; e += kBlock)
    {
      double xe = duv[e];
      for(int i = 0; i < k; i++)
      {
        xe = xe + g[i] * W.V(i)[e];
      }
      duv[e] = xe;
      Uv[e] = Uv[e] + bf.dt * xe;
    }
    iters = k;
    __syncthreads();
    NMPC_UNROLL
    for(int j = 0; j < NUC; j++)
    {
      u[j] = Uv[j];
    }
  }

  /** U and delta_u of the controller between the handle's [element][instance] arrays and LDS. */
  __device__ void loadLists() const
  {
    const CgmresBuffers & bf = ln.bf;
    const Vec Ug = ln.at(bf.U), dug = ln.at(bf.du), Uv = U(), duv = du();
    for(int e = lane; e < n(); e += kBlock)
    {
      Uv[e] = Ug[e];
      duv[e] = dug[e];
    }
    __syncthreads();
  }

  __device__ void storeLists() const
  {
    const CgmresBuffers & bf = ln.bf;
    const Vec Ug = ln.at(bf.U), dug = ln.at(bf.du), Uv = U(), duv = du();
    __syncthreads();
    for(int e = lane; e < n(); e += kBlock)
    {
      Ug[e] = Uv[e];
      dug[e] = duv[e];
    }
  }
};

extern __shared__ __align__(16) double cgmres_wave_lds[];

/** cgmres_run_kernel with one wavefront per controller: ticks i0 .. i0 + n_ticks - 1, x, u, U and delta_u on chip across them. */
template<class P>
__global__ void __launch_bounds__(kBlock) cgmres_wave_run_kernel(CgmresBuffers bf, int i0, int n_ticks, double t0)
{
  constexpr int NX = P::dim_x_, NUC = P::dim_uc_;
  const int b = blockIdx.x;
  const int lane = threadIdx.x;
  if(b >= bf.B || bf.status[b] == kStatusNonFinite || bf.status[b] == kStatusUninitialized)
  {
    return;
  }
  const P prob = loadProblem<P>(bf, b);
  const Lane<P> ln{prob, bf, b};
  const Wave<P> wv{ln, cgmres_wave_lds, lane};
  const Vec xv = ln.at(bf.x), uv = ln.at(bf.u);
  double x[NX], u[NUC];
  NMPC_UNROLL
  for(int a = 0; a < NX; a++)
  {
    x[a] = xv[a];
  }
  NMPC_UNROLL
  for(int j = 0; j < NUC; j++)
  {
    u[j] = uv[j];
  }
  wv.loadLists();
  double t = t0;
  double err = bf.err[b];
  int iters = bf.iters[b], reorth = bf.reorth[b];
  bool finite = true;
  for(int s = 0; s < n_ticks && finite; s++)
  {
    const int i = i0 + s;
    double next_x[NX];
    ln.stateStep(bf.sim_solver, t, x, u, bf.dt, next_x);
    wv.controlInput(t, x, next_x, u, err, iters, reorth);
    NMPC_UNROLL
    for(int a = 0; a < NX; a++)
    {
      x[a] = next_x[a];
      finite = finite && isfinite(x[a]);
    }
    NMPC_UNROLL
    for(int j = 0; j < NUC; j++)
    {
      finite = finite && isfinite(u[j]);
    }
    if(lane == 0 && bf.dump_step > 0 && i % bf.dump_step == 0)
    {
      const size_t row = static_cast<size_t>(i / bf.dump_step);
      if(row < static_cast<size_t>(bf.log_rows))
      {
        const size_t B = bf.B;
        NMPC_UNROLL
        for(int a = 0; a < NX; a++)
        {
          bf.log_x[(row * NX + a) * B + b] = x[a];
        }
        NMPC_UNROLL
        for(int j = 0; j < NUC; j++)
        {
          bf.log_u[(row * NUC + j) * B + b] = u[j];
        }
        bf.log_err[row * B + b] = err;
        bf.log_iters[row * B + b] = iters;
        bf.log_reorth[row * B + b] = reorth;
      }
    }
    t += bf.dt;
  }
  wv.storeLists();
  if(lane == 0)
  {
    NMPC_UNROLL
    for(int a = 0; a < NX; a++)
    {
      xv[a] = x[a];
    }
    NMPC_UNROLL
    for(int j = 0; j < NUC; j++)
    {
      uv[j] = u[j];
    }
    bf.err[b] = err;
    bf.iters[b] = iters;
    bf.reorth[b] = reorth;
    if(!finite)
    {
      bf.status[b] = kStatusNonFinite;
    }
  }
}

/** cgmres_control_input_kernel with one wavefront per controller. */
template<class P>
__global__ void __launch_bounds__(kBlock)
    cgmres_wave_control_input_kernel(CgmresBuffers bf, const double * t, const double * x_in, const double * next_x_in, double * u_out)
{
  constexpr int NX = P::dim_x_, NUC = P::dim_uc_;
  const int b = blockIdx.x;
  const int lane = threadIdx.x;
  if(b >= bf.B || bf.status[b] == kStatusNonFinite || bf.status[b] == kStatusUninitialized)
  {
    return;
  }
  const P prob = loadProblem<P>(bf, b);
  const Lane<P> ln{prob, bf, b};
  const Wave<P> wv{ln, cgmres_wave_lds, lane};
  double x[NX], next_x[NX], u[NUC];
  bool finite = true;
  NMPC_UNROLL
  for(int a = 0; a < NX; a++)
  {
    x[a] = x_in[static_cast<size_t>(b) * NX + a];
    next_x[a] = next_x_in[static_cast<size_t>(b) * NX + a];
  }
  wv.loadLists();
  double err = 0;
  int iters = 0, reorth = 0;
  wv.controlInput(t[b], x, next_x, u, err, iters, reorth);
  wv.storeLists();
  if(lane == 0)
  {
    const Vec uv = ln.at(bf.u);
    NMPC_UNROLL
    for(int j = 0; j < NUC; j++)
    {
      u_out[static_cast<size_t>(b) * NUC + j] = u[j];
      uv[j] = u[j];
      finite = finite && isfinite(u[j]);
    }
    bf.err[b] = err;
    bf.iters[b] = iters;
    bf.reorth[b] = reorth;
    if(!finite)
    {
      bf.status[b] = kStatusNonFinite;
    }
  }
}
#endif // __HIPCC__

/** What the C-ABI knows about the wave kernels of one registered problem type (looked up by name beside its CgmresOps). */
struct CgmresWaveOps
{
  const char * name;
  int nx, nuc;
  hipError_t (*launch_run)(const CgmresBuffers & bf, int i0, int n_ticks, double t0, size_t lds_bytes, hipStream_t stream);
  hipError_t (*launch_control_input)(const CgmresBuffers & bf, const double * t, const double * x, const double * next_x, double * u,
                                     size_t lds_bytes, hipStream_t stream);
};

#ifdef __HIPCC__
template<class P>
struct CgmresWaveOpsOf
{
  static CgmresWaveOps make()
  {
    CgmresWaveOps o{};
    o.name = P::kName;
    o.nx = P::dim_x_;
    o.nuc = P::dim_uc_;
    o.launch_run = [](const CgmresBuffers & bf, int i0, int n_ticks, double t0, size_t lds_bytes, hipStream_t stream) {
      hipLaunchKernelGGL(cgmres_wave_run_kernel<P>, dim3(static_cast<unsigned>(bf.B)), dim3(kBlock), lds_bytes, stream, bf, i0, n_ticks,
                         t0);
      return hipGetLastError();
    };
    o.launch_control_input = [](const CgmresBuffers & bf, const double * t, const double * x, const double * next_x, double * u,
                                size_t lds_bytes, hipStream_t stream) {
      hipLaunchKernelGGL(cgmres_wave_control_input_kernel<P>, dim3(static_cast<unsigned>(bf.B)), dim3(kBlock), lds_bytes, stream, bf, t, x,
                         next_x, u);
      return hipGetLastError();
    };
    return o;
  }
};
#endif
} // namespace cgmres
} // namespace hip
} // namespace nmpc_amd

extern "C" int nmpc_hip_cgmres_register_wave_model(const nmpc_amd::hip::cgmres::CgmresWaveOps * ops);

/** Make the wave kernels of a C/GMRES problem type available to nmpc_hip_cgmres_set_kernel(h, "wave").  Optional, beside
    NMPC_AMD_REGISTER_CGMRES_PROBLEM (which may live in another translation unit): a type registered only there runs on the lane
    kernels and is refused "wave".  Compile the translation unit with -ffp-contract=off. */
#define NMPC_AMD_REGISTER_CGMRES_WAVE_PROBLEM(ProblemType)                                                                  \
  namespace                                                                                                                 \
  {                                                                                                                         \
  struct ProblemType##CgmresWaveRegistrar                                                                                   \
  {                                                                                                                         \
    ProblemType##CgmresWaveRegistrar()                                                                                      \
    {                                                                                                                       \
      static const nmpc_amd::hip::cgmres::CgmresWaveOps ops = nmpc_amd::hip::cgmres::CgmresWaveOpsOf<ProblemType>::make(); \
      nmpc_hip_cgmres_register_wave_model(&ops);                                                                            \
    }                                                                                                                       \
  } g_##ProblemType##_cgmres_wave_registrar;                                                                                \
  }
