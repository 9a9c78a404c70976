// gfx950 kernels of the batched C/GMRES solver (C-ABI: include/nmpc_hip_cgmres.h, nmpc_amd/csrc/cgmres_capi.hip).
//
// One lane per instance.  C/GMRES (Ohtsuka 2004) does one Newton-type update of the whole input horizon per control tick; the
// cost of a tick is a dependent chain of horizon evaluations (calcDhDuList: N forward ODE steps of the state equation, N backward
// steps of the costate equation, N calcDhDu), two for the right-hand side and one per Arnoldi product of the GMRES solve.  Each is
// strictly sequential in time and a few hundred scalar instructions per step, so an instance is one lane and a batch is B
// independent lanes; 64 instances per workgroup (one wavefront), so that small batches spread over the compute units.
//
// What each piece restates (nmpc_cgmres, read, not copied):
//   gmresSolve         Gmres::solve, Kelley Alg. 3.5.1 (include/nmpc_cgmres/Gmres.h:65-125): modified Gram-Schmidt, the
//                      conditional re-orthogonalisation (Avk_norm + 1e-3 new_basis_norm == Avk_norm), Givens rotations,
//                      k_max = min(k_max, n), the triangular solve and the update of the warm start x.
//   odeStep            EulerOdeSolver / RungeKuttaOdeSolver (OdeSolver.h:32-80).
//   calcDhDuList       CgmresSolver::calcDhDuList (src/CgmresSolver.cpp:145-185).
//   controlInput       CgmresSolver::calcControlInput + eqAmulFunc (CgmresSolver.cpp:109-143, 187-202).
//   setupLane          CgmresSolver::setup (CgmresSolver.cpp:8-64): the Newton / GMRES loop on dim_uc (<= 100 iterations,
//                      tolerance 1e-6); a per-instance status replaces the message on std::cout.
//   cgmres_run_kernel  the tick loop of CgmresSolver::run (CgmresSolver.cpp:66-107), a chunk of ticks per launch.
//
// Memory: every per-instance array lives in HBM as [element][instance] (a wavefront's 64 lanes touch 512 consecutive bytes): the
// input list U, DhDu at (t, x) and at (t + delta, x_with_delta), the GMRES warm start delta_u, the state list x_list of the
// current horizon evaluation, and the GMRES workspace (right-hand side, Arnoldi vector, Krylov basis, the rotated Hessenberg
// columns, g and the Givens pairs).  Nothing is indexed at run time in registers (no scratch: tests/test_cgmres_isa.py): the
// small GMRES arrays are O(k_max^2) scalars against O(k_max N dim_uc) model evaluations, so keeping them beside the basis costs
// nothing measurable and the same code serves the dense diagnostic with n up to 512.
//
// Bits: the translation units that instantiate these kernels are compiled with -ffp-contract=off (nmpc_amd/build.py), so every
// operation is the IEEE operation written here, in the order the checker (tests/cpp/cgmres_checker.cpp) writes it.
#pragma once

#include <cstddef>
#include <new>
#include <type_traits>

#include <hip/hip_runtime.h>

#include <nmpc_amd/linalg.hpp>

namespace nmpc_amd
{
namespace hip
{
namespace cgmres
{
constexpr int kMaxKmax = 16; //!< cap on config k_max of the C/GMRES solver
constexpr int kDenseMaxN = 512; //!< cap on n (and so k_max) of the dense diagnostic
constexpr int kBlock = 64; //!< lanes (instances) per workgroup

/** Per-instance status (nmpc_hip_cgmres_instance_status). */
enum : int
{
  kStatusUninitialized = 0,
  kStatusSucceeded = 1, //!< setup converged (|DhDu| <= 1e-6); ticks run
  kStatusSetupNotConverged = 2, //!< setup ended above the tolerance; ticks still run, as in the reference
  kStatusNonFinite = 3 //!< a state or input became NaN / Inf: the instance stopped updating
};

/** A vector of one instance in an [element][instance] array. */
struct Vec
{
  double * p;
  size_t s;
  NMPC_HD double & operator[](int i) const
  {
    return p[static_cast<size_t>(i) * s];
  }
};

/** Doubles per instance of the GMRES workspace for vectors of n elements and at most K iterations. */
NMPC_HD size_t gmresWorkspaceElems(int n, int K)
{
  return static_cast<size_t>(K + 3) * n + static_cast<size_t>(K) * K + static_cast<size_t>(K + 1) + 2 * static_cast<size_t>(K);
}

/** The GMRES workspace of one instance: b [n], w [n], V [K+1][n], R [K][K] (column c of the rotated Hessenberg matrix at
    R[c * K + j]), g [K+1], Givens cosines / sines [K]. */
struct GmresWs
{
  double * base;
  size_t B;
  int n, K;
  NMPC_HD Vec at(size_t off) const
  {
    return Vec{base + off * B, B};
  }
  NMPC_HD Vec b() const
  {
    return at(0);
  }
  NMPC_HD Vec w() const
  {
    return at(n);
  }
  NMPC_HD Vec V(int k) const
  {
    return at(static_cast<size_t>(2 + k) * n);
  }
  NMPC_HD Vec R() const
  {
    return at(static_cast<size_t>(K + 3) * n);
  }
  NMPC_HD Vec g() const
  {
    return at(static_cast<size_t>(K + 3) * n + static_cast<size_t>(K) * K);
  }
  NMPC_HD Vec c() const
  {
    return at(static_cast<size_t>(K + 3) * n + static_cast<size_t>(K) * K + K + 1);
  }
  NMPC_HD Vec s() const
  {
    return at(static_cast<size_t>(K + 3) * n + static_cast<size_t>(K) * K + 2 * K + 1);
  }
};

NMPC_HD double dot(const Vec & a, const Vec & b, int n)
{
  double acc = 0;
  for(int e = 0; e < n; e++)
  {
    acc += a[e] * b[e];
  }
  return acc;
}

/** Eigen's normalized(): v / |v|, a zero vector unchanged. */
NMPC_HD void normalizedInto(const Vec & v, const Vec & out, int n)
{
  const double z = dot(v, v, n);
  if(z > 0)
  {
    const double nrm = sqrt(z);
    for(int e = 0; e < n; e++)
    {
      out[e] = v[e] / nrm;
    }
  }
  else
  {
    for(int e = 0; e < n; e++)
    {
      out[e] = v[e];
    }
  }
}

/** Solve A x = b (b in ws.b(), x the warm start, updated in place) by restart-free GMRES with Givens rotations (Kelley Alg. 3.5.1,
    Gmres.h:65-125).  Amul(v, out) writes A v to out.  k_max is clamped to n and to ws.K.  Every loop is bounded by k_max and n: a
    non-finite residual ends the iteration (NaN > eps |b| is false).
    \param iters out: the number of Arnoldi steps k
    \param reorth_fired out: 1 if the re-orthogonalisation ran in some step */
template<class Amul>
NMPC_HD void gmresSolve(Amul & A, const GmresWs & ws, const Vec & x, int k_max, double eps, bool apply_reorth, int & iters,
                        int & reorth_fired)
{
  const int n = ws.n;
  k_max = k_max < n ? k_max : n;
  k_max = k_max < ws.K ? k_max : ws.K;
  const Vec b = ws.b(), w = ws.w(), R = ws.R(), g = ws.g(), cs = ws.c(), sn = ws.s();
  // 1.  r = b - A x, v_1 = r / |r|
  A(x, w);
  const Vec v0 = ws.V(0);
  for(int e = 0; e < n; e++)
  {
    v0[e] = b[e] - w[e];
  }
  double rho = sqrt(dot(v0, v0, n));
  normalizedInto(v0, v0, n);
  for(int i = 0; i <= k_max; i++)
  {
    g[i] = 0;
  }
  g[0] = rho;
  const double b_norm = sqrt(dot(b, b, n));
  int k = 0;
  reorth_fired = 0;
  // 2.
  while(rho > eps * b_norm && k < k_max)
  {
    k++;
    // (b) w = A v_k, modified Gram-Schmidt against v_1 .. v_k; the new Hessenberg column is kept in R's column k - 1
    A(ws.V(k - 1), w);
    const int col = (k - 1) * ws.K;
    const double Avk_norm = apply_reorth ? sqrt(dot(w, w, n)) : 0.0;
    for(int j = 0; j < k; j++)
    {
      const Vec vj = ws.V(j);
      const double h = dot(w, vj, n);
      R[col + j] = h;
      for(int e = 0; e < n; e++)
      {
        w[e] = w[e] - h * vj[e];
      }
    }
    // (c)
    const double new_basis_norm = sqrt(dot(w, w, n));
    double h_sub = new_basis_norm; // H(k, k-1)
    // (d) re-orthogonalisation when the new vector is lost in rounding
    if(apply_reorth && Avk_norm + 1e-3 * new_basis_norm == Avk_norm)
    {
      reorth_fired = 1;
      for(int j = 0; j < k; j++)
      {
        const Vec vj = ws.V(j);
        const double h = dot(w, vj, n);
        R[col + j] = R[col + j] + h;
        for(int e = 0; e < n; e++)
        {
          w[e] = w[e] - h * vj[e];
        }
      }
    }
    // (e)
    normalizedInto(w, ws.V(k), n);
    // (f) i. the previous rotations on the new column
    for(int i = 0; i < k - 1; i++)
    {
      const double h0 = R[col + i], h1 = R[col + i + 1];
      const double c = cs[i], s = sn[i];
      R[col + i] = c * h0 - s * h1;
      R[col + i + 1] = s * h0 + c * h1;
    }
    // ii. - iii. the new rotation
    const double hd = R[col + k - 1];
    const double nu = sqrt(hd * hd + h_sub * h_sub);
    const double c_k = hd / nu, s_k = -h_sub / nu;
    cs[k - 1] = c_k;
    sn[k - 1] = s_k;
    R[col + k - 1] = c_k * hd - s_k * h_sub;
    // iv.
    const double g0 = g[k - 1], g1 = g[k];
    g[k - 1] = c_k * g0 - s_k * g1;
    g[k] = s_k * g0 + c_k * g1;
    // (g)
    rho = fabs(g[k]);
  }
  // 3. y = R^-1 g by columns, from the last (y overwrites g)
  for(int i = k - 1; i >= 0; i--)
  {
    const double yi = g[i] / R[i * ws.K + i];
    g[i] = yi;
    for(int j = 0; j < i; j++)
    {
      g[j] = g[j] - yi * R[i * ws.K + j];
    }
  }
  // 4. x += V y
  for(int i = 0; i < k; i++)
  {
    const double yi = g[i];
    const Vec vi = ws.V(i);
    for(int e = 0; e < n; e++)
    {
      x[e] = x[e] + yi * vi[e];
    }
  }
  iters = k;
}

/** Launch knobs and device arrays of one handle (all [element][instance] unless noted). */
struct CgmresBuffers
{
  int B = 0;
  int N = 0; //!< horizon_divide_num
  int nx = 0, nuc = 0;
  int k_max = 5;
  int horizon_solver = 0, sim_solver = 0; //!< 0 Euler, 1 RK4
  int dump_step = 0;
  double steady_horizon_duration = 1.0, horizon_increase_ratio = 0.5, dt = 1e-3, eq_zeta = 1000.0, finite_diff_delta = 0.002;
  const void * problems = nullptr;
  int per_instance = 0; //!< problems holds B objects (1) or one shared object (0)
  double * x = nullptr; //!< [nx][B] x_
  double * u = nullptr; //!< [nuc][B] u_
  double * U = nullptr; //!< [N * nuc][B] u_list_ (column i of the reference's matrix is elements i * nuc .. i * nuc + nuc - 1)
  double * DhDu = nullptr; //!< [N * nuc][B] DhDu_list_
  double * DhDu_wd = nullptr; //!< [N * nuc][B] DhDu_list_with_delta_
  double * du = nullptr; //!< [N * nuc][B] delta_u_vec_ (the GMRES warm start, kept across ticks)
  double * xlist = nullptr; //!< [(N + 1) * nx][B] x_list_
  double * ws = nullptr; //!< [gmresWorkspaceElems(N * nuc, kMaxKmax)][B]
  int * status = nullptr; //!< [B]
  double * err = nullptr; //!< [B] |DhDu_vec_| of the last tick (setup: |DhDu| at the end of the Newton loop)
  int * iters = nullptr; //!< [B] GMRES iterations of the last tick
  int * reorth = nullptr; //!< [B] re-orthogonalisation fired in the last tick
  // logs of run(): row r = tick r * dump_step; [row][element][instance]
  double * log_x = nullptr;
  double * log_u = nullptr;
  double * log_err = nullptr;
  int * log_iters = nullptr;
  int * log_reorth = nullptr;
  int log_rows = 0;
};

template<class P>
struct Lane
{
  static constexpr int NX = P::dim_x_, NUC = P::dim_uc_;
  const P & prob;
  const CgmresBuffers & bf;
  int b;

  NMPC_HD Vec at(double * p) const
  {
    return Vec{p + b, static_cast<size_t>(bf.B)};
  }

  NMPC_HD GmresWs ws(int n, int K) const
  {
    return GmresWs{bf.ws + b, static_cast<size_t>(bf.B), n, K};
  }

  /** One step of y' = f(t, y, aux) over h (OdeSolver.h:32-80): Euler (solver 0) or classic Runge-Kutta (solver 1). */
  template<int D, class F>
  NMPC_HD static void odeStep(int solver, const F & f, double t, const double * y, const double * aux, double h, double * out)
  {
    double k1[D];
    f(t, y, aux, k1);
    if(solver == 0)
    {
      NMPC_UNROLL
      for(int a = 0; a < D; a++)
      {
        out[a] = y[a] + h * k1[a];
      }
      return;
    }
    const double hh = h / 2;
    double yt[D], k2[D], k3[D], k4[D];
    NMPC_UNROLL
    for(int a = 0; a < D; a++)
    {
      yt[a] = y[a] + hh * k1[a];
    }
    f(t + hh, yt, aux, k2);
    NMPC_UNROLL
    for(int a = 0; a < D; a++)
    {
      yt[a] = y[a] + hh * k2[a];
    }
    f(t + hh, yt, aux, k3);
    NMPC_UNROLL
    for(int a = 0; a < D; a++)
    {
      yt[a] = y[a] + h * k3[a];
    }
    f(t + h, yt, aux, k4);
    const double h6 = h / 6;
    NMPC_UNROLL
    for(int a = 0; a < D; a++)
    {
      out[a] = y[a] + h6 * (((k1[a] + 2 * k2[a]) + 2 * k3[a]) + k4[a]);
    }
  }

  NMPC_HD void stateStep(int solver, double t, const double * x, const double * u, double h, double * out) const
  {
    const P & p = prob;
    odeStep<NX>(solver, [&p](double tt, const double * y, const double * a, double * dy) { p.stateEquation(tt, y, a, dy); }, t, x, u,
                h, out);
  }

  /** Input column i of the list: U (+ delta v when v is given: the argument of eqAmulFunc). */
  NMPC_HD void loadU(const Vec & U, const Vec * v, double delta, int i, double * u) const
  {
    NMPC_UNROLL
    for(int j = 0; j < NUC; j++)
    {
      u[j] = v ? U[i * NUC + j] + delta * (*v)[i * NUC + j] : U[i * NUC + j];
    }
  }

  /** CgmresSolver::calcDhDuList at (t, x) for the input list U (+ delta v), result to out [N * nuc]. */
  NMPC_HD void calcDhDuList(double t, const double * x0, const Vec & U, const Vec * v, double delta, const Vec & out) const
  {
    const int N = bf.N;
    const double horizon_duration = bf.steady_horizon_duration * (1.0 - exp(-bf.horizon_increase_ratio * t));
    const double step = horizon_duration / N;
    const Vec xl = at(bf.xlist);
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
      loadU(U, v, delta, i, u);
      stateStep(bf.horizon_solver, tau, x, u, step, xn);
      NMPC_UNROLL
      for(int a = 0; a < NX; a++)
      {
        x[a] = xn[a];
        xl[(i + 1) * NX + a] = x[a];
      }
      tau += step;
    }
    double lmd[NX];
    prob.calcDphiDx(tau, x, lmd);
    const P & p = prob;
    for(int i = N - 1; i >= 0; i--)
    {
      double xu[NX + NUC], lmd_prev[NX], dhdu[NUC];
      NMPC_UNROLL
      for(int a = 0; a < NX; a++)
      {
        xu[a] = xl[i * NX + a];
      }
      loadU(U, v, delta, i, xu + NX);
      odeStep<NX>(bf.horizon_solver, [&p](double tt, const double * y, const double * a, double * dy) { p.costateEquation(tt, y, a, dy); },
                  tau, lmd, xu, -step, lmd_prev);
      tau -= step;
      prob.calcDhDu(tau, xu, xu + NX, lmd, dhdu);
      NMPC_UNROLL
      for(int j = 0; j < NUC; j++)
      {
        out[i * NUC + j] = dhdu[j];
      }
      NMPC_UNROLL
      for(int a = 0; a < NX; a++)
      {
        lmd[a] = lmd_prev[a];
      }
    }
  }

  /** CgmresSolver::calcControlInput(t, x, next_x, u): updates U, delta_u, DhDu, DhDu_with_delta of the instance. */
  NMPC_HD void controlInput(double t, const double * x, const double * next_x, double * u, double & err, int & iters, int & reorth) const
  {
    const int n = bf.N * NUC;
    const double delta = bf.finite_diff_delta;
    const Vec U = at(bf.U), D = at(bf.DhDu), Dw = at(bf.DhDu_wd), du = at(bf.du);
    // 1.1, 1.2
    calcDhDuList(t, x, U, nullptr, 0.0, D);
    const double t_wd = t + delta;
    const double a0 = 1 - delta / bf.dt, a1 = delta / bf.dt;
    double x_wd[NX];
    NMPC_UNROLL
    for(int a = 0; a < NX; a++)
    {
      x_wd[a] = a0 * x[a] + a1 * next_x[a];
    }
    calcDhDuList(t_wd, x_wd, U, nullptr, 0.0, Dw);
    // 2.1 b = ((1 - zeta delta) DhDu - DhDu_with_delta) / delta
    const GmresWs W = ws(n, kMaxKmax);
    const Vec rhs = W.b();
    const double zd = 1 - bf.eq_zeta * delta;
    double sq = 0;
    for(int e = 0; e < n; e++)
    {
      const double d = D[e];
      sq += d * d;
      rhs[e] = (zd * d - Dw[e]) / delta;
    }
    err = sqrt(sq);
    // 2.2 eqAmulFunc: (DhDu_list(t + delta, x_with_delta, U + delta v) - DhDu_with_delta) / delta
    auto amul = [&](const Vec & v, const Vec & out) {
      calcDhDuList(t_wd, x_wd, U, &v, delta, out);
      for(int e = 0; e < n; e++)
      {
        out[e] = (out[e] - Dw[e]) / delta;
      }
    };
    gmresSolve(amul, W, du, bf.k_max, 1e-10, true, iters, reorth);
    // 2.3, 3.
    for(int e = 0; e < n; e++)
    {
      U[e] = U[e] + bf.dt * du[e];
    }
    NMPC_UNROLL
    for(int j = 0; j < NUC; j++)
    {
      u[j] = U[j];
    }
  }

  /** CgmresSolver::setup from (x, u) = (x_initial_, u_initial_) of the instance. */
  NMPC_HD void setup() const
  {
    const double t0 = 0;
    const double delta = bf.finite_diff_delta;
    const Vec xv = at(bf.x), uv = at(bf.u);
    double x[NX], u[NUC], lmd[NX], dhdu[NUC];
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
    prob.calcDphiDx(t0, x, lmd);
    // GMRES on dim_uc: the workspace and the first nuc elements of delta_u (its warm start across the Newton steps)
    const GmresWs W = ws(NUC, NUC);
    const Vec du = at(bf.du);
    NMPC_UNROLL
    for(int j = 0; j < NUC; j++)
    {
      du[j] = 0;
    }
    const double tol = 1e-6;
    double nrm = 0;
    for(int it = 0; it < 100; it++)
    {
      prob.calcDhDu(t0, x, u, lmd, dhdu);
      double sq = 0;
      NMPC_UNROLL
      for(int j = 0; j < NUC; j++)
      {
        sq += dhdu[j] * dhdu[j];
      }
      nrm = sqrt(sq);
      if(nrm <= tol)
      {
        break;
      }
      const Vec rhs = W.b();
      NMPC_UNROLL
      for(int j = 0; j < NUC; j++)
      {
        rhs[j] = -dhdu[j];
      }
      auto amul = [&](const Vec & v, const Vec & out) {
        double up[NUC], d[NUC];
        NMPC_UNROLL
        for(int j = 0; j < NUC; j++)
        {
          up[j] = u[j] + delta * v[j];
        }
        prob.calcDhDu(t0, x, up, lmd, d);
        NMPC_UNROLL
        for(int j = 0; j < NUC; j++)
        {
          out[j] = (d[j] - dhdu[j]) / delta;
        }
      };
      int k = 0, ro = 0;
      gmresSolve(amul, W, du, NUC, 1e-10, true, k, ro);
      NMPC_UNROLL
      for(int j = 0; j < NUC; j++)
      {
        u[j] = u[j] + du[j];
      }
    }
    bool finite = isfinite(nrm);
    NMPC_UNROLL
    for(int j = 0; j < NUC; j++)
    {
      uv[j] = u[j];
      finite = finite && isfinite(u[j]);
    }
    const Vec U = at(bf.U), D = at(bf.DhDu), dU = at(bf.du);
    for(int i = 0; i < bf.N; i++)
    {
      NMPC_UNROLL
      for(int j = 0; j < NUC; j++)
      {
        U[i * NUC + j] = u[j];
        D[i * NUC + j] = dhdu[j];
        dU[i * NUC + j] = 0;
      }
    }
    bf.status[b] = !finite ? kStatusNonFinite : (nrm <= tol ? kStatusSucceeded : kStatusSetupNotConverged);
    bf.err[b] = nrm;
    bf.iters[b] = 0;
    bf.reorth[b] = 0;
  }
};

template<class P>
NMPC_HD P loadProblem(const CgmresBuffers & bf, int b)
{
  return static_cast<const P *>(bf.problems)[bf.per_instance ? b : 0];
}

template<class P>
__global__ void __launch_bounds__(kBlock) cgmres_setup_kernel(CgmresBuffers bf)
{
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if(b >= bf.B)
  {
    return;
  }
  const P prob = loadProblem<P>(bf, b);
  Lane<P>{prob, bf, b}.setup();
}

/** Ticks i0 .. i0 + n_ticks - 1 of CgmresSolver::run's loop, t0 the time of tick i0 (accumulated t += dt by the caller exactly
    as here).  Tick i: simulate next_x, calcControlInput, x = next_x, log when dump_step > 0 and i % dump_step == 0. */
template<class P>
__global__ void __launch_bounds__(kBlock) cgmres_run_kernel(CgmresBuffers bf, int i0, int n_ticks, double t0)
{
  constexpr int NX = P::dim_x_, NUC = P::dim_uc_;
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if(b >= bf.B || bf.status[b] == kStatusNonFinite || bf.status[b] == kStatusUninitialized)
  {
    return;
  }
  const P prob = loadProblem<P>(bf, b);
  const Lane<P> lane{prob, bf, b};
  const Vec xv = lane.at(bf.x), uv = lane.at(bf.u);
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
  double t = t0;
  double err = bf.err[b];
  int iters = bf.iters[b], reorth = bf.reorth[b];
  bool finite = true;
  for(int s = 0; s < n_ticks && finite; s++)
  {
    const int i = i0 + s;
    double next_x[NX];
    lane.stateStep(bf.sim_solver, t, x, u, bf.dt, next_x);
    lane.controlInput(t, x, next_x, u, err, iters, reorth);
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
    if(bf.dump_step > 0 && i % bf.dump_step == 0)
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

/** One calcControlInput(t[b], x[b], next_x[b], u[b]) per instance; arguments in the boundary layout [B][dim].  Instances that are
    not set up or have stopped leave u_out as it is. */
template<class P>
__global__ void __launch_bounds__(kBlock)
    cgmres_control_input_kernel(CgmresBuffers bf, const double * t, const double * x_in, const double * next_x_in, double * u_out)
{
  constexpr int NX = P::dim_x_, NUC = P::dim_uc_;
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if(b >= bf.B || bf.status[b] == kStatusNonFinite || bf.status[b] == kStatusUninitialized)
  {
    return;
  }
  const P prob = loadProblem<P>(bf, b);
  const Lane<P> lane{prob, bf, b};
  double x[NX], next_x[NX], u[NUC];
  bool finite = true;
  NMPC_UNROLL
  for(int a = 0; a < NX; a++)
  {
    x[a] = x_in[static_cast<size_t>(b) * NX + a];
    next_x[a] = next_x_in[static_cast<size_t>(b) * NX + a];
  }
  double err = 0;
  int iters = 0, reorth = 0;
  lane.controlInput(t[b], x, next_x, u, err, iters, reorth);
  const Vec uv = lane.at(bf.u);
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

/** The four problem functions at n_points points (boundary layout [point][dim]); point p uses the problem object of instance
    p % B. */
template<class P>
__global__ void __launch_bounds__(kBlock) cgmres_model_eval_kernel(CgmresBuffers bf, int n_points, const double * t, const double * x,
                                                                    const double * u, const double * lmd, double * dotx, double * dotlmd,
                                                                    double * dphidx, double * dhdu)
{
  constexpr int NX = P::dim_x_, NUC = P::dim_uc_;
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if(p >= n_points)
  {
    return;
  }
  const P prob = loadProblem<P>(bf, p % bf.B);
  double xu[NX + NUC], l[NX], o[NX], od[NUC];
  NMPC_UNROLL
  for(int a = 0; a < NX; a++)
  {
    xu[a] = x[static_cast<size_t>(p) * NX + a];
    l[a] = lmd[static_cast<size_t>(p) * NX + a];
  }
  NMPC_UNROLL
  for(int j = 0; j < NUC; j++)
  {
    xu[NX + j] = u[static_cast<size_t>(p) * NUC + j];
  }
  prob.stateEquation(t[p], xu, xu + NX, o);
  NMPC_UNROLL
  for(int a = 0; a < NX; a++)
  {
    dotx[static_cast<size_t>(p) * NX + a] = o[a];
  }
  prob.costateEquation(t[p], l, xu, o);
  NMPC_UNROLL
  for(int a = 0; a < NX; a++)
  {
    dotlmd[static_cast<size_t>(p) * NX + a] = o[a];
  }
  prob.calcDphiDx(t[p], xu, o);
  NMPC_UNROLL
  for(int a = 0; a < NX; a++)
  {
    dphidx[static_cast<size_t>(p) * NX + a] = o[a];
  }
  prob.calcDhDu(t[p], xu, xu + NX, l, od);
  NMPC_UNROLL
  for(int j = 0; j < NUC; j++)
  {
    dhdu[static_cast<size_t>(p) * NUC + j] = od[j];
  }
}

#ifdef NMPC_AMD_CGMRES_COMMON_KERNELS
/** Batched dense GMRES (Gmres::solve with a matrix, Gmres.h:42-50): one lane per system.  A [n * n][B] (row i, column j at element
    i * n + j), b in the workspace, x [n][B] the initial guess, updated in place.  n <= kDenseMaxN, k_max <= n. */
__global__ void __launch_bounds__(kBlock) cgmres_gmres_dense_kernel(int B, int n, int K, int k_max, int apply_reorth, double eps,
                                                                     const double * A, double * x, double * ws, int * iters, int * reorth)
{
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if(b >= B)
  {
    return;
  }
  const GmresWs W{ws + b, static_cast<size_t>(B), n, K};
  const Vec xv{x + b, static_cast<size_t>(B)};
  const double * Ab = A + b;
  auto amul = [&](const Vec & v, const Vec & out) {
    for(int i = 0; i < n; i++)
    {
      double acc = 0;
      for(int j = 0; j < n; j++)
      {
        acc += Ab[(static_cast<size_t>(i) * n + j) * B] * v[j];
      }
      out[i] = acc;
    }
  };
  int k = 0, ro = 0;
  gmresSolve(amul, W, xv, k_max, eps, apply_reorth != 0, k, ro);
  iters[b] = k;
  reorth[b] = ro;
}
#endif

/** Type-erased description of one registered C/GMRES problem type (what the C-ABI knows about it). */
struct CgmresOps
{
  const char * name;
  int nx, nu, nc, nuc;
  size_t param_bytes;
  void (*default_params)(void * out);
  void (*initial)(double * x, double * u);
  hipError_t (*launch_setup)(const CgmresBuffers & bf, hipStream_t stream);
  hipError_t (*launch_run)(const CgmresBuffers & bf, int i0, int n_ticks, double t0, hipStream_t stream);
  hipError_t (*launch_control_input)(const CgmresBuffers & bf, const double * t, const double * x, const double * next_x, double * u,
                                     hipStream_t stream);
  hipError_t (*launch_model_eval)(const CgmresBuffers & bf, int n_points, const double * t, const double * x, const double * u,
                                  const double * lmd, double * dotx, double * dotlmd, double * dphidx, double * dhdu, hipStream_t stream);
};

template<class P>
struct CgmresOpsOf
{
  static_assert(std::is_trivially_copyable<P>::value, "[C/GMRES] a problem object must be trivially copyable");

  static dim3 grid(int n)
  {
    return dim3(static_cast<unsigned>((n + kBlock - 1) / kBlock));
  }

  static CgmresOps make()
  {
    CgmresOps o{};
    o.name = P::kName;
    o.nx = P::dim_x_;
    o.nu = P::dim_u_;
    o.nc = P::dim_c_;
    o.nuc = P::dim_uc_;
    o.param_bytes = sizeof(P);
    o.default_params = [](void * out) { new(out) P(); };
    o.initial = [](double * x, double * u) {
      P::initialState(x);
      P::initialInput(u);
    };
    o.launch_setup = [](const CgmresBuffers & bf, hipStream_t stream) {
      hipLaunchKernelGGL(cgmres_setup_kernel<P>, grid(bf.B), dim3(kBlock), 0, stream, bf);
      return hipGetLastError();
    };
    o.launch_run = [](const CgmresBuffers & bf, int i0, int n_ticks, double t0, hipStream_t stream) {
      hipLaunchKernelGGL(cgmres_run_kernel<P>, grid(bf.B), dim3(kBlock), 0, stream, bf, i0, n_ticks, t0);
      return hipGetLastError();
    };
    o.launch_control_input = [](const CgmresBuffers & bf, const double * t, const double * x, const double * next_x, double * u,
                                hipStream_t stream) {
      hipLaunchKernelGGL(cgmres_control_input_kernel<P>, grid(bf.B), dim3(kBlock), 0, stream, bf, t, x, next_x, u);
      return hipGetLastError();
    };
    o.launch_model_eval = [](const CgmresBuffers & bf, int n_points, const double * t, const double * x, const double * u,
                             const double * lmd, double * dotx, double * dotlmd, double * dphidx, double * dhdu, hipStream_t stream) {
      hipLaunchKernelGGL(cgmres_model_eval_kernel<P>, grid(n_points), dim3(kBlock), 0, stream, bf, n_points, t, x, u, lmd, dotx, dotlmd,
                         dphidx, dhdu);
      return hipGetLastError();
    };
    return o;
  }
};
} // namespace cgmres
} // namespace hip
} // namespace nmpc_amd

extern "C" int nmpc_hip_cgmres_register_model(const nmpc_amd::hip::cgmres::CgmresOps * ops);

/** Make a C/GMRES problem type (see CgmresProblem.hpp) available to nmpc_hip_cgmres_create under ProblemType::kName.  Use once,
    at namespace scope, in a HIP translation unit linked into the library. */
#define NMPC_AMD_REGISTER_CGMRES_PROBLEM(ProblemType)                                                            \
  namespace                                                                                                      \
  {                                                                                                              \
  struct ProblemType##CgmresRegistrar                                                                            \
  {                                                                                                              \
    ProblemType##CgmresRegistrar()                                                                               \
    {                                                                                                            \
      static const nmpc_amd::hip::cgmres::CgmresOps ops = nmpc_amd::hip::cgmres::CgmresOpsOf<ProblemType>::make(); \
      nmpc_hip_cgmres_register_model(&ops);                                                                      \
    }                                                                                                            \
  } g_##ProblemType##_cgmres_registrar;                                                                          \
  }
