// TEST INFRASTRUCTURE — NOT PRODUCT CODE (see oracle/fmpc_oracle.hpp header).
//
// ctypes-loadable C entry points over the CPU FMPC oracle: single solve (with every intermediate the parity tests compare),
// threaded batch solve (also the cpu_baseline leg of bench.py --workload fmpc, kind "port") with or without those
// intermediates, the closed loop solve -> plant step, model evaluation, a step's dimensions, the LDLT restatement and
// l1NormDirectionalDeriv.
#include "fmpc_models.hpp"
#include "fmpc_oracle.hpp"

#include <atomic>
#include <cstring>
#include <thread>

#include <pthread.h>
#include <sched.h>

namespace
{
using namespace oracle_fmpc;

template<class F>
int dispatch(const char * name, F && f)
{
  const std::string s(name);
  if(s == Oscillator::kName)
  {
    return f(Oscillator());
  }
  if(s == CartPole::kName)
  {
    return f(CartPole());
  }
  if(s == PointMass::kName)
  {
    return f(PointMass());
  }
  if(s == Vertical::kName)
  {
    return f(Vertical());
  }
  return -100;
}

/** Every model is a struct of doubles: the parameter blob is its memory image. */
template<class M>
M fromParams(const double * params)
{
  static_assert(sizeof(M) % sizeof(double) == 0, "model structs hold doubles only");
  M m;
  if(params)
  {
    std::memcpy(static_cast<void *>(&m), params, sizeof(M));
  }
  return m;
}

/** Problem object of instance b: one shared parameter blob, or one per instance. */
template<class M>
M fromParams(const double * params, int per_instance_params, int b)
{
  return fromParams<M>(params && per_instance_params ? params + static_cast<size_t>(b) * (sizeof(M) / sizeof(double)) : params);
}

/** p + n, or NULL for an output the caller does not want. */
template<class T>
T * off(T * p, size_t n)
{
  return p ? p + n : nullptr;
}

/** fn(b) for every b < batch on n_threads CPU threads (dynamic chunks, threads pinned to the allowed CPUs in order). */
template<class Fn>
void parallelFor(int batch, int n_threads, Fn && fn)
{
  std::atomic<int> next(0);
  const int chunk = std::max(1, std::min(16, batch / std::max(1, n_threads * 8)));
  cpu_set_t allowed;
  CPU_ZERO(&allowed);
  sched_getaffinity(0, sizeof(allowed), &allowed);
  std::vector<int> cpus;
  for(int i = 0; i < CPU_SETSIZE; i++)
  {
    if(CPU_ISSET(i, &allowed))
    {
      cpus.push_back(i);
    }
  }
  auto work = [&](int tid) {
    if(n_threads > 1 && !cpus.empty())
    {
      cpu_set_t one;
      CPU_ZERO(&one);
      CPU_SET(cpus[tid % cpus.size()], &one);
      pthread_setaffinity_np(pthread_self(), sizeof(one), &one);
    }
    for(;;)
    {
      const int b0 = next.fetch_add(chunk);
      if(b0 >= batch)
      {
        break;
      }
      for(int b = b0; b < std::min(batch, b0 + chunk); b++)
      {
        fn(b);
      }
    }
  };
  if(n_threads <= 1)
  {
    work(0);
  }
  else
  {
    std::vector<std::thread> th;
    for(int i = 0; i < n_threads; i++)
    {
      th.emplace_back(work, i);
    }
    for(auto & t : th)
    {
      t.join();
    }
  }
}
} // namespace

extern "C"
{
  struct oracle_fmpc_config
  {
    int horizon_steps;
    int max_iter;
    double kkt_error_thre;
    int check_nan;
    int init_complementary_variable;
    int update_barrier_eps;
    int break_if_llt_fails;
    int enable_line_search;
    int merit_const_scale_from_lagrange_multipliers;
  };

  enum
  {
    ORACLE_FMPC_NTRACE = 6 // iter, kkt_error, barrier_eps, alpha_s_max, alpha_nu_max, alpha_s
  };

  void oracle_fmpc_default_config(oracle_fmpc_config * c)
  {
    Config d;
    c->horizon_steps = d.horizon_steps;
    c->max_iter = d.max_iter;
    c->kkt_error_thre = d.kkt_error_thre;
    c->check_nan = d.check_nan;
    c->init_complementary_variable = d.init_complementary_variable;
    c->update_barrier_eps = d.update_barrier_eps;
    c->break_if_llt_fails = d.break_if_llt_fails;
    c->enable_line_search = d.enable_line_search;
    c->merit_const_scale_from_lagrange_multipliers = d.merit_const_scale_from_lagrange_multipliers;
  }

  int oracle_fmpc_model_info(const char * model, int * n, int * m, int * g, int * param_doubles)
  {
    return dispatch(model, [&](auto mdl) {
      using M = decltype(mdl);
      *n = M::N;
      *m = M::M;
      *g = M::G;
      *param_doubles = static_cast<int>(sizeof(M) / sizeof(double));
      return 0;
    });
  }

  int oracle_fmpc_default_params(const char * model, double * out)
  {
    return dispatch(model, [&](auto mdl) {
      std::memcpy(out, &mdl, sizeof(mdl));
      return 0;
    });
  }

  /** Input and inequality dimension of a step at time t: (m, g) of oracle_fmpc_model_info unless the model's vary with time. */
  int oracle_fmpc_dims_at(const char * model, const double * params, double t, int * m, int * g)
  {
    return dispatch(model, [&](auto mdl) {
      using M = decltype(mdl);
      *m = M::M;
      *g = M::G;
      if constexpr(HasStepDims<M>::value)
      {
        fromParams<M>(params).dims(t, *m, *g);
      }
      return 0;
    });
  }
}

namespace
{
Config toConfig(const oracle_fmpc_config * c)
{
  Config cfg;
  cfg.print_level = 0;
  cfg.horizon_steps = c->horizon_steps;
  cfg.max_iter = c->max_iter;
  cfg.kkt_error_thre = c->kkt_error_thre;
  cfg.check_nan = c->check_nan != 0;
  cfg.init_complementary_variable = c->init_complementary_variable != 0;
  cfg.update_barrier_eps = c->update_barrier_eps != 0;
  cfg.break_if_llt_fails = c->break_if_llt_fails != 0;
  cfg.enable_line_search = c->enable_line_search != 0;
  cfg.merit_const_scale_from_lagrange_multipliers = c->merit_const_scale_from_lagrange_multipliers != 0;
  return cfg;
}

/** One solve on flat arrays.  Returns the Status, or -1 (std::invalid_argument) / -2 (std::runtime_error) where the
    reference throws (FmpcSolver.hpp:285-354). */
template<class M>
int solveOne(const M & mdl,
             const Config & cfg,
             double current_t,
             const double * current_x,
             double * x,
             double * u,
             double * lambda,
             double * s,
             double * nu,
             double * barrier_eps,
             int * iters,
             double * trace,
             double * gain_k,
             double * gain_K,
             double * gain_s,
             double * gain_P,
             double * delta,
             double * merit)
{
  const int T = cfg.horizon_steps;
  constexpr int N = M::N, MM = M::M, G = M::G;
  FmpcSolver<M> solver(mdl);
  solver.config() = cfg;
  solver.barrierEps() = *barrier_eps;
  Variable v(T, N, MM, G);
  std::copy(x, x + v.x.size(), v.x.begin());
  std::copy(u, u + v.u.size(), v.u.begin());
  std::copy(lambda, lambda + v.lambda.size(), v.lambda.begin());
  std::copy(s, s + v.s.size(), v.s.begin());
  std::copy(nu, nu + v.nu.size(), v.nu.begin());
  int status;
  try
  {
    status = solver.solve(current_t, current_x, v);
  }
  catch(const std::invalid_argument &)
  {
    return -1;
  }
  catch(const std::runtime_error &)
  {
    return -2;
  }
  const Variable & r = solver.variable();
  std::copy(r.x.begin(), r.x.end(), x);
  std::copy(r.u.begin(), r.u.end(), u);
  std::copy(r.lambda.begin(), r.lambda.end(), lambda);
  std::copy(r.s.begin(), r.s.end(), s);
  std::copy(r.nu.begin(), r.nu.end(), nu);
  *barrier_eps = solver.barrierEps();
  const auto & tr = solver.traceDataList();
  if(iters)
  {
    *iters = tr.empty() ? 0 : tr.back().iter;
  }
  if(trace)
  {
    for(int i = 0; i < cfg.max_iter; i++)
    {
      double * row = trace + i * ORACLE_FMPC_NTRACE;
      if(i < static_cast<int>(tr.size()))
      {
        row[0] = tr[i].iter;
        row[1] = tr[i].kkt_error;
        row[2] = tr[i].barrier_eps;
        row[3] = tr[i].alpha_s_max;
        row[4] = tr[i].alpha_nu_max;
        row[5] = tr[i].alpha_s;
      }
      else
      {
        std::fill(row, row + ORACLE_FMPC_NTRACE, 0.0);
      }
    }
  }
  const auto & cl = solver.coeffList();
  for(int i = 0; i <= T; i++)
  {
    if(i < T && gain_k)
    {
      std::copy(cl[i].k, cl[i].k + MM, gain_k + i * MM);
    }
    if(i < T && gain_K)
    {
      std::copy(cl[i].K, cl[i].K + MM * N, gain_K + i * MM * N);
    }
    if(gain_s)
    {
      std::copy(cl[i].s, cl[i].s + N, gain_s + i * N);
    }
    if(gain_P)
    {
      std::copy(cl[i].P, cl[i].P + N * N, gain_P + i * N * N);
    }
  }
  if(delta) // [dx (T+1)N | du TM | dlambda (T+1)N | ds TG | dnu TG] of the last iteration that reached the forward pass
  {
    const Variable & d = solver.deltaVariable();
    double * p = delta;
    for(const auto * vec : {&d.x, &d.u, &d.lambda, &d.s, &d.nu})
    {
      p = std::copy(vec->begin(), vec->end(), p);
    }
  }
  if(merit) // of the last iteration that set up the line search
  {
    merit[0] = solver.meritFunc();
    merit[1] = solver.meritDeriv();
    merit[2] = solver.meritConstScale();
  }
  return status;
}
} // namespace

extern "C"
{
  /** FmpcSolver::solve for one instance; variables in / out.  Optional outputs may be NULL. */
  int oracle_fmpc_solve(const char * model,
                        const oracle_fmpc_config * c,
                        const double * params,
                        double current_t,
                        const double * current_x,
                        double * x,
                        double * u,
                        double * lambda,
                        double * s,
                        double * nu,
                        double * barrier_eps,
                        int * iters,
                        double * trace,
                        double * gain_k,
                        double * gain_K,
                        double * gain_s,
                        double * gain_P,
                        double * delta)
  {
    return dispatch(model, [&](auto mdl) {
      using M = decltype(mdl);
      return solveOne(fromParams<M>(params), toConfig(c), current_t, current_x, x, u, lambda, s, nu, barrier_eps, iters, trace,
                      gain_k, gain_K, gain_s, gain_P, delta, nullptr);
    });
  }

  /** A batch of independent solves on n_threads CPU threads (dynamic chunks, threads pinned to the allowed CPUs in order).
      params: one blob (per_instance_params = 0) or one per instance.  Arrays are batch-major: x [B][T+1][N], ...;
      trace [B][max_iter][ORACLE_FMPC_NTRACE]; gain_K0 [B][M*N] (K of the first step, the caller's feedback gain,
      TestFmpcCartPole.cpp:350) may be NULL. */
  int oracle_fmpc_solve_batch(const char * model,
                              const oracle_fmpc_config * c,
                              const double * params,
                              int per_instance_params,
                              int batch,
                              const double * current_t,
                              const double * current_x,
                              double * x,
                              double * u,
                              double * lambda,
                              double * s,
                              double * nu,
                              double * barrier_eps,
                              int * status,
                              int * iters,
                              double * trace,
                              double * gain_K0,
                              int n_threads)
  {
    return dispatch(model, [&](auto mdl0) {
      using M = decltype(mdl0);
      constexpr int N = M::N, MM = M::M, G = M::G;
      const Config cfg = toConfig(c);
      const size_t T = cfg.horizon_steps;
      parallelFor(batch, n_threads, [&](size_t b) {
        std::vector<double> K(gain_K0 ? T * MM * N : 0);
        status[b] = solveOne(fromParams<M>(params, per_instance_params, b), cfg, current_t ? current_t[b] : 0.0, current_x + b * N,
                             x + b * (T + 1) * N, u + b * T * MM, lambda + b * (T + 1) * N, s + b * T * G, nu + b * T * G,
                             barrier_eps + b, off(iters, b), off(trace, b * cfg.max_iter * ORACLE_FMPC_NTRACE), nullptr,
                             gain_K0 ? K.data() : nullptr, nullptr, nullptr, nullptr, nullptr);
        if(gain_K0)
        {
          std::copy(K.begin(), K.begin() + MM * N, gain_K0 + b * MM * N);
        }
      });
      return 0;
    });
  }

  /** oracle_fmpc_solve_batch with the optional outputs of oracle_fmpc_solve for every instance: gain_k [B][T][M], gain_K
      [B][T][M*N], gain_s [B][T+1][N], gain_P [B][T+1][N*N], delta [B][2 (T+1) N + T M + 2 T G] and merit [B][3] (merit_func_,
      merit_deriv_, merit_const_scale_).  Any of them, iters and trace may be NULL. */
  int oracle_fmpc_solve_batch_full(const char * model,
                                   const oracle_fmpc_config * c,
                                   const double * params,
                                   int per_instance_params,
                                   int batch,
                                   const double * current_t,
                                   const double * current_x,
                                   double * x,
                                   double * u,
                                   double * lambda,
                                   double * s,
                                   double * nu,
                                   double * barrier_eps,
                                   int * status,
                                   int * iters,
                                   double * trace,
                                   double * gain_k,
                                   double * gain_K,
                                   double * gain_s,
                                   double * gain_P,
                                   double * delta,
                                   double * merit,
                                   int n_threads)
  {
    return dispatch(model, [&](auto mdl0) {
      using M = decltype(mdl0);
      constexpr int N = M::N, MM = M::M, G = M::G;
      const Config cfg = toConfig(c);
      const size_t T = cfg.horizon_steps;
      parallelFor(batch, n_threads, [&](size_t b) {
        status[b] = solveOne(fromParams<M>(params, per_instance_params, b), cfg, current_t[b], current_x + b * N, x + b * (T + 1) * N,
                             u + b * T * MM, lambda + b * (T + 1) * N, s + b * T * G, nu + b * T * G, barrier_eps + b, off(iters, b),
                             off(trace, b * cfg.max_iter * ORACLE_FMPC_NTRACE), off(gain_k, b * T * MM), off(gain_K, b * T * MM * N),
                             off(gain_s, b * (T + 1) * N), off(gain_P, b * (T + 1) * N * N),
                             off(delta, b * (2 * (T + 1) * N + T * MM + 2 * T * G)), off(merit, b * 3));
      });
      return 0;
    });
  }

  /** Closed loop of every instance: n_ticks times { log x; solve(t, x) from the variable of the tick before (barrier parameter
      carried); log u_list[0] (0 beyond the step's input dimension), status and iteration count; `substeps` plant steps
      x <- stateEq(t, x, u_list[0], sim_dt), the input keeping the size it has at the tick's time }.  Variable in / out;
      logs [B][n_ticks][...]. */
  int oracle_fmpc_closed_loop(const char * model,
                              const oracle_fmpc_config * c,
                              const double * params,
                              int per_instance_params,
                              int batch,
                              const double * current_t,
                              const double * current_x,
                              double * x,
                              double * u,
                              double * lambda,
                              double * s,
                              double * nu,
                              double * barrier_eps,
                              int n_ticks,
                              double sim_dt,
                              int substeps,
                              double * x_log,
                              double * u0_log,
                              int * status_log,
                              int * iter_log,
                              int n_threads)
  {
    return dispatch(model, [&](auto mdl0) {
      using M = decltype(mdl0);
      constexpr int N = M::N, MM = M::M, G = M::G;
      const Config cfg = toConfig(c);
      const size_t T = cfg.horizon_steps;
      parallelFor(batch, n_threads, [&](size_t b) {
        const M mdl = fromParams<M>(params, per_instance_params, b);
        double t = current_t[b], xt[N];
        std::copy(current_x + b * N, current_x + (b + 1) * N, xt);
        double * u0 = u + b * T * MM;
        for(int k = 0; k < n_ticks; k++)
        {
          const size_t row = b * n_ticks + k;
          std::copy(xt, xt + N, x_log + row * N);
          iter_log[row] = 0;
          status_log[row] = solveOne(mdl, cfg, t, xt, x + b * (T + 1) * N, u0, lambda + b * (T + 1) * N, s + b * T * G,
                                     nu + b * T * G, barrier_eps + b, iter_log + row, nullptr, nullptr, nullptr, nullptr, nullptr,
                                     nullptr, nullptr);
          int m0 = MM, g0 = G;
          if constexpr(HasStepDims<M>::value)
          {
            mdl.dims(t, m0, g0);
          }
          for(int a = 0; a < MM; a++)
          {
            u0_log[row * MM + a] = a < m0 ? u0[a] : 0.0;
          }
          const double tick_t = t;
          for(int sub = 0; sub < substeps; sub++)
          {
            double next[N];
            mdl.stateEqDt(tick_t, xt, u0, sim_dt, next);
            std::copy(next, next + N, xt);
            t += sim_dt;
          }
        }
      });
      return 0;
    });
  }

  /** Model evaluation for the derivative checks and the plant step of the closed-loop tests.  Every output may be NULL.
      step_dt > 0: f = stateEq(t, x, u, step_dt) (TestFmpcOscillator.cpp:27, TestFmpcCartPole.cpp:73), else stateEq(t, x, u). */
  int oracle_fmpc_eval(const char * model,
                       const double * params,
                       double t,
                       const double * x,
                       const double * u,
                       double step_dt,
                       double * f,
                       double * g,
                       double * costs, // [running, terminal]
                       double * A,
                       double * B,
                       double * C,
                       double * D,
                       double * Lx,
                       double * Lu,
                       double * Lxx,
                       double * Luu,
                       double * Lxu,
                       double * Vx,
                       double * Vxx)
  {
    return dispatch(model, [&](auto mdl0) {
      using M = decltype(mdl0);
      const M mdl = fromParams<M>(params);
      if(f)
      {
        if(step_dt > 0)
        {
          mdl.stateEqDt(t, x, u, step_dt, f);
        }
        else
        {
          mdl.stateEq(t, x, u, f);
        }
      }
      if(g)
      {
        mdl.ineqConst(t, x, u, g);
      }
      if(costs)
      {
        costs[0] = mdl.runningCost(t, x, u);
        costs[1] = mdl.terminalCost(t, x);
      }
      if(A && B)
      {
        mdl.calcStateEqDeriv(t, x, u, A, B);
      }
      if(C && D)
      {
        mdl.calcIneqConstDeriv(t, x, u, C, D);
      }
      if(Lx && Lu && Lxx && Luu && Lxu)
      {
        mdl.calcRunningCostDeriv(t, x, u, Lx, Lu, Lxx, Luu, Lxu);
      }
      if(Vx && Vxx)
      {
        mdl.calcTerminalCostDeriv(t, x, Vx, Vxx);
      }
      return 0;
    });
  }

  double oracle_fmpc_l1_dir_deriv(const double * func, const double * jac, const double * dir, int out_dim, int in_dim)
  {
    return l1NormDirectionalDeriv(func, jac, out_dim, dir, out_dim, in_dim);
  }

  /** x = G^-1 b through the LDLT restatement (b: n x c column-major, in place).  Returns 1 if info() == Success. */
  int oracle_fmpc_ldlt_solve(const double * G, int n, double * b, int c, int use_lu)
  {
    if(n > 8)
    {
      return -1;
    }
    if(use_lu)
    {
      fullPivLuSolveInPlace(G, n, b, c);
      return 1;
    }
    Ldlt l;
    const bool ok = l.compute(G, n);
    l.solveInPlace(b, c);
    return ok ? 1 : 0;
  }
}
