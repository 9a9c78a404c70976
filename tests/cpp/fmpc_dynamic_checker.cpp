// TEST INFRASTRUCTURE — NOT PRODUCT CODE.
//
// CPU checker of the batched FMPC solver for problems with TIME-VARYING input / inequality dimensions: FmpcSolver::solve
// (nmpc_fmpc's FmpcSolver.hpp:156-255) with every step i of the horizon sized m(i) = inputDim(t + i dt), g(i) = ineqDim(t + i dt),
// on plain arrays.  The variable is kept padded to the capacities, as at the library's boundary (include/nmpc_hip_fmpc.h):
// x [T+1][N], u [T][MC], lambda [T+1][N], s / nu [T][GC]; the entries beyond a step's dimensions are never read nor written, the
// gains and deltas there are 0.  Conventions follow oracle/fmpc_oracle.hpp (summation order, Eigen's LDLT pivot rule on the
// m(i) x m(i) block, the full-pivot fallback); on the three fixed-dimension models the tests pin this checker to that oracle.
// Built by tests/fmpc_dynamic_checker.py with g++ -O2 -ffp-contract=off into a temporary directory.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <thread>
#include <vector>

#include "../../oracle/fmpc_models.hpp"

namespace
{
constexpr int kMaxN = 8, kMaxM = 8, kMaxG = 8;

/** Adapter of a fixed-dimension oracle model: m(t) = M, g(t) = G. */
template<class Om>
struct Fixed
{
  static constexpr int N = Om::N, MC = Om::M, GC = Om::G;
  Om m;
  double dt() const { return m.dt; }
  void dims(double, int & mi, int & gi) const { mi = MC; gi = GC; }
  void stateEq(double t, const double * x, const double * u, int, double * out) const { m.stateEq(t, x, u, out); }
  void stateEqDt(double t, const double * x, const double * u, int, double step, double * out) const { m.stateEqDt(t, x, u, step, out); }
  double runningCost(double t, const double * x, const double * u, int) const { return m.runningCost(t, x, u); }
  double terminalCost(double t, const double * x) const { return m.terminalCost(t, x); }
  void ineqConst(double t, const double * x, const double * u, int, int, double * g) const { m.ineqConst(t, x, u, g); }
  void calcStateEqDeriv(double t, const double * x, const double * u, int, double * A, double * B) const { m.calcStateEqDeriv(t, x, u, A, B); }
  void calcRunningCostDeriv(double t, const double * x, const double * u, int, double * Lx, double * Lu, double * Lxx, double * Luu,
                            double * Lxu) const
  {
    m.calcRunningCostDeriv(t, x, u, Lx, Lu, Lxx, Luu, Lxu);
  }
  void calcTerminalCostDeriv(double t, const double * x, double * Lx, double * Lxx) const { m.calcTerminalCostDeriv(t, x, Lx, Lxx); }
  void calcIneqConstDeriv(double t, const double * x, const double * u, int, int, double * C, double * D) const
  {
    m.calcIneqConstDeriv(t, x, u, C, D);
  }
};

/** fmpc_vertical (include/nmpc_amd/models/FmpcVerticalMotion.hpp) restated: state [z, vz], one force per contact, rows
    f_min - f_j <= 0, f_j - f_max <= 0.  Same memory image as the library's problem object (14 doubles). */
struct Vertical
{
  static constexpr int N = 2, MC = 2, GC = 4;
  static constexpr double g_ = 9.80665;
  double dt_ = 0.01;
  double running_x[2] = {1.0, 1e-3};
  double running_u = 1e-3;
  double terminal_x[2] = {1.0, 1e-3};
  double mass = 1.0, f_min = 0.0, f_max = 30.0, ref_switch_t = 8.0;
  double ds_begin = 2.0, ds_end = 3.0, fl_begin = 4.5, fl_end = 5.0;

  double dt() const { return dt_; }
  int inputDim(double t) const
  {
    t += 1e-6;
    if(ds_begin < t && t < ds_end)
    {
      return 2;
    }
    if(fl_begin < t && t < fl_end)
    {
      return 0;
    }
    return 1;
  }
  void dims(double t, int & mi, int & gi) const
  {
    mi = inputDim(t);
    gi = 2 * mi;
  }
  double refPos(double t) const
  {
    t += 1e-6;
    return (t < ref_switch_t) ? 1.0 : 0.0;
  }
  void stateEqDt(double, const double * x, const double * u, int m, double step, double * out) const
  {
    double force = 0;
    for(int j = 0; j < m; j++)
    {
      force += u[j];
    }
    out[0] = x[0] + step * x[1];
    out[1] = x[1] + step * (force / mass - g_);
  }
  void stateEq(double t, const double * x, const double * u, int m, double * out) const { stateEqDt(t, x, u, m, dt_, out); }
  double runningCost(double t, const double * x, const double * u, int m) const
  {
    const double e0 = x[0] - refPos(t), e1 = x[1];
    double uu = 0;
    for(int j = 0; j < m; j++)
    {
      uu += u[j] * u[j];
    }
    return 0.5 * (running_x[0] * (e0 * e0) + running_x[1] * (e1 * e1)) + 0.5 * running_u * uu;
  }
  double terminalCost(double t, const double * x) const
  {
    const double e0 = x[0] - refPos(t), e1 = x[1];
    return 0.5 * (terminal_x[0] * (e0 * e0) + terminal_x[1] * (e1 * e1));
  }
  void ineqConst(double, const double *, const double * u, int m, int, double * g) const
  {
    for(int j = 0; j < m; j++)
    {
      g[2 * j] = f_min - u[j];
      g[2 * j + 1] = u[j] - f_max;
    }
  }
  void calcStateEqDeriv(double, const double *, const double *, int m, double * A, double * B) const
  {
    A[0] = 1;
    A[1] = 0;
    A[2] = dt_;
    A[3] = 1;
    for(int j = 0; j < m; j++)
    {
      B[0 + 2 * j] = 0;
      B[1 + 2 * j] = (1.0 / mass) * dt_;
    }
  }
  void calcRunningCostDeriv(double t, const double * x, const double * u, int m, double * Lx, double * Lu, double * Lxx, double * Luu,
                            double * Lxu) const
  {
    Lx[0] = running_x[0] * (x[0] - refPos(t));
    Lx[1] = running_x[1] * x[1];
    Lxx[0] = running_x[0];
    Lxx[1] = 0;
    Lxx[2] = 0;
    Lxx[3] = running_x[1];
    for(int j = 0; j < m; j++)
    {
      Lu[j] = running_u * u[j];
      Lxu[0 + 2 * j] = 0;
      Lxu[1 + 2 * j] = 0;
      for(int k = 0; k < m; k++)
      {
        Luu[k + j * m] = (j == k) ? running_u : 0.0;
      }
    }
  }
  void calcTerminalCostDeriv(double t, const double * x, double * Lx, double * Lxx) const
  {
    Lx[0] = terminal_x[0] * (x[0] - refPos(t));
    Lx[1] = terminal_x[1] * x[1];
    Lxx[0] = terminal_x[0];
    Lxx[1] = 0;
    Lxx[2] = 0;
    Lxx[3] = terminal_x[1];
  }
  void calcIneqConstDeriv(double, const double *, const double *, int m, int g, double * C, double * D) const
  {
    for(int r = 0; r < g; r++)
    {
      C[r + 0 * g] = 0;
      C[r + 1 * g] = 0;
      for(int j = 0; j < m; j++)
      {
        D[r + j * g] = (r == 2 * j) ? -1.0 : ((r == 2 * j + 1) ? 1.0 : 0.0);
      }
    }
  }
};

/** Eigen::LDLT<Matrix, Lower> of an n x n matrix (column-major), as oracle/fmpc_oracle.hpp restates it. */
struct Ldlt
{
  int n = 0;
  double a[kMaxM * kMaxM];
  int tr[kMaxM];
  bool compute(const double * G, int n_)
  {
    n = n_;
    for(int i = 0; i < n * n; i++)
    {
      a[i] = G[i];
    }
    if(n <= 1)
    {
      if(n == 1)
      {
        tr[0] = 0;
      }
      return true;
    }
    bool found_zero_pivot = false, ret = true;
    auto A = [&](int i, int j) -> double & { return a[i + j * n]; };
    for(int k = 0; k < n; k++)
    {
      int p = k;
      double big = std::abs(A(k, k));
      for(int i = k + 1; i < n; i++)
      {
        if(std::abs(A(i, i)) > big)
        {
          big = std::abs(A(i, i));
          p = i;
        }
      }
      tr[k] = p;
      if(p != k)
      {
        for(int j = 0; j < k; j++)
        {
          std::swap(A(k, j), A(p, j));
        }
        for(int i = p + 1; i < n; i++)
        {
          std::swap(A(i, k), A(i, p));
        }
        std::swap(A(k, k), A(p, p));
        for(int i = k + 1; i < p; i++)
        {
          std::swap(A(i, k), A(p, i));
        }
      }
      if(k > 0)
      {
        double temp[kMaxM];
        double acc = 0;
        for(int j = 0; j < k; j++)
        {
          temp[j] = A(j, j) * A(k, j);
          acc += A(k, j) * temp[j];
        }
        A(k, k) -= acc;
        for(int i = k + 1; i < n; i++)
        {
          double sum = 0;
          for(int j = 0; j < k; j++)
          {
            sum += A(i, j) * temp[j];
          }
          A(i, k) -= sum;
        }
      }
      const double akk = A(k, k);
      const bool valid = std::abs(akk) > 0.0;
      if(k == 0 && !valid)
      {
        for(int j = 0; j < n; j++)
        {
          tr[j] = j;
          for(int i = j + 1; i < n; i++)
          {
            ret = ret && (A(i, j) == 0.0);
          }
        }
        return ret;
      }
      if(valid)
      {
        for(int i = k + 1; i < n; i++)
        {
          A(i, k) /= akk;
        }
      }
      else
      {
        for(int i = k + 1; i < n; i++)
        {
          ret = ret && (A(i, k) == 0.0);
        }
      }
      if(found_zero_pivot && valid)
      {
        ret = false;
      }
      else if(!valid)
      {
        found_zero_pivot = true;
      }
    }
    return ret;
  }
  void solveInPlace(double * x) const
  {
    if(n == 1)
    {
      x[0] = std::abs(a[0]) > std::numeric_limits<double>::min() ? x[0] / a[0] : 0.0;
      return;
    }
    for(int k = 0; k < n; k++)
    {
      std::swap(x[k], x[tr[k]]);
    }
    for(int i = 0; i < n; i++)
    {
      for(int j = 0; j < i; j++)
      {
        x[i] -= a[i + j * n] * x[j];
      }
    }
    for(int i = 0; i < n; i++)
    {
      x[i] = std::abs(a[i + i * n]) > std::numeric_limits<double>::min() ? x[i] / a[i + i * n] : 0.0;
    }
    for(int i = n - 1; i >= 0; i--)
    {
      for(int j = i + 1; j < n; j++)
      {
        x[i] -= a[j + i * n] * x[j];
      }
    }
    for(int k = n - 1; k >= 0; k--)
    {
      std::swap(x[k], x[tr[k]]);
    }
  }
};

/** Full-pivot Gaussian elimination, one right-hand side (the FullPivLU fallback). */
void fullPivLuSolveInPlace(const double * Gm, int n, double * b)
{
  double a[kMaxM * kMaxM];
  int colperm[kMaxM];
  std::copy(Gm, Gm + n * n, a);
  for(int i = 0; i < n; i++)
  {
    colperm[i] = i;
  }
  int rank = 0;
  for(int k = 0; k < n; k++)
  {
    int pr = k, pc = k;
    double big = 0;
    for(int j = k; j < n; j++)
    {
      for(int i = k; i < n; i++)
      {
        if(std::abs(a[i + j * n]) > big)
        {
          big = std::abs(a[i + j * n]);
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
    for(int j = 0; j < n; j++)
    {
      std::swap(a[k + j * n], a[pr + j * n]);
    }
    std::swap(b[k], b[pr]);
    for(int i = 0; i < n; i++)
    {
      std::swap(a[i + k * n], a[i + pc * n]);
    }
    std::swap(colperm[k], colperm[pc]);
    for(int i = k + 1; i < n; i++)
    {
      const double f = a[i + k * n] / a[k + k * n];
      for(int j = k + 1; j < n; j++)
      {
        a[i + j * n] -= f * a[k + j * n];
      }
      b[i] -= f * b[k];
    }
  }
  double y[kMaxM];
  for(int i = n - 1; i >= 0; i--)
  {
    if(i >= rank)
    {
      y[i] = 0;
      continue;
    }
    double sum = b[i];
    for(int j = i + 1; j < rank; j++)
    {
      sum -= a[i + j * n] * y[j];
    }
    y[i] = sum / a[i + i * n];
  }
  for(int i = 0; i < n; i++)
  {
    b[colperm[i]] = y[i];
  }
}

double l1Deriv(const double * func, const double * jac, const double * dir, int out_dim, int in_dim)
{
  double deriv = 0.0;
  for(int i = 0; i < out_dim; i++)
  {
    double d = 0;
    for(int j = 0; j < in_dim; j++)
    {
      d += jac[i + j * out_dim] * dir[j];
    }
    deriv += func[i] > 0 ? d : (func[i] < 0 ? -1 * d : std::abs(d));
  }
  return deriv;
}

struct Config
{
  int T, max_iter, check_nan, init_complementary_variable, update_barrier_eps, break_if_llt_fails, enable_line_search,
      merit_const_scale_from_lagrange_multipliers;
  double kkt_error_thre;
};

/** Outputs of one instance (pointers into the caller's [B]... arrays; any may be null). */
struct Out
{
  int * status;
  int * iters;
  double * trace; // [max_iter][6]: iter, kkt_error, barrier_eps, alpha_s_max, alpha_nu_max, alpha_s
  double *dx, *du, *dlam, *ds, *dnu; // padded like the variable
  double *gk, *gK, *gs, *gP; // [T][MC], [T][N][MC] (entry (a, c) at c MC + a), [T+1][N], [T+1][N][N]
  double * merit; // [3]
};

template<class Model>
class Solver
{
public:
  static constexpr int N = Model::N, MC = Model::MC, GC = Model::GC;
  static_assert(N <= kMaxN && MC <= kMaxM && GC <= kMaxG, "checker capacity");

  struct Coef
  {
    int m = 0, g = 0;
    double A[N * N], B[N * MC + 1], C[GC * N + 1], D[GC * MC + 1];
    double Lx[N], Lu[MC + 1], Lxx[N * N], Luu[MC * MC + 1], Lxu[N * MC + 1];
    double x_bar[N], g_bar[GC + 1], Lx_bar[N], Lu_bar[MC + 1];
    double k[MC + 1], K[MC * N + 1], s[N], P[N * N];
  };

  Solver(const Model & p, const Config & c) : pr(p), cfg(c) {}

  /** One solve from the variable in (x, u, lam, s, nu), which it updates.  barrier_eps in / out. */
  int solve(double t0_, const double * x0_, double * x, double * u, double * lam, double * s, double * nu, double & barrier_eps, Out & o)
  {
    T = cfg.T;
    t0 = t0_;
    std::copy(x0_, x0_ + N, x0);
    X = x;
    U = u;
    LAM = lam;
    S = s;
    NU = nu;
    eps = barrier_eps;
    co.assign(T + 1, Coef());
    d_x.assign((T + 1) * N, 0.0);
    d_u.assign(T * MC, 0.0);
    d_lam.assign((T + 1) * N, 0.0);
    d_s.assign(T * GC, 0.0);
    d_nu.assign(T * GC, 0.0);
    for(int i = 0; i < T; i++)
    {
      pr.dims(t0 + i * pr.dt(), co[i].m, co[i].g);
    }
    if(o.trace)
    {
      std::fill(o.trace, o.trace + cfg.max_iter * 6, 0.0);
    }
    if(cfg.init_complementary_variable) // :170-187
    {
      eps = 1e-4;
      for(int i = 0; i < T; i++)
      {
        const int m = co[i].m, g = co[i].g;
        double gv[kMaxG];
        pr.ineqConst(t0 + i * pr.dt(), &X[i * N], &U[i * MC], m, g, gv);
        for(int j = 0; j < g; j++)
        {
          const double sj = (1.0 + 1e-2) * std::max(-1 * gv[j], 1e-2);
          S[i * GC + j] = sj;
          NU[i * GC + j] = (1.0 + 1e-2) * std::max(1e-4 * (1.0 / sj), 1e-2);
        }
      }
    }
    int status = 0;
    int iters = 0;
    bool invalid = false;
    for(int i = 0; i < T && !invalid; i++) // checkVariable (:338-353), active rows only
    {
      for(int j = 0; j < co[i].g; j++)
      {
        if(S[i * GC + j] < 0 || NU[i * GC + j] < 0)
        {
          invalid = true;
        }
      }
    }
    if(invalid)
    {
      status = -2;
    }
    else
    {
      status = 6;
      for(int iter = 1; iter <= cfg.max_iter; iter++)
      {
        iters = iter;
        status = procOnce(iter, o);
        if(status != 6)
        {
          break;
        }
      }
      if(status == 6)
      {
        status = 5;
      }
    }
    barrier_eps = eps;
    if(o.status)
    {
      *o.status = status;
    }
    if(o.iters)
    {
      *o.iters = iters;
    }
    auto put = [](double * dst, const std::vector<double> & src) {
      if(dst)
      {
        std::copy(src.begin(), src.end(), dst);
      }
    };
    put(o.dx, d_x);
    put(o.du, d_u);
    put(o.dlam, d_lam);
    put(o.ds, d_s);
    put(o.dnu, d_nu);
    for(int i = 0; i <= T; i++)
    {
      const Coef & c = co[i];
      if(i < T)
      {
        for(int a = 0; a < MC; a++)
        {
          if(o.gk)
          {
            o.gk[i * MC + a] = a < c.m ? c.k[a] : 0.0;
          }
          for(int q = 0; q < N; q++)
          {
            if(o.gK)
            {
              o.gK[(i * N + q) * MC + a] = a < c.m ? c.K[a + q * c.m] : 0.0;
            }
          }
        }
      }
      for(int a = 0; a < N; a++)
      {
        if(o.gs)
        {
          o.gs[i * N + a] = c.s[a];
        }
        for(int q = 0; q < N; q++)
        {
          if(o.gP)
          {
            o.gP[(i * N + q) * N + a] = c.P[a + q * N];
          }
        }
      }
    }
    if(o.merit)
    {
      o.merit[0] = merit_func;
      o.merit[1] = merit_deriv;
      o.merit[2] = merit_scale;
    }
    return status;
  }

private:
  int procOnce(int iter, Out & o)
  {
    double * row = o.trace ? o.trace + (iter - 1) * 6 : nullptr;
    if(cfg.update_barrier_eps) // :370-392 over the active rows
    {
      double ave = 0;
      int rows = 0;
      for(int i = 0; i < T; i++)
      {
        double dot = 0;
        for(int j = 0; j < co[i].g; j++)
        {
          dot += S[i * GC + j] * NU[i * GC + j];
        }
        ave += dot;
        rows += co[i].g;
      }
      ave /= rows;
      const double v = 0.5 * ave;
      eps = (v < 1e-8) ? 1e-8 : ((1e6 < v) ? 1e6 : v); // std::clamp (a NaN passes through)
    }
    if(row)
    {
      row[0] = iter;
      row[2] = eps;
    }
    const double dt = pr.dt();
    for(int i = 0; i < T; i++) // :394-441
    {
      Coef & c = co[i];
      const int m = c.m, g = c.g;
      const double t = t0 + i * dt;
      const double *x = &X[i * N], *nx = &X[(i + 1) * N], *u = &U[i * MC], *l = &LAM[i * N], *nl = &LAM[(i + 1) * N];
      const double *s = &S[i * GC], *nu = &NU[i * GC];
      pr.calcStateEqDeriv(t, x, u, m, c.A, c.B);
      pr.calcIneqConstDeriv(t, x, u, m, g, c.C, c.D);
      pr.calcRunningCostDeriv(t, x, u, m, c.Lx, c.Lu, c.Lxx, c.Luu, c.Lxu);
      double f[kMaxN], gv[kMaxG];
      pr.stateEq(t, x, u, m, f);
      pr.ineqConst(t, x, u, m, g, gv);
      for(int a = 0; a < N; a++)
      {
        c.x_bar[a] = f[a] - nx[a];
      }
      for(int a = 0; a < g; a++)
      {
        c.g_bar[a] = gv[a] + s[a];
      }
      for(int a = 0; a < N; a++)
      {
        double at = 0, ct = 0;
        for(int r = 0; r < N; r++)
        {
          at += c.A[r + a * N] * nl[r];
        }
        for(int r = 0; r < g; r++)
        {
          ct += c.C[r + a * g] * nu[r];
        }
        c.Lx_bar[a] = ((-1 * l[a] + dt * c.Lx[a]) + at) + ct;
      }
      for(int a = 0; a < m; a++)
      {
        double bt = 0, dn = 0;
        for(int r = 0; r < N; r++)
        {
          bt += c.B[r + a * N] * nl[r];
        }
        for(int r = 0; r < g; r++)
        {
          dn += c.D[r + a * g] * nu[r];
        }
        c.Lu_bar[a] = (dt * c.Lu[a] + bt) + dn;
      }
    }
    {
      Coef & c = co[T];
      pr.calcTerminalCostDeriv(t0 + T * dt, &X[T * N], c.Lx, c.Lxx);
      for(int a = 0; a < N; a++)
      {
        c.Lx_bar[a] = c.Lx[a] - LAM[T * N + a];
      }
    }
    // calcKktError(0) (:493-520)
    double kkt = 0;
    auto sq = [](const double * p, int n) {
      double r = 0;
      for(int i = 0; i < n; i++)
      {
        r += p[i] * p[i];
      }
      return r;
    };
    for(int a = 0; a < N; a++)
    {
      const double e = x0[a] - X[a];
      kkt += e * e;
    }
    for(int i = 0; i < T; i++)
    {
      const Coef & c = co[i];
      kkt += sq(c.x_bar, N);
      kkt += sq(c.g_bar, c.g);
      kkt += sq(c.Lx_bar, N);
      kkt += sq(c.Lu_bar, c.m);
      double comp = 0;
      for(int j = 0; j < c.g; j++)
      {
        const double e = std::max(S[i * GC + j] * NU[i * GC + j], 0.0);
        comp += e * e;
      }
      kkt += comp;
    }
    kkt += sq(co[T].Lx_bar, N);
    kkt = std::sqrt(kkt);
    if(row)
    {
      row[1] = kkt;
    }
    if(kkt <= cfg.kkt_error_thre)
    {
      return 1;
    }
    if(!backwardPass())
    {
      return 3;
    }
    if(!forwardPass())
    {
      return 2;
    }
    if(!updateVariables(row))
    {
      return 4;
    }
    return 6;
  }

  static bool bad(const double * p, int n)
  {
    for(int i = 0; i < n; i++)
    {
      if(std::isnan(p[i]) || std::isinf(p[i]))
      {
        return true;
      }
    }
    return false;
  }

  bool backwardPass() // :522-665 on the m(i) inputs and g(i) rows of every step
  {
    const double dt = pr.dt();
    double s[N], P[N * N];
    {
      Coef & tc = co[T];
      for(int a = 0; a < N; a++)
      {
        s[a] = -1 * tc.Lx_bar[a];
      }
      std::copy(tc.Lxx, tc.Lxx + N * N, P);
      std::copy(s, s + N, tc.s);
      std::copy(P, P + N * N, tc.P);
    }
    for(int i = T - 1; i >= 0; i--)
    {
      Coef & c = co[i];
      const int m = c.m, g = c.g;
      const double *sv = &S[i * GC], *nuv = &NU[i * GC];
      double nu_s[kMaxG], tsub[kMaxG];
      for(int j = 0; j < g; j++)
      {
        nu_s[j] = nuv[j] / sv[j];
        tsub[j] = (nu_s[j] * c.g_bar[j] - nuv[j]) + eps * (1.0 / sv[j]);
      }
      double Qxx[N * N], Quu[kMaxM * kMaxM], Qxu[kMaxN * kMaxM], Lx_t[N], Lu_t[kMaxM];
      for(int b = 0; b < N; b++)
      {
        for(int a = 0; a < N; a++)
        {
          double acc = 0;
          for(int j = 0; j < g; j++)
          {
            acc += (c.C[j + a * g] * nu_s[j]) * c.C[j + b * g];
          }
          Qxx[a + b * N] = dt * c.Lxx[a + b * N] + acc;
        }
      }
      for(int b = 0; b < m; b++)
      {
        for(int a = 0; a < m; a++)
        {
          double acc = 0;
          for(int j = 0; j < g; j++)
          {
            acc += (c.D[j + a * g] * nu_s[j]) * c.D[j + b * g];
          }
          Quu[a + b * m] = dt * c.Luu[a + b * m] + acc;
        }
        for(int a = 0; a < N; a++)
        {
          double acc = 0;
          for(int j = 0; j < g; j++)
          {
            acc += (c.C[j + a * g] * nu_s[j]) * c.D[j + b * g];
          }
          Qxu[a + b * N] = dt * c.Lxu[a + b * N] + acc;
        }
      }
      for(int a = 0; a < N; a++)
      {
        double acc = 0;
        for(int j = 0; j < g; j++)
        {
          acc += c.C[j + a * g] * tsub[j];
        }
        Lx_t[a] = c.Lx_bar[a] + acc;
      }
      for(int a = 0; a < m; a++)
      {
        double acc = 0;
        for(int j = 0; j < g; j++)
        {
          acc += c.D[j + a * g] * tsub[j];
        }
        Lu_t[a] = c.Lu_bar[a] + acc;
      }
      double AtP[N * N], BtP[kMaxM * kMaxN];
      for(int b = 0; b < N; b++)
      {
        for(int a = 0; a < N; a++)
        {
          double acc = 0;
          for(int r = 0; r < N; r++)
          {
            acc += c.A[r + a * N] * P[r + b * N];
          }
          AtP[a + b * N] = acc;
        }
        for(int a = 0; a < m; a++)
        {
          double acc = 0;
          for(int r = 0; r < N; r++)
          {
            acc += c.B[r + a * N] * P[r + b * N];
          }
          BtP[a + b * m] = acc;
        }
      }
      double F[N * N], H[kMaxN * kMaxM], Gm[kMaxM * kMaxM];
      for(int b = 0; b < N; b++)
      {
        for(int a = 0; a < N; a++)
        {
          double acc = 0;
          for(int r = 0; r < N; r++)
          {
            acc += AtP[a + r * N] * c.A[r + b * N];
          }
          F[a + b * N] = Qxx[a + b * N] + acc;
        }
      }
      for(int b = 0; b < m; b++)
      {
        for(int a = 0; a < N; a++)
        {
          double acc = 0;
          for(int r = 0; r < N; r++)
          {
            acc += AtP[a + r * N] * c.B[r + b * N];
          }
          H[a + b * N] = Qxu[a + b * N] + acc;
        }
        for(int a = 0; a < m; a++)
        {
          double acc = 0;
          for(int r = 0; r < N; r++)
          {
            acc += BtP[a + r * m] * c.B[r + b * N];
          }
          Gm[a + b * m] = Quu[a + b * m] + acc;
        }
      }
      double Px_s[N];
      for(int a = 0; a < N; a++)
      {
        double acc = 0;
        for(int r = 0; r < N; r++)
        {
          acc += P[a + r * N] * c.x_bar[r];
        }
        Px_s[a] = acc - s[a];
      }
      double k[kMaxM], K[kMaxM * kMaxN];
      if(m > 0)
      {
        for(int a = 0; a < m; a++)
        {
          double acc = 0;
          for(int r = 0; r < N; r++)
          {
            acc += c.B[r + a * N] * Px_s[r];
          }
          k[a] = acc + Lu_t[a];
        }
        for(int b = 0; b < N; b++)
        {
          for(int a = 0; a < m; a++)
          {
            K[a + b * m] = H[b + a * N];
          }
        }
        Ldlt ldlt;
        if(ldlt.compute(Gm, m))
        {
          ldlt.solveInPlace(k);
          for(int b = 0; b < N; b++)
          {
            ldlt.solveInPlace(K + b * m);
          }
        }
        else
        {
          if(cfg.break_if_llt_fails)
          {
            return false;
          }
          fullPivLuSolveInPlace(Gm, m, k);
          for(int b = 0; b < N; b++)
          {
            fullPivLuSolveInPlace(Gm, m, K + b * m);
          }
        }
        for(int a = 0; a < m; a++)
        {
          k[a] = -1 * k[a];
        }
        for(int a = 0; a < m * N; a++)
        {
          K[a] = -1 * K[a];
        }
      }
      double s_new[N], P_new[N * N];
      for(int a = 0; a < N; a++)
      {
        double at = 0, hk = 0;
        for(int r = 0; r < N; r++)
        {
          at += c.A[r + a * N] * (-1 * Px_s[r]);
        }
        for(int r = 0; r < m; r++)
        {
          hk += H[a + r * N] * k[r];
        }
        s_new[a] = (at - Lx_t[a]) - hk;
      }
      double KtG[kMaxN * kMaxM];
      for(int b = 0; b < m; b++)
      {
        for(int a = 0; a < N; a++)
        {
          double acc = 0;
          for(int r = 0; r < m; r++)
          {
            acc += K[r + a * m] * Gm[r + b * m];
          }
          KtG[a + b * N] = acc;
        }
      }
      for(int b = 0; b < N; b++)
      {
        for(int a = 0; a < N; a++)
        {
          double acc = 0;
          for(int r = 0; r < m; r++)
          {
            acc += KtG[a + r * N] * K[r + b * m];
          }
          P_new[a + b * N] = F[a + b * N] - acc;
        }
      }
      for(int b = 0; b < N; b++)
      {
        for(int a = 0; a < N; a++)
        {
          P[a + b * N] = 0.5 * (P_new[a + b * N] + P_new[b + a * N]);
        }
      }
      std::copy(s_new, s_new + N, s);
      std::copy(k, k + m, c.k);
      std::copy(K, K + m * N, c.K);
      std::copy(s, s + N, c.s);
      std::copy(P, P + N * N, c.P);
    }
    if(cfg.check_nan) // Coefficient::containsNaN over what each step holds
    {
      for(int i = 0; i <= T; i++)
      {
        const Coef & c = co[i];
        if(i == T)
        {
          if(bad(c.Lx, N) || bad(c.Lxx, N * N) || bad(c.Lx_bar, N) || bad(c.s, N) || bad(c.P, N * N))
          {
            return false;
          }
          continue;
        }
        const int m = c.m, g = c.g;
        if(bad(c.A, N * N) || bad(c.B, N * m) || bad(c.C, g * N) || bad(c.D, g * m) || bad(c.Lx, N) || bad(c.Lu, m) || bad(c.Lxx, N * N)
           || bad(c.Luu, m * m) || bad(c.Lxu, N * m) || bad(c.x_bar, N) || bad(c.g_bar, g) || bad(c.Lx_bar, N) || bad(c.Lu_bar, m)
           || bad(c.k, m) || bad(c.K, m * N) || bad(c.s, N) || bad(c.P, N * N))
        {
          return false;
        }
      }
    }
    return true;
  }

  bool forwardPass() // :667-708
  {
    for(int a = 0; a < N; a++)
    {
      d_x[a] = x0[a] - X[a];
    }
    for(int i = 0; i <= T; i++)
    {
      const Coef & c = co[i];
      const double * dx = &d_x[i * N];
      for(int a = 0; a < N; a++)
      {
        double acc = 0;
        for(int r = 0; r < N; r++)
        {
          acc += c.P[a + r * N] * dx[r];
        }
        d_lam[i * N + a] = acc - c.s[a];
      }
      if(i < T)
      {
        const int m = c.m;
        double * du = &d_u[i * MC];
        for(int a = 0; a < m; a++)
        {
          double acc = 0;
          for(int r = 0; r < N; r++)
          {
            acc += c.K[a + r * m] * dx[r];
          }
          du[a] = acc + c.k[a];
        }
        for(int a = 0; a < N; a++)
        {
          double ax = 0, bu = 0;
          for(int r = 0; r < N; r++)
          {
            ax += c.A[a + r * N] * dx[r];
          }
          for(int r = 0; r < m; r++)
          {
            bu += c.B[a + r * N] * du[r];
          }
          d_x[(i + 1) * N + a] = (ax + bu) + c.x_bar[a];
        }
      }
    }
    bool nan = bad(d_x.data(), (T + 1) * N) || bad(d_lam.data(), (T + 1) * N);
    for(int i = 0; i < T; i++)
    {
      const Coef & c = co[i];
      const int m = c.m, g = c.g;
      const double *dx = &d_x[i * N], *du = &d_u[i * MC];
      nan = nan || bad(du, m);
      for(int j = 0; j < g; j++)
      {
        double cx = 0, dd = 0;
        for(int r = 0; r < N; r++)
        {
          cx += c.C[j + r * g] * dx[r];
        }
        for(int r = 0; r < m; r++)
        {
          dd += c.D[j + r * g] * du[r];
        }
        const double ds = -1 * ((cx + dd) + c.g_bar[j]);
        d_s[i * GC + j] = ds;
        const double sv = S[i * GC + j], nv = NU[i * GC + j];
        d_nu[i * GC + j] = -1 * (nv * (ds + sv) - eps) / sv;
        nan = nan || bad(&d_s[i * GC + j], 1) || bad(&d_nu[i * GC + j], 1);
      }
    }
    return !(cfg.check_nan && nan);
  }

  bool updateVariables(double * row) // :710-838
  {
    double a_s = 1.0, a_nu = 1.0;
    for(int i = 0; i < T; i++)
    {
      for(int j = 0; j < co[i].g; j++)
      {
        const int k = i * GC + j;
        if(d_s[k] < 0)
        {
          a_s = std::min(a_s, -1 * 0.995 * S[k] / d_s[k]);
        }
        if(d_nu[k] < 0)
        {
          a_nu = std::min(a_nu, -1 * 0.995 * NU[k] / d_nu[k]);
        }
      }
    }
    if(row)
    {
      row[3] = a_s;
      row[4] = a_nu;
      row[5] = a_s;
    }
    if(!(a_s > 0.0 && a_s <= 1.0 && a_nu > 0.0 && a_nu <= 1.0))
    {
      return false;
    }
    double alpha_s = a_s;
    if(cfg.enable_line_search)
    {
      setupMeritFunc();
      while(true)
      {
        if(alpha_s < 1e-10)
        {
          break;
        }
        if(meritAt(alpha_s) < merit_func + 1e-3 * alpha_s * merit_deriv)
        {
          break;
        }
        alpha_s *= 0.5;
      }
      if(row)
      {
        row[5] = alpha_s;
      }
    }
    for(int i = 0; i < (T + 1) * N; i++)
    {
      X[i] += alpha_s * d_x[i];
      LAM[i] += a_nu * d_lam[i];
    }
    for(int i = 0; i < T; i++)
    {
      for(int a = 0; a < co[i].m; a++)
      {
        U[i * MC + a] += alpha_s * d_u[i * MC + a];
      }
      bool s_neg = false, nu_neg = false;
      const int g = co[i].g;
      for(int j = 0; j < g; j++)
      {
        S[i * GC + j] += alpha_s * d_s[i * GC + j];
        NU[i * GC + j] += a_nu * d_nu[i * GC + j];
        s_neg = s_neg || S[i * GC + j] < 0;
        nu_neg = nu_neg || NU[i * GC + j] < 0;
      }
      for(int j = 0; j < g; j++)
      {
        if(s_neg)
        {
          S[i * GC + j] = std::max(S[i * GC + j], std::numeric_limits<double>::lowest());
        }
        if(nu_neg)
        {
          NU[i * GC + j] = std::max(NU[i * GC + j], std::numeric_limits<double>::lowest());
        }
      }
    }
    return true;
  }

  void setupMeritFunc() // :840-936
  {
    const double dt = pr.dt();
    double fo = 0, fc = 0, dobj = 0, dcon = 0;
    double negI[kMaxN * kMaxN] = {}, Ig[kMaxG * kMaxG] = {};
    for(int a = 0; a < N; a++)
    {
      negI[a + a * N] = -1;
    }
    auto l1 = [](const double * p, int n) {
      double r = 0;
      for(int i = 0; i < n; i++)
      {
        r += std::abs(p[i]);
      }
      return r;
    };
    auto dot = [](const double * p, const double * q, int n) {
      double r = 0;
      for(int i = 0; i < n; i++)
      {
        r += p[i] * q[i];
      }
      return r;
    };
    {
      double cf[kMaxN];
      for(int a = 0; a < N; a++)
      {
        cf[a] = x0[a] - X[a];
      }
      fc += l1(cf, N);
      dcon += l1Deriv(cf, negI, &d_x[0], N, N);
    }
    for(int i = 0; i < T; i++)
    {
      const Coef & c = co[i];
      const int m = c.m, g = c.g;
      const double t = t0 + i * dt;
      const double *x = &X[i * N], *u = &U[i * MC], *s = &S[i * GC], *nx = &X[(i + 1) * N];
      const double *dx = &d_x[i * N], *du = &d_u[i * MC], *ds = &d_s[i * GC], *dnx = &d_x[(i + 1) * N];
      fo += pr.runningCost(t, x, u, m) * dt;
      dobj += (dot(c.Lx, dx, N) + dot(c.Lu, du, m)) * dt;
      double logsum = 0, invdot = 0;
      for(int j = 0; j < g; j++)
      {
        logsum += std::log(s[j]);
        invdot += (1.0 / s[j]) * ds[j];
      }
      fo += -1 * eps * logsum;
      dobj += -1 * eps * invdot;
      {
        double f[kMaxN], cf[kMaxN];
        pr.stateEq(t, x, u, m, f);
        for(int a = 0; a < N; a++)
        {
          cf[a] = f[a] - nx[a];
        }
        fc += l1(cf, N);
        dcon += l1Deriv(cf, c.A, dx, N, N);
        dcon += l1Deriv(cf, c.B, du, N, m);
        dcon += l1Deriv(cf, negI, dnx, N, N);
      }
      {
        double gv[kMaxG], cf[kMaxG];
        pr.ineqConst(t, x, u, m, g, gv);
        for(int a = 0; a < g; a++)
        {
          cf[a] = gv[a] + s[a];
        }
        std::fill(Ig, Ig + kMaxG * kMaxG, 0.0);
        for(int a = 0; a < g; a++)
        {
          Ig[a + a * g] = 1;
        }
        fc += l1(cf, g);
        dcon += l1Deriv(cf, c.C, dx, g, N);
        dcon += l1Deriv(cf, c.D, du, g, m);
        dcon += l1Deriv(cf, Ig, ds, g, g);
      }
    }
    fo += pr.terminalCost(t0 + T * dt, &X[T * N]);
    dobj += dot(co[T].Lx, &d_x[T * N], N);
    if(cfg.merit_const_scale_from_lagrange_multipliers)
    {
      merit_scale = 1e-3;
      for(int i = 0; i < (T + 1) * N; i++)
      {
        merit_scale = std::max(merit_scale, std::abs(LAM[i]));
      }
      for(int i = 0; i < T; i++)
      {
        for(int j = 0; j < co[i].g; j++)
        {
          merit_scale = std::max(merit_scale, std::abs(NU[i * GC + j]));
        }
      }
    }
    else
    {
      merit_scale = std::max(dobj / ((1.0 - 0.5) * fc), 1e-3);
    }
    merit_func = fo + merit_scale * fc;
    merit_deriv = dobj + merit_scale * dcon;
  }

  double meritAt(double alpha) const // calcMeritFunc (:938-981) at variable + alpha delta
  {
    const double dt = pr.dt();
    double fo = 0, fc = 0;
    double x[kMaxN], nx[kMaxN];
    for(int a = 0; a < N; a++)
    {
      x[a] = X[a] + alpha * d_x[a];
      fc += std::abs(x0[a] - x[a]);
    }
    for(int i = 0; i < T; i++)
    {
      const int m = co[i].m, g = co[i].g;
      const double t = t0 + i * dt;
      double u[kMaxM], s[kMaxG];
      for(int a = 0; a < m; a++)
      {
        u[a] = U[i * MC + a] + alpha * d_u[i * MC + a];
      }
      for(int j = 0; j < g; j++)
      {
        s[j] = S[i * GC + j] + alpha * d_s[i * GC + j];
      }
      for(int a = 0; a < N; a++)
      {
        nx[a] = X[(i + 1) * N + a] + alpha * d_x[(i + 1) * N + a];
      }
      fo += pr.runningCost(t, x, u, m) * dt;
      double logsum = 0;
      for(int j = 0; j < g; j++)
      {
        logsum += std::log(s[j]);
      }
      fo += -1 * eps * logsum;
      double f[kMaxN], gv[kMaxG];
      pr.stateEq(t, x, u, m, f);
      double c1 = 0;
      for(int a = 0; a < N; a++)
      {
        c1 += std::abs(f[a] - nx[a]);
      }
      fc += c1;
      pr.ineqConst(t, x, u, m, g, gv);
      double c2 = 0;
      for(int a = 0; a < g; a++)
      {
        c2 += std::abs(gv[a] + s[a]);
      }
      fc += c2;
      std::copy(nx, nx + N, x);
    }
    fo += pr.terminalCost(t0 + T * dt, x);
    return fo + merit_scale * fc;
  }

  Model pr;
  Config cfg;
  int T = 0;
  double t0 = 0, x0[N] = {};
  double *X = nullptr, *U = nullptr, *LAM = nullptr, *S = nullptr, *NU = nullptr;
  double eps = 1e-4;
  std::vector<Coef> co;
  std::vector<double> d_x, d_u, d_lam, d_s, d_nu;
  double merit_func = 0, merit_deriv = 0, merit_scale = 0;
};

template<class F>
int dispatch(int model, F && f)
{
  switch(model)
  {
    case 0: return f(Fixed<oracle_fmpc::Oscillator>{});
    case 1: return f(Fixed<oracle_fmpc::CartPole>{});
    case 2: return f(Fixed<oracle_fmpc::PointMass>{});
    case 3: return f(Vertical{});
    default: return -100;
  }
}

/** Problem object of instance b from the library's memory image (one shared object, or B of them). */
template<class Model>
Model load(const Model & proto, const double * params, int per_instance, int b)
{
  Model p = proto;
  static_assert(sizeof(Model) % sizeof(double) == 0, "a problem image is a struct of doubles");
  if(params)
  {
    std::memcpy(static_cast<void *>(&p), params + (per_instance ? b : 0) * (sizeof(Model) / sizeof(double)), sizeof(Model));
  }
  return p;
}

Config toConfig(const int * ci, double kkt)
{
  return Config{ci[0], ci[1], ci[2], ci[3], ci[4], ci[5], ci[6], ci[7], kkt};
}

template<class Fn>
void parallelFor(int B, int n_threads, Fn && fn)
{
  n_threads = std::max(1, std::min(n_threads, B));
  std::vector<std::thread> th;
  for(int w = 0; w < n_threads; w++)
  {
    th.emplace_back([&, w]() {
      for(int b = w; b < B; b += n_threads)
      {
        fn(b);
      }
    });
  }
  for(auto & t : th)
  {
    t.join();
  }
}

double * off(double * p, size_t n)
{
  return p ? p + n : nullptr;
}
} // namespace

extern "C"
{
  /** (state dim, input capacity, inequality capacity, doubles of the problem image). */
  int chk_model_info(int model, int * n, int * m, int * g, int * p)
  {
    return dispatch(model, [&](auto mdl) {
      using Md = decltype(mdl);
      *n = Md::N;
      *m = Md::MC;
      *g = Md::GC;
      *p = static_cast<int>(sizeof(mdl) / sizeof(double));
      return 0;
    });
  }

  int chk_default_params(int model, double * out)
  {
    return dispatch(model, [&](auto mdl) {
      std::memcpy(out, static_cast<const void *>(&mdl), sizeof(mdl));
      return 0;
    });
  }

  int chk_dims_at(int model, const double * params, double t, int * m, int * g)
  {
    return dispatch(model, [&](auto mdl) {
      load(mdl, params, 0, 0).dims(t, *m, *g);
      return 0;
    });
  }

  /** Batched solves.  cfg: horizon_steps, max_iter, check_nan, init_complementary_variable, update_barrier_eps,
      break_if_llt_fails, enable_line_search, merit_const_scale_from_lagrange_multipliers.  Variable in / out in the padded
      boundary layouts [B][...]; barrier_eps [B] in / out; every output may be NULL. */
  int chk_solve(int model, const double * params, int per_instance, const int * cfg, double kkt_thre, int B, const double * t0,
                const double * x0, double * X, double * U, double * LAM, double * S, double * NU, double * barrier_eps, int * status,
                int * iters, double * trace, double * dX, double * dU, double * dLAM, double * dS, double * dNU, double * gk, double * gK,
                double * gs, double * gP, double * merit, int n_threads)
  {
    const Config c = toConfig(cfg, kkt_thre);
    return dispatch(model, [&](auto mdl) {
      using Md = decltype(mdl);
      constexpr int N = Md::N, MC = Md::MC, GC = Md::GC;
      const size_t T = c.T;
      parallelFor(B, n_threads, [&](int b) {
        Solver<Md> sol(load(mdl, params, per_instance, b), c);
        Out o{status + b,
              iters + b,
              off(trace, b * static_cast<size_t>(c.max_iter) * 6),
              off(dX, b * (T + 1) * N),
              off(dU, b * T * MC),
              off(dLAM, b * (T + 1) * N),
              off(dS, b * T * GC),
              off(dNU, b * T * GC),
              off(gk, b * T * MC),
              off(gK, b * T * N * MC),
              off(gs, b * (T + 1) * N),
              off(gP, b * (T + 1) * N * N),
              off(merit, b * 3)};
        sol.solve(t0[b], x0 + b * N, X + b * (T + 1) * N, U + b * T * MC, LAM + b * (T + 1) * N, S + b * T * GC, NU + b * T * GC,
                  barrier_eps[b], o);
      });
      return 0;
    });
  }

  /** Closed loop of one instance per b (the library's mpc_run): n_ticks times { solve(t, x, resident variable); log;
      `substeps` plant steps x <- stateEq(t, x, u_list[0], sim_dt) with u_list[0] of size m(t) }.  Logs [B][n_ticks][...]. */
  int chk_closed_loop(int model, const double * params, int per_instance, const int * cfg, double kkt_thre, int B, const double * t0,
                      const double * x0, double * X, double * U, double * LAM, double * S, double * NU, double * barrier_eps, int n_ticks,
                      double sim_dt, int substeps, double * x_log, double * u0_log, int * status_log, int * iter_log, int n_threads)
  {
    const Config c = toConfig(cfg, kkt_thre);
    return dispatch(model, [&](auto mdl) {
      using Md = decltype(mdl);
      constexpr int N = Md::N, MC = Md::MC, GC = Md::GC;
      const size_t T = c.T;
      parallelFor(B, n_threads, [&](int b) {
        const Md p = load(mdl, params, per_instance, b);
        Solver<Md> sol(p, c);
        double t = t0[b], x[kMaxN];
        std::copy(x0 + b * N, x0 + (b + 1) * N, x);
        double *Xb = X + b * (T + 1) * N, *Ub = U + b * T * MC, *Lb = LAM + b * (T + 1) * N, *Sb = S + b * T * GC, *Nb = NU + b * T * GC;
        for(int k = 0; k < n_ticks; k++)
        {
          int st = 0, it = 0;
          Out o{&st, &it, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
          const size_t r = static_cast<size_t>(b) * n_ticks + k;
          std::copy(x, x + N, x_log + r * N);
          sol.solve(t, x, Xb, Ub, Lb, Sb, Nb, barrier_eps[b], o);
          int m0 = 0, g0 = 0;
          p.dims(t, m0, g0);
          for(int a = 0; a < MC; a++)
          {
            u0_log[r * MC + a] = a < m0 ? Ub[a] : 0.0;
          }
          status_log[r] = st;
          iter_log[r] = it;
          for(int s = 0; s < substeps; s++)
          {
            double nx[kMaxN];
            p.stateEqDt(t, x, Ub, m0, sim_dt, nx);
            std::copy(nx, nx + N, x);
            t += sim_dt;
          }
        }
      });
      return 0;
    });
  }
}
