// See cgmres_checker.hpp.
#include "cgmres_checker.hpp"

#include <cmath>
#include <thread>
#include <vector>

namespace
{
using Vec = std::vector<double>;

struct Model
{
  int kind;
  const double * p;
  int nx, nuc;

  // ---- cart-pole: p = m1, m2, l, f_max, q[4], r1, r2, sf[4], ref[4], g
  void cartAccel(const double * x, double f, double & pdd, double & thdd) const
  {
    const double m1 = p[0], m2 = p[1], l = p[2], g = p[18];
    const double s = std::sin(x[1]), c = std::cos(x[1]);
    const double D = m1 + m2 * (s * s);
    const double w2 = x[3] * x[3];
    pdd = (f - m2 * l * w2 * s + m2 * g * s * c) / D;
    thdd = (f * c - m2 * l * w2 * s * c + g * (m1 + m2) * s) / (l * D);
  }

  void stateEquation(double, const double * x, const double * u, double * dx) const
  {
    if(kind == 0)
    {
      dx[0] = x[1];
      dx[1] = p[0] * x[0] + p[1] * x[1] * u[0];
      return;
    }
    dx[0] = x[2];
    dx[1] = x[3];
    cartAccel(x, u[0], dx[2], dx[3]);
  }

  void costateEquation(double, const double * lmd, const double * xu, double * dl) const
  {
    const double * x = xu;
    if(kind == 0)
    {
      const double a = p[0], b = p[1], q1 = p[3], q2 = p[4];
      dl[0] = -(q1 * x[0] + a * lmd[1]);
      dl[1] = -(q2 * x[1] + lmd[0] + b * lmd[1] * xu[2]);
      return;
    }
    const double m1 = p[0], m2 = p[1], l = p[2], g = p[18];
    const double * q = p + 4;
    const double * ref = p + 14;
    const double f = xu[4];
    const double s = std::sin(x[1]), c = std::cos(x[1]);
    const double D = m1 + m2 * (s * s);
    const double dD = 2 * m2 * s * c;
    const double w = x[3], w2 = w * w;
    const double c2s2 = c * c - s * s;
    const double Na = f - m2 * l * w2 * s + m2 * g * s * c;
    const double dNa = -m2 * l * w2 * c + m2 * g * c2s2;
    const double Nb = f * c - m2 * l * w2 * s * c + g * (m1 + m2) * s;
    const double dNb = -f * s - m2 * l * w2 * c2s2 + g * (m1 + m2) * c;
    const double a_th = (dNa * D - Na * dD) / (D * D);
    const double b_th = (dNb * D - Nb * dD) / (l * D * D);
    const double a_w = -2 * m2 * l * w * s / D;
    const double b_w = -2 * m2 * w * s * c / D;
    dl[0] = -(q[0] * (x[0] - ref[0]));
    dl[1] = -(q[1] * (x[1] - ref[1]) + lmd[2] * a_th + lmd[3] * b_th);
    dl[2] = -(q[2] * (x[2] - ref[2]) + lmd[0]);
    dl[3] = -(q[3] * (x[3] - ref[3]) + lmd[1] + lmd[2] * a_w + lmd[3] * b_w);
  }

  void calcDphiDx(double, const double * x, double * out) const
  {
    if(kind == 0)
    {
      out[0] = p[7] * x[0];
      out[1] = p[8] * x[1];
      return;
    }
    for(int i = 0; i < 4; i++)
    {
      out[i] = p[10 + i] * (x[i] - p[14 + i]);
    }
  }

  void calcDhDu(double, const double * x, const double * u, const double * lmd, double * out) const
  {
    if(kind == 0)
    {
      const double b = p[1], um = p[2], r1 = p[5], r2 = p[6];
      const double mu = u[2];
      const double d0 = u[0] - um / 2.0;
      out[0] = r1 * u[0] + b * lmd[1] * x[1] + mu * (2 * u[0] - um);
      out[1] = -r2 + 2 * mu * u[1];
      out[2] = d0 * d0 + u[1] * u[1] - um * um / 4.0;
      return;
    }
    const double m1 = p[0], m2 = p[1], l = p[2], fmax = p[3], r1 = p[8], r2 = p[9];
    const double s = std::sin(x[1]), c = std::cos(x[1]);
    const double D = m1 + m2 * (s * s);
    out[0] = r1 * u[0] + lmd[2] / D + lmd[3] * c / (l * D);
    if(kind == 2)
    {
      out[0] += 2 * u[2] * u[0];
      out[1] = -r2 + 2 * u[2] * u[1];
      out[2] = u[0] * u[0] + u[1] * u[1] - fmax * fmax;
    }
  }
};

int dims(int model, int & nx, int & nuc)
{
  switch(model)
  {
    case 0: nx = 2, nuc = 3; return 0;
    case 1: nx = 4, nuc = 1; return 0;
    case 2: nx = 4, nuc = 3; return 0;
  }
  return -1;
}

double dotv(const Vec & a, const Vec & b)
{
  double s = 0;
  for(size_t i = 0; i < a.size(); i++)
  {
    s += a[i] * b[i];
  }
  return s;
}

Vec normalized(const Vec & v)
{
  const double z = dotv(v, v);
  if(!(z > 0))
  {
    return v;
  }
  const double nrm = std::sqrt(z);
  Vec out(v.size());
  for(size_t i = 0; i < v.size(); i++)
  {
    out[i] = v[i] / nrm;
  }
  return out;
}

/** GMRES, Kelley Alg. 3.5.1 with Givens rotations; amul(v) -> A v. */
template<class F>
void gmres(const F & amul, const Vec & b, Vec & x, int k_max, double eps, bool apply_reorth, int & iters, int & fired)
{
  const int n = static_cast<int>(x.size());
  k_max = std::min(k_max, n);
  const Vec Ax = amul(x);
  Vec r(n);
  for(int i = 0; i < n; i++)
  {
    r[i] = b[i] - Ax[i];
  }
  std::vector<Vec> V;
  double rho = std::sqrt(dotv(r, r));
  V.push_back(normalized(r));
  Vec g(k_max + 1, 0.0), cs, sn;
  g[0] = rho;
  const double b_norm = std::sqrt(dotv(b, b));
  std::vector<Vec> H(k_max + 1, Vec(k_max, 0.0)); // H[row][col]
  int k = 0;
  fired = 0;
  while(rho > eps * b_norm && k < k_max)
  {
    k++;
    const Vec Avk = amul(V.back());
    Vec nb = Avk;
    for(int j = 0; j < k; j++)
    {
      H[j][k - 1] = dotv(nb, V[j]);
      for(int e = 0; e < n; e++)
      {
        nb[e] = nb[e] - H[j][k - 1] * V[j][e];
      }
    }
    const double nbn = std::sqrt(dotv(nb, nb));
    H[k][k - 1] = nbn;
    if(apply_reorth)
    {
      const double an = std::sqrt(dotv(Avk, Avk));
      if(an + 1e-3 * nbn == an)
      {
        fired = 1;
        for(int j = 0; j < k; j++)
        {
          const double h = dotv(nb, V[j]);
          H[j][k - 1] = H[j][k - 1] + h;
          for(int e = 0; e < n; e++)
          {
            nb[e] = nb[e] - h * V[j][e];
          }
        }
      }
    }
    V.push_back(normalized(nb));
    for(int i = 0; i < k - 1; i++)
    {
      const double h0 = H[i][k - 1], h1 = H[i + 1][k - 1];
      H[i][k - 1] = cs[i] * h0 - sn[i] * h1;
      H[i + 1][k - 1] = sn[i] * h0 + cs[i] * h1;
    }
    const double a = H[k - 1][k - 1], c = H[k][k - 1];
    const double nu = std::sqrt(a * a + c * c);
    const double ck = a / nu, sk = -c / nu;
    cs.push_back(ck);
    sn.push_back(sk);
    H[k - 1][k - 1] = ck * a - sk * c;
    H[k][k - 1] = 0;
    const double g0 = g[k - 1], g1 = g[k];
    g[k - 1] = ck * g0 - sk * g1;
    g[k] = sk * g0 + ck * g1;
    rho = std::fabs(g[k]);
  }
  // back substitution by columns
  Vec y(g.begin(), g.begin() + k);
  for(int i = k - 1; i >= 0; i--)
  {
    y[i] = y[i] / H[i][i];
    for(int j = 0; j < i; j++)
    {
      y[j] = y[j] - y[i] * H[j][i];
    }
  }
  for(int i = 0; i < k; i++)
  {
    for(int e = 0; e < n; e++)
    {
      x[e] = x[e] + y[i] * V[i][e];
    }
  }
  iters = k;
}

struct Cfg
{
  double sim_duration, steady, ratio, dt, zeta, delta;
  int N, k_max, dump_step, ode, sim_ode;
};

/** One C/GMRES solver instance. */
struct Solver
{
  Model m;
  Cfg c;
  Vec x, u;
  std::vector<Vec> U; // [N][nuc]
  Vec du; // [N * nuc]
  double err = 0;
  int status = 0, iters = 0, reorth = 0;

  template<class F>
  void ode(int solver, const F & f, double t, const Vec & y, const Vec & aux, double h, Vec & out) const
  {
    const size_t D = y.size();
    Vec k1(D), k2(D), k3(D), k4(D), yt(D);
    f(t, y.data(), aux.data(), k1.data());
    out.resize(D);
    if(solver == 0)
    {
      for(size_t a = 0; a < D; a++)
      {
        out[a] = y[a] + h * k1[a];
      }
      return;
    }
    const double hh = h / 2;
    for(size_t a = 0; a < D; a++)
    {
      yt[a] = y[a] + hh * k1[a];
    }
    f(t + hh, yt.data(), aux.data(), k2.data());
    for(size_t a = 0; a < D; a++)
    {
      yt[a] = y[a] + hh * k2[a];
    }
    f(t + hh, yt.data(), aux.data(), k3.data());
    for(size_t a = 0; a < D; a++)
    {
      yt[a] = y[a] + h * k3[a];
    }
    f(t + h, yt.data(), aux.data(), k4.data());
    const double h6 = h / 6;
    for(size_t a = 0; a < D; a++)
    {
      out[a] = y[a] + h6 * (((k1[a] + 2 * k2[a]) + 2 * k3[a]) + k4[a]);
    }
  }

  void stateStep(int solver, double t, const Vec & xx, const Vec & uu, double h, Vec & out) const
  {
    ode(solver, [this](double tt, const double * y, const double * a, double * d) { m.stateEquation(tt, y, a, d); }, t, xx, uu, h, out);
  }

  /** DhDu over the horizon [N * nuc] for input list UL. */
  Vec dhduList(double t, const Vec & x0, const std::vector<Vec> & UL) const
  {
    const int N = c.N;
    const double T = c.steady * (1.0 - std::exp(-c.ratio * t));
    const double h = T / N;
    std::vector<Vec> xs(N + 1);
    xs[0] = x0;
    double tau = t;
    for(int i = 0; i < N; i++)
    {
      stateStep(c.ode, tau, xs[i], UL[i], h, xs[i + 1]);
      tau += h;
    }
    Vec lmd(m.nx), prev;
    m.calcDphiDx(tau, xs[N].data(), lmd.data());
    Vec out(static_cast<size_t>(N) * m.nuc);
    for(int i = N - 1; i >= 0; i--)
    {
      Vec xu(xs[i]);
      xu.insert(xu.end(), UL[i].begin(), UL[i].end());
      ode(c.ode, [this](double tt, const double * y, const double * a, double * d) { m.costateEquation(tt, y, a, d); }, tau, lmd, xu, -h,
          prev);
      tau -= h;
      m.calcDhDu(tau, xs[i].data(), UL[i].data(), lmd.data(), out.data() + static_cast<size_t>(i) * m.nuc);
      lmd = prev;
    }
    return out;
  }

  void setup()
  {
    const double delta = c.delta;
    Vec lmd(m.nx), dh(m.nuc), d0(m.nuc);
    m.calcDphiDx(0, x.data(), lmd.data());
    Vec dlt(m.nuc, 0.0);
    double nrm = 0;
    for(int it = 0; it < 100; it++)
    {
      m.calcDhDu(0, x.data(), u.data(), lmd.data(), dh.data());
      nrm = std::sqrt(dotv(dh, dh));
      if(nrm <= 1e-6)
      {
        break;
      }
      Vec b(m.nuc);
      for(int j = 0; j < m.nuc; j++)
      {
        b[j] = -dh[j];
      }
      auto amul = [&](const Vec & v) {
        Vec up(m.nuc), d(m.nuc), out(m.nuc);
        for(int j = 0; j < m.nuc; j++)
        {
          up[j] = u[j] + delta * v[j];
        }
        m.calcDhDu(0, x.data(), up.data(), lmd.data(), d.data());
        for(int j = 0; j < m.nuc; j++)
        {
          out[j] = (d[j] - dh[j]) / delta;
        }
        return out;
      };
      int k, f;
      gmres(amul, b, dlt, m.nuc, 1e-10, true, k, f);
      for(int j = 0; j < m.nuc; j++)
      {
        u[j] = u[j] + dlt[j];
      }
    }
    bool finite = std::isfinite(nrm);
    for(double v : u)
    {
      finite = finite && std::isfinite(v);
    }
    status = !finite ? 3 : (nrm <= 1e-6 ? 1 : 2);
    err = nrm;
    U.assign(c.N, u);
    du.assign(static_cast<size_t>(c.N) * m.nuc, 0.0);
  }

  void controlInput(double t, const Vec & xx, const Vec & nx)
  {
    const double delta = c.delta;
    const int n = c.N * m.nuc;
    const Vec D = dhduList(t, xx, U);
    const double twd = t + delta;
    const double a0 = 1 - delta / c.dt, a1 = delta / c.dt;
    Vec xwd(m.nx);
    for(int a = 0; a < m.nx; a++)
    {
      xwd[a] = a0 * xx[a] + a1 * nx[a];
    }
    const Vec Dw = dhduList(twd, xwd, U);
    const double zd = 1 - c.zeta * delta;
    Vec b(n);
    for(int e = 0; e < n; e++)
    {
      b[e] = (zd * D[e] - Dw[e]) / delta;
    }
    err = std::sqrt(dotv(D, D));
    auto amul = [&](const Vec & v) {
      std::vector<Vec> UA(U);
      for(int i = 0; i < c.N; i++)
      {
        for(int j = 0; j < m.nuc; j++)
        {
          UA[i][j] = U[i][j] + delta * v[i * m.nuc + j];
        }
      }
      Vec out = dhduList(twd, xwd, UA);
      for(int e = 0; e < n; e++)
      {
        out[e] = (out[e] - Dw[e]) / delta;
      }
      return out;
    };
    gmres(amul, b, du, c.k_max, 1e-10, true, iters, reorth);
    for(int i = 0; i < c.N; i++)
    {
      for(int j = 0; j < m.nuc; j++)
      {
        U[i][j] = U[i][j] + c.dt * du[i * m.nuc + j];
      }
    }
    u = U[0];
  }
};
} // namespace

extern "C"
{
  int chk_model_dims(int model, int * nx, int * nuc)
  {
    return dims(model, *nx, *nuc);
  }

  int chk_model_eval(int model, const double * params, int P, const double * t, const double * x, const double * u, const double * lmd,
                     double * dotx, double * dotlmd, double * dphidx, double * dhdu)
  {
    int nx, nuc;
    if(dims(model, nx, nuc) != 0)
    {
      return -1;
    }
    const Model m{model, params, nx, nuc};
    for(int p = 0; p < P; p++)
    {
      Vec xu(x + p * nx, x + p * nx + nx);
      xu.insert(xu.end(), u + p * nuc, u + p * nuc + nuc);
      m.stateEquation(t[p], xu.data(), xu.data() + nx, dotx + p * nx);
      m.costateEquation(t[p], lmd + p * nx, xu.data(), dotlmd + p * nx);
      m.calcDphiDx(t[p], xu.data(), dphidx + p * nx);
      m.calcDhDu(t[p], xu.data(), xu.data() + nx, lmd + p * nx, dhdu + p * nuc);
    }
    return 0;
  }

  void chk_dense_gmres(int n, const double * A, const double * b, double * x, int k_max, int apply_reorth, double eps, int * iters,
                       int * reorth_fired)
  {
    auto amul = [&](const Vec & v) {
      Vec out(n);
      for(int i = 0; i < n; i++)
      {
        double acc = 0;
        for(int j = 0; j < n; j++)
        {
          acc += A[static_cast<size_t>(i) * n + j] * v[j];
        }
        out[i] = acc;
      }
      return out;
    };
    Vec bv(b, b + n), xv(x, x + n);
    gmres(amul, bv, xv, k_max, eps, apply_reorth != 0, *iters, *reorth_fired);
    std::copy(xv.begin(), xv.end(), x);
  }

  int chk_solve(int model, const double * params, int per_instance, const double * cfg, int B, const double * x0, const double * u0,
                int do_run, int n_threads, double * x_out, double * u_out, double * U_out, int * status, double * err_out,
                double * log_x, double * log_u, double * log_err, int * log_iters, int * log_reorth, int log_rows)
  {
    int nx, nuc;
    if(dims(model, nx, nuc) != 0)
    {
      return -1;
    }
    const int n_params = model == 0 ? 9 : 19;
    Cfg c;
    c.sim_duration = cfg[0];
    c.steady = cfg[1];
    c.N = static_cast<int>(cfg[2]);
    c.ratio = cfg[3];
    c.dt = cfg[4];
    c.zeta = cfg[5];
    c.k_max = static_cast<int>(cfg[6]);
    c.delta = cfg[7];
    c.dump_step = static_cast<int>(cfg[8]);
    c.ode = static_cast<int>(cfg[9]);
    c.sim_ode = static_cast<int>(cfg[10]) < 0 ? c.ode : static_cast<int>(cfg[10]);
    std::vector<double> ts;
    if(do_run)
    {
      for(double t = 0; t <= c.sim_duration; t += c.dt)
      {
        ts.push_back(t);
      }
    }
    auto work = [&](int b) {
      Solver s{Model{model, params + (per_instance ? static_cast<size_t>(b) * n_params : 0), nx, nuc}, c, Vec(x0 + b * nx, x0 + b * nx + nx),
               Vec(u0 + b * nuc, u0 + b * nuc + nuc)};
      s.setup();
      Vec nxt;
      for(size_t i = 0; i < ts.size() && s.status != 3; i++)
      {
        const double t = ts[i];
        s.stateStep(c.sim_ode, t, s.x, s.u, c.dt, nxt);
        s.controlInput(t, s.x, nxt);
        s.x = nxt;
        bool finite = true;
        for(double v : s.x)
        {
          finite = finite && std::isfinite(v);
        }
        for(double v : s.u)
        {
          finite = finite && std::isfinite(v);
        }
        if(c.dump_step > 0 && i % c.dump_step == 0 && static_cast<int>(i / c.dump_step) < log_rows && log_x)
        {
          const size_t r = static_cast<size_t>(b) * log_rows + i / c.dump_step;
          std::copy(s.x.begin(), s.x.end(), log_x + r * nx);
          std::copy(s.u.begin(), s.u.end(), log_u + r * nuc);
          log_err[r] = s.err;
          log_iters[r] = s.iters;
          log_reorth[r] = s.reorth;
        }
        if(!finite)
        {
          s.status = 3;
        }
      }
      std::copy(s.x.begin(), s.x.end(), x_out + b * nx);
      std::copy(s.u.begin(), s.u.end(), u_out + b * nuc);
      for(int i = 0; i < c.N; i++)
      {
        std::copy(s.U[i].begin(), s.U[i].end(), U_out + (static_cast<size_t>(b) * c.N + i) * nuc);
      }
      status[b] = s.status;
      err_out[b] = s.err;
    };
    n_threads = std::max(1, n_threads);
    std::vector<std::thread> pool;
    for(int w = 0; w < n_threads; w++)
    {
      pool.emplace_back([&, w]() {
        for(int b = w; b < B; b += n_threads)
        {
          work(b);
        }
      });
    }
    for(auto & th : pool)
    {
      th.join();
    }
    return static_cast<int>(ts.size());
  }
}
