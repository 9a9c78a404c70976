// TEST INFRASTRUCTURE - NOT PRODUCT CODE.
//
// CPU checker of the batched FMPC iteration on caller-supplied linearisations (include/nmpc_hip_fmpc_step.h): one
// FmpcSolver::procOnce of the reference (nmpc_fmpc/include/nmpc_fmpc/FmpcSolver.hpp:365-493 and what it calls, without the line
// search) restated on plain row-major arrays [B][T][rows][cols] with the capacities (n, m, g) as block sizes.  Every sum runs in
// ascending index order; nothing is contracted into FMAs (-ffp-contract=off).  It has its own Eigen::LDLT restatement and full-pivot
// LU for matrices up to 16 x 16.  Built by the tests into a temporary directory (tests/fmpc_step_checker.py).
#include <cfloat>
#include <cmath>
#include <cstddef>
#include <limits>
#include <thread>
#include <utility>
#include <vector>

namespace
{
constexpr int kMax = 16;

/** Eigen::LDLT<Matrix, Lower> of an m x m matrix (a[i][j]), in place, with symmetric diagonal pivoting. */
struct Ldlt
{
  int m = 0;
  double a[kMax][kMax];
  int tr[kMax];

  /** false where Eigen's info() is NumericalIssue. */
  bool compute(const double * G, int ld, int m_)
  {
    m = m_;
    for(int i = 0; i < m; i++)
    {
      for(int j = 0; j < m; j++)
      {
        a[i][j] = G[i * ld + j];
      }
    }
    if(m <= 1)
    {
      tr[0] = 0;
      return true;
    }
    bool found_zero_pivot = false, ret = true;
    for(int k = 0; k < m; k++)
    {
      int pv = k;
      double big = std::abs(a[k][k]);
      for(int i = k + 1; i < m; i++)
      {
        if(std::abs(a[i][i]) > big)
        {
          big = std::abs(a[i][i]);
          pv = i;
        }
      }
      tr[k] = pv;
      if(pv != k)
      {
        for(int j = 0; j < k; j++)
        {
          std::swap(a[k][j], a[pv][j]);
        }
        for(int i = pv + 1; i < m; i++)
        {
          std::swap(a[i][k], a[i][pv]);
        }
        std::swap(a[k][k], a[pv][pv]);
        for(int i = k + 1; i < pv; i++)
        {
          std::swap(a[i][k], a[pv][i]);
        }
      }
      if(k > 0)
      {
        double temp[kMax];
        for(int j = 0; j < k; j++)
        {
          temp[j] = a[j][j] * a[k][j];
        }
        for(int i = k; i < m; i++)
        {
          double s = 0;
          for(int j = 0; j < k; j++)
          {
            s += a[i][j] * temp[j];
          }
          a[i][k] -= s;
        }
      }
      const double akk = a[k][k];
      const bool pivot_is_valid = std::abs(akk) > 0.0;
      if(k == 0 && !pivot_is_valid)
      {
        for(int j = 0; j < m; j++)
        {
          tr[j] = j;
          for(int i = j + 1; i < m; i++)
          {
            ret = ret && (a[i][j] == 0.0);
          }
        }
        return ret;
      }
      if(pivot_is_valid)
      {
        for(int i = k + 1; i < m; i++)
        {
          a[i][k] /= akk;
        }
      }
      else
      {
        for(int i = k + 1; i < m; i++)
        {
          ret = ret && (a[i][k] == 0.0);
        }
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
    return ret;
  }

  /** x <- G^-1 x (D's pseudo-inverse). */
  void solve(double * x) const
  {
    for(int k = 0; k < m; k++)
    {
      std::swap(x[k], x[tr[k]]);
    }
    for(int i = 0; i < m; i++)
    {
      for(int j = 0; j < i; j++)
      {
        x[i] -= a[i][j] * x[j];
      }
    }
    for(int i = 0; i < m; i++)
    {
      x[i] = (std::abs(a[i][i]) > DBL_MIN) ? x[i] / a[i][i] : 0.0;
    }
    for(int i = m - 1; i >= 0; i--)
    {
      for(int j = i + 1; j < m; j++)
      {
        x[i] -= a[j][i] * x[j];
      }
    }
    for(int k = m - 1; k >= 0; k--)
    {
      std::swap(x[k], x[tr[k]]);
    }
  }
};

/** Full-pivot Gaussian elimination (the role of Eigen::FullPivLU at FmpcSolver.hpp:614-616): rhs[q][i], c right-hand sides, in
    place; rank-deficient directions get 0. */
void luSolve(const double * G, int ld, int m, double (*rhs)[kMax], int c)
{
  double a[kMax][kMax];
  int colperm[kMax];
  for(int i = 0; i < m; i++)
  {
    colperm[i] = i;
    for(int j = 0; j < m; j++)
    {
      a[i][j] = G[i * ld + j];
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
        if(std::abs(a[i][j]) > big)
        {
          big = std::abs(a[i][j]);
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
      std::swap(a[k][j], a[pr][j]);
    }
    for(int q = 0; q < c; q++)
    {
      std::swap(rhs[q][k], rhs[q][pr]);
    }
    for(int i = 0; i < m; i++)
    {
      std::swap(a[i][k], a[i][pc]);
    }
    std::swap(colperm[k], colperm[pc]);
    for(int i = k + 1; i < m; i++)
    {
      const double f = a[i][k] / a[k][k];
      for(int j = k + 1; j < m; j++)
      {
        a[i][j] -= f * a[k][j];
      }
      for(int q = 0; q < c; q++)
      {
        rhs[q][i] -= f * rhs[q][k];
      }
    }
  }
  for(int q = 0; q < c; q++)
  {
    double y[kMax];
    for(int i = m - 1; i >= 0; i--)
    {
      if(i >= rank)
      {
        y[i] = 0;
        continue;
      }
      double s = rhs[q][i];
      for(int j = i + 1; j < rank; j++)
      {
        s -= a[i][j] * y[j];
      }
      y[i] = s / a[i][i];
    }
    for(int i = 0; i < m; i++)
    {
      rhs[q][colperm[i]] = y[i];
    }
  }
}

bool notFinite(double v)
{
  return std::isnan(v) || std::isinf(v);
}

struct Shape
{
  int n, m, g, T;
};

struct Args
{
  Shape sh;
  const int *mdims, *gdims;
  const double *A, *Bm, *C, *D, *Lx, *Lu, *Lxx, *Luu, *Lxu, *f, *gv, *LxT, *LxxT, *cur_x;
  double *x, *u, *lam, *s, *nu, *eps;
  double dt, kkt_error_thre;
  int check_nan, init_complementary_variable, update_barrier_eps, break_if_llt_fails, apply_update;
  int * status;
  double *kkt, *alpha_s, *alpha_nu, *k, *K, *gs, *P, *dx, *du, *dlam, *ds, *dnu;
};

/** One procOnce of instance b. */
int stepOne(const Args & a, size_t b)
{
  const int n = a.sh.n, mc = a.sh.m, gc = a.sh.g, T = a.sh.T;
  auto mAt = [&](int i) { return a.mdims ? a.mdims[i] : mc; };
  auto gAt = [&](int i) { return a.gdims ? a.gdims[i] : gc; };
  const double dt = a.dt;
  double * x = a.x + b * (T + 1) * n;
  double * lam = a.lam + b * (T + 1) * n;
  double * u = a.u + b * T * mc;
  double * s = a.s + b * T * gc;
  double * nu = a.nu + b * T * gc;
  const double * A = a.A + b * T * n * n;
  const double * Bm = a.Bm + b * T * n * mc;
  const double * C = a.C + b * T * gc * n;
  const double * D = a.D + b * T * gc * mc;
  const double * gv = a.gv + b * T * gc;
  double * ok = a.k + b * T * mc;
  double * oK = a.K + b * T * mc * n;
  double * ogs = a.gs + b * (T + 1) * n;
  double * oP = a.P + b * (T + 1) * n * n;
  double * dx = a.dx + b * (T + 1) * n;
  double * dlam = a.dlam + b * (T + 1) * n;
  double * du = a.du + b * T * mc;
  double * ds = a.ds + b * T * gc;
  double * dnu = a.dnu + b * T * gc;
  double eps = a.eps[b];
  a.alpha_s[b] = 1.0;
  a.alpha_nu[b] = 1.0;

  // initial complementarity variables    :172-188
  if(a.init_complementary_variable)
  {
    eps = 1e-4;
    for(int i = 0; i < T; i++)
    {
      for(int j = 0; j < gAt(i); j++)
      {
        const double v = -1 * gv[i * gc + j];
        s[i * gc + j] = (1.0 + 1e-2) * ((v < 1e-2) ? 1e-2 : v);
        const double c = eps * (1.0 / s[i * gc + j]);
        nu[i * gc + j] = (1.0 + 1e-2) * ((c < 1e-2) ? 1e-2 : c);
      }
    }
  }
  // barrier parameter    :378-399
  if(a.update_barrier_eps)
  {
    double s_nu_ave = 0;
    int total = 0;
    for(int i = 0; i < T; i++)
    {
      for(int j = 0; j < gAt(i); j++)
      {
        s_nu_ave += s[i * gc + j] * nu[i * gc + j];
      }
      total += gAt(i);
    }
    s_nu_ave /= total;
    const double v = 0.5 * s_nu_ave;
    eps = (v < 1e-8) ? 1e-8 : ((1e6 < v) ? 1e6 : v);
  }
  a.eps[b] = eps;

  // residuals    :422-434
  std::vector<double> xbar(T * n), gbar(T * gc, 0.0), lxbar((T + 1) * n), lubar(T * mc, 0.0);
  for(int i = 0; i < T; i++)
  {
    const int m = mAt(i), gi = gAt(i);
    const double * Ai = A + i * n * n;
    const double * Bi = Bm + i * n * mc;
    const double * Ci = C + i * gc * n;
    const double * Di = D + i * gc * mc;
    for(int r = 0; r < n; r++)
    {
      xbar[i * n + r] = a.f[(b * T + i) * n + r] - x[(i + 1) * n + r];
      double s1 = 0, s2 = 0;
      for(int k = 0; k < n; k++)
      {
        s1 += Ai[k * n + r] * lam[(i + 1) * n + k];
      }
      for(int j = 0; j < gi; j++)
      {
        s2 += Ci[j * n + r] * nu[i * gc + j];
      }
      lxbar[i * n + r] = ((-1 * lam[i * n + r] + dt * a.Lx[(b * T + i) * n + r]) + s1) + s2;
    }
    for(int r = 0; r < m; r++)
    {
      double s1 = 0, s2 = 0;
      for(int k = 0; k < n; k++)
      {
        s1 += Bi[k * mc + r] * lam[(i + 1) * n + k];
      }
      for(int j = 0; j < gi; j++)
      {
        s2 += Di[j * mc + r] * nu[i * gc + j];
      }
      lubar[i * mc + r] = (dt * a.Lu[(b * T + i) * mc + r] + s1) + s2;
    }
    for(int j = 0; j < gi; j++)
    {
      gbar[i * gc + j] = gv[i * gc + j] + s[i * gc + j];
    }
  }
  for(int r = 0; r < n; r++)
  {
    lxbar[T * n + r] = a.LxT[b * n + r] - lam[T * n + r];
  }

  // KKT error    :496-521
  double kkt = 0;
  for(int r = 0; r < n; r++)
  {
    const double e = a.cur_x[b * n + r] - x[r];
    kkt += e * e;
  }
  for(int i = 0; i < T; i++)
  {
    for(int r = 0; r < n; r++)
    {
      kkt += xbar[i * n + r] * xbar[i * n + r];
    }
    for(int j = 0; j < gAt(i); j++)
    {
      kkt += gbar[i * gc + j] * gbar[i * gc + j];
    }
    for(int r = 0; r < n; r++)
    {
      kkt += lxbar[i * n + r] * lxbar[i * n + r];
    }
    for(int r = 0; r < mAt(i); r++)
    {
      kkt += lubar[i * mc + r] * lubar[i * mc + r];
    }
    for(int j = 0; j < gAt(i); j++)
    {
      const double c = s[i * gc + j] * nu[i * gc + j] - 0.0;
      const double cp = (c < 0) ? 0.0 : c;
      kkt += cp * cp;
    }
  }
  for(int r = 0; r < n; r++)
  {
    kkt += lxbar[T * n + r] * lxbar[T * n + r];
  }
  kkt = std::sqrt(kkt);
  a.kkt[b] = kkt;
  if(kkt <= a.kkt_error_thre)
  {
    return 1;
  }

  // backward pass    :524-665
  bool bad = false;
  std::vector<double> sv(n), P(n * n), F(n * n), Ht(kMax * n), G(kMax * kMax), PA(n * n), PB(n * kMax), v(n), Lxt(n), Lut(kMax), nus(gc + 1),
      tsub(gc + 1), Pn(n * n), GK(kMax * n);
  for(int r = 0; r < n; r++)
  {
    sv[r] = -1 * lxbar[T * n + r];
    ogs[T * n + r] = sv[r];
    bad = bad || notFinite(a.LxT[b * n + r]) || notFinite(lxbar[T * n + r]);
    for(int c = 0; c < n; c++)
    {
      P[r * n + c] = a.LxxT[b * n * n + r * n + c];
      oP[T * n * n + r * n + c] = P[r * n + c];
      bad = bad || notFinite(P[r * n + c]);
    }
  }
  for(int i = T - 1; i >= 0; i--)
  {
    const int m = mAt(i), gi = gAt(i);
    const double * Ai = A + i * n * n;
    const double * Bi = Bm + i * n * mc;
    const double * Ci = C + i * gc * n;
    const double * Di = D + i * gc * mc;
    const double * Lxx = a.Lxx + (b * T + i) * n * n;
    const double * Luu = a.Luu + (b * T + i) * mc * mc;
    const double * Lxu = a.Lxu + (b * T + i) * n * mc;
    // CHECK_NAN over the inputs of the step (Coefficient::containsNaN)
    for(int r = 0; r < n; r++)
    {
      bad = bad || notFinite(a.Lx[(b * T + i) * n + r]) || notFinite(xbar[i * n + r]) || notFinite(lxbar[i * n + r]);
      for(int c = 0; c < n; c++)
      {
        bad = bad || notFinite(Ai[r * n + c]) || notFinite(Lxx[r * n + c]);
      }
      for(int c = 0; c < m; c++)
      {
        bad = bad || notFinite(Bi[r * mc + c]) || notFinite(Lxu[r * mc + c]);
      }
    }
    for(int r = 0; r < m; r++)
    {
      bad = bad || notFinite(a.Lu[(b * T + i) * mc + r]) || notFinite(lubar[i * mc + r]);
      for(int c = 0; c < m; c++)
      {
        bad = bad || notFinite(Luu[r * mc + c]);
      }
    }
    for(int j = 0; j < gi; j++)
    {
      bad = bad || notFinite(gbar[i * gc + j]);
      for(int c = 0; c < n; c++)
      {
        bad = bad || notFinite(Ci[j * n + c]);
      }
      for(int c = 0; c < m; c++)
      {
        bad = bad || notFinite(Di[j * mc + c]);
      }
    }

    for(int j = 0; j < gi; j++)
    {
      const double sj = s[i * gc + j], nj = nu[i * gc + j];
      nus[j] = nj / sj;
      tsub[j] = (nus[j] * gbar[i * gc + j] - nj) + eps * (1.0 / sj);
    }
    // P A, P B, P x_bar - s
    for(int r = 0; r < n; r++)
    {
      for(int c = 0; c < n; c++)
      {
        double t = 0;
        for(int k = 0; k < n; k++)
        {
          t += P[r * n + k] * Ai[k * n + c];
        }
        PA[r * n + c] = t;
      }
      for(int c = 0; c < m; c++)
      {
        double t = 0;
        for(int k = 0; k < n; k++)
        {
          t += P[r * n + k] * Bi[k * mc + c];
        }
        PB[r * kMax + c] = t;
      }
      double t = 0;
      for(int k = 0; k < n; k++)
      {
        t += P[r * n + k] * xbar[i * n + k];
      }
      v[r] = t - sv[r];
    }
    for(int r = 0; r < n; r++)
    {
      double t = 0;
      for(int j = 0; j < gi; j++)
      {
        t += Ci[j * n + r] * tsub[j];
      }
      Lxt[r] = lxbar[i * n + r] + t; // (2.28f)
      for(int c = 0; c < n; c++)
      {
        double q = 0, p2 = 0;
        for(int j = 0; j < gi; j++)
        {
          q += Ci[j * n + r] * (nus[j] * Ci[j * n + c]);
        }
        for(int k = 0; k < n; k++)
        {
          p2 += Ai[k * n + r] * PA[k * n + c];
        }
        F[r * n + c] = (dt * Lxx[r * n + c] + q) + p2; // (2.28c), (2.35b)
      }
    }
    for(int r = 0; r < m; r++)
    {
      double t = 0;
      for(int j = 0; j < gi; j++)
      {
        t += Di[j * mc + r] * tsub[j];
      }
      Lut[r] = lubar[i * mc + r] + t; // (2.28g)
      for(int c = 0; c < n; c++) // H^T(r, c) = H(c, r)    (2.28d), (2.35c)
      {
        double q = 0, p2 = 0;
        for(int j = 0; j < gi; j++)
        {
          q += Di[j * mc + r] * (nus[j] * Ci[j * n + c]);
        }
        for(int k = 0; k < n; k++)
        {
          p2 += Bi[k * mc + r] * PA[k * n + c];
        }
        Ht[r * n + c] = (dt * Lxu[c * mc + r] + q) + p2;
      }
      for(int c = 0; c < m; c++) // (2.28e), (2.35d)
      {
        double q = 0, p2 = 0;
        for(int j = 0; j < gi; j++)
        {
          q += Di[j * mc + r] * (nus[j] * Di[j * mc + c]);
        }
        for(int k = 0; k < n; k++)
        {
          p2 += Bi[k * mc + r] * PB[k * kMax + c];
        }
        G[r * kMax + c] = (dt * Luu[r * mc + c] + q) + p2;
      }
    }
    // gains    :588-627
    double rhs[kMax + 1][kMax]; // column c < n: H^T(:, c); column n: B'(P x_bar - s) + Lu_tilde
    if(m > 0)
    {
      for(int r = 0; r < m; r++)
      {
        for(int c = 0; c < n; c++)
        {
          rhs[c][r] = Ht[r * n + c];
        }
        double t = 0;
        for(int k = 0; k < n; k++)
        {
          t += Bi[k * mc + r] * v[k];
        }
        rhs[n][r] = t + Lut[r];
      }
      Ldlt ldlt;
      if(ldlt.compute(G.data(), kMax, m))
      {
        for(int c = 0; c <= n; c++)
        {
          ldlt.solve(rhs[c]);
        }
      }
      else if(a.break_if_llt_fails)
      {
        return 3;
      }
      else
      {
        luSolve(G.data(), kMax, m, rhs, n + 1);
      }
      for(int c = 0; c <= n; c++)
      {
        for(int r = 0; r < m; r++)
        {
          rhs[c][r] = -1 * rhs[c][r];
        }
      }
    }
    for(int r = 0; r < mc; r++)
    {
      ok[i * mc + r] = (r < m) ? rhs[n][r] : 0.0;
      bad = bad || notFinite(ok[i * mc + r]);
      for(int c = 0; c < n; c++)
      {
        oK[i * mc * n + r * n + c] = (r < m) ? rhs[c][r] : 0.0;
        bad = bad || notFinite(oK[i * mc * n + r * n + c]);
      }
    }
    // post-process    :629-640
    for(int r = 0; r < m; r++)
    {
      for(int c = 0; c < n; c++)
      {
        double t = 0;
        for(int q = 0; q < m; q++)
        {
          t += G[r * kMax + q] * rhs[c][q];
        }
        GK[r * n + c] = t;
      }
    }
    for(int r = 0; r < n; r++)
    {
      double s1 = 0, s2 = 0;
      for(int k = 0; k < n; k++)
      {
        s1 += Ai[k * n + r] * (-1 * v[k]);
      }
      for(int q = 0; q < m; q++)
      {
        s2 += Ht[q * n + r] * rhs[n][q];
      }
      const double t = s1 - Lxt[r];
      Lxt[r] = (m > 0) ? t - s2 : t; // the new s, kept apart until every row has read the old one
      for(int c = 0; c < n; c++)
      {
        double kgk = 0;
        for(int q = 0; q < m; q++)
        {
          kgk += rhs[r][q] * GK[q * n + c];
        }
        Pn[r * n + c] = (m > 0) ? F[r * n + c] - kgk : F[r * n + c];
      }
    }
    for(int r = 0; r < n; r++)
    {
      sv[r] = Lxt[r];
      ogs[i * n + r] = sv[r];
      bad = bad || notFinite(sv[r]);
      for(int c = 0; c < n; c++)
      {
        P[r * n + c] = 0.5 * (Pn[r * n + c] + Pn[c * n + r]);
        oP[i * n * n + r * n + c] = P[r * n + c];
        bad = bad || notFinite(P[r * n + c]);
      }
    }
  }
  if(a.check_nan && bad)
  {
    return 3;
  }

  // forward pass    :668-708
  bool fbad = false;
  for(int r = 0; r < n; r++)
  {
    dx[r] = a.cur_x[b * n + r] - x[r];
  }
  for(int i = 0; i <= T; i++)
  {
    for(int r = 0; r < n; r++)
    {
      double t = 0;
      for(int k = 0; k < n; k++)
      {
        t += oP[i * n * n + r * n + k] * dx[i * n + k];
      }
      dlam[i * n + r] = t - ogs[i * n + r];
      fbad = fbad || notFinite(dx[i * n + r]) || notFinite(dlam[i * n + r]);
    }
    if(i < T)
    {
      const int m = mAt(i);
      for(int r = 0; r < mc; r++)
      {
        double t = 0;
        for(int k = 0; k < n; k++)
        {
          t += oK[i * mc * n + r * n + k] * dx[i * n + k];
        }
        du[i * mc + r] = (r < m) ? t + ok[i * mc + r] : 0.0;
        fbad = fbad || notFinite(du[i * mc + r]);
      }
      for(int r = 0; r < n; r++)
      {
        double s1 = 0, s2 = 0;
        for(int k = 0; k < n; k++)
        {
          s1 += A[i * n * n + r * n + k] * dx[i * n + k];
        }
        for(int q = 0; q < m; q++)
        {
          s2 += Bm[i * n * mc + r * mc + q] * du[i * mc + q];
        }
        dx[(i + 1) * n + r] = ((m > 0) ? s1 + s2 : s1) + xbar[i * n + r];
      }
    }
  }
  double alpha_s = 1.0, alpha_nu = 1.0;
  for(int i = 0; i < T; i++)
  {
    const int m = mAt(i), gi = gAt(i);
    for(int j = 0; j < gc; j++)
    {
      ds[i * gc + j] = dnu[i * gc + j] = 0.0;
      if(j >= gi)
      {
        continue;
      }
      double s1 = 0, s2 = 0;
      for(int k = 0; k < n; k++)
      {
        s1 += C[i * gc * n + j * n + k] * dx[i * n + k];
      }
      for(int q = 0; q < m; q++)
      {
        s2 += D[i * gc * mc + j * mc + q] * du[i * mc + q];
      }
      const double sj = s[i * gc + j], nj = nu[i * gc + j];
      const double d = -1 * ((s1 + s2) + gbar[i * gc + j]);
      const double dn = (-1 * (nj * (d + sj) - eps)) / sj;
      ds[i * gc + j] = d;
      dnu[i * gc + j] = dn;
      fbad = fbad || notFinite(d) || notFinite(dn);
    }
  }
  if(a.check_nan && fbad)
  {
    return 2;
  }
  // step lengths    :713-750
  for(int i = 0; i < T; i++)
  {
    for(int j = 0; j < gAt(i); j++)
    {
      if(ds[i * gc + j] < 0)
      {
        alpha_s = std::min(alpha_s, ((-1 * 0.995) * s[i * gc + j]) / ds[i * gc + j]);
      }
      if(dnu[i * gc + j] < 0)
      {
        alpha_nu = std::min(alpha_nu, ((-1 * 0.995) * nu[i * gc + j]) / dnu[i * gc + j]);
      }
    }
  }
  a.alpha_s[b] = alpha_s;
  a.alpha_nu[b] = alpha_nu;
  if(!(alpha_s > 0.0 && alpha_s <= 1.0 && alpha_nu > 0.0 && alpha_nu <= 1.0))
  {
    return 4;
  }
  // update    :802-831
  if(a.apply_update)
  {
    constexpr double min_positive_value = std::numeric_limits<double>::lowest();
    for(int i = 0; i <= T; i++)
    {
      for(int r = 0; r < n; r++)
      {
        x[i * n + r] += alpha_s * dx[i * n + r];
        lam[i * n + r] += alpha_nu * dlam[i * n + r];
      }
      if(i == T)
      {
        break;
      }
      const int m = mAt(i), gi = gAt(i);
      for(int r = 0; r < m; r++)
      {
        u[i * mc + r] += alpha_s * du[i * mc + r];
      }
      bool s_neg = false, nu_neg = false;
      for(int j = 0; j < gi; j++)
      {
        s[i * gc + j] += alpha_s * ds[i * gc + j];
        nu[i * gc + j] += alpha_nu * dnu[i * gc + j];
        s_neg = s_neg || s[i * gc + j] < 0;
        nu_neg = nu_neg || nu[i * gc + j] < 0;
      }
      for(int j = 0; j < gi; j++)
      {
        if(s_neg)
        {
          s[i * gc + j] = (s[i * gc + j] < min_positive_value) ? min_positive_value : s[i * gc + j];
        }
        if(nu_neg)
        {
          nu[i * gc + j] = (nu[i * gc + j] < min_positive_value) ? min_positive_value : nu[i * gc + j];
        }
      }
    }
  }
  return 6;
}
} // namespace

extern "C"
{
  /** One procOnce of every instance; arrays row-major with the capacities as block sizes; x, u, lam, s, nu, eps in / out. */
  int fmpc_step_chk_step(int B,
                         int n,
                         int m,
                         int g,
                         int T,
                         const int * mdims,
                         const int * gdims,
                         const double * A,
                         const double * Bm,
                         const double * C,
                         const double * D,
                         const double * Lx,
                         const double * Lu,
                         const double * Lxx,
                         const double * Luu,
                         const double * Lxu,
                         const double * f,
                         const double * gv,
                         const double * LxT,
                         const double * LxxT,
                         const double * cur_x,
                         double * x,
                         double * u,
                         double * lam,
                         double * s,
                         double * nu,
                         double * eps,
                         double dt,
                         double kkt_error_thre,
                         int check_nan,
                         int init_complementary_variable,
                         int update_barrier_eps,
                         int break_if_llt_fails,
                         int apply_update,
                         int n_threads,
                         int * status,
                         double * kkt,
                         double * alpha_s,
                         double * alpha_nu,
                         double * k,
                         double * K,
                         double * gs,
                         double * P,
                         double * dx,
                         double * du,
                         double * dlam,
                         double * ds,
                         double * dnu)
  {
    if(n < 1 || n > kMax || m < 0 || m > kMax || g < 0 || g > 32 || T < 1 || B < 1)
    {
      return -1;
    }
    const Args a{{n, m, g, T}, mdims, gdims, A, Bm, C, D, Lx, Lu, Lxx, Luu, Lxu, f, gv, LxT, LxxT, cur_x, x, u, lam, s, nu, eps, dt,
                 kkt_error_thre, check_nan, init_complementary_variable, update_barrier_eps, break_if_llt_fails, apply_update, status,
                 kkt, alpha_s, alpha_nu, k, K, gs, P, dx, du, dlam, ds, dnu};
    const int nt = std::max(1, std::min(n_threads, B));
    std::vector<std::thread> pool;
    for(int t = 0; t < nt; t++)
    {
      pool.emplace_back([&, t]() {
        for(int b = t; b < B; b += nt)
        {
          status[b] = stepOne(a, static_cast<size_t>(b));
        }
      });
    }
    for(auto & th : pool)
    {
      th.join();
    }
    return 0;
  }

  /** x = G^-1 b through the LDLT (use_lu = 0) or the full-pivot LU (use_lu = 1); G row-major m x m, b [c][m] in place.  Returns the
      LDLT's info() == Success (1 / 0); the LDLT path solves whatever info() says. */
  int fmpc_step_chk_ldlt_solve(const double * G, int m, double * b, int c, int use_lu)
  {
    if(m < 1 || m > kMax || c < 1 || c > kMax + 1)
    {
      return -1;
    }
    Ldlt ldlt;
    const bool ok = ldlt.compute(G, m, m);
    double rhs[kMax + 1][kMax];
    for(int q = 0; q < c; q++)
    {
      for(int i = 0; i < m; i++)
      {
        rhs[q][i] = b[q * m + i];
      }
    }
    if(use_lu)
    {
      luSolve(G, m, m, rhs, c);
    }
    else
    {
      for(int q = 0; q < c; q++)
      {
        ldlt.solve(rhs[q]);
      }
    }
    for(int q = 0; q < c; q++)
    {
      for(int i = 0; i < m; i++)
      {
        b[q * m + i] = rhs[q][i];
      }
    }
    return ok ? 1 : 0;
  }
}
