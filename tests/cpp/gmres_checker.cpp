// CPU checker of the batched GMRES solver: a plain-array restatement of the reference's nmpc_cgmres::Gmres::solve
// (nmpc_cgmres/include/nmpc_cgmres/Gmres.h:67-192), both variants (make_triangular_ true: Givens, false: Householder least squares).
// Built by tests/gmres_checker.py with g++ -O2 -ffp-contract=off, so every operation is the IEEE operation written here.
//
// Sums come in two orders (argument `wave`):
//   0  sequential: a dot product is p = 0, p = p + a[i] * b[i] for i ascending, the reference's left-to-right order;
//   1  wave: the order of gmres_wave_kernel (include/nmpc_amd/hip/gmres_kernels.hpp): lane l of 64 sums its rows l, l + 64, ...
//      ascending, then the butterfly p[l] = p[l] + p[l ^ m] for m = 32, 16, 8, 4, 2, 1.
// Everything else is the same in both: entry i of A v is the sum over j ascending; the Gram-Schmidt loop, the re-orthogonalisation
// test, the rotations and the back substitution (by columns) are the reference's statements in its order; the Householder variant
// solves the (k + 1) x k least-squares problem of every iteration by an unblocked Householder QR of [H | g] (the column norm and
// every column's update are sequential sums) and forms rho = || g - H y || as Gmres.h:175 does.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <limits>
#include <thread>
#include <vector>

namespace
{
using Vec = std::vector<double>;

double dotOrdered(const double * a, const double * b, int n, bool wave)
{
  if(!wave)
  {
    double p = 0.0;
    for(int i = 0; i < n; i++)
    {
      p = p + a[i] * b[i];
    }
    return p;
  }
  double p[64], q[64];
  for(int l = 0; l < 64; l++)
  {
    p[l] = 0.0;
    for(int i = l; i < n; i += 64)
    {
      p[l] = p[l] + a[i] * b[i];
    }
  }
  for(int m = 32; m >= 1; m >>= 1)
  {
    for(int l = 0; l < 64; l++)
    {
      q[l] = p[l] + p[l ^ m];
    }
    std::copy(q, q + 64, p);
  }
  return p[0];
}

void matVec(const double * A, const double * v, double * out, int n)
{
  for(int i = 0; i < n; i++)
  {
    double acc = 0.0;
    for(int j = 0; j < n; j++)
    {
      acc = acc + A[static_cast<size_t>(i) * n + j] * v[j];
    }
    out[i] = acc;
  }
}

/** v.normalized(): divided by sqrt(squared norm) where that is > 0, unchanged otherwise. */
void normalizedInto(const double * w, double zz, double * out, int n)
{
  const double nrm = std::sqrt(zz);
  for(int i = 0; i < n; i++)
  {
    out[i] = zz > 0.0 ? w[i] / nrm : w[i];
  }
}

/** y = R^{-1} y by columns: for i = k - 1 .. 0: y[i] = y[i] / R(i, i); y[j] = y[j] - y[i] * R(j, i), j < i. */
template<class R>
void backSubstitute(double * y, int k, const R & r)
{
  for(int i = k - 1; i >= 0; i--)
  {
    y[i] = y[i] / r(i, i);
    for(int j = 0; j < i; j++)
    {
      y[j] = y[j] - y[i] * r(j, i);
    }
  }
}

struct Out
{
  int * iters;
  int * reorth;
  int * status;
  double * err; // [K + 1]
  double * H; // [K + 1][K]
  double * g; // [K + 1]
  double * basis; // [K + 1][n] or null
  double * y; // [K] or null
  int * fired_at; // [K + 1]: fired_at[k] = 1 iff iteration k re-orthogonalised; or null
};

void solveOne(int n, const double * A, const double * b, double * x, int k_max, double eps, bool tri, bool reorth, bool wave, const Out & o)
{
  const int K = std::min(k_max, n); // :73
  const int LD = K + 1;
  Vec w(n), Ax(n), y(K, 0.0), hcol(K + 1), cs, sn, W(static_cast<size_t>(LD) * LD), u(K + 1);
  std::vector<Vec> V;
  Vec g(K + 1, 0.0);
  Vec H(static_cast<size_t>(K + 1) * K, 0.0);
  for(int i = 0; i <= K; i++)
  {
    o.err[i] = std::numeric_limits<double>::quiet_NaN();
    if(o.fired_at)
    {
      o.fired_at[i] = 0;
    }
  }
  // 1.
  matVec(A, x, Ax.data(), n);
  for(int i = 0; i < n; i++)
  {
    w[i] = b[i] - Ax[i];
  }
  const double rr = dotOrdered(w.data(), w.data(), n, wave);
  double rho = std::sqrt(rr);
  const double b_norm = std::sqrt(dotOrdered(b, b, n, wave));
  V.emplace_back(n);
  normalizedInto(w.data(), rr, V[0].data(), n);
  g[0] = rho;
  o.err[0] = rho;
  int k = 0, fired = 0;
  // 2.
  while(rho > eps * b_norm && k < K)
  {
    k++;
    matVec(A, V.back().data(), w.data(), n);
    const double avk_norm = std::sqrt(dotOrdered(w.data(), w.data(), n, wave));
    for(int j = 0; j < k; j++)
    {
      const double h = dotOrdered(w.data(), V[j].data(), n, wave);
      hcol[j] = h;
      for(int i = 0; i < n; i++)
      {
        w[i] = w[i] - h * V[j][i];
      }
    }
    double zz = dotOrdered(w.data(), w.data(), n, wave);
    const double new_basis_norm = std::sqrt(zz);
    hcol[k] = new_basis_norm;
    if(reorth && avk_norm + 1e-3 * new_basis_norm == avk_norm)
    {
      fired++;
      if(o.fired_at)
      {
        o.fired_at[k] = 1;
      }
      for(int j = 0; j < k; j++)
      {
        const double h_tmp = dotOrdered(w.data(), V[j].data(), n, wave);
        hcol[j] = hcol[j] + h_tmp;
        for(int i = 0; i < n; i++)
        {
          w[i] = w[i] - h_tmp * V[j][i];
        }
      }
      zz = dotOrdered(w.data(), w.data(), n, wave);
    }
    V.emplace_back(n);
    normalizedInto(w.data(), zz, V[k].data(), n);
    if(tri)
    {
      double t = hcol[0];
      for(int i = 0; i < k - 1; i++)
      {
        const double h1 = hcol[i + 1], c = cs[i], s = sn[i];
        hcol[i] = c * t - s * h1;
        t = s * t + c * h1;
      }
      const double hk = hcol[k];
      const double nu = std::sqrt(t * t + hk * hk);
      const double c_k = t / nu, s_k = -hk / nu;
      cs.push_back(c_k);
      sn.push_back(s_k);
      hcol[k - 1] = c_k * t - s_k * hk;
      hcol[k] = 0.0;
      const double g0 = g[k - 1], g1 = g[k];
      g[k - 1] = c_k * g0 - s_k * g1;
      g[k] = s_k * g0 + c_k * g1;
      rho = std::fabs(g[k]);
      for(int i = 0; i <= k; i++)
      {
        H[static_cast<size_t>(i) * K + (k - 1)] = hcol[i];
      }
    }
    else
    {
      for(int i = 0; i <= k; i++)
      {
        H[static_cast<size_t>(i) * K + (k - 1)] = hcol[i];
      }
      for(int i = 0; i <= k; i++)
      {
        for(int c = 0; c <= k; c++)
        {
          W[i * LD + c] = c < k ? H[static_cast<size_t>(i) * K + c] : g[i];
        }
      }
      for(int j = 0; j < k; j++)
      {
        const double alpha = W[j * LD + j];
        double ss = 0.0;
        for(int i = j + 1; i <= k; i++)
        {
          ss = ss + W[i * LD + j] * W[i * LD + j];
        }
        if(ss != 0.0)
        {
          const double nrm = std::sqrt(alpha * alpha + ss);
          const double beta = alpha >= 0.0 ? -nrm : nrm;
          const double tau = (beta - alpha) / beta;
          const double den = alpha - beta;
          for(int i = j + 1; i <= k; i++)
          {
            u[i] = W[i * LD + j] / den;
          }
          for(int c = j + 1; c <= k; c++)
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
          W[j * LD + j] = beta;
        }
      }
      for(int i = 0; i < k; i++)
      {
        y[i] = W[i * LD + k];
      }
      backSubstitute(y.data(), k, [&](int r, int c) { return W[r * LD + c]; });
      Vec t(k + 1);
      for(int i = 0; i <= k; i++)
      {
        double s = 0.0;
        for(int j = 0; j < k; j++)
        {
          s = s + H[static_cast<size_t>(i) * K + j] * y[j];
        }
        t[i] = g[i] - s;
      }
      rho = std::sqrt(dotOrdered(t.data(), t.data(), k + 1, wave));
    }
    o.err[k] = rho;
  }
  if(tri)
  {
    // 3.
    for(int i = 0; i < k; i++)
    {
      y[i] = g[i];
    }
    backSubstitute(y.data(), k, [&](int r, int c) { return H[static_cast<size_t>(r) * K + c]; });
  }
  // 4.
  bool finite = std::isfinite(rho);
  for(int i = 0; i < n; i++)
  {
    double xi = x[i];
    for(int j = 0; j < k; j++)
    {
      xi = xi + y[j] * V[j][i];
    }
    x[i] = xi;
    finite = finite && std::isfinite(xi);
  }
  *o.iters = k;
  *o.reorth = fired;
  *o.status = !finite ? 3 : (rho > eps * b_norm ? 2 : 1);
  std::copy(H.begin(), H.end(), o.H);
  std::copy(g.begin(), g.end(), o.g);
  if(o.y)
  {
    std::copy(y.begin(), y.end(), o.y);
  }
  if(o.basis)
  {
    std::fill(o.basis, o.basis + static_cast<size_t>(K + 1) * n, 0.0);
    for(int j = 0; j <= k; j++)
    {
      std::copy(V[j].begin(), V[j].end(), o.basis + static_cast<size_t>(j) * n);
    }
  }
}
} // namespace

extern "C"
{
  /** B systems (A [B][n][n] row-major, b [B][n], x [B][n] in / out); outputs as the fields of include/nmpc_hip_gmres.h with
      K = min(k_max, n); basis, y ([B][K]) and fired_at ([B][K + 1]) may be NULL.  Returns 0. */
  int gmres_chk_solve(int B, int n, const double * A, const double * b, double * x, int k_max, double eps, int make_triangular, int apply_reorth,
                      int wave, int n_threads, int * iters, int * reorth, int * status, double * err, double * H, double * g, double * basis,
                      double * y, int * fired_at)
  {
    const size_t K = std::min(k_max, n), N = n;
    auto work = [&](int s) {
      const Out o{iters + s, reorth + s, status + s, err + s * (K + 1), H + s * (K + 1) * K, g + s * (K + 1),
                  basis ? basis + s * (K + 1) * N : nullptr, y ? y + s * K : nullptr, fired_at ? fired_at + s * (K + 1) : nullptr};
      solveOne(n, A + s * N * N, b + s * N, x + s * N, k_max, eps, make_triangular != 0, apply_reorth != 0, wave != 0, o);
    };
    const int T = std::max(1, std::min(n_threads, B));
    std::vector<std::thread> pool;
    for(int t = 0; t < T; t++)
    {
      pool.emplace_back([&, t] {
        for(int s = t; s < B; s += T)
        {
          work(s);
        }
      });
    }
    for(auto & th : pool)
    {
      th.join();
    }
    return 0;
  }
}
