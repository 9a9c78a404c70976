// CPU checker of the batched Riccati backward pass: a plain-array restatement of the reference's DDPSolver::backwardPass
// (nmpc_ddp/include/nmpc_ddp/DDPSolver.hpp:342-534), the lambda retry loop of procOnce (:188-214) and the BoxQP feed-forward
// (:450-497) on caller-supplied derivatives.  Built by tests/riccati_checker.py with g++ -O2 -ffp-contract=off, so every operation is
// the IEEE operation written here.  The dense helpers, the factorisation and BoxQP are those of oracle/ddp_oracle.hpp (column-major,
// sums in ascending index order); the statements of the pass are in the reference's order.  Threaded over instances.
//
// Arrays at this boundary are the row-major images a contiguous numpy array [B][T][rows][cols] has, with the capacities (n, m) as
// block sizes; at a step with dims[i] = m_i < m only the leading m_i rows and columns are read and outputs beyond m_i are 0.
#include <algorithm>
#include <cstddef>
#include <thread>
#include <vector>

#include "../../oracle/ddp_oracle.hpp"

namespace
{
using oracle::BoxQP;
using oracle::lltInPlace;
using oracle::lltSolveInPlace;
using oracle::mulAB;
using oracle::mulAtB;
using Vec = std::vector<double>;

struct Problem
{
  int n, m, T;
  const int * dims;
  const double *Fx, *Fu, *Lx, *Lu, *Lxx, *Luu, *Lxu, *VxT, *VxxT; // of one instance
  const double *U, *lower, *upper; // U of one instance; limits [m] or this instance's [T][m]
  int limits_per_step, with_constraint, reg_type;
};

struct Outputs
{
  double *k, *K, *dV, *Vx0, *Vxx0; // of one instance
  int * qp_retval;
  unsigned * free_mask;
};

/** rows x cols leading part of a row-major block with `cols_cap` columns -> column-major, compact. */
void toColMajor(const double * src, int rows, int cols, int cols_cap, Vec & dst)
{
  dst.assign(static_cast<size_t>(rows) * cols, 0.0);
  for(int r = 0; r < rows; r++)
  {
    for(int c = 0; c < cols; c++)
    {
      dst[r + static_cast<size_t>(c) * rows] = src[static_cast<size_t>(r) * cols_cap + c];
    }
  }
}

/** One pass at `lambda`; returns the failing step or -1. */
int backwardPass(const Problem & p, double lambda, const Outputs & out)
{
  const int N = p.n, M = p.m, T = p.T;
  Vec Vx(p.VxT, p.VxT + N), Vxx, Vxx_reg(static_cast<size_t>(N) * N);
  toColMajor(p.VxxT, N, N, N, Vxx);
  Vec Fx, Fu, Lxx, Luu, Lxu;
  Vec Qu(M), Qx(N), Qux(static_cast<size_t>(M) * N), Quu(static_cast<size_t>(M) * M), Qxx(static_cast<size_t>(N) * N),
      Qux_reg(static_cast<size_t>(M) * N), Quu_F(static_cast<size_t>(M) * M);
  const size_t pmax = static_cast<size_t>(std::max(N, M)) * std::max(N, M);
  Vec FuT_V(static_cast<size_t>(M) * N), FxT_V(static_cast<size_t>(N) * N), prod(pmax), KtQuu(static_cast<size_t>(N) * M);
  Vec k(M, 0.0), K(static_cast<size_t>(M) * N, 0.0), tmp_m(M), k_next(M, 0.0);
  int m_next = -1;
  out.dV[0] = 0;
  out.dV[1] = 0;

  for(int i = T - 1; i >= 0; i--)
  {
    const int m = p.dims ? p.dims[i] : M;
    toColMajor(p.Fx + static_cast<size_t>(i) * N * N, N, N, N, Fx);
    toColMajor(p.Lxx + static_cast<size_t>(i) * N * N, N, N, N, Lxx);
    toColMajor(p.Fu + static_cast<size_t>(i) * N * M, N, m, M, Fu);
    toColMajor(p.Lxu + static_cast<size_t>(i) * N * M, N, m, M, Lxu);
    toColMajor(p.Luu + static_cast<size_t>(i) * M * M, m, m, M, Luu);
    const double * Lx = p.Lx + static_cast<size_t>(i) * N;
    const double * Lu = p.Lu + static_cast<size_t>(i) * M;

    // Q terms    :386-408
    for(int a = 0; a < m; a++)
    {
      double s = 0;
      for(int r = 0; r < N; r++)
      {
        s += Fu[r + a * N] * Vx[r];
      }
      Qu[a] = Lu[a] + s;
    }
    for(int a = 0; a < N; a++)
    {
      double s = 0;
      for(int r = 0; r < N; r++)
      {
        s += Fx[r + a * N] * Vx[r];
      }
      Qx[a] = Lx[a] + s;
    }
    mulAtB(Fu.data(), Vxx.data(), FuT_V.data(), m, N, N);
    mulAB(FuT_V.data(), Fx.data(), prod.data(), m, N, N);
    for(int c = 0; c < N; c++)
    {
      for(int a = 0; a < m; a++)
      {
        Qux[a + c * m] = Lxu[c + a * N] + prod[a + c * m];
      }
    }
    mulAB(FuT_V.data(), Fu.data(), prod.data(), m, N, m);
    for(int e = 0; e < m * m; e++)
    {
      Quu[e] = Luu[e] + prod[e];
    }
    mulAtB(Fx.data(), Vxx.data(), FxT_V.data(), N, N, N);
    mulAB(FxT_V.data(), Fx.data(), prod.data(), N, N, N);
    for(int e = 0; e < N * N; e++)
    {
      Qxx[e] = Lxx[e] + prod[e];
    }

    // regularisation    :421-441
    Vxx_reg = Vxx;
    if(p.reg_type == 2)
    {
      for(int j = 0; j < N; j++)
      {
        Vxx_reg[j + j * N] += lambda;
      }
    }
    mulAtB(Fu.data(), Vxx_reg.data(), FuT_V.data(), m, N, N);
    mulAB(FuT_V.data(), Fx.data(), prod.data(), m, N, N);
    for(int c = 0; c < N; c++)
    {
      for(int a = 0; a < m; a++)
      {
        Qux_reg[a + c * m] = Lxu[c + a * N] + prod[a + c * m];
      }
    }
    mulAB(FuT_V.data(), Fu.data(), prod.data(), m, N, m);
    for(int e = 0; e < m * m; e++)
    {
      Quu_F[e] = Luu[e] + prod[e];
    }
    if(p.reg_type == 1)
    {
      for(int a = 0; a < m; a++)
      {
        Quu_F[a + a * m] += lambda;
      }
    }

    // gains    :448-517
    if(m > 0)
    {
      if(p.with_constraint)
      {
        Vec initial_k(m, 0.0), lo(m), up(m); // :452-467
        if(i != T - 1 && m_next == m)
        {
          std::copy(k_next.begin(), k_next.begin() + m, initial_k.begin());
        }
        const double * u = p.U + static_cast<size_t>(i) * M;
        const size_t lim_at = p.limits_per_step ? static_cast<size_t>(i) * M : 0;
        for(int a = 0; a < m; a++)
        {
          lo[a] = p.lower[lim_at + a] - u[a]; // :470-472
          up[a] = p.upper[lim_at + a] - u[a];
        }
        BoxQP qp;
        qp.solve(m, Quu_F.data(), Qu.data(), lo.data(), up.data(), initial_k.data());
        out.qp_retval[i] = qp.retval;
        unsigned mask = 0;
        for(int idx : qp.free_idxs)
        {
          mask |= (1u << idx);
        }
        out.free_mask[i] = mask;
        if(qp.retval < 0)
        {
          return i; // :473-480
        }
        std::copy(qp.x.begin(), qp.x.end(), k.begin());
        std::fill(K.begin(), K.end(), 0.0); // :482-496
        const int nf = static_cast<int>(qp.free_idxs.size());
        if(nf > 0)
        {
          Vec Kf(static_cast<size_t>(nf) * N);
          for(int c = 0; c < N; c++)
          {
            for(int j = 0; j < nf; j++)
            {
              Kf[j + c * nf] = Qux_reg[qp.free_idxs[j] + c * m];
            }
          }
          lltSolveInPlace(qp.llt_free.data(), nf, Kf.data(), N);
          for(int c = 0; c < N; c++)
          {
            for(int j = 0; j < nf; j++)
            {
              K[qp.free_idxs[j] + c * m] = -1 * Kf[j + c * nf];
            }
          }
        }
      }
      else
      {
        Vec L(Quu_F.begin(), Quu_F.begin() + static_cast<size_t>(m) * m); // :500-510
        if(lltInPlace(L.data(), m) >= 0)
        {
          return i;
        }
        std::copy(Qu.begin(), Qu.begin() + m, k.begin());
        lltSolveInPlace(L.data(), m, k.data(), 1);
        for(int a = 0; a < m; a++)
        {
          k[a] = -1 * k[a];
        }
        std::copy(Qux_reg.begin(), Qux_reg.begin() + static_cast<size_t>(m) * N, K.begin());
        lltSolveInPlace(L.data(), m, K.data(), N);
        for(int e = 0; e < m * N; e++)
        {
          K[e] = -1 * K[e];
        }
      }
    }

    // value update with the unregularised Quu, Qux    :522-526
    {
      double kQu = 0;
      for(int a = 0; a < m; a++)
      {
        kQu += k[a] * Qu[a];
      }
      double kQuuk = 0;
      for(int a = 0; a < m; a++)
      {
        double s = 0;
        for(int b = 0; b < m; b++)
        {
          s += Quu[a + b * m] * k[b];
        }
        tmp_m[a] = s;
      }
      for(int a = 0; a < m; a++)
      {
        kQuuk += k[a] * tmp_m[a];
      }
      out.dV[0] += kQu;
      out.dV[1] += 0.5 * kQuuk;
    }
    mulAtB(K.data(), Quu.data(), KtQuu.data(), N, m, m);
    for(int r = 0; r < N; r++)
    {
      double s1 = 0, s2 = 0, s3 = 0;
      for(int a = 0; a < m; a++)
      {
        s1 += KtQuu[r + a * N] * k[a];
      }
      for(int a = 0; a < m; a++)
      {
        s2 += K[a + r * m] * Qu[a];
      }
      for(int a = 0; a < m; a++)
      {
        s3 += Qux[a + r * m] * k[a];
      }
      Vx[r] = ((Qx[r] + s1) + s2) + s3;
    }
    for(int c = 0; c < N; c++)
    {
      for(int r = 0; r < N; r++)
      {
        double s1 = 0, s2 = 0, s3 = 0;
        for(int a = 0; a < m; a++)
        {
          s1 += KtQuu[r + a * N] * K[a + c * m];
        }
        for(int a = 0; a < m; a++)
        {
          s2 += K[a + r * m] * Qux[a + c * m];
        }
        for(int a = 0; a < m; a++)
        {
          s3 += Qux[a + r * m] * K[a + c * m];
        }
        prod[r + c * N] = ((Qxx[r + c * N] + s1) + s2) + s3;
      }
    }
    for(int c = 0; c < N; c++)
    {
      for(int r = 0; r < N; r++)
      {
        Vxx[r + c * N] = 0.5 * (prod[r + c * N] + prod[c + r * N]);
      }
    }

    // save gains    :529-530 (row-major blocks, zero beyond m)
    for(int a = 0; a < M; a++)
    {
      out.k[static_cast<size_t>(i) * M + a] = (a < m) ? k[a] : 0.0;
      for(int c = 0; c < N; c++)
      {
        out.K[(static_cast<size_t>(i) * M + a) * N + c] = (a < m) ? K[a + c * m] : 0.0;
      }
    }
    std::copy(k.begin(), k.end(), k_next.begin());
    m_next = m;
  }
  for(int r = 0; r < N; r++)
  {
    out.Vx0[r] = Vx[r];
    for(int c = 0; c < N; c++)
    {
      out.Vxx0[static_cast<size_t>(r) * N + c] = Vxx[r + c * N];
    }
  }
  return -1;
}
} // namespace

extern "C" int riccati_chk_backward(int B,
                                    int n,
                                    int m,
                                    int T,
                                    const int * dims,
                                    const double * Fx,
                                    const double * Fu,
                                    const double * Lx,
                                    const double * Lu,
                                    const double * Lxx,
                                    const double * Luu,
                                    const double * Lxu,
                                    const double * VxT,
                                    const double * VxxT,
                                    const double * U,
                                    const double * lower,
                                    const double * upper,
                                    int limits_per_step,
                                    int with_constraint,
                                    int reg_type,
                                    const double * lambda_in,
                                    const double * dlambda_in,
                                    double lambda_factor,
                                    double lambda_min,
                                    double lambda_max,
                                    int retry,
                                    int n_threads,
                                    double * k,
                                    double * K,
                                    double * dV,
                                    double * Vx0,
                                    double * Vxx0,
                                    int * status,
                                    int * n_backward,
                                    double * lambda_out,
                                    double * dlambda_out,
                                    int * fail_step,
                                    int * qp_retval,
                                    unsigned * free_mask)
{
  auto one = [&](size_t b) {
    const size_t S = b * T;
    const size_t nn = static_cast<size_t>(n) * n, nm = static_cast<size_t>(n) * m, mm = static_cast<size_t>(m) * m;
    Problem p{n, m, T, dims, Fx + S * nn, Fu + S * nm, Lx + S * n, Lu + S * m, Lxx + S * nn, Luu + S * mm, Lxu + S * nm,
              VxT + b * n, VxxT + b * nn, U ? U + S * m : nullptr, (lower && limits_per_step) ? lower + S * m : lower,
              (upper && limits_per_step) ? upper + S * m : upper, limits_per_step, with_constraint, reg_type};
    Outputs out{k + S * m, K + S * nm, dV + b * 2, Vx0 + b * n, Vxx0 + b * nn, qp_retval + S, free_mask + S};
    double lambda = lambda_in[b], dlambda = dlambda_in[b];
    int nb = 0, st = 0, fs = -1;
    for(;;) // :188-214
    {
      nb++;
      const int failed_at = backwardPass(p, lambda, out);
      if(failed_at < 0)
      {
        st = 1;
        break;
      }
      fs = failed_at;
      if(!retry)
      {
        st = -2;
        break;
      }
      dlambda = std::max(dlambda * lambda_factor, lambda_factor);
      lambda = std::max(lambda * dlambda, lambda_min);
      if(lambda > lambda_max)
      {
        st = -1;
        break;
      }
    }
    status[b] = st;
    n_backward[b] = nb;
    lambda_out[b] = lambda;
    dlambda_out[b] = dlambda;
    fail_step[b] = fs;
  };
  const int nt = std::max(1, std::min(n_threads, B));
  std::vector<std::thread> pool;
  for(int t = 0; t < nt; t++)
  {
    pool.emplace_back([&, t] {
      for(size_t b = t; b < static_cast<size_t>(B); b += nt)
      {
        one(b);
      }
    });
  }
  for(auto & th : pool)
  {
    th.join();
  }
  return 0;
}
