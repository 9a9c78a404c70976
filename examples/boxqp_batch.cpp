// Batched box-constrained QPs through nmpc_amd::BoxQPBatch, the mirror of the reference's BoxQP<VarDim> (BoxQP.h): a force
// distribution flavoured example — B = 4096 independent QPs  min 1/2 x'Hx + g'x,  0 <= x <= f_max  of n = 12 variables each.
//
//   g++ -std=c++17 -O2 -Iinclude examples/boxqp_batch.cpp -Lnmpc_amd/lib -lnmpc_hip_ddp -Wl,-rpath,$PWD/nmpc_amd/lib -o boxqp_batch
#include <cstdio>
#include <random>
#include <vector>

#include <nmpc_amd/BoxQPBatch.hpp>

int main()
{
  constexpr int n = 12;
  const int B = 4096;
  std::mt19937_64 rng(1);
  std::normal_distribution<double> normal;
  std::vector<double> H(static_cast<size_t>(B) * n * n), g(static_cast<size_t>(B) * n), lower(g.size(), 0.0), upper(g.size(), 2.0);
  for(int b = 0; b < B; b++)
  {
    // H = A A' + 0.3 I: symmetric positive definite
    double A[n][n];
    for(auto & row : A)
    {
      for(double & a : row)
      {
        a = normal(rng);
      }
    }
    for(int i = 0; i < n; i++)
    {
      for(int j = 0; j < n; j++)
      {
        double s = i == j ? 0.3 : 0.0;
        for(int k = 0; k < n; k++)
        {
          s += A[i][k] * A[j][k];
        }
        H[(static_cast<size_t>(b) * n + i) * n + j] = s;
      }
      g[static_cast<size_t>(b) * n + i] = 2 * normal(rng);
    }
  }

  nmpc_amd::BoxQPBatch<n> qp(B);
  qp.config().print_level = 0;
  const std::vector<double> x = qp.solve(H, g, lower, upper);
  int by_retval[9] = {};
  for(int b = 0; b < B; b++)
  {
    by_retval[qp.retval(b) + 2 < 9 ? qp.retval(b) + 2 : 0]++;
  }
  std::printf("%d QPs of %d variables on %s in %.3f ms\n", B, n, qp.kernelName().c_str(), qp.lastSolveMs());
  for(int r = -2; r <= 6; r++)
  {
    if(by_retval[r + 2])
    {
      std::printf("  retval %2d (%s): %d\n", r, qp.retstr_.at(r).c_str(), by_retval[r + 2]);
    }
  }
  std::printf("x[0] =");
  for(int i = 0; i < n; i++)
  {
    std::printf(" %.6f", x[i]);
  }
  std::printf("\n  free indices of QP 0: %zu of %d\n", qp.freeIdxs(0).size(), n);
  return 0;
}
