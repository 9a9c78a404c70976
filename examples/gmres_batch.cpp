// The loop of the reference's TestGmres.cpp (:98-142) through nmpc_amd::GmresBatch: per size, the ten random systems are ONE batch,
// solved by the Givens variant, the Householder variant (sizes <= 100), without re-orthogonalisation and with k_max = 20, and the
// mean of |A x - b| is held against the reference's bars.
//
//   g++ -std=c++17 -O2 -Iinclude examples/gmres_batch.cpp -Lnmpc_amd/lib -lnmpc_hip_ddp -Wl,-rpath,$PWD/nmpc_amd/lib -o gmres_batch
//   ./gmres_batch [trial_num] [size ...]
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <stdexcept>
#include <string>
#include <vector>

#include <nmpc_amd/GmresBatch.hpp>

namespace
{
/** Positive integers from the command line: trial_num, then sizes in 1 .. 512. */
bool parseArgs(int argc, char ** argv, int & trial_num, std::vector<int> & sizes)
{
  for(int a = 1; a < argc; a++)
  {
    char * end = nullptr;
    const long v = std::strtol(argv[a], &end, 10);
    if(end == argv[a] || *end != '\0' || v < 1 || v > (a == 1 ? 100000 : nmpc_amd::GmresBatch::MaxDim))
    {
      std::fprintf(stderr, "usage: %s [trial_num >= 1] [size in 1 .. %d ...]\n", argv[0], nmpc_amd::GmresBatch::MaxDim);
      return false;
    }
    if(a == 1)
    {
      trial_num = static_cast<int>(v);
    }
    else
    {
      if(a == 2)
      {
        sizes.clear();
      }
      sizes.push_back(static_cast<int>(v));
    }
  }
  return true;
}

double meanResidual(const std::vector<double> & A, const std::vector<double> & b, const std::vector<double> & x, int B, int n)
{
  double err = 0;
  for(int s = 0; s < B; s++)
  {
    double rr = 0;
    for(int i = 0; i < n; i++)
    {
      double r = -b[static_cast<size_t>(s) * n + i];
      for(int j = 0; j < n; j++)
      {
        r += A[(static_cast<size_t>(s) * n + i) * n + j] * x[static_cast<size_t>(s) * n + j];
      }
      rr += r * r;
    }
    err += std::sqrt(rr);
  }
  return err / B;
}
} // namespace

int main(int argc, char ** argv)
{
  int trial_num = 10;
  std::vector<int> sizes = {10, 50, 100, 500};
  if(!parseArgs(argc, argv, trial_num, sizes))
  {
    return 2;
  }
  std::mt19937_64 rng(1);
  std::uniform_real_distribution<double> uniform(-1.0, 1.0); // Eigen's Random()
  bool ok = true;
  try
  {
    for(int n : sizes)
    {
      std::vector<double> A(static_cast<size_t>(trial_num) * n * n), b(static_cast<size_t>(trial_num) * n);
      for(double & a : A)
      {
        a = uniform(rng);
      }
      for(double & e : b)
      {
        e = uniform(rng);
      }
      std::printf("======== eq_size: %d ========\n", n);
      nmpc_amd::GmresBatch solver(n, trial_num, 1000);
      struct Leg
      {
        const char * name;
        int k_max;
        bool make_triangular, apply_reorth;
        double bar;
      };
      const Leg legs[] = {{"Gmres", 1000, true, true, 1e-10},
                          {"Gmres (no triangular)", 1000, false, true, 1e-10},
                          {"Gmres (no reorthogonalization)", 1000, true, false, 1e-10},
                          {"Gmres (small iteration)", 20, true, true, 1e2}};
      for(const Leg & leg : legs)
      {
        if(!leg.make_triangular && n > 100)
        {
          continue; // TestGmres.cpp:122
        }
        solver.make_triangular_ = leg.make_triangular;
        solver.apply_reorth_ = leg.apply_reorth;
        std::vector<double> x(b.size(), 0.0);
        solver.solve(A, b, x, leg.k_max, 1e-10);
        const double err = meanResidual(A, b, x, trial_num, n);
        std::printf("== %s ==\nkernel ms: %.3f, ave err: %g, iterations of system 0: %d, status %d\n", leg.name, solver.lastMs(), err,
                    solver.iters(0), solver.status(0));
        ok = ok && err < leg.bar;
      }
    }
  }
  catch(const std::invalid_argument & e)
  {
    std::printf("invalid_argument: %s\n", e.what());
    return 1;
  }
  catch(const std::runtime_error & e)
  {
    std::printf("runtime_error: %s\n", e.what());
    return std::string(e.what()).rfind("no HIP device available", 0) == 0 ? 0 : 1; // no device: nothing to show
  }
  std::printf(ok ? "ok gmres_wave_kernel\n" : "FAILED\n");
  return ok ? 0 : 1;
}
