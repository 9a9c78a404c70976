// Test program of tests/test_gpu_fmpc_dynamic.py: nmpc_amd::FmpcSolverBatch (include/nmpc_amd/FmpcSolverBatch.hpp) on a problem
// with time-varying dimensions.  Solves B instances from per-step sized initial guesses, prints status, iterations and the
// variable, then checks that a wrongly sized u_list[i] throws std::runtime_error.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <stdexcept>

#include <nmpc_amd/FmpcSolverBatch.hpp>
#include <nmpc_amd/models/FmpcVerticalMotion.hpp>

using Solver = nmpc_amd::FmpcSolverBatch<nmpc_amd::FmpcProblemVerticalMotion>;

int main(int argc, char ** argv)
{
  const int T = argc > 1 ? std::atoi(argv[1]) : 50;
  auto problem = std::make_shared<nmpc_amd::FmpcProblemVerticalMotion>();
  const std::vector<double> t0 = {0.0, 1.95, 2.5, 4.45};
  const int B = static_cast<int>(t0.size());
  Solver solver(problem, B, T);
  solver.config().max_iter = 8;
  std::vector<Solver::StateDimVector> x0(B);
  std::vector<Solver::Variable> var(B, Solver::Variable(T));
  for(int b = 0; b < B; b++)
  {
    x0[b][0] = 1.0;
    x0[b][1] = 0.0;
    var[b].reset(1.0, 9.80665, 0.0, 1.0, 1.0);
    for(int i = 0; i < T; i++)
    {
      const double t = t0[b] + i * problem->dt();
      var[b].u_list[i].resize(problem->inputDim(t), 1);
      var[b].u_list[i].setConstant(9.80665);
      var[b].s_list[i].resize(problem->ineqDim(t), 1);
      var[b].s_list[i].setConstant(1.0);
      var[b].nu_list[i].resize(problem->ineqDim(t), 1);
      var[b].nu_list[i].setConstant(1.0);
    }
  }
  const std::vector<Solver::Status> st = solver.solve(t0, x0, var);
  const std::vector<Solver::Variable> out = solver.variable();
  for(int b = 0; b < B; b++)
  {
    std::printf("status %d %d\n", b, static_cast<int>(st[b]));
    for(int i = 0; i < T; i++)
    {
      std::printf("u %d %d %d", b, i, out[b].u_list[i].size());
      for(int e = 0; e < out[b].u_list[i].size(); e++)
      {
        std::printf(" %.17g", out[b].u_list[i][e]);
      }
      std::printf("\n");
    }
    for(int i = 0; i <= T; i++)
    {
      std::printf("x %d %d %.17g %.17g\n", b, i, out[b].x_list[i][0], out[b].x_list[i][1]);
    }
  }
  var[1].u_list[3].resize(var[1].u_list[3].size() == 1 ? 2 : 1, 1); // wrong size at step 3 of instance 1
  try
  {
    solver.solve(t0, x0, var);
    std::printf("no exception\n");
  }
  catch(const std::runtime_error & e)
  {
    std::printf("runtime_error: %s\n", e.what());
  }
  return 0;
}
