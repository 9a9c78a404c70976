// Test program of tests/test_boxqp_host_cpu.py: nmpc_amd::BoxQPBatch (include/nmpc_amd/BoxQPBatch.hpp) compiled by a host compiler
// alone, with a fixed and a run-time var_dim.  With a gfx950 device it solves the reference's five known answers
// (TestBoxQP.cpp:35-98) and prints them; without one, create() throws std::runtime_error and the program says so.
#include <cmath>
#include <cstdio>
#include <stdexcept>
#include <vector>

#include <nmpc_amd/BoxQPBatch.hpp>

template<class Solver>
int run(Solver & qp)
{
  const int B = 5;
  std::vector<double> H;
  for(int b = 0; b < B; b++)
  {
    H.insert(H.end(), {1.0, 0.0, 0.0, 0.5});
  }
  const std::vector<double> g = {1.5, 1.0, 1.5, 1.0, 1.0, 1.5, 1.5, 1.0, 1.0, 1.5};
  const std::vector<double> lower = {-10, -10, 0.5, -2, 0, -1, -5, -1, -5, -10};
  const std::vector<double> upper = {10, 10, 5, 2, 5, -0.5, -2, 2, -2, 10};
  const std::vector<double> x_gt = {-1.5, -2, 0.5, -2, 0, -1, -2, -1, -2, -3};
  qp.config().print_level = 0;
  qp.config().trace_capacity = 4;
  const std::vector<double> x = qp.solve(H, g, lower, upper);
  int bad = 0;
  for(int b = 0; b < B; b++)
  {
    const double err = std::hypot(x[2 * b] - x_gt[2 * b], x[2 * b + 1] - x_gt[2 * b + 1]);
    std::printf("qp %d x %.17g %.17g retval %d (%s) free %zu trace %zu\n", b, qp.x(b)[0], qp.x(b)[1], qp.retval(b), qp.retstr(b).c_str(),
                qp.freeIdxs(b).size(), qp.traceDataList(b).size());
    bad += !(err < 1e-6) || qp.retval(b) <= 0;
  }
  return bad;
}

int main()
{
  try
  {
    nmpc_amd::BoxQPBatch<2> fixed(5);
    nmpc_amd::BoxQPBatch<nmpc_amd::Dynamic> dynamic(5, 2);
    dynamic.setKernel("wave");
    const int bad = run(fixed) + run(dynamic);
    std::printf("%s %s %s\n", bad ? "FAILED" : "ok", fixed.kernelName().c_str(), dynamic.kernelName().c_str());
    return bad ? 1 : 0;
  }
  catch(const std::invalid_argument & e)
  {
    std::printf("invalid_argument: %s\n", e.what());
    return 2;
  }
  catch(const std::runtime_error & e)
  {
    std::printf("runtime_error: %s\n", e.what());
    return 0;
  }
}
