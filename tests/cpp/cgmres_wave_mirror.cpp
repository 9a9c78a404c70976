// The C++ mirror's kernel choice (include/nmpc_amd/CgmresSolverBatch.hpp: setKernel / kernelName) from plain C++17 (g++, no HIP):
// 8 bounded cart-poles through 0.05 s on the lane kernel and on the wave kernel; exits 0 when the names are right, an unknown kernel
// is refused and the two runs end in the same bits.  Compiled by tests/test_cgmres_wave_host_cpu.py, run by
// tests/test_gpu_cgmres_wave.py.
#include <cstdio>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <vector>

#include <nmpc_amd/CgmresSolverBatch.hpp>
#include <nmpc_amd/models/CgmresCartPole.hpp>

using Problem = nmpc_amd::CgmresProblemCartPoleWithInputBound;
using Solver = nmpc_amd::CgmresSolverBatch<Problem>;

static bool sameBits(const std::vector<double> & a, const std::vector<double> & b)
{
  return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0;
}

int main()
{
  const int B = 8;
  auto problem = std::make_shared<Problem>();
  std::vector<double> x[2], u[2], U[2], dU[2];
  for(int k = 0; k < 2; k++)
  {
    Solver s(problem, B, 25, NMPC_HIP_CGMRES_ODE_EULER, NMPC_HIP_CGMRES_ODE_RUNGE_KUTTA);
    if(s.kernelName() != "cgmres_run_kernel")
    {
      std::printf("default kernel is %s\n", s.kernelName().c_str());
      return 1;
    }
    bool refused = false;
    try
    {
      s.setKernel("nope");
    }
    catch(const std::invalid_argument &)
    {
      refused = true;
    }
    if(!refused)
    {
      std::printf("an unknown kernel was accepted\n");
      return 1;
    }
    s.setKernel(k == 0 ? "lane" : "wave");
    if(s.kernelName() != (k == 0 ? "cgmres_run_kernel" : "cgmres_wave_run_kernel"))
    {
      std::printf("kernel %d is %s\n", k, s.kernelName().c_str());
      return 1;
    }
    for(int b = 0; b < B; b++)
    {
      s.x_initial_[b][1] += 0.01 * b;
    }
    s.sim_duration_ = 0.05;
    s.dump_step_ = 0;
    s.run();
    x[k] = s.x();
    u[k] = s.u();
    U[k] = s.uList();
    dU[k] = s.deltaUVec();
  }
  const bool same = sameBits(x[0], x[1]) && sameBits(u[0], u[1]) && sameBits(U[0], U[1]) && sameBits(dU[0], dU[1]);
  std::printf("wave %s lane\n", same ? "==" : "!=");
  return same ? 0 : 1;
}
