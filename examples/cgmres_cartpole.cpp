// A fleet of cart-poles, each swung up by its own C/GMRES controller, ticked from the host at dt through the device entry point
// nmpc_hip_cgmres_control_input_device: the plant (RK4, as the reference's test simulates it, nmpc_cgmres/tests/src/
// TestCgmresSolver.cpp) runs on the host, the B measured states go to the device, the B inputs come back, once per tick.  Host code
// only (g++, no HIP kernels of its own): the problem type is already compiled into libnmpc_hip_ddp.so.  Prints how many cart-poles
// are upright (|x| < 0.1) at the end; exits non-zero if a state became non-finite.
//
//   g++ -std=c++17 -O2 -Iinclude -I/opt/rocm/include -D__HIP_PLATFORM_AMD__ examples/cgmres_cartpole.cpp -Lnmpc_amd/lib
//       -lnmpc_hip_ddp -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,$PWD/nmpc_amd/lib -o cgmres_cartpole
//   ./cgmres_cartpole [batch=256] [seconds=20] [--kernel lane|wave]
//
// --kernel wave ticks every controller on a wavefront of its own with the horizon in LDS (the low-latency kernel for fleets of up
// to a few thousand; the same inputs bit for bit); the default is the lane kernel (one lane per controller).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include <nmpc_amd/CgmresSolverBatch.hpp>
#include <nmpc_amd/models/CgmresCartPole.hpp>

using Problem = nmpc_amd::CgmresProblemCartPoleWithInputBound;
using Solver = nmpc_amd::CgmresSolverBatch<Problem>;

#define HIP_OK(expr)                                                  \
  do                                                                  \
  {                                                                   \
    if((expr) != hipSuccess)                                          \
    {                                                                 \
      std::fprintf(stderr, "%s failed\n", #expr);                     \
      return 2;                                                       \
    }                                                                 \
  } while(0)

int main(int argc, char ** argv)
{
  const char * kernel = "lane";
  std::vector<const char *> pos;
  for(int i = 1; i < argc; i++)
  {
    if(std::strcmp(argv[i], "--kernel") == 0 && i + 1 < argc)
    {
      kernel = argv[++i];
    }
    else
    {
      pos.push_back(argv[i]);
    }
  }
  const int B = pos.size() > 0 ? std::atoi(pos[0]) : 256;
  const double seconds = pos.size() > 1 ? std::atof(pos[1]) : 20.0;
  constexpr int NX = Problem::dim_x_, NUC = Problem::dim_uc_;
  auto problem = std::make_shared<Problem>();
  Solver solver(problem, B, 25, NMPC_HIP_CGMRES_ODE_EULER);
  for(int b = 0; b < B; b++)
  {
    solver.x_initial_[b][1] += 0.02 * (b % 16) / 16.0 - 0.01; // a spread of pole angles around hanging down
  }
  solver.setKernel(kernel); // throws std::invalid_argument for an unknown name or a shape past the wave kernel's LDS budget
  solver.setup();
  std::vector<double> t(B), x(B * NX), next_x(B * NX), u(B * NUC);
  for(int b = 0; b < B; b++)
  {
    for(int a = 0; a < NX; a++)
    {
      x[b * NX + a] = solver.x_initial_[b][a];
    }
    for(int j = 0; j < NUC; j++)
    {
      u[b * NUC + j] = solver.u_initial_[b][j];
    }
  }
  double *d_t, *d_x, *d_nx, *d_u;
  HIP_OK(hipMalloc(&d_t, B * sizeof(double)));
  HIP_OK(hipMalloc(&d_x, B * NX * sizeof(double)));
  HIP_OK(hipMalloc(&d_nx, B * NX * sizeof(double)));
  HIP_OK(hipMalloc(&d_u, B * NUC * sizeof(double)));
  const double dt = solver.dt_;
  auto f = [&](const double * xs, const double * us, double * dx) { problem->stateEquation(0, xs, us, dx); };
  int ticks = 0;
  for(double tt = 0; tt <= seconds; tt += dt, ticks++)
  {
    for(int b = 0; b < B; b++) // the plants: one RK4 step of each cart-pole under its current input
    {
      double k1[NX], k2[NX], k3[NX], k4[NX], y[NX];
      const double * xb = &x[b * NX];
      const double * ub = &u[b * NUC];
      f(xb, ub, k1);
      for(int a = 0; a < NX; a++)
        y[a] = xb[a] + dt / 2 * k1[a];
      f(y, ub, k2);
      for(int a = 0; a < NX; a++)
        y[a] = xb[a] + dt / 2 * k2[a];
      f(y, ub, k3);
      for(int a = 0; a < NX; a++)
        y[a] = xb[a] + dt * k3[a];
      f(y, ub, k4);
      for(int a = 0; a < NX; a++)
        next_x[b * NX + a] = xb[a] + dt / 6 * (((k1[a] + 2 * k2[a]) + 2 * k3[a]) + k4[a]);
      t[b] = tt;
    }
    HIP_OK(hipMemcpy(d_t, t.data(), B * sizeof(double), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_x, x.data(), B * NX * sizeof(double), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_nx, next_x.data(), B * NX * sizeof(double), hipMemcpyHostToDevice));
    solver.calcControlInputDevice(d_t, d_x, d_nx, d_u);
    solver.synchronize();
    HIP_OK(hipMemcpy(u.data(), d_u, B * NUC * sizeof(double), hipMemcpyDeviceToHost));
    x = next_x;
  }
  int upright = 0, non_finite = 0;
  for(int b = 0; b < B; b++)
  {
    double n2 = 0;
    for(int a = 0; a < NX; a++)
      n2 += x[b * NX + a] * x[b * NX + a];
    upright += std::sqrt(n2) < 0.1;
    non_finite += !std::isfinite(n2);
  }
  std::printf("%d cart-poles, %d ticks of %g s on %s: %d upright (|x| < 0.1), %d non-finite\n", B, ticks, dt, solver.kernelName().c_str(),
              upright, non_finite);
  (void)hipFree(d_t);
  (void)hipFree(d_x);
  (void)hipFree(d_nx);
  (void)hipFree(d_u);
  return non_finite ? 1 : 0;
}
