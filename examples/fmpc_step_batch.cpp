// A batch of input-limited double integrators through nmpc_amd::FmpcStepBatch: the linearisation is written down by hand (no problem
// class is compiled in), each interior-point iteration runs on the device, and the host relinearises at the solver's variable until
// every instance reports Succeeded.  Instance b starts at position 1 + 0.1 b and has to come to rest at the origin with |u| <= 2.
//
//   g++ -std=c++17 -O2 -Iinclude examples/fmpc_step_batch.cpp -Lnmpc_amd/lib -lnmpc_hip_ddp -Wl,-rpath,$PWD/nmpc_amd/lib -o fmpc_step_batch
//   ./fmpc_step_batch [batch] [horizon_steps]
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <vector>

#include <nmpc_amd/FmpcStepBatch.hpp>

int main(int argc, char ** argv)
{
  const int B = argc > 1 ? std::atoi(argv[1]) : 8, T = argc > 2 ? std::atoi(argv[2]) : 20;
  const int n = 2, m = 1, g = 2;
  const double dt = 0.05, r_u = 0.01, u_max = 2.0;
  if(B < 1 || T < 1)
  {
    std::fprintf(stderr, "usage: %s [batch >= 1] [horizon_steps >= 1]\n", argv[0]);
    return 2;
  }
  try
  {
    using Solver = nmpc_amd::FmpcStepBatch;
    Solver solver(n, m, g, T, B);
    solver.config().dt = dt;
    solver.config().init_complementary_variable = 1; // the first call sets s and nu from g
    const size_t S = static_cast<size_t>(B) * T, X = static_cast<size_t>(B) * (T + 1) * n;
    Solver::Variable v;
    v.x.assign(X, 0.0);
    v.lambda.assign(X, 0.0);
    v.u.assign(S * m, 0.0);
    v.s.assign(S * g, 1.0);
    v.nu.assign(S * g, 1.0);
    solver.setVariable(v);

    // what does not depend on the variable (column-major blocks: (r, c) at r + rows c)
    Solver::Linearisation l;
    l.A.assign(S * n * n, 0.0);
    l.B.assign(S * n * m, 0.0);
    l.C.assign(S * g * n, 0.0);
    l.D.assign(S * g * m, 0.0);
    l.Lxx.assign(S * n * n, 0.0);
    l.Luu.assign(S * m * m, r_u);
    l.Lxu.assign(S * n * m, 0.0);
    l.Lx.assign(S * n, 0.0);
    l.Lu.assign(S * m, 0.0);
    l.f.assign(S * n, 0.0);
    l.g.assign(S * g, 0.0);
    l.Lx_T.assign(static_cast<size_t>(B) * n, 0.0);
    l.Lxx_T.assign(static_cast<size_t>(B) * n * n, 0.0);
    l.current_x.assign(static_cast<size_t>(B) * n, 0.0);
    for(size_t s = 0; s < S; s++)
    {
      l.A[s * 4 + 0] = 1, l.A[s * 4 + 2] = dt, l.A[s * 4 + 3] = 1;
      l.B[s * 2 + 0] = 0.5 * dt * dt, l.B[s * 2 + 1] = dt;
      l.D[s * 2 + 0] = 1, l.D[s * 2 + 1] = -1; // g = [u - u_max, -u - u_max] <= 0
      l.Lxx[s * 4 + 0] = 1, l.Lxx[s * 4 + 3] = 1; // running cost 1/2 (x' x + r_u u^2), weighted by dt in the solver
    }
    for(int b = 0; b < B; b++)
    {
      l.Lxx_T[static_cast<size_t>(b) * 4 + 0] = 10, l.Lxx_T[static_cast<size_t>(b) * 4 + 3] = 10; // terminal cost 5 x' x
      l.current_x[static_cast<size_t>(b) * 2] = 1.0 + 0.1 * b;
    }

    Solver::Result r;
    int iter = 0;
    bool done = false;
    double ms = 0;
    for(; iter < 60 && !done; iter++)
    {
      v = solver.variable();
      for(int b = 0; b < B; b++)
      {
        for(int i = 0; i < T; i++)
        {
          const size_t s = static_cast<size_t>(b) * T + i;
          const double * x = &v.x[(static_cast<size_t>(b) * (T + 1) + i) * n];
          const double u = v.u[s];
          l.f[s * 2 + 0] = x[0] + dt * x[1] + 0.5 * dt * dt * u;
          l.f[s * 2 + 1] = x[1] + dt * u;
          l.g[s * 2 + 0] = u - u_max;
          l.g[s * 2 + 1] = -u - u_max;
          l.Lx[s * 2 + 0] = x[0], l.Lx[s * 2 + 1] = x[1];
          l.Lu[s] = r_u * u;
        }
        const double * xT = &v.x[(static_cast<size_t>(b) * (T + 1) + T) * n];
        l.Lx_T[static_cast<size_t>(b) * 2 + 0] = 10 * xT[0], l.Lx_T[static_cast<size_t>(b) * 2 + 1] = 10 * xT[1];
      }
      r = solver.step(l);
      ms += solver.lastMs();
      solver.config().init_complementary_variable = 0;
      done = true;
      for(int b = 0; b < B; b++)
      {
        if(r.status[b] != NMPC_HIP_FMPC_STEP_SUCCEEDED && r.status[b] != NMPC_HIP_FMPC_STEP_ITERATION_CONTINUED)
        {
          std::printf("FAILED: instance %d has status %d at iteration %d\n", b, r.status[b], iter + 1);
          return 1;
        }
        done = done && r.status[b] == NMPC_HIP_FMPC_STEP_SUCCEEDED;
      }
    }
    v = solver.variable();
    double u_abs = 0, kkt = 0;
    for(size_t s = 0; s < S; s++)
    {
      u_abs = std::fmax(u_abs, std::fabs(v.u[s]));
    }
    for(int b = 0; b < B; b++)
    {
      kkt = std::fmax(kkt, r.kkt_error[b]);
    }
    std::printf("kernel %s, %d iterations, %.3f ms on the device for %d instances x %d steps\n", solver.kernelName().c_str(), iter, ms, B, T);
    std::printf("instance 0: u_0 = %.6f, x_T = [%.6f %.6f]; max |u| over the batch %.6f (limit %.1f)\n", v.u[0], v.x[static_cast<size_t>(T) * n],
                v.x[static_cast<size_t>(T) * n + 1], u_abs, u_max);
    const bool ok = done && u_abs <= u_max && kkt <= solver.config().kkt_error_thre;
    std::printf(ok ? "ok fmpc_step_wave_kernel (max KKT error %.2e)\n" : "FAILED (max KKT error %.2e)\n", kkt);
    return ok ? 0 : 1;
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
}
