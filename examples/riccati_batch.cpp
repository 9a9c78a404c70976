// A batch of finite-horizon LQR problems through nmpc_amd::RiccatiBatch: the derivative blocks are written down by hand (no problem
// class is compiled in), the backward pass runs on the device, and the gains of instance 0 are held against the textbook Riccati
// recursion computed here.  Instance b is a double integrator with time step dt and input weight r_b = 0.01 (1 + b).
//
//   g++ -std=c++17 -O2 -Iinclude examples/riccati_batch.cpp -Lnmpc_amd/lib -lnmpc_hip_ddp -Wl,-rpath,$PWD/nmpc_amd/lib -o riccati_batch
//   ./riccati_batch [batch] [horizon_steps]
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <vector>

#include <nmpc_amd/RiccatiBatch.hpp>

int main(int argc, char ** argv)
{
  const int B = argc > 1 ? std::atoi(argv[1]) : 8, T = argc > 2 ? std::atoi(argv[2]) : 50;
  const int n = 2, m = 1;
  const double dt = 0.05;
  if(B < 1 || T < 1)
  {
    std::fprintf(stderr, "usage: %s [batch >= 1] [horizon_steps >= 1]\n", argv[0]);
    return 2;
  }
  try
  {
    nmpc_amd::RiccatiBatch solver(n, m, T, B);
    solver.config().lambda = 0.0; // an LQ problem needs no regularisation
    nmpc_amd::RiccatiBatch::Derivatives d;
    const size_t S = static_cast<size_t>(B) * T;
    d.Fx.assign(S * n * n, 0.0);
    d.Fu.assign(S * n * m, 0.0);
    d.Lx.assign(S * n, 0.0);
    d.Lu.assign(S * m, 0.0);
    d.Lxx.assign(S * n * n, 0.0);
    d.Luu.assign(S * m * m, 0.0);
    d.Lxu.assign(S * n * m, 0.0);
    d.Vx_T.assign(static_cast<size_t>(B) * n, 0.0);
    d.Vxx_T.assign(static_cast<size_t>(B) * n * n, 0.0);
    for(int b = 0; b < B; b++)
    {
      for(int i = 0; i < T; i++)
      {
        const size_t s = static_cast<size_t>(b) * T + i;
        double * Fx = &d.Fx[s * 4]; // column-major: (r, c) at r + 2 c
        Fx[0] = 1, Fx[2] = dt, Fx[3] = 1;
        d.Fu[s * 2 + 0] = 0.5 * dt * dt;
        d.Fu[s * 2 + 1] = dt;
        d.Lxx[s * 4 + 0] = dt; // running cost dt/2 (x' x + r u^2) about the origin
        d.Lxx[s * 4 + 3] = dt;
        d.Luu[s] = dt * 0.01 * (1 + b);
      }
      d.Vxx_T[static_cast<size_t>(b) * 4 + 0] = 10; // terminal cost 5 x' x
      d.Vxx_T[static_cast<size_t>(b) * 4 + 3] = 10;
    }
    const nmpc_amd::RiccatiBatch::Result r = solver.backward(d);

    // P <- Q + A' P A - A' P B (R + B' P B)^-1 B' P A for instance 0, and its first gain
    double P[2][2] = {{10, 0}, {0, 10}}, K0[2] = {0, 0};
    const double A[2][2] = {{1, dt}, {0, 1}}, Bm[2] = {0.5 * dt * dt, dt}, R = dt * 0.01;
    for(int i = T - 1; i >= 0; i--)
    {
      double PA[2][2], PB[2], AtPA[2][2], AtPB[2];
      for(int a = 0; a < 2; a++)
      {
        PB[a] = P[a][0] * Bm[0] + P[a][1] * Bm[1];
        for(int c = 0; c < 2; c++)
        {
          PA[a][c] = P[a][0] * A[0][c] + P[a][1] * A[1][c];
        }
      }
      const double BtPB = Bm[0] * PB[0] + Bm[1] * PB[1];
      for(int a = 0; a < 2; a++)
      {
        AtPB[a] = A[0][a] * PB[0] + A[1][a] * PB[1];
        for(int c = 0; c < 2; c++)
        {
          AtPA[a][c] = A[0][a] * PA[0][c] + A[1][a] * PA[1][c];
        }
      }
      for(int a = 0; a < 2; a++)
      {
        K0[a] = -AtPB[a] / (R + BtPB);
        for(int c = 0; c < 2; c++)
        {
          P[a][c] = (a == c ? dt : 0.0) + AtPA[a][c] - AtPB[a] * AtPB[c] / (R + BtPB);
        }
      }
    }
    double err = 0;
    for(int c = 0; c < 2; c++)
    {
      err = std::fmax(err, std::fabs(r.K[c] - K0[c])); // K of (b = 0, i = 0): 1 x 2
      for(int a = 0; a < 2; a++)
      {
        err = std::fmax(err, std::fabs(r.Vxx0[a + 2 * c] - P[a][c]));
      }
    }
    std::printf("kernel %s, %.3f ms for %d instances x %d steps\n", solver.kernelName().c_str(), solver.lastMs(), B, T);
    std::printf("instance 0: K_0 = [%.6f %.6f], LQR recursion [%.6f %.6f], status %d, passes %d\n", r.K[0], r.K[1], K0[0], K0[1], r.status[0],
                r.n_backward[0]);
    std::printf("instance %d: K_0 = [%.6f %.6f]\n", B - 1, r.K[static_cast<size_t>(B - 1) * T * 2], r.K[static_cast<size_t>(B - 1) * T * 2 + 1]);
    const bool ok = err < 1e-9 && r.status[0] == NMPC_HIP_RICCATI_OK;
    std::printf(ok ? "ok riccati_wave_kernel (max |gain, Vxx - LQR| = %.2e)\n" : "FAILED (%.2e)\n", err);
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
