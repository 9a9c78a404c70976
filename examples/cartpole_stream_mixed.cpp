// A HETEROGENEOUS queue of cart-pole problems through the slots of ONE solver (nmpc_amd::DDPSolverBatch::solveStream with one problem
// object per instance, plain C++ over nmpc_hip_ddp_solve_stream_ex): every cart-pole has its own pole length, input weight and target
// position — a caller of the reference builds one DDPSolver per problem (DDPSolver.hpp:20-24) and runs them through its cores.  Every
// problem is solved to ITS convergence (DDPSolver.hpp:115-123), the slot of a finished one takes the next of the queue together with
// that one's problem object.  Every instance is checked bit for bit against the same problems solved chunk by chunk with solve() and
// setProblemBatch().
//   g++ -std=c++17 -O2 -Iinclude examples/cartpole_stream_mixed.cpp -Lnmpc_amd/lib -lnmpc_hip_ddp -Wl,-rpath,$PWD/nmpc_amd/lib
//       -o /tmp/cartpole_stream_mixed && /tmp/cartpole_stream_mixed [instances] [slots]
#include <array>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>

#include <nmpc_amd/DDPSolverBatch.hpp>
#include <nmpc_amd/models/CartPole.hpp>

using Problem = nmpc_amd::DDPProblemCartPole;
using Solver = nmpc_amd::DDPSolverBatch<Problem>;

// splitmix64 -> U[0, 1): the generator of nmpc_amd/workloads.py
static double uniform01(unsigned long long & state)
{
  state += 0x9E3779B97F4A7C15ull;
  unsigned long long z = state;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return static_cast<double>(z >> 11) * (1.0 / 9007199254740992.0);
}

int main(int argc, char ** argv)
{
  const int N = argc > 1 ? std::atoi(argv[1]) : 600;
  const int S = argc > 2 ? std::atoi(argv[2]) : 256;
  const int T = 100;
  auto problem = std::make_shared<Problem>(0.01);
  std::vector<double> t(N, 0.0);
  std::vector<Problem::StateDimVector> x(N);
  Problem::InputDimVector zero;
  zero.setZero();
  std::vector<std::vector<Problem::InputDimVector>> u(N, std::vector<Problem::InputDimVector>(T, zero));
  std::vector<Problem> problems(N, *problem);
  unsigned long long seed = 4321;
  const double lo[4] = {-1.0, -M_PI, -1.0, -1.0}, hi[4] = {1.0, M_PI, 1.0, 1.0};
  for(int i = 0; i < N; i++)
  {
    for(int j = 0; j < 4; j++)
    {
      x[i][j] = lo[j] + (hi[j] - lo[j]) * uniform01(seed);
    }
    problems[i].param_.pole_length = 1.5 + uniform01(seed); // [m]
    problems[i].cost_weight_.running_u[0] = 0.0005 + 0.0195 * uniform01(seed);
    problems[i].ref_pos_ = -1.0 + 2.0 * uniform01(seed); // [m]
  }

  Solver solver(problem, S);
  solver.config().horizon_steps = T;
  solver.config().print_level = 0;
  solver.config().max_iter = 40;
  solver.config().trace_level = 0;
  solver.setKernel("quad");
  const auto r = solver.solveStream(t, x, u, problems, {}, 4);

  Solver lone(problem, S);
  lone.config() = solver.config();
  lone.config().ragged_schedule = -1;
  lone.setKernel("quad");
  int bad = 0, moved = 0;
  long long its = 0;
  for(int base = 0; base < N; base += S)
  {
    // (the last chunk is padded with copies of its first instance: solve() takes whole batches)
    std::vector<double> tc(S, 0.0);
    std::vector<Problem::StateDimVector> xc(S);
    std::vector<std::vector<Problem::InputDimVector>> uc(S, std::vector<Problem::InputDimVector>(T, zero));
    std::vector<Problem> pc(S, *problem);
    for(int k = 0; k < S; k++)
    {
      xc[k] = x[base + k < N ? base + k : base];
      pc[k] = problems[base + k < N ? base + k : base];
    }
    lone.setProblemBatch(pc);
    lone.solve(tc, xc, uc);
    for(int k = 0; k < S && base + k < N; k++)
    {
      const auto & a = r.control_data[base + k];
      const auto & b = lone.controlData(k);
      bool same = r.status[base + k] == lone.status(k) && std::memcmp(a.cost_list.data(), b.cost_list.data(), a.cost_list.size() * sizeof(double)) == 0;
      for(size_t i = 0; same && i < a.x_list.size(); i++)
      {
        for(int j = 0; j < 4; j++)
        {
          same = same && std::memcmp(&a.x_list[i][j], &b.x_list[i][j], sizeof(double)) == 0;
        }
      }
      for(size_t i = 0; same && i < a.u_list.size(); i++)
      {
        same = same && std::memcmp(&a.u_list[i][0], &b.u_list[i][0], sizeof(double)) == 0;
      }
      bad += same ? 0 : 1;
      its += r.iters[base + k];
    }
  }
  // ... and the problem objects reached the kernel: the same queue on the shared problem gives other trajectories
  const auto shared = solver.solveStream(t, x, u, 4);
  for(int i = 0; i < N; i++)
  {
    double d = 0;
    for(int k = 0; k < T; k++)
    {
      d = std::fmax(d, std::fabs(r.control_data[i].u_list[k][0] - shared.control_data[i].u_list[k][0]));
    }
    moved += d > 1e-3 ? 1 : 0;
  }
  std::printf("%d cart-poles with their own pole length, input weight and target through %d slots: %d rounds, %.2f ms on the device, %lld "
              "instance-iterations, instances differing from their lone solves: %d, from the shared problem's solution: %d\n",
              N, S, r.rounds, r.device_ms, its, bad, moved);
  const bool ok = bad == 0 && 2 * moved >= N;
  std::printf(ok ? "STREAM_MIXED_OK\n" : "STREAM_MIXED_BAD\n");
  return ok ? 0 : 1;
}
