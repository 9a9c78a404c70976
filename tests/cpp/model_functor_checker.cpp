// Host evaluation of the shipped DDP problem functors (include/nmpc_amd/models/*.hpp, compiled with plain g++: NMPC_HD is `inline`
// there) and of the test-only BoxQP probe (boxqp_probe.hpp), behind a small C ABI for tests/test_model_functors_cpu.py.  The same
// statements run on the device; here they are checked against finite differences, the oracle's separately written functors and
// their fp32 twins.  Built by the tests into a temporary directory, never into the tree.
#include <cstddef>
#include <cstring>
#include <new>

#include <nmpc_amd/models/Bipedal.hpp>
#include <nmpc_amd/models/CartPole.hpp>
#include <nmpc_amd/models/CentroidalMotion.hpp>
#include <nmpc_amd/models/Manipulator.hpp>
#include <nmpc_amd/models/PlanarVtol.hpp>
#include <nmpc_amd/models/Quadrotor.hpp>
#include <nmpc_amd/models/VerticalMotion.hpp>

#include "boxqp_probe.hpp"

namespace
{
using namespace nmpc_amd;

struct ProbeD4M2 : test::BoxQPProbe<double, 4, 2>
{
};
struct ProbeD9Dyn16 : test::BoxQPProbe<double, 9, Dynamic, 16>
{
};
struct ProbeF4M2 : test::BoxQPProbe<float, 4, 2>
{
};

/** Every output of one evaluation at (t, x, u), in double, matrices row-major with their run-time extents:
    Fx (n, n), Fu (n, m), Lxx (n, n), Luu (m, m), Lxu (n, m), Vxx (n, n). */
struct Out
{
  int m;
  double * xn;
  double * L;
  double * phi;
  double * Fx;
  double * Fu;
  double * Lx;
  double * Lu;
  double * Lxx;
  double * Luu;
  double * Lxu;
  double * Vx;
  double * Vxx;
};

template<class P>
int eval(const void * params, double t_in, const double * x_in, const double * u_in, Out & o)
{
  using R = typename P::Scalar;
  constexpr int N = P::kStateDim, MM = P::kInputDimMax;
  P p;
  if(params)
  {
    std::memcpy(static_cast<void *>(&p), params, sizeof(P));
  }
  const R t = static_cast<R>(t_in);
  int m = MM;
  if constexpr(P::kDynamicInput)
  {
    m = p.inputDim(t);
  }
  typename P::StateDimVector x;
  typename P::InputDimVector u;
  u.setZero();
  if constexpr(P::kDynamicInput)
  {
    u.resize(m);
  }
  for(int i = 0; i < N; i++)
  {
    x[i] = static_cast<R>(x_in[i]);
  }
  for(int a = 0; a < m; a++)
  {
    u[a] = static_cast<R>(u_in[a]);
  }
  typename P::StateStateDimMatrix Fx, Lxx, Vxx;
  typename P::StateInputDimMatrix Fu, Lxu;
  typename P::StateDimVector Lx, Vx;
  typename P::InputDimVector Lu;
  typename P::InputInputDimMatrix Luu;
  Fx.setZero();
  Lxx.setZero();
  Vxx.setZero();
  Fu.setZero();
  Lxu.setZero();
  Lx.setZero();
  Vx.setZero();
  Lu.setZero();
  Luu.setZero();
  if constexpr(P::kDynamicInput)
  {
    Fu.resize(N, m);
    Lxu.resize(N, m);
    Lu.resize(m);
    Luu.resize(m, m);
  }
  const typename P::StateDimVector xn = p.stateEq(t, x, u);
  p.calcStateEqDeriv(t, x, u, Fx, Fu);
  p.calcRunningCostDeriv(t, x, u, Lx, Lu, Lxx, Luu, Lxu);
  p.calcTerminalCostDeriv(t, x, Vx, Vxx);
  o.m = m;
  *o.L = static_cast<double>(p.runningCost(t, x, u));
  *o.phi = static_cast<double>(p.terminalCost(t, x));
  for(int i = 0; i < N; i++)
  {
    o.xn[i] = xn[i];
    o.Lx[i] = Lx[i];
    o.Vx[i] = Vx[i];
    for(int j = 0; j < N; j++)
    {
      o.Fx[i * N + j] = Fx(i, j);
      o.Lxx[i * N + j] = Lxx(i, j);
      o.Vxx[i * N + j] = Vxx(i, j);
    }
    for(int a = 0; a < m; a++)
    {
      o.Fu[i * m + a] = Fu(i, a);
      o.Lxu[i * m + a] = Lxu(i, a);
    }
  }
  for(int a = 0; a < m; a++)
  {
    o.Lu[a] = Lu[a];
    for(int b = 0; b < m; b++)
    {
      o.Luu[a * m + b] = Luu(a, b);
    }
  }
  return 0;
}

struct Entry
{
  const char * name;
  int n, m_max, dynamic, scalar_bytes;
  size_t param_bytes;
  int (*eval)(const void *, double, const double *, const double *, Out &);
  void (*defaults)(void *);
};

template<class P>
void defaults(void * out)
{
  new(out) P();
}

template<class P>
constexpr Entry entry(const char * name)
{
  return {name, P::kStateDim, P::kInputDimMax, P::kDynamicInput ? 1 : 0, static_cast<int>(sizeof(typename P::Scalar)), sizeof(P),
          &eval<P>, &defaults<P>};
}

const Entry kEntries[] = {
    entry<DDPProblemCartPole>("cartpole"),
    entry<DDPProblemBipedal>("bipedal"),
    entry<DDPProblemVerticalMotion>("vertical"),
    entry<DDPProblemCentroidalMotion>("centroidal"),
    entry<DDPProblemQuadrotor>("quadrotor"),
    entry<DDPProblemManipulator>("manipulator"),
    entry<DDPProblemPlanarVtol>("planar_vtol"),
    entry<DDPProblemCartPoleF32>("cartpole_f32"),
    entry<DDPProblemQuadrotorF32>("quadrotor_f32"),
    entry<DDPProblemManipulatorF32>("manipulator_f32"),
    entry<ProbeD4M2>("boxqp_probe_d4m2"),
    entry<ProbeD9Dyn16>("boxqp_probe_d9dyn16"),
    entry<ProbeF4M2>("boxqp_probe_f4m2"),
};

const Entry * find(const char * name)
{
  for(const Entry & e : kEntries)
  {
    if(std::strcmp(e.name, name) == 0)
    {
      return &e;
    }
  }
  return nullptr;
}
} // namespace

extern "C"
{
  int mfc_info(const char * name, int * n, int * m_max, int * dynamic, int * scalar_bytes, size_t * param_bytes)
  {
    const Entry * e = find(name);
    if(!e)
    {
      return -1;
    }
    *n = e->n;
    *m_max = e->m_max;
    *dynamic = e->dynamic;
    *scalar_bytes = e->scalar_bytes;
    *param_bytes = e->param_bytes;
    return 0;
  }

  int mfc_default_params(const char * name, void * out, size_t bytes)
  {
    const Entry * e = find(name);
    if(!e || bytes != e->param_bytes)
    {
      return -1;
    }
    e->defaults(out);
    return 0;
  }

  //! params: a problem object's memory image (NULL: the default object); u holds m_max entries
  int mfc_eval(const char * name,
               const void * params,
               double t,
               const double * x,
               const double * u,
               int * m,
               double * xn,
               double * L,
               double * phi,
               double * Fx,
               double * Fu,
               double * Lx,
               double * Lu,
               double * Lxx,
               double * Luu,
               double * Lxu,
               double * Vx,
               double * Vxx)
  {
    const Entry * e = find(name);
    if(!e)
    {
      return -1;
    }
    Out o{0, xn, L, phi, Fx, Fu, Lx, Lu, Lxx, Luu, Lxu, Vx, Vxx};
    const int rc = e->eval(params, t, x, u, o);
    *m = o.m;
    return rc;
  }
}
