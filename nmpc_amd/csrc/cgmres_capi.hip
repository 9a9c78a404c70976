// C-ABI of the batched C/GMRES solver (declared in include/nmpc_hip_cgmres.h): handles, device-buffer ownership, layout
// conversion at the boundary and the launch sequence of setup / run / control_input.  No CPU fallback exists: without the HIP
// runtime or a device every entry point that needs the GPU fails loudly.
#include <nmpc_hip_cgmres.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#define NMPC_AMD_CGMRES_COMMON_KERNELS // cgmres_gmres_dense_kernel lives in this translation unit
#include <nmpc_amd/hip/capi_core.hpp>
#include <nmpc_amd/hip/cgmres_kernels.hpp>
#include <nmpc_amd/hip/cgmres_wave_kernels.hpp> // CgmresWaveOps and waveLdsBytes; the wave kernels live in cgmres_wave_models.hip

namespace capi = nmpc_amd::hip::capi;
namespace cg = nmpc_amd::hip::cgmres;
using cg::CgmresBuffers;
using cg::CgmresOps;
using cg::CgmresWaveOps;

namespace
{
struct Family
{
  static constexpr const char * noun = "the C/GMRES solver";
};
constexpr auto fail = capi::fail<Family>;

std::vector<const CgmresOps *> & registry()
{
  static std::vector<const CgmresOps *> r;
  return r;
}

const CgmresOps * findModel(const char * name)
{
  if(!name)
  {
    return nullptr;
  }
  for(const CgmresOps * m : registry())
  {
    if(std::strcmp(m->name, name) == 0)
    {
      return m;
    }
  }
  return nullptr;
}

std::vector<const CgmresWaveOps *> & waveRegistry()
{
  static std::vector<const CgmresWaveOps *> r;
  return r;
}

const CgmresWaveOps * findWaveModel(const char * name)
{
  for(const CgmresWaveOps * m : waveRegistry())
  {
    if(std::strcmp(m->name, name) == 0)
    {
      return m;
    }
  }
  return nullptr;
}

int unknownModel(const char * model)
{
  return fail(NMPC_HIP_ERR_UNKNOWN_MODEL, std::string("unknown C/GMRES problem type: ") + (model ? model : "(null)"));
}

/** [B][E] (boundary) <-> [E][B] (device), on the host. */
void toDevice(const double * src, double * dst, size_t B, size_t E)
{
  for(size_t b = 0; b < B; b++)
  {
    for(size_t e = 0; e < E; e++)
    {
      dst[e * B + b] = src[b * E + e];
    }
  }
}

template<class T>
void toBoundary(const T * src, T * dst, size_t B, size_t E)
{
  for(size_t b = 0; b < B; b++)
  {
    for(size_t e = 0; e < E; e++)
    {
      dst[b * E + e] = src[e * B + b];
    }
  }
}

__global__ void cgmres_fill_kernel(double * p, size_t n, double v)
{
  const size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if(i < n)
  {
    p[i] = v;
  }
}

/** RAII device buffer for the one-shot diagnostics. */
struct DevBuf
{
  void * p = nullptr;
  ~DevBuf()
  {
    if(p)
    {
      (void)hipFree(p);
    }
  }
};
} // namespace

struct nmpc_hip_cgmres_solver
{
  const CgmresOps * ops = nullptr;
  int device = 0;
  nmpc_hip_cgmres_config cfg;
  CgmresBuffers bf;
  std::vector<void *> allocs;
  double * d_x_init = nullptr; // [NX][B]
  double * d_u_init = nullptr; // [NUC][B]
  double * d_ctl = nullptr; // control_input staging: t [B], x [B][NX], next_x [B][NX], u [B][NUC]
  void * d_problems = nullptr;
  void * d_logs = nullptr;
  std::vector<double> log_t;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  float last_ms = 0;
  bool set_up = false;
  const CgmresWaveOps * wave = nullptr; // non-NULL: run / control_input launch the wave kernels
  size_t wave_lds = 0; // their LDS bytes for (N, cfg.k_max)
};

namespace
{
template<class T>
int devAlloc(nmpc_hip_cgmres_solver * h, T ** p, size_t count)
{
  NMPC_CAPI_TRY(hipMalloc(reinterpret_cast<void **>(p), std::max<size_t>(count, 1) * sizeof(T)));
  h->allocs.push_back(*p);
  NMPC_CAPI_TRY(hipMemset(*p, 0, std::max<size_t>(count, 1) * sizeof(T)));
  return NMPC_HIP_OK;
}

int validConfig(const nmpc_hip_cgmres_config & c, int horizon_divide_num)
{
  if(c.horizon_divide_num != horizon_divide_num)
  {
    return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "[C/GMRES] horizon_divide_num is fixed at create()");
  }
  if(!(c.k_max >= 1 && c.k_max <= cg::kMaxKmax))
  {
    return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "[C/GMRES] k_max must be in 1 .. 16");
  }
  if(!(std::isfinite(c.dt) && c.dt > 0 && std::isfinite(c.finite_diff_delta) && c.finite_diff_delta > 0 && std::isfinite(c.sim_duration)
       && std::isfinite(c.steady_horizon_duration) && std::isfinite(c.horizon_increase_ratio) && std::isfinite(c.eq_zeta)))
  {
    return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "[C/GMRES] dt and finite_diff_delta must be positive, every parameter finite");
  }
  if(c.sim_duration / c.dt > 1e8)
  {
    return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "[C/GMRES] sim_duration / dt exceeds 1e8 ticks");
  }
  if(c.dump_step < 0 || c.ticks_per_launch < 0 || (c.ode_solver != 0 && c.ode_solver != 1)
     || (c.sim_ode_solver < -1 || c.sim_ode_solver > 1))
  {
    return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "[C/GMRES] dump_step / ticks_per_launch / ODE solver out of range");
  }
  return NMPC_HIP_OK;
}

/** NMPC_HIP_OK when the wave kernels of problem type m fit the LDS budget at (N, k_max); the refusal names the bytes. */
int waveFits(const CgmresOps * m, int N, int k_max, size_t * bytes)
{
  *bytes = cg::waveLdsBytes(N, m->nx, m->nuc, k_max);
  if(*bytes > cg::kWaveMaxLdsBytes)
  {
    return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, std::string("[C/GMRES] the wave kernel of ") + m->name + " needs " + std::to_string(*bytes)
                                                   + " bytes of LDS at horizon_divide_num = " + std::to_string(N) + ", k_max = "
                                                   + std::to_string(k_max) + "; the budget is " + std::to_string(cg::kWaveMaxLdsBytes)
                                                   + " (use the lane kernel)");
  }
  return NMPC_HIP_OK;
}

hipError_t launchRun(nmpc_hip_cgmres_solver * h, int i0, int n_ticks, double t0)
{
  return h->wave ? h->wave->launch_run(h->bf, i0, n_ticks, t0, h->wave_lds, h->stream)
                 : h->ops->launch_run(h->bf, i0, n_ticks, t0, h->stream);
}

hipError_t launchControlInput(nmpc_hip_cgmres_solver * h, const double * t, const double * x, const double * next_x, double * u,
                              hipStream_t s)
{
  return h->wave ? h->wave->launch_control_input(h->bf, t, x, next_x, u, h->wave_lds, s)
                 : h->ops->launch_control_input(h->bf, t, x, next_x, u, s);
}

void applyConfig(nmpc_hip_cgmres_solver * h)
{
  const nmpc_hip_cgmres_config & c = h->cfg;
  CgmresBuffers & b = h->bf;
  b.k_max = c.k_max;
  b.horizon_solver = c.ode_solver;
  b.sim_solver = c.sim_ode_solver < 0 ? c.ode_solver : c.sim_ode_solver;
  b.dump_step = c.dump_step;
  b.steady_horizon_duration = c.steady_horizon_duration;
  b.horizon_increase_ratio = c.horizon_increase_ratio;
  b.dt = c.dt;
  b.eq_zeta = c.eq_zeta;
  b.finite_diff_delta = c.finite_diff_delta;
}

int launchSetup(nmpc_hip_cgmres_solver * h)
{
  const size_t B = h->bf.B;
  NMPC_CAPI_TRY(hipMemcpyAsync(h->bf.x, h->d_x_init, B * h->ops->nx * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
  NMPC_CAPI_TRY(hipMemcpyAsync(h->bf.u, h->d_u_init, B * h->ops->nuc * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
  NMPC_CAPI_TRY(h->ops->launch_setup(h->bf, h->stream));
  return NMPC_HIP_OK;
}

int finishTimed(nmpc_hip_cgmres_solver * h)
{
  NMPC_CAPI_TRY(hipEventRecord(h->ev1, h->stream));
  NMPC_CAPI_TRY(hipEventSynchronize(h->ev1));
  NMPC_CAPI_TRY(hipEventElapsedTime(&h->last_ms, h->ev0, h->ev1));
  return NMPC_HIP_OK;
}

void freeLogs(nmpc_hip_cgmres_solver * h)
{
  if(h->d_logs)
  {
    (void)hipFree(h->d_logs);
    h->d_logs = nullptr;
  }
  h->bf.log_x = h->bf.log_u = h->bf.log_err = nullptr;
  h->bf.log_iters = h->bf.log_reorth = nullptr;
  h->bf.log_rows = 0;
  h->log_t.clear();
}
} // namespace

extern "C"
{
  int nmpc_hip_cgmres_register_model(const CgmresOps * ops)
  {
    if(!ops || findModel(ops->name))
    {
      return NMPC_HIP_ERR_INVALID_ARGUMENT;
    }
    registry().push_back(ops);
    return NMPC_HIP_OK;
  }

  int nmpc_hip_cgmres_register_wave_model(const CgmresWaveOps * ops)
  {
    if(!ops || !ops->name || findWaveModel(ops->name))
    {
      return NMPC_HIP_ERR_INVALID_ARGUMENT;
    }
    waveRegistry().push_back(ops);
    return NMPC_HIP_OK;
  }

  int nmpc_hip_cgmres_wave_lds_bytes(const char * model, int horizon_divide_num, int k_max, size_t * bytes)
  {
    const CgmresOps * m = findModel(model);
    if(!m)
    {
      return unknownModel(model);
    }
    if(!bytes || horizon_divide_num < 1 || horizon_divide_num > 100000 || k_max < 1 || k_max > cg::kMaxKmax)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "[C/GMRES] wave_lds_bytes: horizon_divide_num >= 1, k_max in 1 .. 16, bytes non-NULL");
    }
    *bytes = cg::waveLdsBytes(horizon_divide_num, m->nx, m->nuc, k_max);
    return NMPC_HIP_OK;
  }

  int nmpc_hip_cgmres_set_kernel(nmpc_hip_cgmres_handle h, const char * kernel)
  {
    if(!h || !kernel)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    }
    if(std::strcmp(kernel, "lane") == 0)
    {
      h->wave = nullptr;
      h->wave_lds = 0;
      return NMPC_HIP_OK;
    }
    if(std::strcmp(kernel, "wave") != 0)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, std::string("[C/GMRES] unknown kernel \"") + kernel + "\": \"lane\" or \"wave\"");
    }
    const CgmresWaveOps * w = findWaveModel(h->ops->name);
    if(!w || w->nx != h->ops->nx || w->nuc != h->ops->nuc)
    {
      size_t bytes = cg::waveLdsBytes(h->bf.N, h->ops->nx, h->ops->nuc, h->cfg.k_max);
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, std::string("[C/GMRES] problem type ") + h->ops->name
                                                     + " has no wave kernels (NMPC_AMD_REGISTER_CGMRES_WAVE_PROBLEM); they would need "
                                                     + std::to_string(bytes) + " bytes of LDS");
    }
    size_t bytes = 0;
    const int rc = waveFits(h->ops, h->bf.N, h->cfg.k_max, &bytes);
    if(rc != NMPC_HIP_OK)
    {
      return rc;
    }
    h->wave = w;
    h->wave_lds = bytes;
    return NMPC_HIP_OK;
  }

  int nmpc_hip_cgmres_kernel_name(nmpc_hip_cgmres_handle h, const char ** name)
  {
    if(!h || !name)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    }
    *name = h->wave ? "cgmres_wave_run_kernel" : "cgmres_run_kernel";
    return NMPC_HIP_OK;
  }

  int nmpc_hip_cgmres_default_config(nmpc_hip_cgmres_config * cfg)
  {
    if(!cfg)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "cfg is NULL");
    }
    cfg->sim_duration = 10;
    cfg->steady_horizon_duration = 1.0;
    cfg->horizon_divide_num = 25;
    cfg->horizon_increase_ratio = 0.5;
    cfg->dt = 0.001;
    cfg->eq_zeta = 1000.0;
    cfg->k_max = 5;
    cfg->finite_diff_delta = 0.002;
    cfg->dump_step = 5;
    cfg->ode_solver = NMPC_HIP_CGMRES_ODE_EULER;
    cfg->sim_ode_solver = -1;
    cfg->ticks_per_launch = 0;
    return NMPC_HIP_OK;
  }

  int nmpc_hip_cgmres_model_count(void)
  {
    return static_cast<int>(registry().size());
  }

  int nmpc_hip_cgmres_model_name(int index, const char ** name)
  {
    if(index < 0 || index >= static_cast<int>(registry().size()) || !name)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "model index out of range");
    }
    *name = registry()[index]->name;
    return NMPC_HIP_OK;
  }

  int nmpc_hip_cgmres_model_info(const char * model, int * dim_x, int * dim_u, int * dim_c, size_t * param_bytes, double * x_initial,
                                 double * u_initial)
  {
    const CgmresOps * m = findModel(model);
    if(!m)
    {
      return unknownModel(model);
    }
    if(dim_x)
    {
      *dim_x = m->nx;
    }
    if(dim_u)
    {
      *dim_u = m->nu;
    }
    if(dim_c)
    {
      *dim_c = m->nc;
    }
    if(param_bytes)
    {
      *param_bytes = m->param_bytes;
    }
    if(x_initial || u_initial)
    {
      std::vector<double> x(m->nx), u(m->nuc);
      m->initial(x.data(), u.data());
      if(x_initial)
      {
        std::copy(x.begin(), x.end(), x_initial);
      }
      if(u_initial)
      {
        std::copy(u.begin(), u.end(), u_initial);
      }
    }
    return NMPC_HIP_OK;
  }

  int nmpc_hip_cgmres_model_default_params(const char * model, void * out, size_t bytes)
  {
    const CgmresOps * m = findModel(model);
    if(!m)
    {
      return unknownModel(model);
    }
    if(!out || bytes != m->param_bytes)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "param blob size mismatch");
    }
    m->default_params(out);
    return NMPC_HIP_OK;
  }

  int nmpc_hip_cgmres_destroy(nmpc_hip_cgmres_handle h)
  {
    if(!h)
    {
      return NMPC_HIP_OK;
    }
    (void)hipSetDevice(h->device);
    if(h->stream)
    {
      (void)hipStreamSynchronize(h->stream);
    }
    freeLogs(h);
    for(void * p : h->allocs)
    {
      (void)hipFree(p);
    }
    if(h->d_problems)
    {
      (void)hipFree(h->d_problems);
    }
    if(h->ev0)
    {
      (void)hipEventDestroy(h->ev0);
    }
    if(h->ev1)
    {
      (void)hipEventDestroy(h->ev1);
    }
    if(h->stream)
    {
      (void)hipStreamDestroy(h->stream);
    }
    delete h;
    return NMPC_HIP_OK;
  }

  int nmpc_hip_cgmres_create(const char * model, int horizon_divide_num, int batch, int device, nmpc_hip_cgmres_handle * out)
  {
    if(!out)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "out is NULL");
    }
    *out = nullptr;
    const CgmresOps * m = findModel(model);
    if(!m)
    {
      return unknownModel(model);
    }
    if(horizon_divide_num < 1 || batch < 1 || horizon_divide_num > 100000)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "[C/GMRES] horizon_divide_num and batch must be positive");
    }
    NMPC_CAPI_CHECK(capi::checkDevice<Family>(device));
    auto * h = new nmpc_hip_cgmres_solver();
    h->ops = m;
    h->device = device;
    nmpc_hip_cgmres_default_config(&h->cfg);
    h->cfg.horizon_divide_num = horizon_divide_num;
    CgmresBuffers & b = h->bf;
    b.B = batch;
    b.N = horizon_divide_num;
    b.nx = m->nx;
    b.nuc = m->nuc;
    applyConfig(h);
    const size_t B = batch, N = horizon_divide_num, NX = m->nx, NUC = m->nuc, n = N * NUC;
    int rc = NMPC_HIP_OK;
    auto A = [&](auto ** p, size_t count) {
      if(rc == NMPC_HIP_OK)
      {
        rc = devAlloc(h, p, count);
      }
    };
    A(&b.x, NX * B);
    A(&b.u, NUC * B);
    A(&b.U, n * B);
    A(&b.DhDu, n * B);
    A(&b.DhDu_wd, n * B);
    A(&b.du, n * B);
    A(&b.xlist, (N + 1) * NX * B);
    A(&b.ws, cg::gmresWorkspaceElems(static_cast<int>(n), cg::kMaxKmax) * B);
    A(&b.status, B);
    A(&b.err, B);
    A(&b.iters, B);
    A(&b.reorth, B);
    A(&h->d_x_init, NX * B);
    A(&h->d_u_init, NUC * B);
    A(&h->d_ctl, (1 + 2 * NX + NUC) * B);
    auto cleanup = [&](int code) {
      nmpc_hip_cgmres_destroy(h);
      return code;
    };
    if(rc != NMPC_HIP_OK)
    {
      return cleanup(rc);
    }
    if(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess || hipEventCreate(&h->ev0) != hipSuccess
       || hipEventCreate(&h->ev1) != hipSuccess)
    {
      return cleanup(fail(NMPC_HIP_ERR_HIP, "stream / event creation failed"));
    }
    std::vector<unsigned char> prob(m->param_bytes);
    m->default_params(prob.data());
    if(hipMalloc(&h->d_problems, m->param_bytes) != hipSuccess
       || hipMemcpy(h->d_problems, prob.data(), m->param_bytes, hipMemcpyHostToDevice) != hipSuccess)
    {
      return cleanup(fail(NMPC_HIP_ERR_HIP, "problem upload failed"));
    }
    b.problems = h->d_problems;
    b.per_instance = 0;
    std::vector<double> x0(NX), u0(NUC), xb(B * NX), ub(B * NUC), xd(B * NX), ud(B * NUC);
    m->initial(x0.data(), u0.data());
    for(size_t i = 0; i < B; i++)
    {
      std::copy(x0.begin(), x0.end(), xb.begin() + i * NX);
      std::copy(u0.begin(), u0.end(), ub.begin() + i * NUC);
    }
    toDevice(xb.data(), xd.data(), B, NX);
    toDevice(ub.data(), ud.data(), B, NUC);
    if(hipMemcpy(h->d_x_init, xd.data(), xd.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess
       || hipMemcpy(h->d_u_init, ud.data(), ud.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess
       || hipMemcpy(b.x, xd.data(), xd.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess
       || hipMemcpy(b.u, ud.data(), ud.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess || hipDeviceSynchronize() != hipSuccess)
    {
      return cleanup(fail(NMPC_HIP_ERR_HIP, "initial values upload failed"));
    }
    *out = h;
    return NMPC_HIP_OK;
  }

  int nmpc_hip_cgmres_set_config(nmpc_hip_cgmres_handle h, const nmpc_hip_cgmres_config * cfg)
  {
    if(!h || !cfg)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    }
    const int rc = validConfig(*cfg, h->bf.N);
    if(rc != NMPC_HIP_OK)
    {
      return rc;
    }
    if(h->wave)
    {
      // a k_max past the wave kernel's LDS budget: refused, the config stays as it was
      size_t bytes = 0;
      const int rw = waveFits(h->ops, h->bf.N, cfg->k_max, &bytes);
      if(rw != NMPC_HIP_OK)
      {
        return rw;
      }
      h->wave_lds = bytes;
    }
    h->cfg = *cfg;
    applyConfig(h);
    return NMPC_HIP_OK;
  }

  int nmpc_hip_cgmres_get_config(nmpc_hip_cgmres_handle h, nmpc_hip_cgmres_config * cfg)
  {
    if(!h || !cfg)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    }
    *cfg = h->cfg;
    return NMPC_HIP_OK;
  }

  int nmpc_hip_cgmres_set_problem(nmpc_hip_cgmres_handle h, const void * params, size_t bytes, int per_instance)
  {
    if(!h || !params)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    }
    const size_t want = h->ops->param_bytes * (per_instance ? static_cast<size_t>(h->bf.B) : 1);
    if(bytes != want)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "[C/GMRES] param blob size mismatch (param_bytes, or batch * param_bytes per instance)");
    }
    NMPC_CAPI_TRY(hipSetDevice(h->device));
    NMPC_CAPI_TRY(hipStreamSynchronize(h->stream));
    void * p = nullptr;
    NMPC_CAPI_TRY(hipMalloc(&p, bytes));
    if(hipMemcpy(p, params, bytes, hipMemcpyHostToDevice) != hipSuccess)
    {
      (void)hipFree(p);
      return fail(NMPC_HIP_ERR_HIP, "problem upload failed");
    }
    (void)hipFree(h->d_problems);
    h->d_problems = p;
    h->bf.problems = p;
    h->bf.per_instance = per_instance ? 1 : 0;
    return NMPC_HIP_OK;
  }

  int nmpc_hip_cgmres_set_initial(nmpc_hip_cgmres_handle h, const double * x, const double * u)
  {
    if(!h)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "NULL handle");
    }
    NMPC_CAPI_TRY(hipSetDevice(h->device));
    NMPC_CAPI_TRY(hipStreamSynchronize(h->stream));
    const size_t B = h->bf.B;
    for(int k = 0; k < 2; k++)
    {
      const double * src = k == 0 ? x : u;
      if(!src)
      {
        continue;
      }
      const size_t E = k == 0 ? h->ops->nx : h->ops->nuc;
      std::vector<double> d(B * E);
      toDevice(src, d.data(), B, E);
      NMPC_CAPI_TRY(hipMemcpy(k == 0 ? h->d_x_init : h->d_u_init, d.data(), d.size() * sizeof(double), hipMemcpyHostToDevice));
      NMPC_CAPI_TRY(hipMemcpy(k == 0 ? h->bf.x : h->bf.u, d.data(), d.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    return NMPC_HIP_OK;
  }

  int nmpc_hip_cgmres_setup(nmpc_hip_cgmres_handle h)
  {
    if(!h)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "NULL handle");
    }
    NMPC_CAPI_TRY(hipSetDevice(h->device));
    NMPC_CAPI_TRY(hipEventRecord(h->ev0, h->stream));
    const int rc = launchSetup(h);
    if(rc != NMPC_HIP_OK)
    {
      return rc;
    }
    h->set_up = true;
    return finishTimed(h);
  }

  int nmpc_hip_cgmres_run(nmpc_hip_cgmres_handle h)
  {
    if(!h)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "NULL handle");
    }
    NMPC_CAPI_TRY(hipSetDevice(h->device));
    NMPC_CAPI_TRY(hipStreamSynchronize(h->stream));
    // the tick times exactly as `for(double t = 0; t <= sim_duration_; t += dt_)` produces them
    std::vector<double> ts;
    for(double t = 0; t <= h->cfg.sim_duration; t += h->cfg.dt)
    {
      ts.push_back(t);
    }
    const int n_ticks = static_cast<int>(ts.size());
    freeLogs(h);
    CgmresBuffers & b = h->bf;
    const size_t B = b.B, NX = b.nx, NUC = b.nuc;
    if(h->cfg.dump_step > 0 && n_ticks > 0)
    {
      const size_t rows = static_cast<size_t>((n_ticks - 1) / h->cfg.dump_step + 1);
      const size_t doubles = rows * B * (NX + NUC + 1), ints = 2 * rows * B;
      NMPC_CAPI_TRY(hipMalloc(&h->d_logs, doubles * sizeof(double) + ints * sizeof(int)));
      b.log_x = static_cast<double *>(h->d_logs);
      b.log_u = b.log_x + rows * NX * B;
      b.log_err = b.log_u + rows * NUC * B;
      b.log_iters = reinterpret_cast<int *>(b.log_err + rows * B);
      b.log_reorth = b.log_iters + rows * B;
      b.log_rows = static_cast<int>(rows);
      // rows an instance does not reach (it stopped on a non-finite value) read NaN / -1
      hipLaunchKernelGGL(cgmres_fill_kernel, dim3(static_cast<unsigned>((doubles + 255) / 256)), dim3(256), 0, h->stream, b.log_x, doubles,
                         std::nan(""));
      NMPC_CAPI_TRY(hipGetLastError());
      NMPC_CAPI_TRY(hipMemsetAsync(b.log_iters, 0xff, ints * sizeof(int), h->stream));
      for(size_t r = 0; r < rows; r++)
      {
        h->log_t.push_back(ts[r * h->cfg.dump_step]);
      }
    }
    NMPC_CAPI_TRY(hipEventRecord(h->ev0, h->stream));
    int rc = launchSetup(h);
    if(rc != NMPC_HIP_OK)
    {
      return rc;
    }
    h->set_up = true;
    int chunk = h->cfg.ticks_per_launch;
    if(chunk <= 0)
    {
      // at most ~0.5 s of work per launch: a tick takes ~0.95 ms while the batch is at most one wavefront per CU (B <= 16384:
      // 500 ticks ~ 0.48 s), ~2.4 ms at B = 65536 (profiles/r07_cgmres_throughput.json)
      chunk = static_cast<int>(std::max<size_t>(1, 500 * 16384 / std::max<size_t>(B, 16384)));
    }
    for(int i0 = 0; i0 < n_ticks; i0 += chunk)
    {
      NMPC_CAPI_TRY(launchRun(h, i0, std::min(chunk, n_ticks - i0), ts[i0]));
    }
    return finishTimed(h);
  }

  int nmpc_hip_cgmres_control_input_device(nmpc_hip_cgmres_handle h, const double * d_t, const double * d_x, const double * d_next_x,
                                           double * d_u, void * stream)
  {
    if(!h || !d_t || !d_x || !d_next_x || !d_u)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    }
    if(!h->set_up)
    {
      return fail(NMPC_HIP_ERR_NOT_SOLVED, "[C/GMRES] control_input needs setup() first");
    }
    NMPC_CAPI_TRY(hipSetDevice(h->device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : h->stream;
    NMPC_CAPI_TRY(launchControlInput(h, d_t, d_x, d_next_x, d_u, s));
    return NMPC_HIP_OK;
  }

  int nmpc_hip_cgmres_control_input(nmpc_hip_cgmres_handle h, const double * t, const double * x, const double * next_x, double * u)
  {
    if(!h || !t || !x || !next_x || !u)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    }
    if(!h->set_up)
    {
      return fail(NMPC_HIP_ERR_NOT_SOLVED, "[C/GMRES] control_input needs setup() first");
    }
    NMPC_CAPI_TRY(hipSetDevice(h->device));
    const size_t B = h->bf.B, NX = h->ops->nx, NUC = h->ops->nuc;
    double * dt = h->d_ctl;
    double * dx = dt + B;
    double * dnx = dx + B * NX;
    double * du = dnx + B * NX;
    NMPC_CAPI_TRY(hipEventRecord(h->ev0, h->stream));
    NMPC_CAPI_TRY(hipMemcpyAsync(dt, t, B * sizeof(double), hipMemcpyHostToDevice, h->stream));
    NMPC_CAPI_TRY(hipMemcpyAsync(dx, x, B * NX * sizeof(double), hipMemcpyHostToDevice, h->stream));
    NMPC_CAPI_TRY(hipMemcpyAsync(dnx, next_x, B * NX * sizeof(double), hipMemcpyHostToDevice, h->stream));
    NMPC_CAPI_TRY(launchControlInput(h, dt, dx, dnx, du, h->stream));
    NMPC_CAPI_TRY(hipMemcpyAsync(u, du, B * NUC * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    return finishTimed(h);
  }

  int nmpc_hip_cgmres_synchronize(nmpc_hip_cgmres_handle h)
  {
    if(!h)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "NULL handle");
    }
    NMPC_CAPI_TRY(hipSetDevice(h->device));
    NMPC_CAPI_TRY(hipStreamSynchronize(h->stream));
    return NMPC_HIP_OK;
  }

  int nmpc_hip_cgmres_field_bytes(nmpc_hip_cgmres_handle h, int field, size_t * bytes)
  {
    if(!h || !bytes)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    }
    const size_t B = h->bf.B, NX = h->ops->nx, NUC = h->ops->nuc, n = static_cast<size_t>(h->bf.N) * NUC, L = h->bf.log_rows;
    switch(field)
    {
      case NMPC_HIP_CGMRES_FIELD_X: *bytes = B * NX * sizeof(double); break;
      case NMPC_HIP_CGMRES_FIELD_U: *bytes = B * NUC * sizeof(double); break;
      case NMPC_HIP_CGMRES_FIELD_U_LIST:
      case NMPC_HIP_CGMRES_FIELD_DELTA_U: *bytes = B * n * sizeof(double); break;
      case NMPC_HIP_CGMRES_FIELD_STATUS: *bytes = B * sizeof(int); break;
      case NMPC_HIP_CGMRES_FIELD_ERR: *bytes = B * sizeof(double); break;
      case NMPC_HIP_CGMRES_FIELD_LOG_T: *bytes = L * sizeof(double); break;
      case NMPC_HIP_CGMRES_FIELD_LOG_X: *bytes = B * L * NX * sizeof(double); break;
      case NMPC_HIP_CGMRES_FIELD_LOG_U: *bytes = B * L * NUC * sizeof(double); break;
      case NMPC_HIP_CGMRES_FIELD_LOG_ERR: *bytes = B * L * sizeof(double); break;
      case NMPC_HIP_CGMRES_FIELD_LOG_ITERS:
      case NMPC_HIP_CGMRES_FIELD_LOG_REORTH: *bytes = B * L * sizeof(int); break;
      default: return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "unknown field");
    }
    return NMPC_HIP_OK;
  }

  int nmpc_hip_cgmres_get(nmpc_hip_cgmres_handle h, int field, void * out, size_t bytes)
  {
    size_t want = 0;
    const int rc = nmpc_hip_cgmres_field_bytes(h, field, &want);
    if(rc != NMPC_HIP_OK)
    {
      return rc;
    }
    if(!out || bytes != want)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "[C/GMRES] output size mismatch");
    }
    if(want == 0)
    {
      return NMPC_HIP_OK;
    }
    NMPC_CAPI_TRY(hipSetDevice(h->device));
    NMPC_CAPI_TRY(hipStreamSynchronize(h->stream));
    if(field == NMPC_HIP_CGMRES_FIELD_LOG_T)
    {
      std::memcpy(out, h->log_t.data(), want);
      return NMPC_HIP_OK;
    }
    const CgmresBuffers & b = h->bf;
    const size_t B = b.B, L = b.log_rows;
    const void * src = nullptr;
    size_t E = 0; // elements per instance (per row for the logs)
    size_t rows = 1;
    bool is_int = false;
    switch(field)
    {
      case NMPC_HIP_CGMRES_FIELD_X: src = b.x, E = b.nx; break;
      case NMPC_HIP_CGMRES_FIELD_U: src = b.u, E = b.nuc; break;
      case NMPC_HIP_CGMRES_FIELD_U_LIST: src = b.U, E = static_cast<size_t>(b.N) * b.nuc; break;
      case NMPC_HIP_CGMRES_FIELD_DELTA_U: src = b.du, E = static_cast<size_t>(b.N) * b.nuc; break;
      case NMPC_HIP_CGMRES_FIELD_STATUS: src = b.status, E = 1, is_int = true; break;
      case NMPC_HIP_CGMRES_FIELD_ERR: src = b.err, E = 1; break;
      case NMPC_HIP_CGMRES_FIELD_LOG_X: src = b.log_x, E = b.nx, rows = L; break;
      case NMPC_HIP_CGMRES_FIELD_LOG_U: src = b.log_u, E = b.nuc, rows = L; break;
      case NMPC_HIP_CGMRES_FIELD_LOG_ERR: src = b.log_err, E = 1, rows = L; break;
      case NMPC_HIP_CGMRES_FIELD_LOG_ITERS: src = b.log_iters, E = 1, rows = L, is_int = true; break;
      case NMPC_HIP_CGMRES_FIELD_LOG_REORTH: src = b.log_reorth, E = 1, rows = L, is_int = true; break;
    }
    // device [row][e][B] -> boundary [B][row][e]: the same transpose with E' = rows * E
    const size_t Et = rows * E;
    if(is_int)
    {
      std::vector<int> tmp(B * Et);
      NMPC_CAPI_TRY(hipMemcpy(tmp.data(), src, want, hipMemcpyDeviceToHost));
      toBoundary(tmp.data(), static_cast<int *>(out), B, Et);
    }
    else
    {
      std::vector<double> tmp(B * Et);
      NMPC_CAPI_TRY(hipMemcpy(tmp.data(), src, want, hipMemcpyDeviceToHost));
      toBoundary(tmp.data(), static_cast<double *>(out), B, Et);
    }
    return NMPC_HIP_OK;
  }

  int nmpc_hip_cgmres_dense_gmres(int device, int batch, int n, const double * A, const double * b, double * x, int k_max,
                                  int apply_reorth, double eps, int * iters, int * reorth)
  {
    if(!A || !b || !x || batch < 1 || n < 1 || n > cg::kDenseMaxN || k_max < 1 || !(eps >= 0))
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "[C/GMRES] dense_gmres: 1 <= n <= 512, batch >= 1, k_max >= 1, eps >= 0, non-NULL arrays");
    }
    NMPC_CAPI_CHECK(capi::checkDevice<Family>(device));
    const size_t B = batch, N = n;
    const int K = std::min(k_max, n);
    const size_t ws_elems = cg::gmresWorkspaceElems(n, K);
    std::vector<double> hA(B * N * N), hx(B * N), hws(B * N);
    toDevice(A, hA.data(), B, N * N);
    toDevice(x, hx.data(), B, N);
    toDevice(b, hws.data(), B, N); // the right-hand side is the workspace's first vector
    DevBuf dA, dx, dws, dit;
    NMPC_CAPI_TRY(hipMalloc(&dA.p, hA.size() * sizeof(double)));
    NMPC_CAPI_TRY(hipMalloc(&dx.p, hx.size() * sizeof(double)));
    NMPC_CAPI_TRY(hipMalloc(&dws.p, ws_elems * B * sizeof(double)));
    NMPC_CAPI_TRY(hipMalloc(&dit.p, 2 * B * sizeof(int)));
    NMPC_CAPI_TRY(hipMemcpy(dA.p, hA.data(), hA.size() * sizeof(double), hipMemcpyHostToDevice));
    NMPC_CAPI_TRY(hipMemcpy(dx.p, hx.data(), hx.size() * sizeof(double), hipMemcpyHostToDevice));
    NMPC_CAPI_TRY(hipMemset(dws.p, 0, ws_elems * B * sizeof(double)));
    NMPC_CAPI_TRY(hipMemcpy(dws.p, hws.data(), hws.size() * sizeof(double), hipMemcpyHostToDevice));
    int * d_it = static_cast<int *>(dit.p);
    hipLaunchKernelGGL(cg::cgmres_gmres_dense_kernel, dim3(static_cast<unsigned>((B + cg::kBlock - 1) / cg::kBlock)), dim3(cg::kBlock), 0,
                       nullptr, batch, n, K, k_max, apply_reorth, eps, static_cast<const double *>(dA.p), static_cast<double *>(dx.p),
                       static_cast<double *>(dws.p), d_it, d_it + B);
    NMPC_CAPI_TRY(hipGetLastError());
    NMPC_CAPI_TRY(hipDeviceSynchronize());
    NMPC_CAPI_TRY(hipMemcpy(hx.data(), dx.p, hx.size() * sizeof(double), hipMemcpyDeviceToHost));
    toBoundary(hx.data(), x, B, N);
    std::vector<int> it(2 * B);
    NMPC_CAPI_TRY(hipMemcpy(it.data(), dit.p, it.size() * sizeof(int), hipMemcpyDeviceToHost));
    if(iters)
    {
      std::copy(it.begin(), it.begin() + B, iters);
    }
    if(reorth)
    {
      std::copy(it.begin() + B, it.end(), reorth);
    }
    return NMPC_HIP_OK;
  }

  int nmpc_hip_cgmres_model_eval(nmpc_hip_cgmres_handle h, int n_points, const double * t, const double * x, const double * u,
                                 const double * lmd, double * dotx, double * dotlmd, double * dphidx, double * dhdu)
  {
    if(!h || n_points < 1 || !t || !x || !u || !lmd || !dotx || !dotlmd || !dphidx || !dhdu)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "NULL argument or n_points < 1");
    }
    NMPC_CAPI_TRY(hipSetDevice(h->device));
    const size_t P = n_points, NX = h->ops->nx, NUC = h->ops->nuc;
    const size_t sizes[8] = {P, P * NX, P * NUC, P * NX, P * NX, P * NX, P * NX, P * NUC};
    size_t total = 0;
    for(size_t s : sizes)
    {
      total += s;
    }
    DevBuf d;
    NMPC_CAPI_TRY(hipMalloc(&d.p, total * sizeof(double)));
    double * p[8];
    p[0] = static_cast<double *>(d.p);
    for(int i = 1; i < 8; i++)
    {
      p[i] = p[i - 1] + sizes[i - 1];
    }
    const double * in[4] = {t, x, u, lmd};
    double * outs[4] = {dotx, dotlmd, dphidx, dhdu};
    NMPC_CAPI_TRY(hipStreamSynchronize(h->stream));
    for(int i = 0; i < 4; i++)
    {
      NMPC_CAPI_TRY(hipMemcpy(p[i], in[i], sizes[i] * sizeof(double), hipMemcpyHostToDevice));
    }
    NMPC_CAPI_TRY(h->ops->launch_model_eval(h->bf, n_points, p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], h->stream));
    NMPC_CAPI_TRY(hipStreamSynchronize(h->stream));
    for(int i = 0; i < 4; i++)
    {
      NMPC_CAPI_TRY(hipMemcpy(outs[i], p[4 + i], sizes[4 + i] * sizeof(double), hipMemcpyDeviceToHost));
    }
    return NMPC_HIP_OK;
  }

  int nmpc_hip_cgmres_last_ms(nmpc_hip_cgmres_handle h, float * ms)
  {
    if(!h || !ms)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    }
    *ms = h->last_ms;
    return NMPC_HIP_OK;
  }

  const char * nmpc_hip_cgmres_last_error(void)
  {
    return capi::lastError<Family>().c_str();
  }
}
