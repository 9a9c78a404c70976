// C-ABI of the batched FMPC iteration on caller-supplied linearisations (declared in include/nmpc_hip_fmpc_step.h): handles,
// device-buffer ownership and the launch of fmpc_step_wave_kernel.  No CPU fallback exists: without the HIP runtime or a device every
// entry point that needs the GPU fails loudly.
#include <nmpc_hip_fmpc_step.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include <nmpc_amd/hip/capi_core.hpp>
#include <nmpc_amd/hip/fmpc_step_kernels.hpp>

namespace capi = nmpc_amd::hip::capi;
namespace fs = nmpc_amd::hip::fmpc_step;

static_assert(NMPC_HIP_FMPC_STEP_MAX_DIM == fs::kMaxDim && NMPC_HIP_FMPC_STEP_MAX_INEQ == fs::kMaxIneq,
              "nmpc_hip_fmpc_step.h and fmpc_step_kernels.hpp disagree");
static_assert(int(NMPC_HIP_FMPC_STEP_SUCCEEDED) == fs::kSucceeded && int(NMPC_HIP_FMPC_STEP_ERROR_IN_FORWARD) == fs::kErrorInForward
                  && int(NMPC_HIP_FMPC_STEP_ERROR_IN_BACKWARD) == fs::kErrorInBackward
                  && int(NMPC_HIP_FMPC_STEP_ERROR_IN_UPDATE) == fs::kErrorInUpdate
                  && int(NMPC_HIP_FMPC_STEP_ITERATION_CONTINUED) == fs::kIterationContinued,
              "nmpc_hip_fmpc_step.h and fmpc_step_kernels.hpp disagree");

namespace
{
struct Family
{
  static constexpr const char * tag = "[FmpcStep]";
  static constexpr const char * noun = "the FMPC step solver";
  static constexpr const char * prefix = "nmpc_hip_fmpc_step";
};
constexpr auto fail = capi::fail<Family>;
using capi::Input;
} // namespace

struct nmpc_hip_fmpc_step_solver : capi::HandleCore<Family>
{
  int n = 0, m = 0, g = 0, T = 0;
  size_t B = 0;
  nmpc_hip_fmpc_step_config cfg;
  bool have_linearisation = false, have_variable = false, have_dims = false, stepped = false;
  int total_ineq_dim = 0;
  Input A, Bm, C, D, Lx, Lu, Lxx, Luu, Lxu, f, gv, LxT, LxxT, cur_x;
  int *d_mdims = nullptr, *d_gdims = nullptr;
  double *d_x = nullptr, *d_u = nullptr, *d_lam = nullptr, *d_s = nullptr, *d_nu = nullptr, *d_eps = nullptr; // the variable
  double * d_out_d = nullptr; // every real result and the workspace, placed by fs::OutputLayout
  int * d_out_i = nullptr; // status
  fs::OutputLayout layout() const
  {
    return fs::OutputLayout(B, T, n, m, g);
  }
};

namespace
{
int validConfig(const nmpc_hip_fmpc_step_config & c)
{
  if(std::isnan(c.dt) || std::isnan(c.kkt_error_thre))
  {
    return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "[FmpcStep] dt and kkt_error_thre must not be NaN");
  }
  return NMPC_HIP_OK;
}

bool isVarField(int field)
{
  return field >= NMPC_HIP_FMPC_STEP_FIELD_VAR_X && field <= NMPC_HIP_FMPC_STEP_FIELD_VAR_NU;
}

int fieldBytes(const nmpc_hip_fmpc_step_solver * h, int field, size_t * bytes)
{
  const size_t B = h->B, n = h->n, m = h->m, g = h->g, T = h->T;
  size_t count = 0;
  switch(field)
  {
    case NMPC_HIP_FMPC_STEP_FIELD_STATUS:
      *bytes = B * sizeof(int);
      return NMPC_HIP_OK;
    case NMPC_HIP_FMPC_STEP_FIELD_KKT_ERROR:
    case NMPC_HIP_FMPC_STEP_FIELD_BARRIER_EPS:
    case NMPC_HIP_FMPC_STEP_FIELD_ALPHA_S_MAX:
    case NMPC_HIP_FMPC_STEP_FIELD_ALPHA_NU_MAX:
      count = B;
      break;
    case NMPC_HIP_FMPC_STEP_FIELD_K_FF:
    case NMPC_HIP_FMPC_STEP_FIELD_DELTA_U:
    case NMPC_HIP_FMPC_STEP_FIELD_VAR_U:
      count = B * T * m;
      break;
    case NMPC_HIP_FMPC_STEP_FIELD_K_FB:
      count = B * T * m * n;
      break;
    case NMPC_HIP_FMPC_STEP_FIELD_S:
    case NMPC_HIP_FMPC_STEP_FIELD_DELTA_X:
    case NMPC_HIP_FMPC_STEP_FIELD_DELTA_LAMBDA:
    case NMPC_HIP_FMPC_STEP_FIELD_VAR_X:
    case NMPC_HIP_FMPC_STEP_FIELD_VAR_LAMBDA:
      count = B * (T + 1) * n;
      break;
    case NMPC_HIP_FMPC_STEP_FIELD_P:
      count = B * (T + 1) * n * n;
      break;
    case NMPC_HIP_FMPC_STEP_FIELD_DELTA_S:
    case NMPC_HIP_FMPC_STEP_FIELD_DELTA_NU:
    case NMPC_HIP_FMPC_STEP_FIELD_VAR_S:
    case NMPC_HIP_FMPC_STEP_FIELD_VAR_NU:
      count = B * T * g;
      break;
    default:
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "[FmpcStep] unknown field");
  }
  *bytes = count * sizeof(double);
  return NMPC_HIP_OK;
}

const void * fieldPtr(const nmpc_hip_fmpc_step_solver * h, int field)
{
  const fs::OutputLayout at = h->layout();
  switch(field)
  {
    case NMPC_HIP_FMPC_STEP_FIELD_STATUS:
      return h->d_out_i;
    case NMPC_HIP_FMPC_STEP_FIELD_KKT_ERROR:
      return h->d_out_d + at.kkt;
    case NMPC_HIP_FMPC_STEP_FIELD_BARRIER_EPS:
      return h->d_eps;
    case NMPC_HIP_FMPC_STEP_FIELD_ALPHA_S_MAX:
      return h->d_out_d + at.alpha_s;
    case NMPC_HIP_FMPC_STEP_FIELD_ALPHA_NU_MAX:
      return h->d_out_d + at.alpha_nu;
    case NMPC_HIP_FMPC_STEP_FIELD_K_FF:
      return h->d_out_d + at.k;
    case NMPC_HIP_FMPC_STEP_FIELD_K_FB:
      return h->d_out_d + at.K;
    case NMPC_HIP_FMPC_STEP_FIELD_S:
      return h->d_out_d + at.gs;
    case NMPC_HIP_FMPC_STEP_FIELD_P:
      return h->d_out_d + at.P;
    case NMPC_HIP_FMPC_STEP_FIELD_DELTA_X:
      return h->d_out_d + at.dx;
    case NMPC_HIP_FMPC_STEP_FIELD_DELTA_U:
      return h->d_out_d + at.du;
    case NMPC_HIP_FMPC_STEP_FIELD_DELTA_LAMBDA:
      return h->d_out_d + at.dlam;
    case NMPC_HIP_FMPC_STEP_FIELD_DELTA_S:
      return h->d_out_d + at.ds;
    case NMPC_HIP_FMPC_STEP_FIELD_DELTA_NU:
      return h->d_out_d + at.dnu;
    case NMPC_HIP_FMPC_STEP_FIELD_VAR_X:
      return h->d_x;
    case NMPC_HIP_FMPC_STEP_FIELD_VAR_U:
      return h->d_u;
    case NMPC_HIP_FMPC_STEP_FIELD_VAR_LAMBDA:
      return h->d_lam;
    case NMPC_HIP_FMPC_STEP_FIELD_VAR_S:
      return h->d_s;
    default:
      return h->d_nu;
  }
}

int launchStep(nmpc_hip_fmpc_step_solver * h, hipStream_t s)
{
  if(!h->have_linearisation || !h->have_variable)
  {
    return fail(NMPC_HIP_ERR_NOT_SOLVED, "[FmpcStep] step needs a set_linearisation and a set_variable first");
  }
  const nmpc_hip_fmpc_step_config & c = h->cfg;
  const int total = h->have_dims ? h->total_ineq_dim : h->g * h->T;
  if(c.update_barrier_eps && total == 0)
  {
    return fail(NMPC_HIP_ERR_INVALID_ARGUMENT,
                "[FmpcStep] update_barrier_eps needs an inequality at some step: the reference divides 0 by 0 there");
  }
  const fs::Params p{h->n, h->m, h->g, h->T, c.row_major != 0 ? 1 : 0, c.check_nan != 0 ? 1 : 0,
                     c.init_complementary_variable != 0 ? 1 : 0, c.update_barrier_eps != 0 ? 1 : 0,
                     c.break_if_llt_fails != 0 ? 1 : 0, c.apply_update != 0 ? 1 : 0, total, h->B, c.dt, c.kkt_error_thre};
  const fs::Buffers buf{h->A.ptr, h->Bm.ptr, h->C.ptr, h->D.ptr, h->Lx.ptr, h->Lu.ptr, h->Lxx.ptr, h->Luu.ptr, h->Lxu.ptr, h->f.ptr,
                        h->gv.ptr, h->LxT.ptr, h->LxxT.ptr, h->cur_x.ptr, h->have_dims ? h->d_mdims : nullptr,
                        h->have_dims ? h->d_gdims : nullptr, h->d_x, h->d_u, h->d_lam, h->d_s, h->d_nu, h->d_eps, h->d_out_d,
                        h->d_out_i};
  NMPC_CAPI_CHECK(h->beginLaunch(s));
  hipLaunchKernelGGL(fs::fmpc_step_wave_kernel, dim3(static_cast<unsigned>(h->B)), dim3(fs::kWave), fs::ldsBytes(h->n, h->m, h->g), s, buf,
                     p);
  NMPC_CAPI_TRY(hipGetLastError());
  NMPC_CAPI_CHECK(h->endLaunch(s));
  h->stepped = true;
  return NMPC_HIP_OK;
}

/** The VAR fields are there from set_variable on, every other field from the first step on. */
bool haveField(const nmpc_hip_fmpc_step_solver * h, int field)
{
  return isVarField(field) ? h->have_variable : h->stepped;
}
} // namespace

extern "C"
{
  int nmpc_hip_fmpc_step_default_config(nmpc_hip_fmpc_step_config * cfg)
  {
    if(!cfg)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "cfg is NULL");
    }
    cfg->dt = 0.01;
    cfg->kkt_error_thre = 1e-4;
    cfg->check_nan = 1;
    cfg->init_complementary_variable = 0;
    cfg->update_barrier_eps = 1;
    cfg->break_if_llt_fails = 0;
    cfg->apply_update = 1;
    cfg->row_major = 0;
    return NMPC_HIP_OK;
  }

  int nmpc_hip_fmpc_step_destroy(nmpc_hip_fmpc_step_handle h)
  {
    if(!h)
    {
      return NMPC_HIP_OK;
    }
    h->close();
    delete h;
    return NMPC_HIP_OK;
  }

  int nmpc_hip_fmpc_step_create(int state_dim,
                                int input_dim,
                                int ineq_dim,
                                int horizon_steps,
                                int batch,
                                int device,
                                nmpc_hip_fmpc_step_handle * out)
  {
    if(!out)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "out is NULL");
    }
    *out = nullptr;
    if(state_dim < 1 || state_dim > NMPC_HIP_FMPC_STEP_MAX_DIM)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "[FmpcStep] state_dim must be in 1 .. 16: " + std::to_string(state_dim));
    }
    if(input_dim < 0 || input_dim > NMPC_HIP_FMPC_STEP_MAX_DIM)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "[FmpcStep] input_dim must be in 0 .. 16: " + std::to_string(input_dim));
    }
    if(ineq_dim < 0 || ineq_dim > NMPC_HIP_FMPC_STEP_MAX_INEQ)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "[FmpcStep] ineq_dim must be in 0 .. 32: " + std::to_string(ineq_dim));
    }
    if(horizon_steps < 1)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "[FmpcStep] horizon_steps must be positive: " + std::to_string(horizon_steps));
    }
    if(batch < 1)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "[FmpcStep] batch must be positive: " + std::to_string(batch));
    }
    NMPC_CAPI_CHECK(capi::checkDevice<Family>(device));
    auto * h = new nmpc_hip_fmpc_step_solver();
    h->n = state_dim;
    h->m = input_dim;
    h->g = ineq_dim;
    h->T = horizon_steps;
    h->B = batch;
    h->device = device;
    nmpc_hip_fmpc_step_default_config(&h->cfg);
    auto cleanup = [&](int code) {
      nmpc_hip_fmpc_step_destroy(h);
      return code;
    };
    int rc_ = h->open();
    if(rc_ != NMPC_HIP_OK)
    {
      return cleanup(rc_);
    }
    const size_t T = horizon_steps, B = batch, n = state_dim, m = input_dim, g = ineq_dim;
    auto A = [&](auto ** p, size_t count, const char * what) {
      if(rc_ == NMPC_HIP_OK)
      {
        rc_ = h->devAlloc(p, count, what);
      }
    };
    A(&h->d_mdims, T, "the input dimensions");
    A(&h->d_gdims, T, "the inequality dimensions");
    A(&h->d_x, B * (T + 1) * n, "x");
    A(&h->d_u, B * T * m, "u");
    A(&h->d_lam, B * (T + 1) * n, "lambda");
    A(&h->d_s, B * T * g, "s");
    A(&h->d_nu, B * T * g, "nu");
    A(&h->d_eps, B, "barrier_eps");
    A(&h->d_out_d, h->layout().doubles, "the gains, the delta and the residuals");
    A(&h->d_out_i, B, "the status");
    if(rc_ != NMPC_HIP_OK)
    {
      return cleanup(rc_);
    }
    {
      const std::vector<double> eps(B, 1e-4); // FmpcSolver.h:414
      if(hipMemcpy(h->d_eps, eps.data(), B * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
      {
        return cleanup(fail(NMPC_HIP_ERR_HIP, "copying the initial barrier_eps failed"));
      }
    }
    // the largest shape asks for 48 128 bytes of LDS: below the 64 KB a kernel may use without asking
    static_assert(fs::ldsBytes(fs::kMaxDim, fs::kMaxDim, fs::kMaxIneq) <= 64 * 1024, "fmpc_step_wave_kernel would need hipFuncSetAttribute");
    *out = h;
    return NMPC_HIP_OK;
  }

  int nmpc_hip_fmpc_step_set_config(nmpc_hip_fmpc_step_handle h, const nmpc_hip_fmpc_step_config * cfg)
  {
    if(!h || !cfg)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    }
    const int rc_ = validConfig(*cfg);
    if(rc_ != NMPC_HIP_OK)
    {
      return rc_;
    }
    h->cfg = *cfg;
    return NMPC_HIP_OK;
  }

  int nmpc_hip_fmpc_step_get_config(nmpc_hip_fmpc_step_handle h, nmpc_hip_fmpc_step_config * cfg)
  {
    if(!h || !cfg)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    }
    *cfg = h->cfg;
    return NMPC_HIP_OK;
  }

  int nmpc_hip_fmpc_step_set_step_dims(nmpc_hip_fmpc_step_handle h, const int * input_dims, const int * ineq_dims)
  {
    if(!h)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "NULL handle");
    }
    if(!input_dims && !ineq_dims)
    {
      h->have_dims = false;
      return NMPC_HIP_OK;
    }
    std::vector<int> md(h->T, h->m), gd(h->T, h->g);
    int total = 0;
    for(int i = 0; i < h->T; i++)
    {
      if(input_dims)
      {
        md[i] = input_dims[i];
      }
      if(ineq_dims)
      {
        gd[i] = ineq_dims[i];
      }
      if(md[i] < 0 || md[i] > h->m)
      {
        return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "[FmpcStep] input_dims[" + std::to_string(i) + "] = " + std::to_string(md[i])
                                                       + " is outside 0 .. " + std::to_string(h->m));
      }
      if(gd[i] < 0 || gd[i] > h->g)
      {
        return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "[FmpcStep] ineq_dims[" + std::to_string(i) + "] = " + std::to_string(gd[i])
                                                       + " is outside 0 .. " + std::to_string(h->g));
      }
      total += gd[i];
    }
    NMPC_CAPI_TRY(hipSetDevice(h->device));
    NMPC_CAPI_CHECK(h->waitForOtherStream());
    NMPC_CAPI_TRY(hipMemcpyAsync(h->d_mdims, md.data(), md.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
    NMPC_CAPI_TRY(hipMemcpyAsync(h->d_gdims, gd.data(), gd.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
    NMPC_CAPI_TRY(hipStreamSynchronize(h->stream));
    h->total_ineq_dim = total;
    h->have_dims = true;
    return NMPC_HIP_OK;
  }

  int nmpc_hip_fmpc_step_set_linearisation(nmpc_hip_fmpc_step_handle h,
                                           const double * A,
                                           const double * B,
                                           const double * C,
                                           const double * D,
                                           const double * Lx,
                                           const double * Lu,
                                           const double * Lxx,
                                           const double * Luu,
                                           const double * Lxu,
                                           const double * f,
                                           const double * g,
                                           const double * Lx_T,
                                           const double * Lxx_T,
                                           const double * current_x,
                                           int on_device)
  {
    if(!h || !A || !Lx || !Lxx || !f || !Lx_T || !Lxx_T || !current_x || (h->m > 0 && (!B || !Lu || !Luu || !Lxu))
       || (h->g > 0 && (!C || !g)) || (h->g > 0 && h->m > 0 && !D))
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    }
    NMPC_CAPI_TRY(hipSetDevice(h->device));
    NMPC_CAPI_CHECK(h->waitForOtherStream());
    const size_t Bn = h->B, n = h->n, m = h->m, gg = h->g, S = h->B * h->T;
    int rc_ = NMPC_HIP_OK;
    auto set = [&](Input & in, const double * src, size_t count, const char * what) {
      if(rc_ == NMPC_HIP_OK)
      {
        rc_ = h->setInput(in, src, count, on_device, what);
      }
    };
    set(h->A, A, S * n * n, "A");
    set(h->Bm, B, S * n * m, "B");
    set(h->C, C, S * gg * n, "C");
    set(h->D, D, S * gg * m, "D");
    set(h->Lx, Lx, S * n, "Lx");
    set(h->Lu, Lu, S * m, "Lu");
    set(h->Lxx, Lxx, S * n * n, "Lxx");
    set(h->Luu, Luu, S * m * m, "Luu");
    set(h->Lxu, Lxu, S * n * m, "Lxu");
    set(h->f, f, S * n, "f");
    set(h->gv, g, S * gg, "g");
    set(h->LxT, Lx_T, Bn * n, "Lx_T");
    set(h->LxxT, Lxx_T, Bn * n * n, "Lxx_T");
    set(h->cur_x, current_x, Bn * n, "current_x");
    if(rc_ != NMPC_HIP_OK)
    {
      return rc_;
    }
    NMPC_CAPI_TRY(hipStreamSynchronize(h->stream));
    h->have_linearisation = true;
    return NMPC_HIP_OK;
  }

  int nmpc_hip_fmpc_step_set_variable(nmpc_hip_fmpc_step_handle h,
                                      const double * x,
                                      const double * u,
                                      const double * lambda,
                                      const double * s,
                                      const double * nu,
                                      const double * barrier_eps,
                                      int on_device)
  {
    if(!h || !x || !lambda || (h->m > 0 && !u) || (h->g > 0 && (!s || !nu)))
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    }
    NMPC_CAPI_TRY(hipSetDevice(h->device));
    NMPC_CAPI_CHECK(h->waitForOtherStream());
    const size_t B = h->B, n = h->n, m = h->m, g = h->g, T = h->T;
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    auto copy = [&](double * dst, const double * src, size_t count) {
      return (count == 0 || !src) ? hipSuccess : hipMemcpyAsync(dst, src, count * sizeof(double), kind, h->stream);
    };
    NMPC_CAPI_TRY(copy(h->d_x, x, B * (T + 1) * n));
    NMPC_CAPI_TRY(copy(h->d_u, u, B * T * m));
    NMPC_CAPI_TRY(copy(h->d_lam, lambda, B * (T + 1) * n));
    NMPC_CAPI_TRY(copy(h->d_s, s, B * T * g));
    NMPC_CAPI_TRY(copy(h->d_nu, nu, B * T * g));
    NMPC_CAPI_TRY(copy(h->d_eps, barrier_eps, B));
    NMPC_CAPI_TRY(hipStreamSynchronize(h->stream));
    h->have_variable = true;
    return NMPC_HIP_OK;
  }

  int nmpc_hip_fmpc_step_step_device(nmpc_hip_fmpc_step_handle h, void * stream)
  {
    if(!h)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "NULL handle");
    }
    NMPC_CAPI_TRY(hipSetDevice(h->device));
    hipStream_t s = h->streamFor(stream);
    NMPC_CAPI_CHECK(h->waitBeforeLaunchOn(s)); // the previous step writes the buffers this one writes
    return launchStep(h, s);
  }

  int nmpc_hip_fmpc_step_step(nmpc_hip_fmpc_step_handle h)
  {
    NMPC_CAPI_CHECK(nmpc_hip_fmpc_step_step_device(h, nullptr));
    return h->syncLast();
  }

  int nmpc_hip_fmpc_step_synchronize(nmpc_hip_fmpc_step_handle h)
  {
    if(!h)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "NULL handle");
    }
    NMPC_CAPI_TRY(hipSetDevice(h->device));
    return h->syncLast();
  }

  int nmpc_hip_fmpc_step_field_bytes(nmpc_hip_fmpc_step_handle h, int field, size_t * bytes)
  {
    if(!h || !bytes)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    }
    return fieldBytes(h, field, bytes);
  }

  int nmpc_hip_fmpc_step_get(nmpc_hip_fmpc_step_handle h, int field, void * out, size_t bytes, int on_device)
  {
    size_t want = 0;
    NMPC_CAPI_CHECK(capi::beginGet<Family>(h, field, out, bytes, &want, fieldBytes, haveField,
                                           "get needs a step (a set_variable for the VAR fields)"));
    return h->copyOut(out, fieldPtr(h, field), want, on_device, capi::kWaitForHostOnly);
  }

  int nmpc_hip_fmpc_step_kernel_name(nmpc_hip_fmpc_step_handle h, const char ** name)
  {
    if(!h || !name)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    }
    *name = "fmpc_step_wave_kernel";
    return NMPC_HIP_OK;
  }

  int nmpc_hip_fmpc_step_last_ms(nmpc_hip_fmpc_step_handle h, float * ms)
  {
    if(!h || !ms)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    }
    return h->lastMs(ms, "last_ms needs a step");
  }

  const char * nmpc_hip_fmpc_step_last_error(void)
  {
    return capi::lastError<Family>().c_str();
  }
}
