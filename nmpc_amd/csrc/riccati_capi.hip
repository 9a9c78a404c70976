// C-ABI of the batched Riccati backward pass (declared in include/nmpc_hip_riccati.h): handles, device-buffer ownership and the
// launch of riccati_wave_kernel.  No CPU fallback exists: without the HIP runtime or a device every entry point that needs the GPU
// fails loudly.
#include <nmpc_hip_riccati.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include <nmpc_amd/hip/capi_core.hpp>
#include <nmpc_amd/hip/riccati_kernels.hpp>

namespace capi = nmpc_amd::hip::capi;
namespace rc = nmpc_amd::hip::riccati;

static_assert(NMPC_HIP_RICCATI_MAX_DIM == rc::kMaxDim, "nmpc_hip_riccati.h and riccati_kernels.hpp disagree");
static_assert(int(NMPC_HIP_RICCATI_OK) == rc::kStatusOk && int(NMPC_HIP_RICCATI_LAMBDA_MAX) == rc::kStatusLambdaMax
                  && int(NMPC_HIP_RICCATI_PASS_FAILED) == rc::kStatusPassFailed,
              "nmpc_hip_riccati.h and riccati_kernels.hpp disagree");

namespace
{
struct Family
{
  static constexpr const char * tag = "[Riccati]";
  static constexpr const char * noun = "the Riccati solver";
  static constexpr const char * prefix = "nmpc_hip_riccati";
};
constexpr auto fail = capi::fail<Family>;
using capi::Input;
} // namespace

struct nmpc_hip_riccati_solver : capi::HandleCore<Family>
{
  int n = 0, m = 0, T = 0;
  size_t B = 0;
  nmpc_hip_riccati_config cfg;
  bool have_derivatives = false, have_inputs = false, have_dims = false, solved = false;
  int limits_per_step = 0;
  Input Fx, Fu, Lx, Lu, Lxx, Luu, Lxu, VxT, VxxT, U, lower, upper, lam, dlam;
  int * d_dims = nullptr;
  double * d_out_d = nullptr; // every real result, placed by rc::OutputLayout
  int * d_out_i = nullptr; // every 32-bit result, likewise
  rc::OutputLayout layout() const
  {
    return rc::OutputLayout(B, T, n, m);
  }
};

namespace
{
int validConfig(const nmpc_hip_riccati_config & c)
{
  if(c.reg_type != 1 && c.reg_type != 2)
  {
    return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "[Riccati] reg_type must be 1 or 2: " + std::to_string(c.reg_type));
  }
  if(!std::isfinite(c.lambda_factor) || !std::isfinite(c.lambda_min) || !std::isfinite(c.lambda_max))
  {
    return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "[Riccati] lambda_factor, lambda_min and lambda_max must be finite");
  }
  return NMPC_HIP_OK;
}

int fieldBytes(const nmpc_hip_riccati_solver * h, int field, size_t * bytes)
{
  const size_t B = h->B, n = h->n, m = h->m, T = h->T;
  switch(field)
  {
    case NMPC_HIP_RICCATI_FIELD_K_FF:
      *bytes = B * T * m * sizeof(double);
      return NMPC_HIP_OK;
    case NMPC_HIP_RICCATI_FIELD_K_FB:
      *bytes = B * T * m * n * sizeof(double);
      return NMPC_HIP_OK;
    case NMPC_HIP_RICCATI_FIELD_DV:
      *bytes = B * 2 * sizeof(double);
      return NMPC_HIP_OK;
    case NMPC_HIP_RICCATI_FIELD_VX0:
      *bytes = B * n * sizeof(double);
      return NMPC_HIP_OK;
    case NMPC_HIP_RICCATI_FIELD_VXX0:
      *bytes = B * n * n * sizeof(double);
      return NMPC_HIP_OK;
    case NMPC_HIP_RICCATI_FIELD_STATUS:
    case NMPC_HIP_RICCATI_FIELD_N_BACKWARD:
    case NMPC_HIP_RICCATI_FIELD_FAIL_STEP:
      *bytes = B * sizeof(int);
      return NMPC_HIP_OK;
    case NMPC_HIP_RICCATI_FIELD_LAMBDA:
    case NMPC_HIP_RICCATI_FIELD_DLAMBDA:
      *bytes = B * sizeof(double);
      return NMPC_HIP_OK;
    case NMPC_HIP_RICCATI_FIELD_QP_RETVAL:
      *bytes = B * T * sizeof(int);
      return NMPC_HIP_OK;
    case NMPC_HIP_RICCATI_FIELD_FREE_MASK:
      *bytes = B * T * sizeof(unsigned);
      return NMPC_HIP_OK;
    default:
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "[Riccati] unknown field");
  }
}

const void * fieldPtr(const nmpc_hip_riccati_solver * h, int field)
{
  const rc::OutputLayout at = h->layout();
  switch(field)
  {
    case NMPC_HIP_RICCATI_FIELD_K_FF:
      return h->d_out_d + at.k;
    case NMPC_HIP_RICCATI_FIELD_K_FB:
      return h->d_out_d + at.K;
    case NMPC_HIP_RICCATI_FIELD_DV:
      return h->d_out_d + at.dV;
    case NMPC_HIP_RICCATI_FIELD_VX0:
      return h->d_out_d + at.Vx0;
    case NMPC_HIP_RICCATI_FIELD_VXX0:
      return h->d_out_d + at.Vxx0;
    case NMPC_HIP_RICCATI_FIELD_LAMBDA:
      return h->d_out_d + at.lam;
    case NMPC_HIP_RICCATI_FIELD_DLAMBDA:
      return h->d_out_d + at.dlam;
    case NMPC_HIP_RICCATI_FIELD_STATUS:
      return h->d_out_i + at.status;
    case NMPC_HIP_RICCATI_FIELD_N_BACKWARD:
      return h->d_out_i + at.n_backward;
    case NMPC_HIP_RICCATI_FIELD_FAIL_STEP:
      return h->d_out_i + at.fail_step;
    case NMPC_HIP_RICCATI_FIELD_QP_RETVAL:
      return h->d_out_i + at.qp_retval;
    default:
      return h->d_out_i + at.free_mask;
  }
}

int launchSolve(nmpc_hip_riccati_solver * h, hipStream_t s)
{
  if(!h->have_derivatives)
  {
    return fail(NMPC_HIP_ERR_NOT_SOLVED, "[Riccati] solve needs a set_derivatives first");
  }
  const bool constrained = h->cfg.with_input_constraint != 0;
  if(constrained && !h->have_inputs)
  {
    return fail(NMPC_HIP_ERR_NOT_SOLVED, "[Riccati] solve with with_input_constraint needs a set_inputs first");
  }
  const nmpc_hip_riccati_config & c = h->cfg;
  const rc::Params p{h->n, h->m, h->T, c.reg_type, constrained ? 1 : 0, c.retry != 0 ? 1 : 0, c.row_major != 0 ? 1 : 0,
                     h->limits_per_step, h->B, c.lambda, c.dlambda, c.lambda_factor, c.lambda_min, c.lambda_max};
  const rc::Buffers buf{h->Fx.ptr, h->Fu.ptr, h->Lx.ptr, h->Lu.ptr, h->Lxx.ptr, h->Luu.ptr, h->Lxu.ptr, h->VxT.ptr, h->VxxT.ptr,
                        h->U.ptr, h->lower.ptr, h->upper.ptr, h->lam.ptr, h->dlam.ptr, h->have_dims ? h->d_dims : nullptr,
                        h->d_out_d, h->d_out_i};
  NMPC_CAPI_CHECK(h->beginLaunch(s));
  // qp_retval_ and the free masks of steps without a QP are 0 (the two fields are neighbours in the allocation)
  static_assert(sizeof(int) == sizeof(unsigned), "the free masks share the 32-bit allocation");
  NMPC_CAPI_TRY(hipMemsetAsync(h->d_out_i + h->layout().qp_retval, 0, 2 * h->B * h->T * sizeof(int), s));
  hipLaunchKernelGGL(rc::riccati_wave_kernel, dim3(static_cast<unsigned>(h->B)), dim3(rc::kWave), rc::ldsBytes(h->n, h->m), s, buf, p);
  NMPC_CAPI_TRY(hipGetLastError());
  NMPC_CAPI_CHECK(h->endLaunch(s));
  h->solved = true;
  return NMPC_HIP_OK;
}

bool solved(const nmpc_hip_riccati_solver * h, int)
{
  return h->solved;
}
} // namespace

extern "C"
{
  int nmpc_hip_riccati_default_config(nmpc_hip_riccati_config * cfg)
  {
    if(!cfg)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "cfg is NULL");
    }
    cfg->reg_type = 1;
    cfg->lambda = 1e-4;
    cfg->dlambda = 1.0;
    cfg->lambda_factor = 1.6;
    cfg->lambda_min = 1e-6;
    cfg->lambda_max = 1e10;
    cfg->with_input_constraint = 0;
    cfg->retry = 1;
    cfg->row_major = 0;
    return NMPC_HIP_OK;
  }

  int nmpc_hip_riccati_destroy(nmpc_hip_riccati_handle h)
  {
    if(!h)
    {
      return NMPC_HIP_OK;
    }
    h->close();
    delete h;
    return NMPC_HIP_OK;
  }

  int nmpc_hip_riccati_create(int state_dim, int input_dim, int horizon_steps, int batch, int device, nmpc_hip_riccati_handle * out)
  {
    if(!out)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "out is NULL");
    }
    *out = nullptr;
    if(state_dim < 1 || state_dim > NMPC_HIP_RICCATI_MAX_DIM)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "[Riccati] state_dim must be in 1 .. 16: " + std::to_string(state_dim));
    }
    if(input_dim < 0 || input_dim > NMPC_HIP_RICCATI_MAX_DIM)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "[Riccati] input_dim must be in 0 .. 16: " + std::to_string(input_dim));
    }
    if(horizon_steps < 1)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "[Riccati] horizon_steps must be positive: " + std::to_string(horizon_steps));
    }
    if(batch < 1)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "[Riccati] batch must be positive: " + std::to_string(batch));
    }
    NMPC_CAPI_CHECK(capi::checkDevice<Family>(device));
    auto * h = new nmpc_hip_riccati_solver();
    h->n = state_dim;
    h->m = input_dim;
    h->T = horizon_steps;
    h->B = batch;
    h->device = device;
    nmpc_hip_riccati_default_config(&h->cfg);
    auto cleanup = [&](int code) {
      nmpc_hip_riccati_destroy(h);
      return code;
    };
    int rc_ = h->open();
    if(rc_ != NMPC_HIP_OK)
    {
      return cleanup(rc_);
    }
    const size_t T = horizon_steps;
    auto A = [&](auto ** p, size_t count, const char * what) {
      if(rc_ == NMPC_HIP_OK)
      {
        rc_ = h->devAlloc(p, count, what);
      }
    };
    A(&h->d_dims, T, "the input dimensions");
    A(&h->d_out_d, h->layout().doubles, "the gains and the value function");
    A(&h->d_out_i, h->layout().ints, "the status fields");
    if(rc_ != NMPC_HIP_OK)
    {
      return cleanup(rc_);
    }
    // the largest shape asks for 37 760 bytes of LDS: below the 64 KB a kernel may use without asking
    static_assert(rc::ldsBytes(rc::kMaxDim, rc::kMaxDim) <= 64 * 1024, "riccati_wave_kernel would need hipFuncSetAttribute");
    *out = h;
    return NMPC_HIP_OK;
  }

  int nmpc_hip_riccati_set_config(nmpc_hip_riccati_handle h, const nmpc_hip_riccati_config * cfg)
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

  int nmpc_hip_riccati_get_config(nmpc_hip_riccati_handle h, nmpc_hip_riccati_config * cfg)
  {
    if(!h || !cfg)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    }
    *cfg = h->cfg;
    return NMPC_HIP_OK;
  }

  int nmpc_hip_riccati_set_input_dims(nmpc_hip_riccati_handle h, const int * dims)
  {
    if(!h)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "NULL handle");
    }
    if(!dims)
    {
      h->have_dims = false;
      return NMPC_HIP_OK;
    }
    for(int i = 0; i < h->T; i++)
    {
      if(dims[i] < 0 || dims[i] > h->m)
      {
        return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "[Riccati] dims[" + std::to_string(i) + "] = " + std::to_string(dims[i])
                                                       + " is outside 0 .. " + std::to_string(h->m));
      }
    }
    NMPC_CAPI_TRY(hipSetDevice(h->device));
    NMPC_CAPI_CHECK(h->waitForOtherStream());
    NMPC_CAPI_TRY(hipMemcpyAsync(h->d_dims, dims, static_cast<size_t>(h->T) * sizeof(int), hipMemcpyHostToDevice, h->stream));
    NMPC_CAPI_TRY(hipStreamSynchronize(h->stream));
    h->have_dims = true;
    return NMPC_HIP_OK;
  }

  int nmpc_hip_riccati_set_derivatives(nmpc_hip_riccati_handle h,
                                       const double * Fx,
                                       const double * Fu,
                                       const double * Lx,
                                       const double * Lu,
                                       const double * Lxx,
                                       const double * Luu,
                                       const double * Lxu,
                                       const double * Vx_T,
                                       const double * Vxx_T,
                                       int on_device)
  {
    if(!h || !Fx || !Lx || !Lxx || !Vx_T || !Vxx_T || (h->m > 0 && (!Fu || !Lu || !Luu || !Lxu)))
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    }
    NMPC_CAPI_TRY(hipSetDevice(h->device));
    NMPC_CAPI_CHECK(h->waitForOtherStream());
    const size_t B = h->B, n = h->n, m = h->m, S = h->B * h->T;
    int rc_ = NMPC_HIP_OK;
    auto set = [&](Input & in, const double * src, size_t count, const char * what) {
      if(rc_ == NMPC_HIP_OK)
      {
        rc_ = h->setInput(in, src, count, on_device, what);
      }
    };
    set(h->Fx, Fx, S * n * n, "Fx");
    set(h->Fu, Fu, S * n * m, "Fu");
    set(h->Lx, Lx, S * n, "Lx");
    set(h->Lu, Lu, S * m, "Lu");
    set(h->Lxx, Lxx, S * n * n, "Lxx");
    set(h->Luu, Luu, S * m * m, "Luu");
    set(h->Lxu, Lxu, S * n * m, "Lxu");
    set(h->VxT, Vx_T, B * n, "Vx_T");
    set(h->VxxT, Vxx_T, B * n * n, "Vxx_T");
    if(rc_ != NMPC_HIP_OK)
    {
      return rc_;
    }
    NMPC_CAPI_TRY(hipStreamSynchronize(h->stream));
    h->have_derivatives = true;
    return NMPC_HIP_OK;
  }

  int nmpc_hip_riccati_set_inputs(nmpc_hip_riccati_handle h,
                                  const double * U,
                                  const double * lower,
                                  const double * upper,
                                  int limits_per_step,
                                  int on_device)
  {
    if(!h || (h->m > 0 && (!U || !lower || !upper)))
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    }
    if(limits_per_step != 0 && limits_per_step != 1)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "[Riccati] limits_per_step must be 0 or 1");
    }
    NMPC_CAPI_TRY(hipSetDevice(h->device));
    NMPC_CAPI_CHECK(h->waitForOtherStream());
    const size_t m = h->m, S = h->B * h->T;
    const size_t lim = limits_per_step ? S * m : m;
    int rc_ = h->setInput(h->U, U, S * m, on_device, "U");
    if(rc_ == NMPC_HIP_OK)
    {
      rc_ = h->setInput(h->lower, lower, lim, on_device, "lower");
    }
    if(rc_ == NMPC_HIP_OK)
    {
      rc_ = h->setInput(h->upper, upper, lim, on_device, "upper");
    }
    if(rc_ != NMPC_HIP_OK)
    {
      return rc_;
    }
    NMPC_CAPI_TRY(hipStreamSynchronize(h->stream));
    h->limits_per_step = limits_per_step;
    h->have_inputs = true;
    return NMPC_HIP_OK;
  }

  int nmpc_hip_riccati_set_lambda(nmpc_hip_riccati_handle h, const double * lambda, const double * dlambda, int on_device)
  {
    if(!h)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "NULL handle");
    }
    NMPC_CAPI_TRY(hipSetDevice(h->device));
    NMPC_CAPI_CHECK(h->waitForOtherStream());
    int rc_ = h->setInput(h->lam, lambda, h->B, on_device, "lambda");
    if(rc_ == NMPC_HIP_OK)
    {
      rc_ = h->setInput(h->dlam, dlambda, h->B, on_device, "dlambda");
    }
    if(rc_ != NMPC_HIP_OK)
    {
      return rc_;
    }
    NMPC_CAPI_TRY(hipStreamSynchronize(h->stream));
    return NMPC_HIP_OK;
  }

  int nmpc_hip_riccati_solve_device(nmpc_hip_riccati_handle h, void * stream)
  {
    if(!h)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "NULL handle");
    }
    NMPC_CAPI_TRY(hipSetDevice(h->device));
    hipStream_t s = h->streamFor(stream);
    NMPC_CAPI_CHECK(h->waitBeforeLaunchOn(s)); // the previous solve writes the buffers this one writes
    return launchSolve(h, s);
  }

  int nmpc_hip_riccati_solve(nmpc_hip_riccati_handle h)
  {
    NMPC_CAPI_CHECK(nmpc_hip_riccati_solve_device(h, nullptr));
    return h->syncLast();
  }

  int nmpc_hip_riccati_synchronize(nmpc_hip_riccati_handle h)
  {
    if(!h)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "NULL handle");
    }
    NMPC_CAPI_TRY(hipSetDevice(h->device));
    return h->syncLast();
  }

  int nmpc_hip_riccati_field_bytes(nmpc_hip_riccati_handle h, int field, size_t * bytes)
  {
    if(!h || !bytes)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    }
    return fieldBytes(h, field, bytes);
  }

  int nmpc_hip_riccati_get(nmpc_hip_riccati_handle h, int field, void * out, size_t bytes, int on_device)
  {
    size_t want = 0;
    NMPC_CAPI_CHECK(capi::beginGet<Family>(h, field, out, bytes, &want, fieldBytes, solved, "get needs a solve"));
    return h->copyOut(out, fieldPtr(h, field), want, on_device, capi::kWaitForHostOnly);
  }

  int nmpc_hip_riccati_kernel_name(nmpc_hip_riccati_handle h, const char ** name)
  {
    if(!h || !name)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    }
    *name = "riccati_wave_kernel";
    return NMPC_HIP_OK;
  }

  int nmpc_hip_riccati_last_ms(nmpc_hip_riccati_handle h, float * ms)
  {
    if(!h || !ms)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    }
    return h->lastMs(ms, "last_ms needs a solve");
  }

  const char * nmpc_hip_riccati_last_error(void)
  {
    return capi::lastError<Family>().c_str();
  }
}
