// C-ABI of the batched BoxQP solver (declared in include/nmpc_hip_boxqp.h): handles, device-buffer ownership, the choice between
// the lane and the wave kernel, layout conversion at the boundary and the launches.  No CPU fallback exists: without the HIP runtime
// or a device every entry point that needs the GPU fails loudly.
#include <nmpc_hip_boxqp.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include <nmpc_amd/hip/boxqp_kernels.hpp>
#include <nmpc_amd/hip/capi_core.hpp>

namespace capi = nmpc_amd::hip::capi;
namespace bq = nmpc_amd::hip::boxqp;

static_assert(NMPC_HIP_BOXQP_MAX_DIM == bq::kMaxDim && NMPC_HIP_BOXQP_LANE_MAX_DIM == bq::kLaneMaxDim
                  && NMPC_HIP_BOXQP_TRACE_COLUMNS == bq::kTraceColumns && NMPC_HIP_BOXQP_AUTO_LANE_MAX_DIM <= NMPC_HIP_BOXQP_LANE_MAX_DIM,
              "nmpc_hip_boxqp.h and boxqp_kernels.hpp disagree");

namespace
{
struct Family
{
  static constexpr const char * tag = "[BoxQP]";
  static constexpr const char * noun = "the BoxQP solver";
  static constexpr const char * prefix = "nmpc_hip_boxqp";
};
constexpr auto fail = capi::fail<Family>;

enum Kernel
{
  kAuto = -1,
  kLane = 0,
  kWave = 1
};

/** The automatic choice (nmpc_hip_boxqp.h): a pure function of (var_dim, batch). */
Kernel autoKernel(int var_dim, int batch)
{
  return (var_dim <= NMPC_HIP_BOXQP_AUTO_LANE_MAX_DIM && batch >= NMPC_HIP_BOXQP_AUTO_LANE_MIN_BATCH) ? kLane : kWave;
}
} // namespace

struct nmpc_hip_boxqp_solver : capi::HandleCore<Family>
{
  int n = 0;
  size_t B = 0;
  nmpc_hip_boxqp_config cfg;
  Kernel pinned = kAuto;
  Kernel last = kAuto; // the kernel of the last solve (-1: none yet)
  // results, boundary layout
  double * d_x = nullptr; // [B][n]
  double * d_factor = nullptr; // [B][n][n]
  bq::Results res{};
  void * d_trace = nullptr; // not one of allocs: set_config frees and reallocates it
  // lane kernel: inputs, workspace and results [element][instance] (allocated for n <= 16)
  bq::LaneBuffers lane{};
  double *lane_H = nullptr, *lane_g = nullptr, *lane_lower = nullptr, *lane_upper = nullptr, *lane_x0 = nullptr;
  bool x_in_lane_layout = false, factor_in_lane_layout = false;
  // staging of solve()'s host arrays (allocated by the first solve())
  double *in_H = nullptr, *in_g = nullptr, *in_lower = nullptr, *in_upper = nullptr, *in_x0 = nullptr;
};

namespace
{
int validConfig(const nmpc_hip_boxqp_config & c)
{
  if(c.max_iter < 1)
  {
    return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "[BoxQP] max_iter must be positive");
  }
  if(!(std::isfinite(c.grad_thre) && std::isfinite(c.rel_improve_thre) && std::isfinite(c.min_step) && std::isfinite(c.armijo_param)
       && c.step_factor > 0 && c.step_factor < 1))
  {
    return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "[BoxQP] every threshold must be finite and step_factor inside (0, 1)");
  }
  if(c.trace_capacity < 0 || c.trace_capacity > (1 << 20))
  {
    return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "[BoxQP] trace_capacity out of range");
  }
  return NMPC_HIP_OK;
}

Kernel chosen(const nmpc_hip_boxqp_solver * h)
{
  return h->pinned != kAuto ? h->pinned : autoKernel(h->n, static_cast<int>(h->B));
}

bq::Params params(const nmpc_hip_boxqp_solver * h)
{
  const nmpc_hip_boxqp_config & c = h->cfg;
  return bq::Params{c.max_iter, c.grad_thre, c.rel_improve_thre, c.step_factor, c.min_step, c.armijo_param, c.trace_capacity};
}

unsigned blocksFor(size_t threads, unsigned block)
{
  return static_cast<unsigned>((threads + block - 1) / block);
}

/** The launches of one solve on stream s, inputs in the boundary layout on the device. */
int launchSolve(nmpc_hip_boxqp_solver * h, const double * dH, const double * dg, const double * dlo, const double * dup, const double * dx0,
                hipStream_t s)
{
  const size_t B = h->B;
  const int n = h->n;
  const Kernel k = chosen(h);
  NMPC_CAPI_CHECK(h->beginLaunch(s));
  if(k == kLane)
  {
    const unsigned block = 256;
    hipLaunchKernelGGL(bq::boxqp_ingest_kernel, dim3(blocksFor(B * n * n, block)), dim3(block), 0, s, dH, h->lane_H, B, n * n, n);
    hipLaunchKernelGGL(bq::boxqp_ingest_kernel, dim3(blocksFor(B * n, block)), dim3(block), 0, s, dg, h->lane_g, B, n, 0);
    hipLaunchKernelGGL(bq::boxqp_ingest_kernel, dim3(blocksFor(B * n, block)), dim3(block), 0, s, dlo, h->lane_lower, B, n, 0);
    hipLaunchKernelGGL(bq::boxqp_ingest_kernel, dim3(blocksFor(B * n, block)), dim3(block), 0, s, dup, h->lane_upper, B, n, 0);
    hipLaunchKernelGGL(bq::boxqp_ingest_kernel, dim3(blocksFor(B * n, block)), dim3(block), 0, s, dx0, h->lane_x0, B, n, 0);
    hipLaunchKernelGGL(bq::boxqp_lane_kernel, dim3(blocksFor(B, bq::kLaneBlock)), dim3(bq::kLaneBlock), 0, s, h->lane, h->res, params(h), n, B);
  }
  else
  {
    const bq::WaveBuffers wb{dH, dg, dlo, dup, dx0, h->d_x, h->d_factor};
    hipLaunchKernelGGL(bq::boxqp_wave_kernel, dim3(static_cast<unsigned>(B)), dim3(64), bq::waveLdsBytes(n), s, wb, h->res, params(h), n);
  }
  NMPC_CAPI_TRY(hipGetLastError());
  NMPC_CAPI_CHECK(h->endLaunch(s));
  h->last = k;
  h->x_in_lane_layout = h->factor_in_lane_layout = (k == kLane);
  return NMPC_HIP_OK;
}

int fieldBytes(const nmpc_hip_boxqp_solver * h, int field, size_t * bytes)
{
  const size_t B = h->B, n = h->n;
  switch(field)
  {
    case NMPC_HIP_BOXQP_FIELD_X:
      *bytes = B * n * sizeof(double);
      return NMPC_HIP_OK;
    case NMPC_HIP_BOXQP_FIELD_RETVAL:
    case NMPC_HIP_BOXQP_FIELD_ITER:
    case NMPC_HIP_BOXQP_FIELD_FACTORIZATION_NUM:
      *bytes = B * sizeof(int);
      return NMPC_HIP_OK;
    case NMPC_HIP_BOXQP_FIELD_FREE_MASK:
      *bytes = B * sizeof(unsigned long long);
      return NMPC_HIP_OK;
    case NMPC_HIP_BOXQP_FIELD_OBJ:
      *bytes = B * sizeof(double);
      return NMPC_HIP_OK;
    case NMPC_HIP_BOXQP_FIELD_FACTOR:
      *bytes = B * n * n * sizeof(double);
      return NMPC_HIP_OK;
    case NMPC_HIP_BOXQP_FIELD_TRACE:
      *bytes = B * h->cfg.trace_capacity * bq::kTraceColumns * sizeof(double);
      return NMPC_HIP_OK;
    default:
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "[BoxQP] unknown field");
  }
}

bool solved(const nmpc_hip_boxqp_solver * h, int)
{
  return h->last != kAuto;
}

/** X and FACTOR of a lane-kernel solve: the transposing store into the boundary layout, once, on the stream of that solve. */
int toBoundaryLayout(nmpc_hip_boxqp_solver * h, int field)
{
  const size_t B = h->B, n = h->n;
  if(field == NMPC_HIP_BOXQP_FIELD_X && h->x_in_lane_layout)
  {
    hipLaunchKernelGGL(bq::boxqp_egress_kernel, dim3(blocksFor(B * n, 256)), dim3(256), 0, h->last_stream, h->lane.x, h->d_x, B,
                       static_cast<int>(n));
    NMPC_CAPI_TRY(hipGetLastError());
    h->x_in_lane_layout = false;
  }
  if(field == NMPC_HIP_BOXQP_FIELD_FACTOR && h->factor_in_lane_layout)
  {
    hipLaunchKernelGGL(bq::boxqp_egress_kernel, dim3(blocksFor(B * n * n, 256)), dim3(256), 0, h->last_stream, h->lane.factor_out, h->d_factor,
                       B, static_cast<int>(n * n));
    NMPC_CAPI_TRY(hipGetLastError());
    h->factor_in_lane_layout = false;
  }
  return NMPC_HIP_OK;
}

const void * fieldPtr(const nmpc_hip_boxqp_solver * h, int field)
{
  switch(field)
  {
    case NMPC_HIP_BOXQP_FIELD_X:
      return h->d_x;
    case NMPC_HIP_BOXQP_FIELD_FACTOR:
      return h->d_factor;
    case NMPC_HIP_BOXQP_FIELD_RETVAL:
      return h->res.retval;
    case NMPC_HIP_BOXQP_FIELD_ITER:
      return h->res.iter;
    case NMPC_HIP_BOXQP_FIELD_FACTORIZATION_NUM:
      return h->res.factorization_num;
    case NMPC_HIP_BOXQP_FIELD_FREE_MASK:
      return h->res.free_mask;
    case NMPC_HIP_BOXQP_FIELD_OBJ:
      return h->res.obj;
    default:
      return h->d_trace;
  }
}
} // namespace

extern "C"
{
  int nmpc_hip_boxqp_default_config(nmpc_hip_boxqp_config * cfg)
  {
    if(!cfg)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "cfg is NULL");
    }
    cfg->max_iter = 500;
    cfg->grad_thre = 1e-8;
    cfg->rel_improve_thre = 1e-8;
    cfg->step_factor = 0.6;
    cfg->min_step = 1e-22;
    cfg->armijo_param = 0.1;
    cfg->trace_capacity = 0;
    return NMPC_HIP_OK;
  }

  int nmpc_hip_boxqp_destroy(nmpc_hip_boxqp_handle h)
  {
    if(!h)
    {
      return NMPC_HIP_OK;
    }
    h->close(); // waits for the work that writes the trace
    if(h->d_trace)
    {
      (void)hipFree(h->d_trace);
    }
    delete h;
    return NMPC_HIP_OK;
  }

  int nmpc_hip_boxqp_create(int var_dim, int batch, int device, nmpc_hip_boxqp_handle * out)
  {
    if(!out)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "out is NULL");
    }
    *out = nullptr;
    if(var_dim < 1 || var_dim > NMPC_HIP_BOXQP_MAX_DIM)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "[BoxQP] var_dim must be in 1 .. 64: " + std::to_string(var_dim));
    }
    if(batch < 1)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "[BoxQP] batch must be positive: " + std::to_string(batch));
    }
    NMPC_CAPI_CHECK(capi::checkDevice<Family>(device));
    auto * h = new nmpc_hip_boxqp_solver();
    h->n = var_dim;
    h->B = batch;
    h->device = device;
    nmpc_hip_boxqp_default_config(&h->cfg);
    auto cleanup = [&](int code) {
      nmpc_hip_boxqp_destroy(h);
      return code;
    };
    int rc = h->open();
    if(rc != NMPC_HIP_OK)
    {
      return cleanup(rc);
    }
    const size_t B = batch, n = var_dim;
    auto A = [&](auto ** p, size_t count, const char * what) {
      if(rc == NMPC_HIP_OK)
      {
        rc = h->devAlloc(p, count, what);
      }
    };
    A(&h->d_x, B * n, "x");
    A(&h->d_factor, B * n * n, "the factor");
    A(&h->res.retval, B, "retval");
    A(&h->res.iter, B, "iter");
    A(&h->res.factorization_num, B, "factorization_num");
    A(&h->res.free_mask, B, "the free masks");
    A(&h->res.obj, B, "obj");
    if(var_dim <= NMPC_HIP_BOXQP_LANE_MAX_DIM)
    {
      A(&h->lane_H, B * n * n, "the lane kernel's H");
      A(&h->lane_g, B * n, "the lane kernel's g");
      A(&h->lane_lower, B * n, "the lane kernel's lower");
      A(&h->lane_upper, B * n, "the lane kernel's upper");
      A(&h->lane_x0, B * n, "the lane kernel's initial_x");
      A(&h->lane.x, B * n, "the lane kernel's x");
      A(&h->lane.grad, B * n, "the lane kernel's gradient");
      A(&h->lane.dir, B * n, "the lane kernel's search direction");
      A(&h->lane.cand, B * n, "the lane kernel's candidate");
      A(&h->lane.fac, B * n * n, "the lane kernel's factor workspace");
      A(&h->lane.factor_out, B * n * n, "the lane kernel's factor");
      h->lane.H = h->lane_H;
      h->lane.g = h->lane_g;
      h->lane.lower = h->lane_lower;
      h->lane.upper = h->lane_upper;
      h->lane.x0 = h->lane_x0;
    }
    if(rc != NMPC_HIP_OK)
    {
      return cleanup(rc);
    }
    // (the wave kernel's LDS passes 64 KB at n = 64: that has to be requested per kernel and device)
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(bq::boxqp_wave_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                             static_cast<int>(bq::waveLdsBytes(NMPC_HIP_BOXQP_MAX_DIM)));
    if(e != hipSuccess)
    {
      return cleanup(fail(NMPC_HIP_ERR_HIP, std::string("hipFuncSetAttribute(boxqp_wave_kernel): ") + hipGetErrorString(e)));
    }
    *out = h;
    return NMPC_HIP_OK;
  }

  int nmpc_hip_boxqp_set_config(nmpc_hip_boxqp_handle h, const nmpc_hip_boxqp_config * cfg)
  {
    if(!h || !cfg)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    }
    NMPC_CAPI_CHECK(validConfig(*cfg));
    if(cfg->trace_capacity != h->cfg.trace_capacity)
    {
      NMPC_CAPI_TRY(hipSetDevice(h->device));
      if(h->last_stream)
      {
        NMPC_CAPI_TRY(hipStreamSynchronize(h->last_stream));
      }
      if(h->d_trace)
      {
        (void)hipFree(h->d_trace);
        h->d_trace = nullptr;
        h->res.trace = nullptr;
      }
      h->cfg.trace_capacity = 0;
      if(cfg->trace_capacity > 0)
      {
        const size_t bytes = h->B * cfg->trace_capacity * bq::kTraceColumns * sizeof(double);
        NMPC_CAPI_CHECK(h->allocBytes(&h->d_trace, bytes, "the trace"));
        NMPC_CAPI_CHECK(h->clear(h->d_trace, bytes));
        h->res.trace = static_cast<double *>(h->d_trace);
      }
    }
    h->cfg = *cfg;
    return NMPC_HIP_OK;
  }

  int nmpc_hip_boxqp_get_config(nmpc_hip_boxqp_handle h, nmpc_hip_boxqp_config * cfg)
  {
    if(!h || !cfg)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    }
    *cfg = h->cfg;
    return NMPC_HIP_OK;
  }

  int nmpc_hip_boxqp_solve_device(nmpc_hip_boxqp_handle h, const double * d_H, const double * d_g, const double * d_lower,
                                  const double * d_upper, const double * d_initial_x, void * stream)
  {
    if(!h || !d_H || !d_g || !d_lower || !d_upper)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    }
    NMPC_CAPI_TRY(hipSetDevice(h->device));
    return launchSolve(h, d_H, d_g, d_lower, d_upper, d_initial_x, h->streamFor(stream));
  }

  int nmpc_hip_boxqp_solve(nmpc_hip_boxqp_handle h, const double * H, const double * g, const double * lower, const double * upper,
                           const double * initial_x)
  {
    if(!h || !H || !g || !lower || !upper)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    }
    NMPC_CAPI_TRY(hipSetDevice(h->device));
    const size_t B = h->B, n = h->n;
    if(!h->in_H)
    {
      const struct
      {
        double ** p;
        size_t count;
        const char * what;
      } stage[] = {{&h->in_H, B * n * n, "the staging copy of H"},
                   {&h->in_g, B * n, "the staging copy of g"},
                   {&h->in_lower, B * n, "the staging copy of lower"},
                   {&h->in_upper, B * n, "the staging copy of upper"},
                   {&h->in_x0, B * n, "the staging copy of initial_x"}};
      int rc = NMPC_HIP_OK;
      for(const auto & a : stage)
      {
        if(rc == NMPC_HIP_OK)
        {
          rc = h->devAlloc(a.p, a.count, a.what);
        }
      }
      if(rc != NMPC_HIP_OK)
      {
        h->in_H = nullptr; // (what was allocated stays owned by the handle)
        return rc;
      }
    }
    NMPC_CAPI_CHECK(h->waitForOtherStream()); // a solve_device on another stream may still be writing the results
    NMPC_CAPI_TRY(hipMemcpyAsync(h->in_H, H, B * n * n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    NMPC_CAPI_TRY(hipMemcpyAsync(h->in_g, g, B * n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    NMPC_CAPI_TRY(hipMemcpyAsync(h->in_lower, lower, B * n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    NMPC_CAPI_TRY(hipMemcpyAsync(h->in_upper, upper, B * n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if(initial_x)
    {
      NMPC_CAPI_TRY(hipMemcpyAsync(h->in_x0, initial_x, B * n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    }
    NMPC_CAPI_CHECK(launchSolve(h, h->in_H, h->in_g, h->in_lower, h->in_upper, initial_x ? h->in_x0 : nullptr, h->stream));
    return h->syncLast();
  }

  int nmpc_hip_boxqp_synchronize(nmpc_hip_boxqp_handle h)
  {
    if(!h)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "NULL handle");
    }
    NMPC_CAPI_TRY(hipSetDevice(h->device));
    return h->syncLast();
  }

  int nmpc_hip_boxqp_field_bytes(nmpc_hip_boxqp_handle h, int field, size_t * bytes)
  {
    if(!h || !bytes)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    }
    return fieldBytes(h, field, bytes);
  }

  int nmpc_hip_boxqp_get(nmpc_hip_boxqp_handle h, int field, void * out, size_t bytes, int on_device)
  {
    size_t want = 0;
    NMPC_CAPI_CHECK(capi::beginGet<Family>(h, field, out, bytes, &want, fieldBytes, solved, "get needs a solve"));
    NMPC_CAPI_CHECK(toBoundaryLayout(h, field));
    return h->copyOut(out, fieldPtr(h, field), want, on_device, capi::kWaitAlways);
  }

  int nmpc_hip_boxqp_kernel_name(nmpc_hip_boxqp_handle h, const char ** name)
  {
    if(!h || !name)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    }
    *name = chosen(h) == kLane ? "boxqp_lane_kernel" : "boxqp_wave_kernel";
    return NMPC_HIP_OK;
  }

  int nmpc_hip_boxqp_set_kernel(nmpc_hip_boxqp_handle h, const char * kernel)
  {
    if(!h)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "NULL handle");
    }
    if(!kernel)
    {
      h->pinned = kAuto;
      return NMPC_HIP_OK;
    }
    if(std::strcmp(kernel, "lane") == 0)
    {
      if(h->n > NMPC_HIP_BOXQP_LANE_MAX_DIM)
      {
        return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "[BoxQP] the lane kernel exists for var_dim <= 16 only");
      }
      h->pinned = kLane;
      return NMPC_HIP_OK;
    }
    if(std::strcmp(kernel, "wave") == 0)
    {
      h->pinned = kWave;
      return NMPC_HIP_OK;
    }
    return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, std::string("[BoxQP] unknown kernel: ") + kernel + " (lane, wave or NULL)");
  }

  int nmpc_hip_boxqp_last_solve_ms(nmpc_hip_boxqp_handle h, float * ms)
  {
    if(!h || !ms)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    }
    return h->lastMs(ms, "last_solve_ms needs a solve");
  }

  const char * nmpc_hip_boxqp_last_error(void)
  {
    return capi::lastError<Family>().c_str();
  }
}
