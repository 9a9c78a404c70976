// C-ABI of the batched GMRES solver (declared in include/nmpc_hip_gmres.h): handles, device-buffer ownership, the ingest of A and
// the launch of gmres_wave_kernel.  No CPU fallback exists: without the HIP runtime or a device every entry point that needs the
// GPU fails loudly.
#include <nmpc_hip_gmres.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include <nmpc_amd/hip/capi_core.hpp>
#include <nmpc_amd/hip/gmres_kernels.hpp>

namespace capi = nmpc_amd::hip::capi;
namespace gm = nmpc_amd::hip::gmres;

static_assert(NMPC_HIP_GMRES_MAX_DIM == gm::kMaxDim && NMPC_HIP_GMRES_HOUSEHOLDER_MAX_K == gm::kHouseholderMaxK,
              "nmpc_hip_gmres.h and gmres_kernels.hpp disagree");
static_assert(int(NMPC_HIP_GMRES_CONVERGED) == int(gm::kConverged) && int(NMPC_HIP_GMRES_K_MAX) == int(gm::kKMax)
                  && int(NMPC_HIP_GMRES_NON_FINITE) == int(gm::kNonFinite),
              "nmpc_hip_gmres.h and gmres_kernels.hpp disagree");

namespace
{
struct Family
{
  static constexpr const char * tag = "[Gmres]";
  static constexpr const char * noun = "the GMRES solver";
  static constexpr const char * prefix = "nmpc_hip_gmres";
};
constexpr auto fail = capi::fail<Family>;
} // namespace

struct nmpc_hip_gmres_solver : capi::HandleCore<Family>
{
  int n = 0;
  size_t B = 0;
  int capacity = 0; // min(k_max_capacity, n)
  nmpc_hip_gmres_config cfg;
  int last_k_max = 0; // the clamped k_max of the last solve: the shapes of its fields (0: none yet)
  bool last_keep_basis = false;
  bool have_system = false;
  double * d_At = nullptr; // [B][n][n] the handle's transposed image
  const double * At = nullptr; // what the kernel reads: d_At, or the caller's device array (a_col_major = 1)
  double * d_stage = nullptr; // [B][n][n] row-major A from the host, allocated by the first such set_system
  double *d_b = nullptr, *d_x = nullptr, *d_basis = nullptr, *d_H = nullptr, *d_g = nullptr, *d_err = nullptr;
  int *d_iters = nullptr, *d_reorth = nullptr, *d_status = nullptr;
};

namespace
{
int clampedKMax(const nmpc_hip_gmres_solver * h, int k_max)
{
  return std::min(k_max, h->n); // Gmres.h:73
}

int validConfig(const nmpc_hip_gmres_solver * h, const nmpc_hip_gmres_config & c)
{
  if(c.k_max < 1)
  {
    return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "[Gmres] k_max must be positive: " + std::to_string(c.k_max));
  }
  if(!(c.eps >= 0.0) || !std::isfinite(c.eps))
  {
    return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "[Gmres] eps must be finite and not negative");
  }
  const int k = clampedKMax(h, c.k_max);
  if(k > h->capacity)
  {
    return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "[Gmres] k_max " + std::to_string(k) + " (clamped to n) is above the handle's capacity "
                                                   + std::to_string(h->capacity));
  }
  if(!c.make_triangular && k > NMPC_HIP_GMRES_HOUSEHOLDER_MAX_K)
  {
    return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "[Gmres] the Householder variant (make_triangular = 0) takes a k_max (clamped to n) of at most "
                                                   + std::to_string(NMPC_HIP_GMRES_HOUSEHOLDER_MAX_K) + ": " + std::to_string(k));
  }
  return NMPC_HIP_OK;
}

int fieldBytes(const nmpc_hip_gmres_solver * h, int field, size_t * bytes)
{
  const size_t B = h->B, n = h->n;
  const size_t K = h->last_k_max ? h->last_k_max : clampedKMax(h, h->cfg.k_max);
  switch(field)
  {
    case NMPC_HIP_GMRES_FIELD_X:
      *bytes = B * n * sizeof(double);
      return NMPC_HIP_OK;
    case NMPC_HIP_GMRES_FIELD_ITERS:
    case NMPC_HIP_GMRES_FIELD_REORTH:
    case NMPC_HIP_GMRES_FIELD_STATUS:
      *bytes = B * sizeof(int);
      return NMPC_HIP_OK;
    case NMPC_HIP_GMRES_FIELD_ERR_LIST:
    case NMPC_HIP_GMRES_FIELD_G:
      *bytes = B * (K + 1) * sizeof(double);
      return NMPC_HIP_OK;
    case NMPC_HIP_GMRES_FIELD_H:
      *bytes = B * (K + 1) * K * sizeof(double);
      return NMPC_HIP_OK;
    case NMPC_HIP_GMRES_FIELD_BASIS:
      if(!(h->last_k_max ? h->last_keep_basis : h->cfg.keep_basis != 0))
      {
        return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "[Gmres] BASIS is kept only with keep_basis = 1");
      }
      *bytes = B * (K + 1) * n * sizeof(double);
      return NMPC_HIP_OK;
    default:
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "[Gmres] unknown field");
  }
}

int launchSolve(nmpc_hip_gmres_solver * h, hipStream_t s)
{
  if(!h->have_system)
  {
    return fail(NMPC_HIP_ERR_NOT_SOLVED, "[Gmres] solve needs a set_system first");
  }
  const int K = clampedKMax(h, h->cfg.k_max);
  const gm::Params p{h->n, K, h->cfg.eps, h->cfg.make_triangular != 0, h->cfg.apply_reorth != 0};
  const gm::Buffers buf{h->At, h->d_b, h->d_x, h->d_basis, h->d_H, h->d_g, h->d_err, h->d_iters, h->d_reorth, h->d_status};
  NMPC_CAPI_CHECK(h->beginLaunch(s));
  NMPC_CAPI_TRY(hipMemsetAsync(h->d_H, 0, h->B * (static_cast<size_t>(K) + 1) * K * sizeof(double), s)); // H_.setZero (Gmres.h:87)
  hipLaunchKernelGGL(gm::gmres_wave_kernel, dim3(static_cast<unsigned>(h->B)), dim3(gm::kWave), gm::waveLdsBytes(h->n, K, p.make_triangular != 0), s,
                     buf, p);
  NMPC_CAPI_TRY(hipGetLastError());
  NMPC_CAPI_CHECK(h->endLaunch(s));
  h->last_k_max = K;
  h->last_keep_basis = h->cfg.keep_basis != 0;
  return NMPC_HIP_OK;
}

bool solved(const nmpc_hip_gmres_solver * h, int)
{
  return h->last_k_max != 0;
}

const void * fieldPtr(const nmpc_hip_gmres_solver * h, int field)
{
  switch(field)
  {
    case NMPC_HIP_GMRES_FIELD_X:
      return h->d_x;
    case NMPC_HIP_GMRES_FIELD_ITERS:
      return h->d_iters;
    case NMPC_HIP_GMRES_FIELD_REORTH:
      return h->d_reorth;
    case NMPC_HIP_GMRES_FIELD_STATUS:
      return h->d_status;
    case NMPC_HIP_GMRES_FIELD_ERR_LIST:
      return h->d_err;
    case NMPC_HIP_GMRES_FIELD_H:
      return h->d_H;
    case NMPC_HIP_GMRES_FIELD_G:
      return h->d_g;
    default:
      return h->d_basis;
  }
}
} // namespace

extern "C"
{
  int nmpc_hip_gmres_default_config(nmpc_hip_gmres_config * cfg)
  {
    if(!cfg)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "cfg is NULL");
    }
    cfg->k_max = 100;
    cfg->eps = 1e-10;
    cfg->make_triangular = 1;
    cfg->apply_reorth = 1;
    cfg->keep_basis = 0;
    return NMPC_HIP_OK;
  }

  int nmpc_hip_gmres_destroy(nmpc_hip_gmres_handle h)
  {
    if(!h)
    {
      return NMPC_HIP_OK;
    }
    h->close();
    delete h;
    return NMPC_HIP_OK;
  }

  int nmpc_hip_gmres_create(int n, int batch, int k_max_capacity, int device, nmpc_hip_gmres_handle * out)
  {
    if(!out)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "out is NULL");
    }
    *out = nullptr;
    if(n < 1 || n > NMPC_HIP_GMRES_MAX_DIM)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "[Gmres] n must be in 1 .. 512: " + std::to_string(n));
    }
    if(batch < 1)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "[Gmres] batch must be positive: " + std::to_string(batch));
    }
    if(k_max_capacity < 1)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "[Gmres] k_max_capacity must be positive: " + std::to_string(k_max_capacity));
    }
    NMPC_CAPI_CHECK(capi::checkDevice<Family>(device));
    auto * h = new nmpc_hip_gmres_solver();
    h->n = n;
    h->B = batch;
    h->capacity = std::min(k_max_capacity, n);
    h->device = device;
    nmpc_hip_gmres_default_config(&h->cfg);
    h->cfg.k_max = std::min(h->cfg.k_max, h->capacity);
    auto cleanup = [&](int code) {
      nmpc_hip_gmres_destroy(h);
      return code;
    };
    int rc = h->open();
    if(rc != NMPC_HIP_OK)
    {
      return cleanup(rc);
    }
    const size_t B = batch, N = n, K = h->capacity;
    auto A = [&](auto ** p, size_t count, const char * what) {
      if(rc == NMPC_HIP_OK)
      {
        rc = h->devAlloc(p, count, what);
      }
    };
    A(&h->d_At, B * N * N, "A");
    A(&h->d_b, B * N, "b");
    A(&h->d_x, B * N, "x");
    A(&h->d_basis, B * (K + 1) * N, "the basis");
    A(&h->d_H, B * (K + 1) * K, "H");
    A(&h->d_g, B * (K + 1), "g");
    A(&h->d_err, B * (K + 1), "err_list");
    A(&h->d_iters, B, "iters");
    A(&h->d_reorth, B, "reorth");
    A(&h->d_status, B, "status");
    if(rc != NMPC_HIP_OK)
    {
      return cleanup(rc);
    }
    // (the Householder variant's LDS passes 64 KB from k_max = 88 on: that has to be requested per kernel and device)
    static_assert(NMPC_HIP_GMRES_HOUSEHOLDER_MAX_K <= NMPC_HIP_GMRES_MAX_DIM, "the largest LDS request is the Householder variant's");
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(gm::gmres_wave_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                             static_cast<int>(gm::waveLdsBytes(NMPC_HIP_GMRES_MAX_DIM, NMPC_HIP_GMRES_HOUSEHOLDER_MAX_K, false)));
    if(e != hipSuccess)
    {
      return cleanup(fail(NMPC_HIP_ERR_HIP, std::string("hipFuncSetAttribute(gmres_wave_kernel): ") + hipGetErrorString(e)));
    }
    *out = h;
    return NMPC_HIP_OK;
  }

  int nmpc_hip_gmres_set_config(nmpc_hip_gmres_handle h, const nmpc_hip_gmres_config * cfg)
  {
    if(!h || !cfg)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    }
    const int rc = validConfig(h, *cfg);
    if(rc != NMPC_HIP_OK)
    {
      return rc;
    }
    h->cfg = *cfg;
    return NMPC_HIP_OK;
  }

  int nmpc_hip_gmres_get_config(nmpc_hip_gmres_handle h, nmpc_hip_gmres_config * cfg)
  {
    if(!h || !cfg)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    }
    *cfg = h->cfg;
    return NMPC_HIP_OK;
  }

  int nmpc_hip_gmres_set_system(nmpc_hip_gmres_handle h, const double * A, const double * b, const double * x0, int on_device, int a_col_major)
  {
    if(!h || !A || !b)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    }
    NMPC_CAPI_TRY(hipSetDevice(h->device));
    const size_t B = h->B, n = h->n;
    NMPC_CAPI_CHECK(h->waitForOtherStream()); // a solve_device on another stream may still be reading the system
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    const double * row_major = nullptr; // device array to transpose
    if(a_col_major)
    {
      if(on_device)
      {
        h->At = A;
      }
      else
      {
        NMPC_CAPI_TRY(hipMemcpyAsync(h->d_At, A, B * n * n * sizeof(double), kind, h->stream));
        h->At = h->d_At;
      }
    }
    else if(on_device)
    {
      row_major = A;
    }
    else
    {
      if(!h->d_stage)
      {
        NMPC_CAPI_CHECK(h->devAlloc(&h->d_stage, B * n * n, "the staging copy of a row-major host A"));
      }
      NMPC_CAPI_TRY(hipMemcpyAsync(h->d_stage, A, B * n * n * sizeof(double), kind, h->stream));
      row_major = h->d_stage;
    }
    if(row_major)
    {
      const unsigned tiles = static_cast<unsigned>((n + gm::kTile - 1) / gm::kTile);
      for(size_t b0 = 0; b0 < B; b0 += 65535) // grid.z is bounded
      {
        const unsigned nb = static_cast<unsigned>(std::min<size_t>(65535, B - b0));
        hipLaunchKernelGGL(gm::gmres_ingest_kernel, dim3(tiles, tiles, nb), dim3(gm::kTile, 8), 0, h->stream, row_major + b0 * n * n,
                           h->d_At + b0 * n * n, static_cast<int>(n));
      }
      NMPC_CAPI_TRY(hipGetLastError());
      h->At = h->d_At;
    }
    NMPC_CAPI_TRY(hipMemcpyAsync(h->d_b, b, B * n * sizeof(double), kind, h->stream));
    if(x0)
    {
      NMPC_CAPI_TRY(hipMemcpyAsync(h->d_x, x0, B * n * sizeof(double), kind, h->stream));
    }
    else
    {
      NMPC_CAPI_TRY(hipMemsetAsync(h->d_x, 0, B * n * sizeof(double), h->stream));
    }
    NMPC_CAPI_TRY(hipStreamSynchronize(h->stream));
    h->have_system = true;
    return NMPC_HIP_OK;
  }

  int nmpc_hip_gmres_solve_device(nmpc_hip_gmres_handle h, void * stream)
  {
    if(!h)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "NULL handle");
    }
    NMPC_CAPI_TRY(hipSetDevice(h->device));
    hipStream_t s = h->streamFor(stream);
    NMPC_CAPI_CHECK(h->waitBeforeLaunchOn(s)); // the previous solve wrote the x this one starts from
    return launchSolve(h, s);
  }

  int nmpc_hip_gmres_solve(nmpc_hip_gmres_handle h)
  {
    NMPC_CAPI_CHECK(nmpc_hip_gmres_solve_device(h, nullptr));
    return h->syncLast();
  }

  int nmpc_hip_gmres_synchronize(nmpc_hip_gmres_handle h)
  {
    if(!h)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "NULL handle");
    }
    NMPC_CAPI_TRY(hipSetDevice(h->device));
    return h->syncLast();
  }

  int nmpc_hip_gmres_field_bytes(nmpc_hip_gmres_handle h, int field, size_t * bytes)
  {
    if(!h || !bytes)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    }
    return fieldBytes(h, field, bytes);
  }

  int nmpc_hip_gmres_get(nmpc_hip_gmres_handle h, int field, void * out, size_t bytes, int on_device)
  {
    size_t want = 0;
    NMPC_CAPI_CHECK(capi::beginGet<Family>(h, field, out, bytes, &want, fieldBytes, solved, "get needs a solve"));
    return h->copyOut(out, fieldPtr(h, field), want, on_device, capi::kWaitAlways);
  }

  int nmpc_hip_gmres_kernel_name(nmpc_hip_gmres_handle h, const char ** name)
  {
    if(!h || !name)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    }
    *name = "gmres_wave_kernel";
    return NMPC_HIP_OK;
  }

  int nmpc_hip_gmres_last_ms(nmpc_hip_gmres_handle h, float * ms)
  {
    if(!h || !ms)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    }
    return h->lastMs(ms, "last_ms needs a solve");
  }

  const char * nmpc_hip_gmres_last_error(void)
  {
    return capi::lastError<Family>().c_str();
  }
}
