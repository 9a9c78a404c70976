// C-ABI of the batched GMRES solver (declared in include/nmpc_hip_gmres.h): handles, device-buffer ownership, the ingest of A and
// the launch of gmres_wave_kernel.  No CPU fallback exists: without the HIP runtime or a device every entry point that needs the
// GPU fails loudly.
#include <nmpc_hip_gmres.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include <nmpc_amd/hip/gmres_kernels.hpp>

namespace gm = nmpc_amd::hip::gmres;

static_assert(NMPC_HIP_GMRES_MAX_DIM == gm::kMaxDim && NMPC_HIP_GMRES_HOUSEHOLDER_MAX_K == gm::kHouseholderMaxK,
              "nmpc_hip_gmres.h and gmres_kernels.hpp disagree");
static_assert(int(NMPC_HIP_GMRES_CONVERGED) == int(gm::kConverged) && int(NMPC_HIP_GMRES_K_MAX) == int(gm::kKMax)
                  && int(NMPC_HIP_GMRES_NON_FINITE) == int(gm::kNonFinite),
              "nmpc_hip_gmres.h and gmres_kernels.hpp disagree");

namespace
{
thread_local std::string g_gmres_last_error;

int fail(int code, const std::string & msg)
{
  g_gmres_last_error = msg;
  return code;
}

#define GM_TRY(expr)                                                                      \
  do                                                                                      \
  {                                                                                       \
    hipError_t e_ = (expr);                                                               \
    if(e_ != hipSuccess)                                                                  \
    {                                                                                     \
      return fail(NMPC_HIP_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));   \
    }                                                                                     \
  } while(0)

int checkDevice(int device)
{
  int n_dev = 0;
  const hipError_t e = hipGetDeviceCount(&n_dev);
  if(e != hipSuccess || n_dev <= 0)
  {
    return fail(NMPC_HIP_ERR_NO_DEVICE, std::string("no HIP device available (") + hipGetErrorString(e) +
                                            "): the GMRES solver has no CPU fallback");
  }
  if(device < 0 || device >= n_dev)
  {
    return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "device index out of range");
  }
  GM_TRY(hipSetDevice(device));
  return NMPC_HIP_OK;
}
} // namespace

struct nmpc_hip_gmres_solver
{
  int n = 0;
  size_t B = 0;
  int capacity = 0; // min(k_max_capacity, n)
  int device = 0;
  nmpc_hip_gmres_config cfg;
  int last_k_max = 0; // the clamped k_max of the last solve: the shapes of its fields (0: none yet)
  bool last_keep_basis = false;
  bool have_system = false;
  std::vector<void *> allocs;
  double * d_At = nullptr; // [B][n][n] the handle's transposed image
  const double * At = nullptr; // what the kernel reads: d_At, or the caller's device array (a_col_major = 1)
  double * d_stage = nullptr; // [B][n][n] row-major A from the host, allocated by the first such set_system
  double *d_b = nullptr, *d_x = nullptr, *d_basis = nullptr, *d_H = nullptr, *d_g = nullptr, *d_err = nullptr;
  int *d_iters = nullptr, *d_reorth = nullptr, *d_status = nullptr;
  hipStream_t stream = nullptr;
  hipStream_t last_stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  bool timed = false;
};

namespace
{
template<class T>
int devAlloc(nmpc_hip_gmres_solver * h, T ** p, size_t count, const char * what)
{
  const size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
  const hipError_t e = hipMalloc(reinterpret_cast<void **>(p), bytes);
  if(e != hipSuccess)
  {
    *p = nullptr;
    (void)hipGetLastError();
    return fail(NMPC_HIP_ERR_RUNTIME, std::string("[Gmres] device allocation of ") + std::to_string(bytes) + " bytes for " + what
                                          + " failed: " + hipGetErrorString(e));
  }
  h->allocs.push_back(*p);
  GM_TRY(hipMemset(*p, 0, bytes));
  return NMPC_HIP_OK;
}

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
  GM_TRY(hipEventRecord(h->ev0, s));
  GM_TRY(hipMemsetAsync(h->d_H, 0, h->B * (static_cast<size_t>(K) + 1) * K * sizeof(double), s)); // H_.setZero (Gmres.h:87)
  hipLaunchKernelGGL(gm::gmres_wave_kernel, dim3(static_cast<unsigned>(h->B)), dim3(gm::kWave), gm::waveLdsBytes(h->n, K, p.make_triangular != 0), s,
                     buf, p);
  GM_TRY(hipGetLastError());
  GM_TRY(hipEventRecord(h->ev1, s));
  h->last_k_max = K;
  h->last_keep_basis = h->cfg.keep_basis != 0;
  h->last_stream = s;
  h->timed = true;
  return NMPC_HIP_OK;
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
    (void)hipSetDevice(h->device);
    if(h->last_stream)
    {
      (void)hipStreamSynchronize(h->last_stream);
    }
    if(h->stream)
    {
      (void)hipStreamSynchronize(h->stream);
    }
    for(void * p : h->allocs)
    {
      (void)hipFree(p);
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
    {
      const int rc = checkDevice(device);
      if(rc != NMPC_HIP_OK)
      {
        return rc;
      }
    }
    auto * h = new nmpc_hip_gmres_solver();
    h->n = n;
    h->B = batch;
    h->capacity = std::min(k_max_capacity, n);
    h->device = device;
    nmpc_hip_gmres_default_config(&h->cfg);
    h->cfg.k_max = std::min(h->cfg.k_max, h->capacity);
    const size_t B = batch, N = n, K = h->capacity;
    int rc = NMPC_HIP_OK;
    auto A = [&](auto ** p, size_t count, const char * what) {
      if(rc == NMPC_HIP_OK)
      {
        rc = devAlloc(h, p, count, what);
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
    auto cleanup = [&](int code) {
      nmpc_hip_gmres_destroy(h);
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
    GM_TRY(hipSetDevice(h->device));
    const size_t B = h->B, n = h->n;
    if(h->last_stream && h->last_stream != h->stream)
    {
      GM_TRY(hipStreamSynchronize(h->last_stream)); // a solve_device on another stream may still be reading the system
    }
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
        GM_TRY(hipMemcpyAsync(h->d_At, A, B * n * n * sizeof(double), kind, h->stream));
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
        const int rc = devAlloc(h, &h->d_stage, B * n * n, "the staging copy of a row-major host A");
        if(rc != NMPC_HIP_OK)
        {
          return rc;
        }
      }
      GM_TRY(hipMemcpyAsync(h->d_stage, A, B * n * n * sizeof(double), kind, h->stream));
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
      GM_TRY(hipGetLastError());
      h->At = h->d_At;
    }
    GM_TRY(hipMemcpyAsync(h->d_b, b, B * n * sizeof(double), kind, h->stream));
    if(x0)
    {
      GM_TRY(hipMemcpyAsync(h->d_x, x0, B * n * sizeof(double), kind, h->stream));
    }
    else
    {
      GM_TRY(hipMemsetAsync(h->d_x, 0, B * n * sizeof(double), h->stream));
    }
    GM_TRY(hipStreamSynchronize(h->stream));
    h->have_system = true;
    return NMPC_HIP_OK;
  }

  int nmpc_hip_gmres_solve_device(nmpc_hip_gmres_handle h, void * stream)
  {
    if(!h)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "NULL handle");
    }
    GM_TRY(hipSetDevice(h->device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : h->stream;
    if(h->last_stream && h->last_stream != s)
    {
      GM_TRY(hipStreamSynchronize(h->last_stream)); // the previous solve wrote the x this one starts from
    }
    return launchSolve(h, s);
  }

  int nmpc_hip_gmres_solve(nmpc_hip_gmres_handle h)
  {
    const int rc = nmpc_hip_gmres_solve_device(h, nullptr);
    if(rc != NMPC_HIP_OK)
    {
      return rc;
    }
    GM_TRY(hipStreamSynchronize(h->stream));
    return NMPC_HIP_OK;
  }

  int nmpc_hip_gmres_synchronize(nmpc_hip_gmres_handle h)
  {
    if(!h)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "NULL handle");
    }
    GM_TRY(hipSetDevice(h->device));
    GM_TRY(hipStreamSynchronize(h->last_stream ? h->last_stream : h->stream));
    return NMPC_HIP_OK;
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
    if(!h)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "NULL handle");
    }
    size_t want = 0;
    {
      const int rc = fieldBytes(h, field, &want);
      if(rc != NMPC_HIP_OK)
      {
        return rc;
      }
    }
    if(bytes != want || !out)
    {
      return fail(NMPC_HIP_ERR_INVALID_ARGUMENT, "[Gmres] get: bytes must equal nmpc_hip_gmres_field_bytes (" + std::to_string(want) + "), got "
                                                     + std::to_string(bytes));
    }
    if(!h->last_k_max)
    {
      return fail(NMPC_HIP_ERR_NOT_SOLVED, "[Gmres] get needs a solve first");
    }
    GM_TRY(hipSetDevice(h->device));
    const void * src = nullptr;
    switch(field)
    {
      case NMPC_HIP_GMRES_FIELD_X:
        src = h->d_x;
        break;
      case NMPC_HIP_GMRES_FIELD_ITERS:
        src = h->d_iters;
        break;
      case NMPC_HIP_GMRES_FIELD_REORTH:
        src = h->d_reorth;
        break;
      case NMPC_HIP_GMRES_FIELD_STATUS:
        src = h->d_status;
        break;
      case NMPC_HIP_GMRES_FIELD_ERR_LIST:
        src = h->d_err;
        break;
      case NMPC_HIP_GMRES_FIELD_H:
        src = h->d_H;
        break;
      case NMPC_HIP_GMRES_FIELD_G:
        src = h->d_g;
        break;
      default:
        src = h->d_basis;
        break;
    }
    hipStream_t s = h->last_stream;
    GM_TRY(hipMemcpyAsync(out, src, want, on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
    GM_TRY(hipStreamSynchronize(s));
    return NMPC_HIP_OK;
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
    if(!h->timed)
    {
      return fail(NMPC_HIP_ERR_NOT_SOLVED, "[Gmres] last_ms needs a solve first");
    }
    GM_TRY(hipSetDevice(h->device));
    GM_TRY(hipEventSynchronize(h->ev1));
    GM_TRY(hipEventElapsedTime(ms, h->ev0, h->ev1));
    return NMPC_HIP_OK;
  }

  const char * nmpc_hip_gmres_last_error(void)
  {
    return g_gmres_last_error.c_str();
  }
}
