// Host scaffolding of the C-ABI translation units (nmpc_amd/csrc/*_capi.hip), stated once: the per-family error slot, fail(), the try
// macro, the device check, and the handle core of the toolbox solvers (BoxQP, GMRES, Riccati, FMPC step).  Host code only: no kernels.
//
// A family is a tag type that names its solver in messages:
//   struct Family { static constexpr const char *tag = "[Gmres]", *noun = "the GMRES solver", *prefix = "nmpc_hip_gmres"; };
// (noun is read by checkDevice, tag and prefix by the handle core; a family that uses neither has none).  Each translation unit is one
// family and calls its tag `Family`: that is the name NMPC_CAPI_TRY reads where it is used.
//
// The handle core answers three questions for every solver built on it ("The handle core"):
//   - a handle's memory is cleared on the handle's own stream, and the clear is waited for;
//   - a launch on a stream other than the last launch's waits for that last stream first;
//   - results are read on the stream of the last launch (the handle's own before any launch).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <string>
#include <vector>

#include <nmpc_hip_ddp.h> // nmpc_hip_status

/** Return NMPC_HIP_ERR_HIP, with the expression and the runtime's text in the family's error slot, unless `expr` is hipSuccess. */
#define NMPC_CAPI_TRY(expr)                                                                                              \
  do                                                                                                                     \
  {                                                                                                                      \
    hipError_t e_ = (expr);                                                                                              \
    if(e_ != hipSuccess)                                                                                                 \
    {                                                                                                                    \
      return ::nmpc_amd::hip::capi::fail<Family>(NMPC_HIP_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));   \
    }                                                                                                                    \
  } while(0)

/** Return the status of a call that has already filled the error slot, unless it is NMPC_HIP_OK. */
#define NMPC_CAPI_CHECK(expr)   \
  do                            \
  {                             \
    const int status_ = (expr); \
    if(status_ != NMPC_HIP_OK)  \
    {                           \
      return status_;           \
    }                           \
  } while(0)

namespace nmpc_amd
{
namespace hip
{
namespace capi
{
// Internal linkage throughout: the library is linked with default visibility and exports the C-ABI only, and every translation unit
// instantiates these for a family of its own.
namespace
{
/** The text behind nmpc_hip_<family>_last_error(): one per family and thread. */
template<class Family>
std::string & lastError()
{
  thread_local std::string text;
  return text;
}

template<class Family>
int fail(int code, const std::string & msg)
{
  lastError<Family>() = msg;
  return code;
}

/** Is there a device with this index?  Makes it the current one. */
template<class Family>
int checkDevice(int device)
{
  int n_dev = 0;
  const hipError_t e = hipGetDeviceCount(&n_dev);
  if(e != hipSuccess || n_dev <= 0)
  {
    return fail<Family>(NMPC_HIP_ERR_NO_DEVICE,
                        std::string("no HIP device available (") + hipGetErrorString(e) + "): " + Family::noun + " has no CPU fallback");
  }
  if(device < 0 || device >= n_dev)
  {
    return fail<Family>(NMPC_HIP_ERR_INVALID_ARGUMENT, "device index out of range");
  }
  NMPC_CAPI_TRY(hipSetDevice(device));
  return NMPC_HIP_OK;
}

/** One input array: the caller's device pointer, or the handle's staging copy of a host array. */
struct Input
{
  const double * ptr = nullptr; // what the kernel reads
  double * stage = nullptr; // owned by the handle (one of its allocs)
  size_t stage_count = 0;
};

constexpr bool kWaitAlways = true, kWaitForHostOnly = false; // HandleCore::copyOut

/** What a toolbox handle owns besides its solver's buffers; the handle struct derives from it. */
template<class Family>
struct HandleCore
{
  int device = 0;
  std::vector<void *> allocs;
  hipStream_t stream = nullptr; // the handle's own (non-blocking)
  hipStream_t last_stream = nullptr; // the stream of the last launch: `stream` or a caller's
  hipEvent_t ev0 = nullptr, ev1 = nullptr; // around the last launch
  bool timed = false;

  /** The stream and the events.  Before the first devAlloc, which clears on the stream. */
  int open()
  {
    if(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) != hipSuccess || hipEventCreate(&ev0) != hipSuccess
       || hipEventCreate(&ev1) != hipSuccess)
    {
      return fail<Family>(NMPC_HIP_ERR_HIP, "stream / event creation failed");
    }
    return NMPC_HIP_OK;
  }

  /** Zero device memory on the handle's stream, and wait: a hipMemset on the null stream returns before it has run and is not
      ordered against the copies that follow on the handle's (non-blocking) stream. */
  int clear(void * p, size_t bytes)
  {
    NMPC_CAPI_TRY(hipMemsetAsync(p, 0, bytes, stream));
    NMPC_CAPI_TRY(hipStreamSynchronize(stream));
    return NMPC_HIP_OK;
  }

  /** hipMalloc; a failure is NMPC_HIP_ERR_RUNTIME with the byte count, and leaves no sticky error behind. */
  int allocBytes(void ** p, size_t bytes, const char * what)
  {
    const hipError_t e = hipMalloc(p, bytes);
    if(e != hipSuccess)
    {
      *p = nullptr;
      (void)hipGetLastError();
      return fail<Family>(NMPC_HIP_ERR_RUNTIME, std::string(Family::tag) + " device allocation of " + std::to_string(bytes) + " bytes for "
                                                    + what + " failed: " + hipGetErrorString(e));
    }
    return NMPC_HIP_OK;
  }

  /** *p <- max(count, 1) zeroed elements that close() frees. */
  template<class T>
  int devAlloc(T ** p, size_t count, const char * what)
  {
    const size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
    NMPC_CAPI_CHECK(allocBytes(reinterpret_cast<void **>(p), bytes, what));
    allocs.push_back(*p);
    return clear(*p, bytes);
  }

  /** Wait for the work, then free what open() and devAlloc() made.  Safe on a handle whose create failed half way. */
  void close()
  {
    (void)hipSetDevice(device);
    if(last_stream)
    {
      (void)hipStreamSynchronize(last_stream);
    }
    if(stream)
    {
      (void)hipStreamSynchronize(stream);
    }
    for(void * p : allocs)
    {
      (void)hipFree(p);
    }
    if(ev0)
    {
      (void)hipEventDestroy(ev0);
    }
    if(ev1)
    {
      (void)hipEventDestroy(ev1);
    }
    if(stream)
    {
      (void)hipStreamDestroy(stream);
    }
  }

  /** The stream argument of a *_device entry point: NULL is the handle's own. */
  hipStream_t streamFor(void * caller_stream) const
  {
    return caller_stream ? static_cast<hipStream_t>(caller_stream) : stream;
  }

  /** The last launch reads and writes the buffers the next one on `s` uses: if it went to another stream, wait for it. */
  int waitBeforeLaunchOn(hipStream_t s)
  {
    if(last_stream && last_stream != s)
    {
      NMPC_CAPI_TRY(hipStreamSynchronize(last_stream));
    }
    return NMPC_HIP_OK;
  }

  /** Before a set_* copies on the handle's stream: a launch on a caller's stream may still be using the buffers. */
  int waitForOtherStream()
  {
    return waitBeforeLaunchOn(stream);
  }

  int syncLast()
  {
    NMPC_CAPI_TRY(hipStreamSynchronize(last_stream ? last_stream : stream));
    return NMPC_HIP_OK;
  }

  /** The event bracket of a launch on `s`: beginLaunch, the solver's memsets and kernels, endLaunch. */
  int beginLaunch(hipStream_t s)
  {
    NMPC_CAPI_TRY(hipEventRecord(ev0, s));
    return NMPC_HIP_OK;
  }

  int endLaunch(hipStream_t s)
  {
    NMPC_CAPI_TRY(hipEventRecord(ev1, s));
    last_stream = s;
    timed = true;
    return NMPC_HIP_OK;
  }

  /** Device time of the last launch; `needs` completes "<tag> <needs> first" when there was none. */
  int lastMs(float * ms, const char * needs)
  {
    if(!timed)
    {
      return fail<Family>(NMPC_HIP_ERR_NOT_SOLVED, std::string(Family::tag) + " " + needs + " first");
    }
    NMPC_CAPI_TRY(hipSetDevice(device));
    NMPC_CAPI_TRY(hipEventSynchronize(ev1));
    NMPC_CAPI_TRY(hipEventElapsedTime(ms, ev0, ev1));
    return NMPC_HIP_OK;
  }

  /** The second half of a get, after beginGet(): copy on the stream of the last launch and wait, for a device destination only
      with kWaitAlways. */
  int copyOut(void * out, const void * src, size_t bytes, int on_device, bool wait_always)
  {
    hipStream_t s = last_stream ? last_stream : stream;
    if(bytes > 0)
    {
      NMPC_CAPI_TRY(hipMemcpyAsync(out, src, bytes, on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
    }
    if(wait_always || !on_device)
    {
      NMPC_CAPI_TRY(hipStreamSynchronize(s));
    }
    return NMPC_HIP_OK;
  }

  /** `in` <- the caller's array of `count` doubles: in place (device) or through the staging copy (host), on the handle's stream. */
  int setInput(Input & in, const double * src, size_t count, int on_device, const char * what)
  {
    if(count == 0 || !src)
    {
      in.ptr = nullptr;
      return NMPC_HIP_OK;
    }
    if(on_device)
    {
      in.ptr = src;
      return NMPC_HIP_OK;
    }
    if(in.stage_count < count)
    {
      NMPC_CAPI_CHECK(devAlloc(&in.stage, count, what));
      in.stage_count = count;
    }
    NMPC_CAPI_TRY(hipMemcpyAsync(in.stage, src, count * sizeof(double), hipMemcpyHostToDevice, stream));
    in.ptr = in.stage;
    return NMPC_HIP_OK;
  }
};

/** The first half of a get (a free function: h may be NULL): the handle, the byte count against the family's field_bytes table, the
    family's "has this field been computed" test, and the device.  `needs` completes "<tag> <needs> first". */
template<class Family, class H>
int beginGet(const H * h, int field, const void * out, size_t bytes, size_t * want, int (*field_bytes)(const H *, int, size_t *),
             bool (*ready)(const H *, int), const char * needs)
{
  if(!h)
  {
    return fail<Family>(NMPC_HIP_ERR_INVALID_ARGUMENT, "NULL handle");
  }
  NMPC_CAPI_CHECK(field_bytes(h, field, want));
  if(bytes != *want || (!out && *want > 0))
  {
    return fail<Family>(NMPC_HIP_ERR_INVALID_ARGUMENT, std::string(Family::tag) + " get: bytes must equal " + Family::prefix
                                                           + "_field_bytes (" + std::to_string(*want) + "), got " + std::to_string(bytes));
  }
  if(!ready(h, field))
  {
    return fail<Family>(NMPC_HIP_ERR_NOT_SOLVED, std::string(Family::tag) + " " + needs + " first");
  }
  NMPC_CAPI_TRY(hipSetDevice(h->device));
  return NMPC_HIP_OK;
}
} // namespace
} // namespace capi
} // namespace hip
} // namespace nmpc_amd
