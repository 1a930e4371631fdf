// host_errors.hpp -- the library's one set of error plumbing, for every translation unit behind the C ABI: a failing HIP
// call or a C++ exception becomes an AWV_ERR_* code and the text awv_last_error() returns.
#pragma once

#include <hip/hip_runtime.h>

#include <exception>
#include <new>
#include <string>

#include "allwave_hip.h"

// engine.hip: records awv_last_error() (one thread-local message for the whole library), returns code
int awv_internal_fail(int code, const std::string& msg);

#define AWV_TRY(expr)                                                                                             \
  do {                                                                                                            \
    const hipError_t _e = (expr);                                                                                 \
    if (_e != hipSuccess)                                                                                         \
      return awv_internal_fail(_e == hipErrorOutOfMemory ? AWV_ERR_OOM : AWV_ERR_HIP,                             \
                               std::string(#expr) + ": " + hipGetErrorString(_e));                                \
  } while (0)

// Nothing C++ may cross the C boundary: a std::bad_alloc / std::length_error out of a host-side container (a caller that hands
// over billions of pairs, a box short of memory) would otherwise reach the foreign caller as std::terminate -> abort().
#define AWV_GUARDED(body)                                                                                         \
  try {                                                                                                           \
    body                                                                                                          \
  } catch (const std::bad_alloc&) {                                                                               \
    return awv_internal_fail(AWV_ERR_OOM, "host memory exhausted");                                               \
  } catch (const std::exception& ex) {                                                                            \
    return awv_internal_fail(AWV_ERR_HIP, std::string("internal error: ") + ex.what());                           \
  } catch (...) {                                                                                                 \
    return awv_internal_fail(AWV_ERR_HIP, "internal error: unknown exception");                                   \
  }

// a null engine: without a GPU there is none to pass, so say that first (as awv_engine_create does)
inline int awv_internal_null_engine() {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return awv_internal_fail(AWV_ERR_NO_DEVICE, "no HIP device available: liballwave_hip has no CPU fallback");
  return awv_internal_fail(AWV_ERR_ARG, "null engine");
}
