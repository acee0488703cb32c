// train_common.h — the error plumbing of libgcd_amd_train.so, shared by its four sources (host code only).  The buffer,
// gcd_train_last_error and gcd_train_abi_version are defined once, in train_wgrad.hip.  An entry returns 2 for an argument
// it refuses (before any launch) and 1 for a launch that failed; gcd_train_last_error() then says why.
#pragma once
#include <hip/hip_runtime.h>

void gcd_train_set_error(const char* fmt, ...);

#define CHECK_ARG(cond, ...)            \
  do {                                  \
    if (!(cond)) {                      \
      gcd_train_set_error(__VA_ARGS__); \
      return 2;                         \
    }                                   \
  } while (0)
#define CHECK_LAUNCH(what)                                                       \
  do {                                                                           \
    hipError_t e_ = hipGetLastError();                                           \
    if (e_ != hipSuccess) {                                                      \
      gcd_train_set_error("%s: launch failed: %s", what, hipGetErrorString(e_)); \
      return 1;                                                                  \
    }                                                                            \
  } while (0)
