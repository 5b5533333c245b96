// Shared helpers for the gfx950 kernels of libyolo_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdio>
#include <cstdint>
#include "../../include/yolo_hip.h"
#include "env.hpp"

namespace yolo {

void set_error(const char* fmt, ...);

inline int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("%s: %s", what, hipGetErrorString(e));
    return YOLO_ERR_LAUNCH;
  }
  return YOLO_OK;
}

// ---- kernels with more dynamic LDS than the default 64 KB limit ----
// Kernel = the address of one kernel instantiation, named once per form. What these helpers learn is cached per process in
// function-local statics, not per device: ops.ensure_conv_workspace refuses a second device in one process.

// Raises Kernel's dynamic-LDS limit at first use; false (and the error text says why) when the runtime refused.
template <auto Kernel, size_t LDS_BYTES>
inline bool lds_limit_ok(const char* what) {
  static const hipError_t err =
      hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_BYTES);
  if (err != hipSuccess)
    set_error("%s: raising the dynamic LDS limit to %zu bytes failed: %s", what, (size_t)LDS_BYTES, hipGetErrorString(err));
  return err == hipSuccess;
}

template <auto Kernel, size_t LDS_BYTES, class Args>
inline int launch_lds(dim3 grid, dim3 block, hipStream_t st, const Args& args, const char* what) {
  if (!lds_limit_ok<Kernel, LDS_BYTES>(what)) return YOLO_ERR_LAUNCH;
  hipLaunchKernelGGL(Kernel, grid, block, LDS_BYTES, st, args);
  return check_launch(what);
}

// Workgroups of Kernel the chip holds at once (occupancy x CUs), asked once, after the limit is raised; 0 = a query failed
// (the call site has its own fallback).
template <auto Kernel, size_t LDS_BYTES>
inline int resident_workgroups(int block_threads, const char* what) {
  if (!lds_limit_ok<Kernel, LDS_BYTES>(what)) return 0;
  static const int resident = [block_threads] {
    int per_cu = 0, dev = 0, cus = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(Kernel), block_threads, LDS_BYTES) ==
            hipSuccess &&
        hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess &&
        per_cu > 0 && cus > 0)
      return per_cu * cus;
    return 0;
  }();
  return resident;
}

#define YOLO_REQUIRE(cond, ...)            \
  do {                                     \
    if (!(cond)) {                         \
      ::yolo::set_error(__VA_ARGS__);      \
      return YOLO_ERR_INVALID_ARG;         \
    }                                      \
  } while (0)

inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

// grid size for bandwidth-bound grid-stride kernels: enough blocks to fill 256 CUs x 8
inline int stream_grid(long long work_items, int block) {
  long long g = (work_items + block - 1) / block;
  if (g < 1) g = 1;
  if (g > 2048) g = 2048;
  return (int)g;
}

// Ordering rows by a score (the NMS visiting order, yolo_rank_desc, yolo_pr_curve) needs a TOTAL order: a NaN score compares
// false both ways, so a comparison sort that is handed such keys can leave its padding entries among the real rows, and a rank
// by counting gives every NaN row -- and the best ordinary row -- rank 0. np.argsort puts NaN LAST, so the reference's
// `argsort()[::-1]` visits NaN rows FIRST: the order key of a NaN score is +inf. Equal order keys (-0.0 and 0.0, two NaNs, NaN
// and +inf) go by index, the higher one first. The score that is stored and reported stays the row's own.
__device__ __forceinline__ double desc_order_key(double s) { return s != s ? __builtin_huge_val() : s; }

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ double wave_reduce_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_reduce_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

}  // namespace yolo
