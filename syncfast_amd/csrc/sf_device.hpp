// sf_device.hpp -- how the .hip files launch a kernel and run a rocprim scan.
// Included by .hip files only (it needs the device compiler); the one place
// in csrc that spells the launch macro and the rocprim scan calls.
#pragma once
#include <hip/hip_runtime.h>

#include <iterator>

#include <rocprim/device/device_scan.hpp>

#include "sf_internal.hpp"

namespace sfi __attribute__((visibility("hidden"))) {

// One lane per item, 256 lanes per workgroup.
inline dim3 grid256(uint64_t n) { return dim3((unsigned)ceil_div(n, 256)); }

// hipGetLastError() answers the last failing HIP call of this thread, whatever
// it was, until it is read.  A launcher reads it after its launch, so it first
// clears what an earlier call left there -- one of ours whose status is
// ignored on purpose (hipHostUnregister in cleanup, an attribute probe), or
// the caller's, or another library's on the same thread -- which would
// otherwise be reported as the launch's failure (SF_ENODEV from a good launch).
inline void clear_stale_error() { (void)hipGetLastError(); }

// kernel<<<grid, block, 0, s>>>(args...), the arguments converted as at a
// direct call (a wrong count does not compile); SF_OK or the launch's error.
template <typename... P, typename... A>
inline int launch(void (*kernel)(P...), dim3 grid, dim3 block, hipStream_t s, A&&... args) {
  static_assert(sizeof...(P) == sizeof...(A), "one argument per kernel parameter");
  clear_stale_error();
  hipLaunchKernelGGL(kernel, grid, block, 0, s, static_cast<P>(args)...);
  return hip_err(hipGetLastError());
}

// rocprim's scans of n items on s, summed in the output's value type.  As in
// rocprim, a call with tmp == nullptr only sets `bytes` to the temporary the
// scan needs (the iterators are then typed nulls) and the call with that
// temporary does the work.  SF_OK, or SF_ENODEV with the sticky error cleared.
template <typename In, typename Out>
inline int scan_inclusive(void* tmp, size_t& bytes, In in, Out out, uint64_t n, hipStream_t s) {
  using T = typename std::iterator_traits<Out>::value_type;
  if (rocprim::inclusive_scan(tmp, bytes, in, out, (size_t)n, rocprim::plus<T>(), s) == hipSuccess) return SF_OK;
  (void)hipGetLastError();
  return SF_ENODEV;
}

template <typename In, typename Out>
inline int scan_exclusive(void* tmp, size_t& bytes, In in, Out out, typename std::iterator_traits<Out>::value_type init,
                          uint64_t n, hipStream_t s) {
  using T = typename std::iterator_traits<Out>::value_type;
  if (rocprim::exclusive_scan(tmp, bytes, in, out, init, (size_t)n, rocprim::plus<T>(), s) == hipSuccess) return SF_OK;
  (void)hipGetLastError();
  return SF_ENODEV;
}

}  // namespace sfi
