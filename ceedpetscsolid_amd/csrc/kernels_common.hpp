// kernels_common.hpp -- device building blocks shared by the gfx950 kernels.
//
// `Geom<Q>` is the point-per-lane mapping of the SET-UP kernels (k_setup_geo, k_diag_sf, k_pbdiag_sf): an
// element owns TPE lanes (Q^3 rounded up to a whole number of waves, or to a power of two when several
// elements share a wave) and a workgroup owns EPB elements.  The operator-apply kernel (kernel_fused_pencil.hpp)
// and, since round 5, the transfer kernels (k_transfer) have their own wave-level pencil mappings.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "kernels.hpp"

namespace cps {

#define CPS_DEV static __device__ __forceinline__

constexpr int cpow3(int n) { return n * n * n; }
constexpr int next_pow2(int n) { int p = 1; while (p < n) p *= 2; return p; }

template <int Q> struct Geom {
  static constexpr int Q3 = cpow3(Q);
  static constexpr int TPE = Q3 <= 32 ? next_pow2(Q3) : ((Q3 + 63) / 64) * 64;
  static constexpr int EPB = TPE >= 256 ? 1 : 256 / TPE;      // workgroups of 256 lanes
  static constexpr int BLOCK = TPE * EPB;
};

// The streaming kernels (HBM-bound, grid-stride): 256 lanes per workgroup, at most 2048 workgroups; nothing is launched for n = 0.
static inline dim3 stream_grid(size_t n) {
  size_t b = (n + 255) / 256;
  return dim3((unsigned)(b < 1 ? 1 : (b > 2048 ? 2048 : b)));
}
template <class... P, class... A>
static inline hipError_t launch_stream(void (*k)(P...), size_t n, hipStream_t s, A... args) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(k, stream_grid(n), dim3(256), 0, s, args...);
  return hipGetLastError();
}

}  // namespace cps
