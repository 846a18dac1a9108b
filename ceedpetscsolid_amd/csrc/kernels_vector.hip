// kernels_vector.hip -- vector utilities (HBM-bound, grid-stride: launch_stream), the reproducible dot product with the device-side
// scalars of a Krylov recurrence, the Chebyshev update, the clock probe and the device's CU count.
#include "kernel_node_sum.hpp"

namespace cps {

__global__ void k_set_value(double *v, size_t n, double val) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) v[i] = val;
}
__global__ void k_reciprocal(double *v, size_t n) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    if (fabs(v[i]) > 1e-300) v[i] = 1. / v[i];
}
__global__ void k_pointwise_mult(double *w, const double *x, const double *y, size_t n) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) w[i] = x[i] * y[i];
}
__global__ void k_axpby(double *y, double a, const double *x, double b, size_t n) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    y[i] = a * x[i] + (b == 0. ? 0. : b * y[i]);
}
__global__ void k_cheb_update(double *x, double *d, double *r, const double *r0, const double *t, const double *dinv, double c1,
                              double c2, int assign_x, size_t n) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    // r0: the right-hand side of a first step (r = b - t without a copy of b)
    cheb_dof(r0 ? r0[i] : r[i], t != nullptr, t ? t[i] : 0., (t || r0) && r, i, x, d, r, dinv, c1, c2, assign_x);
}
__global__ void k_masked_copy(double *dst, const double *src, const unsigned char *mask, size_t n) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    dst[i] = mask[i] ? 0. : src[i];
}
__global__ void k_waxpby(double *w, double a, const double *x, double b, const double *y, size_t n) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) w[i] = a * x[i] + b * y[i];
}
__global__ void k_dot(const double *x, const double *y, const double *w, size_t n, double *result) {
  double s = 0.;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    s += (w ? w[i] : 1.) * x[i] * y[i];
  for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
  __shared__ double part[4];
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
  __syncthreads();
  // per-block partial, summed in a fixed order by k_dot_final: the dot is reproducible run to run
  if (threadIdx.x == 0) result[1 + blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}
__global__ __launch_bounds__(256) void k_dot_final(double *result, int nparts, double *out) {
  __shared__ double sh[256];
  double s = 0.;
  for (int i = threadIdx.x; i < nparts; i += 256) s += result[1 + i];
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) { result[0] = sh[0]; if (out) *out = sh[0]; }
}
// scalars kept on the device (a Krylov recurrence without a host round trip per dot): s[dst] = scale * s[num] / s[den]
// (den < 0: no division); a non-positive denominator gives 0, which the host reads as "breakdown" afterwards
__global__ void k_scalar_div(double *s, int dst, int num, int den, double scale) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    const double d = den < 0 ? 1. : s[den];
    s[dst] = (den < 0 || d > 0.) ? scale * s[num] / d : 0.;
  }
}
// y = sa * (ia < 0 ? 1 : s[ia]) * x + sb * (ib < 0 ? 1 : s[ib]) * y
__global__ void k_axpby_dev(double *y, const double *s, int ia, double sa, const double *x, int ib, double sb, size_t n) {
  const double a = sa * (ia < 0 ? 1. : s[ia]), b = sb * (ib < 0 ? 1. : s[ib]);
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) y[i] = a * x[i] + b * y[i];
}

hipError_t launch_set_value(double *v, size_t n, double val, hipStream_t s) { return launch_stream(k_set_value, n, s, v, n, val); }
hipError_t launch_reciprocal(double *v, size_t n, hipStream_t s) { return launch_stream(k_reciprocal, n, s, v, n); }
hipError_t launch_pointwise_mult(double *w, const double *x, const double *y, size_t n, hipStream_t s) {
  return launch_stream(k_pointwise_mult, n, s, w, x, y, n);
}
hipError_t launch_waxpby(double *w, double a, const double *x, double b, const double *y, size_t n, hipStream_t s) {
  return launch_stream(k_waxpby, n, s, w, a, x, b, y, n);
}
hipError_t launch_axpby(double *y, double a, const double *x, double b, size_t n, hipStream_t s) {
  return launch_stream(k_axpby, n, s, y, a, x, b, n);
}
hipError_t launch_cheb_update(double *x, double *d, double *r, const double *r0, const double *t, const double *dinv, double c1, double c2,
                              int assign_x, size_t n, hipStream_t s) {
  return launch_stream(k_cheb_update, n, s, x, d, r, r0, t, dinv, c1, c2, assign_x, n);
}
hipError_t launch_masked_copy(double *dst, const double *src, const unsigned char *mask, size_t n, hipStream_t s) {
  return launch_stream(k_masked_copy, n, s, dst, src, mask, n);
}
hipError_t launch_axpby_dev(double *y, const double *sc, int ia, double sa, const double *x, int ib, double sb, size_t n, hipStream_t s) {
  return launch_stream(k_axpby_dev, n, s, y, sc, ia, sa, x, ib, sb, n);
}
hipError_t launch_dot(const double *x, const double *y, const double *w, size_t n, double *result_dev, hipStream_t s, double *out) {
  // result_dev: 1 + 2048 doubles ([0] the result, then the per-block partials); out: a second, device-side destination
  const dim3 g = n ? stream_grid(n) : dim3(1);
  hipLaunchKernelGGL(k_dot, g, dim3(256), 0, s, x, y, w, n, result_dev);
  hipLaunchKernelGGL(k_dot_final, dim3(1), dim3(256), 0, s, result_dev, (int)g.x, out);
  return hipGetLastError();
}
hipError_t launch_scalar_div(double *sc, int dst, int num, int den, double scale, hipStream_t s) {
  hipLaunchKernelGGL(k_scalar_div, dim3(1), dim3(64), 0, s, sc, dst, num, den, scale);
  return hipGetLastError();
}

// One wave that idles for `ticks` of the constant 100 MHz counter and reports how many SHADER clock cycles went by: the clock the
// chip runs at under whatever load the other streams put on it (a slow box and a slow build are then told apart: bench.py).
__global__ void k_clock_probe(long long *out, long long ticks) {
  if (threadIdx.x != 0) return;
  const long long t0 = wall_clock64(), c0 = clock64();
  long long t1 = t0;
  while (t1 - t0 < ticks) { __builtin_amdgcn_s_sleep(32); t1 = wall_clock64(); }
  out[0] = clock64() - c0; out[1] = t1 - t0;
}
hipError_t launch_clock_probe(long long *out, int spin_us, hipStream_t s) {
  hipLaunchKernelGGL(k_clock_probe, dim3(1), dim3(64), 0, s, out, (long long)spin_us * 100);
  return hipGetLastError();
}

int device_cu_count() {
  static int ncu = 0;
  if (!ncu) {
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return -1;
    ncu = prop.multiProcessorCount;
  }
  return ncu;
}

}  // namespace cps
