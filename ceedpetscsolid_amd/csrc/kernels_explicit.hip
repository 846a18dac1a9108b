// kernels_explicit.hip -- the explicit (central-difference, "leapfrog") time step of dynamics.ExplicitDynamics as ONE pass over its
// vectors: 7 streams of 8 B per dof with a load vector (x, vh read and written; r, f, m read), 6 without, against the about 17 of the
// same update composed from the calls of kernels_vector.hip.  HBM-bound, grid-stride (launch_stream); the kinetic-energy tally follows
// k_dot / k_dot_final: no atomics, every sum in a fixed order, so two calls give the same bits.  Rates: profiles/explicit.txt.
#include "kernels_common.hpp"

namespace cps {

// One step on the rows with m > 0 (include/ceed.h, CeedXVectorLeapfrogStep); a row with m <= 0 or m NaN -- a constrained row, the tail
// of a longer vector -- is neither written nor summed, whatever r, f, vh hold there.  Every operation is rounded on its own, in the
// order written (plain operators under contract(off): the intrinsics' bodies lie outside the pragma's reach and still fuse), so the
// NumPy form ceed.leapfrog_step_host gives the same bits in x and vh; the division is the correctly rounded one (no fast-math flag).
// part (null: no tally): part[blockIdx.x] = this workgroup's sum of m vm^2, vm the velocity at the step the residual belongs to.
__global__ __launch_bounds__(256) void k_leapfrog(double *__restrict__ x, double *__restrict__ vh, const double *__restrict__ r,
                                                  const double *__restrict__ f, const double *__restrict__ m, double load, double c1,
                                                  double c2, double dt, size_t n, double *__restrict__ part) {
#pragma clang fp contract(off)
  double ke = 0.;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const double mi = m[i];
    if (!(mi > 0.)) continue;
    const double ri = r[i];
    const double g = f ? load * f[i] - ri : -ri;
    const double q = g / mi;
    const double vo = vh[i];
    const double vn = c1 * vo + c2 * q;
    const double vm = 0.5 * (vo + vn);
    ke += mi * (vm * vm);
    vh[i] = vn;
    x[i] = x[i] + dt * vn;
  }
  if (!part) return;       // (uniform over the grid)
  for (int o = 32; o > 0; o >>= 1) ke += __shfl_down(ke, o, 64);
  __shared__ double wsum[4];
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = ke;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

// *out = 0.5 * the sum of part[0 .. nparts), in a fixed order (k_dot_final's)
__global__ __launch_bounds__(256) void k_leapfrog_final(const double *__restrict__ part, int nparts, double *__restrict__ out) {
  __shared__ double sh[256];
  double s = 0.;
  for (int i = threadIdx.x; i < nparts; i += 256) s += part[i];
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) *out = 0.5 * sh[0];
}

hipError_t launch_leapfrog(double *x, double *vh, const double *r, const double *f, const double *m, double load, double c1, double c2,
                           double dt, size_t n, double *part, double *out, hipStream_t s) {
  if (!n) return hipErrorInvalidValue;
  if (out && !part) return hipErrorInvalidValue;
  hipError_t e = launch_stream(k_leapfrog, n, s, x, vh, r, f, m, load, c1, c2, dt, n, out ? part : (double *)nullptr);
  if (e != hipSuccess || !out) return e;
  hipLaunchKernelGGL(k_leapfrog_final, dim3(1), dim3(256), 0, s, (const double *)part, (int)stream_grid(n).x, out);
  return hipGetLastError();
}

}  // namespace cps
