// kernels_stress.hip -- stress recovery: the Cauchy stress THE RESIDUAL INTEGRATES (qfunctions_device.hpp, qf_stress; six components in
// the order xx, yy, zz, yz, xz, xy), from the displacement L-vector, sum-factorised, from ONE kernel template.
//
//   STRESS_POINTS  out[e][m][q]  = sigma_m(q)                                          at the Q^3 points, CEED_STRIDES_BACKEND layout
//   STRESS_NODAL   out[e][m][n]  = sum_q N_n(q) w det J(q) {sigma_0..5(q), 1}_m         element results of the lumped L2 projection: the
//                                  restriction's ordered transpose (k_rstr_transpose) sums them per node, the caller divides by m = 6
// The model (linElas, hyperSS, hyperFS) is a wave-uniform RUN-TIME switch in the arguments: three models as a template argument would
// triple the 56 kernels, and this is not the metric path.  No atomics here or in the sum.
//
// Mapping: k_mass's (kernel_line_pass.hpp) -- a LINE per lane, one slab [c][Q][Q][QP] per element in LDS, QP = Q | 1, in-place passes with
// a barrier between them, TPE lanes per element and EPB = 256 / TPE elements per workgroup.  Stages:
//   1  gather the three components through the offsets (flag bits stripped, the values read as they are: boundary values included)
//   2  x, y, z passes P -> Q on 3 P^2, 3 P Q, 3 Q^2 lines: the displacement at the Q^3 points
//   3  a lane per POINT (two per lane where Q^3 exceeds TPE: Q >= 6): the nine reference derivatives with the collocated table
//      (BasisTables::colo) from the three lines through the point, the ten qdata components of the point (coalesced: lanes run over
//      the points of a component), the physical gradient and the stress in registers
//   4  points: six coalesced stores.
//      nodal: barrier (every read of the interpolated field is done), w det J {sigma, 1} into the slab, now [7][Q][Q][QP] (32.3 KB at
//      Q = 8, static), three transposed passes Q -> P on 7 Q^2, 7 P Q, 7 P^2 lines (looped: more lines than lanes), coalesced stores.
// Per element the kernel moves 4 P^3 B of offsets, 24 P^3 B gathered, 80 Q^3 B of qdata and 48 Q^3 B (points) or 56 P^3 B (nodal) stored.
#include "kernel_diag_sf.hpp"      // CPS_DIAG_PQ: the one list of (P, Q) pairs
#include "kernel_line_pass.hpp"
#include "qfunctions_device.hpp"

namespace cps {

enum StressMode : int { STRESS_POINTS = 0, STRESS_NODAL = 1 };

template <int Q, int MODE> struct StressGeom {
  static constexpr int QP = MassGeom<Q>::QP, TPE = MassGeom<Q>::TPE, EPB = MassGeom<Q>::EPB;
  static constexpr int NC = MODE == STRESS_NODAL ? 7 : 3;            // components of the slab at its fullest
  static constexpr int NE = NC * Q * Q * QP;                         // doubles per element
  static constexpr int NPT = (Q * Q * Q + TPE - 1) / TPE;            // points per lane
  static_assert(sizeof(double) * ((size_t)EPB * NE + 2 * MAXN1D * MAXN1D) <= 64 * 1024, "static LDS");
};

template <int P, int Q, int MODE>
__global__ __launch_bounds__(256) void k_stress(const BasisTables tab, const StressArgs a) {
  using G = StressGeom<Q, MODE>;
  constexpr int QP = G::QP, TPE = G::TPE, EPB = G::EPB, NPT = G::NPT, P3 = P * P * P, Q3 = Q * Q * Q;
  constexpr int SK = Q * QP, SC = Q * Q * QP;             // pitch of k and of c in the slab
  constexpr int NV = MODE == STRESS_NODAL ? 7 : 6;        // values a point leaves
  __shared__ double sB[MAXN1D * MAXN1D];
  __shared__ double sD[MAXN1D * MAXN1D];
  __shared__ double slab[EPB * G::NE];
  const int tid = threadIdx.x, el = tid / TPE, t = tid % TPE;
  double *su = slab + (size_t)el * G::NE;
  const int e = blockIdx.x * EPB + el;
  const bool live = e < a.nelem;
  for (int i = tid; i < Q * P; i += 256) sB[i] = tab.interp[i];
  for (int i = tid; i < Q * Q; i += 256) sD[i] = tab.colo[i];
  if (live) {
    for (int n = t; n < P3; n += TPE) {
      const double *p = a.x + (a.offsets[(size_t)e * P3 + n] & OFF_MASK);
      const int i = n % P, j = (n / P) % P, k = n / (P * P);
#pragma unroll
      for (int c = 0; c < 3; c++) su[c * SC + k * SK + j * QP + i] = p[c];
    }
  }
  __syncthreads();
  if (live && t < 3 * P * P) {                            // x: (c, k, j)
    const int j = t % P, k = (t / P) % P, c = t / (P * P);
    mass_line<P, Q, false>(su + c * SC + k * SK + j * QP, 1, sB);
  }
  __syncthreads();
  if (live && t < 3 * P * Q) {                            // y: (c, k, a)
    const int aa = t % Q, k = (t / Q) % P, c = t / (P * Q);
    mass_line<P, Q, false>(su + c * SC + k * SK + aa, QP, sB);
  }
  __syncthreads();
  if (live && t < 3 * Q * Q) {                            // z: (c, b, a)
    const int aa = t % Q, bb = (t / Q) % Q, c = t / (Q * Q);
    mass_line<P, Q, false>(su + c * SC + bb * QP + aa, SK, sB);
  }
  __syncthreads();
  // a lane per point: reference derivatives from the three lines through it, qdata, the stress
  const Phys ph{a.nu, a.E, a.lambda, a.TwoMu};
  double val[NPT][NV];
#pragma unroll
  for (int r = 0; r < NPT; r++) {
    const int q = t + r * TPE;
    if (live && q < Q3) {
      const int i = q % Q, j = (q / Q) % Q, k = q / (Q * Q);
      double ug[9];
#pragma unroll
      for (int c = 0; c < 3; c++) {
        const double *s = su + c * SC;
        double d0 = 0., d1 = 0., d2 = 0.;
#pragma unroll
        for (int m = 0; m < Q; m++) {
          d0 += sD[i * Q + m] * s[k * SK + j * QP + m];
          d1 += sD[j * Q + m] * s[k * SK + m * QP + i];
          d2 += sD[k * Q + m] * s[m * SK + j * QP + i];
        }
        ug[0 * 3 + c] = d0; ug[1 * 3 + c] = d1; ug[2 * 3 + c] = d2;
      }
      const double *pq = a.qdata + (size_t)e * 10 * Q3 + q;
      double qd[10];
#pragma unroll
      for (int c = 0; c < 10; c++) qd[c] = pq[(size_t)c * Q3];
      double sg[6];
      qf_stress(a.model, ph, ug, qd, sg);
      if constexpr (MODE == STRESS_POINTS) {
        double *dst = a.out + (size_t)e * 6 * Q3 + q;
#pragma unroll
        for (int c = 0; c < 6; c++) dst[(size_t)c * Q3] = sg[c];
      } else {
#pragma unroll
        for (int c = 0; c < 6; c++) val[r][c] = qd[0] * sg[c];
        val[r][6] = qd[0];
      }
    }
  }
  if constexpr (MODE == STRESS_NODAL) {
    __syncthreads();                                      // every lane has read the interpolated field: the slab is overwritten
#pragma unroll
    for (int r = 0; r < NPT; r++) {
      const int q = t + r * TPE;
      if (live && q < Q3) {
        const int i = q % Q, j = (q / Q) % Q, k = q / (Q * Q);
#pragma unroll
        for (int c = 0; c < 7; c++) su[c * SC + k * SK + j * QP + i] = val[r][c];
      }
    }
    __syncthreads();
    if (live)
      for (int l = t; l < 7 * Q * Q; l += TPE) {          // z transposed: (c, b, a)
        const int aa = l % Q, bb = (l / Q) % Q, c = l / (Q * Q);
        mass_line<P, Q, true>(su + c * SC + bb * QP + aa, SK, sB);
      }
    __syncthreads();
    if (live)
      for (int l = t; l < 7 * P * Q; l += TPE) {          // y transposed: (c, k, a)
        const int aa = l % Q, k = (l / Q) % P, c = l / (P * Q);
        mass_line<P, Q, true>(su + c * SC + k * SK + aa, QP, sB);
      }
    __syncthreads();
    if (live)
      for (int l = t; l < 7 * P * P; l += TPE) {          // x transposed: (c, k, j)
        const int j = l % P, k = (l / P) % P, c = l / (P * P);
        mass_line<P, Q, true>(su + c * SC + k * SK + j * QP, 1, sB);
      }
    __syncthreads();
    if (live) {
      double *out = a.out + (size_t)e * 7 * P3;
      for (int o = t; o < 7 * P3; o += TPE) {
        const int c = o / P3, n = o % P3, i = n % P, j = (n / P) % P, k = n / (P * P);
        out[o] = su[c * SC + k * SK + j * QP + i];
      }
    }
  }
}

template <int P, int Q, int MODE>
static hipError_t stress_t(const BasisTables &t, const StressArgs &a, hipStream_t s) {
  if (a.nelem <= 0) return hipSuccess;
  constexpr int EPB = StressGeom<Q, MODE>::EPB;
  hipLaunchKernelGGL((k_stress<P, Q, MODE>), dim3((a.nelem + EPB - 1) / EPB), dim3(256), 0, s, t, a);
  return hipGetLastError();
}

hipError_t launch_stress(int P, int Q, bool nodal, const BasisTables &t, const StressArgs &a, hipStream_t s, const char **name) {
#define CPS_STRESS(Pv, Qv)                                                                             \
  if (P == Pv && Q == Qv) {                                                                            \
    *name = nodal ? "stress<P=" #Pv ",Q=" #Qv ",nodal>" : "stress<P=" #Pv ",Q=" #Qv ",points>";        \
    return nodal ? stress_t<Pv, Qv, STRESS_NODAL>(t, a, s) : stress_t<Pv, Qv, STRESS_POINTS>(t, a, s); \
  }
  CPS_DIAG_PQ(CPS_STRESS)
#undef CPS_STRESS
  return hipErrorInvalidValue;
}

}  // namespace cps
