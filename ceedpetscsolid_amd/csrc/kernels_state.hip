// kernels_state.hip -- the stored state (grad u) of a p-multigrid level that carries its OWN quadrature.
//
// A coarse level with coarse_quadrature="own" (solid.py) evaluates its Jacobian at Q_c = P_c + qextra Gauss points per direction
// instead of the fine level's Q.  Its stored state is the physical gradient of the FINE displacement at those points,
//   gradu[c][d] = sum_m dXdx[m][d] d u_c / d xi_m                                                  (hyperFS.h:215-220),
// i.e. what the residual QFunction would store if it were run with the basis (P_f, Q_c) -- without its physics, its transpose
// contraction, its E-vector and k_assemble: a streaming kernel of 12 P_f^3 B gathered and 72 Q_c^3 B stored per element
// (plus 4 P_f^3 B of offsets and the nine dXdx entries of the level's qdata, 72 Q_c^3 B).
//
// Mapping: a workgroup of 256 lanes owns EPB elements, an element owns TPE = 256 / EPB lanes (32 at Q_c = 2, 3, so no wave idles on a
// handful of points).  Three sum-factorised passes over LDS: x (B and G), y (B B, B G, G B), then z together with the product with dXdx
// and the stores, one point per lane and round.  The 1-D tables are staged into LDS once per workgroup.
#include "kernels_common.hpp"
#include "qfunctions_device.hpp"

namespace cps {

// lanes per element: the points rounded up to a power of two, at least half a wave; widened until the slabs of the 256 / TPE elements
// of a workgroup fit 80 KB of LDS (two workgroups per CU)
constexpr int state_tpe(int Q3, int NE, int NTAB) {
  int t = Q3 <= 32 ? 32 : (Q3 <= 64 ? 64 : (Q3 <= 128 ? 128 : 256));
  while (t < 256 && (size_t)(256 / t) * NE * sizeof(double) + NTAB * sizeof(double) > (size_t)80 * 1024) t *= 2;
  return t;
}
template <int PF, int QC> struct StateGeom {
  static constexpr int Q3 = cpow3(QC), F3 = cpow3(PF), F2 = PF * PF;
  static constexpr int N0 = 3 * F3;                // u        [c][k][j][i]
  static constexpr int N1H = 3 * F2 * QC;          // one of the two x-pass results [c][k][j][a]  (B u, G u)
  static constexpr int N2T = 3 * PF * QC * QC;     // one of the three y-pass results [c][k][b][a] (B B u, B G u, G B u)
  static constexpr int NA = N0 > 3 * N2T ? N0 : 3 * N2T;   // u and the y-pass results share their storage (never live together)
  static constexpr int NE = NA + 2 * N1H;          // doubles per element
  static constexpr int NTAB = 2 * QC * PF;
  static constexpr int TPE = state_tpe(Q3, NE, NTAB), EPB = 256 / TPE;
  static constexpr size_t LDS = sizeof(double) * ((size_t)NTAB + (size_t)EPB * NE);
  static_assert(LDS <= 160 * 1024, "one workgroup's slabs fit the LDS");
};

template <int PF, int QC>
__global__ __launch_bounds__(256) void k_state_at_points(const BasisTables tab, const StateArgs a) {
  using G = StateGeom<PF, QC>;
  constexpr int Q3 = G::Q3, F3 = G::F3, TPE = G::TPE, EPB = G::EPB, N1H = G::N1H, N2T = G::N2T;
  extern __shared__ double dyn[];
  double *sB = dyn, *sG = dyn + QC * PF;           // B[a][i], G[a][i]: QC x PF, the basis (P_f, Q_c)
  const int tid = threadIdx.x, el = tid / TPE, t = tid % TPE;
  double *su = dyn + G::NTAB + (size_t)el * G::NE, *t2 = su, *t1 = su + G::NA;
  const int e = blockIdx.x * EPB + el;
  const bool live = e < a.nelem;
  for (int i = tid; i < QC * PF; i += 256) { sB[i] = tab.interp[i]; sG[i] = tab.grad[i]; }
  if (live) {
    for (int n = t; n < F3; n += TPE) {
      const uint32_t off = a.offsets[(size_t)e * F3 + n];
      const uint32_t fl = a.mask_in ? (off >> OFF_FLAG_SHIFT) : 0u;
      const double *p = a.x + (off & OFF_MASK);
#pragma unroll
      for (int c = 0; c < 3; c++) su[c * F3 + n] = ((fl >> c) & 1u) ? 0. : p[c];
    }
  }
  __syncthreads();
  // x: T1b[line][a] = sum_i B[a][i] u[line][i], T1g with G; line = (c, k, j)
  if (live) {
    for (int o = t; o < N1H; o += TPE) {
      const int aa = o % QC, line = o / QC;
      const double *src = su + line * PF, *B = sB + aa * PF, *Gr = sG + aa * PF;
      double vb = 0., vg = 0.;
#pragma unroll
      for (int i = 0; i < PF; i++) { vb += B[i] * src[i]; vg += Gr[i] * src[i]; }
      t1[o] = vb; t1[N1H + o] = vg;
    }
  }
  __syncthreads();
  // y: T2[0] = B_y T1b, T2[1] = B_y T1g (the xi_0 derivative), T2[2] = G_y T1b (the xi_1 derivative); [c][k][b][a]
  if (live) {
    for (int o = t; o < N2T; o += TPE) {
      const int aa = o % QC, bb = (o / QC) % QC, ck = o / (QC * QC);
      const double *sb = t1 + ck * PF * QC + aa, *sg = sb + N1H, *B = sB + bb * PF, *Gr = sG + bb * PF;
      double v0 = 0., v1 = 0., v2 = 0.;
#pragma unroll
      for (int j = 0; j < PF; j++) { v0 += B[j] * sb[j * QC]; v1 += B[j] * sg[j * QC]; v2 += Gr[j] * sb[j * QC]; }
      t2[o] = v0; t2[N2T + o] = v1; t2[2 * N2T + o] = v2;
    }
  }
  __syncthreads();
  // z, the product with dXdx, the stores: one point per lane and round
  if (live) {
    for (int q = t; q < Q3; q += TPE) {
      const int ab = q % (QC * QC), kk = q / (QC * QC);
      const double *B = sB + kk * PF, *Gr = sG + kk * PF;
      double ug[9], qd[10], g[3][3];
#pragma unroll
      for (int c = 0; c < 3; c++) {
        const double *s0 = t2 + c * PF * QC * QC + ab;
        double d0 = 0., d1 = 0., d2 = 0.;
#pragma unroll
        for (int k = 0; k < PF; k++) {
          d0 += B[k] * s0[N2T + k * QC * QC]; d1 += B[k] * s0[2 * N2T + k * QC * QC]; d2 += Gr[k] * s0[k * QC * QC];
        }
        ug[0 * 3 + c] = d0; ug[1 * 3 + c] = d1; ug[2 * 3 + c] = d2;
      }
      const double *qp = a.qdata + (size_t)e * 10 * Q3 + q;
      qd[0] = 0.;
#pragma unroll
      for (int s = 1; s < 10; s++) qd[s] = qp[s * Q3];
      physical_grad(ug, qd, g);
      double *out = a.state_out + (size_t)e * 9 * Q3 + q;
#pragma unroll
      for (int c = 0; c < 3; c++)
#pragma unroll
        for (int k = 0; k < 3; k++) out[(3 * c + k) * Q3] = g[c][k];
    }
  }
}

template <int PF, int QC>
static hipError_t state_t(const BasisTables &t, const StateArgs &a, hipStream_t s) {
  using G = StateGeom<PF, QC>;
  if (a.nelem <= 0) return hipSuccess;
  static bool attr_set = false;
  if (!attr_set) {
    hipError_t er = hipFuncSetAttribute((const void *)k_state_at_points<PF, QC>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)G::LDS);
    if (er != hipSuccess) return er;
    attr_set = true;
  }
  hipLaunchKernelGGL((k_state_at_points<PF, QC>), dim3((a.nelem + G::EPB - 1) / G::EPB), dim3(256), G::LDS, s, t, a);
  return hipGetLastError();
}

hipError_t launch_state_at_points(int Pf, int Qc, const BasisTables &t, const StateArgs &a, hipStream_t s, const char **name) {
#define CPS_ST(F, C)                                     \
  if (Pf == F && Qc == C) {                              \
    *name = "state<Pf=" #F ",Qc=" #C ">";                \
    return state_t<F, C>(t, a, s);                       \
  }
  // fine P_f = 3 .. 8 (the ladders launch_transfer serves) x the Q_c = P_c + qextra <= 8 a level below it can have (P_c < P_f, qextra <= 2);
  // Q_c = 9 (P_c = 7 under P_f = 8 with qextra = 2) has no fused Jacobian kernel either (MAXN1D): a loud "not instantiated"
  CPS_ST(3, 2) CPS_ST(3, 3) CPS_ST(3, 4)
  CPS_ST(4, 2) CPS_ST(4, 3) CPS_ST(4, 4) CPS_ST(4, 5)
  CPS_ST(5, 2) CPS_ST(5, 3) CPS_ST(5, 4) CPS_ST(5, 5) CPS_ST(5, 6)
  CPS_ST(6, 2) CPS_ST(6, 3) CPS_ST(6, 4) CPS_ST(6, 5) CPS_ST(6, 6) CPS_ST(6, 7)
  CPS_ST(7, 2) CPS_ST(7, 3) CPS_ST(7, 4) CPS_ST(7, 5) CPS_ST(7, 6) CPS_ST(7, 7) CPS_ST(7, 8)
  CPS_ST(8, 2) CPS_ST(8, 3) CPS_ST(8, 4) CPS_ST(8, 5) CPS_ST(8, 6) CPS_ST(8, 7) CPS_ST(8, 8)
#undef CPS_ST
  return hipErrorInvalidValue;
}

}  // namespace cps
