// kernels_geometry.hip -- geometry set-up: the SetupGeo operator (setuplibceed.c:370-389): coordinates (P=2 per direction, :279,339)
// -> d x / d xi at the quadrature points -> qdata[10]; and the provenance kernels that let the fused apply recompute it
// (trilinear-map coefficients, the affine and the swept element classes).
#include "kernels_common.hpp"
#include "qfunctions_device.hpp"

namespace cps {

template <int Q>
__global__ __launch_bounds__(Geom<Q>::BLOCK) void k_setup_geo(const BasisTables tab,
                                                               const SetupGeoArgs a) {
  using G = Geom<Q>;
  constexpr int Q3 = G::Q3, TPE = G::TPE, EPB = G::EPB;
  __shared__ double sx[EPB][24];
  const int tid = threadIdx.x, el = tid / TPE, q = tid % TPE;
  const int e = blockIdx.x * EPB + el;
  const bool live = e < a.nelem;
  if (live && q < 8) {
    const uint32_t base = a.off_x[(size_t)e * 8 + q] & OFF_MASK;
#pragma unroll
    for (int c = 0; c < 3; c++) sx[el][c * 8 + q] = a.xcoord[base + c];
  }
  __syncthreads();
  if (!live || q >= Q3) return;
  const int i = q % Q, j = (q / Q) % Q, k = q / (Q * Q);
  // tables of the coordinate basis: B[q][p], G[q][p] with P = 2
  const double bi[2] = {tab.interp[i * 2], tab.interp[i * 2 + 1]}, gi[2] = {tab.grad[i * 2], tab.grad[i * 2 + 1]};
  const double bj[2] = {tab.interp[j * 2], tab.interp[j * 2 + 1]}, gj[2] = {tab.grad[j * 2], tab.grad[j * 2 + 1]};
  const double bk[2] = {tab.interp[k * 2], tab.interp[k * 2 + 1]}, gk[2] = {tab.grad[k * 2], tab.grad[k * 2 + 1]};
  double Jg[9];
#pragma unroll
  for (int c = 0; c < 3; c++) {
    double s0 = 0., s1 = 0., s2 = 0.;
#pragma unroll
    for (int cc = 0; cc < 2; cc++)
#pragma unroll
      for (int b = 0; b < 2; b++)
#pragma unroll
        for (int aa = 0; aa < 2; aa++) {
          const double x = sx[el][c * 8 + aa + 2 * b + 4 * cc];
          s0 += gi[aa] * bj[b] * bk[cc] * x;
          s1 += bi[aa] * gj[b] * bk[cc] * x;
          s2 += bi[aa] * bj[b] * gk[cc] * x;
        }
    Jg[0 * 3 + c] = s0; Jg[1 * 3 + c] = s1; Jg[2 * 3 + c] = s2;
  }
  double qd[10];
  qf_setup_geo(Jg, tab.qw[i] * tab.qw[j] * tab.qw[k], qd);
  double *out = a.qdata + (size_t)e * 10 * Q3 + q;
#pragma unroll
  for (int c = 0; c < 10; c++) out[c * Q3] = qd[c];
}

// Trilinear-map coefficients of every element (vertices in tensor order v = i + 2 j + 4 k, xi_v = +-1): what the fused
// kernel needs to recompute SetupGeo's output at a point (FusedGradArgs::geo).
__global__ void k_geo_coeffs(const uint32_t *off_x, const double *xcoord, double *geo, int nelem) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x, e = t / 3, c = t % 3;
  if (e >= nelem) return;
  double x[8];
#pragma unroll
  for (int v = 0; v < 8; v++) x[v] = xcoord[(off_x[(size_t)e * 8 + v] & OFF_MASK) + c];
  // monomial m of the bit set B (1: xi, 2: eta, 4: zeta): a = 1/8 sum_v x_v prod_{d in B} s_d(v)
  const int B[7] = {1, 2, 4, 3, 5, 6, 7};
  double *out = geo + (size_t)e * GEO_NCOEF + c * 7;
#pragma unroll
  for (int m = 0; m < 7; m++) {
    double s = 0.;
#pragma unroll
    for (int v = 0; v < 8; v++) s += (__popc((unsigned)(~v & B[m])) & 1) ? -x[v] : x[v];
    out[m] = 0.125 * s;
  }
}
hipError_t launch_geo_coeffs(const uint32_t *off_x, const double *xcoord, double *geo, int nelem, hipStream_t s) {
  if (nelem <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_geo_coeffs, dim3((unsigned)((3 * nelem + 255) / 256)), dim3(256), 0, s, off_x, xcoord, geo, nelem);
  return hipGetLastError();
}

__global__ void k_geo_affine(const double *geo, double *aff, int nelem, int *n_not_affine) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= nelem) return;
  const double *g = geo + (size_t)e * GEO_NCOEF;
  double lin = 0., nonlin = 0., Jg[9];
#pragma unroll
  for (int c = 0; c < 3; c++) {
#pragma unroll
    for (int m = 0; m < 7; m++) {
      const double v = fabs(g[c * 7 + m]);
      if (m < 3) lin = fmax(lin, v); else nonlin = fmax(nonlin, v);
    }
#pragma unroll
    for (int d = 0; d < 3; d++) Jg[d * 3 + c] = g[c * 7 + d];   // J[d][c] = d x_c / d xi_d, constant on the element
  }
  if (nonlin > 1e-14 * lin) atomicAdd(n_not_affine, 1);
  double qd[10];
  qf_setup_geo_rcp(Jg, 1.0, qd);     // {det J, dXdx}: the same arithmetic as the per-point recompute
#pragma unroll
  for (int i = 0; i < GEO_NAFF; i++) aff[(size_t)e * GEO_NAFF + i] = qd[i];
}
hipError_t launch_geo_affine(const double *geo, double *aff, int nelem, int *n_not_affine, hipStream_t s) {
  if (nelem <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_geo_affine, dim3((unsigned)((nelem + 255) / 256)), dim3(256), 0, s, geo, aff, nelem, n_not_affine);
  return hipGetLastError();
}

// axis < 0: COUNT -- count[s]++ for EVERY direction s the element is swept along (an axis-aligned brick qualifies for all three), count[3]++
// if for none; axis >= 0: FILL sw[] for that direction (the host has found every element to qualify for it).
__global__ void k_geo_swept(const double *geo, double *sw, int nelem, int *count, int axis) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= nelem) return;
  const double *g = geo + (size_t)e * GEO_NCOEF;   // [c][m], m: 0 xi, 1 eta, 2 zeta, 3 xi eta, 4 xi zeta, 5 eta zeta, 6 xi eta zeta
  double lin = 0.;
#pragma unroll
  for (int c = 0; c < 3; c++)
#pragma unroll
    for (int m = 0; m < 3; m++) lin = fmax(lin, fabs(g[c * 7 + m]));
  const double tol = 1e-13 * lin;
  int found = 3;
#pragma unroll
  for (int s = 0; s < 3; s++) {
    // monomials that contain direction s: the linear one, the two pairs with it, the triple
    const int p0 = s == 0 ? 3 : (s == 1 ? 3 : 4), p1 = s == 0 ? 4 : (s == 1 ? 5 : 5);
    bool ok = fabs(g[2 * 7 + s]) > tol;
#pragma unroll
    for (int m = 0; m < 7; m++)
      if (m != s) ok = ok && fabs(g[2 * 7 + m]) <= tol;                 // z depends on xi_s alone
#pragma unroll
    for (int c = 0; c < 2; c++)
      ok = ok && fabs(g[c * 7 + s]) <= tol && fabs(g[c * 7 + p0]) <= tol && fabs(g[c * 7 + p1]) <= tol && fabs(g[c * 7 + 6]) <= tol;
    if (ok && axis < 0) atomicAdd(count + s, 1);
    if (ok && found == 3) found = s;
  }
  if (axis < 0) { if (found == 3) atomicAdd(count + 3, 1); return; }
  found = axis;
  const int a = found == 0 ? 1 : 0, b = found == 2 ? 1 : 2, ab = (a == 0 && b == 1) ? 3 : ((a == 0 && b == 2) ? 4 : 5);
  double *o = sw + (size_t)e * GEO_NSWEPT;
  o[0] = g[a]; o[1] = g[b]; o[2] = g[ab];
  o[3] = g[7 + a]; o[4] = g[7 + b]; o[5] = g[7 + ab];
  const double zs = g[14 + found];
  o[6] = found == 1 ? -zs : zs;
  o[7] = 1. / zs;
}
hipError_t launch_geo_swept(const double *geo, double *sw, int nelem, int *count, int axis, hipStream_t s) {
  if (nelem <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_geo_swept, dim3((unsigned)((nelem + 255) / 256)), dim3(256), 0, s, geo, sw, nelem, count, axis);
  return hipGetLastError();
}

template <int Q>
static hipError_t setup_geo_t(const BasisTables &t, const SetupGeoArgs &a, hipStream_t s) {
  using G = Geom<Q>;
  if (a.nelem <= 0) return hipSuccess;
  hipLaunchKernelGGL((k_setup_geo<Q>), dim3((a.nelem + G::EPB - 1) / G::EPB), dim3(G::BLOCK), 0, s, t, a);
  return hipGetLastError();
}
hipError_t launch_setup_geo(int Q, const BasisTables &t, const SetupGeoArgs &a, hipStream_t s,
                            const char **name) {
#define CPS_SG(Qv) case Qv: *name = "setup_geo<Q=" #Qv ">"; return setup_geo_t<Qv>(t, a, s);
  switch (Q) { CPS_SG(2) CPS_SG(3) CPS_SG(4) CPS_SG(5) CPS_SG(6) CPS_SG(7) CPS_SG(8) }
  return hipErrorInvalidValue;
}

}  // namespace cps
