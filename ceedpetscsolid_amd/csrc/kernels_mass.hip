// kernels_mass.hip -- the mass operator v = c B^T (w det J) B u of the elastodynamic solve (QFunction "Mass": v = c qdata[0] u
// at every point, INTERP in and out, 3 components) and its diagonal, from ONE kernel template.
//
//   MASS_APPLY  evec[e][n][c] = c sum_q B(q,n) wdetJ(e,q) sum_m B(q,m) u_c(m)      gather, three passes, one multiply, three passes back
//   MASS_DIAG   evec[e][n][c] = c sum_q B(q,n)^2 wdetJ(e,q)   (every c)            the transposed half alone, on wdetJ, with the host's
//                                                                                 entry-wise SQUARED table in BasisTables::interp
// launch_assemble() then sums the element results per node in element order (no atomics here or there).  Per element the kernel moves
// 4 P^3 B of offsets, 24 P^3 B gathered, 8 Q^3 B of qdata (component 0 only: Q^3 contiguous doubles) and 24 P^3 B stored.
//
// Mapping: a LINE per lane.  The slab of an element is one array [c][Q][Q][QP] in LDS, QP = Q | 1 (an odd row pitch: the lanes of the
// x passes, QP doubles apart, then fall on different banks), 3 Q^2 QP doubles -- 13.8 KB at Q = 8, static.  Every pass is IN PLACE: a
// lane reads the P (or Q) entries of its line into registers, multiplies by the 1-D table and writes Q (or P) entries back into the
// same line, which no other lane touches in that pass (Q >= P: the longer line always fits); a barrier separates the passes.
//   x  lines (c, k, j)  k, j < P     y  lines (c, k, a)  k < P, a < Q     z  lines (c, b, a)  b, a < Q
// The z pass, the product with c wdetJ (read here, coalesced: lanes run over a then b) and the transposed z pass are ONE stage on the
// lane's registers; then y^T, x^T, and coalesced stores of the [P^3][3] block.  The fullest stage has 3 Q^2 lines.
// Packing: an element owns TPE = 3 Q^2 rounded up to a power of two lanes (16, 32, 64, 128, 128, 256, 256 for Q = 2 .. 8), a workgroup of
// 256 lanes EPB = 256 / TPE elements (16, 8, 4, 2, 2, 1, 1), so that no wave idles on a handful of lines; LDS per workgroup 5.1, 5.7,
// 8.2, 6.5, 12.6, 8.7, 14.3 KB with the table.  The 1-D table (BasisTables kernarg) is staged into LDS once per workgroup.
#include "kernel_diag_sf.hpp"      // CPS_DIAG_PQ: the one list of (P, Q) pairs
#include "kernel_line_pass.hpp"    // MassGeom, mass_line: the packing and the in-place line pass, shared with k_stress

namespace cps {

enum MassMode : int { MASS_APPLY = 0, MASS_DIAG = 1, MASS_APPLY_RHO = 2, MASS_DIAG_RHO = 3 };

template <int P, int Q, int MODE>
__global__ __launch_bounds__(256) void k_mass(const BasisTables tab, const MassArgs a) {
  using G = MassGeom<Q>;
  constexpr int QP = G::QP, TPE = G::TPE, EPB = G::EPB, P3 = P * P * P, Q3 = Q * Q * Q;
  constexpr int NC = MODE == MASS_APPLY ? 3 : 1;          // the diagonal is the same for the three components: one is formed
  constexpr int SK = Q * QP, SC = Q * Q * QP;             // pitch of k and of c in the slab
  __shared__ double sB[MAXN1D * MAXN1D];
  __shared__ double slab[EPB * G::NE];
  const int tid = threadIdx.x, el = tid / TPE, t = tid % TPE;
  double *su = slab + (size_t)el * G::NE;
  const int e = blockIdx.x * EPB + el;
  const bool live = e < a.nelem;
  for (int i = tid; i < Q * P; i += 256) sB[i] = tab.interp[i];
  if constexpr (MODE == MASS_APPLY) {
    if (live) {
      for (int n = t; n < P3; n += TPE) {
        const uint32_t off = a.offsets[(size_t)e * P3 + n];
        const uint32_t fl = a.mask_in ? (off >> OFF_FLAG_SHIFT) : 0u;
        const double *p = a.x + (off & OFF_MASK);
        const int i = n % P, j = (n / P) % P, k = n / (P * P);
#pragma unroll
        for (int c = 0; c < 3; c++) su[c * SC + k * SK + j * QP + i] = ((fl >> c) & 1u) ? 0. : p[c];
      }
    }
    __syncthreads();
    if (live && t < 3 * P * P) {                          // x: (c, k, j)
      const int j = t % P, k = (t / P) % P, c = t / (P * P);
      mass_line<P, Q, false>(su + c * SC + k * SK + j * QP, 1, sB);
    }
    __syncthreads();
    if (live && t < 3 * P * Q) {                          // y: (c, k, a)
      const int aa = t % Q, k = (t / Q) % P, c = t / (P * Q);
      mass_line<P, Q, false>(su + c * SC + k * SK + aa, QP, sB);
    }
  }
  __syncthreads();
  // z, the product with c wdetJ at the Q points of the line, z transposed: (c, b, a)
  if (live && t < NC * Q * Q) {
    const int ab = t % (Q * Q), aa = ab % Q, bb = ab / Q, c = t / (Q * Q);
    double *s = su + c * SC + bb * QP + aa;
    const double *wq = a.qdata + (size_t)e * 10 * Q3 + ab;
    double v[Q];
#pragma unroll
    for (int kk = 0; kk < Q; kk++) v[kk] = a.coef * wq[kk * Q * Q];
    if constexpr (MODE == MASS_APPLY) {
      double in[P];
#pragma unroll
      for (int k = 0; k < P; k++) in[k] = s[k * SK];
#pragma unroll
      for (int kk = 0; kk < Q; kk++) {
        double u = 0.;
#pragma unroll
        for (int k = 0; k < P; k++) u += sB[kk * P + k] * in[k];
        v[kk] *= u;
      }
    }
#pragma unroll
    for (int k = 0; k < P; k++) {
      double r = 0.;
#pragma unroll
      for (int kk = 0; kk < Q; kk++) r += sB[kk * P + k] * v[kk];
      s[k * SK] = r;
    }
  }
  __syncthreads();
  if (live && t < NC * P * Q) {                           // y transposed: (c, k, a)
    const int aa = t % Q, k = (t / Q) % P, c = t / (P * Q);
    mass_line<P, Q, true>(su + c * SC + k * SK + aa, QP, sB);
  }
  __syncthreads();
  if (live && t < NC * P * P) {                           // x transposed: (c, k, j)
    const int j = t % P, k = (t / P) % P, c = t / (P * P);
    mass_line<P, Q, true>(su + c * SC + k * SK + j * QP, 1, sB);
  }
  __syncthreads();
  if (live) {
    double *out = a.evec + (size_t)e * P3 * 3;
    for (int o = t; o < 3 * P3; o += TPE) {
      const int n = o / 3, c = o % 3, i = n % P, j = (n / P) % P, k = n / (P * P);
      if constexpr (MODE == MASS_APPLY) out[o] = su[c * SC + k * SK + j * QP + i];     // (masked rows: launch_assemble() takes the row flags)
      else {
        const uint32_t fl = a.mask_out ? (a.offsets[(size_t)e * P3 + n] >> OFF_FLAG_SHIFT) : 0u;
        out[o] = ((fl >> c) & 1u) ? 0. : su[k * SK + j * QP + i];
      }
    }
  }
}

// ---- the density field: MODE = MASS_APPLY_RHO, MASS_DIAG_RHO (QFunction "MassField") ----------------------------------------------------
//   MASS_APPLY_RHO  evec[e][n][c] = c0 sum_q B(q,n) rho_h(e,q) wdetJ(e,q) sum_m B(q,m) u_c(m)
//   MASS_DIAG_RHO   evec[e][n][c] = c0 sum_q B(q,n)^2 rho_h(e,q) wdetJ(e,q)   (every c)
//   rho_h(e,q) = sum_m N_m(q) rho(e,m): the density interpolated with the table of u, gathered from a scalar vector through offsets of
//   its own (MassFieldArgs: plain indices, no flags, no factor 3) -- a continuous nodal field and an element-discontinuous one alike.
// The same name and template parameters as the kernel above with a third argument, the field's own struct, so that MassArgs and with it
// the argument block, the code, the registers and the LDS of the MODE 0 / 1 instantiations stay what they were.
// The apply carries rho as a FOURTH component of the slab, [4][Q][Q][QP] (18.4 KB at Q = 8), through the same x and y passes: 4 P^2 and
// 4 P Q lines can exceed the TPE lanes of an element (Q = 3: 36 lines on 32 lanes), so these two passes LOOP over the lines, as k_stress
// loops its seven components.  The z stage forms rho at the Q points of its line from the P slab entries of component 3, which no lane
// writes in that stage (the three lanes c of a point (b, a) each form it: P Q multiply-adds against a z pass of rho and a barrier more),
// and folds it into c0 wdetJ; from there on the kernel is the one above.  The diagonal carries rho ALONE, one component, with the plain
// table on the way to the points and the squared table (squared here while staging: the same bits as the host's) on the way back.
template <int P, int Q, int MODE>
__global__ __launch_bounds__(256) void k_mass(const BasisTables tab, const MassArgs a, const MassFieldArgs f) {
  static_assert(MODE == MASS_APPLY_RHO || MODE == MASS_DIAG_RHO, "the modes with a density field");
  using G = MassGeom<Q>;
  constexpr bool APPLY = MODE == MASS_APPLY_RHO;
  constexpr int QP = G::QP, TPE = G::TPE, EPB = G::EPB, P3 = P * P * P, Q3 = Q * Q * Q;
  constexpr int NC = APPLY ? 3 : 1;                       // components of the transposed half
  constexpr int NS = APPLY ? 4 : 1;                       // components of the slab: u and rho | rho alone
  constexpr int CR = APPLY ? 3 : 0;                       // the slab component of rho
  constexpr int SK = Q * QP, SC = Q * Q * QP, NE = NS * SC;
  static_assert(sizeof(double) * ((size_t)EPB * NE + 2 * MAXN1D * MAXN1D) <= 64 * 1024, "static LDS");
  __shared__ double sBB[(APPLY ? 1 : 2) * MAXN1D * MAXN1D];     // the table; the diagonal: its squares behind it
  __shared__ double slab[EPB * NE];
  double *sB = sBB, *sB2 = sBB + (APPLY ? 0 : MAXN1D * MAXN1D);
  const int tid = threadIdx.x, el = tid / TPE, t = tid % TPE;
  double *su = slab + (size_t)el * NE;
  const int e = blockIdx.x * EPB + el;
  const bool live = e < a.nelem;
  for (int i = tid; i < Q * P; i += 256) {
    const double b = tab.interp[i];
    sB[i] = b;
    if constexpr (!APPLY) sB2[i] = b * b;
  }
  const double *sT = sB2;                                 // the table of the transposed half (the apply: the table itself)
  if (live) {
    for (int n = t; n < P3; n += TPE) {
      const int i = n % P, j = (n / P) % P, k = n / (P * P);
      su[CR * SC + k * SK + j * QP + i] = f.rho[f.rho_offsets[(size_t)e * P3 + n]];
      if constexpr (APPLY) {
        const uint32_t off = a.offsets[(size_t)e * P3 + n];
        const uint32_t fl = a.mask_in ? (off >> OFF_FLAG_SHIFT) : 0u;
        const double *p = a.x + (off & OFF_MASK);
#pragma unroll
        for (int c = 0; c < 3; c++) su[c * SC + k * SK + j * QP + i] = ((fl >> c) & 1u) ? 0. : p[c];
      }
    }
  }
  __syncthreads();
  if (live) {
    for (int l = t; l < NS * P * P; l += TPE) {           // x: (c, k, j), looped
      const int j = l % P, k = (l / P) % P, c = l / (P * P);
      mass_line<P, Q, false>(su + c * SC + k * SK + j * QP, 1, sB);
    }
  }
  __syncthreads();
  if (live) {
    for (int l = t; l < NS * P * Q; l += TPE) {           // y: (c, k, a), looped
      const int aa = l % Q, k = (l / Q) % P, c = l / (P * Q);
      mass_line<P, Q, false>(su + c * SC + k * SK + aa, QP, sB);
    }
  }
  __syncthreads();
  // z of u and of rho, the product with c0 rho wdetJ at the Q points of the line, z transposed: (c, b, a)
  if (live && t < NC * Q * Q) {
    const int ab = t % (Q * Q), aa = ab % Q, bb = ab / Q, c = t / (Q * Q);
    double *s = su + c * SC + bb * QP + aa;
    const double *sr = su + CR * SC + bb * QP + aa;
    const double *wq = a.qdata + (size_t)e * 10 * Q3 + ab;
    double v[Q], rin[P];
#pragma unroll
    for (int k = 0; k < P; k++) rin[k] = sr[k * SK];
    if constexpr (APPLY) {
      double in[P];
#pragma unroll
      for (int k = 0; k < P; k++) in[k] = s[k * SK];
#pragma unroll
      for (int kk = 0; kk < Q; kk++) {
        double u = 0., r = 0.;
#pragma unroll
        for (int k = 0; k < P; k++) {
          u += sB[kk * P + k] * in[k];
          r += sB[kk * P + k] * rin[k];
        }
        v[kk] = a.coef * wq[kk * Q * Q] * r * u;
      }
    } else {
#pragma unroll
      for (int kk = 0; kk < Q; kk++) {
        double r = 0.;
#pragma unroll
        for (int k = 0; k < P; k++) r += sB[kk * P + k] * rin[k];
        v[kk] = a.coef * wq[kk * Q * Q] * r;
      }
    }
#pragma unroll
    for (int k = 0; k < P; k++) {
      double r = 0.;
#pragma unroll
      for (int kk = 0; kk < Q; kk++) r += sT[kk * P + k] * v[kk];
      s[k * SK] = r;
    }
  }
  __syncthreads();
  if (live && t < NC * P * Q) {                           // y transposed: (c, k, a)
    const int aa = t % Q, k = (t / Q) % P, c = t / (P * Q);
    mass_line<P, Q, true>(su + c * SC + k * SK + aa, QP, sT);
  }
  __syncthreads();
  if (live && t < NC * P * P) {                           // x transposed: (c, k, j)
    const int j = t % P, k = (t / P) % P, c = t / (P * P);
    mass_line<P, Q, true>(su + c * SC + k * SK + j * QP, 1, sT);
  }
  __syncthreads();
  if (live) {
    double *out = a.evec + (size_t)e * P3 * 3;
    for (int o = t; o < 3 * P3; o += TPE) {
      const int n = o / 3, c = o % 3, i = n % P, j = (n / P) % P, k = n / (P * P);
      if constexpr (APPLY) out[o] = su[c * SC + k * SK + j * QP + i];     // (masked rows: launch_assemble() takes the row flags)
      else {
        const uint32_t fl = a.mask_out ? (a.offsets[(size_t)e * P3 + n] >> OFF_FLAG_SHIFT) : 0u;
        out[o] = ((fl >> c) & 1u) ? 0. : su[k * SK + j * QP + i];
      }
    }
  }
}

template <int P, int Q, int MODE>
static hipError_t mass_t(const BasisTables &t, const MassArgs &a, hipStream_t s) {
  if (a.nelem <= 0) return hipSuccess;
  constexpr int EPB = MassGeom<Q>::EPB;
  hipLaunchKernelGGL((k_mass<P, Q, MODE>), dim3((a.nelem + EPB - 1) / EPB), dim3(256), 0, s, t, a);
  return hipGetLastError();
}

hipError_t launch_mass(int P, int Q, bool diag, const BasisTables &t, const MassArgs &a, hipStream_t s, const char **name) {
#define CPS_MASS(Pv, Qv)                                                              \
  if (P == Pv && Q == Qv) {                                                           \
    *name = diag ? "mass_diag<" #Pv "," #Qv ">" : "mass<" #Pv "," #Qv ">";            \
    return diag ? mass_t<Pv, Qv, MASS_DIAG>(t, a, s) : mass_t<Pv, Qv, MASS_APPLY>(t, a, s); \
  }
  CPS_DIAG_PQ(CPS_MASS)
#undef CPS_MASS
  return hipErrorInvalidValue;
}

template <int P, int Q, int MODE>
static hipError_t mass_field_t(const BasisTables &t, const MassArgs &a, const MassFieldArgs &f, hipStream_t s) {
  if (a.nelem <= 0) return hipSuccess;
  constexpr int EPB = MassGeom<Q>::EPB;
  hipLaunchKernelGGL((k_mass<P, Q, MODE>), dim3((a.nelem + EPB - 1) / EPB), dim3(256), 0, s, t, a, f);
  return hipGetLastError();
}

hipError_t launch_mass_field(int P, int Q, bool diag, const BasisTables &t, const MassArgs &a, const MassFieldArgs &f, hipStream_t s, const char **name) {
#define CPS_MASS(Pv, Qv)                                                              \
  if (P == Pv && Q == Qv) {                                                           \
    *name = diag ? "mass_field_diag<" #Pv "," #Qv ">" : "mass_field<" #Pv "," #Qv ">"; \
    return diag ? mass_field_t<Pv, Qv, MASS_DIAG_RHO>(t, a, f, s) : mass_field_t<Pv, Qv, MASS_APPLY_RHO>(t, a, f, s); \
  }
  CPS_DIAG_PQ(CPS_MASS)
#undef CPS_MASS
  return hipErrorInvalidValue;
}

}  // namespace cps
