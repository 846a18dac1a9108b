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

enum StressMode : int { STRESS_POINTS = 0, STRESS_NODAL = 1, STRESS_THERMAL_FORCE = 2, STRESS_THERMAL_TANGENT = 3, STRESS_POINTS_THERMAL = 4,
                        STRESS_NODAL_THERMAL = 5 };

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

// ---- the temperature field: MODE = STRESS_THERMAL_FORCE, STRESS_THERMAL_TANGENT, STRESS_POINTS_THERMAL, STRESS_NODAL_THERMAL -----------------
// theta_h(e,q) = sum_m N_m(q) theta(e,m): a nodal temperature change interpolated with the table of u, gathered from a scalar vector through
// offsets of its own (ThermalArgs: plain indices, no flags, no factor 3), beta = E alpha / (1 - 2 nu) formed on the host.
//   STRESS_THERMAL_FORCE    evec[e][n][c] = sum_q sum_d dN_n/dxi_d(q) G[d][c](q),   G[d][c] = -beta theta_h wdetJ sum_k dXdx[d][k] F^-T[c][k]
//                           (QFunction "ThermalForce"): the residual of the coupling energy -beta theta tr eps (linElas, hyperSS: F^-T = I,
//                           u is not gathered) or -beta theta ln J (hyperFS: F = I + grad u, the first Piola stress -beta theta F^-T)
//   STRESS_THERMAL_TANGENT  the same with  T = +beta theta_h F^-T (grad du)^T F^-T  in place of -beta theta_h F^-T (hyperFS only; QFunction
//                           "ThermalTangent"): du gathered too, its flagged components read as zero (ThermalArgs::mask_in)
//   STRESS_POINTS_THERMAL, STRESS_NODAL_THERMAL   the two modes above with sigma - beta theta_h I (hyperFS: - beta theta_h / det F I)
// The same name and template parameters as the kernel above with a third argument, the field's own struct, so that StressArgs and with it
// the argument block, the code, the registers and the LDS of the MODE 0 / 1 instantiations stay what they were.
// theta rides as a further component of the slab through the forward passes, which LOOP over their lines (4 or 7 components of lines can
// exceed the TPE lanes of an element).  The transposed gradient of the two load modes does not hold the nine G[d][c] in LDS (9 components
// beside EPB elements do not fit at Q = 8): three rounds over the reference direction d -- G[d][0..2] into a 3-component slab, a barrier,
// every point adds sum_m D[m][q_d] slab(.. m ..) in registers, a barrier -- then ONE set of transposed passes Q -> P on the sum, and
// coalesced stores of the [P^3][3] block, which launch_assemble() sums per node in element order under the row flags.  No atomics.
template <int Q, int MODE> struct ThermalGeom {
  static constexpr int QP = MassGeom<Q>::QP, TPE = MassGeom<Q>::TPE, EPB = MassGeom<Q>::EPB;
  static constexpr bool LOAD = MODE == STRESS_THERMAL_FORCE || MODE == STRESS_THERMAL_TANGENT;
  static constexpr int NF = MODE == STRESS_THERMAL_TANGENT ? 7 : 4;   // forward components: u (3), [du (3)], theta
  static constexpr int NB = MODE == STRESS_NODAL_THERMAL ? 7 : 3;     // components of the transposed half (the points mode has none)
  static constexpr int NC = NF > NB ? NF : NB;                         // components of the slab at its fullest
  static constexpr int NE = NC * Q * Q * QP;                           // doubles per element
  static constexpr int NPT = (Q * Q * Q + TPE - 1) / TPE;              // points per lane
  static_assert(sizeof(double) * ((size_t)EPB * NE + 2 * MAXN1D * MAXN1D) <= 64 * 1024, "static LDS");
};

// the nine reference derivatives of three slab components at the point (i, j, k): ug[d * 3 + c] = d u_c / d xi_d
template <int Q, int QP>
CPS_DEV void colo_grad3(const double *s3, const double *sD, int i, int j, int k, double *ug) {
  constexpr int SK = Q * QP, SC = Q * Q * QP;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const double *s = s3 + c * SC;
    double d0 = 0., d1 = 0., d2 = 0.;
#pragma unroll
    for (int m = 0; m < Q; m++) {
      d0 += sD[i * Q + m] * s[k * SK + j * QP + m];
      d1 += sD[j * Q + m] * s[k * SK + m * QP + i];
      d2 += sD[k * Q + m] * s[m * SK + j * QP + i];
    }
    ug[0 * 3 + c] = d0; ug[1 * 3 + c] = d1; ug[2 * 3 + c] = d2;
  }
}
// F^-1 and det F of F = I + g by cofactors
CPS_DEV double inverse_of_f(const double g[3][3], double Fi[3][3]) {
  double F[3][3];
#pragma unroll
  for (int a = 0; a < 3; a++)
#pragma unroll
    for (int b = 0; b < 3; b++) F[a][b] = g[a][b] + (a == b ? 1. : 0.);
  Fi[0][0] = F[1][1] * F[2][2] - F[1][2] * F[2][1]; Fi[0][1] = F[0][2] * F[2][1] - F[0][1] * F[2][2]; Fi[0][2] = F[0][1] * F[1][2] - F[0][2] * F[1][1];
  Fi[1][0] = F[1][2] * F[2][0] - F[1][0] * F[2][2]; Fi[1][1] = F[0][0] * F[2][2] - F[0][2] * F[2][0]; Fi[1][2] = F[0][2] * F[1][0] - F[0][0] * F[1][2];
  Fi[2][0] = F[1][0] * F[2][1] - F[1][1] * F[2][0]; Fi[2][1] = F[0][1] * F[2][0] - F[0][0] * F[2][1]; Fi[2][2] = F[0][0] * F[1][1] - F[0][1] * F[1][0];
  const double det = F[0][0] * Fi[0][0] + F[0][1] * Fi[1][0] + F[0][2] * Fi[2][0];
  const double r = 1. / det;
#pragma unroll
  for (int a = 0; a < 3; a++)
#pragma unroll
    for (int b = 0; b < 3; b++) Fi[a][b] *= r;
  return det;
}

template <int P, int Q, int MODE>
__global__ __launch_bounds__(256) void k_stress(const BasisTables tab, const StressArgs a, const ThermalArgs th) {
  static_assert(MODE >= STRESS_THERMAL_FORCE && MODE <= STRESS_NODAL_THERMAL, "the modes with a temperature field");
  using G = ThermalGeom<Q, MODE>;
  constexpr bool LOAD = G::LOAD, TANGENT = MODE == STRESS_THERMAL_TANGENT, NODAL = MODE == STRESS_NODAL_THERMAL;
  constexpr int QP = G::QP, TPE = G::TPE, EPB = G::EPB, NPT = G::NPT, P3 = P * P * P, Q3 = Q * Q * Q;
  constexpr int SK = Q * QP, SC = Q * Q * QP;             // pitch of k and of c in the slab
  constexpr int NF = G::NF, CT = NF - 1;                  // forward components; the slab component of theta (du: 3 .. 5)
  constexpr int NV = LOAD ? 9 : (NODAL ? 7 : 1);          // values a point keeps over a barrier
  __shared__ double sB[MAXN1D * MAXN1D];
  __shared__ double sD[MAXN1D * MAXN1D];
  __shared__ double slab[EPB * G::NE];
  const int tid = threadIdx.x, el = tid / TPE, t = tid % TPE;
  double *su = slab + (size_t)el * G::NE;
  const int e = blockIdx.x * EPB + el;
  const bool live = e < a.nelem;
  const bool need_u = !LOAD || a.model == 2;              // wave-uniform: the small-strain loads do not read the displacement
  const int c0 = need_u ? 0 : CT;                         // ... and pass theta alone through the tables
  for (int i = tid; i < Q * P; i += 256) sB[i] = tab.interp[i];
  for (int i = tid; i < Q * Q; i += 256) sD[i] = tab.colo[i];
  if (live) {
    for (int n = t; n < P3; n += TPE) {
      const int i = n % P, j = (n / P) % P, k = n / (P * P), at = k * SK + j * QP + i;
      su[CT * SC + at] = th.theta[th.theta_offsets[(size_t)e * P3 + n]];
      const uint32_t off = a.offsets[(size_t)e * P3 + n];
      if (need_u) {
        const double *p = a.x + (off & OFF_MASK);
#pragma unroll
        for (int c = 0; c < 3; c++) su[c * SC + at] = p[c];
      }
      if constexpr (TANGENT) {
        const uint32_t fl = th.mask_in ? (off >> OFF_FLAG_SHIFT) : 0u;
        const double *p = th.dx + (off & OFF_MASK);
#pragma unroll
        for (int c = 0; c < 3; c++) su[(3 + c) * SC + at] = ((fl >> c) & 1u) ? 0. : p[c];
      }
    }
  }
  __syncthreads();
  if (live)
    for (int l = t + c0 * P * P; l < NF * P * P; l += TPE) {  // x: (c, k, j), looped
      const int j = l % P, k = (l / P) % P, c = l / (P * P);
      mass_line<P, Q, false>(su + c * SC + k * SK + j * QP, 1, sB);
    }
  __syncthreads();
  if (live)
    for (int l = t + c0 * P * Q; l < NF * P * Q; l += TPE) {  // y: (c, k, a), looped
      const int aa = l % Q, k = (l / Q) % P, c = l / (P * Q);
      mass_line<P, Q, false>(su + c * SC + k * SK + aa, QP, sB);
    }
  __syncthreads();
  if (live)
    for (int l = t + c0 * Q * Q; l < NF * Q * Q; l += TPE) {  // z: (c, b, a), looped
      const int aa = l % Q, bb = (l / Q) % Q, c = l / (Q * Q);
      mass_line<P, Q, false>(su + c * SC + bb * QP + aa, SK, sB);
    }
  __syncthreads();
  // a lane per point: theta, the reference derivatives from the three lines through it, qdata, the flux or the stress
  const Phys ph{a.nu, a.E, a.lambda, a.TwoMu};
  double val[NPT][NV];
#pragma unroll
  for (int r = 0; r < NPT; r++) {
    const int q = t + r * TPE;
    if (live && q < Q3) {
      const int i = q % Q, j = (q / Q) % Q, k = q / (Q * Q);
      const double bt = th.beta * su[CT * SC + k * SK + j * QP + i];
      const double *pq = a.qdata + (size_t)e * 10 * Q3 + q;
      double qd[10], ug[9];
#pragma unroll
      for (int c = 0; c < 10; c++) qd[c] = pq[(size_t)c * Q3];
      if constexpr (LOAD) {
        double T[3][3];
        if (a.model == 2) {
          double g[3][3], Fi[3][3];
          colo_grad3<Q, QP>(su, sD, i, j, k, ug);
          physical_grad<false>(ug, qd, g);
          inverse_of_f(g, Fi);
          if constexpr (TANGENT) {
            double dg[3][3], M[3][3];
            colo_grad3<Q, QP>(su + 3 * SC, sD, i, j, k, ug);
            physical_grad<false>(ug, qd, dg);
#pragma unroll
            for (int aa = 0; aa < 3; aa++)                // M[a][m] = sum_b dg[b][a] F^-1[m][b]
#pragma unroll
              for (int m = 0; m < 3; m++) M[aa][m] = dg[0][aa] * Fi[m][0] + dg[1][aa] * Fi[m][1] + dg[2][aa] * Fi[m][2];
#pragma unroll
            for (int c = 0; c < 3; c++)                   // T[c][m] = beta theta sum_a F^-1[a][c] M[a][m]
#pragma unroll
              for (int m = 0; m < 3; m++) T[c][m] = bt * (Fi[0][c] * M[0][m] + Fi[1][c] * M[1][m] + Fi[2][c] * M[2][m]);
          } else {
#pragma unroll
            for (int c = 0; c < 3; c++)
#pragma unroll
              for (int m = 0; m < 3; m++) T[c][m] = -bt * Fi[m][c];
          }
        } else {
#pragma unroll
          for (int c = 0; c < 3; c++)
#pragma unroll
            for (int m = 0; m < 3; m++) T[c][m] = c == m ? -bt : 0.;
        }
        pull_back<false>(T, qd, val[r]);                  // val[d * 3 + c] = wdetJ sum_m dXdx[d][m] T[c][m]
      } else {
        double g[3][3], sg[6];
        colo_grad3<Q, QP>(su, sD, i, j, k, ug);
        physical_grad<false>(ug, qd, g);
        double iso = bt;
        if (a.model == 2) {
          double Fi[3][3];
          stress_hyperfs(ph, g, sg);
          iso = bt / inverse_of_f(g, Fi);
        } else if (a.model == 1) stress_hyperss(ph, g, sg);
        else stress_linelas(ph, g, sg);
#pragma unroll
        for (int c = 0; c < 3; c++) sg[c] -= iso;
        if constexpr (!NODAL) {
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
  }
  if constexpr (LOAD) {
    double h[NPT][3];
#pragma unroll
    for (int r = 0; r < NPT; r++) h[r][0] = h[r][1] = h[r][2] = 0.;
#pragma unroll
    for (int d = 0; d < 3; d++) {
      __syncthreads();                                    // every read of the slab (the interpolated field, the round before) is done
#pragma unroll
      for (int r = 0; r < NPT; r++) {
        const int q = t + r * TPE;
        if (live && q < Q3) {
          const int i = q % Q, j = (q / Q) % Q, k = q / (Q * Q);
#pragma unroll
          for (int c = 0; c < 3; c++) su[c * SC + k * SK + j * QP + i] = val[r][d * 3 + c];
        }
      }
      __syncthreads();
#pragma unroll
      for (int r = 0; r < NPT; r++) {
        const int q = t + r * TPE;
        if (live && q < Q3) {
          const int i = q % Q, j = (q / Q) % Q, k = q / (Q * Q);
          const int qd_ = d == 0 ? i : (d == 1 ? j : k);                               // the point's index along d
          const int base = d == 0 ? k * SK + j * QP : (d == 1 ? k * SK + i : j * QP + i), step = d == 0 ? 1 : (d == 1 ? QP : SK);
#pragma unroll
          for (int m = 0; m < Q; m++) {
            const double dm = sD[m * Q + qd_];
#pragma unroll
            for (int c = 0; c < 3; c++) h[r][c] += dm * su[c * SC + base + m * step];
          }
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < NPT; r++) {
      const int q = t + r * TPE;
      if (live && q < Q3) {
        const int i = q % Q, j = (q / Q) % Q, k = q / (Q * Q);
#pragma unroll
        for (int c = 0; c < 3; c++) su[c * SC + k * SK + j * QP + i] = h[r][c];
      }
    }
  } else if constexpr (NODAL) {
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
  }
  if constexpr (LOAD || NODAL) {
    constexpr int NB = G::NB;
    __syncthreads();
    if (live)
      for (int l = t; l < NB * Q * Q; l += TPE) {         // z transposed: (c, b, a)
        const int aa = l % Q, bb = (l / Q) % Q, c = l / (Q * Q);
        mass_line<P, Q, true>(su + c * SC + bb * QP + aa, SK, sB);
      }
    __syncthreads();
    if (live)
      for (int l = t; l < NB * P * Q; l += TPE) {         // y transposed: (c, k, a)
        const int aa = l % Q, k = (l / Q) % P, c = l / (P * Q);
        mass_line<P, Q, true>(su + c * SC + k * SK + aa, QP, sB);
      }
    __syncthreads();
    if (live)
      for (int l = t; l < NB * P * P; l += TPE) {         // x transposed: (c, k, j)
        const int j = l % P, k = (l / P) % P, c = l / (P * P);
        mass_line<P, Q, true>(su + c * SC + k * SK + j * QP, 1, sB);
      }
    __syncthreads();
    if (live) {
      double *out = a.out + (size_t)e * NB * P3;
      for (int o = t; o < NB * P3; o += TPE) {
        // the loads: [n][c], the block launch_assemble() reads (masked rows: its row flags); nodal: [c][n], the output restriction's E-layout
        const int c = LOAD ? o % 3 : o / P3, n = LOAD ? o / 3 : o % P3, i = n % P, j = (n / P) % P, k = n / (P * P);
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

template <int P, int Q, int MODE>
static hipError_t stress_thermal_t(const BasisTables &t, const StressArgs &a, const ThermalArgs &th, hipStream_t s) {
  if (a.nelem <= 0) return hipSuccess;
  constexpr int EPB = ThermalGeom<Q, MODE>::EPB;
  hipLaunchKernelGGL((k_stress<P, Q, MODE>), dim3((a.nelem + EPB - 1) / EPB), dim3(256), 0, s, t, a, th);
  return hipGetLastError();
}

static_assert((int)STRESS_THERMAL_FORCE == (int)THERMAL_MODE_FORCE && (int)STRESS_THERMAL_TANGENT == (int)THERMAL_MODE_TANGENT &&
              (int)STRESS_POINTS_THERMAL == (int)THERMAL_MODE_POINTS && (int)STRESS_NODAL_THERMAL == (int)THERMAL_MODE_NODAL, "the host's names of the modes (kernels.hpp)");
hipError_t launch_stress_thermal(int P, int Q, int mode,const BasisTables &t, const StressArgs &a, const ThermalArgs &th, hipStream_t s, const char **name) {
#define CPS_STRESS(Pv, Qv)                                                                                                  \
  if (P == Pv && Q == Qv) {                                                                                                 \
    switch (mode) {                                                                                                         \
    case STRESS_THERMAL_FORCE: *name = "thermal_force<P=" #Pv ",Q=" #Qv ">"; return stress_thermal_t<Pv, Qv, STRESS_THERMAL_FORCE>(t, a, th, s);       \
    case STRESS_THERMAL_TANGENT: *name = "thermal_tangent<P=" #Pv ",Q=" #Qv ">"; return stress_thermal_t<Pv, Qv, STRESS_THERMAL_TANGENT>(t, a, th, s); \
    case STRESS_POINTS_THERMAL: *name = "stress<P=" #Pv ",Q=" #Qv ",points+thermal>"; return stress_thermal_t<Pv, Qv, STRESS_POINTS_THERMAL>(t, a, th, s); \
    case STRESS_NODAL_THERMAL: *name = "stress<P=" #Pv ",Q=" #Qv ",nodal+thermal>"; return stress_thermal_t<Pv, Qv, STRESS_NODAL_THERMAL>(t, a, th, s);   \
    default: return hipErrorInvalidValue;                                                                                   \
    }                                                                                                                       \
  }
  CPS_DIAG_PQ(CPS_STRESS)
#undef CPS_STRESS
  return hipErrorInvalidValue;
}

}  // namespace cps
