// kernel_diag_sf.hpp -- the sum-factorised diagonal of B^T D B (matops.c:227), scalar and point-block, from ONE source.
//
//   diag_c(n)       = sum_q sum_{d,d2} g_d(n,q) D^{cc}_{d d2}(q) g_d2(n,q)       k_diag_sf    (CeedOperatorLinearAssembleDiagonal)
//   block_n[c'][c]  = sum_q sum_{d,d2} g_d(n,q) D^{c'c}_{d d2}(q) g_d2(n,q)      k_pbdiag_sf  (...AssemblePointBlockDiagonal)
//
// The tangent D is probed with unit reference gradients through the Jacobian physics.  g_d is a product of 1-D factors, so each of the
// 18 tensors S^{c'}_pair(q) (3 output components x 6 direction pairs (d, d2), d <= d2; g_d g_d2 is symmetric in (d, d2), so an
// off-diagonal pair holds D_{d d2} + D_{d2 d} whatever the symmetry of D itself) is contracted direction by direction with the PRODUCT
// tables BB, BG, GG (table_x(i,a) = X_d(i,a) X_d2(i,a), X = G in its own direction, B otherwise): 18 (P Q^2 + P^2 Q + P^3) Q FMAs per
// element instead of P^3 Q^3 60 (25x fewer at P = Q = 5; the unfactorised first version left the tree in round 3).
//
// The two kernels differ in which tangent entries go into the 18 tensors and in how the three sums of a node are masked and stored:
//   k_diag_sf    ONE round: nine probes per point (compile-time unit vectors), the entries with c' == c kept.
//   k_pbdiag_sf  THREE rounds, one per input component c (a runtime c: three probes per round), all c' kept: column c of every block.
//                All 54 tensors at once would not fit the LDS from Q = 7; 27 tangent entries are live per round.  Nothing assumes a
//                symmetric block: the tangent is written as the QFunction gives it.
// Everything else -- the slab, the tables, the store of the tensors, the three passes -- is stated here once (sf_*), and so are the
// launcher and the (P, Q) list.  The instantiations stay in two objects: kernels_dispatch.hip (scalar), kernels_pointblock.hip (blocks).
#pragma once
#include "kernels_common.hpp"
#include "qfunctions_device.hpp"

namespace cps {

template <int P, int Q> struct DiagGeom {
  static constexpr int Q3 = Geom<Q>::Q3, P3 = P * P * P, TPE = Geom<Q>::TPE, NT = 18;
  static constexpr int PQQ = P * Q * Q, PPQ = P * P * Q, S0 = Q3 > PPQ ? Q3 : PPQ;
  // the slab (147 KB at Q = 8: the dynamic-shared-memory attribute), in doubles from its start:
  static constexpr int O_T = 0;                 // [3][Q * P]: BB, BG, GG
  static constexpr int O_S0 = 3 * Q * P;        // [NT][Q3] the tensors, later [NT][P * P * Q]
  static constexpr int O_S1 = O_S0 + NT * S0;   // [NT][P * Q * Q]
  static constexpr size_t LDS_BYTES = sizeof(double) * (O_S1 + NT * PQQ);
};

template <int P, int Q> CPS_DEV void sf_stage_tables(const BasisTables &tab, double *dyn, int q) {
  double *sT = dyn + DiagGeom<P, Q>::O_T;
  for (int i = q; i < Q * P; i += DiagGeom<P, Q>::TPE) {
    const double bb = tab.interp[i], gg = tab.grad[i];
    sT[i] = bb * bb; sT[Q * P + i] = bb * gg; sT[2 * Q * P + i] = gg * gg;
  }
}
// qdata and (where the QFunction reads it) the stored state of point q of element e
template <int Q, int QF> CPS_DEV void sf_load_point(const DiagArgs &a, int e, int q, double (&qd)[10], double (&st)[9]) {
  constexpr int Q3 = Geom<Q>::Q3;
  const double *qp = a.qdata + (size_t)e * 10 * Q3 + q;
#pragma unroll
  for (int c = 0; c < 10; c++) qd[c] = qp[c * Q3];
  if constexpr (QFTraits<QF>::state_in) {
    const double *sp = a.state_in + (size_t)e * 9 * Q3 + q;
#pragma unroll
    for (int c = 0; c < 9; c++) st[c] = sp[c * Q3];
  }
}
// the six pair tensors of output component co at point q, from D[dout][din]
template <int P, int Q> CPS_DEV void sf_store_pairs(double *dyn, int co, int q, const double (&D)[3][3]) {
  constexpr int Q3 = DiagGeom<P, Q>::Q3;
  double *s0 = dyn + DiagGeom<P, Q>::O_S0 + co * 6 * Q3 + q;
  s0[0 * Q3] = D[0][0];
  s0[1 * Q3] = D[1][1];
  s0[2 * Q3] = D[2][2];
  s0[3 * Q3] = D[0][1] + D[1][0];
  s0[4 * Q3] = D[0][2] + D[2][0];
  s0[5 * Q3] = D[1][2] + D[2][1];
}
// table kind of pair p in direction dir: (d == dir) + (d2 == dir)  (0 BB, 1 BG, 2 GG)
CPS_DEV int sf_kind(int p, int dir) {
  const int d = p < 3 ? p : (p == 5 ? 1 : 0), d2 = p < 3 ? p : (p == 3 ? 1 : 2);
  return (d == dir) + (d2 == dir);
}
// The 18 stored tensors contracted with the tables, x then y then z; acc[c'] = the sum over the six pairs at node q (q < P^3: one node
// per thread in the last pass).  Called by every thread of the workgroup; the barrier in front covers the stores of the tensors.
template <int P, int Q> CPS_DEV void sf_contract(double *dyn, int q, double (&acc)[3]) {
  using G = DiagGeom<P, Q>;
  constexpr int Q3 = G::Q3, P3 = G::P3, TPE = G::TPE, NT = G::NT, PQQ = G::PQQ, PPQ = G::PPQ;
  double *sT = dyn + G::O_T, *s0 = dyn + G::O_S0, *s1 = dyn + G::O_S1;
  __syncthreads();
  // x: U1[t][k][j][a] = sum_i T(i,a) S[t][k][j][i]
  for (int o = q; o < NT * PQQ; o += TPE) {
    const int t = o / PQQ, r = o % PQQ, aa = r % P, kj = r / P;
    const double *T = sT + sf_kind(t % 6, 0) * Q * P, *src = s0 + t * Q3 + kj * Q;
    double v = 0.;
#pragma unroll
    for (int i = 0; i < Q; i++) v += T[i * P + aa] * src[i];
    s1[o] = v;
  }
  __syncthreads();
  // y: U2[t][k][b][a] = sum_j T(j,b) U1[t][k][j][a]
  for (int o = q; o < NT * PPQ; o += TPE) {
    const int t = o / PPQ, r = o % PPQ, aa = r % P, bb = (r / P) % P, k = r / (P * P);
    const double *T = sT + sf_kind(t % 6, 1) * Q * P, *src = s1 + t * PQQ + k * Q * P + aa;
    double v = 0.;
#pragma unroll
    for (int j = 0; j < Q; j++) v += T[j * P + bb] * src[j * P];
    s0[o] = v;
  }
  __syncthreads();
  // z, and the sum over the pairs
  if (q < P3) {
    const int ab = q % (P * P), nc = q / (P * P);
#pragma unroll
    for (int c = 0; c < 3; c++) {
      acc[c] = 0.;
#pragma unroll
      for (int p = 0; p < 6; p++) {
        const double *T = sT + sf_kind(p, 2) * Q * P, *src = s0 + (c * 6 + p) * PPQ + ab;
        double v = 0.;
#pragma unroll
        for (int k = 0; k < Q; k++) v += T[k * P + nc] * src[k * P * P];
        acc[c] += v;
      }
    }
  }
}

template <int P, int Q, int QF>
__global__ __launch_bounds__(Geom<Q>::TPE) void k_diag_sf(const BasisTables tab, const DiagArgs a) {
  using G = DiagGeom<P, Q>;
  extern __shared__ double dyn[];
  const int q = threadIdx.x, e = blockIdx.x;
  sf_stage_tables<P, Q>(tab, dyn, q);
  if (q < G::Q3) {
    double qd[10], st[9], dv[9], sto[9], ug[9], D[3][3][3];   // D[c][dout][din]
    sf_load_point<Q, QF>(a, e, q, qd, st);
#pragma unroll
    for (int din = 0; din < 3; din++)
#pragma unroll
      for (int c = 0; c < 3; c++) {
#pragma unroll
        for (int s = 0; s < 9; s++) ug[s] = (s == din * 3 + c) ? 1. : 0.;
        qf_point<QF>(Phys{a.nu, a.E, a.lambda, a.TwoMu}, ug, qd, st, dv, sto);
#pragma unroll
        for (int dout = 0; dout < 3; dout++) D[c][dout][din] = dv[dout * 3 + c];
      }
#pragma unroll
    for (int c = 0; c < 3; c++) sf_store_pairs<P, Q>(dyn, c, q, D[c]);
  }
  double acc[3];
  sf_contract<P, Q>(dyn, q, acc);
  if (q < G::P3) {
    const uint32_t off = a.offsets[(size_t)e * G::P3 + q];
    const uint32_t fl = a.mask_out ? (off >> OFF_FLAG_SHIFT) : 0u;
#pragma unroll
    for (int c = 0; c < 3; c++) a.evec[((size_t)e * G::P3 + q) * 3 + c] = ((fl >> c) & 1u) ? 0. : acc[c];  // summed by launch_assemble()
  }
}

template <int P, int Q, int QF>
__global__ __launch_bounds__(Geom<Q>::TPE) void k_pbdiag_sf(const BasisTables tab, const DiagArgs a) {
  using G = DiagGeom<P, Q>;
  extern __shared__ double dyn[];
  const int q = threadIdx.x, e = blockIdx.x;
  sf_stage_tables<P, Q>(tab, dyn, q);
  double qd[10], st[9];
  if (q < G::Q3) sf_load_point<Q, QF>(a, e, q, qd, st);
  uint32_t fl_in = 0u, fl_out = 0u;
  if (q < G::P3) {
    const uint32_t fl = a.offsets[(size_t)e * G::P3 + q] >> OFF_FLAG_SHIFT;
    fl_in = a.mask_in ? fl : 0u; fl_out = a.mask_out ? fl : 0u;
  }
#pragma unroll 1
  for (int c = 0; c < 3; c++) {      // round c: column c of every block
    if (q < G::Q3) {
      double dv[9], sto[9], ug[9], D[3][3][3];   // D[c'][dout][din]
#pragma unroll
      for (int din = 0; din < 3; din++) {
#pragma unroll
        for (int s = 0; s < 9; s++) ug[s] = (s == din * 3 + c) ? 1. : 0.;
        qf_point<QF>(Phys{a.nu, a.E, a.lambda, a.TwoMu}, ug, qd, st, dv, sto);
#pragma unroll
        for (int co = 0; co < 3; co++)
#pragma unroll
          for (int dout = 0; dout < 3; dout++) D[co][dout][din] = dv[dout * 3 + co];
      }
#pragma unroll
      for (int co = 0; co < 3; co++) sf_store_pairs<P, Q>(dyn, co, q, D[co]);
    }
    double acc[3];
    sf_contract<P, Q>(dyn, q, acc);
    if (q < G::P3) {                 // entry (c', c) of the node's block
      double *out = a.evec + ((size_t)e * G::P3 + q) * 9 + c;
      const bool dead_in = (fl_in >> c) & 1u;
#pragma unroll
      for (int co = 0; co < 3; co++) out[co * 3] = (dead_in || ((fl_out >> co) & 1u)) ? 0. : acc[co];
    }
    __syncthreads();   // the next round overwrites s0
  }
}

// One workgroup of Geom<Q>::TPE lanes per element.  K: the instantiated kernel (a template argument, so that the attribute latch
// below is one per kernel).
template <int P, int Q, void (*K)(BasisTables, DiagArgs)>
static hipError_t launch_sf(const BasisTables &t, const DiagArgs &a, hipStream_t s) {
  using G = DiagGeom<P, Q>;
  if (a.nelem <= 0) return hipSuccess;
  static_assert(G::P3 <= G::TPE, "a lane per node in the last pass");
  static_assert(G::LDS_BYTES <= 160 * 1024, "the slab fits the CU's LDS");
  static bool attr_set = false;
  if (!attr_set) {
    hipError_t er = hipFuncSetAttribute((const void *)K, hipFuncAttributeMaxDynamicSharedMemorySize, (int)G::LDS_BYTES);
    if (er != hipSuccess) return er;
    attr_set = true;
  }
  hipLaunchKernelGGL(K, dim3(a.nelem), dim3(G::TPE), G::LDS_BYTES, s, t, a);
  return hipGetLastError();
}

// The (P, Q) pairs BOTH diagonals are instantiated for, three Jacobian QFunctions each (a ladder needs the pair of every level: one
// list, so that no level can have a scalar diagonal and no blocks).  Rows three and four: degrees 5 and 7 (logarithmic ladders 1, 2,
// 4, p) and the uniform ladders of degrees 5 and 6.  tests/_kernel_matrix.py restates the set; test_kernel_inventory.py holds the
// objects of both kernels against it.
#define CPS_DIAG_PQ(X)                                                                   \
  X(2, 2) X(2, 3) X(3, 3) X(2, 4) X(3, 4) X(4, 4)                                        \
  X(2, 5) X(3, 5) X(4, 5) X(5, 5) X(2, 7) X(3, 7) X(5, 7) X(7, 7)                        \
  X(2, 6) X(3, 6) X(4, 6) X(5, 6) X(6, 6) X(4, 7) X(6, 7)                                \
  X(2, 8) X(3, 8) X(4, 8) X(5, 8) X(6, 8) X(7, 8) X(8, 8)
// The cases of a dispatch function (P, Q, qf, t, a, s, name) for one pair: kernel template K, reported as pre "<P=..,Q=..,QFunction>".
#define CPS_DIAG_CASE(K, pre, Pv, Qv, QFv, nm)                    \
  if (P == Pv && Q == Qv && qf == QFv) {                          \
    *name = pre "<P=" #Pv ",Q=" #Qv "," nm ">";                   \
    return launch_sf<Pv, Qv, K<Pv, Qv, QFv>>(t, a, s);            \
  }
#define CPS_DIAG_CASES(K, pre, Pv, Qv) CPS_DIAG_CASE(K, pre, Pv, Qv, QF_LINELAS, "LinElas") \
  CPS_DIAG_CASE(K, pre, Pv, Qv, QF_HYPERSS_DF, "HyperSSdF") CPS_DIAG_CASE(K, pre, Pv, Qv, QF_HYPERFS_DF, "HyperFSdF")

}  // namespace cps
