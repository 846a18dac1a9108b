// kernels_pointblock.hip -- point-block Jacobi: the 3 x 3 nodal blocks of B^T D B (CeedOperatorLinearAssemblePointBlockDiagonal,
// the matrix PCPBJACOBI inverts), their inverses, and the Chebyshev step that multiplies by them.
//
//   block_n[c'][c] = sum_q sum_{d,d2} g_d(n,q) D^{c'c}_{d d2}(q) g_d2(n,q)
//
// The scalar diagonal (kernels_misc.hip, k_diag_sf) probes the tangent D with nine unit gradients per point and keeps the entries
// with c' == c.  Here nothing is dropped: THREE ROUNDS, one per input component c.  Round c probes with the three unit gradients of
// component c, forms the 18 tensors S^{c'}_pair (3 output components x 6 direction pairs; g_d g_d2 is symmetric in (d, d2), so an
// off-diagonal pair holds D_{d d2} + D_{d2 d} whatever the symmetry of D itself), contracts them with the product tables BB / BG / GG
// exactly as k_diag_sf does, and ends with column c of every node's block.  The LDS slab is therefore k_diag_sf's own (147 KB at
// Q = 8: the dynamic-shared-memory attribute); all 54 tensors at once would not fit from Q = 7.  27 tangent entries are live per round.
// Nothing assumes a symmetric block: the tangent is written as the QFunction gives it.
#include "kernels_common.hpp"
#include "kernels_pointblock.hpp"
#include "qfunctions_device.hpp"

namespace cps {

template <int P, int Q, int QF>
__global__ __launch_bounds__(Geom<Q>::TPE) void k_pbdiag_sf(const BasisTables tab, const PbDiagArgs a) {
  using G = Geom<Q>;
  constexpr int Q3 = G::Q3, P3 = P * P * P, TPE = G::TPE, NT = 18;
  constexpr int PQQ = P * Q * Q, PPQ = P * P * Q, S0 = Q3 > PPQ ? Q3 : PPQ;
  constexpr bool ST_IN = QFTraits<QF>::state_in;
  extern __shared__ double dyn[];
  double *sT = dyn;                  // [3][Q * P]: BB, BG, GG
  double *s0 = sT + 3 * Q * P;       // [NT][Q3] the tensors, later [NT][P * P * Q]
  double *s1 = s0 + NT * S0;         // [NT][P * Q * Q]
  const int q = threadIdx.x, e = blockIdx.x;
  for (int i = q; i < Q * P; i += TPE) {
    const double bb = tab.interp[i], gg = tab.grad[i];
    sT[i] = bb * bb; sT[Q * P + i] = bb * gg; sT[2 * Q * P + i] = gg * gg;
  }
  double qd[10], st[9];
  if (q < Q3) {
    const double *qp = a.qdata + (size_t)e * 10 * Q3 + q;
#pragma unroll
    for (int c = 0; c < 10; c++) qd[c] = qp[c * Q3];
    if constexpr (ST_IN) {
      const double *sp = a.state_in + (size_t)e * 9 * Q3 + q;
#pragma unroll
      for (int c = 0; c < 9; c++) st[c] = sp[c * Q3];
    }
  }
  uint32_t fl_in = 0u, fl_out = 0u;
  if (q < P3) {
    const uint32_t fl = a.offsets[(size_t)e * P3 + q] >> OFF_FLAG_SHIFT;
    fl_in = a.mask_in ? fl : 0u; fl_out = a.mask_out ? fl : 0u;
  }
  // table kind of pair p in direction dir: (d == dir) + (d2 == dir)  (0 BB, 1 BG, 2 GG)
  auto kind = [](int p, int dir) {
    const int d = p < 3 ? p : (p == 5 ? 1 : 0), d2 = p < 3 ? p : (p == 3 ? 1 : 2);
    return (d == dir) + (d2 == dir);
  };
#pragma unroll 1
  for (int c = 0; c < 3; c++) {      // round c: column c of every block
    if (q < Q3) {
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
      for (int co = 0; co < 3; co++) {
        s0[(co * 6 + 0) * Q3 + q] = D[co][0][0];
        s0[(co * 6 + 1) * Q3 + q] = D[co][1][1];
        s0[(co * 6 + 2) * Q3 + q] = D[co][2][2];
        s0[(co * 6 + 3) * Q3 + q] = D[co][0][1] + D[co][1][0];
        s0[(co * 6 + 4) * Q3 + q] = D[co][0][2] + D[co][2][0];
        s0[(co * 6 + 5) * Q3 + q] = D[co][1][2] + D[co][2][1];
      }
    }
    __syncthreads();
    // x: U1[t][k][j][a] = sum_i T(i,a) S[t][k][j][i]
    for (int o = q; o < NT * PQQ; o += TPE) {
      const int t = o / PQQ, r = o % PQQ, aa = r % P, kj = r / P;
      const double *T = sT + kind(t % 6, 0) * Q * P, *src = s0 + t * Q3 + kj * Q;
      double v = 0.;
#pragma unroll
      for (int i = 0; i < Q; i++) v += T[i * P + aa] * src[i];
      s1[o] = v;
    }
    __syncthreads();
    // y: U2[t][k][b][a] = sum_j T(j,b) U1[t][k][j][a]
    for (int o = q; o < NT * PPQ; o += TPE) {
      const int t = o / PPQ, r = o % PPQ, aa = r % P, bb = (r / P) % P, k = r / (P * P);
      const double *T = sT + kind(t % 6, 1) * Q * P, *src = s1 + t * PQQ + k * Q * P + aa;
      double v = 0.;
#pragma unroll
      for (int j = 0; j < Q; j++) v += T[j * P + bb] * src[j * P];
      s0[o] = v;
    }
    __syncthreads();
    // z, and the sum over the pairs: one node per thread; entry (c', c) of its block
    if (q < P3) {
      const int ab = q % (P * P), nc = q / (P * P);
      double *out = a.evec + ((size_t)e * P3 + q) * 9 + c;
      const bool dead_in = (fl_in >> c) & 1u;
#pragma unroll
      for (int co = 0; co < 3; co++) {
        double acc = 0.;
#pragma unroll
        for (int p = 0; p < 6; p++) {
          const double *T = sT + kind(p, 2) * Q * P, *src = s0 + (co * 6 + p) * PPQ + ab;
          double v = 0.;
#pragma unroll
          for (int k = 0; k < Q; k++) v += T[k * P + nc] * src[k * P * P];
          acc += v;
        }
        out[co * 3] = (dead_in || ((fl_out >> co) & 1u)) ? 0. : acc;
      }
    }
    __syncthreads();   // the next round overwrites s0
  }
}
template <int P, int Q, int QF>
static hipError_t pbdiag_t(const BasisTables &t, const PbDiagArgs &a, hipStream_t s) {
  using G = Geom<Q>;
  if (a.nelem <= 0) return hipSuccess;
  static_assert(P * P * P <= G::TPE, "a lane per node in the last pass");
  constexpr int PQQ = P * Q * Q, PPQ = P * P * Q, S0 = G::Q3 > PPQ ? G::Q3 : PPQ;
  constexpr size_t lds = sizeof(double) * (3 * Q * P + 18 * (S0 + PQQ));
  static_assert(lds <= 160 * 1024, "the slab fits the CU's LDS");
  static bool attr_set = false;
  if (!attr_set) {
    hipError_t er = hipFuncSetAttribute((const void *)k_pbdiag_sf<P, Q, QF>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (er != hipSuccess) return er;
    attr_set = true;
  }
  hipLaunchKernelGGL((k_pbdiag_sf<P, Q, QF>), dim3(a.nelem), dim3(G::TPE), lds, s, t, a);
  return hipGetLastError();
}
hipError_t launch_pbdiag(int P, int Q, int qf, const BasisTables &t, const PbDiagArgs &a, hipStream_t s, const char **name) {
#define CPS_PB(Pv, Qv, QFv, nm)                                   \
  if (P == Pv && Q == Qv && qf == QFv) {                          \
    *name = "pbdiag<P=" #Pv ",Q=" #Qv "," nm ">";                 \
    return pbdiag_t<Pv, Qv, QFv>(t, a, s);                        \
  }
#define CPS_PB3(Pv, Qv) CPS_PB(Pv, Qv, QF_LINELAS, "LinElas") CPS_PB(Pv, Qv, QF_HYPERSS_DF, "HyperSSdF") \
  CPS_PB(Pv, Qv, QF_HYPERFS_DF, "HyperFSdF")
  // the (P, Q) set of the scalar diagonal (launch_diag)
  CPS_PB3(2, 2) CPS_PB3(2, 3) CPS_PB3(3, 3) CPS_PB3(2, 4) CPS_PB3(3, 4) CPS_PB3(4, 4)
  CPS_PB3(2, 5) CPS_PB3(3, 5) CPS_PB3(4, 5) CPS_PB3(5, 5) CPS_PB3(2, 7) CPS_PB3(3, 7) CPS_PB3(5, 7) CPS_PB3(7, 7)
  CPS_PB3(2, 6) CPS_PB3(3, 6) CPS_PB3(4, 6) CPS_PB3(5, 6) CPS_PB3(6, 6) CPS_PB3(4, 7) CPS_PB3(6, 7)
  CPS_PB3(2, 8) CPS_PB3(3, 8) CPS_PB3(4, 8) CPS_PB3(5, 8) CPS_PB3(6, 8) CPS_PB3(7, 8) CPS_PB3(8, 8)
#undef CPS_PB3
#undef CPS_PB
  return hipErrorInvalidValue;
}

// One lane per L-node, the contributors summed in element order as k_assemble sums them; nine values per contributor.
__global__ void k_pb_assemble(const uint32_t *rowptr, const uint32_t *cols, const uint32_t *node_off, const double *evec,
                              double *blocks, int nnodes) {
  for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < nnodes; r += gridDim.x * blockDim.x) {
    double acc[9];
#pragma unroll
    for (int j = 0; j < 9; j++) acc[j] = 0.;
    for (uint32_t k = rowptr[r]; k < rowptr[r + 1]; k++) {
      const double *p = evec + (size_t)cols[k] * 9;
#pragma unroll
      for (int j = 0; j < 9; j++) acc[j] += p[j];
    }
    double *dst = blocks + 3 * (size_t)(node_off[r] & OFF_MASK);
#pragma unroll
    for (int j = 0; j < 9; j++) dst[j] = acc[j];
  }
}

static inline dim3 node_grid(size_t n) {
  size_t b = (n + 255) / 256;
  return dim3((unsigned)(b < 1 ? 1 : (b > 2048 ? 2048 : b)));
}

// Inverse of the principal sub-block of the kept components, embedded in zeros.  A dropped component is replaced by a unit row and
// column first (products with 1 and 0 are exact), so one code path serves all eight patterns: inverse = adjugate / determinant, the
// pivots of the elimination without interchanges (all positive iff the block is positive definite) decide what is counted as bad.
__global__ void k_pb_invert(double *blocks, size_t nnodes, int *n_bad) {
#pragma clang fp contract(off)
  int nb = 0;
  for (size_t n = blockIdx.x * (size_t)blockDim.x + threadIdx.x; n < nnodes; n += (size_t)gridDim.x * blockDim.x) {
    double *B = blocks + 9 * n;
    double m[3][3];
    bool keep[3];
#pragma unroll
    for (int i = 0; i < 3; i++) keep[i] = B[4 * i] != 0.;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 3; j++) m[i][j] = (keep[i] && keep[j]) ? B[3 * i + j] : (i == j ? 1. : 0.);
    const double p0 = m[0][0];
    const double l1 = m[1][0] / p0, l2 = m[2][0] / p0;
    const double b11 = m[1][1] - l1 * m[0][1], b12 = m[1][2] - l1 * m[0][2];
    const double b21 = m[2][1] - l2 * m[0][1], b22 = m[2][2] - l2 * m[0][2];
    const double p1 = b11, p2 = b22 - (b21 / p1) * b12;
    const double big = 1.7976931348623157e308;
    if (!(p0 > 0. && p0 <= big && p1 > 0. && p1 <= big && p2 > 0. && p2 <= big)) nb++;
    const double c00 = m[1][1] * m[2][2] - m[1][2] * m[2][1];
    const double c01 = m[1][2] * m[2][0] - m[1][0] * m[2][2];
    const double c02 = m[1][0] * m[2][1] - m[1][1] * m[2][0];
    const double det = (m[0][0] * c00 + m[0][1] * c01) + m[0][2] * c02;
    double inv[3][3];
    inv[0][0] = c00 / det;
    inv[1][0] = c01 / det;
    inv[2][0] = c02 / det;
    inv[0][1] = (m[0][2] * m[2][1] - m[0][1] * m[2][2]) / det;
    inv[1][1] = (m[0][0] * m[2][2] - m[0][2] * m[2][0]) / det;
    inv[2][1] = (m[0][1] * m[2][0] - m[0][0] * m[2][1]) / det;
    inv[0][2] = (m[0][1] * m[1][2] - m[0][2] * m[1][1]) / det;
    inv[1][2] = (m[0][2] * m[1][0] - m[0][0] * m[1][2]) / det;
    inv[2][2] = (m[0][0] * m[1][1] - m[0][1] * m[1][0]) / det;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 3; j++) B[3 * i + j] = (keep[i] && keep[j]) ? inv[i][j] : 0.;
  }
  if (n_bad) {     // (every lane of the wave is back here: one atomic per wave that has something to report)
    for (int o = 32; o > 0; o >>= 1) nb += __shfl_down(nb, o, 64);
    if ((threadIdx.x & 63) == 0 && nb) atomicAdd(n_bad, nb);
  }
}

CPS_DEV void pb_mult3(const double *B, double r0, double r1, double r2, double *z) {
#pragma clang fp contract(off)
#pragma unroll
  for (int i = 0; i < 3; i++) z[i] = (B[3 * i] * r0 + B[3 * i + 1] * r1) + B[3 * i + 2] * r2;
}
__global__ void k_pb_mult(double *w, const double *blocks, const double *x, size_t nnodes) {
  for (size_t n = blockIdx.x * (size_t)blockDim.x + threadIdx.x; n < nnodes; n += (size_t)gridDim.x * blockDim.x) {
    double B[9], z[3];
#pragma unroll
    for (int j = 0; j < 9; j++) B[j] = blocks[9 * n + j];
    const double x0 = x[3 * n], x1 = x[3 * n + 1], x2 = x[3 * n + 2];
    pb_mult3(B, x0, x1, x2, z);
    w[3 * n] = z[0]; w[3 * n + 1] = z[1]; w[3 * n + 2] = z[2];
  }
}
// One node of a Chebyshev step with blocks: cheb_dof's definition (kernels_misc.hip) with dinv .* r replaced by B_n r_n; explicit
// operation order, no contraction left to the compiler.
__global__ void k_pb_cheb_step(double *x, double *d, double *r, const double *b, const double *t, const double *blocks, double c1,
                               double c2, int assign_x, size_t nnodes) {
#pragma clang fp contract(off)
  for (size_t n = blockIdx.x * (size_t)blockDim.x + threadIdx.x; n < nnodes; n += (size_t)gridDim.x * blockDim.x) {
    double B[9], ri[3], z[3];
#pragma unroll
    for (int j = 0; j < 9; j++) B[j] = blocks[9 * n + j];
#pragma unroll
    for (int c = 0; c < 3; c++) ri[c] = t ? b[3 * n + c] - t[3 * n + c] : b[3 * n + c];
    if (r) { r[3 * n] = ri[0]; r[3 * n + 1] = ri[1]; r[3 * n + 2] = ri[2]; }
    pb_mult3(B, ri[0], ri[1], ri[2], z);
#pragma unroll
    for (int c = 0; c < 3; c++) {
      double di = c1 * z[c];
      if (c2 != 0.) di = __builtin_fma(c2, d[3 * n + c], di);
      const double xi = assign_x ? 0. : x[3 * n + c];
      d[3 * n + c] = di;
      x[3 * n + c] = assign_x ? di : xi + di;
    }
  }
}

hipError_t launch_pb_assemble(const uint32_t *rowptr, const uint32_t *cols, const uint32_t *node_off, const double *evec,
                              double *blocks, int nnodes, hipStream_t s) {
  if (nnodes <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_pb_assemble, node_grid((size_t)nnodes), dim3(256), 0, s, rowptr, cols, node_off, evec, blocks, nnodes);
  return hipGetLastError();
}
hipError_t launch_pb_invert(double *blocks, size_t nnodes, int *n_bad, hipStream_t s) {
  if (!nnodes) return hipSuccess;
  hipLaunchKernelGGL(k_pb_invert, node_grid(nnodes), dim3(256), 0, s, blocks, nnodes, n_bad);
  return hipGetLastError();
}
hipError_t launch_pb_mult(double *w, const double *blocks, const double *x, size_t nnodes, hipStream_t s) {
  if (!nnodes) return hipSuccess;
  hipLaunchKernelGGL(k_pb_mult, node_grid(nnodes), dim3(256), 0, s, w, blocks, x, nnodes);
  return hipGetLastError();
}
hipError_t launch_pb_cheb_step(double *x, double *d, double *r, const double *b, const double *t, const double *blocks, double c1,
                               double c2, int assign_x, size_t nnodes, hipStream_t s) {
  if (!nnodes) return hipSuccess;
  hipLaunchKernelGGL(k_pb_cheb_step, node_grid(nnodes), dim3(256), 0, s, x, d, r, b, t, blocks, c1, c2, assign_x, nnodes);
  return hipGetLastError();
}

}  // namespace cps
