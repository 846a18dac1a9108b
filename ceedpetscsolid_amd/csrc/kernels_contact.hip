// kernels_contact.hip -- frictionless penalty contact of element faces with a rigid analytic obstacle (a plane or a sphere).
//
// A face has the P^2 face nodes of its element, (xi, eta) its two in-face reference directions (xi fastest in the node list), x = X + u
// the current position, J = |X_xi x X_eta| the REFERENCE area element, g(x) the signed distance to the obstacle (g > 0: separated),
// n = grad g and eps the penalty per unit reference area.  With the potential Pi(u) = int 1/2 eps <-g>^2 dA0, k_contact forms per face
//   residual  r_a      = -sum_q N_a(q) w_q J_q eps <-g> n
//   tangent   C du |_a =  sum_q N_a(q) K_q du(q),   K_q = w_q J_q eps [H(-g) n (x) n - <-g> grad grad g]      (symmetric)
//   diagonal  d_{a,c}  =  sum_q N_a(q)^2 K_q[c][c]
// on the Q^2 Gauss points of the face and leaves the nodal values in a face E-vector [face][P^2][3]; k_surface_sum (kernels_surface.hip)
// adds them into y per row of the faces' transpose map, in face order.  The residual stores K_q (xx, yy, zz, yz, xz, xy) and the gap g
// per point, [face][7][Q^2]; the tangent and the diagonal read that state and nothing else of the configuration, so a coarse p-level
// (its own P, the fine Q) needs no obstacle, no coordinates and no displacement.  grad grad g = 0 for the plane and s (I - n (x) n) / |x - c|
// for the sphere.
//
// Mapping (k_surface's): one wave64 per workgroup owns FPW = max(1, 64 / Q^2) faces, a face owns S = Q^2 lanes (Q >= P: a lane per point,
// and per node in the last pass).  Residual: the gather of the 24-byte node records (X and X + u), the xi pass (B and D of every line of
// X, B of x), the eta pass with the obstacle at a lane per point and the seven coalesced state stores, then the two transposed passes
// back to the nodes.  Tangent: gather du (flagged components as zeros), two B passes, K_q du_q, two transposed passes; no D table.
// Diagonal: K_q[c][c] at a lane per point and the two transposed passes with the entry-wise squared table (the host passes it, as for
// k_mass's diagonal).  The obstacle is uniform over the launch.  No atomics, no scratch memory, no waiting on other waves.
#include "kernel_diag_sf.hpp"      // CPS_DIAG_PQ: the one list of (P, Q) pairs
#include "kernels_common.hpp"

namespace cps {

template <int P, int Q, int MODE> struct ContactGeom {
  static_assert(Q >= P && Q <= MAXN1D && P >= 2, "a lane per point covers the nodes too");
  static constexpr int P2 = P * P, Q2 = Q * Q;
  static constexpr int S = Q2;                         // lanes of a face
  static constexpr int FPW = 64 / S < 1 ? 1 : 64 / S;  // faces of a wave
  static constexpr int NX = 3 * P2;                    // a gathered field         [c][j][i]
  static constexpr int N1 = 3 * P * Q;                 // one result of the xi pass [c][j][a]
  static constexpr int NV = 3 * Q2;                    // the values at the points  [c][b][a]
  static constexpr int NR = 3 * Q * P;                 // first transposed pass     [c][b][i]
  static constexpr int NIN = MODE == CONTACT_RESIDUAL ? 2 * NX : (MODE == CONTACT_TANGENT ? NX : 0);   // X, x; du; nothing
  static constexpr int NT1 = MODE == CONTACT_RESIDUAL ? 3 * N1 : (MODE == CONTACT_TANGENT ? N1 : 0);   // B X, D X, B x; B du
  static constexpr int NF = NIN + NT1 + NV + NR;       // doubles per face
  static constexpr int NTAB = 2 * Q * P + Q;           // B[a][i], D[a][i], weights
  static_assert((size_t)(NTAB + FPW * NF) * sizeof(double) <= 64 * 1024, "static LDS of one workgroup");
};

template <int P, int Q, int MODE>
__global__ __launch_bounds__(64) void k_contact(const BasisTables tab, const ContactArgs a) {
  using G = ContactGeom<P, Q, MODE>;
  constexpr int P2 = G::P2, Q2 = G::Q2, S = G::S, FPW = G::FPW, NX = G::NX, N1 = G::N1;
  __shared__ double lds[G::NTAB + FPW * G::NF];
  double *sB = lds, *sD = lds + Q * P, *sW = lds + 2 * Q * P;
  const int lane = threadIdx.x, fl = lane / S, t = lane % S;
  const int face = blockIdx.x * FPW + fl;
  const bool live = fl < FPW && face < a.nface;        // (64 % S lanes of the wave own no face)
  double *sin = lds + G::NTAB + (live ? fl : 0) * G::NF, *t1 = sin + G::NIN, *sv = t1 + G::NT1, *sr = sv + G::NV;
  double *st = a.state + ((size_t)(live ? face : 0) * CONTACT_NSTATE) * Q2 + t;      // entry k of this lane's point: st[k * Q2]
  for (int i = lane; i < Q * P; i += 64) { sB[i] = tab.interp[i]; sD[i] = tab.grad[i]; }
  if (lane < Q) sW[lane] = tab.qw[lane];
  // the node records: X and x = X + u (residual); du with its flagged components as zeros (tangent)
  if (MODE != CONTACT_DIAGONAL && live && t < P2) {
    const uint32_t off = a.offsets[(size_t)face * P2 + t];
    const uint32_t o = off & OFF_MASK, flg = off >> OFF_FLAG_SHIFT;
#pragma unroll
    for (int c = 0; c < 3; c++) {
      if (MODE == CONTACT_RESIDUAL) {
        const double xv = a.X[o + c];
        sin[c * P2 + t] = xv;
        sin[NX + c * P2 + t] = xv + a.u[o + c];
      } else {
        sin[c * P2 + t] = ((flg >> c) & 1u) ? 0. : a.du[o + c];
      }
    }
  }
  __syncthreads();
  // xi: per line (c, j) the values at the Q points -- residual: t1[0] = B X, t1[1] = D X, t1[2] = B x; tangent: t1[0] = B du
  if (MODE != CONTACT_DIAGONAL && live) {
    for (int o = t; o < N1; o += S) {
      const int aa = o % Q, line = o / Q;
      const double *src = sin + line * P, *B = sB + aa * P;
      double vb = 0.;
#pragma unroll
      for (int i = 0; i < P; i++) vb += B[i] * src[i];
      t1[o] = vb;
      if (MODE == CONTACT_RESIDUAL) {
        const double *D = sD + aa * P, *cur = src + NX;
        double vd = 0., xb = 0.;
#pragma unroll
        for (int i = 0; i < P; i++) { vd += D[i] * src[i]; xb += B[i] * cur[i]; }
        t1[N1 + o] = vd; t1[2 * N1 + o] = xb;
      }
    }
  }
  __syncthreads();
  // eta and the point work: a lane per point
  if (live) {
    const int aa = t % Q, bb = t / Q;
    const double *B = sB + bb * P;
    double v[3];
    if (MODE == CONTACT_RESIDUAL) {
      const double *D = sD + bb * P;
      double Xa[3], Xb[3], x[3];                       // X_xi, X_eta, x at the point
#pragma unroll
      for (int c = 0; c < 3; c++) {
        const double *vb = t1 + c * P * Q + aa, *vd = vb + N1, *xb = vb + 2 * N1;
        double s0 = 0., s1 = 0., s2 = 0.;
#pragma unroll
        for (int j = 0; j < P; j++) { s0 += B[j] * vd[j * Q]; s1 += D[j] * vb[j * Q]; s2 += B[j] * xb[j * Q]; }
        Xa[c] = s0; Xb[c] = s1; x[c] = s2;
      }
      double m[3];
#pragma unroll
      for (int c = 0; c < 3; c++) {
        const int c1 = (c + 1) % 3, c2 = (c + 2) % 3;
        m[c] = Xa[c1] * Xb[c2] - Xa[c2] * Xb[c1];
      }
      const double wje = sW[aa] * sW[bb] * sqrt(m[0] * m[0] + m[1] * m[1] + m[2] * m[2]) * a.penalty;
      double n[3], g, h;                               // n = grad g; grad grad g = h (I - n (x) n)
      if (a.kind == CONTACT_PLANE) {
        n[0] = a.par[3]; n[1] = a.par[4]; n[2] = a.par[5];
        g = (x[0] - a.par[0]) * n[0] + (x[1] - a.par[1]) * n[1] + (x[2] - a.par[2]) * n[2];
        h = 0.;
      } else {
        const double d0 = x[0] - a.par[0], d1 = x[1] - a.par[1], d2 = x[2] - a.par[2], sgn = a.par[4];
        const double r = sqrt(d0 * d0 + d1 * d1 + d2 * d2), rinv = r > 0. ? 1. / r : 0.;
        n[0] = sgn * d0 * rinv; n[1] = sgn * d1 * rinv; n[2] = sgn * d2 * rinv;
        g = sgn * (r - a.par[3]);
        h = sgn * rinv;
      }
      const bool act = g < 0.;
      const double pen = act ? -g : 0.;
      const double k0 = wje * pen * h, k1 = (act ? wje : 0.) + k0;      // K = k1 n (x) n - k0 I
      st[0 * Q2] = k1 * n[0] * n[0] - k0;
      st[1 * Q2] = k1 * n[1] * n[1] - k0;
      st[2 * Q2] = k1 * n[2] * n[2] - k0;
      st[3 * Q2] = k1 * n[1] * n[2];
      st[4 * Q2] = k1 * n[0] * n[2];
      st[5 * Q2] = k1 * n[0] * n[1];
      st[6 * Q2] = g;
      const double f = -a.scale * wje * pen;
#pragma unroll
      for (int c = 0; c < 3; c++) v[c] = f * n[c];
    } else if (MODE == CONTACT_TANGENT) {
      double d[3];
#pragma unroll
      for (int c = 0; c < 3; c++) {
        const double *vb = t1 + c * P * Q + aa;
        double s0 = 0.;
#pragma unroll
        for (int j = 0; j < P; j++) s0 += B[j] * vb[j * Q];
        d[c] = s0;
      }
      const double kxx = st[0 * Q2], kyy = st[1 * Q2], kzz = st[2 * Q2], kyz = st[3 * Q2], kxz = st[4 * Q2], kxy = st[5 * Q2];
      v[0] = a.scale * (kxx * d[0] + kxy * d[1] + kxz * d[2]);
      v[1] = a.scale * (kxy * d[0] + kyy * d[1] + kyz * d[2]);
      v[2] = a.scale * (kxz * d[0] + kyz * d[1] + kzz * d[2]);
    } else {
#pragma unroll
      for (int c = 0; c < 3; c++) v[c] = a.scale * st[c * Q2];
    }
#pragma unroll
    for (int c = 0; c < 3; c++) sv[c * Q2 + t] = v[c];
  }
  __syncthreads();
  // back along xi: sr[c][b][i] = sum_a B[a][i] v[c][b][a]
  if (live) {
    for (int o = t; o < G::NR; o += S) {
      const int i = o % P, cb = o / P;
      const double *src = sv + cb * Q;
      double r = 0.;
#pragma unroll
      for (int q = 0; q < Q; q++) r += sB[q * P + i] * src[q];
      sr[o] = r;
    }
  }
  __syncthreads();
  // back along eta and the stores: a lane per node, 24-byte records in node order
  if (live && t < P2) {
    const int i = t % P, j = t / P;
    double *out = a.evec + ((size_t)face * P2 + t) * 3;
#pragma unroll
    for (int c = 0; c < 3; c++) {
      double g = 0.;
#pragma unroll
      for (int b = 0; b < Q; b++) g += sB[b * P + j] * sr[(c * Q + b) * P + i];
      out[c] = g;
    }
  }
}

template <int P, int Q, int MODE>
static hipError_t contact_t(const BasisTables &t, const ContactArgs &a, hipStream_t s) {
  if (a.nface <= 0) return hipSuccess;
  constexpr int FPW = ContactGeom<P, Q, MODE>::FPW;
  hipLaunchKernelGGL((k_contact<P, Q, MODE>), dim3((a.nface + FPW - 1) / FPW), dim3(64), 0, s, t, a);
  return hipGetLastError();
}

hipError_t launch_contact(int P, int Q, int mode, const BasisTables &t, const ContactArgs &a, hipStream_t s, const char **name) {
#define CPS_CT(Pv, Qv)                                                                             \
  if (P == Pv && Q == Qv) {                                                                        \
    if (mode == CONTACT_RESIDUAL) {                                                                \
      *name = "contact<P=" #Pv ",Q=" #Qv ",residual>";                                             \
      return contact_t<Pv, Qv, CONTACT_RESIDUAL>(t, a, s);                                         \
    }                                                                                              \
    if (mode == CONTACT_TANGENT) {                                                                 \
      *name = "contact<P=" #Pv ",Q=" #Qv ",tangent>";                                              \
      return contact_t<Pv, Qv, CONTACT_TANGENT>(t, a, s);                                          \
    }                                                                                              \
    if (mode == CONTACT_DIAGONAL) {                                                                \
      *name = "contact<P=" #Pv ",Q=" #Qv ",diagonal>";                                             \
      return contact_t<Pv, Qv, CONTACT_DIAGONAL>(t, a, s);                                         \
    }                                                                                              \
  }
  CPS_DIAG_PQ(CPS_CT)
#undef CPS_CT
  return hipErrorInvalidValue;
}
bool contact_instantiated(int P, int Q) {
#define CPS_CT(Pv, Qv) if (P == Pv && Q == Qv) return true;
  CPS_DIAG_PQ(CPS_CT)
#undef CPS_CT
  return false;
}

}  // namespace cps
