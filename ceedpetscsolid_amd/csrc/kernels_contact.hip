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
// Mapping, LDS layout and the steps every face kernel takes: kernel_face_pass.hpp.  Here -- residual: X and x = X + u are gathered, X
// gets B and D of every line and x gets B, the point work is the obstacle and the seven coalesced state stores.  Tangent: du is gathered
// (flagged components as zeros) and gets B, the point work is K_q du_q; no D table.  Diagonal: K_q[c][c] at a lane per point and the way
// back with the entry-wise squared table (the host passes it, as for k_mass's diagonal).  The obstacle is uniform over the launch.
//
// The spring and dashpot supports (ceed_support.cpp) are two further modes of the same kernel.  Their K_q = w_q J_q [k_t I + (k_n - k_t) n (x) n],
// n = X_xi x X_eta / J (its sign is immaterial), is fixed in the reference configuration.  Support state: X alone is gathered and gets B and
// D of every line, the point work is J, n and the seven coalesced state stores -- K_q, then w_q J_q, whose sum is the area of the faces --
// and there the kernel ends: no way back to the nodes, no E-vector.  A point with J = 0 gets n = 0.  Support force: the tangent's data path
// on a field that is read AS IT IS (a displacement or a velocity carries the prescribed motion of a rim shared with a clamped set, which
// a variation's zeros would drop).  A support's tangent and diagonal are the tangent and diagonal modes on the support state.
#include "kernel_diag_sf.hpp"      // CPS_DIAG_PQ: the one list of (P, Q) pairs
#include "kernel_face_pass.hpp"

namespace cps {

template <int P, int Q, int MODE> struct ContactGeom : FaceGeom<P, Q> {
  using F = FaceGeom<P, Q>;
  static constexpr bool FIELD = MODE == CONTACT_TANGENT || MODE == CONTACT_SUPPORT_FORCE;                     // one gathered field, B alone
  static constexpr int NIN = MODE == CONTACT_RESIDUAL ? 2 * F::NX : (FIELD || MODE == CONTACT_SUPPORT_STATE ? F::NX : 0);   // X, x; du; X; nothing
  static constexpr int NT1 = MODE == CONTACT_RESIDUAL ? 3 * F::N1 : (MODE == CONTACT_SUPPORT_STATE ? 2 * F::N1 : (FIELD ? F::N1 : 0));   // B X, D X, B x; B X, D X; B du
  static constexpr int NBACK = MODE == CONTACT_SUPPORT_STATE ? 0 : F::NV + F::NR;                            // the way back to the nodes
  static constexpr int NF = NIN + NT1 + NBACK;          // doubles per face
  static_assert((size_t)(F::NTAB + F::FPW * NF) * sizeof(double) <= 64 * 1024, "static LDS of one workgroup");
};

template <int P, int Q, int MODE>
__global__ __launch_bounds__(64) void k_contact(const BasisTables tab, const ContactArgs a) {
  using G = ContactGeom<P, Q, MODE>;
  constexpr int P2 = G::P2, Q2 = G::Q2, NX = G::NX, N1 = G::N1;
  __shared__ double lds[G::NTAB + G::FPW * G::NF];
  const double *sB = lds, *sD = lds + Q * P, *sW = lds + 2 * Q * P;
  const FaceLane L = face_lane<G>(a.nface);
  const int t = L.t;
  const bool live = L.live;
  double *sin = lds + G::NTAB + (live ? L.fl : 0) * G::NF, *t1 = sin + G::NIN, *sv = t1 + G::NT1, *sr = sv + G::NV;
  double *st = a.state + ((size_t)(live ? L.face : 0) * CONTACT_NSTATE) * Q2 + t;    // entry k of this lane's point: st[k * Q2]
  face_tables<P, Q>(tab, lds);
  // the node records: X and x = X + u (residual); du with its flagged components as zeros (tangent); X (support state); the field as
  // it is (support force)
  if (MODE != CONTACT_DIAGONAL && live && t < P2) {
    const uint32_t off = a.offsets[(size_t)L.face * P2 + t];
    double v[3], w[3];
    if (MODE == CONTACT_RESIDUAL) {
      face_record<false>(a.X, off, v); face_record<false>(a.u, off, w);
      face_put<P2>(sin, t, v);
#pragma unroll
      for (int c = 0; c < 3; c++) w[c] = v[c] + w[c];
      face_put<P2>(sin + NX, t, w);
    } else {
      if (MODE == CONTACT_SUPPORT_STATE) face_record<false>(a.X, off, v);
      else if (MODE == CONTACT_SUPPORT_FORCE) face_record<false>(a.du, off, v);
      else face_record<true>(a.du, off, v);
      face_put<P2>(sin, t, v);
    }
  }
  __syncthreads();
  // xi: the values of every line at the Q points -- residual: t1[0] = B X, t1[1] = D X, t1[2] = B x; support state: t1[0] = B X,
  // t1[1] = D X; tangent, support force: t1[0] = B du
  if (MODE != CONTACT_DIAGONAL && live) {
    for (int o = t; o < N1; o += Q2) {
      const int aa = o % Q, line = o / Q;
      const double *src = sin + line * P, *B = sB + aa * P;
      if (MODE == CONTACT_RESIDUAL) {
        double vb, vd;
        face_dot2<P, 1>(B, src, sD + aa * P, src, vb, vd);
        const double xb = face_dot<P, 1>(B, src + NX);
        t1[o] = vb; t1[N1 + o] = vd; t1[2 * N1 + o] = xb;
      } else if (MODE == CONTACT_SUPPORT_STATE) {
        double vb, vd;
        face_dot2<P, 1>(B, src, sD + aa * P, src, vb, vd);
        t1[o] = vb; t1[N1 + o] = vd;
      } else {
        t1[o] = face_dot<P, 1>(B, src);
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
        face_dot2<P, Q>(B, vd, D, vb, Xa[c], Xb[c]); x[c] = face_dot<P, Q>(B, xb);
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
    } else if (MODE == CONTACT_SUPPORT_STATE) {
      const double *D = sD + bb * P;
      double Xa[3], Xb[3];                             // X_xi, X_eta at the point
#pragma unroll
      for (int c = 0; c < 3; c++) {
        const double *vb = t1 + c * P * Q + aa, *vd = vb + N1;
        face_dot2<P, Q>(B, vd, D, vb, Xa[c], Xb[c]);
      }
      double m[3];
#pragma unroll
      for (int c = 0; c < 3; c++) {
        const int c1 = (c + 1) % 3, c2 = (c + 2) % 3;
        m[c] = Xa[c1] * Xb[c2] - Xa[c2] * Xb[c1];
      }
      const double J = sqrt(m[0] * m[0] + m[1] * m[1] + m[2] * m[2]), jinv = J > 0. ? 1. / J : 0.;
      const double n[3] = {m[0] * jinv, m[1] * jinv, m[2] * jinv};
      const double wj = sW[aa] * sW[bb] * J, k0 = wj * a.par[1], k1 = wj * (a.par[0] - a.par[1]);   // K = k0 I + k1 n (x) n
      st[0 * Q2] = k0 + k1 * n[0] * n[0];
      st[1 * Q2] = k0 + k1 * n[1] * n[1];
      st[2 * Q2] = k0 + k1 * n[2] * n[2];
      st[3 * Q2] = k1 * n[1] * n[2];
      st[4 * Q2] = k1 * n[0] * n[2];
      st[5 * Q2] = k1 * n[0] * n[1];
      st[6 * Q2] = wj;
    } else if (G::FIELD) {
      const double *vb = t1 + aa;
      const double d[3] = {face_dot<P, Q>(B, vb), face_dot<P, Q>(B, vb + P * Q), face_dot<P, Q>(B, vb + 2 * P * Q)};
      const double kxx = st[0 * Q2], kyy = st[1 * Q2], kzz = st[2 * Q2], kyz = st[3 * Q2], kxz = st[4 * Q2], kxy = st[5 * Q2];
      v[0] = a.scale * (kxx * d[0] + kxy * d[1] + kxz * d[2]);
      v[1] = a.scale * (kxy * d[0] + kyy * d[1] + kyz * d[2]);
      v[2] = a.scale * (kxz * d[0] + kyz * d[1] + kzz * d[2]);
    } else {
#pragma unroll
      for (int c = 0; c < 3; c++) v[c] = a.scale * st[c * Q2];
    }
    if (MODE != CONTACT_SUPPORT_STATE) {
#pragma unroll
      for (int c = 0; c < 3; c++) sv[c * Q2 + t] = v[c];
    }
  }
  if (MODE == CONTACT_SUPPORT_STATE) return;           // (the state is all this mode leaves)
  __syncthreads();
  face_to_nodes<P, Q>(sB, sv, sr, a.evec, L.face, t, live);
}

hipError_t launch_contact(int P, int Q, int mode, const BasisTables &t, const ContactArgs &a, hipStream_t s, const char **name) {
#define CPS_CM(Pv, Qv, MODE, word)                                                                 \
  if (P == Pv && Q == Qv && mode == MODE) {                                                        \
    *name = "contact<P=" #Pv ",Q=" #Qv "," word ">";                                               \
    return launch_faces<FaceGeom<Pv, Qv>::FPW>(k_contact<Pv, Qv, MODE>, t, a, s);                  \
  }
#define CPS_CT(Pv, Qv) CPS_CM(Pv, Qv, CONTACT_RESIDUAL, "residual") CPS_CM(Pv, Qv, CONTACT_TANGENT, "tangent") CPS_CM(Pv, Qv, CONTACT_DIAGONAL, "diagonal") \
                       CPS_CM(Pv, Qv, CONTACT_SUPPORT_STATE, "support_state") CPS_CM(Pv, Qv, CONTACT_SUPPORT_FORCE, "support_force")
  CPS_DIAG_PQ(CPS_CT)
#undef CPS_CT
#undef CPS_CM
  return hipErrorInvalidValue;
}
bool contact_instantiated(int P, int Q) {
#define CPS_CT(Pv, Qv) if (P == Pv && Q == Qv) return true;
  CPS_DIAG_PQ(CPS_CT)
#undef CPS_CT
  return false;
}

}  // namespace cps
