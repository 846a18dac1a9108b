// kernels_surface.hip -- surface loads on element faces: dead traction, follower pressure and the pressure's exact tangent.
//
// A loaded face has the P^2 face nodes of its element, (xi, eta) its two in-face reference directions (xi fastest in the node list,
// ordered on the host so that X_xi x X_eta points out of the body), x = X + u the current position.  k_surface forms, per face,
//   traction  g_a     = sum_q w_q N_a(q) t |X_xi x X_eta|               dead load per unit reference area
//   pressure  g_a(u)  = sum_q w_q N_a(q) (x_xi x x_eta)                 area-weighted current outward normal, quadratic in u
//   tangent   T du |_a = sum_q w_q N_a(q) (du_xi x x_eta + x_xi x du_eta)  the derivative of g(u) in the direction du
// on the Q^2 Gauss points of the face (exact: the integrands have degree <= 2 p - 1 per direction once summed over a), and leaves the
// nodal values in a face E-vector [face][P^2][3]; k_surface_sum adds them into y per row of the faces' transpose map, in face order.
// Signs and loads are the caller's: the coefficients arrive multiplied by the caller's scale.
//
// Mapping, LDS layout and the steps every face kernel takes: kernel_face_pass.hpp.  Here: x = X (+ u) and du are gathered, both get B
// and D of every line, and the point work is the cross product(s) and the weight.  `kind` is uniform over the launch.
// k_surface<P, Q, true> serves the five kinds of loads that vary over the faces (a nodal traction or pressure field, the hydrostatic
// pressure of a fluid at rest, and the two followers' tangents) with the same passes: surface_field_face below.
#include "kernel_face_pass.hpp"
#include "kernel_node_sum.hpp"
#include <type_traits>

namespace cps {

template <int P, int Q> struct SurfGeom : FaceGeom<P, Q> {
  using F = FaceGeom<P, Q>;
  static constexpr int NF = 2 * F::NX + 4 * F::N1 + F::NV + F::NR;   // doubles per face: x, du; (B, D) x (x, du); values; first transposed pass
  static_assert((size_t)(F::NTAB + F::FPW * NF) * sizeof(double) <= 64 * 1024, "static LDS of one workgroup");
};

// Loads that vary over the faces (FIELD): one more gathered field -- a nodal traction (an L-vector) or a nodal pressure (a value per
// node) -- with a B-only xi pass of its own, and the VALUES of x and du at the point beside their derivatives (the hydrostatic kinds).
template <int P, int Q> struct SurfFieldGeom : FaceGeom<P, Q> {
  using F = FaceGeom<P, Q>;
  static constexpr int NF = 3 * F::NX + 5 * F::N1 + F::NV + F::NR;   // doubles per face: x, du, field; (B, D) x (x, du), B x field; values; first transposed pass
  static_assert((size_t)(F::NTAB + F::FPW * NF) * sizeof(double) <= 64 * 1024, "static LDS of one workgroup");
};

// The FIELD kinds, per face (kernels.hpp, SurfaceKind): the steps of the kernel below with the field's gather and passes beside them.
// coef[0] is the caller's scale (times gamma for the hydrostatic kinds).
template <int P, int Q> CPS_DEV void surface_field_face(const BasisTables &tab, const SurfaceFieldArgs &a) {
  using G = SurfFieldGeom<P, Q>;
  constexpr int P2 = G::P2, Q2 = G::Q2, NX = G::NX, N1 = G::N1, PQ = P * Q;
  __shared__ double lds[G::NTAB + G::FPW * G::NF];
  const double *sB = lds, *sD = lds + Q * P, *sW = lds + 2 * Q * P;
  const FaceLane L = face_lane<G>(a.nface);
  const int t = L.t;
  const bool live = L.live;
  double *sx = lds + G::NTAB + (live ? L.fl : 0) * G::NF, *sdu = sx + NX, *sf = sdu + NX, *t1 = sf + NX, *tf = t1 + 4 * N1, *sv = tf + N1,
         *sr = sv + G::NV;
  const int kind = a.kind;
  const bool tang = kind == SURF_PRESSURE_FIELD_TANGENT || kind == SURF_HYDRO_TANGENT;
  const bool hydro = kind == SURF_HYDRO || kind == SURF_HYDRO_TANGENT;
  const bool cur = kind != SURF_TRACTION_FIELD && a.u != nullptr;
  const int nfc = hydro ? 0 : kind == SURF_TRACTION_FIELD ? 3 : 1;       // components of the extra field
  face_tables<P, Q>(tab, lds);
  // the node records: x = X (+ u); du with its flagged components as zeros; the field as it is
  if (live && t < P2) {
    const uint32_t off = a.offsets[(size_t)L.face * P2 + t];
    double x[3], w[3], d[3], f[3] = {0., 0., 0.};
    face_record<false>(a.X, off, x);
    if (cur) face_record<false>(a.u, off, w);
    if (tang) face_record<true>(a.du, off, d);
    if (nfc == 3) face_record<false>(a.field, off, f);
    else if (nfc == 1) f[0] = a.field[(off & OFF_MASK) / 3];
    if (cur) {
#pragma unroll
      for (int c = 0; c < 3; c++) x[c] += w[c];
    }
    face_put<P2>(sx, t, x);
    if (tang) face_put<P2>(sdu, t, d);
    if (nfc == 3) face_put<P2>(sf, t, f);
    else if (nfc == 1) sf[t] = f[0];
  }
  __syncthreads();
  // xi: per field (x; du) B and D of every line as in k_surface, t1[2 f] = B, t1[2 f + 1] = D; of the extra field B alone, tf[c][j][a]
  if (live) {
    const int nout = (tang ? 2 : 1) * N1;
    for (int o = t; o < nout; o += Q2) {
      const int f = o / N1, rem = o % N1, aa = rem % Q, line = rem / Q;
      const double *src = (f ? sdu : sx) + line * P;
      face_dot2<P, 1>(sB + aa * P, src, sD + aa * P, src, t1[(2 * f) * N1 + rem], t1[(2 * f + 1) * N1 + rem]);
    }
    for (int o = t; o < nfc * PQ; o += Q2) {
      const int aa = o % Q, line = o / Q;
      tf[o] = face_dot<P, 1>(sB + aa * P, sf + line * P);
    }
  }
  __syncthreads();
  // eta, the point work and the weight: a lane per point
  if (live) {
    const int aa = t % Q, bb = t / Q;
    const double *B = sB + bb * P, *D = sD + bb * P;
    double xa[3], xb[3], da[3] = {0., 0., 0.}, db[3] = {0., 0., 0.};      // d / d xi, d / d eta
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const double *vb = t1 + c * PQ + aa, *vd = vb + N1;
      face_dot2<P, Q>(B, vd, D, vb, xa[c], xb[c]);
    }
    if (tang) {
#pragma unroll
      for (int c = 0; c < 3; c++) {
        const double *vb = t1 + 2 * N1 + c * PQ + aa, *vd = vb + N1;
        face_dot2<P, Q>(B, vd, D, vb, da[c], db[c]);
      }
    }
    double n[3], m[3] = {0., 0., 0.};                                     // x_xi x x_eta; du_xi x x_eta + x_xi x du_eta
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const int c1 = (c + 1) % 3, c2 = (c + 2) % 3;
      n[c] = xa[c1] * xb[c2] - xa[c2] * xb[c1];
      if (tang) m[c] = (da[c1] * xb[c2] - da[c2] * xb[c1]) + (xa[c1] * db[c2] - xa[c2] * db[c1]);
    }
    const double w = a.coef[0] * (sW[aa] * sW[bb]);
    double v[3];
    if (kind == SURF_TRACTION_FIELD) {
      const double jw = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]) * w;
#pragma unroll
      for (int c = 0; c < 3; c++) v[c] = jw * face_dot<P, Q>(B, tf + c * PQ + aa);
    } else if (!hydro) {
      const double pw = face_dot<P, Q>(B, tf + aa) * w;
#pragma unroll
      for (int c = 0; c < 3; c++) v[c] = pw * (tang ? m[c] : n[c]);
    } else {
      double ex = 0.;                                                     // e . x_h: the B results of the xi pass are in t1
#pragma unroll
      for (int c = 0; c < 3; c++) ex += a.up[c] * face_dot<P, Q>(B, t1 + c * PQ + aa);
      const double d = a.level - ex, dw = (d > 0. ? d : 0.) * w;
      if (tang) {
        double er = 0.;                                                   // e . du_h
#pragma unroll
        for (int c = 0; c < 3; c++) er += a.up[c] * face_dot<P, Q>(B, t1 + 2 * N1 + c * PQ + aa);
        const double hw = d > 0. ? er * w : 0.;
#pragma unroll
        for (int c = 0; c < 3; c++) v[c] = dw * m[c] - hw * n[c];
      } else {
#pragma unroll
        for (int c = 0; c < 3; c++) v[c] = dw * n[c];
      }
    }
#pragma unroll
    for (int c = 0; c < 3; c++) sv[c * Q2 + t] = v[c];
  }
  __syncthreads();
  face_to_nodes<P, Q>(sB, sv, sr, a.evec, L.face, t, live);
}

// FIELD false: the three kinds of one coefficient per launch, below; true: the five kinds that vary over the faces.
template <int P, int Q, bool FIELD = false>
__global__ __launch_bounds__(64) void k_surface(const BasisTables tab, const std::conditional_t<FIELD, SurfaceFieldArgs, SurfaceArgs> a) {
  if constexpr (FIELD) {
    surface_field_face<P, Q>(tab, a);
  } else {
    using G = SurfGeom<P, Q>;
    constexpr int P2 = G::P2, Q2 = G::Q2, NX = G::NX, N1 = G::N1;
    __shared__ double lds[G::NTAB + G::FPW * G::NF];
    const double *sB = lds, *sD = lds + Q * P, *sW = lds + 2 * Q * P;
    const FaceLane L = face_lane<G>(a.nface);
    const int t = L.t;
    const bool live = L.live;
    double *sx = lds + G::NTAB + (live ? L.fl : 0) * G::NF, *sdu = sx + NX, *t1 = sdu + NX, *sv = t1 + 4 * N1, *sr = sv + G::NV;
    const int kind = a.kind;
    const bool tang = kind == SURF_TANGENT, cur = kind != SURF_TRACTION && a.u != nullptr;
    face_tables<P, Q>(tab, lds);
    // the node records: x = X (+ u); du with its flagged components as zeros
    if (live && t < P2) {
      const uint32_t off = a.offsets[(size_t)L.face * P2 + t];
      double x[3], w[3], d[3];
      face_record<false>(a.X, off, x);
      if (cur) {
        face_record<false>(a.u, off, w);
#pragma unroll
        for (int c = 0; c < 3; c++) x[c] += w[c];
      }
      if (tang) face_record<true>(a.du, off, d);
      face_put<P2>(sx, t, x);
      if (tang) face_put<P2>(sdu, t, d);
    }
    __syncthreads();
    // xi: per field (x; du) the value and the derivative of every line at the Q points: t1[2 f] = B, t1[2 f + 1] = D
    if (live) {
      const int nout = (tang ? 2 : 1) * N1;
      for (int o = t; o < nout; o += Q2) {
        const int f = o / N1, rem = o % N1, aa = rem % Q, line = rem / Q;
        const double *src = (f ? sdu : sx) + line * P;
        face_dot2<P, 1>(sB + aa * P, src, sD + aa * P, src, t1[(2 * f) * N1 + rem], t1[(2 * f + 1) * N1 + rem]);
      }
    }
    __syncthreads();
    // eta, the cross product(s) and the weight: a lane per point
    if (live) {
      const int aa = t % Q, bb = t / Q;
      const double *B = sB + bb * P, *D = sD + bb * P;
      double xa[3], xb[3], da[3] = {0., 0., 0.}, db[3] = {0., 0., 0.};      // d / d xi, d / d eta
#pragma unroll
      for (int c = 0; c < 3; c++) {
        const double *vb = t1 + c * P * Q + aa, *vd = vb + N1;
        face_dot2<P, Q>(B, vd, D, vb, xa[c], xb[c]);
      }
      if (tang) {
#pragma unroll
        for (int c = 0; c < 3; c++) {
          const double *vb = t1 + 2 * N1 + c * P * Q + aa, *vd = vb + N1;
          face_dot2<P, Q>(B, vd, D, vb, da[c], db[c]);
        }
      }
      const double w = sW[aa] * sW[bb];
      double v[3];
      if (tang) {
#pragma unroll
        for (int c = 0; c < 3; c++) {
          const int c1 = (c + 1) % 3, c2 = (c + 2) % 3;
          v[c] = a.coef[0] * w * ((da[c1] * xb[c2] - da[c2] * xb[c1]) + (xa[c1] * db[c2] - xa[c2] * db[c1]));
        }
      } else {
        double n[3];
#pragma unroll
        for (int c = 0; c < 3; c++) {
          const int c1 = (c + 1) % 3, c2 = (c + 2) % 3;
          n[c] = xa[c1] * xb[c2] - xa[c2] * xb[c1];
        }
        if (kind == SURF_TRACTION) {
          const double jw = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]) * w;
#pragma unroll
          for (int c = 0; c < 3; c++) v[c] = a.coef[c] * jw;
        } else {
#pragma unroll
          for (int c = 0; c < 3; c++) v[c] = a.coef[0] * w * n[c];
        }
      }
#pragma unroll
      for (int c = 0; c < 3; c++) sv[c * Q2 + t] = v[c];
    }
    __syncthreads();
    face_to_nodes<P, Q>(sB, sv, sr, a.evec, L.face, t, live);
  }
}

// A lane per row of the faces' transpose map: the row's contributors summed in face order (node_sum3: the sum k_assemble forms), then one
// read-modify-write of the row's entries of y.  Flagged components are skipped; a row with all three flagged reads nothing.
__global__ void k_surface_sum(const uint32_t *rowptr, const uint32_t *cols, const uint32_t *node_off, const unsigned char *flags,
                              const double *evec, double *y, int nrows) {
  for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < nrows; r += gridDim.x * blockDim.x) {
    const uint32_t fl = flags ? flags[r] : 0u;
    if ((fl & 7u) == 7u) continue;
    double a0 = 0., a1 = 0., a2 = 0.;
    node_sum3(rowptr, cols, evec, r, a0, a1, a2);
    double *p = y + (node_off[r] & OFF_MASK);
    if (!(fl & 1u)) p[0] += a0;
    if (!(fl & 2u)) p[1] += a1;
    if (!(fl & 4u)) p[2] += a2;
  }
}

// P = 2 .. 8, Q = P .. min(P + 2, 8): the fine level's Q = P + qextra, qextra <= 2
#define CPS_SURFACE_PQ(X)                                                                                       \
  X(2, 2) X(2, 3) X(2, 4) X(3, 3) X(3, 4) X(3, 5) X(4, 4) X(4, 5) X(4, 6) X(5, 5) X(5, 6) X(5, 7) X(6, 6) X(6, 7) \
  X(6, 8) X(7, 7) X(7, 8) X(8, 8)

hipError_t launch_surface(int P, int Q, const BasisTables &t, const SurfaceArgs &a, hipStream_t s, const char **name) {
#define CPS_SF(Pv, Qv)                                                              \
  if (P == Pv && Q == Qv) {                                                         \
    *name = "surface<P=" #Pv ",Q=" #Qv ">";                                         \
    return launch_faces<SurfGeom<Pv, Qv>::FPW>(k_surface<Pv, Qv>, t, a, s);         \
  }
  CPS_SURFACE_PQ(CPS_SF)
#undef CPS_SF
  return hipErrorInvalidValue;
}
hipError_t launch_surface_field(int P, int Q, const BasisTables &t, const SurfaceFieldArgs &a, hipStream_t s, const char **name) {
#define CPS_SF(Pv, Qv)                                                                   \
  if (P == Pv && Q == Qv) {                                                              \
    *name = "surface_field<P=" #Pv ",Q=" #Qv ">";                                        \
    return launch_faces<SurfFieldGeom<Pv, Qv>::FPW>(k_surface<Pv, Qv, true>, t, a, s);   \
  }
  CPS_SURFACE_PQ(CPS_SF)
#undef CPS_SF
  return hipErrorInvalidValue;
}
bool surface_instantiated(int P, int Q) {
#define CPS_SF(Pv, Qv) if (P == Pv && Q == Qv) return true;
  CPS_SURFACE_PQ(CPS_SF)
#undef CPS_SF
  return false;
}

hipError_t launch_surface_sum(const NodeMap &m, const unsigned char *flags, const double *evec, double *y, hipStream_t s) {
  return launch_stream(k_surface_sum, (size_t)(m.nnodes > 0 ? m.nnodes : 0), s, m.rowptr + m.row0, m.cols, m.node_off + m.row0,
                       flags ? flags + m.row0 : nullptr, evec, y, m.nnodes);
}

}  // namespace cps
