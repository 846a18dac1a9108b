// kernel_face_pass.hpp -- the FACE passes that k_surface (kernels_surface.hip) and k_contact (kernels_contact.hip) share.
//
// A face has the P^2 face nodes of its element, xi fastest in its node list, and Q^2 Gauss points.  One wave64 per workgroup owns
// FPW = max(1, 64 / Q^2) faces, a face owns S = Q^2 lanes (Q >= P: a lane per point, and per node in the first and the last step); the
// 64 % S lanes left over, and the lanes of faces past nface, are not `live`: they touch no memory but take every barrier.  Per face in
// LDS: the gathered fields [c][j][i], the results of the xi pass [c][j][a], the values at the points [c][b][a] and the first transposed
// pass [c][b][i]; in front of the faces the 1-D tables B[a][i], D[a][i] and the weights.  The steps, a barrier between each two: the
// gather of the 24-byte node records, the xi pass, the eta sums with the kernel's own point work at a lane per point, and the two
// transposed passes back to the nodes with plain coalesced stores into the face E-vector [face][P^2][3].  Every sum runs in ascending
// index order.  No atomics, no scratch memory, no waiting on other waves.
#pragma once
#include "kernels_common.hpp"

namespace cps {

template <int P, int Q> struct FaceGeom {
  static_assert(Q >= P && Q <= MAXN1D && P >= 2, "a lane per point covers the nodes too");
  static constexpr int P2 = P * P, Q2 = Q * Q;
  static constexpr int S = Q2;                         // lanes of a face
  static constexpr int FPW = 64 / S < 1 ? 1 : 64 / S;  // faces of a wave
  static constexpr int NX = 3 * P2;                    // a gathered field         [c][j][i]
  static constexpr int N1 = 3 * P * Q;                 // one result of the xi pass [c][j][a]
  static constexpr int NV = 3 * Q2;                    // the values at the points  [c][b][a]
  static constexpr int NR = 3 * Q * P;                 // first transposed pass     [c][b][i]
  static constexpr int NTAB = 2 * Q * P + Q;           // B[a][i], D[a][i], weights
};

// this lane's face of the wave, its point (node) of the face, the face, and whether there is one
struct FaceLane { int fl, t, face; bool live; };
template <class G> CPS_DEV FaceLane face_lane(int nface) {
  const int lane = threadIdx.x, fl = lane / G::S, face = blockIdx.x * G::FPW + fl;
  return {fl, lane % G::S, face, fl < G::FPW && face < nface};         // (64 % S lanes of the wave own no face)
}

// the tables into LDS: sB = lds, sD = lds + Q P, sW = lds + 2 Q P
template <int P, int Q> CPS_DEV void face_tables(const BasisTables &tab, double *lds) {
  const int lane = threadIdx.x;
  for (int i = lane; i < Q * P; i += 64) { lds[i] = tab.interp[i]; lds[Q * P + i] = tab.grad[i]; }
  if (lane < Q) lds[2 * Q * P + lane] = tab.qw[lane];
}

// One field of a node's 24-byte record: v[c] = f[o + c] at the offset `off` (its flag bits on top); FLAGGED: flagged components read
// as zero.  Into registers, so that a kernel has the loads of all its fields in flight before the first of them goes to LDS ...
template <bool FLAGGED> CPS_DEV void face_record(const double *f, uint32_t off, double v[3]) {
  const uint32_t o = off & OFF_MASK, flg = off >> OFF_FLAG_SHIFT;
#pragma unroll
  for (int c = 0; c < 3; c++) v[c] = (FLAGGED && ((flg >> c) & 1u)) ? 0. : f[o + c];
}
// ... as node t of a gathered field dst[c][t]
template <int P2> CPS_DEV void face_put(double *dst, int t, const double v[3]) {
#pragma unroll
  for (int c = 0; c < 3; c++) dst[c * P2 + t] = v[c];
}

// sum_i T[i] v[i * STRIDE], i ascending: the line sums of the xi pass (STRIDE 1) and the eta sums at a point (STRIDE Q)
template <int N, int STRIDE> CPS_DEV double face_dot(const double *T, const double *v) {
  double s = 0.;
#pragma unroll
  for (int i = 0; i < N; i++) s += T[i] * v[i * STRIDE];
  return s;
}

// Two such sums in one loop, their terms alternating.  Same values as two face_dot calls, but the compiler schedules them differently:
// with separate sums k_surface<3,3>, <3,5> and <6,6> each lose a wave per SIMD (profiles/surface_load.txt).
template <int N, int STRIDE>
CPS_DEV void face_dot2(const double *T0, const double *v0, const double *T1, const double *v1, double &r0, double &r1) {
  double s0 = 0., s1 = 0.;
#pragma unroll
  for (int i = 0; i < N; i++) { s0 += T0[i] * v0[i * STRIDE]; s1 += T1[i] * v1[i * STRIDE]; }
  r0 = s0; r1 = s1;
}

// The values at the points sv[c][b][a] back to the nodes: sr[c][b][i] = sum_a B[a][i] sv[c][b][a], a barrier, then at a lane per node
// g[c] = sum_b B[b][j] sr[c][b][i] stored as the 24-byte record of node t of the face.  The caller's barrier stands in front.
template <int P, int Q> CPS_DEV void face_to_nodes(const double *sB, const double *sv, double *sr, double *evec, int face, int t, bool live) {
  if (live) {
    for (int o = t; o < 3 * Q * P; o += Q * Q) {
      const int i = o % P, cb = o / P;
      const double *src = sv + cb * Q;
      double r = 0.;
#pragma unroll
      for (int q = 0; q < Q; q++) r += sB[q * P + i] * src[q];
      sr[o] = r;
    }
  }
  __syncthreads();
  if (live && t < P * P) {
    const int i = t % P, j = t / P;
    double *out = evec + ((size_t)face * (P * P) + t) * 3;
#pragma unroll
    for (int c = 0; c < 3; c++) {
      double g = 0.;
#pragma unroll
      for (int b = 0; b < Q; b++) g += sB[b * P + j] * sr[(c * Q + b) * P + i];
      out[c] = g;
    }
  }
}

// ceil(nface / FPW) workgroups of one wave; nothing for nface <= 0
template <int FPW, class A> static inline hipError_t launch_faces(void (*k)(BasisTables, A), const BasisTables &t, const A &a, hipStream_t s) {
  if (a.nface <= 0) return hipSuccess;
  hipLaunchKernelGGL(k, dim3((a.nface + FPW - 1) / FPW), dim3(64), 0, s, t, a);
  return hipGetLastError();
}

}  // namespace cps
