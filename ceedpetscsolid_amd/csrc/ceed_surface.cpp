// ceed_surface.cpp -- surface loads on side sets (CeedXSurfaceLoad*): dead traction, follower pressure and its tangent on a list of
// element faces (kernels_surface.hip).  The faces' transpose map is index_maps.hpp's, their Dirichlet flags ride in the top bits of the
// face offsets like an operator's (flagged_offsets) and per row of the map (row_flag_bits); the sum is k_surface_sum's, in face order.
// The map and the row flags are made at the first apply (never while a graph is recorded), the flagged offsets when they are set.
#include "ceed_impl.hpp"
#include "index_maps.hpp"

using namespace cps;

struct CeedXSurfaceLoad_private {
  Ceed ceed = nullptr;
  int nface = 0, P = 0, Q = 0, lsize = 0;
  std::vector<int> h_offsets;               // [nface][P^2] component-0 L-offsets
  std::vector<unsigned char> h_mask;        // copy of the Dirichlet mask (empty: none)
  DevArray<uint32_t> d_offsets;             // the offsets with the flag bits of their nodes
  RowMap map;                               // transpose map of the faces: rows = the nodes on the loaded surface
  bool map_built = false;
  DevArray<unsigned char> d_row_flags;      // the mask per row of the map
  bool flags_built = false;
  BasisTables tables;                       // 1-D B, D and weights of (P nodes, Q Gauss points)
  std::string kernel_name;
};

extern "C" int CeedXSurfaceLoadDestroy(CeedXSurfaceLoad *sl) {
  if (!sl || !*sl) return 0;
  CeedXSurfaceLoad S = *sl;
  *sl = nullptr;
  Ceed c = S->ceed;
  delete S;            // (before the reference goes: its arrays retire into a Ceed that still exists)
  ceed_unref(c);
  return 0;
}

extern "C" int CeedXSurfaceLoadCreate(Ceed ceed, CeedInt nface, CeedInt P, CeedInt Q, const CeedInt *offsets, CeedInt lsize, CeedXSurfaceLoad *sl) {
  if (ceed->capturing) return ceed_error("CeedXSurfaceLoadCreate during graph capture");
  if (nface < 0) return ceed_error("CeedXSurfaceLoadCreate: nface = %d is negative", nface);
  if (!surface_instantiated(P, Q)) return ceed_error("no surface kernel for P=%d Q=%d (P = 2 .. 8, Q = P .. min(P + 2, 8))", P, Q);
  if (lsize < 0 || (size_t)lsize > (size_t)OFF_MASK) return ceed_error("CeedXSurfaceLoadCreate: L-size %d outside [0, 2^29)", lsize);
  if (nface > 0 && !offsets) return ceed_error("CeedXSurfaceLoadCreate: no offsets");
  if ((size_t)nface * P * P > (size_t)0x7FFFFFFF / 3) return ceed_error("CeedXSurfaceLoadCreate: %d faces are too many", nface);
  const size_t n = (size_t)nface * P * P;
  for (size_t i = 0; i < n; i++) {
    const long o = offsets[i];
    if (o < 0 || o + 2 >= (long)lsize) return ceed_error("CeedXSurfaceLoadCreate: offset %ld of face %zu lies past the L-size %d", o, i / ((size_t)P * P), lsize);
    if (o % 3) return ceed_error("CeedXSurfaceLoadCreate: offset %ld of face %zu is no multiple of 3 (component-0 offsets of interlaced nodes)", o, i / ((size_t)P * P));
  }
  CeedXSurfaceLoad S = new CeedXSurfaceLoad_private;
  S->ceed = ceed; ceed_ref(ceed);
  S->nface = nface; S->P = P; S->Q = Q; S->lsize = lsize;
  S->h_offsets.assign(offsets, offsets + n);
  auto fill = [&]() -> int {
    CeedBasis b = nullptr;
    CHK(CeedBasisCreateTensorH1Lagrange(ceed, 3, 3, P, Q, CEED_GAUSS, &b));
    memset(&S->tables, 0, sizeof S->tables);
    memcpy(S->tables.interp, b->interp1d.data(), sizeof(double) * b->interp1d.size());
    memcpy(S->tables.grad, b->grad1d.data(), sizeof(double) * b->grad1d.size());
    memcpy(S->tables.qw, b->qweight1d.data(), sizeof(double) * b->qweight1d.size());
    CHK(CeedBasisDestroy(&b));
    return S->d_offsets.upload(ceed, face_offsets(S->h_offsets, nullptr));
  };
  const int ierr = fill();
  if (ierr) { (void)CeedXSurfaceLoadDestroy(&S); return ierr; }
  *sl = S;
  return 0;
}

extern "C" int CeedXSurfaceLoadSetDirichletMask(CeedXSurfaceLoad S, CeedMemType mtype, const unsigned char *mask, CeedInt lsize) {
  Ceed c = S->ceed;
  if (c->capturing) return ceed_error("CeedXSurfaceLoadSetDirichletMask during graph capture");
  if (mask && mtype != CEED_MEM_HOST) return ceed_error("pass the Dirichlet mask in host memory (it is folded into the offsets once)");
  if (mask && lsize < S->lsize) return ceed_error("Dirichlet mask shorter than the L-vector");
  if (mask) S->h_mask.assign(mask, mask + S->lsize); else S->h_mask.clear();
  S->d_row_flags.release(); S->flags_built = false;
  return S->d_offsets.upload(c, face_offsets(S->h_offsets, mask ? S->h_mask.data() : nullptr));
}

// the lazily made arrays: the faces' transpose map and the mask in its row order
static int surface_prepare(CeedXSurfaceLoad S) {
  Ceed c = S->ceed;
  if (S->map_built && S->flags_built) return 0;
  if (c->capturing) return ceed_error("first apply of a surface load (or the first after its mask was set) during graph capture: apply once before recording");
  if (!S->map_built) {
    TransposeMap T = transpose_map(S->h_offsets, S->lsize, S->P * S->P, 3, nullptr, 0);
    RowMap &M = S->map;
    M.nrows = (int)T.node_off.size();
    CHK(M.d_rowptr.upload(c, T.rowptr)); CHK(M.d_cols.upload(c, T.cols)); CHK(M.d_node_off.upload(c, T.node_off));
    M.h_node_off.swap(T.node_off);
    S->map_built = true;
  }
  if (!S->flags_built) {
    if (!S->h_mask.empty()) CHK(S->d_row_flags.upload(c, row_flag_bits(S->map.h_node_off, S->h_mask.data(), 3, 1)));
    S->flags_built = true;
  }
  return 0;
}

static int surface_apply(CeedXSurfaceLoad S, const char *who, int kind, const double coef[3], CeedVector X, CeedVector u, CeedVector du, CeedVector y) {
  Ceed c = S->ceed;
  if (!X || !y) return ceed_error("%s: no coordinate / output vector", who);
  if (X->length < S->lsize || y->length < S->lsize || (u && u->length < S->lsize) || (du && du->length < S->lsize))
    return ceed_error("%s: vector shorter than the L-size %d", who, S->lsize);
  if (y == X || y == u || y == du) return ceed_error("%s: the output vector aliases an input", who);
  if (S->nface == 0) return 0;
  CHK(surface_prepare(S));
  SurfaceArgs a{};
  double *pX = nullptr, *pu = nullptr, *pdu = nullptr, *py = nullptr;
  CHK(vec_dev(X, false, &pX));
  if (u) CHK(vec_dev(u, false, &pu));
  if (du) CHK(vec_dev(du, false, &pdu));
  CHK(vec_dev(y, true, &py));
  CHK(ceed_need_evec(c, (size_t)S->nface * S->P * S->P * 3));
  a.offsets = S->d_offsets.get(); a.X = pX; a.u = pu; a.du = pdu; a.evec = c->evec.get();
  a.nface = S->nface; a.kind = kind;
  for (int i = 0; i < 3; i++) a.coef[i] = coef[i];
  const char *kname = "";
  hipError_t e = launch_surface(S->P, S->Q, S->tables, a, c->stream, &kname);
  if (e == hipErrorInvalidValue && !*kname) return ceed_error("no surface kernel for P=%d Q=%d", S->P, S->Q);
  HIPCHK(e);
  S->kernel_name = kname;
  HIPCHK(launch_surface_sum(S->map.view(), S->d_row_flags.get(), a.evec, py, c->stream));
  return 0;
}

extern "C" int CeedXSurfaceLoadApplyAdd(CeedXSurfaceLoad S, int kind, const CeedScalar coef[3], CeedScalar scale, CeedVector X, CeedVector u, CeedVector y) {
  if (kind != CEED_X_SURFACE_TRACTION && kind != CEED_X_SURFACE_PRESSURE) return ceed_error("CeedXSurfaceLoadApplyAdd: kind %d is neither traction nor pressure", kind);
  if (u == CEED_VECTOR_NONE) u = nullptr;
  const bool tr = kind == CEED_X_SURFACE_TRACTION;
  const double cf[3] = {scale * coef[0], tr ? scale * coef[1] : 0., tr ? scale * coef[2] : 0.};
  return surface_apply(S, "CeedXSurfaceLoadApplyAdd", tr ? SURF_TRACTION : SURF_PRESSURE, cf, X, tr ? nullptr : u, nullptr, y);
}

extern "C" int CeedXSurfaceLoadApplyTangentAdd(CeedXSurfaceLoad S, CeedScalar p, CeedScalar scale, CeedVector X, CeedVector u, CeedVector du, CeedVector y) {
  if (!du) return ceed_error("CeedXSurfaceLoadApplyTangentAdd: no variation vector");
  if (u == CEED_VECTOR_NONE) u = nullptr;
  const double cf[3] = {scale * p, 0., 0.};
  return surface_apply(S, "CeedXSurfaceLoadApplyTangentAdd", SURF_TANGENT, cf, X, u, du, y);
}

extern "C" int CeedXSurfaceLoadGetKernelName(CeedXSurfaceLoad S, const char **name) { *name = S->kernel_name.c_str(); return 0; }
