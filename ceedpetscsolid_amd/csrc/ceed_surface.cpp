// ceed_surface.cpp -- the face set every term on a side set keeps (face_set.hpp), and the surface loads (CeedXSurfaceLoad*): dead
// traction, follower pressure and its tangent on a list of element faces (kernels_surface.hip), and the loads that vary over the faces
// (include/ceed_surface_field.h): a nodal traction or pressure field, a hydrostatic pressure, and the two followers' tangents.
#include <cmath>
#include <ceed_surface_field.h>
#include "face_set.hpp"
#include "index_maps.hpp"

using namespace cps;

int face_set_create(FaceSet &F, const char *who, Ceed ceed, CeedInt nface, CeedInt P, CeedInt Q, const CeedInt *offsets, CeedInt lsize,
                    bool (*instantiated)(int, int), const char *term, const char *pairs) {
  F.ceed = ceed; ceed_ref(ceed);
  if (ceed->capturing) return ceed_error("%s during graph capture", who);
  if (nface < 0) return ceed_error("%s: nface = %d is negative", who, nface);
  if (!instantiated(P, Q)) return ceed_error("no %s kernel for P=%d Q=%d (%s)", term, P, Q, pairs);
  if (lsize < 0 || (size_t)lsize > (size_t)OFF_MASK) return ceed_error("%s: L-size %d outside [0, 2^29)", who, lsize);
  if (nface > 0 && !offsets) return ceed_error("%s: no offsets", who);
  const FaceOffsetCheck k = check_face_offsets(offsets, (size_t)nface, P * P, lsize);
  if (k.fault == FACE_OFFSETS_TOO_MANY) return ceed_error("%s: %d faces are too many", who, nface);
  if (k.fault == FACE_OFFSET_PAST_LSIZE) return ceed_error("%s: offset %ld of face %zu lies past the L-size %d", who, k.offset, k.face, lsize);
  if (k.fault == FACE_OFFSET_NOT_NODE)
    return ceed_error("%s: offset %ld of face %zu is no multiple of 3 (component-0 offsets of interlaced nodes)", who, k.offset, k.face);
  F.nface = nface; F.P = P; F.Q = Q; F.lsize = lsize;
  F.h_offsets.assign(offsets, offsets + (size_t)nface * P * P);
  CeedBasis b = nullptr;
  CHK(CeedBasisCreateTensorH1Lagrange(ceed, 3, 3, P, Q, CEED_GAUSS, &b));
  fill_tables(F.tables, b);
  CHK(CeedBasisDestroy(&b));
  return F.d_offsets.upload(ceed, face_offsets(F.h_offsets, nullptr));
}

int face_set_mask(FaceSet &F, const char *who, CeedMemType mtype, const unsigned char *mask, CeedInt lsize) {
  if (F.ceed->capturing) return ceed_error("%s during graph capture", who);
  if (mask && mtype != CEED_MEM_HOST) return ceed_error("pass the Dirichlet mask in host memory (it is folded into the offsets once)");
  if (mask && lsize < F.lsize) return ceed_error("Dirichlet mask shorter than the L-vector");
  if (mask) F.h_mask.assign(mask, mask + F.lsize); else F.h_mask.clear();
  F.d_row_flags.release(); F.flags_built = false;
  return F.d_offsets.upload(F.ceed, face_offsets(F.h_offsets, mask ? F.h_mask.data() : nullptr));
}

int face_set_prepare(FaceSet &F, const char *what) {
  Ceed c = F.ceed;
  if (F.map_built && F.flags_built) return 0;
  if (c->capturing) return ceed_error("first apply of %s (or the first after its mask was set) during graph capture: apply once before recording", what);
  if (!F.map_built) {
    TransposeMap T = transpose_map(F.h_offsets, F.lsize, F.P * F.P, 3, nullptr, 0);
    RowMap &M = F.map;
    M.nrows = (int)T.node_off.size();
    CHK(M.d_rowptr.upload(c, T.rowptr)); CHK(M.d_cols.upload(c, T.cols)); CHK(M.d_node_off.upload(c, T.node_off));
    M.h_node_off.swap(T.node_off);
    F.map_built = true;
  }
  if (!F.flags_built) {
    if (!F.h_mask.empty()) CHK(F.d_row_flags.upload(c, row_flag_bits(F.map.h_node_off, F.h_mask.data(), 3, 1)));
    F.flags_built = true;
  }
  return 0;
}

struct CeedXSurfaceLoad_private { FaceSet fs; };

extern "C" int CeedXSurfaceLoadDestroy(CeedXSurfaceLoad *sl) { return face_handle_destroy(sl); }

extern "C" int CeedXSurfaceLoadCreate(Ceed ceed, CeedInt nface, CeedInt P, CeedInt Q, const CeedInt *offsets, CeedInt lsize, CeedXSurfaceLoad *sl) {
  CeedXSurfaceLoad S = new CeedXSurfaceLoad_private;
  const int ierr = face_set_create(S->fs, "CeedXSurfaceLoadCreate", ceed, nface, P, Q, offsets, lsize, surface_instantiated, "surface",
                                   "P = 2 .. 8, Q = P .. min(P + 2, 8)");
  if (ierr) { (void)CeedXSurfaceLoadDestroy(&S); return ierr; }
  *sl = S;
  return 0;
}

extern "C" int CeedXSurfaceLoadSetDirichletMask(CeedXSurfaceLoad S, CeedMemType mtype, const unsigned char *mask, CeedInt lsize) {
  return face_set_mask(S->fs, "CeedXSurfaceLoadSetDirichletMask", mtype, mask, lsize);
}

// What the kinds that vary over the faces pass besides: the nodal field with the length it must have (or none), level and unit up.
struct SurfaceField { CeedVector field = nullptr; int length = 0; double level = 0., up[3] = {0., 0., 0.}; };

static int surface_apply(FaceSet &F, const char *who, int kind, const double coef[3], CeedVector X, CeedVector u, CeedVector du, CeedVector y,
                         const SurfaceField *fld = nullptr) {
  if (!X || !y) return ceed_error("%s: no coordinate / output vector", who);
  if (X->length < F.lsize || y->length < F.lsize || (u && u->length < F.lsize) || (du && du->length < F.lsize))
    return ceed_error("%s: vector shorter than the L-size %d", who, F.lsize);
  if (y == X || y == u || y == du || (fld && y == fld->field)) return ceed_error("%s: the output vector aliases an input", who);
  if (fld && fld->field && fld->field->length != fld->length)
    return ceed_error("%s: the field holds %d values where %d are expected (L-size %d)", who, (int)fld->field->length, fld->length, F.lsize);
  if (F.nface == 0) return 0;
  CHK(face_set_prepare(F, "a surface load"));
  SurfaceFieldArgs a{};
  double *pX = nullptr, *pu = nullptr, *pdu = nullptr, *py = nullptr, *pf = nullptr;
  CHK(vec_dev(X, false, &pX));
  if (u) CHK(vec_dev(u, false, &pu));
  if (du) CHK(vec_dev(du, false, &pdu));
  if (fld && fld->field) CHK(vec_dev(fld->field, false, &pf));
  CHK(vec_dev(y, true, &py));
  a.offsets = F.d_offsets.get(); a.X = pX; a.u = pu; a.du = pdu;
  a.nface = F.nface; a.kind = kind;
  for (int i = 0; i < 3; i++) a.coef[i] = coef[i];
  if (fld) {
    a.field = pf; a.level = fld->level;
    for (int i = 0; i < 3; i++) a.up[i] = fld->up[i];
  }
  return face_set_apply(F, "surface", py, [&](double *evec, const char **name) {
    a.evec = evec;
    return fld ? launch_surface_field(F.P, F.Q, F.tables, a, F.ceed->stream, name) : launch_surface(F.P, F.Q, F.tables, a, F.ceed->stream, name);
  });
}

extern "C" int CeedXSurfaceLoadApplyAdd(CeedXSurfaceLoad S, int kind, const CeedScalar coef[3], CeedScalar scale, CeedVector X, CeedVector u, CeedVector y) {
  if (kind != CEED_X_SURFACE_TRACTION && kind != CEED_X_SURFACE_PRESSURE) return ceed_error("CeedXSurfaceLoadApplyAdd: kind %d is neither traction nor pressure", kind);
  if (u == CEED_VECTOR_NONE) u = nullptr;
  const bool tr = kind == CEED_X_SURFACE_TRACTION;
  const double cf[3] = {scale * coef[0], tr ? scale * coef[1] : 0., tr ? scale * coef[2] : 0.};
  return surface_apply(S->fs, "CeedXSurfaceLoadApplyAdd", tr ? SURF_TRACTION : SURF_PRESSURE, cf, X, tr ? nullptr : u, nullptr, y);
}

extern "C" int CeedXSurfaceLoadApplyTangentAdd(CeedXSurfaceLoad S, CeedScalar p, CeedScalar scale, CeedVector X, CeedVector u, CeedVector du, CeedVector y) {
  if (!du) return ceed_error("CeedXSurfaceLoadApplyTangentAdd: no variation vector");
  if (u == CEED_VECTOR_NONE) u = nullptr;
  const double cf[3] = {scale * p, 0., 0.};
  return surface_apply(S->fs, "CeedXSurfaceLoadApplyTangentAdd", SURF_TANGENT, cf, X, u, du, y);
}

extern "C" int CeedXSurfaceLoadGetKernelName(CeedXSurfaceLoad S, const char **name) { *name = S->fs.kernel_name.c_str(); return 0; }

// ---- loads that vary over the faces (include/ceed_surface_field.h) ------------------------------------------------------------------
static int field_of(const char *who, const FaceSet &F, int kind, CeedVector field, SurfaceField &fld) {
  if (!field || field == CEED_VECTOR_NONE) return ceed_error("%s: no field vector", who);
  fld.field = field;
  fld.length = kind == CEED_X_SURFACE_TRACTION ? F.lsize : F.lsize / 3;
  return 0;
}

static int hydrostatic_of(const char *who, double gamma, double level, const double up[3], SurfaceField &fld) {
  if (!std::isfinite(gamma) || !std::isfinite(level)) return ceed_error("%s: gamma = %g and level = %g must be finite", who, gamma, level);
  if (!up) return ceed_error("%s: no up vector", who);
  const double n2 = up[0] * up[0] + up[1] * up[1] + up[2] * up[2];
  if (!std::isfinite(n2) || !(n2 > 0.)) return ceed_error("%s: up = (%g, %g, %g) is not a finite, non-zero vector", who, up[0], up[1], up[2]);
  const double n = std::sqrt(n2);
  for (int i = 0; i < 3; i++) fld.up[i] = up[i] / n;
  fld.level = level;
  return 0;
}

extern "C" int CeedXSurfaceLoadApplyFieldAdd(CeedXSurfaceLoad S, int kind, CeedVector field, CeedScalar scale, CeedVector X, CeedVector u, CeedVector y) {
  const char *who = "CeedXSurfaceLoadApplyFieldAdd";
  if (kind != CEED_X_SURFACE_TRACTION && kind != CEED_X_SURFACE_PRESSURE) return ceed_error("%s: kind %d is neither traction nor pressure", who, kind);
  if (u == CEED_VECTOR_NONE) u = nullptr;
  const bool tr = kind == CEED_X_SURFACE_TRACTION;
  SurfaceField fld;
  CHK(field_of(who, S->fs, kind, field, fld));
  const double cf[3] = {scale, 0., 0.};
  return surface_apply(S->fs, who, tr ? SURF_TRACTION_FIELD : SURF_PRESSURE_FIELD, cf, X, tr ? nullptr : u, nullptr, y, &fld);
}

extern "C" int CeedXSurfaceLoadApplyFieldTangentAdd(CeedXSurfaceLoad S, CeedVector field, CeedScalar scale, CeedVector X, CeedVector u, CeedVector du, CeedVector y) {
  const char *who = "CeedXSurfaceLoadApplyFieldTangentAdd";
  if (!du) return ceed_error("%s: no variation vector", who);
  if (u == CEED_VECTOR_NONE) u = nullptr;
  SurfaceField fld;
  CHK(field_of(who, S->fs, CEED_X_SURFACE_PRESSURE, field, fld));
  const double cf[3] = {scale, 0., 0.};
  return surface_apply(S->fs, who, SURF_PRESSURE_FIELD_TANGENT, cf, X, u, du, y, &fld);
}

extern "C" int CeedXSurfaceLoadApplyHydrostaticAdd(CeedXSurfaceLoad S, CeedScalar gamma, CeedScalar level, const CeedScalar up[3], CeedScalar scale,
                                                   CeedVector X, CeedVector u, CeedVector y) {
  const char *who = "CeedXSurfaceLoadApplyHydrostaticAdd";
  if (u == CEED_VECTOR_NONE) u = nullptr;
  SurfaceField fld;
  CHK(hydrostatic_of(who, gamma, level, up, fld));
  const double cf[3] = {scale * gamma, 0., 0.};
  return surface_apply(S->fs, who, SURF_HYDRO, cf, X, u, nullptr, y, &fld);
}

extern "C" int CeedXSurfaceLoadApplyHydrostaticTangentAdd(CeedXSurfaceLoad S, CeedScalar gamma, CeedScalar level, const CeedScalar up[3], CeedScalar scale,
                                                          CeedVector X, CeedVector u, CeedVector du, CeedVector y) {
  const char *who = "CeedXSurfaceLoadApplyHydrostaticTangentAdd";
  if (!du) return ceed_error("%s: no variation vector", who);
  if (u == CEED_VECTOR_NONE) u = nullptr;
  SurfaceField fld;
  CHK(hydrostatic_of(who, gamma, level, up, fld));
  const double cf[3] = {scale * gamma, 0., 0.};
  return surface_apply(S->fs, who, SURF_HYDRO_TANGENT, cf, X, u, du, y, &fld);
}
