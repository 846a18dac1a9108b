// ceed_contact.cpp -- frictionless penalty contact of side sets with a rigid plane or sphere (CeedXContact*, include/ceed_contact.h):
// residual, tangent and diagonal on a list of element faces (kernels_contact.hip) over a face set (face_set.hpp).  The contact state
// [nface][7][Q^2] is the caller's vector: the residual writes it, the tangent and the diagonal of any p-level read it.
#include "face_set.hpp"
#include <ceed_contact.h>

using namespace cps;

struct CeedXContact_private {
  FaceSet fs;
  BasisTables tables_sq;                    // fs.tables with B entry-wise squared (diagonal)
  bool has_obstacle = false;
  int kind = 0;
  double par[8] = {0., 0., 0., 0., 0., 0., 0., 0.}, penalty = 0.;
  size_t state_len() const { return (size_t)fs.nface * CONTACT_NSTATE * fs.Q * fs.Q; }
};

extern "C" int CeedXContactDestroy(CeedXContact *ct) { return face_handle_destroy(ct); }

extern "C" int CeedXContactCreate(Ceed ceed, CeedInt nface, CeedInt P, CeedInt Q, const CeedInt *offsets, CeedInt lsize, CeedXContact *ct) {
  if (nface > 0 && contact_instantiated(P, Q) && (size_t)nface * Q * Q > (size_t)0x7FFFFFFF / CONTACT_NSTATE)    // the state is indexed in 32 bits
    return ceed_error("CeedXContactCreate: %d faces are too many", nface);
  CeedXContact S = new CeedXContact_private;
  const int ierr = face_set_create(S->fs, "CeedXContactCreate", ceed, nface, P, Q, offsets, lsize, contact_instantiated, "contact", "P = 2 .. 8, Q = P .. 8");
  if (ierr) { (void)CeedXContactDestroy(&S); return ierr; }
  memset(&S->tables_sq, 0, sizeof S->tables_sq);
  for (int i = 0; i < Q * P; i++) S->tables_sq.interp[i] = S->fs.tables.interp[i] * S->fs.tables.interp[i];
  *ct = S;
  return 0;
}

extern "C" int CeedXContactSetDirichletMask(CeedXContact S, CeedMemType mtype, const unsigned char *mask, CeedInt lsize) {
  return face_set_mask(S->fs, "CeedXContactSetDirichletMask", mtype, mask, lsize);
}

extern "C" int CeedXContactSetObstacle(CeedXContact S, int kind, const CeedScalar params[8], CeedScalar penalty) {
  if (kind != CEED_X_CONTACT_PLANE && kind != CEED_X_CONTACT_SPHERE) return ceed_error("CeedXContactSetObstacle: kind %d is neither plane nor sphere", kind);
  if (!params) return ceed_error("CeedXContactSetObstacle: no parameters");
  if (!(penalty > 0.) || !std::isfinite(penalty)) return ceed_error("CeedXContactSetObstacle: the penalty %g is not positive", penalty);
  for (int i = 0; i < (kind == CEED_X_CONTACT_PLANE ? 6 : 5); i++)
    if (!std::isfinite(params[i])) return ceed_error("CeedXContactSetObstacle: parameter %d is not finite", i);
  if (kind == CEED_X_CONTACT_PLANE) {
    const double len = std::sqrt(params[3] * params[3] + params[4] * params[4] + params[5] * params[5]);
    if (!(std::fabs(len - 1.) <= 1e-12)) return ceed_error("CeedXContactSetObstacle: the plane normal has length %g, not 1", len);
  } else {
    if (!(params[3] > 0.)) return ceed_error("CeedXContactSetObstacle: the sphere radius %g is not positive", params[3]);
    if (params[4] != 1. && params[4] != -1.) return ceed_error("CeedXContactSetObstacle: the sphere side s = %g is neither +1 (ball) nor -1 (cavity)", params[4]);
  }
  S->kind = kind == CEED_X_CONTACT_PLANE ? CONTACT_PLANE : CONTACT_SPHERE;
  for (int i = 0; i < 8; i++) S->par[i] = params[i];
  S->penalty = penalty;
  S->has_obstacle = true;
  return 0;
}

// The checks every apply makes before anything is launched, then the launch and the node sum.  in0, in1: the L-vector inputs (either may
// be null); `state` is written by the residual and read otherwise; `y` is the L-vector the face results are added to.
static int contact_apply(CeedXContact S, const char *who, int mode, double scale, CeedVector in0, CeedVector in1, CeedVector state, CeedVector y) {
  FaceSet &F = S->fs;
  if (!y || !state) return ceed_error("%s: no output / state vector", who);
  if (y->length < F.lsize || (in0 && in0->length < F.lsize) || (in1 && in1->length < F.lsize))
    return ceed_error("%s: vector shorter than the L-size %d", who, F.lsize);
  if ((size_t)state->length < S->state_len())
    return ceed_error("%s: state vector shorter than %zu = nface x 7 x Q^2 (nface = %d, Q = %d)", who, S->state_len(), F.nface, F.Q);
  if (y == in0 || y == in1 || y == state || (mode == CONTACT_RESIDUAL && (state == in0 || state == in1)))
    return ceed_error("%s: the output vector aliases an input", who);
  if (F.nface == 0) return 0;
  CHK(face_set_prepare(F, "a contact surface"));
  ContactArgs a{};
  double *p0 = nullptr, *p1 = nullptr, *ps = nullptr, *py = nullptr;
  if (in0) CHK(vec_dev(in0, false, &p0));
  if (in1) CHK(vec_dev(in1, false, &p1));
  CHK(vec_dev(state, mode == CONTACT_RESIDUAL, &ps));
  CHK(vec_dev(y, true, &py));
  a.offsets = F.d_offsets.get(); a.state = ps;
  if (mode == CONTACT_RESIDUAL) { a.X = p0; a.u = p1; } else { a.du = p0; }
  a.nface = F.nface; a.kind = S->kind; a.penalty = S->penalty; a.scale = scale;
  for (int i = 0; i < 8; i++) a.par[i] = S->par[i];
  return face_set_apply(F, "contact", py, [&](double *evec, const char **name) {
    a.evec = evec;
    return launch_contact(F.P, F.Q, mode, mode == CONTACT_DIAGONAL ? S->tables_sq : F.tables, a, F.ceed->stream, name);
  });
}

extern "C" int CeedXContactApplyResidualAdd(CeedXContact S, CeedScalar scale, CeedVector X, CeedVector u, CeedVector y, CeedVector state) {
  if (!X || !u) return ceed_error("CeedXContactApplyResidualAdd: no coordinate / displacement vector");
  if (!S->has_obstacle) return ceed_error("CeedXContactApplyResidualAdd: no obstacle set (CeedXContactSetObstacle)");
  return contact_apply(S, "CeedXContactApplyResidualAdd", CONTACT_RESIDUAL, scale, X, u, state, y);
}

extern "C" int CeedXContactApplyTangentAdd(CeedXContact S, CeedScalar scale, CeedVector state, CeedVector du, CeedVector y) {
  if (!du) return ceed_error("CeedXContactApplyTangentAdd: no variation vector");
  return contact_apply(S, "CeedXContactApplyTangentAdd", CONTACT_TANGENT, scale, du, nullptr, state, y);
}

extern "C" int CeedXContactDiagonalAdd(CeedXContact S, CeedScalar scale, CeedVector state, CeedVector d) {
  return contact_apply(S, "CeedXContactDiagonalAdd", CONTACT_DIAGONAL, scale, nullptr, nullptr, state, d);
}

extern "C" int CeedXContactGetKernelName(CeedXContact S, const char **name) { *name = S->fs.kernel_name.c_str(); return 0; }
