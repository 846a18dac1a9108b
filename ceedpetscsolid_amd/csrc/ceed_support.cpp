// ceed_support.cpp -- linear spring and dashpot supports on side sets (CeedXSupport*, include/ceed_support.h): the state of a layer
// (k_n, k_t) on a list of element faces, and force, tangent and diagonal from a state (the support modes of k_contact and its tangent and
// diagonal modes, kernels_contact.hip) over a face set (face_set.hpp).  The state [nface][7][Q^2] is the caller's vector, laid out as the
// contact state: FormState writes it, the applies of any p-level read it.
#include "face_set.hpp"
#include <ceed_support.h>

using namespace cps;

struct CeedXSupport_private {
  FaceSet fs;
  BasisTables tables_sq;                    // fs.tables with B entry-wise squared (diagonal)
  size_t state_len() const { return (size_t)fs.nface * CONTACT_NSTATE * fs.Q * fs.Q; }
};

extern "C" int CeedXSupportDestroy(CeedXSupport *sp) { return face_handle_destroy(sp); }

extern "C" int CeedXSupportCreate(Ceed ceed, CeedInt nface, CeedInt P, CeedInt Q, const CeedInt *offsets, CeedInt lsize, CeedXSupport *sp) {
  if (nface > 0 && contact_instantiated(P, Q) && (size_t)nface * Q * Q > (size_t)0x7FFFFFFF / CONTACT_NSTATE)    // the state is indexed in 32 bits
    return ceed_error("CeedXSupportCreate: %d faces are too many", nface);
  CeedXSupport S = new CeedXSupport_private;
  const int ierr = face_set_create(S->fs, "CeedXSupportCreate", ceed, nface, P, Q, offsets, lsize, contact_instantiated, "support", "P = 2 .. 8, Q = P .. 8");
  if (ierr) { (void)CeedXSupportDestroy(&S); return ierr; }
  memset(&S->tables_sq, 0, sizeof S->tables_sq);
  for (int i = 0; i < Q * P; i++) S->tables_sq.interp[i] = S->fs.tables.interp[i] * S->fs.tables.interp[i];
  *sp = S;
  return 0;
}

extern "C" int CeedXSupportSetDirichletMask(CeedXSupport S, CeedMemType mtype, const unsigned char *mask, CeedInt lsize) {
  return face_set_mask(S->fs, "CeedXSupportSetDirichletMask", mtype, mask, lsize);
}

static int support_check_state(CeedXSupport S, const char *who, CeedVector state) {
  if (!state) return ceed_error("%s: no state vector", who);
  if ((size_t)state->length < S->state_len())
    return ceed_error("%s: state vector shorter than %zu = nface x 7 x Q^2 (nface = %d, Q = %d)", who, S->state_len(), S->fs.nface, S->fs.Q);
  return 0;
}

// The state kernel writes the state and nothing else: no E-vector, no node sum, so no transpose map either.
extern "C" int CeedXSupportFormState(CeedXSupport S, CeedScalar kn, CeedScalar kt, CeedVector X, CeedVector state) {
  const char *who = "CeedXSupportFormState";
  FaceSet &F = S->fs;
  if (!(kn >= 0.) || !(kt >= 0.) || !std::isfinite(kn) || !std::isfinite(kt))
    return ceed_error("%s: the coefficients kn = %g, kt = %g are not finite and non-negative", who, kn, kt);
  if (!X) return ceed_error("%s: no coordinate vector", who);
  CHK(support_check_state(S, who, state));
  if (X->length < F.lsize) return ceed_error("%s: vector shorter than the L-size %d", who, F.lsize);
  if (state == X) return ceed_error("%s: the output vector aliases an input", who);
  if (F.nface == 0) return 0;
  ContactArgs a{};
  double *px = nullptr, *ps = nullptr;
  CHK(vec_dev(X, false, &px));
  CHK(vec_dev(state, true, &ps));
  a.offsets = F.d_offsets.get(); a.X = px; a.state = ps; a.nface = F.nface;
  a.par[0] = kn; a.par[1] = kt;
  const char *kname = "";
  hipError_t e = launch_contact(F.P, F.Q, CONTACT_SUPPORT_STATE, F.tables, a, F.ceed->stream, &kname);
  if (e == hipErrorInvalidValue && !*kname) return ceed_error("no support kernel for P=%d Q=%d", F.P, F.Q);
  HIPCHK(e);
  F.kernel_name = kname;
  return 0;
}

// The checks every apply makes before anything is launched, then the launch and the node sum.  `in`: the L-vector input (null for the
// diagonal); `state` is read; `y` is the L-vector the face results are added to.
static int support_apply(CeedXSupport S, const char *who, int mode, double scale, CeedVector state, CeedVector in, CeedVector y) {
  FaceSet &F = S->fs;
  if (!y) return ceed_error("%s: no output vector", who);
  CHK(support_check_state(S, who, state));
  if (y->length < F.lsize || (in && in->length < F.lsize)) return ceed_error("%s: vector shorter than the L-size %d", who, F.lsize);
  if (y == in || y == state) return ceed_error("%s: the output vector aliases an input", who);
  if (F.nface == 0) return 0;
  CHK(face_set_prepare(F, "a support surface"));
  ContactArgs a{};
  double *pi = nullptr, *ps = nullptr, *py = nullptr;
  if (in) CHK(vec_dev(in, false, &pi));
  CHK(vec_dev(state, false, &ps));
  CHK(vec_dev(y, true, &py));
  a.offsets = F.d_offsets.get(); a.state = ps; a.du = pi; a.nface = F.nface; a.scale = scale;
  return face_set_apply(F, "support", py, [&](double *evec, const char **name) {
    a.evec = evec;
    return launch_contact(F.P, F.Q, mode, mode == CONTACT_DIAGONAL ? S->tables_sq : F.tables, a, F.ceed->stream, name);
  });
}

extern "C" int CeedXSupportApplyForceAdd(CeedXSupport S, CeedScalar scale, CeedVector state, CeedVector x, CeedVector y) {
  if (!x) return ceed_error("CeedXSupportApplyForceAdd: no input vector");
  return support_apply(S, "CeedXSupportApplyForceAdd", CONTACT_SUPPORT_FORCE, scale, state, x, y);
}

extern "C" int CeedXSupportApplyTangentAdd(CeedXSupport S, CeedScalar scale, CeedVector state, CeedVector dx, CeedVector y) {
  if (!dx) return ceed_error("CeedXSupportApplyTangentAdd: no variation vector");
  return support_apply(S, "CeedXSupportApplyTangentAdd", CONTACT_TANGENT, scale, state, dx, y);
}

extern "C" int CeedXSupportDiagonalAdd(CeedXSupport S, CeedScalar scale, CeedVector state, CeedVector d) {
  return support_apply(S, "CeedXSupportDiagonalAdd", CONTACT_DIAGONAL, scale, state, nullptr, d);
}

extern "C" int CeedXSupportGetKernelName(CeedXSupport S, const char **name) { *name = S->fs.kernel_name.c_str(); return 0; }
