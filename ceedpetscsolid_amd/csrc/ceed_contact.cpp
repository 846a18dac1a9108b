// ceed_contact.cpp -- frictionless penalty contact of side sets with a rigid plane or sphere (CeedXContact*, include/ceed_contact.h):
// residual, tangent and diagonal on a list of element faces (kernels_contact.hip).  The host layer is the surface loads': the faces'
// transpose map is index_maps.hpp's, their Dirichlet flags ride in the top bits of the face offsets (face_offsets) and per row of the
// map (row_flag_bits), the sum is k_surface_sum's, in face order.  The map and the row flags are made at the first apply (never while a
// graph is recorded), the flagged offsets when they are set.  The contact state [nface][7][Q^2] is the caller's vector: the residual
// writes it, the tangent and the diagonal of any p-level read it.
#include "ceed_impl.hpp"
#include <ceed_contact.h>
#include "index_maps.hpp"

using namespace cps;

struct CeedXContact_private {
  Ceed ceed = nullptr;
  int nface = 0, P = 0, Q = 0, lsize = 0;
  std::vector<int> h_offsets;               // [nface][P^2] component-0 L-offsets
  std::vector<unsigned char> h_mask;        // copy of the Dirichlet mask (empty: none)
  DevArray<uint32_t> d_offsets;             // the offsets with the flag bits of their nodes
  RowMap map;                               // transpose map of the faces: rows = the nodes on the contact surface
  bool map_built = false;
  DevArray<unsigned char> d_row_flags;      // the mask per row of the map
  bool flags_built = false;
  BasisTables tables, tables_sq;            // 1-D B, D and weights of (P nodes, Q Gauss points); B entry-wise squared (diagonal)
  bool has_obstacle = false;
  int kind = 0;
  double par[8] = {0., 0., 0., 0., 0., 0., 0., 0.}, penalty = 0.;
  std::string kernel_name;
  size_t state_len() const { return (size_t)nface * CONTACT_NSTATE * Q * Q; }
};

extern "C" int CeedXContactDestroy(CeedXContact *ct) {
  if (!ct || !*ct) return 0;
  CeedXContact S = *ct;
  *ct = nullptr;
  Ceed c = S->ceed;
  delete S;            // (before the reference goes: its arrays retire into a Ceed that still exists)
  ceed_unref(c);
  return 0;
}

extern "C" int CeedXContactCreate(Ceed ceed, CeedInt nface, CeedInt P, CeedInt Q, const CeedInt *offsets, CeedInt lsize, CeedXContact *ct) {
  if (ceed->capturing) return ceed_error("CeedXContactCreate during graph capture");
  if (nface < 0) return ceed_error("CeedXContactCreate: nface = %d is negative", nface);
  if (!contact_instantiated(P, Q)) return ceed_error("no contact kernel for P=%d Q=%d (P = 2 .. 8, Q = P .. 8)", P, Q);
  if (lsize < 0 || (size_t)lsize > (size_t)OFF_MASK) return ceed_error("CeedXContactCreate: L-size %d outside [0, 2^29)", lsize);
  if (nface > 0 && !offsets) return ceed_error("CeedXContactCreate: no offsets");
  if ((size_t)nface * P * P > (size_t)0x7FFFFFFF / 3 || (size_t)nface * Q * Q > (size_t)0x7FFFFFFF / CONTACT_NSTATE)
    return ceed_error("CeedXContactCreate: %d faces are too many", nface);
  const size_t n = (size_t)nface * P * P;
  for (size_t i = 0; i < n; i++) {
    const long o = offsets[i];
    if (o < 0 || o + 2 >= (long)lsize) return ceed_error("CeedXContactCreate: offset %ld of face %zu lies past the L-size %d", o, i / ((size_t)P * P), lsize);
    if (o % 3) return ceed_error("CeedXContactCreate: offset %ld of face %zu is no multiple of 3 (component-0 offsets of interlaced nodes)", o, i / ((size_t)P * P));
  }
  CeedXContact S = new CeedXContact_private;
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
    memset(&S->tables_sq, 0, sizeof S->tables_sq);
    for (size_t i = 0; i < b->interp1d.size(); i++) S->tables_sq.interp[i] = b->interp1d[i] * b->interp1d[i];
    CHK(CeedBasisDestroy(&b));
    return S->d_offsets.upload(ceed, face_offsets(S->h_offsets, nullptr));
  };
  const int ierr = fill();
  if (ierr) { (void)CeedXContactDestroy(&S); return ierr; }
  *ct = S;
  return 0;
}

extern "C" int CeedXContactSetDirichletMask(CeedXContact S, CeedMemType mtype, const unsigned char *mask, CeedInt lsize) {
  Ceed c = S->ceed;
  if (c->capturing) return ceed_error("CeedXContactSetDirichletMask during graph capture");
  if (mask && mtype != CEED_MEM_HOST) return ceed_error("pass the Dirichlet mask in host memory (it is folded into the offsets once)");
  if (mask && lsize < S->lsize) return ceed_error("Dirichlet mask shorter than the L-vector");
  if (mask) S->h_mask.assign(mask, mask + S->lsize); else S->h_mask.clear();
  S->d_row_flags.release(); S->flags_built = false;
  return S->d_offsets.upload(c, face_offsets(S->h_offsets, mask ? S->h_mask.data() : nullptr));
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

// the lazily made arrays: the faces' transpose map and the mask in its row order
static int contact_prepare(CeedXContact S) {
  Ceed c = S->ceed;
  if (S->map_built && S->flags_built) return 0;
  if (c->capturing) return ceed_error("first apply of a contact surface (or the first after its mask was set) during graph capture: apply once before recording");
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

// The checks every apply makes before anything is launched, then the launch and the node sum.  in0, in1: the L-vector inputs (either may
// be null); `state` is written by the residual and read otherwise; `y` is the L-vector the face results are added to.
static int contact_apply(CeedXContact S, const char *who, int mode, double scale, CeedVector in0, CeedVector in1, CeedVector state, CeedVector y) {
  Ceed c = S->ceed;
  if (!y || !state) return ceed_error("%s: no output / state vector", who);
  if (y->length < S->lsize || (in0 && in0->length < S->lsize) || (in1 && in1->length < S->lsize))
    return ceed_error("%s: vector shorter than the L-size %d", who, S->lsize);
  if ((size_t)state->length < S->state_len())
    return ceed_error("%s: state vector shorter than %zu = nface x 7 x Q^2 (nface = %d, Q = %d)", who, S->state_len(), S->nface, S->Q);
  if (y == in0 || y == in1 || y == state || (mode == CONTACT_RESIDUAL && (state == in0 || state == in1)))
    return ceed_error("%s: the output vector aliases an input", who);
  if (S->nface == 0) return 0;
  CHK(contact_prepare(S));
  ContactArgs a{};
  double *p0 = nullptr, *p1 = nullptr, *ps = nullptr, *py = nullptr;
  if (in0) CHK(vec_dev(in0, false, &p0));
  if (in1) CHK(vec_dev(in1, false, &p1));
  CHK(vec_dev(state, mode == CONTACT_RESIDUAL, &ps));
  CHK(vec_dev(y, true, &py));
  CHK(ceed_need_evec(c, (size_t)S->nface * S->P * S->P * 3));
  a.offsets = S->d_offsets.get(); a.state = ps; a.evec = c->evec.get();
  if (mode == CONTACT_RESIDUAL) { a.X = p0; a.u = p1; } else { a.du = p0; }
  a.nface = S->nface; a.kind = S->kind; a.penalty = S->penalty; a.scale = scale;
  for (int i = 0; i < 8; i++) a.par[i] = S->par[i];
  const char *kname = "";
  hipError_t e = launch_contact(S->P, S->Q, mode, mode == CONTACT_DIAGONAL ? S->tables_sq : S->tables, a, c->stream, &kname);
  if (e == hipErrorInvalidValue && !*kname) return ceed_error("no contact kernel for P=%d Q=%d", S->P, S->Q);
  HIPCHK(e);
  S->kernel_name = kname;
  HIPCHK(launch_surface_sum(S->map.view(), S->d_row_flags.get(), a.evec, py, c->stream));
  return 0;
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

extern "C" int CeedXContactGetKernelName(CeedXContact S, const char **name) { *name = S->kernel_name.c_str(); return 0; }
