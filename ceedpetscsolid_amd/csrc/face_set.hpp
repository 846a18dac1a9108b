// face_set.hpp -- what every term on a list of element faces keeps on the host (the surface loads of ceed_surface.cpp, where the
// functions below are defined, and the contact term of ceed_contact.cpp).  The faces' transpose map is index_maps.hpp's, their Dirichlet
// flags ride in the top bits of the face offsets like an operator's (face_offsets) and per row of the map (row_flag_bits); the sum is
// k_surface_sum's, in face order.  The map and the row flags are made at the first apply (never while a graph is recorded), the flagged
// offsets when they are set.  A handle holds a FaceSet as its member `fs`; the entry points keep the checks of their own arguments.
#pragma once
#include "ceed_impl.hpp"

struct FaceSet {
  Ceed ceed = nullptr;
  int nface = 0, P = 0, Q = 0, lsize = 0;
  std::vector<int> h_offsets;               // [nface][P^2] component-0 L-offsets
  std::vector<unsigned char> h_mask;        // copy of the Dirichlet mask (empty: none)
  DevArray<uint32_t> d_offsets;             // the offsets with the flag bits of their nodes
  RowMap map;                               // transpose map of the faces: rows = the nodes on the surface
  bool map_built = false;
  DevArray<unsigned char> d_row_flags;      // the mask per row of the map
  bool flags_built = false;
  cps::BasisTables tables;                  // 1-D B, D and weights of (P nodes, Q Gauss points)
  std::string kernel_name;
};

// `who`: the entry point, for the messages; `term` ("surface", "contact") and `pairs` word the refusal of a pair no kernel is built for.
// The set holds its reference to the Ceed from the first line on: after a refusal the caller destroys its handle as after a success.
int face_set_create(FaceSet &F, const char *who, Ceed ceed, CeedInt nface, CeedInt P, CeedInt Q, const CeedInt *offsets, CeedInt lsize,
                    bool (*instantiated)(int, int), const char *term, const char *pairs);
int face_set_mask(FaceSet &F, const char *who, CeedMemType mtype, const unsigned char *mask, CeedInt lsize);
// the lazily made arrays: the faces' transpose map and the mask in its row order; `what` ("a surface load") words the capture refusal
int face_set_prepare(FaceSet &F, const char *what);

// The tail of every apply: the face E-vector, the caller's launch(evec, &name) of its face kernel, then the node sum into y.
template <class Launch> int face_set_apply(FaceSet &F, const char *term, double *py, Launch launch) {
  Ceed c = F.ceed;
  CHK(ceed_need_evec(c, (size_t)F.nface * F.P * F.P * 3));
  const char *kname = "";
  hipError_t e = launch(c->evec.get(), &kname);
  if (e == hipErrorInvalidValue && !*kname) return ceed_error("no %s kernel for P=%d Q=%d", term, F.P, F.Q);
  HIPCHK(e);
  F.kernel_name = kname;
  HIPCHK(cps::launch_surface_sum(F.map.view(), F.d_row_flags.get(), c->evec.get(), py, c->stream));
  return 0;
}

// a handle with a FaceSet `fs`: gone before its reference to the Ceed (its arrays retire into a Ceed that still exists)
template <class H> int face_handle_destroy(H **h) {
  if (!h || !*h) return 0;
  H *S = *h;
  *h = nullptr;
  Ceed c = S->fs.ceed;
  delete S;
  ceed_unref(c);
  return 0;
}
