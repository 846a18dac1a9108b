// ceed_restriction.cpp -- CeedElemRestriction (offsets and strided) and the transpose maps the deterministic, atomic-free
// scatter is built on (set-up time, host).  Reference: CreateRestrictionPlex -> CeedElemRestrictionCreate
// (src/setuplibceed.c:194-240), CeedElemRestrictionCreateStrided with CEED_STRIDES_BACKEND (:304-318).
#include "ceed_impl.hpp"
#include "index_maps.hpp"
#include "row_code.hpp"

using namespace cps;

extern "C" int CeedElemRestrictionCreate(Ceed ceed, CeedInt nelem, CeedInt elemsize, CeedInt ncomp,
                                         CeedInt compstride, CeedInt lsize, CeedMemType mtype,
                                         CeedCopyMode, const CeedInt *offsets, CeedElemRestriction *rstr) {
  if (mtype != CEED_MEM_HOST) return ceed_error("restriction offsets are expected in host memory (setuplibceed.c:235)");
  if ((uint32_t)lsize > OFF_MASK) return ceed_error("L-vector of %d entries exceeds the 2^29 offset range of this backend", lsize);
  const size_t n = (size_t)nelem * elemsize;
  for (size_t i = 0; i < n; i++) {
    const long last = (long)offsets[i] + (long)(ncomp - 1) * compstride;
    if (offsets[i] < 0 || last >= lsize)
      return ceed_error("restriction offset %zu = %d out of range [0,%d)", i, offsets[i], lsize);
  }
  CeedElemRestriction r = new CeedElemRestriction_private;
  r->ceed = ceed; ceed_ref(ceed);
  r->nelem = nelem; r->elemsize = elemsize; r->ncomp = ncomp; r->compstride = compstride; r->lsize = lsize;
  r->h_offsets.assign(offsets, offsets + n);
  static_assert(sizeof(CeedInt) == sizeof(uint32_t), "the offsets are uploaded as they are (checked non-negative above)");
  const int ierr = r->d_offsets.upload(ceed, (const uint32_t *)offsets, n);
  if (ierr) { (void)CeedElemRestrictionDestroy(&r); return ierr; }
  *rstr = r;
  return 0;
}
extern "C" int CeedElemRestrictionCreateStrided(Ceed ceed, CeedInt nelem, CeedInt elemsize, CeedInt ncomp,
                                                CeedInt lsize, const CeedInt strides[3], CeedElemRestriction *rstr) {
  if ((long)nelem * elemsize * ncomp > lsize) return ceed_error("strided restriction larger than its L-vector");
  CeedElemRestriction r = new CeedElemRestriction_private;
  r->ceed = ceed; ceed_ref(ceed);
  r->nelem = nelem; r->elemsize = elemsize; r->ncomp = ncomp; r->lsize = lsize;
  r->strided = true;
  // CEED_STRIDES_BACKEND (setuplibceed.c:304-318): this backend lays q-point data out as
  // [element][component][point]: one contiguous run per wave-instruction in the fused kernels.
  r->backend_strides = strides[0] < 0;
  if (r->backend_strides) { r->strides[0] = 1; r->strides[1] = elemsize; r->strides[2] = elemsize * ncomp; }
  else {
    memcpy(r->strides, strides, sizeof r->strides);
    if (!(strides[0] == 1 && strides[1] == elemsize && strides[2] == elemsize * ncomp)) {
      (void)CeedElemRestrictionDestroy(&r);
      return ceed_error("only the [elem][comp][node] strided layout is supported on /gpu/hip/mi355x");
    }
  }
  *rstr = r;
  return 0;
}
extern "C" int CeedElemRestrictionCreateVector(CeedElemRestriction r, CeedVector *lvec, CeedVector *evec) {
  if (lvec) CHK(CeedVectorCreate(r->ceed, r->lsize, lvec));
  if (evec) CHK(CeedVectorCreate(r->ceed, r->nelem * r->elemsize * r->ncomp, evec));
  return 0;
}
extern "C" int CeedElemRestrictionApply(CeedElemRestriction r, CeedTransposeMode tmode, CeedVector u,
                                        CeedVector ru, CeedRequest *) {
  hipStream_t s = r->ceed->stream;
  const size_t esize = (size_t)r->nelem * r->elemsize * r->ncomp;
  CeedVector lv = tmode == CEED_NOTRANSPOSE ? u : ru, ev = tmode == CEED_NOTRANSPOSE ? ru : u;
  if (lv->length < r->lsize || (size_t)ev->length < esize) return ceed_error("restriction apply: L- or E-vector too short");
  double *pu, *pv;
  CHK(vec_dev(u, false, &pu));
  CHK(vec_dev(ru, true, &pv));
  if (r->strided) {  // identity layout: E == L
    if (tmode == CEED_NOTRANSPOSE) HIPCHK(hipMemcpyAsync(pv, pu, esize * sizeof(double), hipMemcpyDeviceToDevice, s));
    else HIPCHK(launch_axpby(pv, 1., pu, 1., esize, s));
    return 0;
  }
  if (tmode == CEED_NOTRANSPOSE) HIPCHK(launch_rstr_gather(r->d_offsets.get(), r->nelem, r->elemsize, r->ncomp, r->compstride, pu, pv, s));
  else if (r->nelem > 0) {   // v += E^T u: per row of the transpose map the contributors in element order, then one add
    CHK(build_csr(r, r->csr, nullptr));
    HIPCHK(launch_rstr_transpose(r->csr.view(), r->elemsize, r->ncomp, r->compstride, pu, pv, 1, s));
  }
  return 0;
}
extern "C" int CeedElemRestrictionGetMultiplicity(CeedElemRestriction r, CeedVector mult) {
  if (r->strided) return CeedVectorSetValue(mult, 1.);
  if (mult->length < r->lsize) return ceed_error("multiplicity vector shorter than the L-size");
  CHK(CeedVectorSetValue(mult, 0.));      // (entries no element holds stay zero)
  if (r->nelem <= 0) return 0;
  CHK(build_csr(r, r->csr, nullptr));
  HIPCHK(launch_multiplicity(r->csr.view(), r->ncomp, r->compstride, mult->d, r->ceed->stream));
  return 0;
}
extern "C" int CeedElemRestrictionDestroy(CeedElemRestriction *rstr) {
  if (!rstr || !*rstr) return 0;
  CeedElemRestriction r = *rstr;
  *rstr = nullptr;
  if (r == CEED_ELEMRESTRICTION_NONE) return 0;
  if (--r->refcount > 0) return 0;
  Ceed c = r->ceed;
  delete r;            // (before the reference goes: its arrays and maps retire into a Ceed that still exists)
  ceed_unref(c);
  return 0;
}

// The stencil code of a map's rows beside the arrays it was made from (row_code.hpp), under the options of the map's Ceed.  Called where a
// RowMap gets its arrays, so never while a graph is recorded.
int upload_row_code(Ceed c, RowMap &M, const std::vector<uint32_t> &rowptr, const std::vector<uint32_t> &cols) {
  if (!c->opt.row_code) return 0;
  const RowCode code = row_code_encode(rowptr, cols, c->opt.row_code_max);
  static_assert(sizeof(RowStencil) == 8 * sizeof(uint32_t), "a stencil is uploaded as eight words");
  CHK(M.d_pos0.upload(c, code.pos0)); CHK(M.d_sid.upload(c, code.sid));
  CHK(M.d_stencil.upload(c, (const uint32_t *)code.table.data(), code.table.size() * 8));
  M.nstencils = (int)code.table.size(); M.nescape = (int)code.nescape;
  return 0;
}

// The transpose map of a restriction (index_maps.hpp: transpose_map), built once per map and uploaded with its stencil code.  With `prio`
// the flagged nodes come first; `skipP` > 0 leaves the element-interior nodes out (the caller has checked rstr_interior_private()).
int build_csr(CeedElemRestriction r, CsrMap &M, const unsigned char *prio, int skipP) {
  if (M.built) return 0;
  if (r->ceed->capturing)
    return ceed_error("first apply of an operator during graph capture: its restriction's transpose map is built on the host; "
                      "apply the operator once before recording");
  TransposeMap T = transpose_map(r->h_offsets, r->lsize, r->elemsize, r->ncomp, prio, skipP);
  M.h_node_off = std::move(T.node_off); M.h_rowptr = std::move(T.rowptr); M.h_cols = std::move(T.cols);
  M.nprio = T.nprio; M.nskipped = T.nskipped; M.full_cover = T.full_cover;
  M.nrows = (int)M.h_node_off.size();
  CHK(M.d_rowptr.upload(r->ceed, M.h_rowptr)); CHK(M.d_cols.upload(r->ceed, M.h_cols)); CHK(M.d_node_off.upload(r->ceed, M.h_node_off));
  CHK(upload_row_code(r->ceed, M, M.h_rowptr, M.h_cols));
  M.built = true;
  return 0;
}
// Are the element-interior nodes of an offsets restriction private to their element (index_maps.hpp)?  Asked once per restriction.
bool rstr_interior_private(CeedElemRestriction r, int P) {
  if (r->interior_private) return r->interior_private > 0;
  r->interior_private = interior_nodes_private(r->h_offsets, r->lsize, r->elemsize, r->ncomp, r->compstride, P) ? 1 : -1;
  return r->interior_private > 0;
}

// Node offsets of the element-interior nodes (the ones the fused kernel stores itself), [elem][(P-2)^3] in element-local order.
int build_interior_list(CeedElemRestriction r, int P) {
  if (r->d_int_off || P < 3) return 0;
  if (r->ceed->capturing) return ceed_error("first apply of an operator during graph capture: apply it once before recording");
  CHK(r->d_int_off.upload(r->ceed, interior_node_list(r->h_offsets, r->elemsize, P)));
  r->int_per_elem = (P - 2) * (P - 2) * (P - 2);
  return 0;
}

// The pipelined re-ordering of map M (index_maps.hpp: pipe_segment_count, pipe_elem_bound, pipe_reorder), under the round limits of the
// restriction's Ceed.
// Maps are cached per restriction and never replaced: a recorded graph, or a second operator with another quadrature on
// the same restriction, keeps valid pointers.  A launch too small to pipeline gets a map with nseg = 1 and NO copies.
int get_pipe(CeedElemRestriction r, const CsrMap &M, int E, int per_elem, int req_seg_in, int waves, int mb, PipeMap **out) {
  for (auto &p : r->pipes)
    if (p->E == E && p->req_seg == req_seg_in && p->waves == waves && p->mb == mb && p->base == &M) { *out = p.get(); return 0; }
  const CeedOptions &opt = r->ceed->opt;
  const int nseg = pipe_segment_count(r->nelem, E, per_elem, req_seg_in, waves, mb, opt.pipe_min_rounds, opt.pipe_min_total_rounds);
  if (nseg >= 2 && r->ceed->capturing) { *out = nullptr; return 0; }   // cold map while recording: the caller takes the serial path (its map exists)
  std::unique_ptr<PipeMap> Gp(new PipeMap);     // (dropped with its arrays by an error return below)
  PipeMap &G = *Gp;
  G.E = E; G.req_seg = req_seg_in; G.waves = waves; G.mb = mb; G.base = &M;
  if (nseg < 2) { G.nseg = 1; *out = Gp.get(); r->pipes.push_back(std::move(Gp)); return 0; }
  G.elem_bound = pipe_elem_bound(r->nelem, E, nseg, waves, opt.pipe_min_rounds);
  G.nseg = (int)G.elem_bound.size() - 1;
  PipeRows R = pipe_reorder(M.h_node_off, M.h_rowptr, M.h_cols, G.elem_bound, per_elem);
  G.row_bound = std::move(R.row_bound); G.h_node_off = std::move(R.node_off);
  G.nrows = M.nrows;
  CHK(G.d_rowptr.upload(r->ceed, R.rowptr)); CHK(G.d_cols.upload(r->ceed, R.cols)); CHK(G.d_node_off.upload(r->ceed, G.h_node_off));
  CHK(upload_row_code(r->ceed, G, R.rowptr, R.cols));
  *out = Gp.get();
  r->pipes.push_back(std::move(Gp));
  return 0;
}
