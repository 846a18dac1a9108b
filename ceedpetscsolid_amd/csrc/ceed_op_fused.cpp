// ceed_op_fused.cpp -- the residual / Jacobian operator family of the MI355X backend (op_plan's fused_grad, ceed_operator.cpp): every form
// of its apply -- serial, pipelined, split phase, split phase with the halo exchange, fused with its consumer -- the two diagonals of the
// Jacobian operators, and the state kernel's entry point.
#include "ceed_operator.hpp"
#include "kernels_pointblock.hpp"

using namespace cps;

// a recording remembers each provenance buffer it read once (a V-cycle applies the same operators many times)
static void capture_dep(Ceed c, const GraphDep &d) {
  for (const GraphDep &e : c->capture_deps)
    if (e.v == d.v && e.geo == d.geo && e.derived == d.derived) return;
  d.v->refcount++;      // held from here: the vector may be destroyed by its creator before the recording ends
  c->capture_deps.push_back(d);
}
// how the last apply was launched (CeedXOperatorGetLaunchInfo)
static void set_launch_info(CeedOperator op, int segments, int streams, int assemble_launches, int last_segment_elems) {
  op->launch_info[0] = segments; op->launch_info[1] = streams; op->launch_info[2] = assemble_launches; op->launch_info[3] = last_segment_elems;
}

// The residual / Jacobian operator: k_fused_pencil (+ k_assemble).  Everything of one apply that does not depend on the element range of a launch.
struct FusedApply {
  FusedGradArgs a{};
  CeedElemRestriction r = nullptr;
  CeedBasis b = nullptr;
  int qfkind = 0;
  bool add = false, direct = false, split = false;
  CeedVector derived_for = nullptr;        // residual applies: the state vector whose derived state this apply writes
  double *py = nullptr;
  const CsrMap *M = nullptr;               // the transpose map of this apply (restriction's, shell, or the operator's split map)
  const RowMap *rows = nullptr;            // the rows it sums: M's, or (apply_fused) those of M's pipelined re-ordering
  const unsigned char *flags = nullptr;    // Dirichlet flags per row of `rows` (null: none)
};
// The Dirichlet flags of the operator's mask in the row order of a transpose map (index_maps.hpp: row_flag_bits) as an apply reads them
// (*flags null: no mask, or none on the output side): ONE cache per operator, keyed by the map.  Like every lazily built array of this layer they are made by an eager apply only, never while a graph is recorded.
int op_row_flags(CeedOperator op, CeedElemRestriction r, const RowMap &M, const unsigned char **flags) {
  *flags = nullptr;
  if (op->h_mask.empty() || !(op->mask_mode & 2)) return 0;
  for (auto &e : op->row_flags) if (e.first == &M) { *flags = e.second.get(); return 0; }
  if (op->ceed->capturing) return ceed_error("apply the operator once before recording (Dirichlet row flags)");
  DevArray<unsigned char> d;
  CHK(d.upload(op->ceed, row_flag_bits(M.h_node_off, op->h_mask.data(), r->ncomp, r->compstride)));
  *flags = d.get();
  op->row_flags.emplace_back(&M, std::move(d));
  return 0;
}
// vectors, tables, geometry provenance, physics, transpose map, flags, scratch: the launch arguments of this apply
static int fused_prepare(CeedOperator op, CeedVector in, CeedVector out, bool add, bool split, FusedApply &F) {
  CeedQFunction qf = op->qf;
  OpField &ai = op->in[op->i_active];
  CeedElemRestriction r = ai.rstr;
  Ceed c = op->ceed;
  if (!in || in == CEED_VECTOR_NONE || !out || out == CEED_VECTOR_NONE) return ceed_error("active vectors required");
  if (in->length < r->lsize || out->length < r->lsize) return ceed_error("active vector shorter than the restriction's L-size");
  if (in == out) return ceed_error("in-place operator apply is not supported");
  if (ai.basis->P1d > ai.basis->Q1d)   // planned for CeedXOperatorApplyState only (op_plan builds no even-odd tables for it)
    return ceed_error("operator with QFunction '%s' on a basis with more nodes than points (P=%d > Q=%d): no fused kernel applies it; "
                      "only its stored state can be written (CeedXOperatorApplyState)", qf->name.c_str(), ai.basis->P1d, ai.basis->Q1d);
  FusedGradArgs &a = F.a;
  F.r = r; F.b = ai.basis; F.qfkind = qf->kind; F.add = add; F.split = split;
  double *px, *pq, *ps = nullptr;
  CHK(vec_dev(in, false, &px));
  CHK(vec_dev(out, true, &F.py));
  CHK(vec_dev(op->in[op->i_qdata].vec, false, &pq));
  a.offsets = op->d_off_flagged ? op->d_off_flagged.get() : r->d_offsets.get();
  a.x = px; a.y = F.py; a.qdata = pq;
  CHK(read_phys(qf, &a.nu, &a.E));
  const int Q3 = ai.basis->Q1d * ai.basis->Q1d * ai.basis->Q1d;
  if (op->i_state >= 0) {
    CeedVector sv = op->in[op->i_state].vec;
    CHK(vec_dev(sv, false, &ps)); a.state_in = ps;
    // the derived state the residual kernel left beside grad u, if it still belongs to it (same elements, points, material)
    if (qf->kind == QF_HYPERFS_DF && c->opt.derived_state && pencil_derived_state(ai.basis->Q1d) && sv->derived_valid && sv->derived_nelem == r->nelem && sv->derived_Q3 == Q3 &&
        sv->derived_nu == a.nu && sv->derived_E == a.E) {
      F.qfkind = QF_HYPERFS_DF_DS;
      a.state_in = sv->derived.get();
      if (c->capturing) capture_dep(c, GraphDep{sv, nullptr, sv->derived.get()});
    }
  }
  if (op->o_state >= 0) {
    CeedVector sv = op->out[op->o_state].vec;
    if (!is_passive(sv)) return ceed_error("state output needs a passive vector");
    CHK(vec_dev(sv, true, &ps)); a.state_out = ps;  // every point is overwritten (and the derived state invalidated)
    if (qf->kind == QF_HYPERFS_F && c->opt.derived_state && pencil_derived_state(ai.basis->Q1d) && !split) {
      const size_t need = (size_t)r->nelem * 10 * Q3;
      if (sv->derived.size() < need) {
        if (c->capturing) return ceed_error("evaluate the residual once before recording (derived-state buffer)");
        CHK(sv->derived.alloc(c, need));
      }
      a.state_out2 = sv->derived.get();
      F.derived_for = sv;
    }
  }
  a.mask_in = (op->mask_mode & 1) ? 1 : 0; a.mask_out = (op->mask_mode & 2) ? 1 : 0;
  a.mass_c = op->mass_term;     // (non-zero on a Jacobian operator only: CeedXOperatorSetMassTerm)
  if (pencil_even_odd(ai.basis->Q1d)) memcpy(a.eo, op->eo, sizeof a.eo);
  {  // geometric factors recomputed in the kernel if the qdata vector still is what SetupGeo wrote on these elements
    CeedVector qv = op->in[op->i_qdata].vec;
    bool same_rule = qv->geo && qv->geo_nelem == r->nelem && qv->geo_Q == ai.basis->Q1d;
    for (int i = 0; same_rule && i < ai.basis->Q1d; i++)
      same_rule = qv->geo_qref[i] == ai.basis->qref1d[i] && qv->geo_qwt[i] == ai.basis->qweight1d[i];
    if (same_rule && c->opt.recompute_geo) {
      a.geo = qv->geo.get();
      a.geo_aff = qv->geo_aff.get();
      a.geo_swept = qv->geo_swept.get(); a.geo_axis = qv->geo_axis;
      for (int i = 0; i < ai.basis->Q1d; i++) { a.qref[i] = qv->geo_qref[i]; a.qwt[i] = qv->geo_qwt[i]; }
      if (c->capturing) capture_dep(c, GraphDep{qv, qv->geo.get(), nullptr});
    }
  }
  lame_constants(a.nu, a.E, &a.lambda, &a.TwoMu);
  if (split && (add || op->ovl_lead <= 0 || !op->ovl_csr.built))
    return ceed_error("split-phase apply needs CeedXOperatorSetOverlapSplit and overwrite mode");
  a.elem_begin = 0; a.nelem = r->nelem;
  // element-interior nodes straight to y: overwrite mode only (split maps are built to match, see SetOverlapSplit)
  F.direct = !add && c->opt.direct_interior && rstr_interior_private(r, ai.basis->P1d);
  a.direct = F.direct ? 1 : 0;
  // atomic-free, deterministic scatter: element results -> E-vector -> per-node sums
  if (split) {
    F.M = &op->ovl_csr;
    if ((F.M->nskipped > 0) != F.direct) return ceed_error("split-phase map and direct-store mode disagree");
  } else if (F.direct) {
    CHK(build_csr(r, r->csr_shell, nullptr, ai.basis->P1d));
    CHK(build_interior_list(r, ai.basis->P1d));
    F.M = &r->csr_shell;
  } else {
    CHK(build_csr(r, r->csr, nullptr));
    F.M = &r->csr;
  }
  F.rows = F.M;
  CHK(op_row_flags(op, r, *F.rows, &F.flags));
  a.evec_stride = 3 * (F.direct ? element_shell_size(ai.basis->P1d) : r->elemsize);
  CHK(ceed_need_evec(c, (size_t)r->nelem * std::max((size_t)3 * (size_t)r->elemsize, (size_t)a.evec_stride)));   // (an aligned shell block may exceed P^3 records at small P)
  a.evec = c->evec.get();
  if (F.derived_for) {   // this (whole) residual apply also writes the tangent's derived state beside grad u: valid from here on in stream order
    CeedVector sv = F.derived_for;
    sv->derived_valid = true; sv->derived_nelem = r->nelem; sv->derived_Q3 = Q3;
    sv->derived_nu = a.nu; sv->derived_E = a.E;
  }
  return 0;
}
// one launch of the fused kernel over elements [e0, e0 + ne); its name and how it obtained the geometric factors stay on the operator
static int fused_launch(CeedOperator op, const FusedApply &F, int e0, int ne, int wave_groups, hipStream_t s) {
  FusedGradArgs ak = F.a;
  ak.elem_begin = e0; ak.nelem = ne;
  const char *kname = "";
  // with a mass term the other entry of the same body, K + c M in this one launch; without, the kernels there always were
  const bool mass = F.a.mass_c != 0.;
  hipError_t e = (mass ? launch_fused_mass : launch_fused_grad)(F.b->P1d, F.b->Q1d, F.qfkind, op->tables, ak, FusedLaunch{wave_groups, op->ceed->opt.pencil_waves}, s, &kname);
  if (no_kernel(e, kname))
    return ceed_error("no fused kernel %sinstantiated for P=%d Q=%d QFunction %s", mass ? "with the mass term " : "", F.b->P1d, F.b->Q1d, op->qf->name.c_str());
  HIPCHK(e);
  set_kernel_name(op, kname, true);
  op->geo_mode = fused_geo_mode(F.a);
  return 0;
}
// rows [row0, row0 + nrows) of the apply's row map summed into y: the one k_assemble launch of the serial, split-phase and pipelined forms
static int assemble_rows(const FusedApply &F, int row0, int nrows, hipStream_t s, const HaloUnpackArgs *un = nullptr,
                         const HaloPackFold *pk = nullptr) {
  HIPCHK(launch_assemble(F.rows->view().rows(row0, nrows), F.flags, F.a.evec, F.py, F.add ? 1 : 0, s, un, pk));
  return 0;
}
// The pack of halo H folded into the launch that sums the rows of map M: per row the send slots of its node's entries (index_maps.hpp:
// pack_fold).  Built once per (map, halo); not ok (-> the separate pack kernel) if an entry of the halo is no row of the map.
static int get_pack_fold(CeedOperator op, CeedElemRestriction r, const RowMap *M, CeedXHalo H, HaloPackFold *out, bool *ok) {
  for (auto &pf : op->pack_folds)
    if (pf.M == M && pf.H == H && pf.serial == H->serial) { *ok = pf.ok; *out = HaloPackFold{pf.d_ptr.get(), pf.d_slot.get(), H->send.get()}; return 0; }
  CeedOperator_private::PackFold pf{M, H, H->serial, {}, {}, false};
  if (op->ceed->capturing) { *ok = false; return 0; }     // cold while recording: the separate pack kernel
  const PackFoldLists L = pack_fold(M->h_node_off, H->h_idx, r->ncomp, r->compstride);
  if (L.ok) {
    CHK(pf.d_ptr.upload(op->ceed, L.ptr)); CHK(pf.d_slot.upload(op->ceed, L.slot));
    pf.ok = true;
  }
  *ok = pf.ok; *out = HaloPackFold{pf.d_ptr.get(), pf.d_slot.get(), H->send.get()};
  op->pack_folds.push_back(std::move(pf));
  return 0;
}

// The second chain of an apply on two streams: the side stream starts behind what the Ceed's stream holds (fork), the Ceed's stream
// goes on behind the side stream's work (join); seg_event: the event of segment k, made when first asked for.
static int side_fork(Ceed c) {
  CHK(ceed_need_side_stream(c));
  HIPCHK(hipEventRecord(c->ev_fork, c->stream));
  HIPCHK(hipStreamWaitEvent(c->side_stream, c->ev_fork, 0));
  return 0;
}
static int side_join(Ceed c) {
  HIPCHK(hipEventRecord(c->ev_join, c->side_stream));
  HIPCHK(hipStreamWaitEvent(c->stream, c->ev_join, 0));
  return 0;
}
static int seg_event(Ceed c, int k, hipEvent_t *ev) {
  if (!c->ev_seg[k]) HIPCHK(hipEventCreateWithFlags(&c->ev_seg[k], hipEventDisableTiming));
  *ev = c->ev_seg[k];
  return 0;
}

// Whole apply, pipelined form: segment k's fused kernel AND its rows on stream k % 2 -- the fused kernel of
// segment k + 1 sits in the other queue and fills the chip as the waves of segment k retire (no kernel boundary between
// fused kernels), every k_assemble but the last runs beside a fused kernel.  Every row is summed in contributor order by
// one thread, whatever the segment: bitwise the serial result.
static int apply_pipelined(CeedOperator op, const FusedApply &F, const PipeMap *PM) {
  Ceed c = op->ceed;
  const int nseg = PM->nseg;
  set_launch_info(op, nseg, 2, nseg, PM->elem_bound[nseg] - PM->elem_bound[nseg - 1]);
  CHK(side_fork(c));
  hipEvent_t ev = nullptr, ev_before = nullptr;
  for (int k = 0; k < nseg; k++, ev_before = ev) {
    hipStream_t sk = (k & 1) ? c->side_stream : c->stream;     // (the FIRST segment on the operator's own stream; putting the last one there instead, so that the join is never waited for, measured 6-9 % slower at even segment counts)
    CHK(fused_launch(op, F, PM->elem_bound[k], PM->elem_bound[k + 1] - PM->elem_bound[k], 0, sk));
    // the rows of segment k have contributors in EARLIER segments too (the nodes on the cut between two segments):
    // segment k - 1's fused kernel runs on the other stream, the ones before it precede one of the two in stream order
    CHK(seg_event(c, k, &ev));
    HIPCHK(hipEventRecord(ev, sk));
    if (k >= 1) HIPCHK(hipStreamWaitEvent(sk, ev_before, 0));
    CHK(assemble_rows(F, PM->row_bound[k], PM->row_bound[k + 1] - PM->row_bound[k], sk));
  }
  return side_join(c);
}

// The segments of the pipelined form for a whole apply (get_pipe): from the persistent waves of a full launch of THIS kernel
// (pencil_waves_per_cu: LDS-limited from Q = 6 on), the E-vector records per element and the MB of E-vector per segment.  *PM null or
// of one segment: the serial form.
static int choose_pipe(CeedOperator op, const FusedApply &F, PipeMap **PM) {
  Ceed c = op->ceed;
  const int waves = device_cu_count() * (c->opt.pencil_waves > 0 ? c->opt.pencil_waves : pencil_waves_per_cu(F.b->Q1d));
  if (waves <= 0) return ceed_error("pipelined assembly: no persistent-wave count for P=%d Q=%d", F.b->P1d, F.b->Q1d);
  const int per_elem = F.direct ? element_shell_size(F.b->P1d) : F.r->elemsize;
  const bool fs = F.qfkind == QF_HYPERFS_DF || F.qfkind == QF_HYPERFS_DF_DS || F.qfkind == QF_HYPERFS_F;
  const int mb = c->opt.pipe_mb > 0 ? c->opt.pipe_mb : (fs ? 160 : 90);     // MB of E-vector per segment (get_pipe)
  return get_pipe(F.r, *F.M, pencil_group_elems(F.b->Q1d), per_elem, std::max(c->opt.pipe_segments, 0), waves, mb, PM);
}

// The interface sum of y behind a whole apply, in order on s: the pack (unless the rows' launch has done it), the RCCL group, the
// unpack-add launch.
static int halo_sum_behind(CeedXHalo H, double *y, bool packed, hipStream_t s) {
  if (packed) CHK(halo_send(H, s)); else CHK(halo_pack_and_send(H, y, s));
  CHK(halo_wait_arrivals(H, s));
  HIPCHK(launch_halo_unpack_add(halo_unpack_args(H), y, s));
  return 0;
}

// The whole apply.  `H` (overwrite mode only): the interface sum of the output follows IN ORDER on the same stream -- in the serial
// form the pack is folded into the rows' launch (HaloPackFold), then the RCCL group and the unpack-add launch.
int apply_fused(CeedOperator op, CeedVector in, CeedVector out, bool add, CeedXHalo H) {
  Ceed c = op->ceed;
  hipStream_t s = c->stream;
  FusedApply F;
  CHK(fused_prepare(op, in, out, add, false, F));
  // pipelined assembly: whole applies in overwrite mode, large enough for two segments -- the rows summed are then the pipelined map's
  PipeMap *PM = nullptr;
  if (c->opt.pipe_segments != 0 && !add) CHK(choose_pipe(op, F, &PM));
  if (PM && PM->nseg >= 2) { F.rows = PM; CHK(op_row_flags(op, F.r, *PM, &F.flags)); } else PM = nullptr;
  if (!add && !F.M->full_cover) CHK(dev_zero(c, F.py, (size_t)out->length));
  TimerScope ts(op, s);
  bool folded = false;
  if (PM) CHK(apply_pipelined(op, F, PM));
  else {
    set_launch_info(op, 1, 1, 1, F.r->nelem);
    CHK(fused_launch(op, F, 0, F.r->nelem, 0, s));
    HaloPackFold pk{nullptr, nullptr, nullptr};
    if (H && c->opt.fold_pack) CHK(get_pack_fold(op, F.r, F.M, H, &pk, &folded));
    CHK(assemble_rows(F, 0, F.M->nrows, s, nullptr, folded ? &pk : nullptr));   // timed together with the fused kernel: the launches ARE the operator apply
  }
  if (H) CHK(halo_sum_behind(H, F.py, folded, s));
  op->launches++;
  return 0;
}

// One half of a split-phase apply (CeedXOperatorApplyPhase) on the Ceed's stream: phase 0 the leading elements and the priority rows they
// alone contribute to, phase 1 the other elements and the other rows.
static int apply_fused_phase(CeedOperator op, CeedVector in, CeedVector out, int phase) {
  hipStream_t s = op->ceed->stream;
  FusedApply F;
  CHK(fused_prepare(op, in, out, false, true, F));
  if (phase == 0 && !F.M->full_cover) CHK(dev_zero(op->ceed, F.py, (size_t)out->length));
  const int e0 = phase ? op->ovl_lead : 0, ne = phase ? F.r->nelem - op->ovl_lead : op->ovl_lead;
  const int row0 = phase ? F.M->nprio : 0, nrows = phase ? F.M->nrows - F.M->nprio : F.M->nprio;
  TimerScope ts(op, s);
  CHK(fused_launch(op, F, e0, ne, 0, s));
  CHK(assemble_rows(F, row0, nrows, s));
  set_launch_info(op, 1, 1, 1, ne);
  op->launches++;
  return 0;
}

// The apply with its consumer fused behind it (CeedXOperatorApplyChebyshev / ApplyResidual): the launches of a whole apply in
// overwrite mode, with k_assemble_epi in place of k_assemble -- the shell rows' sums and the element-interior values the fused kernel
// stored into `t` go straight into the Chebyshev step (or the residual), y = t is never written or re-read as a whole.
// An apply that is not of that shape (a restriction that leaves L-vector entries without an element: full_cover) runs on its own, and
// *pt, null otherwise, is then the array of t for the caller to launch the consumer behind it: the two steps, one after the other.
static int apply_fused_epilogue(CeedOperator op, CeedVector in, CeedVector t, EpilogueArgs ep, double **pt) {
  hipStream_t s = op->ceed->stream;
  FusedApply F;
  *pt = nullptr;
  CHK(fused_prepare(op, in, t, false, false, F));
  const CsrMap *M = F.M;
  if (!M->full_cover) { CHK(apply_fused(op, in, t, false)); return vec_dev(t, false, pt); }
  const int nint = F.direct ? F.r->int_per_elem : 0;
  if (F.direct && !F.r->d_int_off) return ceed_error("interior-node list of the restriction missing");
  ep.t = F.py;
  TimerScope ts(op, s);
  // Always the serial form: with the consumer in the epilogue the rows' launch is no longer light enough to hide beside the next
  // segment's fused kernel, and the fork / join costs inside a replayed graph -- V-cycle at config 4's size: serial 6.05 ms eager and
  // replayed, pipelined 6.10 eager / 6.83 replayed (profiles/r05_ab_experiments.txt item 10).
  set_launch_info(op, 1, 1, 1, F.r->nelem);
  CHK(fused_launch(op, F, 0, F.r->nelem, 0, s));
  ep.int_off = nint ? F.r->d_int_off.get() : nullptr;
  ep.n_int = F.r->nelem * nint;
  HIPCHK(launch_assemble_epi(M->view(), F.flags, F.a.evec, ep, s));
  op->launches++;
  return 0;
}

// Split-phase apply WITH the interface sum, as one call (CeedXOperatorApplyWithHalo; the library-side form of
// ApplyLocalCeedOp + DMLocalToGlobal(ADD_VALUES), src/matops.c:46,57, on several GPUs).  Two chains:
//   Ceed's stream : fused kernel of the interface-touching elements -> their nodes' rows -> pack -> [RCCL on the comm stream]
//   side stream   : fused kernel of the interior elements (queued right behind the first: it fills the chip beside it and
//                   takes over the slots its waves free) -> the remaining rows + the arrivals of the exchange, ONE launch
// and the join.  Both chains are bitwise the whole apply followed by the exchange (same rows, same order, same sums).
static int apply_fused_with_halo(CeedOperator op, CeedVector in, CeedVector out, CeedXHalo H) {
  Ceed c = op->ceed;
  hipStream_t s = c->stream;
  FusedApply F;
  CHK(fused_prepare(op, in, out, false, true, F));
  const CsrMap *M = F.M;
  const int lead = op->ovl_lead, rest = F.r->nelem - lead;
  // Contract of this form: the arrivals are added by the SAME launch that overwrites the non-priority rows, and
  // the exchange starts when only the priority rows are complete -- so every entry of the halo must lie on a priority row of
  // the split map.  Checked once per (operator, halo) on the host.
  if (op->ovl_halo_checked != H->serial) {
    const long k = halo_entry_off_priority(M->h_node_off, M->nprio, H->h_idx);
    if (k >= 0)
      return ceed_error("CeedXOperatorApplyWithHalo: entry %u of the halo is not on a priority node of the operator's overlap split "
                        "(CeedXOperatorSetOverlapSplit): its partial sum would be exchanged before it is complete", H->h_idx[(size_t)k]);
    op->ovl_halo_checked = H->serial;
  }
  if (!M->full_cover) CHK(dev_zero(c, F.py, (size_t)out->length));
  TimerScope ts(op, s);
  const CeedOptions &o = c->opt;
  const HaloUnpackArgs un = halo_unpack_args(H);
  set_launch_info(op, 2, o.ovl_mode == 2 ? 2 : 1, 2, rest);
  if (o.ovl_mode != 2) {   // round 2's sequence on one stream
    CHK(fused_launch(op, F, 0, lead, 0, s));
    CHK(assemble_rows(F, 0, M->nprio, s));
    CHK(halo_pack_and_send(H, F.py, s));
    CHK(fused_launch(op, F, lead, rest, 0, s));
    CHK(halo_wait_arrivals(H, s));
    CHK(assemble_rows(F, M->nprio, M->nrows - M->nprio, s, &un));
    op->launches++;
    return 0;
  }
  CHK(side_fork(c));
  hipStream_t s1 = c->side_stream;
  hipEvent_t lead_done = nullptr;
  CHK(fused_launch(op, F, 0, lead, o.ovl_groups0, s));
  CHK(fused_launch(op, F, lead, rest, o.ovl_groups1, s1));
  CHK(seg_event(c, 0, &lead_done));
  HIPCHK(hipEventRecord(lead_done, s));             // the interface-touching elements also hold interior rows' contributors
  CHK(assemble_rows(F, 0, M->nprio, s));
  CHK(halo_pack_and_send(H, F.py, s));
  HIPCHK(hipStreamWaitEvent(s1, lead_done, 0));
  CHK(halo_wait_arrivals(H, s1));
  CHK(assemble_rows(F, M->nprio, M->nrows - M->nprio, s1, &un));
  CHK(side_join(c));
  op->launches++;
  return 0;
}

// Split-phase apply for communication overlap (the halo sum of matops.c:57 hidden under the interior
// elements): the first `n_leading_elems` elements must be the ONLY contributors of the nodes flagged in
// `priority` (one byte per L-vector entry, read at each node's first component).  Phase 0 computes those
// elements and finishes the flagged nodes; phase 1 does the rest.  Phase 0 then 1 == CeedOperatorApply.
extern "C" int CeedXOperatorSetOverlapSplit(CeedOperator op, CeedInt n_leading_elems, const unsigned char *priority,
                                            CeedInt lsize) {
  CHK(need_fused(op, "overlap split", Kind::either));
  CeedElemRestriction r = op->in[op->i_active].rstr;
  op->ovl_csr = CsrMap();     // a map not built, its counts and host copies reset with it (every reader asks `built` first); recorded
                              // graphs may still read the old split map and its flags: both are DevArrays
  op->ovl_halo_checked = 0;
  op->row_flags.erase(std::remove_if(op->row_flags.begin(), op->row_flags.end(), [&](const auto &e) { return e.first == &op->ovl_csr; }),
                      op->row_flags.end());     // (same address, new content)
  op->ovl_lead = 0;
  if (!priority) return 0;
  if (lsize < r->lsize || n_leading_elems < 0 || n_leading_elems > r->nelem) return ceed_error("bad overlap split arguments");
  // check the contract: every contributor of a priority node is a leading element
  const long bad = overlap_split_violation(r->h_offsets, r->elemsize, priority, n_leading_elems);
  if (bad >= 0) return ceed_error("element %zu touches a priority node but is not among the %d leading elements", (size_t)bad, n_leading_elems);
  const int P1 = op->in[op->i_active].basis->P1d;
  CHK(build_csr(r, op->ovl_csr, priority, (op->ceed->opt.direct_interior && rstr_interior_private(r, P1)) ? P1 : 0));
  op->ovl_lead = n_leading_elems;
  return 0;
}
extern "C" int CeedXOperatorApplyPhase(CeedOperator op, CeedVector in, CeedVector out, int phase) {
  CHK(need_fused(op, "split-phase apply", Kind::either));
  if (phase != 0 && phase != 1) return ceed_error("bad split-phase apply");
  return apply_fused_phase(op, in, out, phase);
}

// The split-phase apply and the interface sum of its output in ONE call: phase 0, the exchange started, phase 1 beside it,
// the arrivals added (apply_fused_with_halo).  `halo` with no neighbours: a plain apply.
extern "C" int CeedXOperatorApplyWithHalo(CeedOperator op, CeedVector in, CeedVector out, CeedXHalo halo) {
  CHK(need_fused(op, "split-phase apply", Kind::any));
  // refused whatever the halo holds (none, no neighbours, several): the call is the several-rank form of the apply
  if (op->mass_term != 0.)
    return ceed_error("CeedXOperatorApplyWithHalo: the operator carries a mass term (CeedXOperatorSetMassTerm); the interface sums of the "
                      "mass operator were never run over several ranks -- clear the term and apply the mass operator on its own");
  if (!halo || halo->nb.empty()) return CeedOperatorApply(op, in, out, CEED_REQUEST_IMMEDIATE);
  if (op->plan != PLAN_FUSED_GRAD) {
    CHK(CeedOperatorApply(op, in, out, CEED_REQUEST_IMMEDIATE));
    CHK(CeedXHaloStart(halo, out));
    return CeedXHaloFinish(halo, out);
  }
  if (halo->in_flight) return ceed_error("CeedXOperatorApplyWithHalo: an exchange is already in flight");
  if (is_passive(out) && out->length < halo->lsize_min) return ceed_error("CeedXOperatorApplyWithHalo: vector shorter than the halo's indices");
  // Default (CeedOptions::ovl_mode 0): the whole apply, then pack / RCCL group / unpack-add, IN ORDER on the Ceed's stream.
  // Measured on the emulated rank 3 of 8: 13 200 hexes at p = 4 -- split-phase on two streams 119 us, split-phase on
  // one stream 112 us, whole apply + exchange through the communicator's stream 120 us; a hand-over between two streams costs
  // more than the exchange it would hide.
  // (while a graph is recorded always this form: RCCL's calls record correctly only in order on the capturing stream)
  if (op->ceed->opt.ovl_mode == 0 || op->ceed->capturing || op->ovl_lead <= 0 || !op->ovl_csr.built) return apply_fused(op, in, out, false, halo);
  return apply_fused_with_halo(op, in, out, halo);
}

// The mass term of a Jacobian operator (include/ceed.h): K + c M in the launches of K.  The coefficient lives on the operator and goes into
// the launch arguments of every apply form (fused_prepare, fused_launch); the two diagonals never read it.
static int mass_term_shape(CeedOperator op, const char *who, int *P, int *Q) {
  if (op->composite) return ceed_error("%s: not provided for composite operators (call it on the sub-operators)", who);
  CHK(op_plan(op));
  if (op->plan != PLAN_FUSED_GRAD || op->o_state >= 0)
    return ceed_error("%s: a mass term belongs to a Jacobian operator (K + c M, the tangent of a dynamic solve); QFunction '%s' is %s", who,
                      op->qf ? op->qf->name.c_str() : "?", op->plan == PLAN_FUSED_GRAD ? "a residual" : "not of the residual / Jacobian family");
  *P = op->in[op->i_active].basis->P1d; *Q = op->in[op->i_active].basis->Q1d;
  return 0;
}
extern "C" int CeedXOperatorMassTermAvailable(CeedOperator op, int *has) {
  int P, Q;
  CHK(mass_term_shape(op, "CeedXOperatorMassTermAvailable", &P, &Q));
  *has = fused_mass_instantiated(P, Q, op->qf->kind) ? 1 : 0;
  return 0;
}
extern "C" int CeedXOperatorSetMassTerm(CeedOperator op, double c) {
  int P, Q;
  CHK(mass_term_shape(op, "CeedXOperatorSetMassTerm", &P, &Q));
  if (!(c == c) || c - c != 0.) return ceed_error("CeedXOperatorSetMassTerm: the coefficient must be finite");
  if (c != 0. && !fused_mass_instantiated(P, Q, op->qf->kind))
    return ceed_error("CeedXOperatorSetMassTerm: no fused kernel with the mass term is instantiated for P=%d Q=%d QFunction %s "
                      "(CeedXOperatorMassTermAvailable); apply the mass operator on its own", P, Q, op->qf->name.c_str());
  op->mass_term = c;
  return 0;
}

// The apply fused with its consumer (include/ceed.h; elasticity.c:539-552, 588-590)
static int epi_check(CeedOperator op, CeedVector in, CeedVector t, const char *who) {
  CHK(need_fused(op, who, Kind::jacobian));
  if (!in || !t || in == t) return ceed_error("%s: the scratch vector t must be a vector of its own", who);
  return 0;
}
extern "C" int CeedXOperatorApplyChebyshev(CeedOperator op, CeedVector in, CeedVector t, CeedVector x, CeedVector d, CeedVector r,
                                           CeedVector b, CeedVector dinv, double c1, double c2, int assign_x) {
  CHK(epi_check(op, in, t, "CeedXOperatorApplyChebyshev"));
  const bool first = b && b != CEED_VECTOR_NONE, has_r = r && r != CEED_VECTOR_NONE;
  const CeedInt n = x->length;
  if (d->length != n || (has_r && r->length != n) || dinv->length != n || t->length != n || in->length != n || (first && b->length != n))
    return ceed_error("CeedXOperatorApplyChebyshev: vector lengths differ");
  if (!first && !has_r) return ceed_error("CeedXOperatorApplyChebyshev: a residual vector r or a right-hand side b is needed");
  if (first && ((has_r && b == r) || b == x || b == d)) return ceed_error("CeedXOperatorApplyChebyshev: the right-hand side must be a vector of its own");
  if (t == x || t == d || (has_r && t == r) || t == dinv || (first && t == b)) return ceed_error("CeedXOperatorApplyChebyshev: the scratch vector t aliases an operand");
  EpilogueArgs ep{};
  ep.kind = EPI_CHEB;
  double *pb = nullptr, *pi;
  CHK(vec_dev(dinv, false, &pi));
  if (first) CHK(vec_dev(b, false, &pb));
  if (has_r) CHK(vec_dev(r, true, &ep.r));
  CHK(vec_dev(d, true, &ep.d)); CHK(vec_dev(x, true, &ep.x));
  ep.r0 = pb; ep.dinv = pi; ep.c1 = c1; ep.c2 = c2; ep.assign_x = assign_x;
  double *pt;
  CHK(apply_fused_epilogue(op, in, t, ep, &pt));
  if (pt) HIPCHK(launch_cheb_update(ep.x, ep.d, ep.r, ep.r0, pt, ep.dinv, c1, c2, assign_x, (size_t)n, op->ceed->stream));
  return 0;
}
extern "C" int CeedXOperatorApplyResidual(CeedOperator op, CeedVector in, CeedVector t, CeedVector b, CeedVector w) {
  CHK(epi_check(op, in, t, "CeedXOperatorApplyResidual"));
  const CeedInt n = w->length;
  if (b->length != n || t->length != n || in->length != n) return ceed_error("CeedXOperatorApplyResidual: vector lengths differ");
  if (t == b || t == w) return ceed_error("CeedXOperatorApplyResidual: the scratch vector t aliases an operand");
  EpilogueArgs ep{};
  ep.kind = EPI_RESID;
  double *pb;
  CHK(vec_dev(b, false, &pb));
  CHK(vec_dev(w, true, &ep.w));
  ep.b = pb;
  double *pt;
  CHK(apply_fused_epilogue(op, in, t, ep, &pt));
  if (pt) HIPCHK(launch_waxpby(ep.w, 1.0, pb, -1.0, pt, (size_t)n, op->ceed->stream));
  return 0;
}

// The scalar diagonal and libCEED's point-block diagonal of the Jacobian operators (width 1 / 3 values per L-dof of `assembled`; include/ceed.h),
// one call: the checks, the kernel's arguments, `assembled` zeroed (overwrite semantics, matops.c:227; nodes no element holds keep zeros), the
// kernel (k_diag_sf / k_pbdiag_sf, kernel_diag_sf.hpp: the 3 x 3 nodal blocks kept whole) and the sum over the transpose map.
// Deterministic: element contributions -> E-vector -> per-node sums in element order, no atomics.  The blocks are summed nine values wide
// (launch_pb_assemble: the destination of node offset o is 3 o, which the three-value kernel cannot address).
static int assemble_diagonal(CeedOperator op, CeedVector assembled, int width) {
  const char *who = width == 3 ? "point-block diagonal" : "diagonal";
  if (!op->composite) {
    CHK(op_plan(op));
    if (op->plan == PLAN_MASS)
      return width == 3 ? ceed_error("point-block diagonal assembly is not provided for the mass operator: its nodal blocks are its scalar "
                                     "diagonal times the identity (CeedOperatorLinearAssembleDiagonal)")
                        : mass_diagonal(op, assembled);
  }
  CHK(need_fused(op, (std::string(who) + " assembly").c_str(), Kind::jacobian));
  OpField &ai = op->in[op->i_active];
  CeedElemRestriction r = ai.rstr;
  hipStream_t s = op->ceed->stream;
  if (width == 3 && (r->ncomp != 3 || r->compstride != 1)) return ceed_error("%s: the active field must have 3 interlaced components", who);
  if (!is_passive(assembled) || (size_t)assembled->length < (size_t)width * (size_t)r->lsize)
    return ceed_error("%s vector too short: %d entries for %d x the L-size %d", who, assembled ? (int)assembled->length : 0, width, (int)r->lsize);
  DiagArgs a{};
  double *pd, *pq, *ps = nullptr;
  CHK(vec_dev(assembled, true, &pd));
  CHK(vec_dev(op->in[op->i_qdata].vec, false, &pq));
  if (op->i_state >= 0) CHK(vec_dev(op->in[op->i_state].vec, false, &ps));
  a.offsets = op->d_off_flagged ? op->d_off_flagged.get() : r->d_offsets.get();
  a.qdata = pq; a.state_in = ps; a.nelem = r->nelem;
  // one form for both widths: without flagged offsets the plain ones carry no flag bits, so the kernels read "nothing masked" either way
  a.mask_in = (op->d_off_flagged && (op->mask_mode & 1)) ? 1 : 0; a.mask_out = (op->d_off_flagged && (op->mask_mode & 2)) ? 1 : 0;
  CHK(read_phys(op->qf, &a.nu, &a.E));
  lame_constants(a.nu, a.E, &a.lambda, &a.TwoMu);
  CHK(dev_zero(op->ceed, pd, (size_t)assembled->length));
  CHK(build_csr(r, r->csr, nullptr));
  CHK(ceed_need_evec(op->ceed, (size_t)r->nelem * r->elemsize * 3 * width));
  a.evec = op->ceed->evec.get();
  const char *kname = "";
  hipError_t e = (width == 3 ? launch_pbdiag : launch_diag)(ai.basis->P1d, ai.basis->Q1d, op->qf->kind, op->tables, a, s, &kname);
  if (no_kernel(e, kname)) return ceed_error("no %s kernel for P=%d Q=%d %s", who, ai.basis->P1d, ai.basis->Q1d, op->qf->name.c_str());
  HIPCHK(e);
  if (width == 3) { HIPCHK(launch_pb_assemble(r->csr.view(), a.evec, pd, s)); set_kernel_name(op, kname, false); }
  else HIPCHK(launch_assemble(r->csr.view(), nullptr, a.evec, pd, 0, s));     // (and no name: the operator keeps that of its last apply)
  return 0;
}
extern "C" int CeedOperatorLinearAssembleDiagonal(CeedOperator op, CeedVector assembled, CeedRequest *) { return assemble_diagonal(op, assembled, 1); }
extern "C" int CeedOperatorLinearAssemblePointBlockDiagonal(CeedOperator op, CeedVector assembled, CeedRequest *) { return assemble_diagonal(op, assembled, 3); }

// The stored state alone (include/ceed.h): of an operator of the residual's shape -- du GRAD active, qdata NONE, dv GRAD active, gradu NONE
// passive -- only the passive output is written, grad u of `u` at the points of the operator's basis.  That basis may have MORE nodes than
// points (P_f, Q_c < P_f): the state of a coarse multigrid level that carries its own quadrature, refreshed from the fine displacement
// (solid.py, coarse_quadrature="own").  No physics, no transpose contraction, no E-vector, no k_assemble; the active output is not touched.
// The state vector is written through vec_dev(write): its version moves on and a derived state it may have carried is invalid from here,
// exactly as after any other writer -- recorded graphs that read the plain array replay correctly.
extern "C" int CeedXOperatorApplyState(CeedOperator op, CeedVector u) {
  CHK(need_fused(op, "CeedXOperatorApplyState", Kind::residual));
  Ceed c = op->ceed;
  hipStream_t s = c->stream;
  OpField &ai = op->in[op->i_active];
  CeedElemRestriction r = ai.rstr;
  CeedBasis b = ai.basis;
  CeedVector qv = op->in[op->i_qdata].vec, sv = op->out[op->o_state].vec;
  if (!is_passive(u) || u->length < r->lsize) return ceed_error("CeedXOperatorApplyState: displacement vector missing or shorter than the restriction's L-size");
  if (!is_passive(sv)) return ceed_error("state output needs a passive vector");
  if (!is_passive(qv)) return ceed_error("qdata needs a passive vector");
  const size_t Q3 = (size_t)b->Q1d * b->Q1d * b->Q1d;
  if ((size_t)sv->length < (size_t)r->nelem * 9 * Q3 || (size_t)qv->length < (size_t)r->nelem * 10 * Q3)
    return ceed_error("CeedXOperatorApplyState: state / qdata vector shorter than nelem x 9 (10) x Q^3");
  if (sv == u || qv == u || sv == qv) return ceed_error("CeedXOperatorApplyState: the vectors alias");
  StateArgs a{};
  double *px, *pq, *ps;
  CHK(vec_dev(u, false, &px));
  CHK(vec_dev(qv, false, &pq));
  CHK(vec_dev(sv, true, &ps));
  a.offsets = op->d_off_flagged ? op->d_off_flagged.get() : r->d_offsets.get();
  a.x = px; a.qdata = pq; a.state_out = ps; a.nelem = r->nelem; a.mask_in = (op->mask_mode & 1) ? 1 : 0;
  const char *kname = "";
  {
    TimerScope ts(op, s);
    hipError_t e = launch_state_at_points(b->P1d, b->Q1d, op->tables, a, s, &kname);
    if (no_kernel(e, kname)) return ceed_error("no state kernel instantiated for Pf=%d Qc=%d", b->P1d, b->Q1d);
    HIPCHK(e);
  }
  op->launches++;
  set_kernel_name(op, kname, false);
  return 0;
}
