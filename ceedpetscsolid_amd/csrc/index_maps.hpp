// index_maps.hpp -- the index arithmetic of set-up (host): everything the device kernels index through, as free functions over
// std::vector -- the transpose maps and their pipelined re-orderings, the interior-node list, the Dirichlet flags, the owner map of the
// transfers, the pack fold of a halo and the arrival lists of an exchange.  Plain C++ like row_code.hpp: no HIP, no Ceed types, no
// options, so that tests/index_maps_host.cpp runs it alone under the sanitizers.  The library's builders (ceed_restriction.cpp,
// ceed_operator.cpp, ceed_op_fused.cpp, ceed_op_other.cpp, ceed_halo.cpp) keep the caches, the capture refusals and the uploads.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cstddef>
#include <utility>
#include <vector>

#include "kernels.hpp"

namespace cps {

// Transpose map of an offsets restriction: distinct node offsets and, per node, the E-vector positions of its contributors in element
// order.  Rows [0, nprio) are the priority nodes when the map was built with a priority mask.
struct TransposeMap {
  std::vector<uint32_t> node_off, rowptr, cols;
  int nprio = 0, nskipped = 0;
  bool full_cover = false;
};
// Build a transpose map (setup time, host): counting sort over the L-vector.  With `prio`
// (one byte per L-vector entry, tested at each node's component-0 offset) the flagged nodes
// come first.
// `skipP` > 0 (elemsize == skipP^3): nodes interior to an element are left out of the map -- the fused kernel
// stores them itself (FusedGradArgs::direct); the caller has checked interior_nodes_private().
inline TransposeMap transpose_map(const std::vector<int> &offsets, int lsize, int elemsize, int ncomp, const unsigned char *prio, int skipP) {
  TransposeMap M;
  const size_t n = offsets.size();
  std::vector<uint32_t> cnt((size_t)lsize + 1, 0u);
  for (size_t i = 0; i < n; i++) cnt[(size_t)offsets[i]]++;
  if (skipP > 0)
    for (size_t i = 0; i < n; i++)
      if (node_is_element_interior((int)(i % (size_t)elemsize), skipP)) { cnt[(size_t)offsets[i]] = 0; M.nskipped++; }   // stored by the fused kernel itself
  std::vector<uint32_t> slot((size_t)lsize, 0xFFFFFFFFu);
  std::vector<uint32_t> &rowptr = M.rowptr, &cols = M.cols;
  rowptr.push_back(0u);
  for (int pass = prio ? 0 : 1; pass < 2; pass++)
    for (int o = 0; o < lsize; o++) {
      if (!cnt[o]) continue;
      if (prio && ((prio[o] != 0) != (pass == 0))) continue;
      slot[o] = (uint32_t)M.node_off.size();
      M.node_off.push_back((uint32_t)o);
      rowptr.push_back(rowptr.back() + cnt[o]);
      if (prio && pass == 0) M.nprio++;
    }
  std::vector<uint32_t> cursor(rowptr.begin(), rowptr.end() - 1);
  cols.assign(rowptr.back() ? rowptr.back() : 1, 0u);
  for (size_t i = 0; i < n; i++) {  // element order => each node's contributors are sorted by element
    const uint32_t sl = slot[(size_t)offsets[i]];
    if (sl == 0xFFFFFFFFu) continue;
    // E position: e * elemsize + n, or in the shell-only E-vector of the direct-store mode e * shell size + shell rank
    const size_t e = i / (size_t)elemsize; const int ln = (int)(i % (size_t)elemsize);
    cols[cursor[sl]++] = skipP > 0 ? (uint32_t)(e * (size_t)element_shell_size(skipP) + (size_t)node_shell_rank(ln, skipP)) : (uint32_t)i;
  }
  // every L-vector entry is written by the assembly (or, for the skipped nodes, by the fused kernel)
  M.full_cover = (M.node_off.size() + (size_t)M.nskipped) * (size_t)ncomp == (size_t)lsize;
  return M;
}

// Are the element-interior nodes (local index 0 < i,j,k < P-1) of an offsets restriction private to their
// element?  True for every conforming mesh; checked because offsets are caller data.
inline bool interior_nodes_private(const std::vector<int> &offsets, int lsize, int elemsize, int ncomp, int compstride, int P) {
  if (P < 3 || (size_t)P * P * P != (size_t)elemsize || ncomp != 3 || compstride != 1) return false;
  std::vector<unsigned char> cnt((size_t)lsize, 0);
  for (size_t i = 0; i < offsets.size(); i++) {
    unsigned char &c = cnt[(size_t)offsets[i]];
    if (c < 2) c++;
  }
  for (size_t i = 0; i < offsets.size(); i++)
    if (node_is_element_interior((int)(i % (size_t)elemsize), P) && cnt[(size_t)offsets[i]] != 1) return false;
  return true;
}
// Node offsets of the element-interior nodes (the ones the fused kernel stores itself), [elem][(P-2)^3] in element-local order.
inline std::vector<uint32_t> interior_node_list(const std::vector<int> &offsets, int elemsize, int P) {
  const int m = (P - 2) * (P - 2) * (P - 2);
  const size_t nelem = offsets.size() / (size_t)elemsize;
  std::vector<uint32_t> lst(nelem * m);
  size_t k = 0;
  for (size_t e = 0; e < nelem; e++)
    for (int n = 0; n < elemsize; n++)
      if (node_is_element_interior(n, P)) lst[k++] = (uint32_t)offsets[e * elemsize + n];
  return lst;
}

// Segments of the pipelined assembly: element ranges whose group counts are whole rounds of the fused kernel's persistent
// waves (`waves` per launch) where the mesh is large enough for that -- a launch then ends with every wave finishing its
// last group at about the same time -- and the rows of the map sorted by the segment of their last contributor.
// The count first: `req_seg` segments asked for (0: one per `mb` MB of E-vector) of `nelem` elements in groups of `E`, `per_elem`
// E-vector records each.  1: a launch too small to pipeline.
inline int pipe_segment_count(int nelem, int E, int per_elem, int req_seg, int waves, int mb, int min_rounds, int min_total_rounds) {
  const int ngroups = (nelem + E - 1) / E;
  // at least `min_rounds` rounds per segment, else fewer segments (down to one: the caller then takes the serial path)
  // Below ~20 rounds of the persistent waves the fixed cost of the form (fork and join of the second stream, the summing
  // kernels competing with the fused kernel for memory: ~40 us at p = 4) exceeds what is hidden: measured -3 % at 24 rounds
  // (99 000 hexes, p = 4), +7 % at 11 rounds (44 928 hexes) -- such launches keep the serial form.
  if (min_rounds > 0 && ngroups < min_total_rounds * std::max(waves, 1)) req_seg = 1;
  // Segments asked for = 0: one per `mb` MB of E-vector -- a segment boundary costs ~10 us, and the smaller a segment the more of
  // its E-vector is still in the 256 MB last-level cache when its rows are summed (config 5, 1.4 GB of E-vector: 4.27 ms serial,
  // 4.00 with 3 segments, 3.57 with 8, 3.42 with 12-16 in round 2).  Rounds 2-3 used ~90 MB for every kernel (3 segments at config
  // 4); with round 4's faster fused kernel the finite-strain applies measure best at ~160 MB (config 4: 2 segments, -1.5 %; twice its
  // mesh: 3, -2 %; the whole of config 5: 9, +-0), the cheaper kernels (hyperSS, linElas: a shorter fused kernel to hide the same
  // rows behind) still at ~90 (profiles/r04_ab_experiments.txt item 14).  The caller passes the figure (apply_fused_grad).
  else if (req_seg == 0) req_seg = std::max(2, std::min(16, (int)((double)nelem * per_elem * 24. / (1e6 * std::max(mb, 1)) + 0.5)));
  return min_rounds > 0 ? std::max(1, std::min(req_seg, ngroups / (min_rounds * std::max(waves, 1)))) : std::min(req_seg, std::max(1, ngroups));
}
// The element boundaries of `nseg` >= 2 segments, 0 ... nelem; boundaries that coincide collapse (the result may hold fewer segments).
// Boundaries are laid out FROM THE END in whole rounds of the waves: the last segment (whose rows are summed with nothing
// to hide behind) is `last_rounds` rounds, the others share the rest equally in whole rounds, and the odd remainder of the
// mesh lands in the FIRST segment, where the next fused kernel fills the chip behind its ragged last round.  (Four rounds:
// the pipe sweeps of rounds 3-4.)
inline std::vector<int> pipe_elem_bound(int nelem, int E, int nseg, int waves, int min_rounds) {
  const int ngroups = (nelem + E - 1) / E;
  std::vector<int> elem_bound(1, 0);
  constexpr int last_rounds = 4;
  const long total_rounds = ngroups / std::max(waves, 1);
  std::vector<long> gb;        // group boundaries, descending
  if (min_rounds > 0 && total_rounds >= last_rounds + (long)(nseg - 1) * min_rounds) {
    long g = (long)ngroups - (long)last_rounds * waves;
    gb.push_back(g);
    const long per = (total_rounds - last_rounds) / (nseg - 1);       // rounds of the middle segments
    for (int k = nseg - 2; k >= 1; k--) { g -= per * waves; gb.push_back(g); }
  } else {
    for (int k = nseg - 1; k >= 1; k--) {
      long g = (long)ngroups * k / nseg;
      const long up = (long)ngroups - (((long)ngroups - g) / waves) * waves;           // whole rounds behind it, if that moves it sensibly
      gb.push_back(min_rounds > 0 && up > 0 && up < ngroups ? up : g);
    }
  }
  for (auto it = gb.rbegin(); it != gb.rend(); ++it) {
    const int e = (int)std::min<long>((long)nelem, *it * E);
    if (e > elem_bound.back() && e < nelem) elem_bound.push_back(e);
  }
  elem_bound.push_back(nelem);
  return elem_bound;
}
// The rows of a transpose map sorted by the segment of their last contributor: rows [row_bound[k], row_bound[k + 1]) are segment k's.
struct PipeRows {
  std::vector<int> row_bound;
  std::vector<uint32_t> node_off, rowptr, cols;
};
inline PipeRows pipe_reorder(const std::vector<uint32_t> &node_off, const std::vector<uint32_t> &rowptr, const std::vector<uint32_t> &cols,
                             const std::vector<int> &elem_bound, int per_elem) {
  PipeRows G;
  const int nn = (int)node_off.size(), nseg = (int)elem_bound.size() - 1;
  std::vector<int> seg((size_t)nn);
  std::vector<uint32_t> cnt((size_t)nseg + 1, 0u);
  for (int i = 0; i < nn; i++) {
    const int elast = (int)(cols[rowptr[i + 1] - 1] / (uint32_t)per_elem);      // contributors are in element order
    const int k = (int)(std::upper_bound(elem_bound.begin(), elem_bound.end(), elast) - elem_bound.begin()) - 1;
    seg[i] = k; cnt[(size_t)k + 1]++;
  }
  for (int k = 0; k < nseg; k++) cnt[k + 1] += cnt[k];
  G.row_bound.assign(cnt.begin(), cnt.end());
  std::vector<uint32_t> cursor(cnt.begin(), cnt.end() - 1), order((size_t)nn);
  for (int i = 0; i < nn; i++) order[cursor[seg[i]]++] = (uint32_t)i;   // stable: ascending node offset within a segment
  G.rowptr.assign((size_t)nn + 1, 0u); G.cols.resize(cols.size()); G.node_off.resize((size_t)nn);
  for (int j = 0; j < nn; j++) {
    const uint32_t i = order[j], len = rowptr[i + 1] - rowptr[i];
    for (uint32_t k = 0; k < len; k++) G.cols[G.rowptr[j] + k] = cols[rowptr[i] + k];
    G.rowptr[j + 1] = G.rowptr[j] + len;
    G.node_off[j] = node_off[i];
  }
  return G;
}

// the Dirichlet flag bits of the node at `offset`: bit c set where component c is masked
inline uint32_t node_flag_bits(const unsigned char *mask, uint32_t offset, int ncomp, int compstride) {
  uint32_t f = 0;
  for (int c = 0; c < ncomp && c < 3; c++) if (mask[(size_t)offset + (size_t)c * compstride]) f |= 1u << c;
  return f;
}
// the offsets of a restriction with the flag bits of their nodes in the top bits (OFF_FLAG_SHIFT)
inline std::vector<uint32_t> flagged_offsets(const std::vector<int> &offsets, const unsigned char *mask, int ncomp, int compstride) {
  std::vector<uint32_t> fl(offsets.size());
  for (size_t i = 0; i < fl.size(); i++) {
    const uint32_t o = (uint32_t)offsets[i];
    fl[i] = o | (node_flag_bits(mask, o, ncomp, compstride) << OFF_FLAG_SHIFT);
  }
  return fl;
}
// the offsets of the faces of a surface load (three interlaced components per node) as its kernel reads them: the flag bits of their
// nodes in the top bits under a mask, plain without one (`mask` null)
inline std::vector<uint32_t> face_offsets(const std::vector<int> &offsets, const unsigned char *mask) {
  if (mask) return flagged_offsets(offsets, mask, 3, 1);
  return std::vector<uint32_t>(offsets.begin(), offsets.end());
}
// The face offsets a caller hands to a face term, [nface][per_face] component-0 offsets of interlaced nodes in an L-vector of `lsize`
// entries, checked before anything is built from them: the first face that breaks a rule, its offset and which rule.
enum FaceOffsetFault : int { FACE_OFFSETS_OK = 0, FACE_OFFSETS_TOO_MANY, FACE_OFFSET_PAST_LSIZE, FACE_OFFSET_NOT_NODE };
struct FaceOffsetCheck { FaceOffsetFault fault; size_t face; long offset; };
inline FaceOffsetCheck check_face_offsets(const int *offsets, size_t nface, int per_face, int lsize) {
  if (nface * (size_t)per_face > (size_t)0x7FFFFFFF / 3) return {FACE_OFFSETS_TOO_MANY, 0, 0};    // the face E-vector is indexed in 32 bits
  for (size_t i = 0; i < nface * (size_t)per_face; i++) {
    const long o = offsets[i];
    if (o < 0 || o + 2 >= (long)lsize) return {FACE_OFFSET_PAST_LSIZE, i / (size_t)per_face, o};
    if (o % 3) return {FACE_OFFSET_NOT_NODE, i / (size_t)per_face, o};
  }
  return {FACE_OFFSETS_OK, 0, 0};
}
// the Dirichlet flags of a mask in the row order of a transpose map
inline std::vector<unsigned char> row_flag_bits(const std::vector<uint32_t> &node_off, const unsigned char *mask, int ncomp, int compstride) {
  std::vector<unsigned char> fl(node_off.size(), 0);
  for (size_t i = 0; i < fl.size(); i++) fl[i] = (unsigned char)node_flag_bits(mask, node_off[i], ncomp, compstride);
  return fl;
}

// The transfer operators in OWNER form (kernels_transfer.hip, k_transfer).
// own_f[e][n] = offset | fine-side Dirichlet flags if element e is the FIRST (in element order) to hold fine node n, else
// 0xFFFFFFFF.  `mask` null: no flags.  *full_cover: every entry of the fine L-vector has an owner.
inline std::vector<uint32_t> owner_map(const std::vector<int> &offsets, int lsize, const unsigned char *mask, int ncomp, int compstride,
                                       bool *full_cover) {
  const size_t n = offsets.size();
  std::vector<uint32_t> own(n ? n : 1);
  std::vector<unsigned char> seen((size_t)lsize, 0);
  size_t distinct = 0;
  for (size_t i = 0; i < n; i++) {
    const uint32_t o = (uint32_t)offsets[i];
    if (seen[o]) { own[i] = 0xFFFFFFFFu; continue; }
    seen[o] = 1; distinct++;
    own[i] = o | ((mask ? node_flag_bits(mask, o, ncomp, compstride) : 0u) << OFF_FLAG_SHIFT);
  }
  *full_cover = distinct * 3 == (size_t)lsize;
  return own;
}

// the node (component-0 offset) an entry of a halo belongs to: three interlaced components per node
inline uint32_t halo_entry_node(uint32_t d) { return d - d % 3u; }
// The pack of a halo folded into the launch that sums the rows of a map: per row the send slots of its node's entries, each with the
// entry's component in bits 30-31.  Not ok (-> the separate pack kernel) if an entry of the halo is no row of the map.
struct PackFoldLists {
  bool ok = false;
  std::vector<uint32_t> ptr, slot;
};
inline PackFoldLists pack_fold(const std::vector<uint32_t> &node_off, const std::vector<uint32_t> &halo_idx, int ncomp, int compstride) {
  PackFoldLists F;
  const int nn = (int)node_off.size(), total = (int)halo_idx.size();
  bool good = ncomp == 3 && compstride == 1 && halo_idx.size() < (1u << 30);
  std::vector<uint32_t> &ptr = F.ptr, &slot = F.slot;
  ptr.assign((size_t)nn + 1, 0u); slot.resize((size_t)(total ? total : 1));
  if (good) {
    // row of a node offset: the map's rows are distinct node offsets (ascending within each priority class): look up by sort
    std::vector<std::pair<uint32_t, uint32_t>> rows((size_t)nn);
    for (int i = 0; i < nn; i++) rows[(size_t)i] = {node_off[(size_t)i], (uint32_t)i};
    std::sort(rows.begin(), rows.end());
    std::vector<uint32_t> row_of((size_t)total);
    for (int k = 0; k < total && good; k++) {
      const uint32_t node = halo_entry_node(halo_idx[(size_t)k]);
      auto it = std::lower_bound(rows.begin(), rows.end(), std::make_pair(node, 0u));
      if (it == rows.end() || it->first != node) good = false;
      else { row_of[(size_t)k] = it->second; ptr[(size_t)it->second + 1]++; }
    }
    if (good) {
      for (int i = 0; i < nn; i++) ptr[(size_t)i + 1] += ptr[(size_t)i];
      std::vector<uint32_t> cur(ptr.begin(), ptr.end() - 1);
      for (int k = 0; k < total; k++) slot[cur[row_of[(size_t)k]]++] = (uint32_t)k | ((halo_idx[(size_t)k] % 3u) << 30);
    }
  }
  F.ok = good;
  return F;
}
// The first entry of a halo (its index in the list) whose node is none of the priority rows [0, nprio) of a map; -1: every entry lies on one.
inline long halo_entry_off_priority(const std::vector<uint32_t> &node_off, int nprio, const std::vector<uint32_t> &halo_idx) {
  std::vector<uint32_t> prio(node_off.begin(), node_off.begin() + nprio);
  std::sort(prio.begin(), prio.end());
  for (size_t k = 0; k < halo_idx.size(); k++)
    if (!std::binary_search(prio.begin(), prio.end(), halo_entry_node(halo_idx[k]))) return (long)k;
  return -1;
}
// The contract of an overlap split: every contributor of a priority node is one of the `n_leading` first elements.  The first element
// that breaks it; -1: it holds.
inline long overlap_split_violation(const std::vector<int> &offsets, int elemsize, const unsigned char *priority, int n_leading) {
  const size_t es = (size_t)elemsize;
  for (size_t i = 0; i < offsets.size(); i++)
    if (priority[(size_t)offsets[i]] && i / es >= (size_t)n_leading) return (long)(i / es);
  return -1;
}

// arrivals of an exchange by destination entry, each entry's slots in neighbour-list order (slots ascend with the neighbour):
// destination j = dst[j] receives the slots uslot[uptr[j] .. uptr[j + 1])
struct HaloArrivals { std::vector<uint32_t> dst, uptr, uslot; };
inline HaloArrivals halo_arrivals(const std::vector<uint32_t> &idx) {
  HaloArrivals A;
  std::vector<uint32_t> order(idx.size());
  for (size_t i = 0; i < order.size(); i++) order[i] = (uint32_t)i;
  std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return idx[a] < idx[b]; });
  std::vector<uint32_t> &dst = A.dst, &uptr = A.uptr, &uslot = A.uslot;
  uptr.assign(1, 0u);
  for (size_t i = 0; i < order.size(); i++) {
    if (i == 0 || idx[order[i]] != idx[order[i - 1]]) { if (i) uptr.push_back((uint32_t)uslot.size()); dst.push_back(idx[order[i]]); }
    uslot.push_back(order[i]);
  }
  uptr.push_back((uint32_t)uslot.size());
  if (dst.empty()) uptr.assign(1, 0u);
  return A;
}

}  // namespace cps
