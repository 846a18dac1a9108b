// index_maps_host.cpp -- the index arithmetic of set-up (csrc/index_maps.hpp) on the host alone: built by test_index_maps.py with g++ under
// the address and undefined-behaviour sanitizers and run as a child process.  The inputs are made here: boxes of 1, 2 and 3 elements per
// side at P = 2, 3, 5 (three interlaced components, nodes numbered lexicographically over the box), a 6 x 6 x 6 box at P = 3 for the
// pipelined map.  What is asserted are properties of the results, not the algorithms again:
//   transpose map (whole, shell, with priority rows), interior nodes, segment count and boundaries (two full-size shapes by arithmetic),
//   the pipelined re-ordering, the Dirichlet flags, the owner map, the pack fold and the arrival lists of a halo, empty inputs;
//   the flags, row flags, owner map and folded rows once more under component-wise masks of all eight node patterns, entry by entry.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "index_maps.hpp"
#include "row_code.hpp"

using namespace cps;

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (g_fail++ < 40) { fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } } while (0)

struct Box {
  int n, P, N, nelem, P3, nnodes, lsize;
  std::vector<int> off;      // [elem][P^3] component-0 offsets: 3 x node
  int node(int ix, int iy, int iz) const { return (iz * N + iy) * N + ix; }
};
// `fold`: one element thick in x, its node layers i and P - 1 - i identified (the two x-faces share their nodes, and at P = 5 the
// interior layers 1 and 3 do too: an interior node repeats inside its element)
static Box make_box(int nx, int n, int P, bool fold = false) {
  Box b;
  b.n = n; b.P = P; b.N = n * (P - 1) + 1; b.P3 = P * P * P; b.nelem = nx * n * n; b.nnodes = b.N * b.N * b.N; b.lsize = 3 * b.nnodes;
  b.off.resize((size_t)b.nelem * b.P3);
  for (int ez = 0, e = 0; ez < n; ez++)
    for (int ey = 0; ey < n; ey++)
      for (int ex = 0; ex < nx; ex++, e++)
        for (int k = 0, l = 0; k < P; k++)
          for (int j = 0; j < P; j++)
            for (int i = 0; i < P; i++, l++) {
              int ix = ex * (P - 1) + i;
              if (fold && ix > (P - 1) / 2) ix = P - 1 - ix;
              b.off[(size_t)e * b.P3 + l] = 3 * b.node(ix, ey * (P - 1) + j, ez * (P - 1) + k);
            }
  return b;
}
static unsigned lcg(unsigned &s) { s = s * 1664525u + 1013904223u; return s >> 16; }

// rows are distinct node offsets; every E-vector position that is not skipped sits in exactly one row, its node's; contributors ascend
static void check_transpose(const char *what, const Box &b, const TransposeMap &M, int skipP, const int lsize) {
  const int per = skipP ? element_shell_size(skipP) : b.P3;
  const size_t nrows = M.node_off.size();
  CHECK(M.rowptr.size() == nrows + 1 && M.rowptr[0] == 0, "%s: %zu row pointers for %zu rows", what, M.rowptr.size(), nrows);
  std::vector<int> row_of((size_t)lsize, -1);
  for (size_t r = 0; r < nrows; r++) {
    CHECK(M.node_off[r] < (uint32_t)lsize && row_of[M.node_off[r]] < 0, "%s: row %zu repeats node offset %u", what, r, M.node_off[r]);
    row_of[M.node_off[r]] = (int)r;
    CHECK(M.rowptr[r + 1] > M.rowptr[r], "%s: row %zu has no contributor", what, r);
    for (uint32_t k = M.rowptr[r] + 1; k < M.rowptr[r + 1]; k++)
      CHECK(M.cols[k] / per > M.cols[k - 1] / per, "%s: row %zu: contributors %u, %u do not ascend by element", what, r, M.cols[k - 1], M.cols[k]);
  }
  std::vector<int> row_at((size_t)b.nelem * per, -1);
  for (size_t r = 0; r < nrows; r++)
    for (uint32_t k = M.rowptr[r]; k < M.rowptr[r + 1]; k++) {
      CHECK(M.cols[k] < row_at.size() && row_at[M.cols[k]] < 0, "%s: E-vector position %u occurs twice", what, M.cols[k]);
      if (M.cols[k] < row_at.size()) row_at[M.cols[k]] = (int)r;
    }
  size_t nskipped = 0;
  for (size_t i = 0; i < b.off.size(); i++) {
    const int l = (int)(i % b.P3);
    if (skipP && node_is_element_interior(l, skipP)) { nskipped++; continue; }
    const size_t pos = skipP ? (i / b.P3) * per + node_shell_rank(l, skipP) : i;
    CHECK(row_at[pos] >= 0 && row_at[pos] == row_of[b.off[i]], "%s: position %zu of node %d is in row %d, the node's row is %d", what, pos, b.off[i], row_at[pos], row_of[b.off[i]]);
  }
  CHECK(M.rowptr[nrows] == b.off.size() - nskipped, "%s: %u contributors for %zu positions", what, M.rowptr[nrows], b.off.size() - nskipped);
  CHECK((size_t)M.nskipped == nskipped && nskipped == (skipP ? (size_t)b.nelem * (b.P - 2) * (b.P - 2) * (b.P - 2) : 0), "%s: %d nodes skipped", what, M.nskipped);
}

static void test_box(int n, int P) {
  char what[96];
  const Box b = make_box(n, n, P);
  for (int shell = 0; shell < 2; shell++) {
    if (shell && P < 3) continue;
    const int skipP = shell ? P : 0;
    snprintf(what, sizeof what, "box %d^3 P=%d %s", n, P, shell ? "shell" : "whole");
    const TransposeMap M = transpose_map(b.off, b.lsize, b.P3, 3, nullptr, skipP);
    check_transpose(what, b, M, skipP, b.lsize);
    CHECK(M.full_cover && M.nprio == 0, "%s: full_cover %d, nprio %d", what, (int)M.full_cover, M.nprio);
    for (size_t r = 1; r < M.node_off.size(); r++) CHECK(M.node_off[r] > M.node_off[r - 1], "%s: rows not in ascending offset order at %zu", what, r);
    const TransposeMap U = transpose_map(b.off, b.lsize + 3, b.P3, 3, nullptr, skipP);      // three entries no element holds
    check_transpose(what, b, U, skipP, b.lsize + 3);
    CHECK(!U.full_cover && U.node_off == M.node_off && U.cols == M.cols, "%s with unused entries: full_cover %d", what, (int)U.full_cover);
    // priority rows: the face x = 0
    std::vector<unsigned char> prio((size_t)b.lsize, 0);
    size_t nflag = 0;
    for (int iz = 0; iz < b.N; iz++)
      for (int iy = 0; iy < b.N; iy++) { prio[(size_t)3 * b.node(0, iy, iz)] = 1; nflag++; }
    const TransposeMap Q = transpose_map(b.off, b.lsize, b.P3, 3, prio.data(), skipP);
    check_transpose(what, b, Q, skipP, b.lsize);
    CHECK((size_t)Q.nprio == nflag && Q.full_cover && Q.node_off.size() == M.node_off.size(), "%s: %d priority rows for %zu flagged nodes", what, Q.nprio, nflag);
    for (size_t r = 0; r < Q.node_off.size(); r++) {
      CHECK((prio[Q.node_off[r]] != 0) == (r < (size_t)Q.nprio), "%s: row %zu (node %u) on the wrong side of nprio = %d", what, r, Q.node_off[r], Q.nprio);
      if (r && r != (size_t)Q.nprio) CHECK(Q.node_off[r] > Q.node_off[r - 1], "%s: priority map not ascending within its parts at %zu", what, r);
    }
    // the contract of an overlap split, on the face z = 0: its only contributors are the first n x n elements
    std::vector<unsigned char> pz((size_t)b.lsize, 0);
    for (int iy = 0; iy < b.N; iy++)
      for (int ix = 0; ix < b.N; ix++) pz[(size_t)3 * b.node(ix, iy, 0)] = 1;
    CHECK(overlap_split_violation(b.off, b.P3, pz.data(), n * n) == -1, "%s: the leading layer breaks the contract", what);
    CHECK(overlap_split_violation(b.off, b.P3, pz.data(), n * n - 1) == n * n - 1, "%s: element %d not named", what, n * n - 1);
  }
  snprintf(what, sizeof what, "box %d^3 P=%d", n, P);
  // interior nodes
  CHECK(interior_nodes_private(b.off, b.lsize, b.P3, 3, 1, P) == (P >= 3), "%s: interior nodes private?", what);
  if (P >= 3) {
    const int m = (P - 2) * (P - 2) * (P - 2);
    const std::vector<uint32_t> lst = interior_node_list(b.off, b.P3, P);
    CHECK(lst.size() == (size_t)b.nelem * m, "%s: %zu interior nodes listed", what, lst.size());
    std::vector<unsigned char> seen((size_t)b.lsize, 0);
    size_t q = 0;
    for (int e = 0; e < b.nelem; e++)
      for (int k = 1; k < P - 1; k++)
        for (int j = 1; j < P - 1; j++)
          for (int i = 1; i < P - 1; i++, q++) {
            if (q >= lst.size()) continue;
            CHECK(lst[q] == (uint32_t)b.off[(size_t)e * b.P3 + (k * P + j) * P + i], "%s: interior list entry %zu is %u", what, q, lst[q]);
            CHECK(!seen[lst[q]], "%s: interior node %u listed twice", what, lst[q]);
            seen[lst[q]] = 1;
          }
    const Box f = make_box(1, n, P, true);      // one element thick in x, folded
    CHECK(interior_nodes_private(f.off, f.lsize, f.P3, 3, 1, P) == (P < 5), "%s folded in x: interior nodes private?", what);
  }
  // flags
  unsigned seed = 12345u + (unsigned)(n * 16 + P);
  std::vector<unsigned char> mask((size_t)b.lsize);
  for (auto &m : mask) m = (unsigned char)(lcg(seed) % 3 == 0 ? 1 + lcg(seed) % 200 : 0);
  const std::vector<uint32_t> fo = flagged_offsets(b.off, mask.data(), 3, 1);
  CHECK(fo.size() == b.off.size(), "%s: %zu flagged offsets", what, fo.size());
  for (size_t i = 0; i < fo.size() && i < b.off.size(); i++) {
    const uint32_t o = (uint32_t)b.off[i], bits = (mask[o] ? 1u : 0u) | (mask[o + 1] ? 2u : 0u) | (mask[o + 2] ? 4u : 0u);
    CHECK(node_flag_bits(mask.data(), o, 3, 1) == bits, "%s: flag bits of node %u", what, o);
    CHECK((fo[i] & OFF_MASK) == o && (fo[i] >> OFF_FLAG_SHIFT) == bits, "%s: flagged offset %zu is %08x", what, i, fo[i]);
  }
  CHECK(node_flag_bits(mask.data(), 0, 1, 1) == (mask[0] ? 1u : 0u), "%s: one component", what);
  CHECK(node_flag_bits(mask.data(), 0, 3, b.nnodes) == ((mask[0] ? 1u : 0u) | (mask[(size_t)b.nnodes] ? 2u : 0u) | (mask[(size_t)2 * b.nnodes] ? 4u : 0u)), "%s: component stride", what);
  const TransposeMap M = transpose_map(b.off, b.lsize, b.P3, 3, nullptr, 0);
  const std::vector<unsigned char> rf = row_flag_bits(M.node_off, mask.data(), 3, 1);
  CHECK(rf.size() == M.node_off.size(), "%s: %zu row flags", what, rf.size());
  for (size_t r = 0; r < rf.size(); r++) CHECK(rf[r] == node_flag_bits(mask.data(), M.node_off[r], 3, 1), "%s: row flag %zu", what, r);
  // owner map: with a mask, without one, with unused entries
  for (int variant = 0; variant < 3; variant++) {
    bool cover = false;
    const unsigned char *mk = variant == 0 ? mask.data() : nullptr;
    std::vector<unsigned char> longer;
    if (variant == 2) { longer = mask; longer.resize(mask.size() + 3, 1); mk = longer.data(); }
    const std::vector<uint32_t> own = owner_map(b.off, b.lsize + (variant == 2 ? 3 : 0), mk, 3, 1, &cover);
    CHECK(own.size() == b.off.size() && cover == (variant != 2), "%s: owner map variant %d: cover %d", what, variant, (int)cover);
    std::vector<int> first((size_t)b.lsize, -1);
    for (size_t i = 0; i < b.off.size(); i++) if (first[b.off[i]] < 0) first[b.off[i]] = (int)i;
    for (size_t i = 0; i < own.size() && i < b.off.size(); i++) {
      const uint32_t o = (uint32_t)b.off[i];
      if (first[o] != (int)i) CHECK(own[i] == 0xFFFFFFFFu, "%s: entry %zu of node %u is owned twice", what, i, o);
      else CHECK((own[i] & OFF_MASK) == o && (own[i] >> OFF_FLAG_SHIFT) == (mk ? node_flag_bits(mk, o, 3, 1) : 0u), "%s: owner entry %zu is %08x", what, i, own[i]);
    }
  }
}

// a halo of the dofs of the face x = max to one neighbour and of the face y = max to another: the shared edge goes to both
static void test_halo(int n, int P) {
  char what[96];
  snprintf(what, sizeof what, "halo of box %d^3 P=%d", n, P);
  const Box b = make_box(n, n, P);
  std::vector<uint32_t> idx;
  std::vector<unsigned char> prio((size_t)b.lsize + 3, 0);
  for (int nb = 0; nb < 2; nb++)
    for (int s = 0; s < b.N; s++)
      for (int t = 0; t < b.N; t++)
        for (int c = 0; c < 3; c++) {
          const int node = nb == 0 ? b.node(b.N - 1, t, s) : b.node(t, b.N - 1, s);
          idx.push_back((uint32_t)(3 * node + c)); prio[(size_t)3 * node] = 1;
        }
  const size_t total = idx.size();
  const TransposeMap M = transpose_map(b.off, b.lsize + 3, b.P3, 3, prio.data(), P >= 3 ? P : 0);
  const PackFoldLists F = pack_fold(M.node_off, idx, 3, 1);
  CHECK(F.ok && F.ptr.size() == M.node_off.size() + 1 && F.ptr.back() == total, "%s: fold ok %d, %u slots of %zu", what, (int)F.ok, F.ptr.empty() ? 0u : F.ptr.back(), total);
  if (F.ok && F.ptr.size() == M.node_off.size() + 1) {
    std::vector<int> hits(total, 0);
    for (size_t r = 0; r < M.node_off.size(); r++)
      for (uint32_t k = F.ptr[r]; k < F.ptr[r + 1]; k++) {
        const uint32_t e = F.slot[k] & 0x3FFFFFFFu, comp = F.slot[k] >> 30;
        CHECK(e < total, "%s: slot %u names entry %u", what, k, e);
        if (e >= total) continue;
        hits[e]++;
        CHECK(halo_entry_node(idx[e]) == M.node_off[r] && comp == idx[e] % 3, "%s: entry %u (dof %u) folded into the row of node %u as component %u", what, e, idx[e], M.node_off[r], comp);
      }
    for (size_t e = 0; e < total; e++) CHECK(hits[e] == 1, "%s: entry %zu folded %d times", what, e, hits[e]);
  }
  CHECK(halo_entry_off_priority(M.node_off, M.nprio, idx) == -1, "%s: an entry off the priority rows", what);
  CHECK(!pack_fold(M.node_off, idx, 1, 1).ok && !pack_fold(M.node_off, idx, 3, 2).ok, "%s: folded without three interlaced components", what);
  {  // an entry whose node no element holds; an entry on a row that is no priority row
    std::vector<uint32_t> bad = idx;
    bad.insert(bad.begin() + 5, (uint32_t)b.lsize + 1);
    CHECK(!pack_fold(M.node_off, bad, 3, 1).ok, "%s: folded with an entry that is no row", what);
    CHECK(halo_entry_off_priority(M.node_off, M.nprio, bad) == 5, "%s: the entry that is no row is not named", what);
    bad = idx;
    bad.push_back((uint32_t)(3 * b.node(0, 0, 0) + 2));
    CHECK(pack_fold(M.node_off, bad, 3, 1).ok, "%s: an entry on an ordinary row does not fold", what);
    CHECK(halo_entry_off_priority(M.node_off, M.nprio, bad) == (long)total, "%s: the entry off the priority rows is not named", what);
  }
  const HaloArrivals A = halo_arrivals(idx);
  CHECK(A.uptr.size() == A.dst.size() + 1 && A.uptr[0] == 0 && A.uptr.back() == total && A.uslot.size() == total, "%s: arrival lists of %zu / %zu / %zu", what, A.dst.size(), A.uptr.size(), A.uslot.size());
  CHECK(A.dst.size() == total - (size_t)3 * b.N, "%s: %zu destinations", what, A.dst.size());
  std::vector<int> hits(total, 0);
  for (size_t j = 0; j + 1 < A.uptr.size() && j < A.dst.size(); j++) {
    if (j) CHECK(A.dst[j] > A.dst[j - 1], "%s: destinations %zu not ascending", what, j);
    CHECK(A.uptr[j + 1] > A.uptr[j], "%s: destination %zu without a slot", what, j);
    for (uint32_t k = A.uptr[j]; k < A.uptr[j + 1] && k < A.uslot.size(); k++) {
      CHECK(A.uslot[k] < total && idx[A.uslot[k]] == A.dst[j], "%s: slot %u does not arrive at %u", what, A.uslot[k], A.dst[j]);
      if (A.uslot[k] < total) hits[A.uslot[k]]++;
      if (k > A.uptr[j]) CHECK(A.uslot[k] > A.uslot[k - 1], "%s: slots of destination %u not in neighbour order", what, A.dst[j]);
    }
  }
  for (size_t e = 0; e < total; e++) CHECK(hits[e] == 1, "%s: slot %zu arrives %d times", what, e, hits[e]);
  // an empty halo
  const std::vector<uint32_t> none;
  const HaloArrivals E = halo_arrivals(none);
  CHECK(E.dst.empty() && E.uslot.empty() && E.uptr == std::vector<uint32_t>(1, 0u), "%s: arrivals of an empty halo", what);
  const PackFoldLists F0 = pack_fold(M.node_off, none, 3, 1);
  CHECK(F0.ok && F0.ptr == std::vector<uint32_t>(M.node_off.size() + 1, 0u), "%s: fold of an empty halo", what);
  CHECK(halo_entry_off_priority(M.node_off, M.nprio, none) == -1, "%s: empty halo off the priority rows", what);
}

// Component-wise masks: node k carries the pattern (k + shift) % 8, bit c = component c masked, so every one of the eight patterns
// occurs (asserted).  Every builder that folds mask bytes into flag bits against a loop over the L-vector ENTRIES: one byte, one bit.
static int test_patterns(int n, int P, int shift) {
  char what[96];
  snprintf(what, sizeof what, "patterns on box %d^3 P=%d shift %d", n, P, shift);
  const Box b = make_box(n, n, P);
  std::vector<unsigned char> mask((size_t)b.lsize, 0);
  int seen = 0;
  for (int k = 0; k < b.nnodes; k++) {
    const int pat = (k + shift) % 8;
    seen |= 1 << pat;
    for (int c = 0; c < 3; c++) mask[(size_t)3 * k + c] = (unsigned char)((pat >> c) & 1 ? 1 + 37 * c : 0);     // any non-zero byte masks
  }
  CHECK(seen == 0xFF, "%s: patterns %02x only", what, seen);
  const std::vector<uint32_t> fo = flagged_offsets(b.off, mask.data(), 3, 1);
  CHECK(fo.size() == b.off.size(), "%s: %zu flagged offsets", what, fo.size());
  for (size_t i = 0; i < fo.size() && i < b.off.size(); i++) {
    CHECK((fo[i] & OFF_MASK) == (uint32_t)b.off[i], "%s: flagged offset %zu lost its offset", what, i);
    for (int c = 0; c < 3; c++)
      CHECK(((fo[i] >> (OFF_FLAG_SHIFT + c)) & 1u) == (mask[(size_t)b.off[i] + c] ? 1u : 0u), "%s: flagged offset %zu, component %d", what, i, c);
  }
  for (int shell = 0; shell < 2; shell++) {
    if (shell && P < 3) continue;
    const TransposeMap M = transpose_map(b.off, b.lsize, b.P3, 3, nullptr, shell ? P : 0);
    const std::vector<unsigned char> rf = row_flag_bits(M.node_off, mask.data(), 3, 1);
    CHECK(rf.size() == M.node_off.size(), "%s: %zu row flags", what, rf.size());
    int rows_seen = 0;
    for (size_t r = 0; r < rf.size(); r++) {
      rows_seen |= 1 << (rf[r] & 7);
      for (int c = 0; c < 3; c++)
        CHECK(((rf[r] >> c) & 1) == (mask[(size_t)M.node_off[r] + c] ? 1 : 0), "%s: row %zu (%s map), component %d", what, r, shell ? "shell" : "whole", c);
      CHECK((rf[r] >> 3) == 0, "%s: row flag %zu is %02x", what, r, rf[r]);
    }
    CHECK(rows_seen == 0xFF, "%s: the %s map's rows carry the patterns %02x only", what, shell ? "shell" : "whole", rows_seen);
  }
  bool cover = false;
  const std::vector<uint32_t> own = owner_map(b.off, b.lsize, mask.data(), 3, 1, &cover);
  CHECK(own.size() == b.off.size() && cover, "%s: owner map", what);
  std::vector<int> owners((size_t)b.lsize, 0);
  for (size_t i = 0; i < own.size() && i < b.off.size(); i++) {
    if (own[i] == 0xFFFFFFFFu) continue;
    const uint32_t o = own[i] & OFF_MASK;
    CHECK(o == (uint32_t)b.off[i], "%s: owner entry %zu names node %u", what, i, o);
    if (o >= (uint32_t)b.lsize) continue;
    owners[o]++;
    for (int c = 0; c < 3; c++)
      CHECK(((own[i] >> (OFF_FLAG_SHIFT + c)) & 1u) == (mask[(size_t)o + c] ? 1u : 0u), "%s: owner entry %zu, component %d", what, i, c);
  }
  for (int k = 0; k < b.nnodes; k++) CHECK(owners[(size_t)3 * k] == 1, "%s: node %d has %d owners", what, k, owners[(size_t)3 * k]);
  // the pack fold of the face x = max: the send buffer's entry e takes component comp of its row, and that row's flag bit comp is the
  // mask byte of the entry itself -- what the folded pack drops is what the mask names, entry by entry
  std::vector<uint32_t> idx;
  std::vector<unsigned char> prio((size_t)b.lsize, 0);
  for (int s = 0; s < b.N; s++)
    for (int t = 0; t < b.N; t++) {
      const int node = b.node(b.N - 1, t, s);
      prio[(size_t)3 * node] = 1;
      for (int c = 2; c >= 0; c--) idx.push_back((uint32_t)(3 * node + c));        // components in descending order: no order is assumed
    }
  const TransposeMap M = transpose_map(b.off, b.lsize, b.P3, 3, prio.data(), P >= 3 ? P : 0);
  const std::vector<unsigned char> rf = row_flag_bits(M.node_off, mask.data(), 3, 1);
  const PackFoldLists F = pack_fold(M.node_off, idx, 3, 1);
  CHECK(F.ok && F.ptr.size() == M.node_off.size() + 1 && F.ptr.back() == idx.size(), "%s: fold", what);
  int folded_seen = 0;
  std::vector<int> hits(idx.size(), 0);
  if (F.ok && F.ptr.size() == M.node_off.size() + 1 && rf.size() == M.node_off.size())
    for (size_t r = 0; r < M.node_off.size(); r++) {
      if (F.ptr[r + 1] > F.ptr[r]) folded_seen |= 1 << (rf[r] & 7);
      for (uint32_t k = F.ptr[r]; k < F.ptr[r + 1]; k++) {
        const uint32_t e = F.slot[k] & 0x3FFFFFFFu, comp = F.slot[k] >> 30;
        CHECK(e < idx.size() && comp < 3, "%s: slot %u is %08x", what, k, F.slot[k]);
        if (e >= idx.size() || comp >= 3) continue;
        hits[e]++;
        CHECK(M.node_off[r] + comp == idx[e], "%s: entry %u (dof %u) folded into row %zu as component %u", what, e, idx[e], r, comp);
        CHECK(((rf[r] >> comp) & 1) == (mask[idx[e]] ? 1 : 0), "%s: entry %u (dof %u): row flag %02x, mask byte %d", what, e, idx[e], rf[r], (int)mask[idx[e]]);
      }
    }
  for (size_t e = 0; e < idx.size(); e++) CHECK(hits[e] == 1, "%s: entry %zu folded %d times", what, e, hits[e]);
  return folded_seen;
}

static bool increasing(const std::vector<int> &v) {
  for (size_t i = 1; i < v.size(); i++) if (v[i] <= v[i - 1]) return false;
  return true;
}
static void test_segments() {
  // the 6 x 6 x 6 box in groups of E = 4 on two waves: 54 groups
  CHECK(pipe_segment_count(216, 4, 26, 3, 3, 160, 4, 20) == 1, "a launch below min_total_rounds x waves groups is pipelined");
  CHECK(pipe_segment_count(216, 4, 26, 3, 2, 160, 4, 20) == 3, "54 groups on 2 waves, 3 segments asked for");
  CHECK(pipe_segment_count(216, 4, 26, 16, 2, 160, 4, 20) == 6, "54 groups on 2 waves: at most six segments of 4 rounds");
  const Box b = make_box(6, 6, 3);
  for (int shell = 0; shell < 2; shell++) {
    const int per = shell ? element_shell_size(3) : 27;
    const TransposeMap M = transpose_map(b.off, b.lsize, b.P3, 3, nullptr, shell ? 3 : 0);
    std::vector<int> base_row((size_t)b.lsize, -1);
    for (size_t r = 0; r < M.node_off.size(); r++) base_row[M.node_off[r]] = (int)r;
    for (int req = 2; req <= 4; req++) {
      char what[96];
      snprintf(what, sizeof what, "box 6^3 P=3 %s, %d segments", shell ? "shell" : "whole", req);
      const int nseg = pipe_segment_count(216, 4, per, req, 2, 160, 0, 20);
      CHECK(nseg == req, "%s: %d segments with min_rounds = 0", what, nseg);
      const std::vector<int> eb = pipe_elem_bound(216, 4, nseg, 2, 0);
      CHECK(eb.size() == (size_t)nseg + 1 && eb.front() == 0 && eb.back() == 216 && increasing(eb), "%s: %zu boundaries", what, eb.size());
      const PipeRows G = pipe_reorder(M.node_off, M.rowptr, M.cols, eb, per);
      const size_t nrows = M.node_off.size();
      CHECK(G.row_bound.size() == eb.size() && G.row_bound.front() == 0 && G.row_bound.back() == (int)nrows, "%s: row_bound does not span the rows", what);
      CHECK(G.node_off.size() == nrows && G.rowptr.size() == nrows + 1 && G.cols.size() == M.cols.size() && G.rowptr[0] == 0, "%s: sizes", what);
      if (G.row_bound.size() != eb.size() || G.node_off.size() != nrows || G.rowptr.size() != nrows + 1) continue;
      std::vector<unsigned char> seen(nrows, 0);
      for (size_t k = 0; k + 1 < eb.size(); k++) {
        CHECK(G.row_bound[k + 1] >= G.row_bound[k], "%s: row_bound descends", what);
        int before = -1;
        for (int j = G.row_bound[k]; j < G.row_bound[k + 1]; j++) {
          const int i = base_row[G.node_off[j]];
          CHECK(i >= 0 && !seen[i], "%s: row %d (node %u) is no row of the base map, or twice", what, j, G.node_off[j]);
          if (i < 0) continue;
          seen[i] = 1;
          CHECK(i > before, "%s: segment %zu does not keep the base map's order at row %d", what, k, j);
          before = i;
          const uint32_t len = M.rowptr[i + 1] - M.rowptr[i];
          CHECK(G.rowptr[j + 1] - G.rowptr[j] == len, "%s: row %d has %u contributors, the base row %u", what, j, G.rowptr[j + 1] - G.rowptr[j], len);
          if (G.rowptr[j + 1] - G.rowptr[j] != len) continue;
          for (uint32_t q = 0; q < len; q++) {
            const uint32_t col = G.cols[G.rowptr[j] + q];
            CHECK(col == M.cols[M.rowptr[i] + q], "%s: row %d, contributor %u differs from the base map's", what, j, q);
            CHECK((int)(col / per) < eb[k + 1], "%s: row %d of segment %zu has a contributor in element %u", what, j, k, col / per);
            if (q == len - 1) CHECK((int)(col / per) >= eb[k], "%s: the last contributor of row %d lies before segment %zu", what, j, k);
          }
        }
      }
      for (size_t i = 0; i < nrows; i++) CHECK(seen[i], "%s: base row %zu is in no segment", what, i);
      const RowCode c = row_code_encode(G.rowptr, G.cols);
      std::vector<uint32_t> rp, cl;
      CHECK(row_code_decode(c, G.rowptr, G.cols, rp, cl) && rp == G.rowptr && cl == G.cols && c.nescape == 0, "%s: the stencil code does not give the map back", what);
    }
  }
  // boundaries that coincide collapse: two groups cannot be cut in four
  const std::vector<int> few = pipe_elem_bound(8, 4, 4, 2, 0);
  CHECK(few == std::vector<int>({0, 4, 8}), "two groups in four segments: %zu boundaries", few.size());
  CHECK(increasing(pipe_elem_bound(216, 4, 6, 2, 4)) && increasing(pipe_elem_bound(216, 4, 5, 8, 4)), "boundaries in whole rounds do not increase");
  // Two full-size shapes, by arithmetic.  Config 4: 99 000 elements in groups of 2, 98 shell records, 256 x 8 waves, 160 MB per segment, limits 20 / 4:
  // 49 500 groups are 24 whole rounds; 228 MB of E-vector make 2 segments; the last is 4 rounds x 2048 waves x 2 = 16 384 elements.
  CHECK(pipe_segment_count(99000, 2, 98, 0, 2048, 160, 4, 20) == 2, "config 4: %d segments", pipe_segment_count(99000, 2, 98, 0, 2048, 160, 4, 20));
  CHECK(pipe_elem_bound(99000, 2, 2, 2048, 4) == std::vector<int>({0, 82616, 99000}), "config 4: boundaries");
  // The whole of config 5: 262 144 elements one by one, 218 shell records, 256 x 6 waves: 170 rounds, 1.37 GB make 9 segments; the last is 4 rounds =
  // 6 144 elements, each middle one (170 - 4) / 8 = 20 rounds = 30 720 elements, the first takes the rest, 40 960.
  CHECK(pipe_segment_count(262144, 1, 218, 0, 1536, 160, 4, 20) == 9, "config 5: %d segments", pipe_segment_count(262144, 1, 218, 0, 1536, 160, 4, 20));
  const std::vector<int> b5 = pipe_elem_bound(262144, 1, 9, 1536, 4);
  CHECK(b5.size() == 10 && b5[0] == 0 && b5[1] == 40960 && b5[9] == 262144 && b5[8] == 262144 - 6144, "config 5: boundaries");
  for (size_t k = 2; k < b5.size() && k <= 8; k++) CHECK(b5[k] - b5[k - 1] == 30720, "config 5: segment %zu has %d elements", k - 1, b5[k] - b5[k - 1]);
}

int main() {
  for (int n = 1; n <= 3; n++)
    for (int P : {2, 3, 5}) { test_box(n, P); test_halo(n, P); }
  test_segments();
  for (int n = 1; n <= 3; n++)
    for (int P : {2, 3, 5})
      for (int shift : {0, 5}) {
        const int folded = test_patterns(n, P, shift);
        const int N = n * (P - 1) + 1;
        if (N % 2) CHECK(folded == 0xFF, "box %d^3 P=%d: the folded rows carry the patterns %02x only", n, P, folded);    // N odd: the face's node numbers run through every residue mod 8
      }
  if (!g_fail) printf("component patterns ok\n");
  if (g_fail) { fprintf(stderr, "FAIL: %d checks\n", g_fail); return 1; }
  printf("index_maps_host ok\n");
  return 0;
}
