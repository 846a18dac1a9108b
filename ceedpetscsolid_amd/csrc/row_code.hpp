// row_code.hpp -- the stencil code of a transpose map (set-up time, host; plain C++ over std::vector: no HIP, no Ceed types, so that
// tests/row_code_host.cpp builds it alone under the sanitizers).
//
// The contributors of a row are E-vector positions in element order.  On a mesh almost every row repeats one of a few patterns: the
// tuple (contributor count, distances of the contributors from the first one) takes 17 values over the 357 720 shell rows of a
// 10 x 110 x 8 hollow cylinder at degree 4 (tools/assemble_line_model.py).  So a row is coded as {pos0, sid}: the first contributor's position
// and the index of its pattern in a table of stencils -- 6 bytes in place of rowptr (4) and cols (4 per contributor), and one load
// before the E-vector instead of two dependent ones.  node_sum3_coded (kernel_node_sum.hpp) reads it.
//
// A row whose pattern the table cannot hold gets the ESCAPE id and stays with rowptr / cols: more than ROWCODE_MAXC contributors, a
// contributor before the first one (only a map that is not in ascending order has one), or a pattern beyond the table limit.
#pragma once
#include <stdint.h>

#include <cstddef>
#include <map>
#include <vector>

namespace cps {

constexpr int ROWCODE_MAXC = 8;                  // contributors of a coded row (a vertex of a hex mesh has eight)
constexpr uint16_t ROWCODE_ESCAPE = 0xFFFFu;
constexpr int ROWCODE_MAX_DEFAULT = 4096;        // stencils a table holds unless the caller says otherwise (at most 0xFFFF)

// contributor j of a coded row sits at pos0 + (j ? dist[j - 1] : 0).  The entries from `count` - 1 on REPEAT the last distance (0 for
// a single contributor), so that a reader may load ROWCODE_MAXC positions unconditionally and discard the ones past the count.
struct RowStencil {
  uint32_t count;
  uint32_t dist[ROWCODE_MAXC - 1];
};
static_assert(sizeof(RowStencil) == 32, "the kernels read a stencil as two 16-byte halves");

struct RowCode {
  std::vector<uint32_t> pos0;      // per row (0 for an escape row)
  std::vector<uint16_t> sid;       // per row: index into `table`, or ROWCODE_ESCAPE
  std::vector<RowStencil> table;
  size_t nescape = 0;
};

inline RowCode row_code_encode(const std::vector<uint32_t> &rowptr, const std::vector<uint32_t> &cols, int max_stencils = ROWCODE_MAX_DEFAULT) {
  RowCode c;
  const size_t nrows = rowptr.empty() ? 0 : rowptr.size() - 1;
  const size_t limit = (size_t)(max_stencils < 0 ? 0 : (max_stencils > (int)ROWCODE_ESCAPE ? (int)ROWCODE_ESCAPE : max_stencils));
  c.pos0.assign(nrows, 0u);
  c.sid.assign(nrows, ROWCODE_ESCAPE);
  std::map<std::vector<uint32_t>, uint16_t> ids;     // pattern {count, distances} -> id
  std::vector<uint32_t> key;
  for (size_t r = 0; r < nrows; r++) {
    const uint32_t k0 = rowptr[r], k1 = rowptr[r + 1];
    bool ok = k1 >= k0 && k1 - k0 <= (uint32_t)ROWCODE_MAXC;
    key.assign(1, ok ? k1 - k0 : 0u);
    for (uint32_t k = k0 + 1; ok && k < k1; k++) {
      if (cols[k] < cols[k0]) ok = false;            // (a distance is unsigned)
      else key.push_back(cols[k] - cols[k0]);
    }
    if (ok) {
      auto it = ids.find(key);
      if (it == ids.end()) {
        if (c.table.size() >= limit) ok = false;
        else {
          RowStencil s{};
          s.count = key[0];
          for (int j = 0; j < ROWCODE_MAXC - 1; j++)
            s.dist[j] = (size_t)j + 1 < key.size() ? key[(size_t)j + 1] : (key.size() > 1 ? key.back() : 0u);
          it = ids.emplace(key, (uint16_t)c.table.size()).first;
          c.table.push_back(s);
        }
      }
      if (ok) { c.sid[r] = it->second; c.pos0[r] = k1 > k0 ? cols[k0] : 0u; }
    }
    if (!ok) c.nescape++;
  }
  return c;
}

// The map a code stands for: the coded rows from {pos0, sid, table} alone, the escape rows copied from (rowptr, cols).  False if the
// code is not one of a map with these row pointers (a stencil id outside the table, a row count that differs).
inline bool row_code_decode(const RowCode &c, const std::vector<uint32_t> &rowptr, const std::vector<uint32_t> &cols,
                            std::vector<uint32_t> &rowptr_out, std::vector<uint32_t> &cols_out) {
  const size_t nrows = rowptr.empty() ? 0 : rowptr.size() - 1;
  rowptr_out.assign(1, 0u);
  cols_out.clear();
  if (c.pos0.size() != nrows || c.sid.size() != nrows) return false;
  for (size_t r = 0; r < nrows; r++) {
    if (c.sid[r] == ROWCODE_ESCAPE) {
      for (uint32_t k = rowptr[r]; k < rowptr[r + 1]; k++) cols_out.push_back(cols[k]);
    } else {
      if ((size_t)c.sid[r] >= c.table.size()) return false;
      const RowStencil &s = c.table[c.sid[r]];
      if (s.count > (uint32_t)ROWCODE_MAXC) return false;
      for (uint32_t j = 0; j < s.count; j++) cols_out.push_back(c.pos0[r] + (j ? s.dist[j - 1] : 0u));
    }
    rowptr_out.push_back((uint32_t)cols_out.size());
  }
  return true;
}

}  // namespace cps
