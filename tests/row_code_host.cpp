// row_code_host.cpp -- the stencil coder of the transpose maps (csrc/row_code.hpp) on the host alone: built by test_row_code.py with g++
// under the address and undefined-behaviour sanitizers and run as a child process.  Every map is encoded and decoded again; the decoded
// (rowptr, cols) must be the map itself, entry for entry.
//   boxes 2x2x2 and 3x3x3 at P = 2, 3, 5: the whole map (columns e * P^3 + n) and the shell map of the direct-store mode (interior nodes
//     left out, columns e * shell size + shell rank), both built by the library's transpose_map (csrc/index_maps.hpp);
//   a map with a 12-contributor row and one with a contributor BEFORE its row's first: escape rows;
//   an empty map; rows without contributors;
//   a table limit of 4 (coded and escape rows side by side: half the shell rows of the 3x3x3 box at P = 5 escape) and of 0 (all escape).
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "index_maps.hpp"
#include "row_code.hpp"

using namespace cps;

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { g_fail++; fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

struct Map { std::vector<uint32_t> rowptr, cols; };

// the transpose map of an n x n x n box of degree P - 1 (nodes numbered lexicographically over the box), rows in ascending node order,
// a row's contributors in element order: the offsets made here, the map by the library's own transpose_map (index_maps.hpp), with its `skipP`
static Map box_map(int n, int P, bool shell) {
  const int N = n * (P - 1) + 1, P3 = P * P * P, nelem = n * n * n;
  std::vector<int> off((size_t)nelem * P3);
  for (int ez = 0, e = 0; ez < n; ez++)
    for (int ey = 0; ey < n; ey++)
      for (int ex = 0; ex < n; ex++, e++)
        for (int k = 0, l = 0; k < P; k++)
          for (int j = 0; j < P; j++)
            for (int i = 0; i < P; i++, l++)
              off[(size_t)e * P3 + l] = ((ez * (P - 1) + k) * N + ey * (P - 1) + j) * N + ex * (P - 1) + i;
  TransposeMap T = transpose_map(off, N * N * N, P3, 1, nullptr, shell ? P : 0);
  return Map{std::move(T.rowptr), std::move(T.cols)};
}

// encode, decode, compare; returns the code for the caller's own checks
static RowCode round_trip(const char *what, const Map &M, int limit) {
  const RowCode c = row_code_encode(M.rowptr, M.cols, limit);
  const size_t nrows = M.rowptr.empty() ? 0 : M.rowptr.size() - 1;
  CHECK(c.pos0.size() == nrows && c.sid.size() == nrows, "%s: %zu rows coded as %zu / %zu", what, nrows, c.pos0.size(), c.sid.size());
  CHECK(c.table.size() <= (size_t)(limit < 0 ? 0 : limit), "%s: %zu stencils over the limit %d", what, c.table.size(), limit);
  size_t nesc = 0;
  for (size_t r = 0; r < nrows && r < c.sid.size(); r++) {
    if (c.sid[r] == ROWCODE_ESCAPE) { nesc++; continue; }
    CHECK((size_t)c.sid[r] < c.table.size(), "%s: row %zu names stencil %u of %zu", what, r, (unsigned)c.sid[r], c.table.size());
    if ((size_t)c.sid[r] >= c.table.size()) continue;
    const RowStencil &s = c.table[c.sid[r]];
    CHECK(s.count == M.rowptr[r + 1] - M.rowptr[r], "%s: row %zu has %u contributors, its stencil %u", what, r, M.rowptr[r + 1] - M.rowptr[r], s.count);
    // the padding a reader relies on: every distance past the count repeats the last one (a valid E-vector position of this row)
    for (int j = (int)s.count; j < ROWCODE_MAXC; j++)
      if (j >= 1) CHECK(s.dist[j - 1] == (s.count > 1 ? s.dist[s.count - 2] : 0u), "%s: stencil %u, distance %d is not the padding", what, (unsigned)c.sid[r], j);
  }
  CHECK(nesc == c.nescape, "%s: %zu escape rows, %zu counted", what, nesc, c.nescape);
  std::vector<uint32_t> rp, cl;
  CHECK(row_code_decode(c, M.rowptr, M.cols, rp, cl), "%s: the code does not decode", what);
  if (M.rowptr.empty()) CHECK(rp.size() == 1 && cl.empty(), "%s: an empty map decodes to something", what);
  else CHECK(rp == M.rowptr, "%s: decoded row pointers differ", what);
  CHECK(cl == M.cols, "%s: decoded columns differ (%zu against %zu)", what, cl.size(), M.cols.size());
  return c;
}

int main() {
  char what[96];
  for (int n = 2; n <= 3; n++)
    for (int P : {2, 3, 5})
      for (int shell = 0; shell < 2; shell++) {
        if (shell && P < 3) continue;
        const Map M = box_map(n, P, shell != 0);
        snprintf(what, sizeof what, "box %d^3 P=%d %s", n, P, shell ? "shell" : "whole");
        const RowCode c = round_trip(what, M, ROWCODE_MAX_DEFAULT);
        CHECK(c.nescape == 0, "%s: %zu escape rows on a hex mesh", what, c.nescape);
        CHECK(c.table.size() >= 2 && c.table.size() < c.sid.size(), "%s: %zu stencils for %zu rows", what, c.table.size(), c.sid.size());
        snprintf(what, sizeof what, "box %d^3 P=%d %s, table limit 4", n, P, shell ? "shell" : "whole");
        const RowCode c4 = round_trip(what, M, 4);
        CHECK(c4.table.size() == 4, "%s: %zu stencils", what, c4.table.size());
        if (P > 2) CHECK(c4.nescape > 0 && c4.nescape < c4.sid.size(), "%s: %zu of %zu rows escape: both kinds of row are wanted", what, c4.nescape, c4.sid.size());
        snprintf(what, sizeof what, "box %d^3 P=%d %s, table limit 0", n, P, shell ? "shell" : "whole");
        const RowCode c0 = round_trip(what, M, 0);
        CHECK(c0.nescape == c0.sid.size() && c0.table.empty(), "%s: %zu of %zu rows escape", what, c0.nescape, c0.sid.size());
      }
  {  // a row of 12 contributors between two ordinary ones; exactly 8 is still coded
    Map M;
    M.rowptr = {0, 2, 14, 22, 23};
    for (uint32_t k = 0; k < 23; k++) M.cols.push_back(7u * k + (k & 1u));
    const RowCode c = round_trip("12-contributor row", M, ROWCODE_MAX_DEFAULT);
    CHECK(c.nescape == 1 && c.sid[1] == ROWCODE_ESCAPE && c.sid[0] != ROWCODE_ESCAPE && c.sid[2] != ROWCODE_ESCAPE && c.sid[3] != ROWCODE_ESCAPE,
          "12-contributor row: %zu escapes", c.nescape);
    CHECK(c.table[c.sid[2]].count == 8, "the 8-contributor row has a stencil of %u", c.table[c.sid[2]].count);
  }
  {  // a contributor before the row's first: its distance has no unsigned form
    Map M;
    M.rowptr = {0, 3, 5};
    M.cols = {40, 10, 50, 0, 0xFFFFFFF0u};
    const RowCode c = round_trip("descending row", M, ROWCODE_MAX_DEFAULT);
    CHECK(c.sid[0] == ROWCODE_ESCAPE && c.sid[1] != ROWCODE_ESCAPE && c.pos0[1] == 0u, "descending row: not the escape");
  }
  {  // nothing at all, a map of no rows, rows of no contributors
    Map none;
    const RowCode c = round_trip("no arrays", none, ROWCODE_MAX_DEFAULT);
    CHECK(c.table.empty() && c.nescape == 0, "no arrays: a table of %zu", c.table.size());
    Map empty;
    empty.rowptr = {0};
    round_trip("empty map", empty, ROWCODE_MAX_DEFAULT);
    Map hollow;
    hollow.rowptr = {0, 0, 1, 1};
    hollow.cols = {5};
    const RowCode h = round_trip("rows without contributors", hollow, ROWCODE_MAX_DEFAULT);
    CHECK(h.nescape == 0 && h.sid[0] == h.sid[2] && h.table[h.sid[0]].count == 0, "rows without contributors are not coded as such");
  }
  if (g_fail) { fprintf(stderr, "FAIL: %d checks\n", g_fail); return 1; }
  printf("row_code_host ok\n");
  return 0;
}
