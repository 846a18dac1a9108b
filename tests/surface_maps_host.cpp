// surface_maps_host.cpp -- the index arithmetic of a surface load (csrc/index_maps.hpp as csrc/ceed_surface.cpp calls it) on the host
// alone: built by test_surface_maps.py with g++ under the address and undefined-behaviour sanitizers.  Faces of an nx x ny patch of
// P x P face nodes, numbered with gaps (offset = 3 * (7 + 2 * node)), with and without a Dirichlet mask: the face offsets (plain
// without a mask: the call must not touch a null mask), the faces' transpose map (every E position in exactly one row, its node's,
// contributors in face order, valences 1, 2, 4) and the mask in row order; and the check of a caller's offsets (check_face_offsets: a
// valid patch, a negative offset, o + 2 == lsize, o % 3 != 0, the reported face, the empty list).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "index_maps.hpp"

using namespace cps;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); fails++; } } while (0)

static void patch(int nx, int ny, int P) {
  const int p = P - 1, NX = nx * p + 1, NY = ny * p + 1;
  std::vector<int> off;
  for (int fy = 0; fy < ny; fy++)
    for (int fx = 0; fx < nx; fx++)
      for (int j = 0; j < P; j++)
        for (int i = 0; i < P; i++) off.push_back(3 * (7 + 2 * ((fy * p + j) * NX + fx * p + i)));
  const int lsize = 3 * (7 + 2 * NX * NY + 5);
  std::vector<unsigned char> mask((size_t)lsize, 0);
  for (int n = 0; n < NX * NY; n++)
    if (n % NX == 0) { mask[3 * (7 + 2 * n)] = 1; mask[3 * (7 + 2 * n) + 2] = 1; }      // x = 0: components 0 and 2
  const std::vector<uint32_t> plain = face_offsets(off, nullptr), fl = face_offsets(off, mask.data());
  CHECK(plain.size() == off.size() && fl.size() == off.size());
  for (size_t i = 0; i < off.size(); i++) {
    CHECK(plain[i] == (uint32_t)off[i]);
    CHECK((fl[i] & OFF_MASK) == (uint32_t)off[i]);
    const bool at0 = ((off[i] / 3 - 7) / 2) % NX == 0;
    CHECK((fl[i] >> OFF_FLAG_SHIFT) == (at0 ? 5u : 0u));
  }
  const TransposeMap T = transpose_map(off, lsize, P * P, 3, nullptr, 0);
  CHECK((int)T.node_off.size() == NX * NY && T.rowptr.size() == T.node_off.size() + 1 && T.nskipped == 0);
  std::vector<int> seen(off.size(), 0);
  int valence[5] = {0, 0, 0, 0, 0};
  for (size_t r = 0; r < T.node_off.size(); r++) {
    CHECK(r == 0 || T.node_off[r] > T.node_off[r - 1]);
    const uint32_t len = T.rowptr[r + 1] - T.rowptr[r];
    CHECK(len >= 1 && len <= 4);
    if (len <= 4) valence[len]++;
    for (uint32_t k = T.rowptr[r]; k < T.rowptr[r + 1]; k++) {
      const uint32_t c = T.cols[k];
      CHECK(c < off.size());
      if (c < off.size()) { seen[c]++; CHECK((uint32_t)off[c] == T.node_off[r]); }
      CHECK(k == T.rowptr[r] || T.cols[k - 1] < c);                 // face order
    }
  }
  for (int s : seen) CHECK(s == 1);
  CHECK(valence[4] == (nx - 1) * (ny - 1) && valence[3] == 0);
  CHECK(valence[2] == (nx - 1) * (ny * p + 1 - (ny - 1)) + (ny - 1) * (nx * p + 1 - (nx - 1)));
  const std::vector<unsigned char> rf = row_flag_bits(T.node_off, mask.data(), 3, 1);
  CHECK(rf.size() == T.node_off.size());
  for (size_t r = 0; r < rf.size(); r++) CHECK(rf[r] == ((((T.node_off[r] / 3 - 7) / 2) % NX == 0) ? 5 : 0));
  // the check of a caller's offsets: the patch holds, and holds in the smallest L-vector that has its last node
  const size_t nface = (size_t)nx * ny;
  const int last = off.back();                                       // the largest offset of the patch
  CHECK(check_face_offsets(off.data(), nface, P * P, lsize).fault == FACE_OFFSETS_OK);
  CHECK(check_face_offsets(off.data(), nface, P * P, last + 3).fault == FACE_OFFSETS_OK);
  // o + 2 == lsize: the last face holds the node, and is the one reported (the first that does, when it is not the only one)
  const FaceOffsetCheck past = check_face_offsets(off.data(), nface, P * P, last + 2);
  CHECK(past.fault == FACE_OFFSET_PAST_LSIZE && past.offset == last && past.face == nface - 1);
  // one bad entry in face k: that face, that offset, that rule -- wherever in the face it stands
  for (size_t k = 0; k < nface; k += (nface > 1 ? nface - 1 : 1))
    for (int n : {0, P * P - 1}) {
      std::vector<int> bad = off;
      const size_t at = k * P * P + n;
      bad[at] = -3;
      FaceOffsetCheck c = check_face_offsets(bad.data(), nface, P * P, lsize);
      CHECK(c.fault == FACE_OFFSET_PAST_LSIZE && c.face == k && c.offset == -3);
      bad[at] = off[at] + 1;
      c = check_face_offsets(bad.data(), nface, P * P, lsize);
      CHECK(c.fault == FACE_OFFSET_NOT_NODE && c.face == k && c.offset == off[at] + 1);
      bad[at] = lsize - 2;                                           // o + 2 == lsize; lsize is a multiple of 3, so only this rule breaks ...
      c = check_face_offsets(bad.data(), nface, P * P, lsize);
      CHECK(c.fault == FACE_OFFSET_PAST_LSIZE && c.face == k && c.offset == lsize - 2);
      bad[at] = lsize - 3;                                           // ... and the last node of the L-vector holds
      CHECK(check_face_offsets(bad.data(), nface, P * P, lsize).fault == FACE_OFFSETS_OK);
    }
}

int main() {
  for (int P = 2; P <= 8; P += 3) { patch(1, 1, P); patch(2, 2, P); patch(3, 1, P); patch(2, 3, P); }
  // no faces at all: empty arrays, valid to upload
  const std::vector<int> none;
  CHECK(face_offsets(none, nullptr).empty());
  const TransposeMap T0 = transpose_map(none, 24, 4, 3, nullptr, 0);
  CHECK(T0.node_off.empty() && T0.rowptr.size() == 1 && T0.cols.size() == 1);
  // ... and nothing to check: the list is never read (a null one must not be), whatever the L-size
  CHECK(check_face_offsets(nullptr, 0, 4, 24).fault == FACE_OFFSETS_OK && check_face_offsets(nullptr, 0, 64, 0).fault == FACE_OFFSETS_OK);
  // more entries than the face E-vector can index in 32 bits are refused before the list is read
  CHECK(check_face_offsets(nullptr, (size_t)0x7FFFFFFF / 3 / 4 + 1, 4, 24).fault == FACE_OFFSETS_TOO_MANY);
  if (fails) { fprintf(stderr, "FAIL: %d checks\n", fails); return 1; }
  printf("surface_maps_host ok\n");
  return 0;
}
