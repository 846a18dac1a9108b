// block_args_host.cpp -- the argument checks of the block-vector entry points (csrc/block_args.hpp) on the host alone, built with g++
// under the address and undefined-behaviour sanitizers (tests/test_block_args.py).  Shapes at the limits of CeedInt: a block of
// 48 columns of 19 537 320 rows (k * ld = 9.4e8), ranges that end exactly at / one past the end of their vector, products that would
// overflow 32 bits, and the overlap test on element addresses against a brute-force walk over small shapes.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "block_args.hpp"

static int failures = 0;
#define EXPECT(c) do { if (!(c)) { fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } } while (0)

int main() {
  using namespace cps;
  // shape
  EXPECT(block_shape_check(0, 0) == BLOCK_ARG_ROWS);
  EXPECT(block_shape_check(-1, 5) == BLOCK_ARG_ROWS);
  EXPECT(block_shape_check(5, 4) == BLOCK_ARG_LD);
  EXPECT(block_shape_check(5, 5) == BLOCK_ARG_OK);
  EXPECT(block_shape_check(1, INT32_MAX) == BLOCK_ARG_OK);
  // counts and first columns
  EXPECT(block_range_check(0, 0, 4, 4, 1000) == BLOCK_ARG_COUNT);
  EXPECT(block_range_check(0, 49, 4, 4, 1000) == BLOCK_ARG_COUNT);
  EXPECT(block_range_check(0, -3, 4, 4, 1000) == BLOCK_ARG_COUNT);
  EXPECT(block_range_check(-1, 2, 4, 4, 1000) == BLOCK_ARG_FIRST);
  EXPECT(block_range_check(0, 48, 4, 4, 192) == BLOCK_ARG_OK);
  // the padding behind the last column is not part of the range
  EXPECT(block_range_end(2, 3, 5, 8) == 5 * 8 - 3);
  EXPECT(block_range_check(2, 3, 5, 8, 37) == BLOCK_ARG_OK);
  EXPECT(block_range_check(2, 3, 5, 8, 36) == BLOCK_ARG_RANGE);
  // the largest shapes: the products need 64 bits
  const int64_t n = 19537320, kmax = 48;
  EXPECT(block_range_check(0, kmax, n, n, n * kmax) == BLOCK_ARG_OK);
  EXPECT(block_range_check(1, kmax, n, n, n * kmax) == BLOCK_ARG_RANGE);
  EXPECT(block_range_check(INT32_MAX - 48, 48, INT32_MAX, INT32_MAX, INT32_MAX) == BLOCK_ARG_RANGE);
  EXPECT(block_range_check(INT32_MAX, 1, 1, INT32_MAX, INT32_MAX) == BLOCK_ARG_RANGE);
  EXPECT(block_range_end(INT32_MAX - 48, 48, INT32_MAX, INT32_MAX) == (int64_t)INT32_MAX * INT32_MAX);
  for (int e = BLOCK_ARG_ROWS; e <= BLOCK_ARG_RANGE; e++) EXPECT(block_arg_message(e)[0] != 0);
  EXPECT(block_arg_message(BLOCK_ARG_OK)[0] == 0);
  // overlap against a walk over the elements, two views of one allocation at different bases included
  for (int ld = 3; ld <= 5; ld++)
    for (int nn = 1; nn <= ld; nn++)
      for (int y0 = 0; y0 < 4; y0++) for (int ky = 1; ky <= 3; ky++)
        for (int a0 = 0; a0 < 4; a0++) for (int ka = 1; ka <= 3; ka++)
          for (int shift = 0; shift <= 2 * ld; shift += ld) {
            const uint64_t base_y = 1000, base_a = 1000 + (uint64_t)shift;
            std::vector<char> hit(2000, 0);
            for (int64_t i = y0 * ld; i < block_range_end(y0, ky, nn, ld); i++) hit[base_y + i] = 1;
            bool brute = false;
            for (int64_t i = a0 * ld; i < block_range_end(a0, ka, nn, ld); i++) brute = brute || hit[base_a + i];
            EXPECT(block_ranges_overlap(base_y, y0, ky, base_a, a0, ka, nn, ld) == brute);
          }
  EXPECT(!block_ranges_overlap(0, 0, 24, 0, 24, 24, n, n));
  EXPECT(block_ranges_overlap(0, 0, 24, 0, 23, 24, n, n));
  EXPECT(!block_ranges_overlap(1u << 20, 0, 48, (1u << 20) + (uint64_t)(n * 48), 0, 48, n, n));
  if (failures) { fprintf(stderr, "block_args_host: %d FAILures\n", failures); return 1; }
  printf("block_args_host ok\n");
  return 0;
}
