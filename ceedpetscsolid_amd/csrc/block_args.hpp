// block_args.hpp -- the argument checks of the block-vector entry points (ceed_block.cpp) as pure functions: no HIP, no library
// object, 64-bit arithmetic throughout (tests/block_args_host.cpp runs them under the sanitizers).
//
// A block is k columns of length n in one array, column j at element j * ld, ld >= n.  A column range [x0, x0 + kx) of it touches the
// elements [x0 * ld, (x0 + kx) * ld - (ld - n)): the padding behind its last column is not part of it.
#pragma once
#include <cstdint>

namespace cps {

constexpr int BLOCK_ARG_MAX_COLS = 48;   // = BLOCK_MAX_COLS of kernels.hpp (ceed_block.cpp asserts it)

enum BlockArgError : int {
  BLOCK_ARG_OK = 0,
  BLOCK_ARG_ROWS,        // n < 1
  BLOCK_ARG_LD,          // ld < n
  BLOCK_ARG_COUNT,       // a column count outside 1 .. 48
  BLOCK_ARG_FIRST,       // a negative first column
  BLOCK_ARG_RANGE,       // the column range reaches past the end of its vector
};

static inline const char *block_arg_message(int e) {
  switch (e) {
    case BLOCK_ARG_ROWS: return "the number of rows n must be at least 1";
    case BLOCK_ARG_LD: return "the leading dimension ld must be at least n";
    case BLOCK_ARG_COUNT: return "a column count must lie in 1 .. 48";
    case BLOCK_ARG_FIRST: return "a first column must not be negative";
    case BLOCK_ARG_RANGE: return "the column range reaches past the end of its vector";
    default: return "";
  }
}

static inline int block_shape_check(int64_t n, int64_t ld) {
  if (n < 1) return BLOCK_ARG_ROWS;
  if (ld < n) return BLOCK_ARG_LD;
  return BLOCK_ARG_OK;
}
// one past the last element columns [x0, x0 + kx) touch (the shape already checked)
static inline int64_t block_range_end(int64_t x0, int64_t kx, int64_t n, int64_t ld) { return (x0 + kx) * ld - (ld - n); }
static inline int block_range_check(int64_t x0, int64_t kx, int64_t n, int64_t ld, int64_t length) {
  if (kx < 1 || kx > BLOCK_ARG_MAX_COLS) return BLOCK_ARG_COUNT;
  if (x0 < 0) return BLOCK_ARG_FIRST;
  if (block_range_end(x0, kx, n, ld) > length) return BLOCK_ARG_RANGE;
  return BLOCK_ARG_OK;
}
// do the element ranges [base_a + a0 ld, ...) and [base_y + y0 ld, ...) of two checked column ranges share an element?  The bases are
// the arrays' addresses in elements (address / 8): two vectors over one allocation (a block's owner and a view of it) are seen too.
static inline bool block_ranges_overlap(uint64_t base_y, int64_t y0, int64_t ky, uint64_t base_a, int64_t a0, int64_t ka, int64_t n, int64_t ld) {
  const uint64_t yb = base_y + (uint64_t)(y0 * ld), ye = base_y + (uint64_t)block_range_end(y0, ky, n, ld);
  const uint64_t ab = base_a + (uint64_t)(a0 * ld), ae = base_a + (uint64_t)block_range_end(a0, ka, n, ld);
  return yb < ae && ab < ye;
}

}  // namespace cps
