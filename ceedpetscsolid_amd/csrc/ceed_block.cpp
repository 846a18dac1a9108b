// ceed_block.cpp -- block vectors (CeedXVectorBlockGram, CeedXVectorBlockCombine; kernels_block.hip): k columns of length n in one
// CeedVector, column j at element j * ld.  Every argument is checked before anything is launched (block_args.hpp holds the
// arithmetic); both calls only queue kernels on the Ceed's stream -- no host read, no array made here -- so both can be recorded.
#include "block_args.hpp"
#include "ceed_impl.hpp"

static_assert(cps::BLOCK_ARG_MAX_COLS == cps::BLOCK_MAX_COLS, "block_args.hpp and kernels.hpp disagree on the column limit");

static bool given(CeedVector v) { return v && v != CEED_VECTOR_NONE; }

extern "C" int CeedXVectorBlockGetLimits(CeedInt *max_cols, CeedInt *gram_rows, CeedInt *gram_max_parts, CeedInt *combine_rows,
                                         CeedInt *combine_max_groups) {
  if (max_cols) *max_cols = cps::BLOCK_MAX_COLS;
  if (gram_rows) *gram_rows = cps::BLOCK_GRAM_ROWS;
  if (gram_max_parts) *gram_max_parts = cps::BLOCK_GRAM_MAX_PARTS;
  if (combine_rows) *combine_rows = cps::BLOCK_COMBINE_ROWS;
  if (combine_max_groups) *combine_max_groups = cps::BLOCK_COMBINE_MAX_GROUPS;
  return 0;
}

extern "C" int CeedXVectorBlockGram(CeedVector A, CeedInt a0, CeedInt ka, CeedVector B, CeedInt b0, CeedInt kb, CeedInt n, CeedInt ld,
                                    CeedVector weight, CeedVector G) {
  const char *who = "CeedXVectorBlockGram";
  if (!given(A) || !given(B) || !given(G)) return ceed_error("%s: A, B and G must be vectors", who);
  int e = cps::block_shape_check(n, ld);
  if (e) return ceed_error("%s: %s (n = %d, ld = %d)", who, cps::block_arg_message(e), n, ld);
  if ((e = cps::block_range_check(a0, ka, n, ld, A->length)))
    return ceed_error("%s: A: %s (columns %d .. %d, n = %d, ld = %d, length %d)", who, cps::block_arg_message(e), a0, a0 + ka, n, ld, A->length);
  if ((e = cps::block_range_check(b0, kb, n, ld, B->length)))
    return ceed_error("%s: B: %s (columns %d .. %d, n = %d, ld = %d, length %d)", who, cps::block_arg_message(e), b0, b0 + kb, n, ld, B->length);
  if ((int64_t)G->length < (int64_t)ka * kb) return ceed_error("%s: G holds %d entries, %d x %d are written", who, G->length, ka, kb);
  if (given(weight) && weight->length < n) return ceed_error("%s: the weight holds %d entries, n = %d are read", who, weight->length, n);
  if (G == A || G == B || (given(weight) && G == weight)) return ceed_error("%s: G must not be one of the operands", who);
  Ceed c = A->ceed;
  double *pa, *pb, *pw = nullptr, *pg;
  CHK(vec_dev(A, false, &pa)); CHK(vec_dev(B, false, &pb));
  if (given(weight)) CHK(vec_dev(weight, false, &pw));
  CHK(vec_dev(G, true, &pg));
  HIPCHK(cps::launch_block_gram(pa + (size_t)a0 * (size_t)ld, ka, pb + (size_t)b0 * (size_t)ld, kb, pw, (size_t)n, (size_t)ld,
                                c->d_block_part.get(), pg, c->stream));
  return 0;
}

extern "C" int CeedXVectorBlockCombine(CeedVector Y, CeedInt y0, CeedInt ky, CeedVector A, CeedInt a0, CeedInt ka, CeedVector C,
                                       double beta, CeedInt n, CeedInt ld) {
  const char *who = "CeedXVectorBlockCombine";
  if (!given(Y) || !given(A) || !given(C)) return ceed_error("%s: Y, A and C must be vectors", who);
  int e = cps::block_shape_check(n, ld);
  if (e) return ceed_error("%s: %s (n = %d, ld = %d)", who, cps::block_arg_message(e), n, ld);
  if ((e = cps::block_range_check(y0, ky, n, ld, Y->length)))
    return ceed_error("%s: Y: %s (columns %d .. %d, n = %d, ld = %d, length %d)", who, cps::block_arg_message(e), y0, y0 + ky, n, ld, Y->length);
  if ((e = cps::block_range_check(a0, ka, n, ld, A->length)))
    return ceed_error("%s: A: %s (columns %d .. %d, n = %d, ld = %d, length %d)", who, cps::block_arg_message(e), a0, a0 + ka, n, ld, A->length);
  if ((int64_t)C->length < (int64_t)ka * ky) return ceed_error("%s: C holds %d entries, %d x %d are read", who, C->length, ka, ky);
  if (C == Y) return ceed_error("%s: C must not be the output", who);
  Ceed c = Y->ceed;
  double *py, *pa, *pc;
  // (read access first: the overlap is decided on the arrays' addresses, and a refused call must leave Y as it was)
  CHK(vec_dev(A, false, &pa)); CHK(vec_dev(C, false, &pc)); CHK(vec_dev(Y, false, &py));
  if (cps::block_ranges_overlap((uint64_t)(uintptr_t)py / sizeof(double), y0, ky, (uint64_t)(uintptr_t)pa / sizeof(double), a0, ka, n, ld))
    return ceed_error("%s: the columns %d .. %d of Y overlap the columns %d .. %d of A: the kernel does not work in place", who, y0, y0 + ky,
                      a0, a0 + ka);
  CHK(vec_dev(Y, true, &py));
  HIPCHK(cps::launch_block_combine(py + (size_t)y0 * (size_t)ld, ky, pa + (size_t)a0 * (size_t)ld, ka, pc, beta, (size_t)n, (size_t)ld,
                                   c->stream));
  return 0;
}
