// kernels_pointblock.hpp -- launch interface of the point-block Jacobi kernels (kernels_pointblock.hip): the 3 x 3 nodal blocks of
// the Jacobian (CeedOperatorLinearAssemblePointBlockDiagonal), their inverses, and the smoother step that uses them.  A header of its
// own: kernels.hpp is a dependency of every fused-kernel object, and none of them needs this.
#pragma once
#include "kernels.hpp"

namespace cps {

// `name` as for launch_diag: "pbdiag<P=..,Q=..,LinElas|HyperSSdF|HyperFSdF>", hipErrorInvalidValue with *name untouched when the
// combination is not instantiated (the set of launch_diag: CPS_DIAG_PQ, kernel_diag_sf.hpp)
hipError_t launch_pbdiag(int P, int Q, int qf, const BasisTables &t, const DiagArgs &a, hipStream_t s, const char **name);
// blocks[3 * node_off[r] + j] = sum over the node's contributors, in element order, of evec[9 * cols[k] + j], j < 9: the transpose
// map of launch_assemble() with nine values per contributor.  No atomics.
hipError_t launch_pb_assemble(const NodeMap &m, const double *evec, double *blocks, hipStream_t s);
// In place, per node: components whose diagonal entry is exactly zero are dropped, the remaining principal sub-block is inverted and
// embedded in zeros.  *n_bad (device, may be null; zeroed by the caller) counts the blocks with a non-finite or non-positive pivot.
hipError_t launch_pb_invert(double *blocks, size_t nnodes, int *n_bad, hipStream_t s);
// w_n = B_n x_n
hipError_t launch_pb_mult(double *w, const double *blocks, const double *x, size_t nnodes, hipStream_t s);
// ri = b - t (t may be null), stored if r is given;  d = c1 B ri + c2 d;  x = d or x + d
hipError_t launch_pb_cheb_step(double *x, double *d, double *r, const double *b, const double *t, const double *blocks, double c1,
                               double c2, int assign_x, size_t nnodes, hipStream_t s);

}  // namespace cps
