// kernels.hpp -- host-visible launch interface of the gfx950 kernels.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

namespace cps {

enum QFKind : int {
  QF_NONE = 0,
  QF_SETUP_GEO,
  QF_LINELAS,     // LinElasF and LinElasdF: same linear map
  QF_HYPERSS_F,
  QF_HYPERSS_DF,
  QF_HYPERFS_F,
  QF_HYPERFS_DF,
  QF_IDENTITY,
  QF_CONST_FORCE,
  QF_MMS_FORCE,
  QF_MMS_TRUE,
  QF_ENERGY_LINELAS,
  QF_ENERGY_HYPERSS,
  QF_ENERGY_HYPERFS,
  QF_DIAG_LINELAS,
  QF_DIAG_HYPERSS,
  QF_DIAG_HYPERFS,
  QF_HYPERFS_DF_DS,   // HyperFSdF reading the DERIVED state (F^-1, lambda ln J - mu) the residual kernel wrote beside grad u
  QF_MASS,            // v = c qdata[0] u: the mass operator of the elastodynamic solve (kernels_mass.hip)
  QF_STRESS_LINELAS,  // the Cauchy stress the residual integrates, at the points or projected to the nodes (kernels_stress.hip)
  QF_STRESS_HYPERSS,
  QF_STRESS_HYPERFS,
  QF_MASS_FIELD,      // v = c rho qdata[0] u, rho a passive INTERP field: the mass operator with a density field (kernels_mass.hip)
  QF_THERMAL_FORCE,   // the residual of the thermal coupling energy from a nodal temperature field (kernels_stress.hip, modes with a field)
  QF_THERMAL_TANGENT, // its tangent in the finite-strain model
  QF_STRESS_LINELAS_THERMAL,  // the stress with the thermal term: QF_STRESS_* plus a passive INTERP(1) temperature field
  QF_STRESS_HYPERSS_THERMAL,
  QF_STRESS_HYPERFS_THERMAL,
};

constexpr int MAXN1D = 8;  // largest P or Q supported by the kernel tables
constexpr int EO_TAB = 36;  // doubles per even-odd table (see FusedGradArgs::eo)

// 1-D tables handed to kernels by value: they live in the kernarg segment; the pencil kernel reads them from
// there as scalar operands, the other kernels stage them into LDS once per block.
struct BasisTables {
  double interp[MAXN1D * MAXN1D];  // B[q][p], Q x P row-major (CeedBasis interp1d)
  double colo[MAXN1D * MAXN1D];    // Dq[q][m], Q x Q: derivative of the Lagrange basis on the
                                   // quadrature points, evaluated there (collocated gradient)
  double grad[MAXN1D * MAXN1D];    // G[q][p], Q x P (CeedBasis grad1d; diagonal assembly)
  double qw[MAXN1D];               // 1-D quadrature weights
};

// Offsets carry the Dirichlet flags of the three components of a node in their
// top bits (set by CeedXOperatorSetDirichletMask); plain offsets have none.
constexpr uint32_t OFF_MASK = 0x1FFFFFFFu;
constexpr int OFF_FLAG_SHIFT = 29;

// Even-odd form of the 1-D products (FusedGradArgs::eo): used wherever the form exists -- the bases of this ABI are built
// on Gauss / Gauss-Lobatto points (CeedBasisCreateTensorH1Lagrange), whose tables are centro-(anti)symmetric.  Below 4 x 4
// the additions cost what the halved products save (measured -1.6 % at Q = 3); at Q = 8 an even-odd table (36
// coefficients) no longer fits the 60 SGPRs a pass has for its table.
constexpr bool pencil_even_odd(int Q) { return Q >= 4 && Q <= 7; }
// The derived state of the finite-strain tangent (QF_HYPERFS_DF_DS) is used -- and written by the residual kernel -- from Q = 6 on:
// measured -2.6 ... -3.1 % there, +-0 % at Q = 5 (profiles/r03_ab_experiments.txt item 3; again r04 item 15), for ten more doubles
// per point stored.
constexpr bool pencil_derived_state(int Q) { return Q >= 6; }

struct FusedGradArgs {
  const uint32_t *offsets;  // [nelem][P^3] (flagged)
  const double *x;          // active input L-vector, interlaced [node][3]
  double *y;                // active output L-vector: element-interior nodes are stored here directly (direct)
  const double *qdata;      // [nelem][10][Q^3]
  const double *state_in;   // [nelem][9][Q^3] (QF_HYPERFS_DF_DS: [nelem][10][Q^3], the derived state) or null
  double *state_out;        // [nelem][9][Q^3] or null
  double *state_out2;       // HyperFSF only, may be null: [nelem][10][Q^3] derived state of the tangent (qf_hyperfs_df_ds), written too
  int nelem;                // elements processed by this launch ...
  int elem_begin;           // ... starting at this element (segments of a pipelined apply, split-phase apply)
  int mask_in, mask_out;    // honour the Dirichlet flags on gather / scatter
  double nu, E, lambda, TwoMu;
  double *evec;               // element results ([elem][shell node or node][3], plain coalesced stores); launch_assemble()
                               // sums them into y per node in element order
  int evec_stride;            // doubles between the E-vector blocks of consecutive elements: 3 * nodes per block
  const double *geo;          // if set, [nelem][GEO_NCOEF] trilinear-map coefficients of the elements (launch_geo_coeffs);
                               // the kernel then RECOMPUTES qdata = SetupGeo(x) at every point (27 FMAs + adjugate) instead
                               // of streaming its 80 bytes per point from HBM
  const double *geo_aff;      // set (with geo) only when EVERY element is affine: [nelem][GEO_NAFF] = {det J, dXdx[9]} of the
                               // element (launch_geo_affine) -- the kernel then multiplies det J by the point's weight and
                               // reads the nine factors instead of forming J, its adjugate and a reciprocal at every point
  const double *geo_swept;    // set (with geo, without geo_aff) when EVERY element is SWEPT along the same reference direction geo_axis:
                               // x and y bilinear in the other two directions, z linear in that one (the prisms of an extruded mesh: the
                               // reference's cylinders).  [nelem][GEO_NSWEPT] (launch_geo_swept); J is then a 2 x 2 block and a constant,
                               // dXdx has five entries and the two products of the physics with it take 15 multiply-adds instead of 27
  int geo_axis;               // the sweep's reference direction (0, 1, 2), one for the whole mesh
  double qref[MAXN1D], qwt[MAXN1D];  // 1-D quadrature points / weights of the geometry (used with geo)
  // Even-odd form of the 1-D tables (pencil_even_odd(Q)).  The tables of symmetric point sets are
  // centro-symmetric (interp: M[N-1-i][K-1-j] = M[i][j]) or centro-antisymmetric (derivatives), so with
  // xe = x_j + x_{K-1-j}, xo = x_j - x_{K-1-j} an N x K product costs ~N K / 2 FMAs + N + K adds instead of N K FMAs.
  // eo[t]: t = 0 B, 1 B^T, 2 D, 3 D^T, 4 G, 5 G^T; per table Me[r][j] at r * (K/2) + j, Mo at 16 + r * (K/2) + j, the
  // middle column at 32 + r (r < (N+1)/2, j < K/2); built and checked by the host when the operator is planned.
  double eo[6][EO_TAB];
  int direct;                 // results at ELEMENT-INTERIOR nodes (0 < i,j,k < P-1; one contributor, verified on the
                               // host) are stored straight into y and skip the E-vector round trip; the E-vector then is
                               // [elem][shell node][3] and the transpose map handed to launch_assemble() holds the shell
                               // nodes only, its columns being positions e * element_shell_size(P) + rank
  double mass_c;              // k_fused_pencil_mass only: the coefficient c of K + c M (CeedXOperatorSetMassTerm), read at every launch
                               // like MassArgs::coef -- a recorded graph keeps the value it was recorded with
#ifdef CPS_PHASE_TIMING       // (diagnostic build only) the time-stamp buffer, filled in by the launcher from CEED_MI355X_PHASE_BUF
  long long *phase_buf;
#endif
};
// how a launch obtains the geometric factors (k_fused_pencil's GEO): 0 qdata read, 1 recomputed per point, 2 affine, 3 swept elements
static inline int fused_geo_mode(const FusedGradArgs &a) { return !a.geo ? 0 : (a.geo_aff ? 2 : (a.geo_swept ? 3 : 1)); }
// the launch shape of the fused kernel (launch_fused_pencil_t): host side only, none of it reaches the kernel
struct FusedLaunch {
  int wave_groups;    // > 0: every wave is given at most this many groups (grid = groups / wave_groups) instead of the persistent grid
  int waves_per_cu;   // > 0: persistent waves per CU (tuning hook CEED_MI355X_PENCIL_WAVES) instead of pencil_waves_per_cu(Q)
};
hipError_t launch_clock_probe(long long *out /* device: shader cycles, 100 MHz ticks */, int spin_us, hipStream_t s);
// compute units of the current device (one device per process: cached)
int device_cu_count();
// element-interior test shared by the kernel and the host-side map builder
#ifdef __HIPCC__
__host__ __device__
#endif
static inline bool node_is_element_interior(int n, int P) {
  const int i = n % P, j = (n / P) % P, k = n / (P * P);
  return i > 0 && i < P - 1 && j > 0 && j < P - 1 && k > 0 && k < P - 1;
}
// rank of node n among the SHELL (non-interior) nodes of its element: the E-vector of the direct-store mode holds shell
// entries only, [element][shell rank][component].  FACE-MAJOR order (round 2): the two k-faces whole (edges and vertices
// included), then the two j-faces without the rows the k-faces hold, then the two i-faces' interiors -- so the nodes an
// element shares with ONE neighbour are contiguous in both elements' blocks, and k_assemble, whose consecutive rows are
// the nodes of one shared face, reads runs of whole faces instead of every fifth 24-byte record of an i-face (round 1's
// lexicographic order: 0.15 GB of line over-fetch per apply; profiles/r02_ab_experiments.txt item 5).
#ifdef __HIPCC__
__host__ __device__
#endif
static inline int node_shell_rank(int n, int P) {
  const int m = P - 2, i = n % P, j = (n / P) % P, k = n / (P * P);
  if (k == 0) return j * P + i;
  if (k == P - 1) return P * P + j * P + i;
  if (j == 0) return 2 * P * P + (k - 1) * P + i;
  if (j == P - 1) return 2 * P * P + P * m + (k - 1) * P + i;
  if (i == 0) return 2 * P * P + 2 * P * m + (k - 1) * m + (j - 1);
  return 2 * P * P + 2 * P * m + m * m + (k - 1) * m + (j - 1);   // i == P - 1 (interior nodes have no rank)
}
// shell nodes of an element = 24-byte records between the shell E-vector blocks of consecutive elements: the blocks are packed
// (every block padded to whole 128-byte lines was measured in round 4, nothing: profiles/r04_ab_experiments.txt item 19)
#ifdef __HIPCC__
__host__ __device__
#endif
static inline int element_shell_size(int P) { return P * P * P - (P > 2 ? (P - 2) * (P - 2) * (P - 2) : 0); }

// p-multigrid transfer in OWNER form (kernels_transfer.hip, k_transfer): every fine node belongs to the first element that holds it.
struct TransferArgs {
  const uint32_t *off_c;  // coarse [nelem][Pc^3], the coarse side's Dirichlet flags in the top bits
  const uint32_t *own_f;  // fine   [nelem][Pf^3]: offset | Dirichlet flags of the nodes this element OWNS, 0xFFFFFFFF for the others
  const double *x;
  double *y;              // prolong: the fine L-vector, stored by the owners
  const double *w_f;      // per fine dof: (scale, e.g. multiplicity^-1 over all ranks) x (local multiplicity); null when every entry is 1
  int nelem;
  int mask_c, mask_f;     // honour the flags of the coarse / fine side
  int add;                // prolong: y += (restrict: launch_assemble() adds)
  double *evec;           // restrict: element results ([elem][Pc^3][3], masked entries as zeros); launch_assemble() sums them
                          // into y in element order
};
hipError_t launch_transfer_weights(double *w, const double *scale, size_t n, int *n_not_unit, hipStream_t s);

// x_c(xi) = a0 + a[c][0] xi + a[c][1] eta + a[c][2] zeta + a[c][3] xi eta + a[c][4] xi zeta + a[c][5] eta zeta + a[c][6] xi eta zeta
// on [-1,1]^3: the 7 coefficients per component that the Jacobian d x / d xi needs, [c][m] per element.
constexpr int GEO_NCOEF = 21;
hipError_t launch_geo_coeffs(const uint32_t *off_x, const double *xcoord, double *geo, int nelem, hipStream_t s);
// Affine elements (the 12 coefficients of the xi eta ... terms vanish to 1e-14 of the linear ones: parallelepipeds).  For
// every element {det J, dXdx[9]} -- SetupGeo's output at ANY of its points but for the quadrature weight -- goes to
// aff[e][GEO_NAFF]; *n_not_affine (device, zeroed by the caller) counts the elements that are NOT affine.
constexpr int GEO_NAFF = 10;
hipError_t launch_geo_affine(const double *geo, double *aff, int nelem, int *n_not_affine, hipStream_t s);
// Swept elements: z = z0 + zs xi_s for one reference direction s, x and y bilinear in the other two (a < b) and free of xi_s, all to
// 1e-13 of the largest linear coefficient.  sw[e][GEO_NSWEPT] = {x_a, x_b, x_ab, y_a, y_b, y_ab, sgn zs, 1 / zs} for the element's OWN
// sweep direction (sgn = -1 for s = 1: (a, b, s) is then an odd permutation of the reference directions).  Two passes: axis < 0 COUNTS --
// count[s] (device, zeroed by the caller) the elements swept along s, EVERY direction an element qualifies for (an axis-aligned brick
// qualifies for all three, so a mesh that mixes bricks with z-swept prisms still finds its common direction), count[3] the ones that are
// not swept at all (or along x or y in space); axis >= 0 FILLS sw[] for that direction.
constexpr int GEO_NSWEPT = 8;
hipError_t launch_geo_swept(const double *geo, double *sw, int nelem, int *count, int axis, hipStream_t s);

struct SetupGeoArgs {
  const uint32_t *off_x;  // [nelem][8]
  const double *xcoord;   // interlaced [vertex][3]
  double *qdata;          // [nelem][10][Q^3]
  int nelem;
};

// The scalar diagonal and the point-block diagonal (kernel_diag_sf.hpp; launch_diag here, launch_pbdiag in kernels_pointblock.hpp)
struct DiagArgs {
  const uint32_t *offsets;  // [nelem][P^3] (flagged)
  const double *qdata, *state_in;
  int nelem;
  // a dropped row zeroes its entry (scalar) / row c' of the node's block (mask_out); blocks only: entry (c', c) is also zero where
  // input c reads as zero (mask_in).  The scalar diagonal has c' == c and never reads mask_in.
  int mask_in, mask_out;
  double nu, E, lambda, TwoMu;
  double *evec;  // element contributions, [elem][P^3][3] (launch_assemble() sums them) or [elem][P^3][c'][c] (launch_pb_assemble())
};

// The stored state of a level with its own quadrature (kernels_state.hip, k_state_at_points): grad u of the FINE displacement at the
// level's Q_c^3 points, through the basis (P_f, Q_c) and the dXdx entries of the level's qdata.
struct StateArgs {
  const uint32_t *offsets;  // fine restriction [nelem][Pf^3] (flagged)
  const double *x;          // the displacement L-vector, interlaced [node][3]
  const double *qdata;      // the level's [nelem][10][Qc^3]
  double *state_out;        // the level's [nelem][9][Qc^3]: every entry is overwritten
  int nelem;
  int mask_in;              // honour the Dirichlet flags on the gather (constrained entries read as zero)
};

// The mass operator and its diagonal (kernels_mass.hip, k_mass): v = coef B^T (w det J) B u on 3 interlaced components.
struct MassArgs {
  const uint32_t *offsets;  // [nelem][P^3] (flagged)
  const double *x;          // the input L-vector, interlaced [node][3] (apply; the diagonal reads none)
  const double *qdata;      // [nelem][10][Q^3]: component 0 (w det J) is the only one read
  double *evec;             // element results [elem][P^3][3], plain coalesced stores; launch_assemble() sums them per node in element order
  int nelem;
  int mask_in;              // apply: flagged components of the input read as zero
  int mask_out;             // diagonal: flagged rows are stored as zeros (the apply leaves its masked rows to launch_assemble's row flags)
  double coef;              // the QFunction context c, read by the host at every apply
};

// The density field of the mass operator (QFunction "MassField"; k_mass's modes MASS_APPLY_RHO and MASS_DIAG_RHO), a struct of its own
// beside MassArgs, whose layout the kernels without a field keep.
struct MassFieldArgs {
  const double *rho;            // the scalar density vector; its address is the launch argument, so a recording sees new values behind it
  const uint32_t *rho_offsets;  // [nelem][P^3] plain indices into rho: no Dirichlet flags, no factor 3
};

// Stress recovery (kernels_stress.hip, k_stress): the Cauchy stress the residual integrates (qfunctions_device.hpp, qf_stress), six
// components in the order xx, yy, zz, yz, xz, xy, from the displacement L-vector read AS IT IS (boundary values included, no mask).
struct StressArgs {
  const uint32_t *offsets;  // [nelem][P^3]; Dirichlet flags in the top bits, if any, are stripped and never honoured
  const double *x;          // the displacement L-vector, interlaced [node][3]
  const double *qdata;      // [nelem][10][Q^3]
  double *out;              // points: [nelem][6][Q^3], plain coalesced stores.  nodal: the element results [nelem][7][P^3] of
                            // B^T (w det J {sigma, 1}), the E-layout of the output restriction; launch_rstr_transpose() sums them per node
  int nelem;
  int model;                // 0 linElas, 1 hyperSS, 2 hyperFS: wave-uniform, read at run time
  double nu, E, lambda, TwoMu;
};

// The temperature field of the thermal loads and of the stress with a thermal term (QFunctions "ThermalForce", "ThermalTangent",
// "{LinElas,HyperSS,HyperFS}StressThermal"; k_stress's modes 2 .. 5), a struct of its own beside StressArgs, whose layout the kernels
// without a field keep.  The two load modes store element results [nelem][P^3][3] into StressArgs::out, which launch_assemble() sums.
struct ThermalArgs {
  const double *theta;            // the scalar temperature change; its address is the launch argument, so a recording sees new values behind it
  const uint32_t *theta_offsets;  // [nelem][P^3] plain indices into theta: no Dirichlet flags, no factor 3
  double beta;                    // E alpha / (1 - 2 nu), formed on the host at every apply
  const double *dx;               // tangent: the variation, an L-vector interlaced [node][3], read through StressArgs::offsets
  int mask_in;                    // tangent: flagged components of dx read as zero (the flags ride in StressArgs::offsets)
  int mask_out;                   // the loads: flagged rows are dropped -- by launch_assemble's row flags, not by the kernel
};

// Each returns hipSuccess or the launch error; `name` receives a static string
// naming the instantiation, or the call returns hipErrorInvalidValue when the
// (P, Q, qf) combination is not instantiated.
hipError_t launch_fused_grad(int P, int Q, int qf, const BasisTables &t, const FusedGradArgs &a, FusedLaunch l, hipStream_t s, const char **name);
// The Jacobian operators with the mass term, K + a.mass_c M, in the same launch (k_fused_pencil_mass; name "fused_grad<P=..,Q=..,<QF>+mass>/pencil").
// Instantiated for the Jacobian functors of every (P, Q) of the fused kernel up to Q = FUSED_MASS_QMAX; elsewhere hipErrorInvalidValue, the name empty.
constexpr int FUSED_MASS_QMAX = 7;
constexpr bool fused_mass_instantiated(int P, int Q, int qf) {
  return Q >= 2 && Q <= FUSED_MASS_QMAX && P >= 2 && P <= Q &&
         (qf == QF_LINELAS || qf == QF_HYPERSS_DF || qf == QF_HYPERFS_DF || (qf == QF_HYPERFS_DF_DS && pencil_derived_state(Q)));
}
hipError_t launch_fused_mass(int P, int Q, int qf, const BasisTables &t, const FusedGradArgs &a, FusedLaunch l, hipStream_t s, const char **name);
hipError_t launch_transfer(int Pc, int Pf, bool prolong, const BasisTables &t, const TransferArgs &a,
                           hipStream_t s, const char **name);
hipError_t launch_setup_geo(int Q, const BasisTables &t, const SetupGeoArgs &a, hipStream_t s,
                            const char **name);
hipError_t launch_diag(int P, int Q, int qf, const BasisTables &t, const DiagArgs &a, hipStream_t s,
                       const char **name);
hipError_t launch_state_at_points(int Pf, int Qc, const BasisTables &t, const StateArgs &a, hipStream_t s,
                                  const char **name);
// diag: `t.interp` holds the entry-wise SQUARED table; names "mass<P,Q>" / "mass_diag<P,Q>"; the pairs of CPS_DIAG_PQ (kernel_diag_sf.hpp)
hipError_t launch_mass(int P, int Q, bool diag, const BasisTables &t, const MassArgs &a, hipStream_t s, const char **name);
// the same operator with the density field: `t.interp` is the PLAIN table in both forms (the diagonal squares it while staging); names
// "mass_field<P,Q>" / "mass_field_diag<P,Q>"; the pairs of CPS_DIAG_PQ
hipError_t launch_mass_field(int P, int Q, bool diag, const BasisTables &t, const MassArgs &a, const MassFieldArgs &f, hipStream_t s, const char **name);
// names "stress<P=..,Q=..,points>" / "stress<P=..,Q=..,nodal>"; the pairs of CPS_DIAG_PQ
hipError_t launch_stress(int P, int Q, bool nodal, const BasisTables &t, const StressArgs &a, hipStream_t s, const char **name);
// the modes with a temperature field (`mode`: THERMAL_MODE_*, the values of kernels_stress.hip's StressMode); names "thermal_force<P=..,Q=..>",
// "thermal_tangent<P=..,Q=..>", "stress<P=..,Q=..,points+thermal>", "stress<P=..,Q=..,nodal+thermal>"; the pairs of CPS_DIAG_PQ
enum ThermalMode : int { THERMAL_MODE_FORCE = 2, THERMAL_MODE_TANGENT = 3, THERMAL_MODE_POINTS = 4, THERMAL_MODE_NODAL = 5 };
hipError_t launch_stress_thermal(int P, int Q, int mode, const BasisTables &t, const StressArgs &a, const ThermalArgs &th, hipStream_t s, const char **name);

// The instantiations of one quadrature size are compiled as pencil_inst_parts(Q) objects (kernels_fused_inst.hip, -DCPS_PART=<k>): the kernels
// with (Q - P) % parts == k -- the Q = 8 object alone took 72 s of a 90 s build.  csrc/Makefile lists the same parts.
constexpr int pencil_inst_parts(int Q) { return Q == 8 ? 4 : (Q == 7 ? 2 : 1); }
// elements per wave (= per group) of the pencil kernel, PencilGeom<P, Q>::E: 3 Q^2 pencils per element and pass against 64
// lanes and the 9 Q^3-double LDS slab per element
// (Q = 5: two; one element per wave was 8-25 % slower, profiles/r03_ab_experiments.txt item 12)
constexpr int pencil_group_elems(int Q) { return Q <= 2 ? 8 : (Q <= 4 ? 4 : (Q == 5 ? 2 : 1)); }
// LDS of one wave: PencilGeom<P, Q>::LDS_BYTES, as the launcher asserts.  No P in it: the persistent waves a CU holds -- what its 160 KB of LDS
// take, at most the 4 x PENCIL_MINW the registers allow -- depend on Q alone, and the host sizes a full launch itself (choose_pipe).
constexpr int PENCIL_MINW = 2;   // waves per SIMD the register allocation is held to (256 VGPRs), at every Q (a Q = 5 value of its own: profiles/r05_ab_experiments.txt item 13)
constexpr int pencil_lds_bytes(int Q) { return (pencil_group_elems(Q) * (9 * Q * Q * Q + (Q == 5 ? 5 : 1) + GEO_NCOEF) + 2 * Q) * 8; }
constexpr int pencil_waves_per_cu(int Q) {   // 1 ... 4 x PENCIL_MINW: 8 waves per CU = 2 per SIMD at <= 256 VGPRs
  const int by_lds = (160 * 1024) / pencil_lds_bytes(Q); return by_lds < 1 ? 1 : (by_lds > 4 * PENCIL_MINW ? 4 * PENCIL_MINW : by_lds);
}

// The transpose map of a restriction as the kernels read it: rows [row0, row0 + nnodes) of rowptr / node_off, the contributors
// of row r being cols[rowptr[r] .. rowptr[r + 1]).  Made by RowMap::view() (ceed_impl.hpp) of whichever map the apply sums.
// The STENCIL CODE of the same rows (row_code.hpp), read by k_assemble and k_assemble_epi in place of rowptr / cols where `sid` is set:
// contributor j of row r at pos0[r] + distance j of stencil sid[r]; rows with the escape id take rowptr / cols.
struct NodeMap {
  const uint32_t *rowptr, *cols, *node_off;
  int nnodes, row0;
  const uint32_t *pos0 = nullptr;
  const uint16_t *sid = nullptr;
  const uint32_t *stencil = nullptr;     // [stencils][8]: RowStencil
  NodeMap rows(int first, int n) const { NodeMap m = *this; m.row0 = first; m.nnodes = n; return m; }
};
// Deterministic, atomic-free E^T (kernels_assemble.hip): y[node_off[r] + c] (+)= sum over the node's contributors, in element
// order, of E[3 * cols[k] + c] (cols[k] = e * P3 + n).  `flags` (one byte per node of the whole map, bit c = component c constrained) may be null.
// `unpack` (may be null): the arrivals of a halo exchange, added to y by extra workgroups of the SAME launch (one launch
// less on the critical path of a split-phase apply): y[dst[u]] += recv[slot[k]], k in [ptr[u], ptr[u+1]), in list order.
struct HaloUnpackArgs { const uint32_t *dst, *ptr, *slot; const double *recv; int n; };
// `pack` (may be null): the pack of a halo exchange folded into the rows' launch -- row r's finished sums also go to
// send[slot[k] & 0x3FFFFFFF], component slot[k] >> 30, k in [ptr[r], ptr[r+1]) (ptr, like `flags`, over the rows of the whole map).
struct HaloPackFold { const uint32_t *ptr, *slot; double *send; };
hipError_t launch_assemble(const NodeMap &m, const unsigned char *flags, const double *evec, double *y, int add, hipStream_t s,
                           const HaloUnpackArgs *unpack = nullptr, const HaloPackFold *pack = nullptr);

// The same sum with an epilogue in place of the store of y (k_assemble_epi): the output of a fused apply consumed
// where it is formed -- a Chebyshev step or the residual b - A v.
enum EpilogueKind : int { EPI_NONE = 0, EPI_CHEB = 1, EPI_RESID = 2 };
struct EpilogueArgs {
  int kind;
  const double *t;          // the apply's output vector: holds the ELEMENT-INTERIOR nodes' values (stored by the fused kernel) only
  const uint32_t *int_off;  // node offsets of the element-interior nodes handled by this launch, n_int of them (0: none)
  int n_int;
  // EPI_CHEB: r = (r0 ? r0 : r) - t (stored if r is given; r0 = the right-hand side b: the residual recomputed, not recurred);
  //           d = c1 dinv r + c2 d;  x = assign_x ? d : x + d
  double *x, *d, *r;
  const double *r0, *dinv;
  double c1, c2;
  int assign_x;
  // EPI_RESID: w = b - t
  double *w;
  const double *b;
};
hipError_t launch_assemble_epi(const NodeMap &m, const unsigned char *flags, const double *evec, const EpilogueArgs &ep, hipStream_t s);

// Surface loads on element faces (kernels_surface.hip, k_surface): per face the P^2 nodal values of one of three geometric vectors,
//   traction  g_a = int N_a t |X_xi x X_eta|,   pressure  g_a = int N_a (x_xi x x_eta),   tangent  T du |_a = int N_a (du_xi x x_eta + x_xi x du_eta),
// x = X + u, (xi, eta) the two in-face directions (xi fastest in the face's node list) with X_xi x X_eta pointing out of the body.
// The face mapping and the passes it shares with k_contact: kernel_face_pass.hpp.
// Five further kinds vary over the faces (k_surface<P, Q, true>, launch_surface_field).  With t_h, p_h, x_h, du_h the nodal values at
// the point, e = up, d = level - e . x_h, <d> = max(d, 0), H(d) = 1 for d > 0 and 0 otherwise, per face
//   traction field    g_a = sum_q w_q N_a t_h |X_xi x X_eta|       pressure field  g_a = sum_q w_q N_a p_h (x_xi x x_eta)
//   hydrostatic       g_a = sum_q w_q N_a gamma <d> (x_xi x x_eta)
//   and the two followers' tangents: p_h (du_xi x x_eta + x_xi x du_eta);  gamma [<d> (du_xi x x_eta + x_xi x du_eta) - H(d) (e . du_h) (x_xi x x_eta)].
// The discrete forms are DEFINED by these sums (at Q = P they are not exact integrals for p >= 3); each tangent is their derivative.
enum SurfaceKind : int { SURF_TRACTION = 0, SURF_PRESSURE = 1, SURF_TANGENT = 2,
                         SURF_TRACTION_FIELD = 3, SURF_PRESSURE_FIELD = 4, SURF_PRESSURE_FIELD_TANGENT = 5, SURF_HYDRO = 6, SURF_HYDRO_TANGENT = 7 };
struct SurfaceArgs {
  const uint32_t *offsets;  // [nface][P^2] component-0 L-offsets, the Dirichlet flags of their nodes in the top bits
  const double *X;          // node coordinates, an L-vector interlaced [node][3]
  const double *u;          // displacement (pressure, tangent) or null: the reference configuration; read as it is (boundary values)
  const double *du;         // tangent: the variation; flagged components read as zero
  double *evec;             // face results [face][P^2][3], plain coalesced stores; launch_surface_sum() adds them into y
  int nface, kind;
  double coef[3];           // scale x t (traction); scale x p in coef[0] (pressure, tangent); scale (x gamma) in coef[0] (the field kinds)
};
// what the field kinds take besides (an argument type of their own: the kernels of the three kinds above keep their argument block)
struct SurfaceFieldArgs : SurfaceArgs {
  const double *field;      // traction field: an L-vector read at the offsets; pressure field: a value per node, read at offset / 3
  double level, up[3];      // hydrostatic: the level of the fluid along the UNIT vector up (gamma rides in coef[0])
};
// hipErrorInvalidValue with *name left empty when (P, Q) is not instantiated: P = 2 .. 8, Q = P .. min(P + 2, 8)
hipError_t launch_surface(int P, int Q, const BasisTables &t, const SurfaceArgs &a, hipStream_t s, const char **name);
// the field kinds (a.kind >= SURF_TRACTION_FIELD), same pairs; *name is "surface_field<P=..,Q=..>"
hipError_t launch_surface_field(int P, int Q, const BasisTables &t, const SurfaceFieldArgs &a, hipStream_t s, const char **name);
bool surface_instantiated(int P, int Q);
// y[node_off[r] + c] += the sum of row r's face contributions in face order (node_sum3), one read-modify-write per row of the face
// transpose map; components flagged in `flags` (a byte per row, may be null) are skipped, rows off the faces are never touched
hipError_t launch_surface_sum(const NodeMap &m, const unsigned char *flags, const double *evec, double *y, hipStream_t s);

// Frictionless penalty contact of element faces with a rigid obstacle (kernels_contact.hip, k_contact): g(x) the signed distance to the
// obstacle (g > 0: separated), n = grad g, x = X + u, J = |X_xi x X_eta|, eps the penalty per unit REFERENCE area.  Per face
//   residual  r_a      = -sum_q N_a(q) w_q J_q eps <-g> n                             and the state K_q, g per point (below)
//   tangent   C du |_a =  sum_q N_a(q) K_q du(q),   K_q = w_q J_q eps [H(-g) n (x) n - <-g> grad grad g]
//   diagonal  d_{a,c}  =  sum_q N_a(q)^2 K_q[c][c]                                    (the tables come entry-wise squared)
// in a face E-vector [face][P^2][3] that launch_surface_sum() adds into y.  The tangent and the diagonal read the state alone.
// Mapping and passes: kernel_face_pass.hpp, as for k_surface.
// Two further modes serve the spring and dashpot supports (ceed_support.cpp), whose K_q = w_q J_q [k_t I + (k_n - k_t) n (x) n] with
// n = X_xi x X_eta / J is fixed in the reference configuration: SUPPORT_STATE gathers X alone and writes that K_q per point, entry 6
// being w_q J_q (no E-vector, no node sum); SUPPORT_FORCE is the tangent's data path on an input read AS IT IS, boundary values included.
// A support's tangent and diagonal are CONTACT_TANGENT and CONTACT_DIAGONAL on the support state.
enum ContactMode : int { CONTACT_RESIDUAL = 0, CONTACT_TANGENT = 1, CONTACT_DIAGONAL = 2, CONTACT_SUPPORT_STATE = 3, CONTACT_SUPPORT_FORCE = 4 };
enum ContactObstacle : int { CONTACT_PLANE = 0, CONTACT_SPHERE = 1 };
constexpr int CONTACT_NSTATE = 7;   // K_q as (xx, yy, zz, yz, xz, xy), then the gap g
struct ContactArgs {
  const uint32_t *offsets;  // [nface][P^2] component-0 L-offsets, the Dirichlet flags of their nodes in the top bits
  const double *X;          // residual, support state: node coordinates, an L-vector interlaced [node][3]
  const double *u;          // residual: displacement, read as it is (boundary values)
  const double *du;         // tangent: the variation; flagged components read as zero.  Support force: the field, read as it is
  double *state;            // [nface][7][Q^2]: written by the residual (the support state), read by the tangent, the diagonal and the support force
  double *evec;             // face results [face][P^2][3], plain coalesced stores
  int nface, kind;          // kind: ContactObstacle, uniform over the launch (residual)
  double par[8];            // plane: x0[3], n[3] (unit, from the obstacle to the body); sphere: c[3], R, s = +1 (ball) / -1 (cavity);
                            // support state: k_n, k_t
  double penalty, scale;    // eps (residual: it is inside the stored K_q); the caller's factor on the face results (never on the state)
};
// hipErrorInvalidValue with *name left empty when (P, Q) is not instantiated: the pairs of CPS_DIAG_PQ (P = 2 .. 8, Q = P .. 8);
// names "contact<P=..,Q=..,residual|tangent|diagonal|support_state|support_force>".  `t.interp` of the diagonal holds the entry-wise SQUARED table.
hipError_t launch_contact(int P, int Q, int mode, const BasisTables &t, const ContactArgs &a, hipStream_t s, const char **name);
bool contact_instantiated(int P, int Q);

// Coordinate-driven set-up operators (kernels_coord.hip): opSetupForce and opTrue of setuplibceed.c:555-623.  The 1-D tables of the output
// (displacement) basis come by value (BasisTables, forcing only); the element results go to `evec` in the E-layout [elem][3][Pout^3] of the
// output restriction, whose transpose (launch_rstr_transpose) sums them into the L-vector.
struct CoordOpArgs {
  const uint32_t *off_x;   // [nelem][8] coordinate restriction
  const double *xcoord;    // interlaced [vertex][3]
  double *evec;            // element results, [nelem][3][Pout^3]
  const double *qdata;     // [nelem][10][Q^3] (forcing) or null (true solution)
  int nelem, Q, Pout, mode;  // mode 0: SetupConstantForce, 1: SetupMMSForce, 2: MMSTrueSoln
  double ctx[3];           // direction (mode 0)
  double lambda, TwoMu;    // mode 1: the Lame constants of (nu, E), formed on the host (lame_constants)
  double bx[MAXN1D * 2];   // coordinate basis interp1d, Q x 2
};
hipError_t launch_coord_op(const BasisTables &t, const CoordOpArgs &a, hipStream_t s);
// Strain-energy operator (kernels_coord.hip): opEnergy of setuplibceed.c:651-670.  The tables are the displacement basis's, which the
// energy basis shares (op_plan compares them).
struct EnergyOpArgs {
  const uint32_t *off_u;   // [nelem][P^3] displacement restriction (3 interlaced components)
  const double *u;         // displacement L-vector
  double *evec;            // element results: [nelem][1][P^3] (energy) or [nelem][8][Q^3] (diagnostic), E-layout of the output restriction
  const double *qdata;     // [nelem][10][Q^3]
  int nelem, Q, P, model;  // model 0: LinElas, 1: HyperSS, 2: HyperFS
  int diag;                // 0: *Energy -> 1 component through INTERP^T; 1: *Diagnostic (opDiagnostic, setuplibceed.c:712-737)
                           // -> 8 components collocated with the points
  double nu, E, lambda, TwoMu;
};
hipError_t launch_energy_op(const BasisTables &t, const EnergyOpArgs &a, hipStream_t s);

// Interface-dof halo exchange (CeedXHalo*, the L-vector sum of src/matops.c:57 across GPUs).  ONE launch packs the entries
// of all neighbour lists into the (contiguous) send buffer; ONE launch adds all arrivals: a thread per distinct destination
// entry adds that entry's arrivals in neighbour-list order (no atomics; the sum is reproducible).
hipError_t launch_halo_pack(const uint32_t *idx, int n, const double *y, double *buf, hipStream_t s);
hipError_t launch_halo_unpack_add(const HaloUnpackArgs &u, double *y, hipStream_t s);

// Assembled coarse-level operator (kernels_csr.hip).
hipError_t launch_csr_sum(const uint32_t *slotptr, const uint32_t *perm, const double *coo, double *vals, int nnz,
                          const uint32_t *unit_diag_slot, int n_unit, hipStream_t s);
// y = A x, CSR-stream form: row_block[b] .. row_block[b + 1] are consecutive rows with at most 2048 entries in all (a longer row is a run of its
// own), at most 256 rows per run; cut by csr_row_blocks() on the host
hipError_t launch_csr_spmv_stream(const uint32_t *row_block, int nblocks, const uint32_t *rowptr, const uint32_t *cols, const double *vals,
                                  const double *x, double *y, hipStream_t s);
hipError_t launch_csr_diag(const uint32_t *diag_slot_of_row, const double *vals, double *d, int nrows, hipStream_t s);
hipError_t launch_csr_spgemm(const uint32_t *l_rowptr, const uint32_t *l_cols, const double *l_vals, const uint32_t *r_rowptr,
                             const uint32_t *r_cols, const double *r_vals, const uint32_t *c_rowptr, const uint32_t *c_cols, double *c_vals,
                             int nrows, hipStream_t s, int dense_ncols = 0, int max_row_c = 0);   // C = L R on fixed patterns (R's columns sorted within each row);
                             // dense_ncols > 0: C is a dense row-major nrows x dense_ncols matrix (LDS row accumulation);
                             // max_row_c > 0: the longest row of C -- up to 4096 entries a wave per row with an LDS accumulator (k_csr_spgemm_row)
hipError_t launch_dense_spd_inverse(double *A, int n, double *scratch /* 1024 doubles */, int *info, hipStream_t s);

// Vector utilities (kernels_vector.hip) and the plain restriction (kernels_assemble.hip).
hipError_t launch_set_value(double *v, size_t n, double val, hipStream_t s);
hipError_t launch_waxpby(double *w, double a, const double *x, double b, const double *y, size_t n, hipStream_t s);
hipError_t launch_cheb_update(double *x, double *d, double *r, const double *r0, const double *t, const double *dinv, double c1, double c2,
                              int assign_x, size_t n, hipStream_t s);
hipError_t launch_reciprocal(double *v, size_t n, hipStream_t s);
hipError_t launch_pointwise_mult(double *w, const double *x, const double *y, size_t n, hipStream_t s);
hipError_t launch_axpby(double *y, double a, const double *x, double b, size_t n, hipStream_t s);
hipError_t launch_masked_copy(double *dst, const double *src, const unsigned char *mask, size_t n,
                              hipStream_t s);  // dst = mask ? 0 : src
hipError_t launch_rstr_gather(const uint32_t *off, int nelem, int elemsize, int ncomp, int compstride,
                              const double *l, double *e, hipStream_t s);
// v += E^T u (add) or v = E^T u (store; entries no element holds are left) for the E-layout [elem][comp][node], and the number of
// contributors of every entry some element holds: a lane per (row of the restriction's transpose map, component), no atomics
hipError_t launch_rstr_transpose(const NodeMap &m, int elemsize, int ncomp, int compstride, const double *e, double *l, int add, hipStream_t s);
hipError_t launch_multiplicity(const NodeMap &m, int ncomp, int compstride, double *l, hipStream_t s);
hipError_t launch_dot(const double *x, const double *y, const double *w, size_t n, double *result_dev,
                      hipStream_t s, double *out = nullptr);  // result_dev[0] (and *out) = sum w_i x_i y_i (w may be null), reproducibly; result_dev: 1 + 2048 doubles
hipError_t launch_scalar_div(double *sc, int dst, int num, int den, double scale, hipStream_t s);
hipError_t launch_axpby_dev(double *y, const double *sc, int ia, double sa, const double *x, int ib, double sb, size_t n, hipStream_t s);

// Block vectors (kernels_block.hip): k columns of length n in one array, column j at element j * ld (ld >= n).  A and B point at the first
// column of their ranges.  G (ka x kb, row-major, device) = sum_r w[r] A_i[r] B_j[r] (w may be null) through per-workgroup partial
// matrices in `part` (BLOCK_GRAM_MAX_PARTS x ka x kb doubles) summed in a fixed order; Y_j = sum_i A_i C[i][j] + beta Y_j with C (ka x ky,
// row-major) on the device.  A row chunk of the Gram kernel is BLOCK_GRAM_ROWS rows; its grid is at most BLOCK_GRAM_MAX_PARTS workgroups.
constexpr int BLOCK_MAX_COLS = 48;
constexpr int BLOCK_GRAM_ROWS = 64;
constexpr int BLOCK_GRAM_MAX_PARTS = 1024;
constexpr int BLOCK_COMBINE_ROWS = 512;          // rows of a chunk of the combination: two per lane
constexpr int BLOCK_COMBINE_MAX_GROUPS = 2048;   // its largest grid
hipError_t launch_block_gram(const double *A, int ka, const double *B, int kb, const double *w, size_t n, size_t ld, double *part,
                             double *G, hipStream_t s);
hipError_t launch_block_combine(double *Y, int ky, const double *A, int ka, const double *C, double beta, size_t n, size_t ld,
                                hipStream_t s);

// The explicit time step (kernels_explicit.hip; formulas: include/ceed.h, CeedXVectorLeapfrogStep) on the first n rows: f may be null;
// with out the kinetic-energy tally goes to *out (device) through `part`, one double per workgroup of the streaming grid (at most 2048:
// stream_grid), summed in a fixed order; without out no reduction is launched.  n >= 1.
hipError_t launch_leapfrog(double *x, double *vh, const double *r, const double *f, const double *m, double load, double c1, double c2,
                           double dt, size_t n, double *part, double *out, hipStream_t s);

}  // namespace cps
