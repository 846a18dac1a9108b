/*
 * ceed.h -- C-ABI boundary of the MI355X-native operator-apply backend.
 *
 * This is the drop-in boundary named in BASELINE.json's north_star: the subset
 * of the public libCEED (v0.7-era) C interface that ArashMehraban/CeedPetscSolid
 * binds for its residual / Jacobian / p-multigrid-transfer / diagonal path.
 * The mini-app's own translation units (`src/setuplibceed.c`, `src/matops.c`,
 * `src/misc.c`, `elasticity.c`) and its `qfunctions/ *.h` compile against this
 * header unchanged (`#include <ceed.h>`, reference elasticity.h:24), and link
 * against either
 *
 *   ceedpetscsolid_amd/csrc/libceed_mi355x.so   (the product: resource
 *                                                "/gpu/hip/mi355x", hand-written
 *                                                gfx950 kernels), or
 *   oracle/liboracle_ceed.so                     (TEST INFRASTRUCTURE ONLY: the
 *                                                plain-C CPU restatement,
 *                                                resource "/cpu/self/oracle").
 *
 * Every entry point returns 0 on success.  Because the reference never checks
 * a Ceed return code (e.g. src/matops.c:40-50) every failure also goes through
 * an aborting error handler: the message is printed to stderr and abort() is
 * called, unless CeedSetErrorReturn() (extension, below) was used to ask for
 * plain error returns (the Python tests do, so that pytest can see them).
 *
 * Each declaration cites the reference call site(s) it serves.
 * Plain pointers and sizes only; no C++/torch types cross this boundary.
 */
#ifndef CEED_MI355X_CEED_H
#define CEED_MI355X_CEED_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
#  define CEED_EXTERN extern "C"
#else
#  define CEED_EXTERN extern
#endif
/* Entry points a backend of this ABI MAY leave out (same linkage): a caller looks */
/* the symbol up in the loaded library and takes the portable path without it.     */
#define CEED_EXTERN_OPTIONAL CEED_EXTERN

/* ------------------------------------------------------------------------- */
/* Scalar / index types (f64 data, int32 indices)                   */
/* ------------------------------------------------------------------------- */
typedef int32_t CeedInt;
typedef double  CeedScalar;

/* QFunction-side helper macros used by qfunctions/ *.h                       */
/*   CEED_QFUNCTION(name): defines the "file:name" locator string `name_loc`  */
/*   (consumed at setuplibceed.c:49-53) and opens the static callback.        */
#ifndef CEED_QFUNCTION
#  define CEED_QFUNCTION(name) \
     static const char name ## _loc[] = __FILE__ ":" #name; \
     static int name
#endif
#ifndef CEED_Q_VLA
#  define CEED_Q_VLA Q
#endif
#ifndef CeedPragmaSIMD
#  if defined(_OPENMP) || defined(__clang__) || defined(__GNUC__)
#    define CeedPragmaSIMD _Pragma("GCC ivdep")
#  else
#    define CeedPragmaSIMD
#  endif
#endif

/* ------------------------------------------------------------------------- */
/* Opaque handles                                                             */
/* ------------------------------------------------------------------------- */
typedef struct Ceed_private                *Ceed;
typedef struct CeedRequest_private         *CeedRequest;
typedef struct CeedVector_private          *CeedVector;
typedef struct CeedElemRestriction_private *CeedElemRestriction;
typedef struct CeedBasis_private           *CeedBasis;
typedef struct CeedQFunction_private       *CeedQFunction;
typedef struct CeedOperator_private        *CeedOperator;

/* ------------------------------------------------------------------------- */
/* Enums                                                                      */
/* ------------------------------------------------------------------------- */
typedef enum { CEED_MEM_HOST = 0, CEED_MEM_DEVICE = 1 } CeedMemType;
typedef enum { CEED_COPY_VALUES = 0, CEED_USE_POINTER = 1,
               CEED_OWN_POINTER = 2 } CeedCopyMode;
typedef enum { CEED_NOTRANSPOSE = 0, CEED_TRANSPOSE = 1 } CeedTransposeMode;
typedef enum { CEED_EVAL_NONE = 0, CEED_EVAL_INTERP = 1, CEED_EVAL_GRAD = 2,
               CEED_EVAL_DIV = 4, CEED_EVAL_CURL = 8,
               CEED_EVAL_WEIGHT = 16 } CeedEvalMode;
typedef enum { CEED_GAUSS = 0, CEED_GAUSS_LOBATTO = 1 } CeedQuadMode;

/* Printable names, indexed by CeedMemType (elasticity.c:316-318).            */
CEED_EXTERN const char *const CeedMemTypes[];

/* ------------------------------------------------------------------------- */
/* Sentinels (setuplibceed.c:378-385, 531-539, 849-862; matops.c:46)          */
/* ------------------------------------------------------------------------- */
CEED_EXTERN const CeedVector          CEED_VECTOR_ACTIVE;
CEED_EXTERN const CeedVector          CEED_VECTOR_NONE;
CEED_EXTERN const CeedElemRestriction CEED_ELEMRESTRICTION_NONE;
CEED_EXTERN const CeedBasis           CEED_BASIS_COLLOCATED;
CEED_EXTERN const CeedQFunction       CEED_QFUNCTION_NONE;
CEED_EXTERN CeedRequest *const        CEED_REQUEST_IMMEDIATE;
CEED_EXTERN CeedRequest *const        CEED_REQUEST_ORDERED;
CEED_EXTERN const CeedInt             CEED_STRIDES_BACKEND[3];

/* ------------------------------------------------------------------------- */
/* Ceed (context)            elasticity.c:110-116, 308, 897-898               */
/* ------------------------------------------------------------------------- */
CEED_EXTERN int CeedInit(const char *resource, Ceed *ceed);
CEED_EXTERN int CeedDestroy(Ceed *ceed);               /* NULL-safe (:898)   */
CEED_EXTERN int CeedGetResource(Ceed ceed, const char **resource);
CEED_EXTERN int CeedGetPreferredMemType(Ceed ceed, CeedMemType *type);

/* ------------------------------------------------------------------------- */
/* CeedVector   matops.c:40-50,134-143,183-192,224-235,274-290;               */
/*              setuplibceed.c:326-328,355-361,601,626-639,808-809;           */
/*              misc.c:123-139; elasticity.c:243-244,292,300,782-798          */
/* ------------------------------------------------------------------------- */
CEED_EXTERN int CeedVectorCreate(Ceed ceed, CeedInt length, CeedVector *vec);
CEED_EXTERN int CeedVectorSetArray(CeedVector vec, CeedMemType mtype,
                                   CeedCopyMode cmode, CeedScalar *array);
CEED_EXTERN int CeedVectorTakeArray(CeedVector vec, CeedMemType mtype,
                                    CeedScalar **array /* may be NULL: a buffer of the library's own is then freed */);
CEED_EXTERN int CeedVectorSetValue(CeedVector vec, CeedScalar value);
CEED_EXTERN int CeedVectorSyncArray(CeedVector vec, CeedMemType mtype);
CEED_EXTERN int CeedVectorGetArray(CeedVector vec, CeedMemType mtype,
                                   CeedScalar **array);
CEED_EXTERN int CeedVectorGetArrayRead(CeedVector vec, CeedMemType mtype,
                                       const CeedScalar **array);
CEED_EXTERN int CeedVectorRestoreArray(CeedVector vec, CeedScalar **array);
CEED_EXTERN int CeedVectorRestoreArrayRead(CeedVector vec,
                                           const CeedScalar **array);
CEED_EXTERN int CeedVectorGetLength(CeedVector vec, CeedInt *length);
CEED_EXTERN int CeedVectorReciprocal(CeedVector vec);
CEED_EXTERN int CeedVectorDestroy(CeedVector *vec);    /* NULL-safe (:133)   */

/* ------------------------------------------------------------------------- */
/* CeedElemRestriction   setuplibceed.c:235-236 (offsets; constrained dofs    */
/*   already sign-decoded at :221-223), :304-318 (strided, backend layout),   */
/*   :326,626 (CreateVector), :628 + misc.c:123,278 (multiplicity)            */
/* ------------------------------------------------------------------------- */
CEED_EXTERN int CeedElemRestrictionCreate(Ceed ceed, CeedInt nelem,
    CeedInt elemsize, CeedInt ncomp, CeedInt compstride, CeedInt lsize,
    CeedMemType mtype, CeedCopyMode cmode, const CeedInt *offsets,
    CeedElemRestriction *rstr);
CEED_EXTERN int CeedElemRestrictionCreateStrided(Ceed ceed, CeedInt nelem,
    CeedInt elemsize, CeedInt ncomp, CeedInt lsize, const CeedInt strides[3],
    CeedElemRestriction *rstr);
CEED_EXTERN int CeedElemRestrictionCreateVector(CeedElemRestriction rstr,
    CeedVector *lvec /* or NULL */, CeedVector *evec /* or NULL */);
CEED_EXTERN int CeedElemRestrictionApply(CeedElemRestriction rstr,
    CeedTransposeMode tmode, CeedVector u, CeedVector ru, CeedRequest *request);
CEED_EXTERN int CeedElemRestrictionGetMultiplicity(CeedElemRestriction rstr,
    CeedVector mult);
CEED_EXTERN int CeedElemRestrictionDestroy(CeedElemRestriction *rstr);

/* ------------------------------------------------------------------------- */
/* CeedBasis   setuplibceed.c:335-348, 604, 782-803                           */
/* ------------------------------------------------------------------------- */
CEED_EXTERN int CeedBasisCreateTensorH1Lagrange(Ceed ceed, CeedInt dim,
    CeedInt ncomp, CeedInt P, CeedInt Q, CeedQuadMode qmode, CeedBasis *basis);
CEED_EXTERN int CeedBasisGetNumQuadraturePoints(CeedBasis basis, CeedInt *Q);
CEED_EXTERN int CeedBasisGetNumNodes(CeedBasis basis, CeedInt *P);
CEED_EXTERN int CeedBasisApply(CeedBasis basis, CeedInt nelem,
    CeedTransposeMode tmode, CeedEvalMode emode, CeedVector u, CeedVector v);
CEED_EXTERN int CeedBasisDestroy(CeedBasis *basis);
/* 1-D rules and tables (host copies; used by parity tests)                   */
CEED_EXTERN int CeedGaussQuadrature(CeedInt Q, CeedScalar *qref1d,
                                    CeedScalar *qweight1d);
CEED_EXTERN int CeedLobattoQuadrature(CeedInt Q, CeedScalar *qref1d,
                                      CeedScalar *qweight1d);
CEED_EXTERN int CeedBasisGetInterp1D(CeedBasis basis,
                                     const CeedScalar **interp1d);
CEED_EXTERN int CeedBasisGetGrad1D(CeedBasis basis, const CeedScalar **grad1d);
CEED_EXTERN int CeedBasisGetQWeights1D(CeedBasis basis,
                                       const CeedScalar **qweight1d);

/* ------------------------------------------------------------------------- */
/* CeedQFunction   setuplibceed.c:370-375,518-526,818-826; elasticity.c:249;  */
/*                 matops.c:215-232 (context swap for -nu_smoother)           */
/* ------------------------------------------------------------------------- */
typedef int (*CeedQFunctionUser)(void *ctx, const CeedInt Q,
                                 const CeedScalar *const *in,
                                 CeedScalar *const *out);
CEED_EXTERN int CeedQFunctionCreateInterior(Ceed ceed, CeedInt vlength,
    CeedQFunctionUser f, const char *source, CeedQFunction *qf);
CEED_EXTERN int CeedQFunctionCreateIdentity(Ceed ceed, CeedInt size,
    CeedEvalMode inmode, CeedEvalMode outmode, CeedQFunction *qf);
CEED_EXTERN int CeedQFunctionAddInput(CeedQFunction qf, const char *fieldname,
                                      CeedInt size, CeedEvalMode emode);
CEED_EXTERN int CeedQFunctionAddOutput(CeedQFunction qf, const char *fieldname,
                                       CeedInt size, CeedEvalMode emode);
/* ctx is borrowed: the pointer is kept and re-read at every apply.  The       */
/* reference passes sizeof(pointer) at setuplibceed.c:826, so `ctxsize` is    */
/* recorded but never trusted for the known QFunctions.       */
CEED_EXTERN int CeedQFunctionSetContext(CeedQFunction qf, void *ctx,
                                        size_t ctxsize);
CEED_EXTERN int CeedQFunctionDestroy(CeedQFunction *qf);

/* ------------------------------------------------------------------------- */
/* CeedOperator   setuplibceed.c:378-393,529-542,829-839,849-862;             */
/*                matops.c:46,138,187,227,277                                 */
/* ------------------------------------------------------------------------- */
CEED_EXTERN int CeedOperatorCreate(Ceed ceed, CeedQFunction qf,
    CeedQFunction dqf, CeedQFunction dqfT, CeedOperator *op);
CEED_EXTERN int CeedCompositeOperatorCreate(Ceed ceed, CeedOperator *op);
CEED_EXTERN int CeedCompositeOperatorAddSub(CeedOperator compositeop,
                                            CeedOperator subop);
CEED_EXTERN int CeedOperatorSetField(CeedOperator op, const char *fieldname,
    CeedElemRestriction r, CeedBasis b, CeedVector v);
/* Overwrites every output, passive ones included (residual's `gradu`).       */
CEED_EXTERN int CeedOperatorApply(CeedOperator op, CeedVector in,
                                  CeedVector out, CeedRequest *request);
CEED_EXTERN int CeedOperatorApplyAdd(CeedOperator op, CeedVector in,
                                     CeedVector out, CeedRequest *request);
/* Overwrites `assembled` (matops.c:227; Xloc is not zero on entry).          */
CEED_EXTERN int CeedOperatorLinearAssembleDiagonal(CeedOperator op,
    CeedVector assembled, CeedRequest *request);
CEED_EXTERN int CeedOperatorDestroy(CeedOperator *op);

/* ------------------------------------------------------------------------- */
/* Extensions (not in libCEED; prefixed CeedX).  None is needed by the        */
/* reference's call sites; they serve the harness, bench.py and the tests.    */
/* ------------------------------------------------------------------------- */
/* 0: abort on error (default, libCEED's behaviour);  1: return the code and  */
/* keep the message for CeedXLastError().                                     */
CEED_EXTERN int CeedXSetErrorReturn(int enable);
CEED_EXTERN const char *CeedXLastError(void);
/* Launch all device work of this Ceed on the given hipStream_t (as void*).   */
CEED_EXTERN int CeedXSetStream(Ceed ceed, void *hip_stream);
/* Block until all device work queued by this Ceed has finished.              */
CEED_EXTERN int CeedXSynchronize(Ceed ceed);
/* hipGraph capture of a launch-bound sequence (e.g. one multigrid V-cycle:   */
/* ~150 small kernels).  Between Begin and End every CeedOperatorApply /      */
/* CeedX vector helper on this Ceed is recorded instead of run; nothing that  */
/* needs the host (CeedXVectorDot, host array access, first-use setup) may be */
/* called, so run the sequence once eagerly first.  Scalars passed to the     */
/* recorded calls are baked in; vectors are referenced by device address.     */
/* Launch replays the recording on the Ceed's stream.                         */
typedef struct CeedXGraph_private *CeedXGraph;
CEED_EXTERN int CeedXGraphBeginCapture(Ceed ceed);
CEED_EXTERN int CeedXGraphEndCapture(Ceed ceed, CeedXGraph *graph);
CEED_EXTERN int CeedXGraphLaunch(CeedXGraph graph);
/* The staleness check of CeedXGraphLaunch without the launch (0: replayable). */
/* Local to the calling rank: several ranks agree on it before replaying a     */
/* graph that holds RCCL sends / receives.                                     */
CEED_EXTERN int CeedXGraphIsStale(CeedXGraph graph, int *stale);
CEED_EXTERN int CeedXGraphDestroy(CeedXGraph *graph);
/* Name of the kernel family an operator was lowered to, e.g.                 */
/* "fused_grad<P=5,Q=5,HyperFSdF>" (empty before the first apply).            */
CEED_EXTERN int CeedXOperatorGetKernelName(CeedOperator op, const char **name);
/* Fused BC handling for the MatShell wrappers (matops.c:33-34,56-57,106):    */
/* `mask` has one byte per L-vector entry of the operator's ACTIVE fields;    */
/* entries with mask!=0 are read as zero on input and dropped on output.      */
/* Pass NULL to clear.  Device or host pointer according to mtype; copied.    */
CEED_EXTERN int CeedXOperatorSetDirichletMask(CeedOperator op,
    CeedMemType mtype, const unsigned char *mask, CeedInt lsize);
/* General form: `mode` 1 = masked entries read as zero on input (matops.c:106 */
/* VecZeroEntries(Xloc)), 2 = masked rows dropped on output (matops.c:57       */
/* DMLocalToGlobal skips constrained dofs), 3 = both.  Transfer operators have */
/* different L-vectors on their two sides and take both masks.                 */
CEED_EXTERN int CeedXOperatorSetDirichletMaskMode(CeedOperator op,
    CeedMemType mtype, const unsigned char *mask_in, CeedInt lsize_in,
    const unsigned char *mask_out, CeedInt lsize_out, int mode);
/* Fine-side 1/multiplicity of the p-multigrid transfer operators, folded     */
/* into the fine scatter (Prolong_Ceed, matops.c:149) or gather               */
/* (Restrict_Ceed, matops.c:176).  NULL / CEED_VECTOR_NONE clears.            */
CEED_EXTERN int CeedXOperatorSetFineScale(CeedOperator op, CeedVector scale);
/* Split-phase apply, to hide the inter-GPU halo sum (the DMLocalToGlobal(ADD)  */
/* of matops.c:57) under the interior elements.  The first n_leading_elems      */
/* elements must be the only contributors of the L-vector nodes flagged in      */
/* `priority` (one byte per L-vector entry; all components of a node alike).    */
/* Phase 0 computes those elements and completes the flagged nodes, phase 1 the  */
/* rest; phase 0 followed by phase 1 equals CeedOperatorApply.  NULL clears.     */
CEED_EXTERN int CeedXOperatorSetOverlapSplit(CeedOperator op,
    CeedInt n_leading_elems, const unsigned char *priority, CeedInt lsize);
CEED_EXTERN int CeedXOperatorApplyPhase(CeedOperator op, CeedVector in,
                                        CeedVector out, int phase);
/* Stand-ins for the PETSc Vec calls of src/matops.c / src/misc.c on backend   */
/* memory: w = x .* y (VecPointwiseMult), y = a x + b y, weighted dot.        */
CEED_EXTERN int CeedXVectorPointwiseMult(CeedVector w, CeedVector x,
                                         CeedVector y);
CEED_EXTERN int CeedXVectorAXPBY(CeedVector y, double a, CeedVector x,
                                 double b);
CEED_EXTERN int CeedXVectorDot(CeedVector x, CeedVector y,
                               CeedVector weight /* or NULL */, double *result);
/* Scalars that stay in backend memory: a CeedVector as a register file, for  */
/* recurrences with a fixed number of steps (KSPChebyshevEstEig's Lanczos,    */
/* elasticity.c:546-549) without a host round trip per dot:                    */
/*   DotTo: scalars[idx] = sum weight .* x .* y;                               */
/*   ScalarDivide: scalars[dst] = scale * scalars[num] / scalars[den]          */
/*     (den < 0: no division; a non-positive denominator gives 0);             */
/*   AXPBYScalars: y = a x + b y, a = sa * scalars[ia], b = sb * scalars[ib];  */
/*     a negative index stands for the constant 1.                            */
CEED_EXTERN int CeedXVectorDotTo(CeedVector x, CeedVector y, CeedVector weight /* or NULL */,
                                 CeedVector scalars, CeedInt idx);
CEED_EXTERN int CeedXScalarDivide(CeedVector scalars, CeedInt dst, CeedInt num, CeedInt den, double scale);
CEED_EXTERN int CeedXVectorAXPBYScalars(CeedVector y, CeedVector scalars, CeedInt ia, double sa,
                                        CeedVector x, CeedInt ib, double sb);
/* OPTIONAL entry points: BLOCK vectors.  A block is k columns of length n in  */
/* one CeedVector, column j at element j * ld, ld >= n (column-major); the     */
/* rows n <= r < ld of a column are padding: never read into a result, never   */
/* written.  Column counts lie in 1 .. 48.  A column range [x0, x0 + kx) must  */
/* fit its vector: (x0 + kx) * ld - (ld - n) <= length.                        */
/*   BlockGram:    G[i][j] = sum_{r < n} weight[r] * A_{a0+i}[r] * B_{b0+j}[r], */
/*     i < ka, j < kb; G row-major, at least ka * kb long, stays in backend    */
/*     memory; weight NULL stands for ones and gives the same bits as a vector */
/*     of ones.  A and B may be the same vector with overlapping ranges.       */
/*     Every entry sums its rows in one fixed order: two calls give the same   */
/*     bits, and G(A, A) is symmetric bit for bit.                             */
/*   BlockCombine: Y_{y0+j}[r] = sum_{i < ka} A_{a0+i}[r] * C[i][j]             */
/*     + beta * Y_{y0+j}[r], j < ky, r < n; C row-major, at least ka * ky long, */
/*     in backend memory.  beta == 0 does not read Y.  The columns of Y must   */
/*     not overlap the columns of A (refused: the call is not in place).       */
/* Every argument is checked before anything is queued.  Both calls can be    */
/* recorded in a CeedXGraph.  BlockGetLimits reports the largest column count, */
/* the rows of one chunk of the Gram reduction, the largest number of partial  */
/* matrices it sums, the rows of one chunk of the combination and its largest  */
/* grid (any pointer may be NULL).                                             */
CEED_EXTERN_OPTIONAL int CeedXVectorBlockGram(CeedVector A, CeedInt a0, CeedInt ka, CeedVector B, CeedInt b0, CeedInt kb,
                                              CeedInt n, CeedInt ld, CeedVector weight /* or NULL */, CeedVector G);
CEED_EXTERN_OPTIONAL int CeedXVectorBlockCombine(CeedVector Y, CeedInt y0, CeedInt ky, CeedVector A, CeedInt a0, CeedInt ka,
                                                 CeedVector C, double beta, CeedInt n, CeedInt ld);
CEED_EXTERN_OPTIONAL int CeedXVectorBlockGetLimits(CeedInt *max_cols, CeedInt *gram_rows, CeedInt *gram_max_parts,
                                                   CeedInt *combine_rows, CeedInt *combine_max_groups);
/* OPTIONAL entry point: one leapfrog (central-difference) step of explicit    */
/* elastodynamics with a lumped mass, on the rows i < n with m[i] > 0:         */
/*     g  = load * f[i] - r[i]            (f NULL: g = -r[i])                  */
/*     q  = g / m[i]                                                           */
/*     vn = c1 * vh[i] + c2 * q                                                */
/*     vm = 0.5 * (vh[i] + vn)   (the velocity AT the step r belongs to)       */
/*     ke += m[i] * (vm * vm)                                                  */
/*     vh[i] = vn;   x[i] = x[i] + dt * vn                                     */
/* every operation rounded on its own, in the order written.  Rows with        */
/* m[i] <= 0 (constrained rows, a longer vector's tail) are neither written    */
/* nor summed, whatever r, f, vh hold there (NaN included).                    */
/* scalars[slot] = 0.5 * ke when scalars is given (a fixed summation order:    */
/* two calls give the same bits); with scalars NULL no reduction is launched.  */
/* c1 = (1 - alpha dt/2) / (1 + alpha dt/2), c2 = dt / (1 + alpha dt/2) carry  */
/* a mass-proportional damping alpha (the caller computes them).               */
/* Checked before anything is queued: x, vh, r, m are vectors; n >= 1 and      */
/* every vector holds at least n entries; x, vh, r, m, f are pairwise          */
/* distinct; 0 <= slot < length of scalars; scalars is none of the operands.   */
/* Only queues kernels on the Ceed's stream: it can be recorded in a           */
/* CeedXGraph (after one eager call with a tally, if the tally is recorded).   */
CEED_EXTERN_OPTIONAL int CeedXVectorLeapfrogStep(CeedVector x, CeedVector vh, CeedVector r, CeedVector f /* or NULL */,
                                                 CeedVector m, double load, double c1, double c2, double dt,
                                                 CeedInt n, CeedVector scalars /* or NULL */, CeedInt slot);
/* One Jacobi-Chebyshev smoother update in a single pass over the vectors     */
/* (the KSPCHEBYSHEV + PCJACOBI smoother of elasticity.c:539-552):            */
/*   r -= t (skipped if t is NULL);  d = c1 * dinv .* r + c2 * d;             */
/*   x = d if assign_x else x + d.                                            */
/* ALIAS RULE of Update, Start and Step alike: the outputs x, d and r are      */
/* pairwise distinct vectors, and none of them is t, dinv or b (an absent     */
/* vector aliases nothing).  Anything else is refused before a vector is       */
/* touched -- the entries work entry by entry in one pass, so an alias would   */
/* return success with a meaningless result.                                   */
CEED_EXTERN int CeedXVectorChebyshevUpdate(CeedVector x, CeedVector d, CeedVector r,
                                           CeedVector t /* or NULL */, CeedVector dinv,
                                           double c1, double c2, int assign_x);
/* First step of a sweep, without copying the right-hand side into r first:   */
/*   r = b - t (t may be NULL);  d = c1 * dinv .* r;  x = d if assign_x else  */
/*   x + d.  And w = a x + b y (VecWAXPY-like; the residual z = b - A x).     */
CEED_EXTERN int CeedXVectorChebyshevStart(CeedVector x, CeedVector d, CeedVector r, CeedVector b,
                                          CeedVector t /* or NULL */, CeedVector dinv,
                                          double c1, int assign_x);
CEED_EXTERN int CeedXVectorWAXPBY(CeedVector w, double a, CeedVector x, double b, CeedVector y);
/* A step with the residual recomputed from the right-hand side (t = A x_k):   */
/*   ri = b - t (t may be NULL);  d = c1 * dinv .* ri + c2 * d;  x = d or     */
/*   x + d;  ri is stored only if r is not NULL.                               */
CEED_EXTERN int CeedXVectorChebyshevStep(CeedVector x, CeedVector d, CeedVector r /* or NULL */, CeedVector b,
                                         CeedVector t /* or NULL */, CeedVector dinv, double c1, double c2, int assign_x);
/* The operator apply with its CONSUMER fused behind it (round 5): t = A in is  */
/* used where it is formed and never stored as a whole (t: scratch L-vector;  */
/* its contents afterwards are unspecified).  What the smoother and the       */
/* V-cycle of elasticity.c:539-552, 588-590 do with a Jacobian apply:         */
/*   ApplyChebyshev: r = (b or r) - A in;  d = c1 * dinv .* r + c2 * d;       */
/*     x = d if assign_x else x + d.  `in` may be d or x themselves.  With b  */
/*     (and in = x) the residual is RECOMPUTED from the iterate every step,   */
/*     as KSPCHEBYSHEV does, and r may be NULL (it is then not stored).       */
/*     Same bits as CeedOperatorApply + CeedXVectorChebyshevStep / Update.    */
/*   ApplyResidual: w = b - A in.                                             */
/* Single-rank L-vectors (no interface sum between the apply and its consumer).*/
CEED_EXTERN int CeedXOperatorApplyChebyshev(CeedOperator op, CeedVector in, CeedVector t, CeedVector x, CeedVector d,
                                            CeedVector r, CeedVector b /* or NULL */, CeedVector dinv,
                                            double c1, double c2, int assign_x);
/* Measurement aid: the shader clock (GHz) the device runs at WHILE the work   */
/* already queued on the Ceed's stream executes (a one-wave probe on a stream */
/* of its own, `spin_us` long).  bench.py reports it beside the timed blocks. */
CEED_EXTERN int CeedXClockProbe(Ceed ceed, int spin_us, double *ghz);
CEED_EXTERN int CeedXOperatorApplyResidual(CeedOperator op, CeedVector in, CeedVector t, CeedVector b, CeedVector w);
/* OPTIONAL entry point: a caller looks it up in the loaded library and, where */
/* it is absent, applies the operator itself with a scratch output (the same   */
/* stored state, by include/ceed.h calls alone).                               */
/* The stored state alone: for an operator of the residual's shape (du GRAD    */
/* active, qdata NONE, dv GRAD active, gradu NONE passive) write ONLY the      */
/* passive gradu output, the physical gradient of `u` at the points of the     */
/* operator's basis (hyperFS.h:215-220).  The basis may have more nodes than   */
/* points: the state of a coarse p-multigrid level on its own quadrature,      */
/* refreshed from the fine displacement.  The active output does not exist for */
/* this call; kernel name "state<Pf=..,Qc=..>".                                */
CEED_EXTERN_OPTIONAL int CeedXOperatorApplyState(CeedOperator op, CeedVector u);
/* OPTIONAL entry points: the mass term of a Jacobian operator.  With c != 0    */
/* the operator applies K + c M -- M the consistent mass matrix of its basis    */
/* and qdata, B^T (w det J) B on the three components, the "Mass" QFunction     */
/* with context c -- in the launches of K alone: the effective tangent          */
/* K + a0 rho M of an implicit Newmark step (c = a0 rho) without a second pass. */
/* The Dirichlet mask applies to the sum as it does to K: masked inputs read as */
/* zero, masked rows dropped (mask mode 3 of a mass operator).                  */
/*   SetMassTerm: Jacobian operators only (an operator that stores grad u, and  */
/*     every other kind, is refused).  c = 0 clears the term: the operator then */
/*     launches the kernels and gives the bits it gave before.  Every apply     */
/*     form carries the term -- CeedOperatorApply / ApplyAdd (serial and        */
/*     pipelined), CeedXOperatorApplyPhase, CeedXOperatorApplyChebyshev,        */
/*     CeedXOperatorApplyResidual (both with the bits of apply-then-step) and a */
/*     recorded CeedXGraph, which FREEZES the coefficient it was recorded with: */
/*     record again after changing the term.  CeedXOperatorApplyWithHalo        */
/*     refuses an operator with a term, whatever the halo (the interface sums   */
/*     of the mass operator were never run over ranks).                         */
/*     CeedOperatorLinearAssembleDiagonal and ...PointBlockDiagonal IGNORE the  */
/*     term: they return the diagonal of K, bit for bit; add c diag(M) from the */
/*     mass operator's own diagonal.                                            */
/*     Kernel name after an apply: "fused_grad<P=..,Q=..,<QF>+mass>/pencil".    */
/*   MassTermAvailable: *has = 1 where a kernel with the term is instantiated   */
/*     for this operator's (P, Q, QFunction), else 0 -- SetMassTerm with c != 0 */
/*     is then an error, and the caller keeps the two-pass form.                */
CEED_EXTERN_OPTIONAL int CeedXOperatorSetMassTerm(CeedOperator op, double c);
CEED_EXTERN_OPTIONAL int CeedXOperatorMassTermAvailable(CeedOperator op, int *has);
/* OPTIONAL entry point: does the QFunction `name` ("Mass", or a source string  */
/* "file:Mass") have a device functor in this library?  *has = 1 or 0.  A      */
/* caller looks the entry point up and, where it is absent or answers 0, takes */
/* its portable form (ceedpetscsolid_amd/mass.py for the mass operator).       */
/* The QFunction "Mass" (no call site in the reference, which is quasi-static):*/
/*   inputs   u      size 3   CEED_EVAL_INTERP  active                         */
/*            qdata  size 10  CEED_EVAL_NONE    passive (SetupGeo's output)    */
/*   output   v      size 3   CEED_EVAL_INTERP  active                         */
/*   context  one double c, borrowed and re-read at every apply (as Physics    */
/*            is); a missing context is an error                               */
/*   at every point  v = c * qdata[0] * u,  qdata[0] = w det J                 */
/* so the operator is y = c B^T (w det J) B x, component by component.  Input  */
/* and output share one offsets restriction (any offsets: 3 interlaced         */
/* components, element size P^3) and one basis with P <= Q; qdata is strided   */
/* 10 x Q^3.  CeedOperatorApply / ApplyAdd, alone or as a sub-operator of a    */
/* composite; CeedXOperatorSetDirichletMaskMode as for the Jacobian operators  */
/* (masked input reads as zero; masked rows are stored as zeros by Apply and   */
/* left alone by ApplyAdd).  CeedOperatorLinearAssembleDiagonal gives          */
/* diag_n = c sum_q B(q,n)^2 w det J(q) for all three components; the point-   */
/* block diagonal is refused.  The element results are summed per node in      */
/* element order: bit-reproducible.  After one eager apply the operator can be */
/* recorded in a CeedXGraph; c is a launch argument, so a recording keeps the  */
/* value it was made with -- record again after changing it.  Kernel names     */
/* "mass<P,Q>" and "mass_diag<P,Q>".                                           */
/* The QFunction "MassField" (no call site in the reference;                   */
/* ceedpetscsolid_amd/mass.py, MassOperator(..., density=)): the mass operator */
/* with a density FIELD,                                                       */
/*   inputs   u      size 3   CEED_EVAL_INTERP  active                         */
/*            rho    size 1   CEED_EVAL_INTERP  passive                        */
/*            qdata  size 10  CEED_EVAL_NONE    passive (SetupGeo's output)    */
/*   output   v      size 3   CEED_EVAL_INTERP  active                         */
/*   context  one double c, as for "Mass"                                      */
/*   at every point  v = c * rho * qdata[0] * u                                */
/* so y = c B^T (rho_h w det J) B x with rho_h(q) = sum_m N_m(q) rho(m), the   */
/* density interpolated with u's table.  u, v and qdata as for "Mass".  rho is */
/* on an offsets restriction with 1 component, u's element count and element   */
/* size P^3 (plain indices into the scalar vector: a continuous restriction    */
/* for a nodal field, offsets e P^3 + n for an element-discontinuous one) and  */
/* a 1-component basis with u's P, Q and interp table, entry by entry; its     */
/* vector is at least the restriction's L-size long.  Every departure is       */
/* refused with a message of its own before anything is queued.  Apply,        */
/* ApplyAdd, sub-operator of a composite, CeedXOperatorSetDirichletMaskMode    */
/* and CeedOperatorLinearAssembleDiagonal (diag_n = c sum_q B(q,n)^2 rho_h(q)  */
/* w det J(q)) as for "Mass"; the point-block diagonal is refused.  After one  */
/* eager apply the operator can be recorded in a CeedXGraph: c is frozen as    */
/* for "Mass", but rho's ADDRESS is the launch argument, so new values written */
/* behind the same device address are seen by a replay.  Kernel names          */
/* "mass_field<P,Q>" and "mass_field_diag<P,Q>".                               */
/* The QFunctions "LinElasStress", "HyperSSStress", "HyperFSStress" (no call   */
/* site in the reference; ceedpetscsolid_amd/postprocess.py, Stress): the      */
/* Cauchy stress THE RESIDUAL INTEGRATES, six components xx yy zz yz xz xy --  */
/* for LinElas with the shear entries of linElas.h:137-139 as written, mu e_ij */
/* with the tensor strain, half of Hooke's law.                                */
/*   inputs   du      size 9   CEED_EVAL_GRAD   active (displacement, P <= Q)  */
/*            qdata   size 10  CEED_EVAL_NONE   passive                        */
/*   output   stress  size 6   CEED_EVAL_NONE   active: at the points, on a    */
/*                    strided 6 x Q^3 restriction, no basis; every entry of    */
/*                    [elem][6][Q^3] is stored, ApplyAdd is refused            */
/*        or  stress  size 7   CEED_EVAL_INTERP active: w det J {sigma, 1}     */
/*                    through B^T, summed per node in element order, on an     */
/*                    offsets restriction with 7 interlaced components and a   */
/*                    7-component basis with du's P, Q and interp table; the   */
/*                    caller divides components 0..5 by component 6 (the nodal */
/*                    volume; 0 at a node no element holds)                    */
/*   context  Physics {nu, E}                                                  */
/* du is read as it is (boundary values included); the operator takes no       */
/* Dirichlet mask.  Kernel names "stress<P=..,Q=..,points>" / "...,nodal>".    */
/* The thermal QFunctions (no call site in the reference;                      */
/* ceedpetscsolid_amd/thermal.py, ThermalLoad; postprocess.py, Stress(thermal=)*/
/* ): a nodal temperature change theta from the stress-free state,             */
/* theta_h(q) = sum_m N_m(q) theta(m), beta = E alpha / (1 - 2 nu).            */
/* "ThermalForce": the residual of the coupling energy -beta theta_h tr eps    */
/* (models 0 linElas, 1 hyperSS) or -beta theta_h ln J (model 2 hyperFS),      */
/*   inputs   theta  size 1   CEED_EVAL_INTERP  active                         */
/*            qdata  size 10  CEED_EVAL_NONE    passive                        */
/*            du     size 9   CEED_EVAL_GRAD    passive: the displacement, read*/
/*                   as it is; optional, required iff the model is hyperFS     */
/*   output   dv     size 9   CEED_EVAL_GRAD    active                         */
/*   context  four doubles {nu, E, alpha, model}, borrowed, read at every apply*/
/*   at every point  dv = -beta theta_h w det J dXdx F^-T,  F = I | I + grad u */
/* "ThermalTangent": its derivative in the finite-strain model,                */
/*   inputs   ddu    size 9   CEED_EVAL_GRAD    active                         */
/*            du     size 9   CEED_EVAL_GRAD    passive                        */
/*            theta  size 1   CEED_EVAL_INTERP  passive                        */
/*            qdata  size 10  CEED_EVAL_NONE    passive                        */
/*   output   dv     size 9   CEED_EVAL_GRAD    active                         */
/*   at every point  dv = +beta theta_h w det J dXdx F^-T (grad ddu)^T F^-T    */
/* (symmetric); a context whose model is not 2 is refused.                     */
/* "LinElasStressThermal", "HyperSSStressThermal", "HyperFSStressThermal": the */
/* stress operators above with theta (size 1, CEED_EVAL_INTERP, passive) as    */
/* their second input and the context {nu, E, alpha}: sigma - beta theta_h I,  */
/* for HyperFS sigma - (beta theta_h / det F) I.                               */
/* dv, du and ddu share one offsets restriction with 3 interlaced components   */
/* and one basis, P <= Q.  theta is on an offsets restriction with 1 component,*/
/* that restriction's element count and element size P^3 (plain indices into   */
/* the scalar vector) and a 1-component basis with its P, Q and interp table;  */
/* its vector is at least the restriction's L-size long: the rules of rho in   */
/* "MassField".  Every departure is refused with a message of its own before   */
/* anything is queued.  Apply, ApplyAdd and CeedXOperatorSetDirichletMaskMode  */
/* (the mask of the DISPLACEMENT vector: masked rows dropped; ThermalTangent:  */
/* masked entries of ddu read as zero) as for "Mass"; the diagonal and the     */
/* point-block diagonal are refused.  The element results are summed per node  */
/* in element order, no atomics.  After one eager apply the operators can be   */
/* recorded in a CeedXGraph: the context is frozen, theta's ADDRESS is the     */
/* launch argument, so new values behind it are seen by a replay.  Kernel names*/
/* "thermal_force<P=..,Q=..>", "thermal_tangent<P=..,Q=..>",                   */
/* "stress<P=..,Q=..,points+thermal>" / "...,nodal+thermal>".                  */
CEED_EXTERN_OPTIONAL int CeedXHasQFunction(Ceed ceed, const char *name, int *has);
/* OPTIONAL entry points: point-block Jacobi (PCPBJACOBI) for the 3-component  */
/* displacement field.  A caller looks them up and, where they are absent,     */
/* forms the blocks from element matrices assembled through the entry points   */
/* above and does the small dense algebra itself.                              */
/* libCEED's CeedOperatorLinearAssemblePointBlockDiagonal for the Jacobian     */
/* operators: the 3 x 3 block of every node, [node][comp out][comp in] row-    */
/* major; the block of the node whose component-0 L-offset is o sits at 3 * o, */
/* so `assembled` has at least 3 x the L-size entries.  Overwrites `assembled`. */
/* Nothing is symmetrised.  With a Dirichlet mask entry (c', c) is zero where  */
/* the masked operator gives zero (row c' dropped, input c read as zero).  The */
/* QFunction context is read at call time (the -nu_smoother swap of            */
/* matops.c:215-232 works as for the diagonal).  Kernel name                   */
/* "pbdiag<P=..,Q=..,LinElas|HyperSSdF|HyperFSdF>".                            */
CEED_EXTERN_OPTIONAL int CeedOperatorLinearAssemblePointBlockDiagonal(CeedOperator op,
    CeedVector assembled, CeedRequest *request);
/* In place, per node: the components whose diagonal entry is exactly zero     */
/* (constrained, or an L-vector entry no element holds) are dropped and the    */
/* inverse of the remaining principal sub-block is embedded in zeros -- what   */
/* CeedVectorReciprocal leaving zeros alone is for the scalar diagonal.        */
/* *n_bad (or NULL) receives the number of blocks with a non-finite or non-    */
/* positive pivot; reading it synchronises, NULL leaves the host out (and is   */
/* the form that can be recorded in a CeedXGraph).                             */
CEED_EXTERN_OPTIONAL int CeedXVectorPointBlockInvert(CeedVector blocks, int *n_bad /* or NULL */);
/* w_n = B_n x_n for every node n (the lengths are multiples of 3, `blocks`    */
/* holds at least 3 x the length of x).                                        */
CEED_EXTERN_OPTIONAL int CeedXVectorPointBlockMult(CeedVector w, CeedVector blocks, CeedVector x);
/* CeedXVectorChebyshevStep with dinv .* ri replaced by B_n ri_n:              */
/*   ri = b - t (t may be NULL);  d = c1 * B ri + c2 * d;  x = d or x + d;     */
/*   ri is stored only if r is not NULL.  x may alias no other operand.        */
/* Recordable into a CeedXGraph like the scalar step.                          */
CEED_EXTERN_OPTIONAL int CeedXVectorChebyshevStepPointBlock(CeedVector x, CeedVector d, CeedVector r /* or NULL */,
    CeedVector b, CeedVector t /* or NULL */, CeedVector blocks, double c1, double c2, int assign_x);
/* OPTIONAL entry points: surface loads on a list of element faces (a union of */
/* side sets): a dead traction, a pressure that follows the deforming surface  */
/* and that pressure's exact tangent.  (The reference has no surface loads:    */
/* no call site is cited.)  A caller looks them up and, where they are absent, */
/* integrates over the faces itself (ceedpetscsolid_amd/surface.py).           */
/* A face has the P x P face nodes of its element, N_a their tensor Lagrange   */
/* functions on the Gauss-Lobatto points, (xi, eta) its two reference          */
/* directions -- xi runs fastest in the face's node list -- ordered by the     */
/* caller so that X_xi x X_eta points out of the body.  X are the node         */
/* coordinates, x = X + u the current position, the quadrature Q x Q Gauss     */
/* points.  Three geometric vectors; signs and load factors are the caller's:  */
/*   traction:  g_a      = int N_a t |X_xi x X_eta| dxi deta                   */
/*              (t a constant 3-vector, per unit REFERENCE area)               */
/*   pressure:  g_a(u)   = int N_a (x_xi x x_eta) dxi deta                     */
/*              (area-weighted current outward normal; quadratic in u)         */
/*   tangent:   T(u) du |_a = int N_a (du_xi x x_eta + x_xi x du_eta) dxi deta */
/*              (the derivative of g(u) in the direction du)                   */
/* The face results are summed per node in face order: bit-reproducible.       */
/*   Create: offsets[nface][P*P] are the component-0 L-offsets of the face     */
/*     nodes (three interlaced components per node, so multiples of 3 with     */
/*     offset + 2 < lsize), xi fastest; copied.  (P, Q) must be instantiated:  */
/*     P = 2..8, Q = P..min(P+2, 8).  nface = 0 is legal: every apply is then  */
/*     a no-op.                                                                */
/*   SetDirichletMask: the byte mask of CeedXOperatorSetDirichletMaskMode      */
/*     (host memory, copied; NULL clears).  Masked rows of y are never         */
/*     written and masked entries of du read as zero; u is read as it is (it   */
/*     carries the boundary values).                                           */
/*   ApplyAdd: y += scale * g.  Traction: coef = t, u is ignored.  Pressure:   */
/*     g is multiplied by coef[0]; u = NULL is the reference configuration.    */
/*   ApplyTangentAdd: y += scale * p * T(u) du.                                */
/* Both applies check the vector lengths against lsize before anything is      */
/* launched, run on the Ceed's stream, and can be recorded in a CeedXGraph     */
/* after one eager apply (the first builds the faces' transpose map).  Rows of */
/* y that lie on no face are never touched.                                    */
typedef struct CeedXSurfaceLoad_private *CeedXSurfaceLoad;
#define CEED_X_SURFACE_TRACTION 0
#define CEED_X_SURFACE_PRESSURE 1
CEED_EXTERN_OPTIONAL int CeedXSurfaceLoadCreate(Ceed ceed, CeedInt nface, CeedInt P, CeedInt Q,
    const CeedInt *offsets, CeedInt lsize, CeedXSurfaceLoad *sl);
CEED_EXTERN_OPTIONAL int CeedXSurfaceLoadSetDirichletMask(CeedXSurfaceLoad sl, CeedMemType mtype,
    const unsigned char *mask, CeedInt lsize);
CEED_EXTERN_OPTIONAL int CeedXSurfaceLoadApplyAdd(CeedXSurfaceLoad sl, int kind, const CeedScalar coef[3],
    CeedScalar scale, CeedVector X, CeedVector u /* or NULL */, CeedVector y);
CEED_EXTERN_OPTIONAL int CeedXSurfaceLoadApplyTangentAdd(CeedXSurfaceLoad sl, CeedScalar p, CeedScalar scale,
    CeedVector X, CeedVector u /* or NULL */, CeedVector du, CeedVector y);
/* Instantiation of the last launch, e.g. "surface<P=3,Q=3>" (empty before).   */
CEED_EXTERN_OPTIONAL int CeedXSurfaceLoadGetKernelName(CeedXSurfaceLoad sl, const char **name);
CEED_EXTERN_OPTIONAL int CeedXSurfaceLoadDestroy(CeedXSurfaceLoad *sl);
/* (Penalty contact of such faces with a rigid plane or sphere, CeedXContact*: */
/* include/ceed_contact.h, a header of its own on top of this one.)            */
/* Assembled sparse operator on L-vectors: the coarse level of the multigrid. */
/* The reference builds it by finite-difference colouring of the p=1 operator */
/* (misc.c:151-183, elasticity.c:457-483) and hands it to GAMG; here the      */
/* caller supplies the sparsity pattern and, per Newton step, element-matrix  */
/* entries in COO form (e.g. the outputs of the Jacobian operator on an       */
/* element-discontinuous restriction applied to unit vectors).                */
/*   rowptr[nrows+1], cols[nnz]: CSR pattern (host, copied).                  */
/*   coo_slot[ncoo]: CSR slot that COO entry k is summed into, or -1 to drop  */
/*     it (host, copied); each slot sums its entries in ascending k, so the   */
/*     assembly is deterministic.                                            */
/*   unit_rows[n_unit]: rows whose diagonal entry is set to 1 after assembly  */
/*     (constrained dofs whose other entries were dropped).                   */
typedef struct CeedXCsr_private *CeedXCsr;
CEED_EXTERN int CeedXCsrCreate(Ceed ceed, CeedInt nrows, const CeedInt *rowptr, const CeedInt *cols,
                               CeedInt ncoo, const CeedInt *coo_slot, CeedInt n_unit,
                               const CeedInt *unit_rows, CeedXCsr *csr);
CEED_EXTERN int CeedXCsrAssemble(CeedXCsr csr, CeedVector coo_values);
CEED_EXTERN int CeedXCsrApply(CeedXCsr csr, CeedVector x, CeedVector y);       /* y = A x */
CEED_EXTERN int CeedXCsrGetDiagonal(CeedXCsr csr, CeedVector d);
CEED_EXTERN int CeedXCsrDestroy(CeedXCsr *csr);
/* Algebraic hierarchy under the assembled level: what PCGAMG builds for the  */
/* reference's coarse solve (elasticity.c:579-581, one V-cycle per outer      */
/* iteration under KSPPREONLY, :575).  The library supplies the pieces with a */
/* fixed sparsity, the caller the aggregation (ceedpetscsolid_amd/amg.py):    */
/*  - CeedXCsrCreateRect: an nrows x ncols matrix; `vals` fixed (prolongation */
/*    P, restriction P^T) or NULL for zeros;                                  */
/*    CeedXCsrApply takes x of ncols, y of nrows.                             */
/*  - CeedXCsrCreateProduct / CeedXCsrUpdate: C = left * right on FIXED       */
/*    patterns.  The pattern of C is worked out once, on the host; every      */
/*    update recomputes the values on the device from the operands' current   */
/*    values -- one launch, a wave per row, each entry summed in the order of */
/*    the left operand's row (deterministic); no term lists are kept.         */
/*    `variable` (0 left, 1 right) names the operand that changes between      */
/*    updates; the right operand's columns must be sorted within a row.       */
/*    Two of these form the Galerkin product T = A P, A_c = P^T T each Newton */
/*    step.  dense != 0 gives C the full pattern (for the inverse below).     */
/*  - CeedXCsrGetPattern: sizes and the host copy of the pattern (borrowed).  */
/*  - CeedXCsrGetValues: copy of the values in pattern order.                 */
/*  - CeedXCsrInvertDenseSPD: in-place inverse of a matrix whose pattern is   */
/*    full (row r holds columns 0..n-1 in order) and whose values are         */
/*    symmetric positive definite (the coarsest Galerkin matrix); an error    */
/*    if a pivot is not positive.  Not recordable into a graph.               */
CEED_EXTERN int CeedXCsrCreateRect(Ceed ceed, CeedInt nrows, CeedInt ncols, const CeedInt *rowptr,
                                   const CeedInt *cols, const CeedScalar *vals, CeedXCsr *csr);
CEED_EXTERN int CeedXCsrCreateProduct(CeedXCsr left, CeedXCsr right, int variable, int dense, CeedXCsr *csr);
CEED_EXTERN int CeedXCsrGetPattern(CeedXCsr csr, CeedInt *nrows, CeedInt *ncols, CeedInt *nnz,
                                   const CeedInt **rowptr, const CeedInt **cols);
CEED_EXTERN int CeedXCsrUpdate(CeedXCsr csr);
CEED_EXTERN int CeedXCsrGetValues(CeedXCsr csr, CeedVector values);
CEED_EXTERN int CeedXCsrInvertDenseSPD(CeedXCsr csr);
/* Accumulated device time (ms) and launch count of the operator's dominant   */
/* kernel since the last reset; measured with hipEvents on the Ceed's stream  */
/* when timing is enabled.                                                    */
CEED_EXTERN int CeedXOperatorSetTiming(CeedOperator op, int enable);
CEED_EXTERN int CeedXOperatorGetTiming(CeedOperator op, double *ms,
                                       int64_t *launches);
/* Halo exchange between the element partitions of several GPUs: the replacement */
/* of DMLocalToGlobal(ADD_VALUES) (src/matops.c:57, :33) for L-vectors whose       */
/* interface entries are replicated.  RCCL point-to-point over xGMI, one group of  */
/* sends and receives per exchange on a stream of its own; pack and unpack-add are */
/* kernels of this library.  Bootstrap as with any NCCL communicator: rank 0 calls */
/* CeedXCommGetUniqueId, the host program distributes the 128 bytes (MPI_Bcast in  */
/* the reference's world), every rank calls CeedXCommInit.  `index[k]` lists the   */
/* `count[k]` L-vector entries shared with rank `neigh_rank[k]` in an order both    */
/* sides agree on.  Start after the interface nodes are complete (e.g. after       */
/* CeedXOperatorApplyPhase 0), Finish after the interior work has been queued.     */
typedef struct CeedXHalo_private *CeedXHalo;
CEED_EXTERN int CeedXCommGetUniqueId(Ceed ceed, char id[128]);
CEED_EXTERN int CeedXCommInit(Ceed ceed, int nranks, int rank, const char id[128]);
CEED_EXTERN int CeedXCommDestroy(Ceed ceed);
/* Ranks of the communicator and this rank's number as RCCL itself reports them   */
/* (ncclCommCount / ncclCommUserRank); 0 and -1 without a communicator.           */
CEED_EXTERN int CeedXCommGetSize(Ceed ceed, int *nranks, int *rank);
CEED_EXTERN int CeedXHaloCreate(Ceed ceed, CeedInt nneigh, const int *neigh_rank,
                                const CeedInt *count, const CeedInt *const *index,
                                CeedXHalo *halo);
CEED_EXTERN int CeedXHaloStart(CeedXHalo halo, CeedVector y);
CEED_EXTERN int CeedXHaloFinish(CeedXHalo halo, CeedVector y);
CEED_EXTERN int CeedXHaloDestroy(CeedXHalo *halo);
/* CeedOperatorApply of a residual / Jacobian operator AND the interface sum of  */
/* its output in one call -- ApplyLocalCeedOp's CeedOperatorApply followed by     */
/* DMLocalToGlobal(ADD_VALUES) (src/matops.c:46,57) on several GPUs.  With a      */
/* split set (CeedXOperatorSetOverlapSplit) the interface-touching elements and   */
/* the interior elements run as two launches on two streams, the exchange starts  */
/* as soon as the interface nodes are complete and its arrivals are added by the  */
/* launch that sums the interior rows.  Bitwise CeedOperatorApply, then           */
/* CeedXHaloStart / Finish.  Recordable into a CeedXGraph.                        */
CEED_EXTERN int CeedXOperatorApplyWithHalo(CeedOperator op, CeedVector in, CeedVector out,
                                           CeedXHalo halo);
/* Sum of entries [first, first + n) of a device vector over all ranks of the     */
/* communicator, in place, on the Ceed's stream: the MPI_Allreduce behind VecDot  */
/* and VecNorm (src/matops.c:292, the Krylov norms) with the scalars left on the  */
/* device.  One rank (or no communicator): nothing happens.                       */
CEED_EXTERN int CeedXCommAllReduce(Ceed ceed, CeedVector v, CeedInt first, CeedInt n);
/* Diagnostic: how the last apply of a residual / Jacobian operator was        */
/* launched.  out[0] segments (fused-kernel launches) of the apply, 1 = the    */
/* serial form; out[1] streams they alternate between; out[2] k_assemble       */
/* launches; out[3] elements of the last segment.                              */
/* NOTE one device per process: the library caches device properties process-  */
/* wide (one rank per GPU, as under mpirun / torchrun).                         */
CEED_EXTERN int CeedXOperatorGetLaunchInfo(CeedOperator op, int out[4]);

#endif /* CEED_MI355X_CEED_H */
