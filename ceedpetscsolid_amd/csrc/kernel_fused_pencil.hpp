// kernel_fused_pencil.hpp -- the fused operator kernel: PENCIL PER LANE.
//
// The whole CeedOperatorApply of the residual / Jacobian operators (setuplibceed.c:517-542, :817-839) in one launch:
// gather, interp, grad, QFunction, grad^T, interp^T, element results to y / the shell E-vector.
//
// Why pencils.  The first-generation kernel of round 1 (one OUTPUT point of a contraction per lane; removed from the
// tree in round 3, last present at commit 14cd5f8) gave every lane one output point, so the Q lanes
// that share an input row each read the whole row from LDS (Q-fold redundant LDS reads) and
// per-lane coefficient rows also come from LDS: ~71 % LDS-pipe busy, LDS bound.  Here a lane
// owns a whole PENCIL (one line of the element along the contraction direction, one
// component): it reads the NIN inputs once, produces all NOUT outputs in registers and writes
// them back IN PLACE.  Every value is read once and written once per pass, and the
// coefficients are wave-uniform, so they are scalar operands (kernarg -> SGPR), not LDS
// traffic.  Measured (PMC, config 4): LDS instructions per element 441 -> 220, LDS index unit ~30 % busy.
//
// Pipeline for a group of E elements owned by ONE wave64 (no s_barrier anywhere: a wave's LDS
// queue is executed in order).  Arrays A, BX, BZ: [c][k][j][i], strides (1, Q, Q^2, Q^3) doubles.
//   gather  x -> A (nodes)                          node-owner lanes
//   F1..F3  interpolate along i, j, k in place      pencil lanes;  F3 also writes dU/dz -> BZ (grad1d)
//   F4, F5  collocated d/dx: A -> BX, d/dy: A -> A  pencil lanes
//   QF      9 gradient entries in, 9 out, in place  point-owner lanes, one round of 64 points at a
//                                                   time; stored state prefetched two rounds ahead; the
//                                                   geometric factors RECOMPUTED from the element's
//                                                   trilinear map (GEO) or read with the state
//   B1..B5  transposes of F5..F1, accumulating      pencil lanes
//   final   A (nodes) -> y (element-interior nodes), shell E-vector (shared nodes) / atomics   node-owner lanes
// Elements per wave E: 8 (Q=2), 4 (Q=3,4), 2 (Q=5), 1 (Q>=6): a pass has 3*Q^2 pencils per element,
// E picks how well they fill 64 lanes against the LDS slab (9*Q^3 doubles per element).
#pragma once
#include "kernels_common.hpp"
#include "qfunctions_device.hpp"

namespace cps {

template <int P, int Q> struct PencilGeom {
  static constexpr int Q3 = Q * Q * Q, P3 = P * P * P;
  static constexpr int E = pencil_group_elems(Q);                            // elements per wave
  static constexpr int SJ = Q, SK = Q * Q, SC = Q3;                         // strides in doubles
  static constexpr int ARR = 3 * SC;                                        // one 3-component array
  static constexpr int PAD = Q == 5 ? 5 : 1;                                // tools/pencil_layout_search.py
  static constexpr int SE = 3 * ARR + PAD;                                  // element slab: A, BX, BZ (a 6 Q^3 slab, the upper bound of
                                                                            // holding the k-direction in registers, bought nothing at
                                                                            // Q = 7: profiles/r05_ab_experiments.txt item 1)
  static constexpr int RQ = (E * Q3 + 63) / 64;                             // point rounds per group
  static constexpr int RN = (E * P3 + 63) / 64;                             // node rounds per group
  static constexpr int GEO = E * GEO_NCOEF + 2 * Q;                           // element map coefficients + 1-D points / weights
  static constexpr int LDS_BYTES = (E * SE + GEO) * 8;
};

// ---- LDS accessors: VOLATILE 8-byte accesses through an LDS pointer + constant offset ----------
// Volatile does two jobs.  (1) hipcc keeps each access a separate ds_read_b64 / ds_write_b64 with an
// immediate offset (and still tracks them: it places counted s_waitcnt lgkmcnt(N) itself) instead of
// pairing the strided pencil reads into ds_read2_b64, which runs at half the byte rate of ds_read_b64
// on gfx950 (MI355X_MICROARCH.md, LDS table).  (2) Volatile accesses are never reordered against
// each other, which is all the ordering the passes need: they communicate through LDS across lanes
// of ONE wave, whose LDS queue the hardware executes in order.
// (Inline-asm ds_read_b64 + explicit waits were tried first: the compiler does not know that an asm
// output is still in flight, so it may copy or spill the register before the wait -- it did.)
typedef __attribute__((address_space(3))) double lds_double;
typedef volatile lds_double *ldsp_t;
typedef volatile __attribute__((address_space(3))) char *ldsb_t;
// Wave priority by phase (s_setprio, 0 ... 3).  The two waves of a SIMD share its vector pipe; the arbiter prefers the higher
// priority.  A wave in its pencil passes issues short bursts of FMAs between LDS round trips, a wave in its q-point rounds a long
// run of them: with the passes at 3 and the q-point rounds at 0 a pass never waits behind the other wave's physics, its LDS
// latency is hidden by that physics, and two waves that started together drift half a group apart by themselves.  Same-box A/B
// (profiles/r03_ab_experiments.txt item 13): config 4 -2.6 %, 13 200 hexes -8 %, config 5's block -3.6 %, p = 2 -6.5 %; a
// level for the requests / gather / final stores of their own, and for the loads and stores inside a q-point round: no
// further gain; the staggered start of round 2 (-1.9 % then) adds nothing beside it and left the kernel.
constexpr int PRIO_PASS = 3;   // the twelve pencil passes, forward and transposed alike (item 15d of that file); the requests for the next
                               // group, the gather and the final stores stay at it
constexpr int PRIO_PHYS = 0;   // the q-point rounds
// (diagnostic build only, tools/phase_timing.py) -DCPS_PHASE_TIMING=<k>: every wave writes the shader-clock time stamps of the
// phase boundaries of its k-th group to the buffer whose address the environment gives (CEED_MI355X_PHASE_BUF), 32 per wave.
#ifdef CPS_PHASE_TIMING
#define CPS_PH(i) do { if (ph_iter == CPS_PHASE_TIMING && lane == 0 && ph_buf) ph_buf[(size_t)blockIdx.x * 32 + (i)] = clock64(); } while (0)
#else
#define CPS_PH(i) do { } while (0)
#endif
template <int OFF>
CPS_DEV double lds_rd(ldsp_t a) {
  static_assert(OFF >= 0 && OFF < 65536 && OFF % 8 == 0, "ds offset field is 16 bits");
  return a[OFF / 8];
}
template <int OFF>
CPS_DEV void lds_wr(ldsp_t a, double v) {
  static_assert(OFF >= 0 && OFF < 65536 && OFF % 8 == 0, "ds offset field is 16 bits");
  a[OFF / 8] = v;
}
// N values at stride SB bytes from byte offset OFF
template <int N, int SB, int OFF, int M = 0>
CPS_DEV void pencil_ld(ldsp_t a, double *r) {
  if constexpr (M < N) {
    r[M] = lds_rd<OFF + M * SB>(a);
    pencil_ld<N, SB, OFF, M + 1>(a, r);
  }
}
template <int N, int SB, int OFF, int M = 0>
CPS_DEV void pencil_st(ldsp_t a, const double *r) {
  if constexpr (M < N) {
    lds_wr<OFF + M * SB>(a, r[M]);
    pencil_st<N, SB, OFF, M + 1>(a, r);
  }
}

// Coefficient tables are read straight from the kernarg segment (constant address space ->
// s_load, SGPR operands of the FMAs).  Each pass takes a freshly "laundered" pointer, so the
// compiler loads that pass's coefficients inside the pass instead of hoisting all three tables
// out of the element loop (150 SGPRs: it then spilled them to VGPR lanes, 900 v_readlane per group).
typedef const __attribute__((address_space(4))) double *ktab_t;
CPS_DEV ktab_t ktab_fresh(ktab_t p) {
  // "memory": the previous pass's last stores (and the FMAs feeding them) stay above this point, so two passes'
  // tables are never live together (they do not fit the SGPR file: 16 of them were spilled to VGPR lanes)
  asm volatile("" : "+s"(p) : : "memory");
  return p;
}
// a fresh table pointer that the compiler cannot use before the N values at `dep` have been computed
template <int N>
CPS_DEV ktab_t ktab_fresh_after(ktab_t p, const double *dep) {
#pragma unroll
  for (int i = 0; i < N; i++) asm volatile("" : "+s"(p) : "v"(dep[i]));
  return p;
}
// The launch arguments are read the same way: a laundered pointer into the kernarg segment at every use site, so
// that pointers and scalars are re-read with s_load (no VALU) where they are needed instead of living in SGPRs
// through the whole element loop, where the register allocator spills them to VGPR lanes (v_readlane per use).
typedef const __attribute__((address_space(4))) FusedGradArgs *kargs_t;
template <bool LAUNDER>
CPS_DEV kargs_t kargs_fresh() {
  static_assert(sizeof(BasisTables) % 8 == 0, "second kernel argument follows the tables without padding");
  auto p = (const __attribute__((address_space(4))) char *)__builtin_amdgcn_kernarg_segment_ptr() + sizeof(BasisTables);
  if constexpr (LAUNDER) asm volatile("" : "+s"(p));
  return (kargs_t)p;
}
// out[o] += sum_m M(o, m) in[m];  M(o, m) = TR ? tab[m * LD + o] : tab[o * LD + m]  (wave-uniform -> SGPR operands)
template <int NOUT, int NIN, int LD, bool TR>
CPS_DEV void pencil_mac(ktab_t tab, const double *in, double *out) {
#pragma unroll
  for (int o = 0; o < NOUT; o++) {
#pragma unroll
    for (int m = 0; m < NIN; m++) out[o] += (TR ? tab[m * LD + o] : tab[o * LD + m]) * in[m];
  }
}
// The same product with the table in even-odd form (FusedGradArgs::eo; SGN = +1 centro-symmetric, -1 antisymmetric):
// xe_j = x_j + x_{K-1-j}, xo_j = x_j - x_{K-1-j};  E_i = sum_j Me[i][j] xe_j + Mm[i] x_mid,  O_i = sum_j Mo[i][j] xo_j;
// y_i = E_i + O_i,  y_{N-1-i} = SGN (E_i - O_i);  the middle row keeps only its non-vanishing half.
template <int NOUT, int NIN, int SGN>
CPS_DEV void pencil_mac_eo(ktab_t T, const double *in, double *out) {
  constexpr int HIN = NIN / 2, HOUT = NOUT / 2;
  double xe[HIN > 0 ? HIN : 1], xo[HIN > 0 ? HIN : 1];
#pragma unroll
  for (int j = 0; j < HIN; j++) { xe[j] = in[j] + in[NIN - 1 - j]; xo[j] = in[j] - in[NIN - 1 - j]; }
#pragma unroll
  for (int i = 0; i < HOUT; i++) {
    double ev = (NIN & 1) ? T[32 + i] * in[HIN] : 0., od = 0.;
#pragma unroll
    for (int j = 0; j < HIN; j++) { ev += T[i * HIN + j] * xe[j]; od += T[16 + i * HIN + j] * xo[j]; }
    out[i] += ev + od;
    out[NOUT - 1 - i] += SGN > 0 ? ev - od : od - ev;
  }
  if constexpr (NOUT & 1) {
    double mid = (SGN > 0 && (NIN & 1)) ? T[32 + HOUT] * in[HIN] : 0.;
#pragma unroll
    for (int j = 0; j < HIN; j++) mid += SGN > 0 ? T[HOUT * HIN + j] * xe[j] : T[16 + HOUT * HIN + j] * xo[j];
    out[NOUT - 1 - HOUT] += mid;
  }
}
// plain or even-odd product; `tab` is the matching table (BasisTables entry or FusedGradArgs::eo[t])
template <int NOUT, int NIN, int LD, bool TR, int SGN, bool EO>
CPS_DEV void mac_sel(ktab_t tab, const double *in, double *out) {
  if constexpr (EO) pencil_mac_eo<NOUT, NIN, SGN>(tab, in, out);
  else pencil_mac<NOUT, NIN, LD, TR>(tab, in, out);
}
// round r of a pass with `ntask` tasks: is this lane's task t = lane + 64 r a real one?
CPS_DEV bool pencil_ok(int lane, int r, int ntask) { return ntask == 0 ? lane < 0 : ((r + 1) * 64 <= ntask ? true : lane + 64 * r < ntask); }
// Task -> lane mapping of a pass.  FLAT: task t = lane + 64 r over (element, component, b, a), a fastest.  BLOCKED (round 4): every
// (element, component) block of n = NA NB pencils starts on a 32- or 64-lane boundary, the lanes behind its last pencil idle --
// taken where that padding costs no extra round (Q = 5: 6 blocks of 25 in 6 half-waves = the same 3 rounds; Q = 7: 3 blocks of 49 in
// 3 waves).  A ds_read_b64 is served in the lane groups {0-31}, {32-63} (MI355X_MICROARCH.md, LDS): with the blocks aligned to them a
// group reads ONE component's pencils -- consecutive or evenly strided words, conflict-free along i and k -- instead of the tail of
// one component and the head of the next, 125 words further on, whose banks collide (tools/lds_conflict_model.py: LDS-array cycles
// per group of two elements 2 021 -> 1 896 at Q = 5).  Validity keeps the form of pencil_ok: the pass is handed a VIRTUAL lane
// (negative for the lanes of a real block, huge for idle ones) and ntask = 0, so that `vlane + 64 r < 0` holds exactly for the
// rounds in which the lane's block exists.
// A blocked pass is ONE exec region with the idle lanes off (pencil_pass), every round unconditional inside it: ntask = 0 means
// that every block exists (3 E blk = 64 rounds exactly).  Measured (profiles/r04_ab_experiments.txt item 3): -0.6 % (config 4) to
// -1.3 % (13 200 hexes) against flat, 198 -> 184 VGPRs.  The idle lanes loading and multiplying too, only their stores masked:
// +2.7 % (28 % more lane-FMAs under the power limit); per-round predicates on the loads: 256 VGPRs and scratch.
constexpr int pencil_blk(int n, int E) {   // lanes per block, or 0: flat
  const int flat = (3 * E * n + 63) / 64, b = n <= 32 ? 32 : (n <= 64 ? 64 : 0);
  return (b && b != n && (3 * E * b) % 64 == 0 && (3 * E * b) / 64 == flat) ? b : 0;
}
// the guard of a round's loads and arithmetic: pencil_ok under a second name, the stores inside test pencil_ok itself.  The same
// predicate, and it stays a function of its own: with the two written as one name the compiler inlines them in another order and
// schedules every kernel at Q = 2 and Q = 6 differently (HISTORY.md, "compile-time hooks retired").  That rests on one compiler's
// inlining order: before folding or moving it, and after a compiler update, compare the disassembly of every kernel of every object
// with the previous build's (llvm-objdump -d --mcpu=gfx950 on the code objects tools/isa_guard.py extracts) -- isa_summary.txt alone
// shows only five of the 124 kernels that change
CPS_DEV bool pencil_ok_ld(int lane, int r, int ntask) { return pencil_ok(lane, r, ntask); }

// One single-input pass: every task reads its pencil (NIN entries at stride SB bytes from array SRC),
// applies the NOUT x NIN matrix and writes NOUT entries to array DST (DST == SRC: in place).  All
// rounds' reads are issued first, so the waits are counted ones and the FMAs of one round overlap the
// reads of the next; tasks are disjoint pencils, so reads may pass the in-place writes of other rounds.
// A NOUT x NIN table is 2 NOUT NIN SGPRs: 50 at 5 x 5, but 98 at 7 x 7 and 128 at 8 x 8 -- more than the SGPR file, and
// the register allocator then spills coefficients to VGPR lanes (~950 v_readlane / v_writelane per element at Q = 7,
// a fifth of the VALU work).  Larger tables are therefore applied in SPLITS of whole output rows, each split loaded
// (s_load) only after the previous one's FMAs: all rounds of a pass keep their inputs and outputs in VGPRs meanwhile.
template <int NOUT, int NIN, bool EO = false> constexpr int table_splits() {
  return (EO || NOUT * NIN <= 30) ? 1 : (NOUT * NIN <= 56 ? 2 : 3);   // an even-odd table is at most 30 coefficients
}
// rows [O0, O1) of the product of pencil_mac
template <int O0, int O1, int NIN, int LD, bool TR>
CPS_DEV void pencil_mac_rows(ktab_t tab, const double *in, double *out) {
#pragma unroll
  for (int o = O0; o < O1; o++) {
#pragma unroll
    for (int m = 0; m < NIN; m++) out[o] += (TR ? tab[m * LD + o] : tab[o * LD + m]) * in[m];
  }
}
// out[r] += M in[r] for all rounds r of a pass, the table taken in table_splits() row blocks
// (DEP0: the first block, too, waits for the values already in `out` -- a previous product accumulated there)
template <int NOUT, int NIN, int LD, bool TR, int R, bool DEP0 = false, int S = 0>
CPS_DEV void mac_rounds(ktab_t table, const double (&in)[R][NIN], double (&out)[R][NOUT], int lane, int ntask) {
  constexpr int NS = table_splits<NOUT, NIN>(), H = (NOUT + NS - 1) / NS;
  if constexpr (S < NS) {
    const ktab_t t = (S > 0 || DEP0) ? ktab_fresh_after<R * NOUT>(table, &out[0][0]) : ktab_fresh(table);
#pragma unroll
    for (int r = 0; r < R; r++)
      if (pencil_ok_ld(lane, r, ntask)) pencil_mac_rows<S * H, ((S + 1) * H < NOUT ? (S + 1) * H : NOUT), NIN, LD, TR>(t, in[r], out[r]);
    mac_rounds<NOUT, NIN, LD, TR, R, DEP0, S + 1>(table, in, out, lane, ntask);
  }
}
template <int NIN, int NOUT, int LD, bool TR, int SB, int SRC, int DST, int SGN, bool EO, int R>
CPS_DEV void pencil_pass_impl(ktab_t table, const ldsp_t (&addr)[R], int lane, int ntask) {
  double in[R][NIN];
#pragma unroll
  for (int r = 0; r < R; r++)
    if (pencil_ok_ld(lane, r, ntask)) pencil_ld<NIN, SB, SRC>(addr[r], in[r]);
  if constexpr (table_splits<NOUT, NIN, EO>() == 1) {
    const ktab_t t = ktab_fresh(table);
#pragma unroll
    for (int r = 0; r < R; r++)
      if (pencil_ok_ld(lane, r, ntask)) {
        double out[NOUT] = {};
        mac_sel<NOUT, NIN, LD, TR, SGN, EO>(t, in[r], out);
        if (pencil_ok(lane, r, ntask)) pencil_st<NOUT, SB, DST>(addr[r], out);
      }
  } else {
    double out[R][NOUT];
#pragma unroll
    for (int r = 0; r < R; r++)
#pragma unroll
      for (int o = 0; o < NOUT; o++) out[r][o] = 0.;
    mac_rounds<NOUT, NIN, LD, TR, R>(table, in, out, lane, ntask);
#pragma unroll
    for (int r = 0; r < R; r++)
      if (pencil_ok(lane, r, ntask)) pencil_st<NOUT, SB, DST>(addr[r], out[r]);
  }
}

// blocked pass (ntask = 0, lane = the virtual lane): ONE exec region around the whole pass for the lanes that own a pencil, every
// round unconditional inside it (per-round predicates on loads and products cost 256 VGPRs and scratch when tried)
template <int NIN, int NOUT, int LD, bool TR, int SB, int SRC, int DST, int SGN, bool EO, int R>
CPS_DEV void pencil_pass(ktab_t table, const ldsp_t (&addr)[R], int lane, int ntask) {
  if (ntask == 0) {
    if (lane < 0) pencil_pass_impl<NIN, NOUT, LD, TR, SB, SRC, DST, SGN, EO, R>(table, addr, 0, 64 * R);
  } else pencil_pass_impl<NIN, NOUT, LD, TR, SB, SRC, DST, SGN, EO, R>(table, addr, lane, ntask);
}

constexpr int PENCIL_NSET = 2;   // q-point register sets: 2 = every round's data is requested two rounds ahead
                                 // (198 VGPRs with the hyperFS tangent; 1 set: 4-6 % slower; 3 sets: no gain; profiles/r04_ab_experiments.txt
                                 // item 10).  Q >= 6: two sets as well since round 4.  Rounds 1-3 had ONE (a second set pushed the hyperFS
                                 // tangent past 256 VGPRs: 26 spilled); the blocked task -> lane mapping freed ~18 registers at Q = 7 and the
                                 // second set fits (202-236 VGPRs at Q = 6, 7).  Same-box A/B (profiles/r04_ab_experiments.txt item 12):
                                 // config 5's block -3.3 %, the whole 64^3 box -4.5 %, Q = 6 -2.3 %, hyperSS at Q = 7 -7.1 %
// GEO = 1: the geometric factors are recomputed per point from the element's trilinear map (FusedGradArgs::geo) instead of
// read; GEO = 2: every element of the mesh is AFFINE (a parallelepiped: the box meshes of configs 1, 2 and 5), dXdx and
// det J are constants of the element (FusedGradArgs::geo_aff, ten doubles) and only the weight varies from point to point;
// GEO = 3: every element is SWEPT along the same reference direction (FusedGradArgs::geo_swept, geo_axis): x and y bilinear in the other two
// directions, z linear in that one -- the prisms of an extruded mesh, which the reference's cylinders are.  J is a 2 x 2 block and a
// constant: four FMAs, a 2 x 2 determinant and one reciprocal per point instead of 27 FMAs, an adjugate and a 3 x 3 determinant, and the
// physics multiplies with the five entries of dXdx that are left (qf_point<QF, true>): 15 multiply-adds for each of its two products
// instead of 27.  The q-point round hands the reference directions to the physics in the order (in-plane, in-plane, sweep) by choosing
// which of the three arrays it reads first -- a relabelling of a sum's terms, no arithmetic;
// GEO = 0: qdata is read.  The 1-D tables are applied in even-odd form wherever that form exists (pencil_even_odd(Q)).
//
// MASS (k_fused_pencil_mass, the Jacobian functors only): the operator K + c M in the same launch -- the effective tangent of the Newmark
// solve.  The mass term B_i^T B_j^T B_k^T (c w det J u_q) needs nothing the kernel does not hold: u at the quadrature points is array A
// after F3 (F5 overwrites it), w det J is qdl[0] of the physics round under every GEO.  The point owners read their three u_q values before
// F5, scale them in their physics round and add them to W2 (A after B2, before B3) with an in-wave read-modify-write -- no barrier, like
// the rest; 3 RQ more doubles are live across the physics.  Every such line sits under `if constexpr (MASS)`: the kernels without the
// term are the ones they were (no run-time switch; one of that kind measured +2.3 ... 4.5 % in round 4).
//
// The two entries of the ONE body, kernel_fused_pencil_body.hpp, which each of them includes as its function body behind its own
// `constexpr bool MASS`.  The body as a __device__ __forceinline__ template<..., bool MASS> that both entries call was built first and
// rejected: every function of this file is inlined in one pass, the extra level changes the order in which that happens, and all 552
// kernels WITHOUT the term then came out different (Q = 2, LinElas, qdata read: 37 -> 50 SGPRs, 329 -> 331 VALU instructions; every row
// of the ISA summary moved) -- the sensitivity the note at pencil_ok_ld describes.  Included as text, the kernels without the term are
// instruction for instruction the ones of the build before (profiles/fused_mass.txt).
// (tab_, the first kernel argument, lives at offset 0 of the kernarg segment and is read through it.)
template <int P, int Q, int QF, int GEO>
__global__ __launch_bounds__(64, PENCIL_MINW) void k_fused_pencil(const BasisTables tab_, const FusedGradArgs a) {
  (void)tab_;
  constexpr bool MASS = false;
#include "kernel_fused_pencil_body.hpp"
}
// K + c M (FusedGradArgs::mass_c): a name of its own, in objects of its own (kernels_fused_inst.hip with -DCPS_MASS)
template <int P, int Q, int QF, int GEO>
__global__ __launch_bounds__(64, PENCIL_MINW) void k_fused_pencil_mass(const BasisTables tab_, const FusedGradArgs a) {
  (void)tab_;
  constexpr bool MASS = true;
#include "kernel_fused_pencil_body.hpp"
}

// Launch shape.  Default: a PERSISTENT grid -- as many one-wave workgroups as the device holds at once (CUs x waves per CU), each walking
// its strided list of groups with the next group's data requested a group ahead.  `l.wave_groups` > 0 (small launches): the grid grows
// instead (rounded to whole XCD sets) -- workgroups beyond the resident set are dispatched as earlier ones retire, which balances a launch
// of a few rounds and gives co-scheduled kernels (the halo exchange's) a slot at every retirement.
// MASS: the entry with the mass term (k_fused_pencil_mass), the same launch shape.
template <int P, int Q, int QF, bool MASS = false>
hipError_t launch_fused_pencil_t(const BasisTables &t, const FusedGradArgs &a_in, FusedLaunch l, hipStream_t s) {
  static_assert(PencilGeom<P, Q>::LDS_BYTES == pencil_lds_bytes(Q), "the host sizes the persistent grid from pencil_lds_bytes (kernels.hpp)");
  if (a_in.nelem <= 0) return hipSuccess;
  const int ngroups = (a_in.nelem + pencil_group_elems(Q) - 1) / pencil_group_elems(Q), ncu = device_cu_count();
  if (ncu <= 0) return hipErrorUnknown;
#ifdef CPS_PHASE_TIMING   // (diagnostic build) the time-stamp buffer rides behind the arguments
  FusedGradArgs a = a_in;
  if (const char *e = getenv("CEED_MI355X_PHASE_BUF")) a.phase_buf = (long long *)strtoull(e, nullptr, 0);
#else
  const FusedGradArgs &a = a_in;
#endif
  int grid = l.wave_groups > 0 ? ((ngroups + l.wave_groups - 1) / l.wave_groups + 7) / 8 * 8 : ncu * (l.waves_per_cu > 0 ? l.waves_per_cu : pencil_waves_per_cu(Q));
  // (A persistent grid SHRUNK so that every wave gets the same number of groups -- 1 650 waves x 4 groups instead of 2 048 x 3.2 at
  // 13 200 hexes -- was measured in round 3: 3 ... 14 % slower at every size from 5 500 to 99 000 hexes.  More waves in flight beat an
  // even finish: profiles/r03_ab_experiments.txt item 11.)
  if (grid > ngroups) grid = ngroups;
  const int geo = fused_geo_mode(a);
  if constexpr (MASS) {
    if (geo == 2) hipLaunchKernelGGL((k_fused_pencil_mass<P, Q, QF, 2>), dim3(grid), dim3(64), 0, s, t, a);
    else if (geo == 3) hipLaunchKernelGGL((k_fused_pencil_mass<P, Q, QF, 3>), dim3(grid), dim3(64), 0, s, t, a);
    else if (geo == 1) hipLaunchKernelGGL((k_fused_pencil_mass<P, Q, QF, 1>), dim3(grid), dim3(64), 0, s, t, a);
    else hipLaunchKernelGGL((k_fused_pencil_mass<P, Q, QF, 0>), dim3(grid), dim3(64), 0, s, t, a);
  } else {   // (a discarded branch instantiates nothing: an object holds the kernels of one entry only)
    if (geo == 2) hipLaunchKernelGGL((k_fused_pencil<P, Q, QF, 2>), dim3(grid), dim3(64), 0, s, t, a);
    else if (geo == 3) hipLaunchKernelGGL((k_fused_pencil<P, Q, QF, 3>), dim3(grid), dim3(64), 0, s, t, a);
    else if (geo == 1) hipLaunchKernelGGL((k_fused_pencil<P, Q, QF, 1>), dim3(grid), dim3(64), 0, s, t, a);
    else hipLaunchKernelGGL((k_fused_pencil<P, Q, QF, 0>), dim3(grid), dim3(64), 0, s, t, a);
  }
  return hipGetLastError();
}

}  // namespace cps
