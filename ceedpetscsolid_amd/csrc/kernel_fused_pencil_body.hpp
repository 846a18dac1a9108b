// kernel_fused_pencil_body.hpp -- the body of the fused operator kernel: NOT a header of its own.  kernel_fused_pencil.hpp includes it
// INSIDE its two __global__ entries, k_fused_pencil<P, Q, QF, GEO> and k_fused_pencil_mass<P, Q, QF, GEO>, each behind its own
// `constexpr bool MASS` (why as text and not as a function: the note above the entries).  It reads the entries' template arguments and
// their argument `a`; every line of the mass term sits under `if constexpr (MASS)`.
  static_assert(offsetof(BasisTables, interp) == 0 && offsetof(BasisTables, colo) == 8 * MAXN1D * MAXN1D &&
                offsetof(BasisTables, grad) == 16 * MAXN1D * MAXN1D, "kernarg layout of the tables");
  static_assert(!MASS || QF == QF_LINELAS || QF == QF_HYPERSS_DF || QF == QF_HYPERFS_DF || QF == QF_HYPERFS_DF_DS, "the mass term belongs to a tangent");
  constexpr bool EO = pencil_even_odd(Q);
  const ktab_t kt = (ktab_t)__builtin_amdgcn_kernarg_segment_ptr();
  const ktab_t ktB = kt, ktD = kt + MAXN1D * MAXN1D, ktG = kt + 2 * MAXN1D * MAXN1D;
  // the six products' tables: plain (B, D, G read forward or transposed) or their even-odd forms (FusedGradArgs::eo)
  const ktab_t eo0 = (ktab_t)((const __attribute__((address_space(4))) char *)kt + sizeof(BasisTables) + offsetof(FusedGradArgs, eo));
  const ktab_t tBf = EO ? eo0 : ktB, tBt = EO ? eo0 + EO_TAB : ktB, tDf = EO ? eo0 + 2 * EO_TAB : ktD,
               tDt = EO ? eo0 + 3 * EO_TAB : ktD, tGf = EO ? eo0 + 4 * EO_TAB : ktG, tGt = EO ? eo0 + 5 * EO_TAB : ktG;
  using G = PencilGeom<P, Q>;
  constexpr int Q3 = G::Q3, P3 = G::P3, E = G::E, RQ = G::RQ, RN = G::RN;
  constexpr int SJ = G::SJ, SK = G::SK, SC = G::SC, SE = G::SE;
  constexpr int BI = 8, BJ = 8 * SJ, BK = 8 * SK, BC = 8 * SC;        // byte strides
  constexpr int oA = 0, oBX = 8 * G::ARR, oBZ = 16 * G::ARR;         // byte offsets of the arrays
  constexpr bool ST_IN = QFTraits<QF>::state_in, ST_OUT = QFTraits<QF>::state_out;
  constexpr int NST = QFTraits<QF>::nstate;
  constexpr int QS = Q3;
  static_assert(P <= Q, "interpolation to at least as many points as nodes");
  // re-read the launch arguments at every use (kargs_fresh) where that frees the SGPR file of spills: Q <= 5.  At
  // Q >= 6 one coefficient table alone (2 Q^2 SGPRs) overflows it and the extra scalar-load waits only cost (measured).
  constexpr bool KA = Q <= 5;

  __shared__ __attribute__((aligned(16))) double slab[E * SE + G::GEO];
  const ldsp_t lds0 = (lds_double *)slab;
  constexpr bool geo = GEO != 0;   // the geometric factors are not read from qdata
  constexpr int NCO = GEO == 2 ? GEO_NAFF : (GEO == 3 ? GEO_NSWEPT : GEO_NCOEF);   // doubles per element kept in LDS for them
  const int lane = threadIdx.x & 63;
  // ---- work list of this wave -----------------------------------------------------------------------
  // The groups are cut into 8 contiguous chunks, one per XCD (neighbouring elements share their nodes through one L2):
  // block b serves chunk b % 8 (blocks b and b + 8 share an XCD under the round-robin placement), group = chunk begin +
  // wave rank + k * waves per chunk.  (A dynamic per-XCD ticket schedule was built and measured in round 2: not faster on
  // large launches, slower on small ones; removed in round 3.)
  const int ngroups = (a.nelem + E - 1) / E;
  const int nxcd = gridDim.x % 8 == 0 ? 8 : 1;
  const int wrank = (int)blockIdx.x / nxcd, wper = (int)gridDim.x / nxcd;
  const int gend = min(ngroups, (int)(blockIdx.x % nxcd + 1) * ((ngroups + nxcd - 1) / nxcd));
  int grp = (int)(blockIdx.x % nxcd) * ((ngroups + nxcd - 1) / nxcd) + wrank;
  if (grp >= gend) return;

  // ---- loop-invariant lane -> work maps -----------------------------------------------------
  // pencil passes: task t = lane + 64 r over (element, component, b, a), a fastest; address of the
  // pencil's first entry.  Five families: direction i over nodal / quadrature (j,k), direction j over
  // (i', nodal / quadrature k), direction k over (i', j').
  auto pencil_addr = [&](int t, int NA, int NB, int sa, int sb, int blk) -> ldsp_t {
    const int n = NA * NB;
    const int bl = blk ? t / blk : t / n, pen = blk ? min(t % blk, n - 1) : t % n;      // (idle lanes of a block: any address in it)
    const int el = min(bl / 3, E - 1), c = bl % 3, ia = pen % NA, ib = pen / NA;
    return lds0 + (el * SE + c * SC + (ia * sa + ib * sb) / 8);
  };
  // virtual lane of pencil_ok for a blocked family (see pencil_blk): real block <=> vlane + 64 r < 0
  auto pencil_vlane = [&](int n, int blk) -> int { return blk == 0 ? lane : ((lane % blk) < n ? blk * (lane / blk) - blk * 3 * E : (1 << 24)); };
  constexpr int T_IP = 3 * P * P, T_IQ = 3 * Q * Q, T_JP = 3 * Q * P, T_JQ = 3 * Q * Q, T_K = 3 * Q * Q;
  constexpr int B_PP = pencil_blk(P * P, E), B_QP = pencil_blk(Q * P, E), B_QQ = pencil_blk(Q * Q, E);
  constexpr int R_IP = (E * T_IP + 63) / 64, R_IQ = (E * T_IQ + 63) / 64, R_JP = (E * T_JP + 63) / 64,
                R_JQ = (E * T_JQ + 63) / 64, R_K = (E * T_K + 63) / 64;
  // what the passes are handed as (lane, ntask): the real ones (flat) or (virtual lane, 0) (blocked)
  constexpr int N_IP = B_PP ? 0 : E * T_IP, N_JP = B_QP ? 0 : E * T_JP, N_QQ = B_QQ ? 0 : E * T_IQ;
  const int lPP = pencil_vlane(P * P, B_PP), lQP = pencil_vlane(Q * P, B_QP), lQQ = pencil_vlane(Q * Q, B_QQ);
  // the k passes and the two-input j pass are written out below: a blocked one sits in ONE exec region (lQQ < 0), all its rounds
  // unconditional inside it (as in pencil_pass: lane 0 of 64 R_K tasks)
  const int lQQi = B_QQ ? 0 : lQQ;
  constexpr int N_QQi = B_QQ ? 64 * R_K : N_QQ;
  ldsp_t aIP[R_IP], aIQ[R_IQ], aJP[R_JP], aJQ[R_JQ], aK[R_K];
#pragma unroll
  for (int r = 0; r < R_IP; r++) aIP[r] = pencil_addr(lane + 64 * r, P, P, BJ, BK, B_PP);
#pragma unroll
  for (int r = 0; r < R_IQ; r++) aIQ[r] = pencil_addr(lane + 64 * r, Q, Q, BJ, BK, B_QQ);
#pragma unroll
  for (int r = 0; r < R_JP; r++) aJP[r] = pencil_addr(lane + 64 * r, Q, P, BI, BK, B_QP);
#pragma unroll
  for (int r = 0; r < R_JQ; r++) aJQ[r] = pencil_addr(lane + 64 * r, Q, Q, BI, BK, B_QQ);
#pragma unroll
  for (int r = 0; r < R_K; r++) aK[r] = pencil_addr(lane + 64 * r, Q, Q, BI, BJ, B_QQ);
  // point owners: q = lane + 64 r over (element, k, j, i); node owners likewise over P^3
  ldsp_t aPt[RQ], aNd[RN];
#pragma unroll
  for (int r = 0; r < RQ; r++) {
    const int t = lane + 64 * r, el = t / Q3, q = t % Q3;
    aPt[r] = lds0 + (el * SE + (q / (Q * Q)) * SK + ((q / Q) % Q) * SJ + q % Q);
  }
  // geometry recompute: packed byte offsets of the point's 1-D indices into the LDS tables, and its element
  uint32_t pqi[RQ];
#pragma unroll
  for (int r = 0; r < RQ; r++) {
    const int t = min(lane + 64 * r, E * Q3 - 1), el = t / Q3, q = t % Q3;
    pqi[r] = (uint32_t)((q % Q) * 8) | ((uint32_t)(((q / Q) % Q) * 8) << 8) | ((uint32_t)((q / (Q * Q)) * 8) << 16) | ((uint32_t)el << 24);
  }
  constexpr int oGC = E * SE * 8, oGT = oGC + E * GEO_NCOEF * 8;   // byte offsets of the coefficient / table areas (sized for GEO = 1)
  if (geo && lane < 2 * Q) {   // 1-D points then weights (written once; the LDS queue orders it before any read)
    const auto kp = (const __attribute__((address_space(4))) char *)__builtin_amdgcn_kernarg_segment_ptr() + sizeof(BasisTables);
    const double v = lane < Q ? ((kargs_t)kp)->qref[lane] : ((kargs_t)kp)->qwt[lane - Q];
    *(ldsp_t)((ldsb_t)lds0 + oGT + lane * 8) = v;
  }
  uint32_t nd_interior = 0;  // bit r: this lane's node of round r is interior to its element (direct store to y)
  uint32_t ev_idx[(RN + 1) / 2] = {};  // E-vector entry (in doubles) of this lane's node within the group's block, 16 bits each
  static_assert(E * (P3 * 3 + 15) < 65536, "16-bit E-vector entry index");
#pragma unroll
  for (int r = 0; r < RN; r++) {
    const int t = lane + 64 * r, el = t / P3, n = t % P3;
    aNd[r] = lds0 + (el * SE + (n / (P * P)) * SK + ((n / P) % P) * SJ + n % P);
    if (a.direct && node_is_element_interior(n, P)) nd_interior |= 1u << r;
    // [element][shell rank or node][3], the element blocks a.evec_stride doubles apart
    ev_idx[r / 2] |= (uint32_t)(min(el, E - 1) * a.evec_stride + (a.direct ? node_shell_rank(n, P) : n) * 3) << (16 * (r % 2));
  }
  // element-in-group of owner slot t, recomputed where needed (a few compares) instead of held in
  // registers through the physics
  auto el_of = [&](int t, int n3) {
    int el = 0;
#pragma unroll
    for (int e = 1; e < E; e++) el += (t >= e * n3) ? 1 : 0;
    return el;
  };

  // ---- global-memory side: clamped, unconditional loads ------------------------------------------
  // Addressing: a wave-uniform 64-bit base per group (SGPRs) plus a 32-bit per-lane index inside the
  // group's block.  Lanes of a dead element (only in the last, partial group) read the group's last
  // live element instead.
  auto nlive_of = [&](int nelem, int g) { const int n = nelem - g * E; return n < E ? n : E; };  // uniform, >= 1
  // (Q >= 6 with qdata READ -- ten more doubles per point and set -- keeps one set: the residual kernel at Q = 6 spilled with two)
  // (MASS: the finite-strain tangents at Q = 6 on P >= 5 nodes keep one set too -- with the 12 doubles of u_q live across the physics the
  // second set spilled 6 ... 14 VGPRs to scratch)
  constexpr bool MASS_ONE_SET = MASS && Q == 6 && P >= 5 && (QF == QF_HYPERFS_DF || QF == QF_HYPERFS_DF_DS);
  constexpr int NSET = RQ >= 2 ? ((GEO == 0 && Q >= 6) || MASS_ONE_SET ? 1 : PENCIL_NSET) : 1;
  double qd[NSET][10], st[NSET][NST];
  auto load_point = [&](double *qdv, double *stv, int g, int r) {
    const kargs_t ka = kargs_fresh<KA>();  // one scalar load for the fields used here
    const int t = lane + 64 * r, el0 = el_of(t, Q3);
    const int q = min(t - el0 * Q3, Q3 - 1), el = min(el0, nlive_of(ka->nelem, g) - 1);
    const size_t e0 = (size_t)(ka->elem_begin + g * E);
    const double *qb = ka->qdata + e0 * (10 * Q3);
    const uint32_t vo = (uint32_t)(el * (10 * Q3) + q);
    if (!geo) {
#pragma unroll
      for (int c = 0; c < 10; c++) qdv[c] = (qb + c * Q3)[vo];
    }
    if constexpr (ST_IN) {
      const double *sb = ka->state_in + e0 * (NST * QS);
      const uint32_t vs = (uint32_t)(el * (NST * QS) + q);
#pragma unroll
      for (int c = 0; c < NST; c++) stv[c] = (sb + c * QS)[vs];
    }
  };
  auto load_offsets = [&](int g, uint32_t *o) {
    const kargs_t ka = kargs_fresh<KA>();
    const uint32_t *ob = ka->offsets + (size_t)(ka->elem_begin + g * E) * P3;
    const int nlive = nlive_of(ka->nelem, g);
#pragma unroll
    for (int r = 0; r < RN; r++) {
      const int t = lane + 64 * r, el0 = el_of(t, P3);
      const int n = min(t - el0 * P3, P3 - 1), el = min(el0, nlive - 1);
      o[r] = ob[(uint32_t)(el * P3 + n)];
    }
  };
  auto load_x = [&](const uint32_t *o, double (*xv)[3]) {
    const kargs_t kx = kargs_fresh<KA>();
    const double *xb = kx->x;
#pragma unroll
    for (int r = 0; r < RN; r++) {
      const uint32_t base = o[r] & OFF_MASK;
#pragma unroll
      for (int c = 0; c < 3; c++) xv[r][c] = xb[base + c];
    }
  };

  uint32_t off[RN], off_nx[RN];
  double xin[RN][3];
  load_offsets(grp, off);
  load_x(off, xin);
#pragma unroll
  for (int t = 0; t < NSET; t++) load_point(qd[t], st[t], grp, t);

#ifdef CPS_PHASE_TIMING
  int ph_iter = 0;
  long long *const ph_buf = a.phase_buf;
#endif
  for (;;) {
    CPS_PH(0);
#ifdef CPS_PHASE_TIMING
    if (ph_iter == CPS_PHASE_TIMING && lane == 0 && ph_buf) ph_buf[(size_t)blockIdx.x * 32 + 24] = wall_clock64();   // 100 MHz
#endif
    const int grp_nx = grp + wper;
    const bool more = grp_nx < gend;  // wave-uniform
    const int g_nx = more ? grp_nx : grp;
    load_offsets(g_nx, off_nx);
    constexpr int RG = (E * NCO + 63) / 64;
    double gcoef[RG];    // this group's element-map coefficients (or affine factors), lane + 64 i; into LDS right before the physics
    if (geo) {
      const kargs_t ka = kargs_fresh<KA>();
      const int nlive = nlive_of(ka->nelem, grp);
      const double *gb = (GEO == 2 ? ka->geo_aff : (GEO == 3 ? ka->geo_swept : ka->geo)) + (size_t)(ka->elem_begin + grp * E) * NCO;
#pragma unroll
      for (int i = 0; i < RG; i++) {
        const int t = min(lane + 64 * i, E * NCO - 1), el = min(t / NCO, nlive - 1);
        gcoef[i] = gb[(uint32_t)(el * NCO + t % NCO)];
      }
    }

    // ---- gather: x -> A at the nodes (Dirichlet flags applied; dead elements of the last group zero) ----
    const kargs_t kg = kargs_fresh<KA>();
    const int g_nelem = kg->nelem, g_mask_in = kg->mask_in;
#pragma unroll
    for (int r = 0; r < RN; r++) {
      if (pencil_ok(lane, r, E * P3)) {
        const bool live = grp * E + el_of(lane + 64 * r, P3) < g_nelem;
        const uint32_t fl = live ? (g_mask_in ? (off[r] >> OFF_FLAG_SHIFT) : 0u) : 7u;
        lds_wr<oA + 0 * BC>(aNd[r], (fl & 1u) ? 0. : xin[r][0]);
        lds_wr<oA + 1 * BC>(aNd[r], (fl & 2u) ? 0. : xin[r][1]);
        lds_wr<oA + 2 * BC>(aNd[r], (fl & 4u) ? 0. : xin[r][2]);
      }
    }

    // ---- B: nodes -> points, in place -----------------------------------------------------------------
    __builtin_amdgcn_s_setprio(PRIO_PASS);
    CPS_PH(1);
    pencil_pass<P, Q, P, false, BI, oA, oA, +1, EO>(tBf, aIP, lPP, N_IP);   // F1: along i at nodal (j, k)
    CPS_PH(2);
    pencil_pass<P, Q, P, false, BJ, oA, oA, +1, EO>(tBf, aJP, lQP, N_JP);   // F2: along j at (i', nodal k)
    CPS_PH(3);
    if (!B_QQ || lQQ < 0) {  // F3: along k at (i', j'): U -> A in place and dU/dz -> BZ (grad1d on the nodal values), one
       // table at a time (both = 100 SGPRs = SGPR spills)
      double in[R_K][P];
#pragma unroll
      for (int r = 0; r < R_K; r++)
        if (pencil_ok_ld(lQQi, r, N_QQi)) pencil_ld<P, BK, oA>(aK[r], in[r]);
      if constexpr (table_splits<Q, P, EO>() == 1) {
        const ktab_t tB = ktab_fresh(tBf);
#pragma unroll
        for (int r = 0; r < R_K; r++)
          if (pencil_ok_ld(lQQi, r, N_QQi)) {
            double out[Q] = {};
            mac_sel<Q, P, P, false, +1, EO>(tB, in[r], out);
            if (pencil_ok(lQQi, r, N_QQi)) pencil_st<Q, BK, oA>(aK[r], out);
          }
        const ktab_t tG = ktab_fresh(tGf);
#pragma unroll
        for (int r = 0; r < R_K; r++)
          if (pencil_ok_ld(lQQi, r, N_QQi)) {
            double dz[Q] = {};
            mac_sel<Q, P, P, false, -1, EO>(tG, in[r], dz);
            if (pencil_ok(lQQi, r, N_QQi)) pencil_st<Q, BK, oBZ>(aK[r], dz);
          }
      } else {  // large tables: row blocks (mac_rounds), one product after the other
        double out[R_K][Q];
#pragma unroll
        for (int pass = 0; pass < 2; pass++) {
#pragma unroll
          for (int r = 0; r < R_K; r++)
#pragma unroll
            for (int o = 0; o < Q; o++) out[r][o] = 0.;
          mac_rounds<Q, P, P, false, R_K>(pass == 0 ? ktB : ktG, in, out, lQQi, N_QQi);
#pragma unroll
          for (int r = 0; r < R_K; r++)
            if (pencil_ok(lQQi, r, N_QQi)) {
              if (pass == 0) pencil_st<Q, BK, oA>(aK[r], out[r]);
              else pencil_st<Q, BK, oBZ>(aK[r], out[r]);
            }
        }
      }
    }
    // ---- collocated gradient on the quadrature points -----------------------------------------------------
    CPS_PH(4);
    pencil_pass<Q, Q, Q, false, BI, oA, oBX, -1, EO>(tDf, aIQ, lQQ, N_QQ);  // F4: d/dx: A -> BX
    CPS_PH(5);
    double uq[MASS ? RQ : 1][3];   // MASS: u at this lane's points, then c w det J u_q (the physics rounds), added to W2 behind B2
    if constexpr (MASS) {
#pragma unroll
      for (int r = 0; r < RQ; r++)
        if (pencil_ok(lane, r, E * Q3)) {
          uq[r][0] = lds_rd<oA + 0 * BC>(aPt[r]); uq[r][1] = lds_rd<oA + 1 * BC>(aPt[r]); uq[r][2] = lds_rd<oA + 2 * BC>(aPt[r]);
        }
    }
    pencil_pass<Q, Q, Q, false, BJ, oA, oA, -1, EO>(tDf, aJQ, lQQ, N_QQ);   // F5: d/dy: A -> A in place
    CPS_PH(6);

    __builtin_amdgcn_s_setprio(PRIO_PHYS);
    if (geo) {
#pragma unroll
      for (int i = 0; i < RG; i++)
        if (lane + 64 * i < E * NCO)
          *(ldsp_t)((ldsb_t)lds0 + oGC + (lane + 64 * i) * 8) = gcoef[i];
    }
    // ---- physics: point owners, one round at a time; ug[d*3+c] from (BX, A, BZ), dv back in place ----
#pragma unroll
    for (int r = 0; r < RQ; r++) {
      CPS_PH(7 + (r < 8 ? r : 8));
      const kargs_t ka = kargs_fresh<KA>();
      const bool okp = pencil_ok(lane, r, E * Q3);
      const int pel = el_of(lane + 64 * r, Q3), pq = lane + 64 * r - pel * Q3;
      const bool live = okp && (grp * E + pel < ka->nelem);
      double ug[9], dv[9], sto[9];
      // swept elements: the arrays of the two in-plane reference directions first, the sweep direction's last (wave-uniform byte offsets)
      ldsp_t pd0 = aPt[r], pd1 = aPt[r], pd2 = aPt[r];
      int sw_a = 0, sw_b = 1;
      if constexpr (GEO == 3) {
        const int ax = ka->geo_axis;
        sw_a = ax == 0 ? 1 : 0; sw_b = ax == 2 ? 1 : 2;
        auto arr = [](int d) { return d == 0 ? oBX : (d == 1 ? oA : oBZ); };
        pd0 = (ldsp_t)((ldsb_t)aPt[r] + arr(sw_a)); pd1 = (ldsp_t)((ldsb_t)aPt[r] + arr(sw_b)); pd2 = (ldsp_t)((ldsb_t)aPt[r] + arr(ax));
      }
      if (okp) {
        if constexpr (GEO == 3) {
          ug[0] = lds_rd<0 * BC>(pd0); ug[1] = lds_rd<1 * BC>(pd0); ug[2] = lds_rd<2 * BC>(pd0);
          ug[3] = lds_rd<0 * BC>(pd1); ug[4] = lds_rd<1 * BC>(pd1); ug[5] = lds_rd<2 * BC>(pd1);
          ug[6] = lds_rd<0 * BC>(pd2); ug[7] = lds_rd<1 * BC>(pd2); ug[8] = lds_rd<2 * BC>(pd2);
        } else {
          ug[0] = lds_rd<oBX + 0 * BC>(aPt[r]); ug[1] = lds_rd<oBX + 1 * BC>(aPt[r]); ug[2] = lds_rd<oBX + 2 * BC>(aPt[r]);
          ug[3] = lds_rd<oA + 0 * BC>(aPt[r]);  ug[4] = lds_rd<oA + 1 * BC>(aPt[r]);  ug[5] = lds_rd<oA + 2 * BC>(aPt[r]);
          ug[6] = lds_rd<oBZ + 0 * BC>(aPt[r]); ug[7] = lds_rd<oBZ + 1 * BC>(aPt[r]); ug[8] = lds_rd<oBZ + 2 * BC>(aPt[r]);
        }
      }
      double qdl[10];
      if constexpr (GEO == 2) {  // affine element: dXdx and det J are the element's, the weight the point's (common.h:47-101)
        const uint32_t pk = pqi[r];
        const auto lb = (ldsb_t)lds0;
        const ldsp_t ti = (ldsp_t)(lb + oGT + (pk & 0xFFu)), tj = (ldsp_t)(lb + oGT + ((pk >> 8) & 0xFFu)),
                     tk = (ldsp_t)(lb + oGT + ((pk >> 16) & 0xFFu)), cf = (ldsp_t)(lb + oGC + (pk >> 24) * (GEO_NAFF * 8));
        qdl[0] = ti[Q] * tj[Q] * tk[Q] * cf[0];
#pragma unroll
        for (int c = 1; c < 10; c++) qdl[c] = cf[c];
      } else if constexpr (GEO == 3) {  // swept element: J = {2 x 2 block in the plane, zs along the sweep} (common.h:47-101 on that J)
        const uint32_t pk = pqi[r];
        const auto lb = (ldsb_t)lds0;
        const ldsp_t ti = (ldsp_t)(lb + oGT + (pk & 0xFFu)), tj = (ldsp_t)(lb + oGT + ((pk >> 8) & 0xFFu)),
                     tk = (ldsp_t)(lb + oGT + ((pk >> 16) & 0xFFu)), cf = (ldsp_t)(lb + oGC + (pk >> 24) * (GEO_NSWEPT * 8));
        const ldsp_t ta = (ldsp_t)(lb + oGT + ((pk >> (8 * sw_a)) & 0xFFu)), tb = (ldsp_t)(lb + oGT + ((pk >> (8 * sw_b)) & 0xFFu));
        const double xa = ta[0], xb = tb[0], w = ti[Q] * tj[Q] * tk[Q];
        const double xab = cf[2], yab = cf[5];
        const double J00 = __builtin_fma(xab, xb, cf[0]), J10 = __builtin_fma(xab, xa, cf[1]);   // d x / d xi_a, d x / d xi_b
        const double J01 = __builtin_fma(yab, xb, cf[3]), J11 = __builtin_fma(yab, xa, cf[4]);   // d y / d xi_a, d y / d xi_b
        const double d2 = __builtin_fma(J00, J11, -(J01 * J10));
        const double r2 = rcp_nr(d2), nr2 = -r2;
        qdl[0] = w * cf[6] * d2;                       // w det J (cf[6] = sgn zs: the sign of the permutation (a, b, sweep))
        qdl[1] = J11 * r2; qdl[2] = J10 * nr2; qdl[3] = 0.;
        qdl[4] = J01 * nr2; qdl[5] = J00 * r2; qdl[6] = 0.;
        qdl[7] = 0.; qdl[8] = 0.; qdl[9] = cf[7];      // 1 / zs
      } else if (geo) {  // SetupGeo (common.h:47-101) recomputed at this point from the element's trilinear map
        const uint32_t pk = pqi[r];
        const auto lb = (ldsb_t)lds0;
        const ldsp_t ti = (ldsp_t)(lb + oGT + (pk & 0xFFu)), tj = (ldsp_t)(lb + oGT + ((pk >> 8) & 0xFFu)),
                     tk = (ldsp_t)(lb + oGT + ((pk >> 16) & 0xFFu)), cf = (ldsp_t)(lb + oGC + (pk >> 24) * (GEO_NCOEF * 8));
        const double xi = ti[0], eta = tj[0], zeta = tk[0], w = ti[Q] * tj[Q] * tk[Q];
        const double xe = xi * eta, xz = xi * zeta, ez = eta * zeta;
        double Jg[9];
#pragma unroll
        for (int c = 0; c < 3; c++) {  // m: 0 xi, 1 eta, 2 zeta, 3 xi eta, 4 xi zeta, 5 eta zeta, 6 xi eta zeta
          const double a0 = cf[c * 7 + 0], a1 = cf[c * 7 + 1], a2 = cf[c * 7 + 2], a3 = cf[c * 7 + 3], a4 = cf[c * 7 + 4],
                       a5 = cf[c * 7 + 5], a6 = cf[c * 7 + 6];
          Jg[0 * 3 + c] = a0 + a3 * eta + a4 * zeta + a6 * ez;
          Jg[1 * 3 + c] = a1 + a3 * xi + a5 * zeta + a6 * xz;
          Jg[2 * 3 + c] = a2 + a4 * xi + a5 * eta + a6 * xe;
        }
        qf_setup_geo_rcp(Jg, w, qdl);
      } else {
#pragma unroll
        for (int c = 0; c < 10; c++) qdl[c] = qd[r % NSET][c];
      }
      if (live) {
        if constexpr (QF == QF_HYPERFS_F) {
          double dso[10];
          double *db = ka->state_out2;      // wave-uniform: also write the derived state of the tangent?
          qf_point<QF, GEO == 3>(Phys{ka->nu, ka->E, ka->lambda, ka->TwoMu}, ug, qdl, st[r % NSET], dv, sto, db ? dso : nullptr);
          if (db) {
            db += (size_t)(ka->elem_begin + grp * E) * (10 * QS);
            const uint32_t vd = (uint32_t)(pel * (10 * QS) + pq);
#pragma unroll
            for (int c = 0; c < 10; c++) (db + c * QS)[vd] = dso[c];
          }
        } else {
          qf_point<QF, GEO == 3>(Phys{ka->nu, ka->E, ka->lambda, ka->TwoMu}, ug, qdl, st[r % NSET], dv, sto);
        }
        if constexpr (ST_OUT) {
          double *sb = ka->state_out + (size_t)(ka->elem_begin + grp * E) * (9 * QS);
          const uint32_t vs = (uint32_t)(pel * (9 * QS) + pq);
#pragma unroll
          for (int c = 0; c < 9; c++) (sb + c * QS)[vs] = sto[c];
        }
      } else {
#pragma unroll
        for (int c = 0; c < 9; c++) dv[c] = 0.;
      }
      if constexpr (MASS) {   // the mass term's point values (a dead element's are zero: its gathered u is)
        const double mw = live ? ka->mass_c * qdl[0] : 0.;
        uq[r][0] *= mw; uq[r][1] *= mw; uq[r][2] *= mw;
      }
      // refill this register set for the round NSET further down the stream (this group or the next)
      if (r + NSET < RQ) load_point(qd[r % NSET], st[r % NSET], grp, r + NSET);
      else load_point(qd[r % NSET], st[r % NSET], g_nx, r + NSET - RQ);
      if (okp) {
        if constexpr (GEO == 3) {
          lds_wr<0 * BC>(pd0, dv[0]); lds_wr<1 * BC>(pd0, dv[1]); lds_wr<2 * BC>(pd0, dv[2]);
          lds_wr<0 * BC>(pd1, dv[3]); lds_wr<1 * BC>(pd1, dv[4]); lds_wr<2 * BC>(pd1, dv[5]);
          lds_wr<0 * BC>(pd2, dv[6]); lds_wr<1 * BC>(pd2, dv[7]); lds_wr<2 * BC>(pd2, dv[8]);
        } else {
          lds_wr<oBX + 0 * BC>(aPt[r], dv[0]); lds_wr<oBX + 1 * BC>(aPt[r], dv[1]); lds_wr<oBX + 2 * BC>(aPt[r], dv[2]);
          lds_wr<oA + 0 * BC>(aPt[r], dv[3]);  lds_wr<oA + 1 * BC>(aPt[r], dv[4]);  lds_wr<oA + 2 * BC>(aPt[r], dv[5]);
          lds_wr<oBZ + 0 * BC>(aPt[r], dv[6]); lds_wr<oBZ + 1 * BC>(aPt[r], dv[7]); lds_wr<oBZ + 2 * BC>(aPt[r], dv[8]);
        }
      }
    }

    // ---- gradient^T --------------------------------------------------------------------------------------
    __builtin_amdgcn_s_setprio(PRIO_PASS);
    CPS_PH(16);
    pencil_pass<Q, Q, Q, true, BI, oBX, oBX, -1, EO>(tDt, aIQ, lQQ, N_QQ);  // B1: W1 = Dx^T g0, BX in place
    CPS_PH(17);
    if (!B_QQ || lQQ < 0) {  // B2: W2 = W1 + Dy^T g1, A in place.  Two inputs per task: software-pipelined over the rounds
       // (two rounds of inputs live instead of all)
      if constexpr (table_splits<Q, Q, EO>() == 1) {
        const ktab_t tD = ktab_fresh(tDt);
        double in[2][Q], acc[2][Q];
        if (pencil_ok_ld(lQQi, 0, N_QQi)) { pencil_ld<Q, BJ, oA>(aJQ[0], in[0]); pencil_ld<Q, BJ, oBX>(aJQ[0], acc[0]); }
#pragma unroll
        for (int r = 0; r < R_JQ; r++) {
          if (r + 1 < R_JQ && pencil_ok_ld(lQQi, r + 1, N_QQi)) {
            pencil_ld<Q, BJ, oA>(aJQ[r + 1], in[(r + 1) & 1]);
            pencil_ld<Q, BJ, oBX>(aJQ[r + 1], acc[(r + 1) & 1]);
          }
          if (pencil_ok_ld(lQQi, r, N_QQi)) {
            mac_sel<Q, Q, Q, true, -1, EO>(tD, in[r & 1], acc[r & 1]);
            if (pencil_ok(lQQi, r, N_QQi)) pencil_st<Q, BJ, oA>(aJQ[r], acc[r & 1]);
          }
        }
      } else {  // large tables: all rounds live, the table in row blocks
        double in[R_JQ][Q], acc[R_JQ][Q];
#pragma unroll
        for (int r = 0; r < R_JQ; r++) {
#pragma unroll
          for (int o = 0; o < Q; o++) acc[r][o] = 0.;
          if (pencil_ok_ld(lQQi, r, N_QQi)) { pencil_ld<Q, BJ, oA>(aJQ[r], in[r]); pencil_ld<Q, BJ, oBX>(aJQ[r], acc[r]); }
        }
        mac_rounds<Q, Q, Q, true, R_JQ>(ktD, in, acc, lQQi, N_QQi);
#pragma unroll
        for (int r = 0; r < R_JQ; r++)
          if (pencil_ok(lQQi, r, N_QQi)) pencil_st<Q, BJ, oA>(aJQ[r], acc[r]);
      }
    }
    if constexpr (MASS) {   // W2 += c w det J u_q at this lane's points: behind B2's stores and before B3's loads in the wave's LDS queue
#pragma unroll
      for (int r = 0; r < RQ; r++)
        if (pencil_ok(lane, r, E * Q3)) {
          const double w0 = lds_rd<oA + 0 * BC>(aPt[r]), w1 = lds_rd<oA + 1 * BC>(aPt[r]), w2 = lds_rd<oA + 2 * BC>(aPt[r]);
          lds_wr<oA + 0 * BC>(aPt[r], w0 + uq[r][0]); lds_wr<oA + 1 * BC>(aPt[r], w1 + uq[r][1]); lds_wr<oA + 2 * BC>(aPt[r], w2 + uq[r][2]);
        }
    }
    CPS_PH(18);
    if (!B_QQ || lQQ < 0) {  // B3: along k: A[k<P] = B^T W2 + G^T g2, in two sweeps so that one coefficient table is live at a time
      double out[R_K][P];
      if constexpr (table_splits<P, Q, EO>() > 1) {  // large tables: all rounds live, the tables in row blocks
        double in[R_K][Q];
#pragma unroll
        for (int r = 0; r < R_K; r++) {
#pragma unroll
          for (int m = 0; m < P; m++) out[r][m] = 0.;
          if (pencil_ok_ld(lQQi, r, N_QQi)) pencil_ld<Q, BK, oA>(aK[r], in[r]);
        }
        mac_rounds<P, Q, P, true, R_K>(ktB, in, out, lQQi, N_QQi);
#pragma unroll
        for (int r = 0; r < R_K; r++)
          if (pencil_ok_ld(lQQi, r, N_QQi)) pencil_ld<Q, BK, oBZ>(aK[r], in[r]);
        mac_rounds<P, Q, P, true, R_K, true>(ktG, in, out, lQQi, N_QQi);
#pragma unroll
        for (int r = 0; r < R_K; r++)
          if (pencil_ok(lQQi, r, N_QQi)) pencil_st<P, BK, oA>(aK[r], out[r]);
      } else {
      {
        const ktab_t tB = ktab_fresh(tBt);
        double in[2][Q];
        if (pencil_ok_ld(lQQi, 0, N_QQi)) pencil_ld<Q, BK, oA>(aK[0], in[0]);
#pragma unroll
        for (int r = 0; r < R_K; r++) {
          if (r + 1 < R_K && pencil_ok_ld(lQQi, r + 1, N_QQi)) pencil_ld<Q, BK, oA>(aK[r + 1], in[(r + 1) & 1]);
#pragma unroll
          for (int m = 0; m < P; m++) out[r][m] = 0.;
          if (pencil_ok_ld(lQQi, r, N_QQi)) mac_sel<P, Q, P, true, +1, EO>(tB, in[r & 1], out[r]);
        }
      }
      {
        // not before the first sweep has used its table: both at once do not fit the SGPR file (they were spilled)
        const ktab_t tG = ktab_fresh_after<R_K * P>(tGt, &out[0][0]);
        double in2[2][Q];
        if (pencil_ok_ld(lQQi, 0, N_QQi)) pencil_ld<Q, BK, oBZ>(aK[0], in2[0]);
#pragma unroll
        for (int r = 0; r < R_K; r++) {
          if (r + 1 < R_K && pencil_ok_ld(lQQi, r + 1, N_QQi)) pencil_ld<Q, BK, oBZ>(aK[r + 1], in2[(r + 1) & 1]);
          if (pencil_ok_ld(lQQi, r, N_QQi)) {
            mac_sel<P, Q, P, true, -1, EO>(tG, in2[r & 1], out[r]);
            if (pencil_ok(lQQi, r, N_QQi)) pencil_st<P, BK, oA>(aK[r], out[r]);
          }
        }
      }
      }
    }
    CPS_PH(19);
    load_x(off_nx, xin);  // next group's x (its offsets landed long ago): issued this late so its 6 RN registers
                          // are not live across the physics and the register-hungry passes; B4, B5, the
                          // final store and the next gather's address work hide most of its latency
    // ---- B^T: points -> nodes ---------------------------------------------------------------------------
    pencil_pass<Q, P, P, true, BJ, oA, oA, +1, EO>(tBt, aJP, lQP, N_JP);    // B4: along j
    CPS_PH(20);
    pencil_pass<Q, P, P, true, BI, oA, oA, +1, EO>(tBt, aIP, lPP, N_IP);    // B5: along i
    CPS_PH(21);
    // ---- final: node owners -> y (element-interior nodes) / shell E-vector (plain coalesced stores) ------------------
    {
      double v[RN][3];
#pragma unroll
      for (int r = 0; r < RN; r++)
        if (pencil_ok(lane, r, E * P3)) {
          v[r][0] = lds_rd<oA + 0 * BC>(aNd[r]); v[r][1] = lds_rd<oA + 1 * BC>(aNd[r]); v[r][2] = lds_rd<oA + 2 * BC>(aNd[r]);
        }
      const kargs_t ka = kargs_fresh<KA>();
#pragma unroll
      for (int r = 0; r < RN; r++) {
        const int nel = el_of(lane + 64 * r, P3);
        if (pencil_ok(lane, r, E * P3) && grp * E + nel < ka->nelem) {
          if ((nd_interior >> r) & 1u) {  // no contributor outside this wave: the node's final value goes straight to y
            const uint32_t base = off[r] & OFF_MASK;
            const uint32_t fl = ka->mask_out ? (off[r] >> OFF_FLAG_SHIFT) : 0u;
            double *yb = ka->y;
            yb[base] = (fl & 1u) ? 0. : v[r][0]; (yb + 1)[base] = (fl & 2u) ? 0. : v[r][1]; (yb + 2)[base] = (fl & 4u) ? 0. : v[r][2];
          } else {
            double *eb = ka->evec + (size_t)(ka->elem_begin + grp * E) * ka->evec_stride;
            const uint32_t ve = (r % 2) ? (ev_idx[r / 2] >> 16) : (ev_idx[r / 2] & 0xFFFFu);
            eb[ve] = v[r][0]; (eb + 1)[ve] = v[r][1]; (eb + 2)[ve] = v[r][2];
          }
        }
      }
    }
    CPS_PH(22);
#ifdef CPS_PHASE_TIMING
    if (ph_iter == CPS_PHASE_TIMING && lane == 0 && ph_buf) ph_buf[(size_t)blockIdx.x * 32 + 25] = wall_clock64();
    ph_iter++;
#endif
    if (!more) break;
    grp = grp_nx;
#pragma unroll
    for (int r = 0; r < RN; r++) off[r] = off_nx[r];
  }
