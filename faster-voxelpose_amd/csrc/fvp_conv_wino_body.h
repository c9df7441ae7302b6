// The body of the Winograd kernels of fvp_conv_wino.hip - k_conv_wino (SH = 0) and k_conv_wsc (SH = 1, 2) - included inside
// each of the two kernel templates: NOT a header of its own.  The including function provides the kernel argument `a` and the
// compile-time constants WC, WT, CC, NI, HAS_RES, RESW, CW, SH and SKIP.  (One text instead of a shared __device__ function: behind
// a call boundary hipcc allocates the scalar registers of the own-patch instances differently - one of them spilled.)
  static_assert(SH == 0 || ((SH == 1 || SH == 2) && CW == 2), "shared columns: two-block waves");
  constexpr bool kSkip = SKIP != 0;                  // SKIP = MFMA steps (4 channels each) of the fused 1x1 skip conv, 0: none
  static_assert(SKIP == 0 || ((SKIP == 4 || SKIP == 8) && HAS_RES), "the fused skip is the residual: 16 or 32 channels");
  HIP_DYNAMIC_SHARED(float, smem)
  constexpr int NWV = WC * WT;                       // waves per workgroup: 8 / 16 (one workgroup per CU) or 4 (two per CU)
  constexpr int NT = NWV * 64;
  static_assert(NWV == 16 || NWV == 8 || NWV == 4, "4, 8 or 16 waves");
  static_assert(CW == 1 || CW == 2, "cout blocks per wave");
  static_assert(CC == 4 || CC == 8, "chunk");
  static_assert(NI >= 1 && NI <= 4, "input DMA rounds");
  constexpr int CBW = 16 * CW * WC;                  // couts of the workgroup
  constexpr int WCH = CC * CBW * 16;                 // floats of one weight chunk
  constexpr int WS_SZ = RESW ? 0 : WCH;              // ... streamed through a slot
  constexpr int NW = RESW ? 0 : CC * CBW * 4 / NT;   // weight DMA instructions per wave per chunk
  static_assert(RESW || (CC * CBW * 4) % NT == 0, "whole weight DMA rounds");
  constexpr int NPS = NI + NW;                       // DMA instructions per wave per chunk
  constexpr int S = CC / 4;                          // steps (4 channels) per chunk
  constexpr int XS_SZ = NI * NT * 4;                 // input slot: NI rounds of one 16-byte item per thread (floats)
  constexpr int BUF_SZ = XS_SZ + WS_SZ;              // one ring slot
  constexpr bool kDiag = FVP_WINO_ABLATE != 0;       // ablation switches: a variant build only (see FVP_WINO_ABLATE)
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int k4 = lane >> 4, l15 = lane & 15;
  const int wc = wave % WC, wt = wave / WC;
  const int W = a.W, THp = a.TH + 2, WP = W + 4;
  const int plane_sz = THp * WP;
  const int CS = a.TN * plane_sz;
  const int ablate = kDiag ? a.ablate : 0;
  const bool dma = !(ablate & 1);

  // ---- LDS map (floats): [4 pad][3 ring slots][resident weights][bias | scale | shift][plane-group flags]
  // (SKIP: [the skip's bias | scale | shift][the skip's weights] behind the flags, at a.skip_off)
  const int epi_off = 4 + 3 * BUF_SZ + (RESW ? a.cinp * CBW * 16 : 0);
  const unsigned char* const vflag = reinterpret_cast<const unsigned char*>(smem + epi_off + 3 * a.coutp);

  // Persistent workgroups: unit u = (plane group, row band, cout block); workgroup b walks
  // u = b, b + G, b + 2G, ... (G = gridDim.x <= number of CUs).  The chunk stream (DMA two chunks
  // ahead) runs across unit boundaries, so a unit's first chunks land while the previous unit is
  // still computing and there is no workgroup relaunch between tiles.  Units of invalid plane groups
  // (persons below the score threshold) are skipped: flags from global memory while the prologue runs,
  // from their LDS copy afterwards (a global load inside the K loop would sit in the vmcnt queue of the ring).
  const int G = gridDim.x, nunits = a.nunits;
  auto next_unit = [&](int u, auto from_lds) {
    if (a.nflags > 0) {
      while (u < nunits) {
        const int pg = fdiv_nb(fdiv_nb(u, a.m_ys), a.m_ty);
        const int f = fdiv_nb(pg, a.m_vd);
        const int ok = decltype(from_lds)::value ? int(vflag[f]) : int(a.plane_valid[f]);
        if (__builtin_amdgcn_readfirstlane(ok)) break;
        u += G;
      }
    }
    return u;
  };
  using LdsFlags = std::integral_constant<bool, true>;
  using GlobalFlags = std::integral_constant<bool, false>;
  int u = next_unit(int(blockIdx.x), GlobalFlags{});
  if (u >= nunits) return;

  // this lane's 2x2 output tile inside the workgroup tile: TN planes x TR rows x tpr tiles; lanes beyond that
  // product (row lengths that do not divide 16*WT) compute on tile 0's data and store nothing
  // (SH = 2: two tile rows interleaved in the DPP row, lane 2 * tx + row)
  const int q0 = wt * 16 + (SH == 2 ? ((l15 & 1) << 3) | (l15 >> 1) : l15);
  int poff;
  {
    const bool q_ok = q0 < a.TN * a.tpp;
    const int q = q_ok ? q0 : 0;
    const int tn = fdiv_nb(q, a.m_tpp), trem = q - tn * a.tpp;
    const int ty = fdiv_nb(trem, a.m_tpr), tx = trem - ty * a.tpr;
    // LDS row 0 of the tile is image row y0 - 1; column 4 of a row slot is image x = 0
    poff = tn * plane_sz + 2 * ty * WP + 3 + 2 * tx + k4 * CS;
  }
  const int swz = (l15 >> 2) & 3;
  // A operand of quad xi: float index ((row * 4 + (xi ^ swz)) * 4 = a0 ^ (xi << 2), a0 = row * 16 + swz * 4 (cout block cb adds
  // 16 rows = 256 floats).  The two-block form keeps the four offsets in registers; the one-block form (128 registers in all)
  // keeps a0 and pays three XORs per fetch.
  const int a0 = (k4 * CBW + wc * (16 * CW) + l15) * 16 + swz * 4;
  int aoff[4];
#pragma unroll
  for (int xi = 0; xi < 4; ++xi) aoff[xi] = a0 ^ (xi << 2);
  const float* const wres = smem + 4 + 3 * BUF_SZ;   // RESW: resident weights [cinp][CBW][16]
  // first weight float of chunk k living in slot `slot` (streamed) or in the resident copy
  auto wchunk = [&](const float* slot, int k) { return RESW ? wres + k * WCH : slot + XS_SZ; };

  f32x4 acc[CW][16];

  const int HW = a.H * W;
  const int nchunks = a.cinp / CC;

  // ---- LDS-DMA items.  Input item j of this lane: quad `qd` of row `row` of the slot (rows = channel-major, then
  // plane, then row of the band; quad 0 is the left zero margin; the item behind the last row is the zero quad the
  // halo reads of the last row run into).  Its byte offset from the unit's descriptor base (plane group's first plane,
  // channel 0 of the chunk, one row above the band) is unit-independent; whether it lies inside the image depends on
  // the unit's band (top / bottom rows) and plane group (last, partial one).  Bit 31 = outside: the buffer range check
  // fails and the hardware writes zeros to LDS (tools/micro/buflds.hip) - no zero page, no select, no vector
  // instruction per chunk.  The item's (row, plane) is recomputed from the lane number when the cursor enters a unit
  // (a dozen vector instructions per item and unit) rather than kept in a register.
  unsigned voff[NI];
  // (row in band, plane in group) of input item j of this lane and whether the item can lie inside the image at all
  auto item_pos = [&](int j, int& ry, int& n, bool& inside, int& ci, int& qd) {
    const int qpr = (W >> 2) + 1;
    const int rows_per_ch = a.TN * THp;
    const int nin = CC * rows_per_ch * qpr + 1;      // + the zero quad behind the last row
    int ln = lane;
    FVP_OPAQUE_V(ln);                                // (recomputed where it is used: per unit, not kept in registers)
    const int it = (wave + NWV * j) * 64 + ln;
    const int row = fdiv_nb(it, a.m_qpr);
    qd = it - row * qpr;
    ci = fdiv_nb(row, a.m_rpc);
    const int rem = row - ci * rows_per_ch;
    n = fdiv_nb(rem, a.m_thp);
    ry = rem - n * THp;
    inside = it < nin && qd > 0 && ci < CC;
  };
#pragma unroll
  for (int j = 0; j < NI; ++j) {
    int ry, n, ci, qd;
    bool inside;
    item_pos(j, ry, n, inside, ci, qd);
    voff[j] = inside ? unsigned((n * a.cin + ci) * HW + ry * W + 4 * (qd - 1)) * 4u : 0u;
    __builtin_amdgcn_sched_barrier(0);
  }
  // this lane's weight item j: channel ci0 + j * DCI of the chunk, quad qd0 of the cout block's row
  constexpr int DCI = NT / (CBW * 4);
  const unsigned woffb = (unsigned(t / (CBW * 4)) * unsigned(a.coutp) * 16u + 4u * unsigned(t % (CBW * 4))) * 4u;
  const unsigned wdj4 = unsigned(DCI) * unsigned(a.coutp) * 64u;        // bytes between weight items j and j + 1
  const unsigned in_step4 = unsigned(CC) * unsigned(HW) * 4u;           // bytes per chunk: input, weights
  const unsigned w_step4 = unsigned(CC) * unsigned(a.coutp) * 64u;
  const unsigned lds0 = FVP_LDS_BYTE_ADDRESS(smem) + 16u + unsigned(wave) * 1024u;   // this wave's first item of slot 0
  i32x4 rs_in = {0, 0, 0x7ffffff0, 0x00020000}, rs_w = {0, 0, 0x7ffffff0, 0x00020000};   // raw buffers, stride 0
  auto set_base = [](i32x4& rs, const float* p) {
    const unsigned long long b = reinterpret_cast<unsigned long long>(p);
    rs[0] = __builtin_amdgcn_readfirstlane(int(unsigned(b)));
    rs[1] = __builtin_amdgcn_readfirstlane(int(unsigned(b >> 32) & 0xffffu));
  };
  int su = u, sk = 0;                                // DMA cursor (unit su, chunk sk)
  auto enter_unit = [&](int su_) {
    const KArgsPtr ka = FVP_FRESH_ARGS(a);
    const int ys = ka->ysplit, tys = ka->tiles_y;
    const int st = fdiv_nb(su_, ka->m_ys), sy = su_ - st * ys;
    const int spg = fdiv_nb(st, ka->m_ty), sty = st - spg * tys;
    const int splane0 = spg * ka->TN, sy0 = sty * ka->TH;
    const int H = ka->H, planes = ka->planes;
    // row 0 of a slot is image row sy0 - 1: the descriptor starts one row above the band so that offsets are >= 0
    set_base(rs_in, ka->src + size_t(splane0) * ka->cin * HW + sy0 * W - W);
    set_base(rs_w, ka->wts + size_t(sy) * (CBW * 16));
#pragma unroll
    for (int j = 0; j < NI; ++j) {
      int ry, n, ci, qd;
      bool inside;
      item_pos(j, ry, n, inside, ci, qd);
      const bool ok = inside && unsigned(sy0 + ry - 1) < unsigned(H) && splane0 + n < planes;
      voff[j] = (voff[j] & 0x7fffffffu) | (ok ? 0u : kWinoOOB);
      __builtin_amdgcn_sched_barrier(0);             // one item at a time: the items' temporaries must not pile up (16-wave form: 128 registers)
    }
  };
  // every wave issues exactly NPS DMA instructions per chunk (counted s_waitcnt vmcnt below)
  auto stage = [&](int k, int slot) {
    const unsigned la0 = lds0 + unsigned(slot) * unsigned(BUF_SZ * 4);
    const unsigned so_in = unsigned(k) * in_step4;
#pragma unroll
    for (int j = 0; j < NI; ++j) asm_buffer_load_lds16(la0 + unsigned(NWV * j) * 1024u, voff[j], rs_in, so_in);
    const unsigned so_w = unsigned(k) * w_step4;
#pragma unroll
    for (int j = 0; j < NW; ++j)
      asm_buffer_load_lds16(la0 + unsigned(XS_SZ * 4 + NWV * j * 1024), woffb, rs_w, so_w + unsigned(j) * wdj4);
  };
  enter_unit(su);
  // stage the cursor's chunk into `slot` and advance; false once every unit has been requested
  auto stage_next = [&](int slot, auto from_lds) {
    if (su >= nunits) return false;
    stage(sk, slot);
    if (++sk == nchunks) {
      sk = 0;
      su = next_unit(su + G, from_lds);
      if (su < nunits) enter_unit(su);
    }
    return true;
  };

  // ---- operand fetch / transform / MFMA building blocks
  float4 av[CW][4];
  float d[4][4];                                     // the lane's 4x4 patch
  float v[4][4];                                     // V[xi][nu] = B^T d B
  auto fetch_a = [&](int cb, const float* wbase, int s) {     // wbase = weights of the chunk, s = step in chunk
    if (kDiag && (ablate & 256)) return;                      // diagnostics: no A-operand reads
    int a0o = a0;
    if (CW == 1) FVP_OPAQUE_V(a0o);                  // (recomputed per fetch: hipcc would hoist the four offsets again)
#pragma unroll
    for (int xi = 0; xi < 4; ++xi)
      av[cb][xi] = *reinterpret_cast<const float4*>(wbase + (CW == 1 ? (a0o ^ (xi << 2)) : aoff[xi]) + (s * 4 * CBW * 16 + cb * 256));
  };
  // (shared-column form: the lane's own two columns only - the outer ones, the reads with the built-in 2-way bank conflict,
  // are never fetched)
  auto fetch_d = [&](const float* base, int s, int wp) {
    const float* xs = base + poff + s * 4 * CS;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float* row = xs + r * wp;
      const float2 m = *reinterpret_cast<const float2*>(row + 1);       // 8-byte aligned: column 4 + 2*tx
      if (SH == 0) d[r][0] = row[0];
      d[r][1] = m.x;
      d[r][2] = m.y;
      if (SH == 0) d[r][3] = row[3];
    }
  };
  // V = B^T d B as 32 plain scalar adds (rows, then columns); the patch registers die in the row pass.
  // Shared-column form (SH != 0), 24 adds.  Horizontally adjacent tiles overlap by two patch columns: tr[xi][0] of a tile is
  // tr[xi][2] of its left neighbour and tr[xi][3] is tr[xi][1] of its right neighbour - the same two operands in the same
  // operation, the same bits.  The lane runs the row pass on its own two columns only (8 adds), and the column pass takes the
  // neighbours' values as the DPP source operand of its outer subtractions (v_sub_f32 / v_subrev_f32 with row_shr / row_shl:
  // no instruction of their own).  A tile at an image border gets +0.0 from beyond the end of the DPP row - what the row pass
  // makes of the DMA's zero margin, (+0) +- (+0).
  auto transform = [&](float (&tr)[4][4]) {
#pragma unroll
    for (int c = (SH ? 1 : 0); c < (SH ? 3 : 4); ++c) {
      tr[0][c] = d[0][c] - d[2][c];
      tr[1][c] = d[1][c] + d[2][c];
      tr[2][c] = d[2][c] - d[1][c];
      tr[3][c] = d[1][c] - d[3][c];
    }
  };
  auto columns = [&](const float (&tr)[4][4]) {
#pragma unroll
    for (int xi = 0; xi < 4; ++xi) {
      if constexpr (SH == 0) {
        v[xi][0] = tr[xi][0] - tr[xi][2];
      } else {
        v[xi][0] = dpp_row_neighbour<SH, true>(tr[xi][2]) - tr[xi][2];
      }
      v[xi][1] = tr[xi][1] + tr[xi][2];
      v[xi][2] = tr[xi][2] - tr[xi][1];
      if constexpr (SH == 0) {
        v[xi][3] = tr[xi][1] - tr[xi][3];
      } else {
        v[xi][3] = tr[xi][1] - dpp_row_neighbour<SH, false>(tr[xi][1]);
      }
    }
  };
  // first = the unit's first step: the MFMAs take the constant 0 as C (clearing the 128 accumulator registers between
  // units cost 128 vector moves per wave and unit - and on this part a vector instruction of either wave of a SIMD is
  // matrix time lost: tools/micro/coexec.hip)
  auto mfma16 = [&](int cb, auto firstc) {
    if (kDiag && (ablate & 4)) return;                        // diagnostics: no MFMA
    const f32x4 z = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int xi = 0; xi < 4; ++xi) {
      const float aw[4] = {av[cb][xi].x, av[cb][xi].y, av[cb][xi].z, av[cb][xi].w};
#pragma unroll
      for (int nu = 0; nu < 4; ++nu)
        acc[cb][4 * xi + nu] = __builtin_amdgcn_mfma_f32_16x16x4f32(
            aw[nu], v[xi][nu], decltype(firstc)::value ? z : acc[cb][4 * xi + nu], 0, 0, 0);
    }
  };

  // ---- prologue: resident weights, BN vectors, validity flags, the first two chunks
  if (RESW) {                                        // cinp * CBW * 4 quads, NT per round
    const int rounds = (a.cinp * CBW * 4) / NT;
    for (int j = 0; j < rounds; ++j)
      asm_global_load_lds16(a.wts + size_t((wave + NWV * j) * 64 + lane) * 4,
                            __builtin_amdgcn_readfirstlane(FVP_LDS_BYTE_ADDRESS(smem) +
                                                           4u * unsigned(4 + 3 * BUF_SZ + (wave + NWV * j) * 256)));
  }
  // bias | scale | shift of every cout, [3][coutp], behind the slots (and the resident weights): the epilogue reads them
  // with ds_read (lgkmcnt).  As global loads they sat in the in-order vmcnt queue behind the previous cout's stores.
  {
    float* const e = const_cast<float*>(smem) + epi_off;
    for (int i = t; i < 3 * a.coutp; i += NT) e[i] = a.epi[i];
    unsigned char* const f = const_cast<unsigned char*>(vflag);
    for (int i = t; i < a.nflags; i += NT) f[i] = a.plane_valid[i];
  }
  // SKIP: the 1x1 skip conv's BN vectors and weights, once per workgroup.  Weights as A operands of its 16x16x4 MFMAs:
  // Ws[cout][k4][g][j] = W[channel 4 (4 g + j) + k4][cout] - one ds_read_b128 gives a lane (cout, k4) four steps.
  if constexpr (kSkip) {
    float* const e = const_cast<float*>(smem) + a.skip_off;
    for (int i = t; i < 3 * a.coutp; i += NT) e[i] = a.skip_epi[i];
    float* const w = e + 3 * a.coutp;
    constexpr int sg = SKIP / 4;
    for (int i = t; i < a.skip_cin * a.coutp; i += NT) {
      const int ci = i / a.coutp, co = i - ci * a.coutp;
      w[((co * 4 + (ci & 3)) * sg + (ci >> 4)) * 4 + ((ci >> 2) & 3)] = a.skip_wts[i];
    }
  }
  if (dma) {
    stage_next(0, GlobalFlags{});
    stage_next(1, GlobalFlags{});
  }
  wait_vmcnt_imm<0>();                               // both chunks (and the resident weights) have landed: see chunk_barrier
  __syncthreads();

  int cur = 0;                                       // ring slot of the chunk being consumed
  auto slot_ptr = [&](int slot) { return smem + 4 + slot * BUF_SZ; };
  fetch_a(0, wchunk(slot_ptr(0), 0), 0);
  fetch_d(slot_ptr(0), 0, WP);
  while (true) {
    // The chunk body exists twice: the unit's first chunk (its first step's MFMAs take C = 0, its barrier needs no vmcnt
    // wait) and every other one.
    auto chunk = [&](int k, auto firstc) {
      constexpr bool kFirst = decltype(firstc)::value;
      const int nxt = cur == 2 ? 0 : cur + 1;
      const int nn = nxt == 2 ? 0 : nxt + 1;
      const bool more = dma && stage_next(nn, LdsFlags{});
      const float* const cs = slot_ptr(cur);
      const float* const ns = slot_ptr(nxt);
      int wp = WP;
      FVP_OPAQUE(wp);
      if constexpr (CW == 2) {
#pragma unroll
      for (int s = 0; s < S; ++s) {
        // ---- half-step 0: patch transform, cout block 0
        __builtin_amdgcn_s_waitcnt(0xc07f);          // lgkmcnt(0): av[0] and the patch have landed
        __builtin_amdgcn_sched_barrier(0);
        fetch_a(1, wchunk(cs, k), s);
        __builtin_amdgcn_sched_barrier(0);           // issue the reads now: left alone hipcc sinks them below the MFMAs
        float tr[4][4];
        if (kDiag && (ablate & 512)) {               // diagnostics: no input transform
#pragma unroll
          for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) v[r][c] = d[r][(SH && (c == 0 || c == 3)) ? 1 : c];
        } else {
          transform(tr);
        }
        if (s + 1 < S) fetch_d(cs, s + 1, wp);       // the patch registers are dead: refill for the next step
        __builtin_amdgcn_sched_barrier(0);
        if (!(kDiag && (ablate & 512))) columns(tr);
        if (kFirst && s == 0) mfma16(0, std::integral_constant<bool, true>{});
        else mfma16(0, std::integral_constant<bool, false>{});
        __builtin_amdgcn_sched_barrier(0);
        // ---- half-step 1: cout block 1; the last one of a chunk crosses into the next slot
        __builtin_amdgcn_s_waitcnt(0xc07f);
        __builtin_amdgcn_sched_barrier(0);
        if (s + 1 < S) {
          fetch_a(0, wchunk(cs, k), s + 1);
        } else {
          // All reads of this slot are complete (lgkmcnt above); once every wave is here the slot may be overwritten by
          // the DMA of chunk g+3, and chunk g+1 has landed for everybody: every wave waits for ITS items of chunk g+1
          // (vmcnt(NPS): only the NPS instructions of chunk g+2 may still be in flight) before the barrier.  A unit's
          // first chunk needs no wait: chunk g+1 was requested before the previous unit's epilogue, whose vmcnt(0) (or the
          // prologue's) it has passed - and the epilogue's stores may stay in flight across this barrier.
          if (!kFirst && dma) {
            if (more) wait_vmcnt_imm<NPS>();
            else wait_vmcnt_imm<0>();
          }
          if (!(kDiag && (ablate & 128))) __builtin_amdgcn_s_barrier();     // plain barrier: no fence, the counters are ours
          if (k + 1 < nchunks) {                     // (a unit's last chunk: the epilogue needs the registers)
            fetch_a(0, wchunk(ns, k + 1), 0);
            fetch_d(ns, 0, wp);
          }
        }
        __builtin_amdgcn_sched_barrier(0);
        if (kFirst && s == 0) mfma16(1, std::integral_constant<bool, true>{});
        else mfma16(1, std::integral_constant<bool, false>{});
        __builtin_amdgcn_sched_barrier(0);
      }
      } else {
        // ---- one cout block per wave (four waves per SIMD): per step  wait - transform - 16 MFMAs - request the next
        // step's operands.  Nothing is double-buffered (patch, V and the next patch share 16 registers: with the next
        // patch in flight beside V the wave would need 128 registers before anything else): the other three waves of the
        // SIMD cover the LDS latency.
#pragma unroll
        for (int s = 0; s < S; ++s) {
          __builtin_amdgcn_s_waitcnt(0xc07f);        // lgkmcnt(0): av[0] and the patch have landed
          __builtin_amdgcn_sched_barrier(0);
          {
            float tr[4][4];
            transform(tr);
            columns(tr);
          }
          __builtin_amdgcn_sched_barrier(0);
          if (kFirst && s == 0) mfma16(0, std::integral_constant<bool, true>{});
          else mfma16(0, std::integral_constant<bool, false>{});
          __builtin_amdgcn_sched_barrier(0);
          if (s + 1 < S) {
            fetch_a(0, wchunk(cs, k), s + 1);
            fetch_d(cs, s + 1, wp);
          } else {
            // (chunk barrier: see the two-block form above; no LDS read of this slot is pending here)
            if (!kFirst && dma) {
              if (more) wait_vmcnt_imm<NPS>();
              else wait_vmcnt_imm<0>();
            }
            __builtin_amdgcn_s_barrier();
            if (k + 1 < nchunks) {
              fetch_a(0, wchunk(ns, k + 1), 0);
              fetch_d(ns, 0, wp);
            }
          }
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      cur = nxt;
    };
    chunk(0, std::integral_constant<bool, true>{});
    for (int k = 1; k < nchunks; ++k) chunk(k, std::integral_constant<bool, false>{});

    // ---- unit finished: output transform + epilogue, then the next unit of this workgroup.  Everything the epilogue
    // needs from the launch arguments is read here, not kept in SGPRs across the K loop.
    if (!(ablate & 8)) {
      const KArgsPtr ka = FVP_FRESH_ARGS(a);
      const int ys = ka->ysplit, tys = ka->tiles_y;
      const int ut = fdiv_nb(u, ka->m_ys), uy = u - ut * ys;
      const int pg = fdiv_nb(ut, ka->m_ty), ty_i = ut - pg * tys;
      const int plane0 = pg * ka->TN, y0 = ty_i * ka->TH, co0 = uy * CBW;
      const int cout = ka->cout, coutp = ka->coutp;
      const int flags = ka->flags;
      float* const dst = ka->dst;
      const float* const res = ka->res;
      float* const pool_dst = ka->pool_dst;
      // per lane: tile (plane, y, x), 8 (or 4) couts; the tile coordinates are recomputed from the lane's tile number here
      // instead of living in three registers across the K loop
      int le = lane;
      FVP_OPAQUE_V(le);
      const int k4 = le >> 4;
      const int le15 = le & 15;
      const int qe = wt * 16 + (SH == 2 ? ((le15 & 1) << 3) | (le15 >> 1) : le15);   // (the K loop's lane-to-tile map)
      const bool q_ok = qe < ka->TN * ka->tpp;
      const int qq = q_ok ? qe : 0;
      const int tn = fdiv_nb(qq, ka->m_tpp), trem = qq - tn * ka->tpp;
      const int ty = fdiv_nb(trem, ka->m_tpr), tx = trem - ty * ka->tpr;
      const bool relu = flags & FVP_EPI_RELU;
      const bool res_after = flags & FVP_EPI_RES_AFTER_RELU;
      const int plane = plane0 + tn, y = y0 + 2 * ty, x = 2 * tx;
      const bool tile_ok = q_ok && plane < ka->planes && y < ka->H;
      const unsigned ppix = unsigned((y >> 1) * (W >> 1) + tx);
      const float* const epi_s = smem + epi_off;
      // Epilogue addressing (round 5): raw descriptors of the unit's first plane (output, residual, pooled output) in SGPRs,
      // ONE per-lane byte offset - cout 4 k4 of the wave's block, the lane's tile; bit 31 (range check: loads return 0,
      // stores are dropped) for masked tiles - and a scalar byte offset per (cout, row): no address arithmetic and no
      // predicate per access (the per-access 64-bit pointer adds were ~15 % of the epilogue's vector instructions).
      // vmcnt is in-order and counts stores: every residual load of the lane is issued before the first store.
      const bool fast = relu && !res_after;            // (every cout of the block exists: the planner takes cout % 32 == 0 only)
      unsigned HW4 = unsigned(HW) * 4u, W4 = unsigned(W) * 4u, HWq4 = unsigned(HW >> 2) * 4u;
      FVP_OPAQUE(HW4);                                 // (the 8-16 scalar row offsets are formed here, per unit: hoisted out
      FVP_OPAQUE(W4);                                  // of the K loop as multiples of the loop-invariant HW they spilled)
      FVP_OPAQUE(HWq4);
      // (one descriptor register set, re-pointed per phase - residual loads, output stores, pooled stores: three sets at
      // once do not fit the SGPR file beside the K loop's state)
      i32x4 rs = {0, 0, 0x7ffffff0, 0x00020000};
      if (HAS_RES) set_base(rs, res + size_t(plane0) * cout * HW);
      const unsigned lco = unsigned(tn * cout + co0 + wc * (16 * CW) + 4 * k4);     // this lane's first cout, as a row of the unit
      const unsigned omask = (kDiag && (ablate & 1024)) ? 0x3ffffu : 0x7fffffffu;   // (bit 1024, diagnostics: epilogue traffic stays inside 1 MB)
      const unsigned voff0 = tile_ok ? ((lco * unsigned(HW) + unsigned(y * W + x)) * 4u) & omask : kWinoOOB;
      const unsigned voffp = tile_ok ? (lco * unsigned(HW >> 2) + ppix) * 4u : kWinoOOB;
      fvp_f32x2 r0[CW][4], r1[CW][4];
      // SKIP: the residual is s = BN(conv1x1(x)), computed below from x instead of read back: the B operands of its MFMAs -
      // x[4 s + k4] at the tile's 2x2 pixels, one 8-byte load per tile row and step - take the place of the residual loads
      // (2 * skip_cin / 4 loads instead of 8 * CW; a masked tile reads zeros).
      fvp_f32x2 xb[kSkip ? SKIP : 1][2];
      if constexpr (kSkip) {
        constexpr int scin = 4 * SKIP;
        set_base(rs, ka->skip_src + size_t(plane0) * scin * HW);
        const unsigned voffx = tile_ok ? unsigned((tn * scin + k4) * HW + y * W + x) * 4u : kWinoOOB;
        unsigned so = 0;
#pragma unroll
        for (int s = 0; s < SKIP; ++s) {
          xb[s][0] = asm_buffer_load_f32x2(voffx, rs, so);
          xb[s][1] = asm_buffer_load_f32x2(voffx, rs, so + W4);
          so += 4u * HW4;
          FVP_OPAQUE(so);
        }
      } else if (HAS_RES && !(kDiag && (ablate & 16))) {      // (bit 16, diagnostics: no residual loads)
        unsigned so = 0;                               // scalar row offset (cb * 16 + r) * HW4, advanced as it is used: formed
#pragma unroll                                         // up front, the 16 offsets of a lane's accesses are 16 more SGPRs
        for (int cb = 0; cb < CW; ++cb) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            r0[cb][r] = asm_buffer_load_f32x2(voff0, rs, so);
            r1[cb][r] = asm_buffer_load_f32x2(voff0, rs, so + W4);
            so += HW4;
            FVP_OPAQUE(so);
          }
          so += 12u * HW4;
        }
      } else {
#pragma unroll
        for (int cb = 0; cb < CW; ++cb)
#pragma unroll
          for (int r = 0; r < 4; ++r) r0[cb][r] = r1[cb][r] = fvp_f32x2{0.f, 0.f};
      }
      // output transform A^T M A of the 8 couts while the residual loads are in flight (the accumulators die here)
      float o[CW][4][2][2];
#pragma unroll
      for (int cb = 0; cb < CW; ++cb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float s[4][2];
#pragma unroll
          for (int xi = 0; xi < 4; ++xi) {
            const float m0 = acc[cb][4 * xi][r], m1 = acc[cb][4 * xi + 1][r], m2 = acc[cb][4 * xi + 2][r],
                        m3 = acc[cb][4 * xi + 3][r];
            s[xi][0] = (m0 + m1) + m2;
            s[xi][1] = (m1 - m2) - m3;
          }
#pragma unroll
          for (int e = 0; e < 2; ++e) {
            o[cb][r][0][e] = (s[0][e] + s[1][e]) + s[2][e];
            o[cb][r][1][e] = (s[1][e] - s[2][e]) - s[3][e];
          }
        }
      // ONE wait for all residual loads.  The stores below are conditional (masked tiles), so behind the first of them the
      // compiler's counter no longer knows how many younger operations are in the queue and every later use of a loaded
      // value would get a full vmcnt(0) - i.e. wait for the stores issued so far.
      // The same wait (taken by the kernels without a residual too) is what makes "stores stay in flight" safe BY
      // CONSTRUCTION: the only DMA chunk still in the in-order vmcnt queue here is the one requested at the top of this
      // unit's last chunk - the chunk the NEXT unit's first barrier has to see landed.  After vmcnt(0) it has landed, so
      // that barrier needs no vmcnt wait at all, whatever the number of store instructions hipcc emits below.
      __builtin_amdgcn_sched_barrier(0);
      wait_vmcnt_imm<0>();
      __builtin_amdgcn_sched_barrier(0);
      // SKIP: s[cout][pixel] = sum_ci Wskip[cout][ci] x[ci][pixel] as 16x16x4 MFMAs in the D layout of the accumulators (lane:
      // tile l15, couts 4 k4 + r of the block), channels ascending from the constant-zero C - the fmaf chain k_conv_reg runs
      // for the stand-alone skip, the same bits - then the skip's own BN.  One cout block at a time (four independent chains of
      // skip_cin / 4 MFMAs, one per pixel of the tile): 16 result registers in flight, not 16 CW.
      // The step count is the template parameter SKIP (4: 16 channels, 8: 32): with a run-time count the guarded steps cost
      // 16 SGPRs of conditions and 21-46 spilled VGPRs in every two-block instance.
      float sk[kSkip ? CW : 1][4][2][2];
      if constexpr (kSkip) {
        const float* const sk_s = smem + ka->skip_off;
        constexpr int sg = SKIP / 4;
        const f32x4 z = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int cb = 0; cb < CW; ++cb) {
          const int cob = co0 + wc * (16 * CW) + cb * 16;
          const float* const wrow = sk_s + 3 * coutp + ((cob + le15) * 4 + k4) * sg * 4;
          f32x4 aw[kSkip ? sg : 1];
#pragma unroll
          for (int g = 0; g < sg; ++g) aw[g] = *reinterpret_cast<const f32x4*>(wrow + 4 * g);
          f32x4 dd[2][2];
#pragma unroll
          for (int s = 0; s < SKIP; ++s)
#pragma unroll
            for (int i = 0; i < 2; ++i) {
              dd[i][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(aw[s >> 2][s & 3], xb[s][i].x, s == 0 ? z : dd[i][0], 0, 0, 0);
              dd[i][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(aw[s >> 2][s & 3], xb[s][i].y, s == 0 ? z : dd[i][1], 0, 0, 0);
            }
          f32x4 bn[3];
#pragma unroll
          for (int i = 0; i < 3; ++i) bn[i] = *reinterpret_cast<const f32x4*>(sk_s + i * coutp + cob + 4 * k4);
#pragma unroll
          for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
              for (int e = 0; e < 2; ++e) sk[cb][r][i][e] = bn_affine(dd[i][e][r], bn[0][r], bn[1][r], bn[2][r]);
        }
      }
      // every P2PNet / CenterNet layer on this kernel is BN (+ residual) -> ReLU: that order gets its own copy of the loop (as
      // run-time flags the two selects per value were a quarter of the epilogue's instructions)
      auto finalize = [&](auto fastc) {
        // kFast: BN (+ residual) -> ReLU, the order of every P2PNet / CenterNet layer on this kernel
        constexpr bool kFast = decltype(fastc)::value;
        set_base(rs, dst + size_t(plane0) * cout * HW);
        float pm[CW][4];                             // fused max_pool(2,2): this lane's tile is one pooled pixel
        unsigned sso = 0;
#pragma unroll
        for (int cb = 0; cb < CW; ++cb) {
          const int co4 = co0 + wc * (16 * CW) + cb * 16 + 4 * k4;
          f32x4 bn[3];
#pragma unroll
          for (int i = 0; i < 3; ++i) bn[i] = *reinterpret_cast<const f32x4*>(epi_s + i * coutp + co4);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float b = bn[0][r], sc = bn[1][r], sh = bn[2][r];
            float rr[2][2];                          // the residual: loaded, or the fused skip's result
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
              for (int e = 0; e < 2; ++e) {
                if constexpr (kSkip) rr[i][e] = sk[cb][r][i][e];
                else rr[i][e] = i ? r1[cb][r][e] : r0[cb][r][e];
              }
            float vv[2][2];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
              for (int e = 0; e < 2; ++e) {
                float xv = bn_affine(o[cb][r][i][e], b, sc, sh);
                if (HAS_RES && (kFast || !res_after)) xv += rr[i][e];
                if (kFast || relu) xv = fmaxf(xv, 0.0f);
                if (HAS_RES && !kFast && res_after) xv += rr[i][e];
                vv[i][e] = xv;
              }
            pm[cb][r] = fmaxf(fmaxf(vv[0][0], vv[0][1]), fmaxf(vv[1][0], vv[1][1]));
            if (kDiag && (ablate & 32) && vv[0][0] != 1.2345e-30f) { sso += HW4; continue; }   // (bit 32, diagnostics: no stores)
            asm_buffer_store_f32x2(fvp_f32x2{vv[0][0], vv[0][1]}, voff0, rs, sso);
            asm_buffer_store_f32x2(fvp_f32x2{vv[1][0], vv[1][1]}, voff0, rs, sso + W4);
            sso += HW4;
            FVP_OPAQUE(sso);
          }
          sso += 12u * HW4;
        }
        if (pool_dst && !(kDiag && (ablate & 32))) {
          set_base(rs, pool_dst + size_t(plane0) * cout * (HW >> 2));
#pragma unroll
          for (int cb = 0; cb < CW; ++cb)
#pragma unroll
            for (int r = 0; r < 4; ++r)
              asm_buffer_store_f32(pm[cb][r], voffp, rs, unsigned(cb * 16 + r) * HWq4);
        }
      };
      if (fast) finalize(std::integral_constant<bool, true>{});
      else finalize(std::integral_constant<bool, false>{});
    } else {
      wait_vmcnt_imm<0>();                           // (diagnostics, no epilogue: the ring invariant still needs the drain)
    }
    u = next_unit(u + G, LdsFlags{});
    if (u >= nunits) break;
    fetch_a(0, wchunk(slot_ptr(cur), 0), 0);
    fetch_d(slot_ptr(cur), 0, WP);
  }
