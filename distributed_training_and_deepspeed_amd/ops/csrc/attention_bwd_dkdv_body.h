// Body of attn_bwd_dkdv_kernel / attn_bwd_dkdv_doc_kernel (attention.hip), included inside both (see
// attention_fwd_body.h).  Expects D, OCC, BM, DROP, ALIBI, MASK, RANGE, DOC, GQA, WIN and the argument `a`.
  static_assert(MASK || !(RANGE || DOC), "a key range needs the masked form");
  static_assert(!(RANGE && DOC), "a key range and document spans are exclusive");
  constexpr bool SWZ = D == 64;                 // swizzled unpadded image (swz64_off)
  constexpr int QP = SWZ ? D : D + 8, NC = D / 16, NDB = D / 32;
  // One LDS block, row statistics first: placed after the 72 KiB of Q/dO tiles (BM = 128) their
  // ds_read offsets exceed the 16-bit immediate and every read needed a VALU address add.
  struct Smem {
    float lse_s[2][BM], del_s[2][BM];
    bf16 Qs[2][BM * QP];
    bf16 Os[2][BM * QP];
  };
  __shared__ __attribute__((aligned(16))) Smem sm;
  auto& lse_s = sm.lse_s;
  auto& del_s = sm.del_s;
  auto& Qs = sm.Qs;
  auto& Os = sm.Os;

  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), hh = lane >> 5,
            r = lane & 31;
  int tx, ty;
  if constexpr (RANGE || DOC) xcd_tile_grouped(tx, ty);
  else xcd_tile(tx, ty);
  // GQA: grid y = B * Hkv (Hkv = a.hkv(), see FwdArgs).  The workgroup
  // owns key/value head hk of sequence b and walks the query tiles of its G = H / Hkv query heads
  // hk * G .. hk * G + G - 1 in turn; `h` / `bh` name the query head whose tile is being fetched.
  int bh = ty, b = bh / a.H, h = bh % a.H, hk = h, G = 1;
  if constexpr (GQA) {
    b = ty / a.hkv();
    hk = ty % a.hkv();
    G = a.H / a.hkv();
    h = hk * G;
    bh = b * a.H + h;
  }
  const int S = a.S;
  const int kblk = tx * 128;
  const int key = kblk + w * 32 + r;
  const bool kvalid = key < S;
  int klo = 0, khi = S;
  // DOC: (klo, khi) are the block's document bounds = the queries that may see one of its keys
  if constexpr (DOC) load_block_range(a.doc(), a.B, b, gridDim.x, tx, S, klo, khi);
  if constexpr (RANGE || DOC) {
    if constexpr (RANGE) load_range(a.kv_range, b, S, klo, khi);
    // block-uniform: no key of this block is in the range (DOC: every key of it is a pad)
    if (DOC ? klo >= khi : (kblk >= khi || kblk + 128 <= klo)) {
      if (!GQA && a.bias_part && D == 64) {
        float* row = a.bias_part + ((size_t)b * gridDim.x * 4 + (kblk >> 5) + w) * (3 * a.H * D) + h * D + colsum_col(r, hh);
        row[a.H * D] = 0.f;
        row[2 * a.H * D] = 0.f;
      }
      if (kvalid) {
        bf16* dkp = a.dk + (size_t)(b * S + key) * a.ld + hk * D;
        bf16* dvp = a.dv + (size_t)(b * S + key) * a.ld + hk * D;
#pragma unroll
        for (int c = 0; c < D / 16; ++c) {   // both half-waves hold lane r's key: 8 of 16 columns each
          *reinterpret_cast<bf16x8*>(dkp + 16 * c + 8 * hh) = bf16x8{};
          *reinterpret_cast<bf16x8*>(dvp + 16 * c + 8 * hh) = bf16x8{};
        }
      }
      return;
    }
  }
  const bool kin = key >= klo && key < khi;     // this lane's key takes part (RANGE)
  SpanOf<DOC> doc{};                            // this lane's key's document = its valid queries (DOC)
  if constexpr (DOC) doc = load_span(a.doc(), b, S, key);
  // WIN: key j is seen by the queries j <= q < j + win (a.window(), see FwdArgs); a span takes that end in
  int win = 0;
  if constexpr (WIN) {
    win = __builtin_amdgcn_readfirstlane(a.window());
    if constexpr (DOC) doc.clip_hi(key + win);
  }
  const float sl2 = a.slopes ? a.slopes[h] * kLog2e : 0.f;
  const float sc2 = a.scale * kLog2e;
  constexpr bool drop = DROP;
  const float inv_keep = drop ? 1.f / (1.f - a.p) : 1.f;
  const float kbias = sl2 * (float)key;   // ALiBi bias of this lane's key (0 without ALiBi)
  // keep masks: this wave's 32 keys are one key word of the query-major layout A, so a 32-query
  // block's masks are 16 aligned 64-bit words (lm_pos) -- scalar loads, one v_cndmask per use
  const int Sp = 32 * a.W;
  const uint32_t* mrow = drop ? a.maskA + ((size_t)bh * a.W + min((kblk >> 5) + w, a.W - 1)) * Sp : nullptr;
  const __amdgpu_buffer_rsrc_t mrs = bounded_rsrc(drop ? (const void*)mrow : (const void*)a.lse, drop ? (uint32_t)Sp * 4u : 0u);
  RowSrc qsrc = row_src<D>(a.q + (size_t)b * S * a.ld + h * D, a.ld, S);
  RowSrc osrc = row_src<D>(a.dout + (size_t)b * S * a.ldo + h * D, a.ldo, S);
  // row statistics of one (batch, head): bounded resources over the [S] rows, so rows past S read 0
  __amdgpu_buffer_rsrc_t lse_rs = bounded_rsrc(a.lse + (size_t)bh * S, (uint32_t)S * 4u);
  __amdgpu_buffer_rsrc_t del_rs = bounded_rsrc(a.delta + (size_t)bh * S, (uint32_t)S * 4u);

  bf16x8 kf[NC], vf[NC];
  load_frags<D>(kf, a.k + (size_t)b * S * a.ld + hk * D, a.ld, S, key, hh);   // keys past S: 0
  load_frags<D>(vf, a.v + (size_t)b * S * a.ld + hk * D, a.ld, S, key, hh);
  f32x16 dk[NDB], dv[NDB];
#pragma unroll
  for (int d = 0; d < NDB; ++d) { dk[d] = f32x16{}; dv[d] = f32x16{}; }

  int qstart = a.causal ? (kblk / BM) * BM : 0, qend = S;
  if constexpr (DOC) {   // the query tiles holding [klo, khi), from the causal start on
    qstart = (max(qstart, klo) / BM) * BM;
    qend = khi;
  }
  if constexpr (WIN) qend = min(qend, kblk + 127 + win);   // the block's last key's last query, + 1
  const int nt = (qend - qstart + BM - 1) / BM;
  TileLoader<D, BM> ql, ol;
  // Raw lse / delta of a query tile, one row per thread of the first BM, issued straight behind the
  // tile's Q / dO loads with no arithmetic on them: vmcnt retires in order, so a consumer placed
  // here would drain the whole prefetch it was just issued behind (a full memory round trip at the
  // head of every tile).  The values are transformed where they go to LDS (store_stats), after the
  // tile's compute.  Threads past BM get an offset beyond any row: 0, without touching memory.
  float lse_r = 0.f, del_r = 0.f;
  const int stat_off = threadIdx.x < BM ? (int)threadIdx.x * 4 : 0x40000000;
  auto load_stats = [&](int q0) {
    lse_r = load_stat(lse_rs, q0 * 4 + stat_off);
    del_r = load_stat(del_rs, q0 * 4 + stat_off);
  };
  auto store_stats = [&](int buf, int q0) {
    if (threadIdx.x < BM) {
      const bool in = q0 + (int)threadIdx.x < S;
      float nl = in ? -lse_r * kLog2e : 0.f;       // stored negated: P = 2^fma(s, sc2, -lse)
      // a row without a key (lse = -inf): P = 2^(s - inf) = 0, not 2^(s + inf)
      if constexpr (RANGE || DOC) nl = nl == INFINITY ? -INFINITY : nl;
      lse_s[buf][threadIdx.x] = nl;
      // dS = P (dP - delta); with dropout the kernel forms dS' = (1 - p) dS = Pm dP - P (1 - p) delta
      // (Pm = P * keep), so delta is stored pre-scaled and dK takes the 1 / (1 - p) at the end
      del_s[buf][threadIdx.x] = in ? -del_r * (DROP ? 1.f - a.p : 1.f) : 0.f;
    }
  };
  // L2 prefetch of the next query tile's keep words (BM words, value unused)
  constexpr int NPF = BM / 64;
  uint32_t pfw[NPF] = {};
  auto prefetch_words = [&](int q0) {
#pragma unroll
    for (int j = 0; j < NPF; ++j) {
      asm volatile("" :: "v"(pfw[j]));
      pfw[j] = __builtin_amdgcn_raw_buffer_load_b32(mrs, (lane + 64 * j) * 4, q0 * 4, 0);
    }
  };
  ql.load(qsrc, qstart);
  ol.load(osrc, qstart);
  load_stats(qstart);
  ql.store_bwd(Qs[0], QP);
  ol.store_bwd(Os[0], QP);
  store_stats(0, qstart);
  __syncthreads();
  // GQA: the G heads' tile sequences run as one, nt tiles each, into the same accumulators.  The
  // sources are only read by the prefetch, so they are rebased (scalar registers) where the
  // prefetch crosses a head seam: the last tile of a head fetches the next head's first tile, and
  // the double buffer never drains.  tq = the tile being fetched, inside its head.
  const int ntot = GQA ? nt * G : nt;
  int tq = 0, qseam = 0;   // (GQA only) qseam: the tile fetched is the first of the next head
  for (int t = 0; t < ntot; ++t) {
    const int buf = t & 1, q0 = qstart + (GQA ? tq : t) * BM;
    if (t + 1 < ntot) {
      if constexpr (GQA) {
        qseam = 0;
        if (++tq == nt) {
          tq = 0;
          qseam = 1;
          ++h;
          bh = b * a.H + h;
          qsrc.rs = row_src<D>(a.q + (size_t)b * S * a.ld + h * D, a.ld, S).rs;   // (voff, ld2 stay)
          osrc.rs = row_src<D>(a.dout + (size_t)b * S * a.ldo + h * D, a.ldo, S).rs;
          lse_rs = bounded_rsrc(a.lse + (size_t)bh * S, (uint32_t)S * 4u);
          del_rs = bounded_rsrc(a.delta + (size_t)bh * S, (uint32_t)S * 4u);
        }
      }
      ql.load(qsrc, GQA && qseam ? qstart : q0 + BM);
      ol.load(osrc, GQA && qseam ? qstart : q0 + BM);
      load_stats(GQA && qseam ? qstart : q0 + BM);
      if (drop) prefetch_words(q0 + BM);
    }
    const bf16* Q = Qs[buf];
    const bf16* O = Os[buf];
    // one wave per SIMD (OCC 1, 512 registers): unroll the query sub-blocks so the S/dP MFMAs
    // of sub-block qb+1 can be scheduled under the softmax VALU of qb; at OCC 2 the register
    // budget keeps the sub-blocks serial
    constexpr int kQbUnroll = OCC == 1 ? BM / 32 : 1;
#pragma unroll kQbUnroll
    for (int qb = 0; qb < BM / 32; ++qb) {
      f32x16 sacc = f32x16{}, pacc = f32x16{};
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        if constexpr (SWZ) {
          sacc = mfma32(swz_row_read(Q, qb * 32, r, 2 * c + hh), kf[c], sacc);
          pacc = mfma32(swz_row_read(O, qb * 32, r, 2 * c + hh), vf[c], pacc);
        } else {
          sacc = mfma32(*reinterpret_cast<const bf16x8*>(&Q[(qb * 32 + r) * QP + 16 * c + 8 * hh]), kf[c], sacc);
          pacc = mfma32(*reinterpret_cast<const bf16x8*>(&O[(qb * 32 + r) * QP + 16 * c + 8 * hh]), vf[c], pacc);
        }
      }
      const int qrow0 = q0 + qb * 32;
      // block-uniform predicate (a scalar branch, never a per-element one)
      bool needmask = MASK && ((kblk + 128 > S) || (qrow0 + 32 > S) || (a.causal && kblk + 127 > qrow0));
      if constexpr (RANGE) needmask = needmask || kblk + 128 > khi || kblk < klo;   // the blocks holding lo / hi
      if constexpr (WIN && !DOC) needmask = needmask || qrow0 + 31 - kblk >= win;   // the sub-block's last query is past the block's first key's window
      // (DOC: some key's span -- a pad's is empty -- leaves out some of the 32 queries; wave-uniform)
      if constexpr (DOC) needmask = !__all(doc.covers(qrow0, 32)) || (a.causal && kblk + 127 > qrow0);
      // this query block's keep masks (after the S / dP MFMAs consumed their LDS operands)
      uint64_t mk[16];
      if constexpr (DROP) {
        const cu64* mp = (const cu64*)(uintptr_t)(mrow + keep_off(qrow0, Sp));
#pragma unroll
        for (int i = 0; i < 16; ++i) mk[i] = mp[i];
      }
      // row statistics of this lane's 16 accumulator rows (rows 8g + 4hh + 0..3 are contiguous):
      // 8 ds_read_b128 issued together instead of 32 dependent scalar LDS reads
      f32x4 L4[4], D4[4];
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        L4[g] = *reinterpret_cast<const f32x4*>(&lse_s[buf][qb * 32 + 8 * g + 4 * hh]);
        D4[g] = *reinterpret_cast<const f32x4*>(&del_s[buf][qb * 32 + 8 * g + 4 * hh]);
      }
      // P = 2^(s sc2 + kbias - lse): score pairs (i, i+1) share a row group, so the row terms pair up
      const f32x2 sc2v = pk2(sc2, sc2), kb2 = pk2(kbias, kbias);
#pragma unroll
      for (int i = 0; i < 16; i += 2) {
        f32x2 nl = pk2(L4[i >> 2][i & 3], L4[i >> 2][(i & 3) + 1]);
        if constexpr (ALIBI) nl += kb2;
        const f32x2 x = pk_fma(pk2(sacc[i], sacc[i + 1]), sc2v, nl);
        sacc[i] = fexp2(x.x);
        sacc[i + 1] = fexp2(x.y);
      }
      if (MASK && needmask) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int qq = qrow0 + crow(i, hh);
          bool ok = kvalid && qq < S && !(a.causal && key > qq);
          if constexpr (RANGE) ok = ok && kin;
          if constexpr (WIN) ok = ok && qq < key + win;
          if constexpr (DOC) ok = doc.has(qq) && !(a.causal && key > qq);   // (the span lies inside [0, S))
          sacc[i] = ok ? sacc[i] : 0.f;
        }
      }
#pragma unroll
      for (int i = 0; i < 16; i += 2) {
        const f32x2 nd = pk2(D4[i >> 2][i & 3], D4[i >> 2][(i & 3) + 1]);
        if constexpr (DROP) {
          // 2 VALU issues per score instead of 3: one keep select (Pm feeds both dV and dS')
          const f32x2 pm = pk2(sel_keep(sacc[i], mk[i]), sel_keep(sacc[i + 1], mk[i + 1]));
          const f32x2 u = pk2(sacc[i], sacc[i + 1]) * nd;                 // -P (1 - p) delta
          const f32x2 ds = pk_fma(pm, pk2(pacc[i], pacc[i + 1]), u);      // dS' = (1 - p) dS
          pacc[i] = ds.x;
          pacc[i + 1] = ds.y;
          sacc[i] = pm.x;                                                 // P*mask (dV)
          sacc[i + 1] = pm.y;
        } else {
          const f32x2 ds = pk2(sacc[i], sacc[i + 1]) * (pk2(pacc[i], pacc[i + 1]) + nd);
          pacc[i] = ds.x;
          pacc[i + 1] = ds.y;
        }
      }
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        bf16x8 pb, sb;
#pragma unroll
        for (int j = 0; j < 8; ++j) { pb[j] = (bf16)sacc[8 * s + j]; sb[j] = (bf16)pacc[8 * s + j]; }
#pragma unroll
        for (int d = 0; d < NDB; ++d) {
          if constexpr (SWZ) {
            dv[d] = mfma32(tr_operand_swz(O, qb * 32 + 16 * s, d * 32, lane), pb, dv[d]);
            dk[d] = mfma32(tr_operand_swz(Q, qb * 32 + 16 * s, d * 32, lane), sb, dk[d]);
          } else {
            dv[d] = mfma32(tr_operand(O, QP, qb * 32 + 16 * s, d * 32, lane), pb, dv[d]);
            dk[d] = mfma32(tr_operand(Q, QP, qb * 32 + 16 * s, d * 32, lane), sb, dk[d]);
          }
        }
      }
    }
    if (t + 1 < ntot) {
      ql.store_bwd(Qs[buf ^ 1], QP);
      ol.store_bwd(Os[buf ^ 1], QP);
      store_stats(buf ^ 1, GQA && qseam ? qstart : q0 + BM);
    }
    __syncthreads();
  }
  const float dv_scale = inv_keep;   // the dropped P fed to dV carried keep bits only
  const float dk_scale = a.scale * inv_keep;   // dS' = (1 - p) dS (see load_stats)
  if (!GQA && a.bias_part && D == 64) {
    float vk[32], vv[32];
#pragma unroll
    for (int d = 0; d < NDB; ++d)
#pragma unroll
      for (int i = 0; i < 16; ++i) {   // the stored (bf16-rounded) values, 0 past S
        vk[16 * d + i] = kvalid ? (float)(bf16)(dk[d][i] * dk_scale) : 0.f;
        vv[16 * d + i] = kvalid ? (float)(bf16)(dv[d][i] * dv_scale) : 0.f;
      }
    const float sk = colsum32(vk, r), sv = colsum32(vv, r);
    float* row = a.bias_part + ((size_t)b * gridDim.x * 4 + (kblk >> 5) + w) * (3 * a.H * D) + h * D + colsum_col(r, hh);
    row[a.H * D] = sk;
    row[2 * a.H * D] = sv;
  }
  store_rows16<NDB>(a.dk + (size_t)(b * S + key) * a.ld + hk * D, dk, dk_scale, hh, kvalid);
  store_rows16<NDB>(a.dv + (size_t)(b * S + key) * a.ld + hk * D, dv, dv_scale, hh, kvalid);
