// Body of attn_bwd_dq_kernel / attn_bwd_dq_doc_kernel (attention.hip), included inside both (see
// attention_fwd_body.h).  Expects D, OCC, BN, RING, PK, RANGE, DOC, GQA, WIN and the argument `a`.
  static_assert(!(RANGE && DOC), "a key range and document spans are exclusive");
  constexpr bool RNG = RANGE || DOC || WIN;
  constexpr bool SWZ = D == 64;                 // swizzled unpadded K / V images (swz64_off)
  constexpr int KP = SWZ ? D : D + 8, NC = D / 16, NDB = D / 32;
  __shared__ __attribute__((aligned(16))) bf16 Ks[2][BN * KP];
  __shared__ __attribute__((aligned(16))) bf16 Vs[2][BN * KP];

  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), hh = lane >> 5,
            r = lane & 31;
  int tx, ty;
  xcd_tile(tx, ty);
  const int bh = ty, b = bh / a.H, h = bh % a.H;
  const int S = a.S;
  const int qblk = tx * 128, q0 = qblk + w * 32;
  const int q = q0 + r;
  const bool qvalid = q < S;
  int hk = h;   // GQA: the key/value head h / G (a.hkv(), see FwdArgs)
  if constexpr (GQA) hk = __builtin_amdgcn_readfirstlane(h / (a.H / a.hkv()));
  const float sl2 = a.slopes ? a.slopes[h] * kLog2e : 0.f;
  const float sc2 = a.scale * kLog2e;
  const bool drop = a.maskA != nullptr;
  const float inv_keep = drop ? 1.f / (1.f - a.p) : 1.f;
  const RowSrc ksrc = row_src<D>(a.k + (size_t)b * S * a.ld + hk * D, a.ld, S);
  const RowSrc vsrc = row_src<D>(a.v + (size_t)b * S * a.ld + hk * D, a.ld, S);
  // keep masks as in attn_fwd_kernel: 64-bit lane masks of the key-major layout, scalar loads
  const int Sp = 32 * a.W;
  const uint32_t* mrow = drop ? a.maskB + ((size_t)bh * a.W + min(q0 >> 5, a.W - 1)) * Sp : nullptr;
  const __amdgpu_buffer_rsrc_t mrs = bounded_rsrc(drop ? (const void*)mrow : (const void*)a.lse, drop ? (uint32_t)Sp * 4u : 0u);

  f32x16 dq[NDB];
#pragma unroll
  for (int d = 0; d < NDB; ++d) dq[d] = f32x16{};

  // key range, first tile and look-ahead clamp as in attn_fwd_kernel
  int klo = 0, khi = S;
  if constexpr (RANGE) load_range(a.kv_range, b, S, klo, khi);
  SpanOf<DOC> doc{};
  if constexpr (DOC) {
    load_block_range(a.doc(), a.B, b, gridDim.x, tx, S, klo, khi);
    doc = load_span(a.doc(), b, S, q);
  }
  int win = 0;   // WIN: the sliding window, folded into the tile range and the span as in attn_fwd_kernel
  if constexpr (WIN) {
    win = __builtin_amdgcn_readfirstlane(a.window());
    klo = max(klo, qblk - win + 1);
    if constexpr (DOC) doc.clip_lo(q - win + 1);
  }
  const int kend = a.causal ? min(khi, qblk + 128) : khi;
  const int nt = (kend + BN - 1) / BN;
  const int t0 = RNG ? klo / BN : 0;
  const int last = RNG ? max(nt - 1, t0) : nt - 1;
  // K/V tiles + dropout keep words through a 2-deep register ring (see attn_fwd_kernel)
  constexpr int NKB = BN / 32;
  // RING = 1: one register set in flight (fewer VGPRs -> 3 waves per SIMD), see attn_fwd_kernel
  TileLoader<D, BN> kl0, vl0, kl1r, vl1r;
  TileLoader<D, BN>& kl1 = RING == 2 ? kl1r : kl0;
  TileLoader<D, BN>& vl1 = RING == 2 ? vl1r : vl0;
  uint32_t pf0 = 0, pf1r = 0;   // L2 prefetch of keep words (value unused)
  uint32_t& pf1 = RING == 2 ? pf1r : pf0;
  auto prefetch_words = [&](int k0, uint32_t& out) {
    asm volatile("" :: "v"(out));
    out = __builtin_amdgcn_raw_buffer_load_b32(mrs, lane * 4, k0 * 4, 0);
  };
  // Prologue: one memory round trip.  Every load -- K/V tiles t0 and t0 + 1, then this lane's Q,
  // dO and O fragments and its lse, all branch-free -- is issued before anything waits; tile t0
  // goes to LDS as soon as it lands (it was issued first: a partial vmcnt) and delta is formed
  // while the rest arrives.  With RING = 1 tile t0 has a register set of its own, which only
  // lives here: the accumulators are not live yet, so the prologue stays below the loop's
  // register peak.
  bf16x8 qf[NC], of[NC];
  float lse2, dl;
  {
    TileLoader<D, BN> kpr, vpr;
    TileLoader<D, BN>& kp = RING == 2 ? kl0 : kpr;
    TileLoader<D, BN>& vp = RING == 2 ? vl0 : vpr;
    const int k1 = min(t0 + 1, last) * BN, k2 = min(t0 + 2, last) * BN;
    kp.load(ksrc, t0 * BN);
    vp.load(vsrc, t0 * BN);
    kl1.load(ksrc, k1); vl1.load(vsrc, k1); prefetch_words(k1, pf1);
    bf16x8 ov[NC];
    load_frags<D>(qf, a.q + (size_t)b * S * a.ld + h * D, a.ld, S, q, hh);       // rows past S: 0
    load_frags<D>(of, a.dout + (size_t)b * S * a.ldo + h * D, a.ldo, S, q, hh);
    load_frags<D>(ov, a.o + (size_t)b * S * a.ldo + h * D, a.ldo, S, q, hh);
    lse2 = load_stat(bounded_rsrc(a.lse + (size_t)bh * S, (uint32_t)S * 4u), q * 4) * kLog2e;
    // a row without a key: every key it meets is masked below (P = 0 by select); +inf here also
    // makes the unmasked exponent 2^(s - inf) = 0 instead of 2^(s + inf)
    if constexpr (RNG) lse2 = lse2 == -INFINITY ? INFINITY : lse2;
    asm volatile("" ::: "memory");   // keeps every load above issued ahead of the first wait
    kp.store_bwd(Ks[0], KP);
    vp.store_bwd(Vs[0], KP);
    if constexpr (RING == 2) { kl0.load(ksrc, k2); vl0.load(vsrc, k2); prefetch_words(k2, pf0); }
    // delta = rowsum(dO * O) of this lane's query, from the dO fragments already in registers and
    // one O row read (no separate delta pass re-reading dO); stored for the dK/dV kernel, which
    // runs after this one
    float part = 0.f;
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
      for (int j = 0; j < 8; ++j) part = fmaf((float)ov[c][j], (float)of[c][j], part);
    dl = xhalf_sum(part);
    if (qvalid && hh == 0) a.delta[(size_t)bh * S + q] = dl;
  }
  __syncthreads();
  auto tile = [&](auto set_c, int t) {
    constexpr int SET = decltype(set_c)::value;
    TileLoader<D, BN>& kn = SET ? kl1 : kl0;
    TileLoader<D, BN>& vn = SET ? vl1 : vl0;
    uint32_t& pfn = SET ? pf1 : pf0;
    const int buf = (t - t0) & 1, k0 = t * BN;
    const bf16* K = Ks[buf];
    const bf16* V = Vs[buf];
    bool needmask = !qvalid || (k0 + BN > khi) || (RANGE && k0 < klo) || (a.causal && k0 + BN - 1 > q0);
    if constexpr (WIN && !DOC) needmask = needmask || k0 + win <= q0 + 31;
    // (DOC: a wave-uniform vote; a row past S has an empty span)
    if constexpr (DOC) needmask = !__all(doc.covers(k0, BN)) || (a.causal && k0 + BN - 1 > q0);
#pragma unroll
    for (int kb = 0; kb < BN / 32; ++kb) {
      f32x16 sacc = f32x16{}, pacc = f32x16{};
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        if constexpr (SWZ) {
          sacc = mfma32(swz_row_read(K, kb * 32, r, 2 * c + hh), qf[c], sacc);
          pacc = mfma32(swz_row_read(V, kb * 32, r, 2 * c + hh), of[c], pacc);
        } else {
          sacc = mfma32(*reinterpret_cast<const bf16x8*>(&K[(kb * 32 + r) * KP + 16 * c + 8 * hh]), qf[c], sacc);
          pacc = mfma32(*reinterpret_cast<const bf16x8*>(&V[(kb * 32 + r) * KP + 16 * c + 8 * hh]), of[c], pacc);
        }
      }
      // this block's keep masks (after the S / dP MFMAs consumed their LDS operands)
      uint64_t mk[16];
      if (drop) {
        const cu64* mp = (const cu64*)(uintptr_t)(mrow + keep_off(k0 + kb * 32, Sp));
#pragma unroll
        for (int i = 0; i < 16; ++i) mk[i] = mp[i];
      }
      // P = exp2(s*log2e - lse): 2 VALU on interior tiles without ALiBi
      if (needmask || sl2 != 0.f) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int key = k0 + kb * 32 + crow(i, hh);
          float pv = fexp2(fmaf(sacc[i], sc2, sl2 * (float)key - lse2));
          if constexpr (DOC) {
            if (needmask && (!doc.has(key) || (a.causal && key > q))) pv = 0.f;
          } else {
            if (needmask && (!qvalid || key >= khi || (RANGE && key < klo) || (a.causal && key > q) || (WIN && key + win <= q))) pv = 0.f;
          }
          sacc[i] = pv;
        }
      } else if constexpr (PK) {
        const f32x2 sc22 = pk2(sc2, sc2), nl2 = pk2(-lse2, -lse2);
#pragma unroll
        for (int i = 0; i < 16; i += 2) {
          const f32x2 x = pk_fma(pk2(sacc[i], sacc[i + 1]), sc22, nl2);
          sacc[i] = fexp2(x.x);
          sacc[i + 1] = fexp2(x.y);
        }
      } else {
#pragma unroll
        for (int i = 0; i < 16; ++i) sacc[i] = fexp2(fmaf(sacc[i], sc2, -lse2));
      }
      // dS^T = P * (dP - delta), dP = dropout(dP') (keep bit, 1/(1-p))
      if constexpr (PK) {
        const f32x2 ik2 = pk2(drop ? inv_keep : 1.f, drop ? inv_keep : 1.f), nd2 = pk2(-dl, -dl);
#pragma unroll
        for (int i = 0; i < 16; i += 2) {
          f32x2 dp = pk2(pacc[i], pacc[i + 1]);
          if (drop) dp = pk2(sel_keep(pacc[i], mk[i]), sel_keep(pacc[i + 1], mk[i + 1]));
          const f32x2 ds = pk2(sacc[i], sacc[i + 1]) * pk_fma(dp, ik2, nd2);
          sacc[i] = ds.x;
          sacc[i + 1] = ds.y;
        }
      } else if (drop) {
#pragma unroll
        for (int i = 0; i < 16; ++i) sacc[i] *= fmaf(sel_keep(pacc[i], mk[i]), inv_keep, -dl);
      } else {
#pragma unroll
        for (int i = 0; i < 16; ++i) sacc[i] *= pacc[i] - dl;
      }
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        bf16x8 sb;
#pragma unroll
        for (int j = 0; j < 8; ++j) sb[j] = (bf16)sacc[8 * s + j];
#pragma unroll
        for (int d = 0; d < NDB; ++d) {
          if constexpr (SWZ) dq[d] = mfma32(tr_operand_swz(K, kb * 32 + 16 * s, d * 32, lane), sb, dq[d]);
          else dq[d] = mfma32(tr_operand(K, KP, kb * 32 + 16 * s, d * 32, lane), sb, dq[d]);
        }
      }
    }
    if (t + 1 < nt) {
      kn.store_bwd(Ks[buf ^ 1], KP);
      vn.store_bwd(Vs[buf ^ 1], KP);
      // tile t+1+RING (clamped to the last tile: a harmless reload keeps the issue unconditional)
      const int kf = min(t + 1 + RING, nt - 1) * BN;
      kn.load(ksrc, kf);
      vn.load(vsrc, kf);
      prefetch_words(kf, pfn);
    }
    __syncthreads();
  };
  for (int t = t0; t < nt; t += 2) {
    tile(std::integral_constant<int, 1>{}, t);
    if (t + 1 < nt) tile(std::integral_constant<int, 0>{}, t + 1);
  }
  if (!GQA && a.bias_part && D == 64) {
    float vq[32];
#pragma unroll
    for (int d = 0; d < NDB; ++d)
#pragma unroll
      for (int i = 0; i < 16; ++i) vq[16 * d + i] = qvalid ? (float)(bf16)(dq[d][i] * a.scale) : 0.f;
    const float sq = colsum32(vq, r);
    a.bias_part[((size_t)b * gridDim.x * 4 + (qblk >> 5) + w) * (3 * a.H * D) + h * D + colsum_col(r, hh)] = sq;
  }
  store_rows16<NDB>(a.dq + (size_t)(b * S + q) * a.ld + h * D, dq, a.scale, hh, qvalid);
