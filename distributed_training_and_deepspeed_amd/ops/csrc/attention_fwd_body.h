// Body of attn_fwd_kernel / attn_fwd_doc_kernel (attention.hip), included inside both: a shared
// __device__ function, inlined, did not leave the existing instantiations' registers as they were.
// Expects the template parameters D, OCC, BN, RING and the constants PK, RANGE, DOC, GQA in scope, and
// the kernel argument `a`.  WIN (attn_fwd_win_kernel): a causal sliding window of `win` keys per query.
  static_assert(!(RANGE && DOC), "a key range and document spans are exclusive");
  constexpr bool RNG = RANGE || DOC || WIN;     // a tile range [t0, nt) that need not start at 0
  // K rows (ds_read_b128, 4x16-lane groups): pitch D+8 puts the 16 rows of a group on 16
  // distinct 4-bank windows.  V (ds_read_b64_tr_b16, rows rr = 0..3 x column halves g = 0,1 per
  // 32-lane group): pitch D+32 (48 / 80 dwords = 16 mod 64) places the eight 8-dword windows
  // at distinct multiples of 8 mod 64 -- D+8 aliased rows 0/2 and 1/3 (2-way conflicts).
  constexpr int KP = D + 8, VP = D + 32, NC = D / 16, NDB = D / 32, NKB = BN / 32;
  __shared__ __attribute__((aligned(16))) bf16 Ks[2][BN * KP];
  __shared__ __attribute__((aligned(16))) bf16 Vs[2][BN * VP];

  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), hh = lane >> 5,
            r = lane & 31;
  int tx, ty;
  xcd_tile(tx, ty);
  const int bh = ty, b = bh / a.H, h = bh % a.H;
  const int S = a.S;
  const int qblk = tx * 128, q0 = qblk + w * 32;
  const int q = q0 + r;
  const bool qvalid = q < S;
  // GQA: K/V come from head h / G (G = H / Hkv query heads per key/value head; the GQA forms run
  // without dropout, so the argument block carries Hkv where the keep-word count was: FwdArgs::hkv); workgroup-uniform
  int hk = h;
  if constexpr (GQA) hk = __builtin_amdgcn_readfirstlane(h / (a.H / a.hkv()));
  const float sl2 = a.slopes ? a.slopes[h] * kLog2e : 0.f;
  const float sc2 = a.scale * kLog2e;
  const bool drop = a.maskA != nullptr;
  const float inv_keep = drop ? 1.f / (1.f - a.p) : 1.f;
  const RowSrc ksrc = row_src<D>(a.k + (size_t)b * S * a.ld + hk * D, a.ld, S);
  const RowSrc vsrc = row_src<D>(a.v + (size_t)b * S * a.ld + hk * D, a.ld, S);
  // dropout: this wave's 32 queries are one query word of the key-major layout, so the keep masks
  // of a 32-key block are 16 aligned 64-bit words (lm_pos) -- scalar loads, one v_cndmask per
  // score.  A one-dword-per-lane vector load of the same 64 words a tile ahead pulls them into L2.
  const int Sp = 32 * a.W;
  // keep-word addresses stay inside the real mask buffer: the row is clamped to the plane (a wave
  // whose queries lie past S still forms it) and each block's offset to the row (keep_off)
  const uint32_t* mrow = drop ? a.maskB + ((size_t)bh * a.W + min(q0 >> 5, a.W - 1)) * Sp : nullptr;
  const __amdgpu_buffer_rsrc_t mrs = bounded_rsrc(drop ? (const void*)mrow : (const void*)a.lse, drop ? (uint32_t)Sp * 4u : 0u);

  bf16x8 qf[NC];
  {
    const bf16* qp = a.q + ((size_t)(b * S + (qvalid ? q : 0)) * a.ld + h * D);
#pragma unroll
    for (int c = 0; c < NC; ++c) qf[c] = qvalid ? *reinterpret_cast<const bf16x8*>(qp + 16 * c + 8 * hh) : bf16x8{};
  }
  f32x16 oacc[NDB];
#pragma unroll
  for (int d = 0; d < NDB; ++d) oacc[d] = f32x16{};
  float m = -INFINITY, l = 0.f;

  // key range of this sequence (RANGE): (0, S) otherwise; khi replaces S as the end of the keys
  int klo = 0, khi = S;
  if constexpr (RANGE) load_range(a.kv_range, b, S, klo, khi);
  // DOC: the block's bounds take the range's place; the lane's own span does the masking
  SpanOf<DOC> doc{};
  if constexpr (DOC) {
    load_block_range(a.doc(), a.B, b, gridDim.x, tx, S, klo, khi);
    doc = load_span(a.doc(), b, S, q);
  }
  // WIN: query q sees key j iff q - win < j <= q (the windowed forms run causal, without dropout, so
  // the argument block carries the window: FwdArgs::window).  The block's first key is that of its
  // first query, so the tile range starts there; a span takes the window in at no cost.
  int win = 0;
  if constexpr (WIN) {
    win = __builtin_amdgcn_readfirstlane(a.window());
    klo = max(klo, qblk - win + 1);
    if constexpr (DOC) doc.clip_lo(q - win + 1);
  }
  const int kend = a.causal ? min(khi, qblk + 128) : khi;
  const int nt = (kend + BN - 1) / BN;
  // first tile of the range; with no tile to run (t0 >= nt) the loop below is skipped and the
  // epilogue writes the empty rows.  `last` clamps the ring's look-ahead loads to a tile >= t0.
  const int t0 = RNG ? klo / BN : 0;
  const int last = RNG ? max(nt - 1, t0) : nt - 1;
  // K/V tiles stream through a 2-deep register ring: tile t+2's global loads are issued while
  // tile t is computed and written to LDS only at the end of tile t+1, so each load has two
  // tiles of compute to arrive (one tile of MFMA/softmax work is shorter than an HBM round trip).
  // The dropout keep words (one per 32 keys) ride along in the same ring.
  // RING = 1: one register set (tile t+1 in flight during tile t) -- 16 fewer VGPRs at BN = 64,
  // which is what 3 waves per SIMD needs.
  TileLoader<D, BN> kl0, vl0, kl1r, vl1r;
  TileLoader<D, BN>& kl1 = RING == 2 ? kl1r : kl0;
  TileLoader<D, BN>& vl1 = RING == 2 ? vl1r : vl0;
  uint32_t pf0 = 0, pf1r = 0;   // L2 prefetch of keep words (value unused)
  uint32_t& pf1 = RING == 2 ? pf1r : pf0;
  auto prefetch_words = [&](int k0, uint32_t& out) {
    asm volatile("" :: "v"(out));   // retire the previous prefetch held in this register
    out = __builtin_amdgcn_raw_buffer_load_b32(mrs, lane * 4, k0 * 4, 0);
  };
  kl0.load(ksrc, t0 * BN);
  vl0.load(vsrc, t0 * BN);
  kl0.store(Ks[0], KP);
  vl0.store(Vs[0], VP);
  {
    const int k1 = min(t0 + 1, last) * BN, k2 = min(t0 + 2, last) * BN;
    kl1.load(ksrc, k1); vl1.load(vsrc, k1); prefetch_words(k1, pf1);
    if constexpr (RING == 2) { kl0.load(ksrc, k2); vl0.load(vsrc, k2); prefetch_words(k2, pf0); }
  }
  __syncthreads();
  // SET = register set holding tile t+1 (t - t0 even -> 1, odd -> 0)
  auto tile = [&](auto set_c, int t) {
    constexpr int SET = decltype(set_c)::value;
    TileLoader<D, BN>& kn = SET ? kl1 : kl0;
    TileLoader<D, BN>& vn = SET ? vl1 : vl0;
    uint32_t& pfn = SET ? pf1 : pf0;
    const int buf = (t - t0) & 1, k0 = t * BN;
    const bf16* K = Ks[buf];
    const bf16* V = Vs[buf];
    // keep masks of the tile's first 32-key block: issued ahead of the score MFMAs (their L2
    // round trip hides under the QK^T / softmax work); the next block's after this one's selects
    uint64_t mk[16];
    auto load_masks = [&](int kb) {
      const cu64* mp = (const cu64*)(uintptr_t)(mrow + keep_off(k0 + kb * 32, Sp));
#pragma unroll
      for (int i = 0; i < 16; ++i) mk[i] = mp[i];
    };
    f32x16 sacc[NKB];
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) {
      f32x16 acc = f32x16{};
#pragma unroll
      for (int c = 0; c < NC; ++c)
        acc = mfma32(*reinterpret_cast<const bf16x8*>(&K[(kb * 32 + r) * KP + 16 * c + 8 * hh]), qf[c], acc);
      sacc[kb] = acc;
    }
    // the first block's keep masks: issued once the score MFMAs' LDS operands are consumed (an
    // outstanding scalar load makes every later LDS wait a full lgkmcnt(0)), landing under the
    // max / exp work
    if (drop) load_masks(0);
    // log2-domain scores.  Fast path (no ALiBi, interior tile): the row max is taken on the raw
    // accumulator (scale > 0) and the scale is folded into the exponent's FMA -- 4 VALU per score
    // incl. the running sum, vs 10+ with a per-element scale/bias/mask pass.
    // (RANGE: khi <= S stands for the end of the keys, and the tile holding klo is masked too)
    bool needmask = (k0 + BN > khi) || (RANGE && k0 < klo) || (a.causal && k0 + BN - 1 > q0);
    // (WIN: the wave's last query no longer sees the tile's first key)
    if constexpr (WIN && !DOC) needmask = needmask || k0 + win <= q0 + 31;
    // (DOC: some lane's span -- a pad's is empty -- leaves part of the tile out)
    if constexpr (DOC) needmask = !__all(doc.covers(k0, BN)) || (a.causal && k0 + BN - 1 > q0);
    const bool slow = needmask || sl2 != 0.f;
    float tmax = -INFINITY;
    if (slow) {
#pragma unroll
      for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int key = k0 + kb * 32 + crow(i, hh);
          float s = fmaf(sacc[kb][i], sc2, sl2 * (float)key);
          if constexpr (DOC) {
            if (needmask && (!doc.has(key) || (a.causal && key > q))) s = -INFINITY;
          } else {
            if (needmask && (key >= khi || (RANGE && key < klo) || (a.causal && key > q) || (WIN && key + win <= q))) s = -INFINITY;
          }
          sacc[kb][i] = s;
          tmax = fmaxf(tmax, s);
        }
    } else {
#pragma unroll
      for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
        for (int i = 0; i < 16; ++i) tmax = fmaxf(tmax, sacc[kb][i]);
      tmax *= sc2;
    }
    tmax = xhalf_max(tmax);
    // defer-max (wave-uniform decision): keep the running max unless some row's tile max
    // exceeds it by > kRescaleThr; the previous tile's P.V is complete, so O and l are the
    // only terms at the old scale.  m = -inf (first tile / fully masked so far) -> alpha 0.
    // (A row with every key masked so far has tmax = m = -inf: the NaN difference takes the
    // rescale, which leaves m = -inf, l = 0, O = 0.)
    // (DOC: the lanes of another document meet tiles without a key of theirs all the time; their
    // NaN difference does not vote for a rescale, which would leave them at m = -inf anyway.)
    if (DOC ? __any(tmax - m > a.thr) : !__all(tmax - m <= a.thr)) {
      const float mnew = fmaxf(m, tmax);
      const float alpha = m == -INFINITY ? 0.f : fexp2(m - mnew);
      m = mnew;
      l *= alpha;
#pragma unroll
      for (int d = 0; d < NDB; ++d) oacc[d] *= alpha;
    }
    const float mexp = m == -INFINITY ? 0.f : m;
    const float msc = slow ? 1.f : sc2;
    // l stays a per-half partial (both halves share m, hence every rescale); the two halves
    // are combined once in the epilogue.  Four independent partial sums shorten the add chain.
    if constexpr (PK) {
      const f32x2 msc2 = pk2(msc, msc), nm2 = pk2(-mexp, -mexp);
      f32x2 ps2[2];
#pragma unroll
      for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
        for (int i = 0; i < 16; i += 2) {
          const f32x2 x = pk_fma(pk2(sacc[kb][i], sacc[kb][i + 1]), msc2, nm2);
          const f32x2 pv = pk2(fexp2(x.x), fexp2(x.y));
          const int j = (i >> 1) & 1;
          ps2[j] = (kb == 0 && i < 4) ? pv : ps2[j] + pv;
          sacc[kb][i] = pv.x;
          sacc[kb][i + 1] = pv.y;
        }
      l += (ps2[0].x + ps2[0].y) + (ps2[1].x + ps2[1].y);
    } else {
      float ps[4];
#pragma unroll
      for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const float pv = fexp2(fmaf(sacc[kb][i], msc, -mexp));
          ps[i & 3] = (kb == 0 && i < 4) ? pv : ps[i & 3] + pv;   // no "+ 0" adds (-0 semantics keep them)
          sacc[kb][i] = pv;
        }
      l += (ps[0] + ps[1]) + (ps[2] + ps[3]);
    }
    if (drop) {
#pragma unroll
      for (int kb = 0; kb < NKB; ++kb) {
        if (kb > 0) load_masks(kb);
#pragma unroll
        for (int i = 0; i < 16; ++i) sacc[kb][i] = sel_keep(sacc[kb][i], mk[i]);
      }
    }
    // O^T += V^T . P^T: the score accumulator is the B operand; V^T comes from transposed reads
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        bf16x8 pf;
#pragma unroll
        for (int j = 0; j < 8; ++j) pf[j] = (bf16)sacc[kb][8 * s + j];
#pragma unroll
        for (int d = 0; d < NDB; ++d) oacc[d] = mfma32(tr_operand(V, VP, kb * 32 + 16 * s, d * 32, lane), pf, oacc[d]);
      }
    if (t + 1 < nt) {
      kn.store(Ks[buf ^ 1], KP);
      vn.store(Vs[buf ^ 1], VP);
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
  l = xhalf_sum(l);
  if (!qvalid) return;
  const float inv_l = l > 0.f ? inv_keep / l : 0.f;   // dropout 1/(1-p) folded in here
  bf16* op = a.o + (size_t)(b * S + q) * a.ldo + h * D;
#pragma unroll
  for (int d = 0; d < NDB; ++d)
#pragma unroll
    for (int gq = 0; gq < 4; ++gq) {
      bf16x4 v4;
#pragma unroll
      for (int t = 0; t < 4; ++t) v4[t] = (bf16)(oacc[d][4 * gq + t] * inv_l);
      *reinterpret_cast<bf16x4*>(op + d * 32 + 8 * gq + 4 * hh) = v4;
    }
  // (a row without a key: m = -inf, l = 0 -> -inf)
  if (hh == 0) a.lse[(size_t)bh * S + q] = (m + log2f(l)) * kLn2;
