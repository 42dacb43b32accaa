// Body of attn_bwd_dkdv_pipe_kernel (attention.hip).  Expects DROP, PIPE and the argument `a`.
// The benchmark's form of attention_bwd_dkdv_body.h only -- D = 64, 128-row query tiles, 4 waves x
// 32 keys, 2 workgroups per CU, not causal, no ALiBi, S % 128 == 0 (launch_dkdv's MASK = false) --
// with the same arithmetic in the same order (the results are bit-equal), and two changes in how the
// work is delivered and ordered:
//  * the Q / dO tiles reach LDS by LDS-DMA (dma16) instead of through 32 registers (TileLoader)
//    that were parked for a whole query tile.  The tile image is unpadded 128-byte rows whose
//    16-byte chunks are permuted inside the row (swz64_off), and a DMA piece writes 64 lanes x 16
//    bytes = 8 such rows linearly: lane L fills slot (row r0 + L / 8, position L % 8), so it FETCHES
//    chunk (L % 8) ^ swz64(row) of that row -- the swizzle sits on the source address and the
//    readers (swz_row_read, tr_operand_swz) do not change.
//  * PIPE: those 32 registers hold a second score accumulator pair, and the S / dP MFMAs of
//    sub-block qb + 1 are issued ahead of the softmax of qb, whose own scores were formed one
//    sub-block earlier: a wave no longer waits for MFMA results it has just issued.  The pipeline
//    drains at every query-tile seam (the first sub-block of a tile is not overlapped).
// S % 128 == 0: no query row and no key lies past S, so no DMA lane is out of range and nothing
// depends on what an out-of-range lane would write.  The masked forms keep attn_bwd_dkdv_kernel.
  constexpr int D = 64, BM = 128, NC = D / 16, NDB = D / 32;
  struct Smem {   // as attention_bwd_dkdv_body.h (row statistics first: 16-bit ds_read offsets)
    float lse_s[2][BM], del_s[2][BM];
    bf16 Qs[2][BM * D];
    bf16 Os[2][BM * D];
  };
  __shared__ __attribute__((aligned(16))) Smem sm;
  auto& lse_s = sm.lse_s;
  auto& del_s = sm.del_s;
  auto& Qs = sm.Qs;
  auto& Os = sm.Os;

  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), hh = lane >> 5,
            r = lane & 31;
  int tx, ty;
  xcd_tile(tx, ty);
  const int bh = ty, b = bh / a.H, h = bh % a.H;
  const int S = a.S;
  const int kblk = tx * 128;
  const int key = kblk + w * 32 + r;
  const float sc2 = a.scale * kLog2e;
  const float inv_keep = DROP ? 1.f / (1.f - a.p) : 1.f;
  // keep masks: see attention_bwd_dkdv_body.h
  const int Sp = 32 * a.W;
  const uint32_t* mrow = DROP ? a.maskA + ((size_t)bh * a.W + min((kblk >> 5) + w, a.W - 1)) * Sp : nullptr;
  const __amdgpu_buffer_rsrc_t mrs = bounded_rsrc(DROP ? (const void*)mrow : (const void*)a.lse, DROP ? (uint32_t)Sp * 4u : 0u);
  const __amdgpu_buffer_rsrc_t q_rs = bounded_rsrc(a.q + (size_t)b * S * a.ld + h * D, (uint32_t)(((S - 1) * a.ld + D) * 2));
  const __amdgpu_buffer_rsrc_t o_rs = bounded_rsrc(a.dout + (size_t)b * S * a.ldo + h * D, (uint32_t)(((S - 1) * a.ldo + D) * 2));
  const __amdgpu_buffer_rsrc_t lse_rs = bounded_rsrc(a.lse + (size_t)bh * S, (uint32_t)S * 4u);
  const __amdgpu_buffer_rsrc_t del_rs = bounded_rsrc(a.delta + (size_t)bh * S, (uint32_t)S * 4u);

  bf16x8 kf[NC], vf[NC];
  load_frags<D>(kf, a.k + (size_t)b * S * a.ld + h * D, a.ld, S, key, hh);
  load_frags<D>(vf, a.v + (size_t)b * S * a.ld + h * D, a.ld, S, key, hh);
  f32x16 dk[NDB], dv[NDB];
#pragma unroll
  for (int d = 0; d < NDB; ++d) { dk[d] = f32x16{}; dv[d] = f32x16{}; }

  const int nt = S / BM;
  // A tile is 16 pieces of 8 rows; wave w sends pieces 4 i + w (i = 0..3) of each operand, so bit 3 of
  // its rows -- the one swz64 bit that does not come from the lane -- is w & 1 for all of them and one
  // byte offset per operand serves every piece; the piece's first row goes into the scalar offset.
  const int dma_row = lane >> 3, dma_ch = ((lane & 7) ^ swz64(8 * (w & 1) + dma_row)) * 8;
  const int q_voff = (dma_row * a.ld + dma_ch) * 2, o_voff = (dma_row * a.ldo + dma_ch) * 2;
  const int q_ld2 = a.ld * 2, o_ld2 = a.ldo * 2;
  auto dma_tile = [&](int nb, int q0) {
    const uint32_t ql = lds_addr(Qs[nb]), ol = lds_addr(Os[nb]);
#pragma unroll
    for (int i = 0; i < BM / 32; ++i) dma16(q_rs, ql + (32 * i + 8 * w) * (D * 2), q_voff, (q0 + 32 * i + 8 * w) * q_ld2);
#pragma unroll
    for (int i = 0; i < BM / 32; ++i) dma16(o_rs, ol + (32 * i + 8 * w) * (D * 2), o_voff, (q0 + 32 * i + 8 * w) * o_ld2);
  };
  // Raw lse / delta of a query tile and the L2 prefetch of its keep words: compiler-visible loads,
  // issued BEFORE the tile's DMA pieces and consumed at the tile's end only (store_stats).  vmcnt
  // retires in order, so a consumer of them placed mid-tile would drain the DMA behind them.
  float lse_r = 0.f, del_r = 0.f;
  const int stat_off = threadIdx.x < BM ? (int)threadIdx.x * 4 : 0x40000000;
  auto load_stats = [&](int q0) {
    lse_r = load_stat(lse_rs, q0 * 4 + stat_off);
    del_r = load_stat(del_rs, q0 * 4 + stat_off);
  };
  auto store_stats = [&](int buf) {
    if (threadIdx.x < BM) {
      lse_s[buf][threadIdx.x] = -lse_r * kLog2e;   // stored negated: P = 2^fma(s, sc2, -lse)
      // with dropout delta is stored pre-scaled (dS' = (1 - p) dS, see attention_bwd_dkdv_body.h)
      del_s[buf][threadIdx.x] = -del_r * (DROP ? 1.f - a.p : 1.f);
    }
  };
  constexpr int NPF = BM / 64;
  uint32_t pfw[NPF] = {};
  auto prefetch_words = [&](int q0) {
#pragma unroll
    for (int j = 0; j < NPF; ++j) {
      asm volatile("" :: "v"(pfw[j]));
      pfw[j] = __builtin_amdgcn_raw_buffer_load_b32(mrs, (lane + 64 * j) * 4, q0 * 4, 0);
    }
  };
  // S and dP of sub-block qb of the tile (Q, O): 8 MFMAs on ds_read_b128 rows
  auto row_reads = [&](const bf16* Q, const bf16* O, int qb, bf16x8 (&qa)[NC], bf16x8 (&oa)[NC]) {
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      qa[c] = swz_row_read(Q, qb * 32, r, 2 * c + hh);
      oa[c] = swz_row_read(O, qb * 32, r, 2 * c + hh);
    }
  };
  auto score_mfmas = [&](const bf16x8 (&qa)[NC], const bf16x8 (&oa)[NC], f32x16& sacc, f32x16& pacc) {
    sacc = f32x16{};
    pacc = f32x16{};
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      sacc = mfma32(qa[c], kf[c], sacc);
      pacc = mfma32(oa[c], vf[c], pacc);
    }
  };
  auto scores = [&](const bf16* Q, const bf16* O, int qb, f32x16& sacc, f32x16& pacc) {
    bf16x8 qa[NC], oa[NC];
    row_reads(Q, O, qb, qa, oa);
    score_mfmas(qa, oa, sacc, pacc);
  };
  auto load_keep = [&](int qrow0, uint64_t (&mk)[16]) {
    if constexpr (DROP) {
      const cu64* mp = (const cu64*)(uintptr_t)(mrow + keep_off(qrow0, Sp));
#pragma unroll
      for (int i = 0; i < 16; ++i) mk[i] = mp[i];
    }
  };
  // row statistics of this lane's 16 accumulator rows (rows 8g + 4hh + 0..3 are contiguous)
  auto read_stats = [&](int buf, int qb, f32x4 (&L4)[4], f32x4 (&D4)[4]) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      L4[g] = *reinterpret_cast<const f32x4*>(&lse_s[buf][qb * 32 + 8 * g + 4 * hh]);
      D4[g] = *reinterpret_cast<const f32x4*>(&del_s[buf][qb * 32 + 8 * g + 4 * hh]);
    }
  };
  // P = 2^(s sc2 - lse), dS (dropout: P keep and dS' = (1 - p) dS): attention_bwd_dkdv_body.h's, unmasked
  auto softmax = [&](f32x16& sacc, f32x16& pacc, const uint64_t (&mk)[16], const f32x4 (&L4)[4], const f32x4 (&D4)[4]) {
    const f32x2 sc2v = pk2(sc2, sc2);
#pragma unroll
    for (int i = 0; i < 16; i += 2) {
      const f32x2 nl = pk2(L4[i >> 2][i & 3], L4[i >> 2][(i & 3) + 1]);
      const f32x2 x = pk_fma(pk2(sacc[i], sacc[i + 1]), sc2v, nl);
      sacc[i] = fexp2(x.x);
      sacc[i + 1] = fexp2(x.y);
    }
#pragma unroll
    for (int i = 0; i < 16; i += 2) {
      const f32x2 nd = pk2(D4[i >> 2][i & 3], D4[i >> 2][(i & 3) + 1]);
      if constexpr (DROP) {
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
  };
  // dV^T += dO^T P, dK^T += Q^T dS of sub-block qb: 8 MFMAs on transposed LDS reads
  auto grads = [&](const bf16* Q, const bf16* O, int qb, const f32x16& sacc, const f32x16& pacc) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      bf16x8 pb, sb;
#pragma unroll
      for (int j = 0; j < 8; ++j) { pb[j] = (bf16)sacc[8 * s + j]; sb[j] = (bf16)pacc[8 * s + j]; }
#pragma unroll
      for (int d = 0; d < NDB; ++d) {
        dv[d] = mfma32(tr_operand_swz(O, qb * 32 + 16 * s, d * 32, lane), pb, dv[d]);
        dk[d] = mfma32(tr_operand_swz(Q, qb * 32 + 16 * s, d * 32, lane), sb, dk[d]);
      }
    }
  };

  load_stats(0);
  dma_tile(0, 0);
  store_stats(0);
  // A use of the K / V fragments here, so that the compiler waits for them in the prologue: left to
  // their first MFMA, in the loop, their counted waits (vmcnt(9) .. vmcnt(2): the loads the compiler
  // knows of) would stand behind the loop head's DMA pieces and drain them at the head of every tile.
#pragma unroll
  for (int c = 0; c < NC; ++c) asm volatile("" : "+v"(kf[c]), "+v"(vf[c]));
  wait_vm<0>();   // the DMA is hidden from the compiler: __syncthreads() does not wait for it
  __syncthreads();
  for (int t = 0; t < nt; ++t) {
    const int buf = t & 1, q0 = t * BM;
    if (t + 1 < nt) {   // (the barrier that ended tile t - 1: nobody reads buffer buf ^ 1 any more)
      load_stats(q0 + BM);
      if (DROP) prefetch_words(q0 + BM);
      dma_tile(buf ^ 1, q0 + BM);
    }
    const bf16* Q = Qs[buf];
    const bf16* O = Os[buf];
    if constexpr (PIPE) {
      f32x16 sacc[2], pacc[2];
      scores(Q, O, 0, sacc[0], pacc[0]);
#pragma unroll
      for (int qb = 0; qb < BM / 32; ++qb) {
        const int cur = qb & 1;
        __builtin_amdgcn_sched_barrier(0);
        uint64_t mk[16];
        f32x4 L4[4], D4[4];
        read_stats(buf, qb, L4, D4);
        if constexpr (DROP) {
          // The scalar mask loads share lgkmcnt with LDS and return out of order: with one in flight
          // every wait for an LDS read is lgkmcnt(0), the mask round trip included.  So all the LDS
          // operands are read and waited for first (the empty asm is their use), and the mask loads
          // go out just ahead of the MFMAs, whose operands are then in registers: their round trip
          // passes under the MFMAs and the exponentials, which do not need them.
          bf16x8 qa[NC], oa[NC];
          if (qb + 1 < BM / 32) {
            row_reads(Q, O, qb + 1, qa, oa);
#pragma unroll
            for (int c = 0; c < NC; ++c) asm volatile("" : "+v"(qa[c]), "+v"(oa[c]));
          }
#pragma unroll
          for (int g = 0; g < 4; ++g) asm volatile("" : "+v"(L4[g]), "+v"(D4[g]));
          __builtin_amdgcn_sched_barrier(0);
          load_keep(q0 + qb * 32, mk);
          if (qb + 1 < BM / 32) score_mfmas(qa, oa, sacc[cur ^ 1], pacc[cur ^ 1]);
        } else {
          if (qb + 1 < BM / 32) scores(Q, O, qb + 1, sacc[cur ^ 1], pacc[cur ^ 1]);
        }
        __builtin_amdgcn_sched_barrier(0);   // the statistics (and masks) of qb land under those MFMAs
        softmax(sacc[cur], pacc[cur], mk, L4, D4);
        grads(Q, O, qb, sacc[cur], pacc[cur]);
      }
    } else {
#pragma unroll 1
      for (int qb = 0; qb < BM / 32; ++qb) {
        f32x16 sacc, pacc;
        uint64_t mk[16];
        f32x4 L4[4], D4[4];
        scores(Q, O, qb, sacc, pacc);
        load_keep(q0 + qb * 32, mk);   // (after the S / dP MFMAs consumed their LDS operands)
        read_stats(buf, qb, L4, D4);
        softmax(sacc, pacc, mk, L4, D4);
        grads(Q, O, qb, sacc, pacc);
      }
    }
    if (t + 1 < nt) store_stats(buf ^ 1);
    wait_vm<0>();   // this wave's DMA pieces have landed; the barrier makes that true of every wave's
    __syncthreads();
  }
  const float dv_scale = inv_keep;   // the dropped P fed to dV carried keep bits only
  const float dk_scale = a.scale * inv_keep;   // dS' = (1 - p) dS
  if (a.bias_part) {
    float vk[32], vv[32];
#pragma unroll
    for (int d = 0; d < NDB; ++d)
#pragma unroll
      for (int i = 0; i < 16; ++i) {   // the stored (bf16-rounded) values
        vk[16 * d + i] = (float)(bf16)(dk[d][i] * dk_scale);
        vv[16 * d + i] = (float)(bf16)(dv[d][i] * dv_scale);
      }
    const float sk = colsum32(vk, r), sv = colsum32(vv, r);
    float* row = a.bias_part + ((size_t)b * gridDim.x * 4 + (kblk >> 5) + w) * (3 * a.H * D) + h * D + colsum_col(r, hh);
    row[a.H * D] = sk;
    row[2 * a.H * D] = sv;
  }
  store_rows16<NDB>(a.dk + (size_t)(b * S + key) * a.ld + h * D, dk, dk_scale, hh, true);
  store_rows16<NDB>(a.dv + (size_t)(b * S + key) * a.ld + h * D, dv, dv_scale, hh, true);
