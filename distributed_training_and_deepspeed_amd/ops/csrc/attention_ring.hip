// The ring layout of the KV cache, for sliding-window models: the append and the single-query attention of
// attention_decode.hip on a cache of R slots per (sequence, key/value head) in which position j lives in slot
// j mod R.  K, V [B, Hkv, R, D] in the model's dtype, or e4m3fn codes with k_scale / v_scale fp32 [B, Hkv, R]
// (the FP8 cache; its quantisation law is attention_decode.hip's).  R is a multiple of the 64-key tile and at
// least the window W.  kv_len and kv_start stay absolute positions -- they are the rotary positions too --
// and are read on the device only, so the launch sequence is static.
//
// dtd_rope_append_ring / _fp8: dtd_rope_append's rotation of every q and k row at position
// p = kv_len[b] + s, bit for bit (the same expressions, the same table), and the copy of the rotated k row
// and the v row into slot p mod R -- but only for s >= Sq - R, the last R rows of the call, so that one
// launch writes no slot twice (a prompt longer than the ring).  A position outside [0, max_pos) writes
// nothing and raises the overflow flag (a plain vector store of 1); there is no slot overflow.
//
// dtd_attn_decode_ring / _fp8: sequence b attends the positions lo <= j < hi, hi = kv_len[b] (the new token
// counted), lo = max(kv_start[b], 0, hi - W) -- hi - R is no further bound, as W <= R.  Slot u holds
//     pos(u) = u + off - (u > e ? R : 0),   e = (hi - 1) mod R (the newest slot),   off = hi - 1 - e,
// and takes part iff pos(u) >= lo.  The softmax sum does not depend on the order of the keys, so
// ring_split_kernel<D, GP, FP8>, grid (splits, Hkv, B), walks the ring in PHYSICAL order: split s owns the
// slots [s * kps, (s + 1) * kps), kps a multiple of the tile, and streams them exactly as the linear kernel
// streams positions -- 16-byte loads of contiguous tile-aligned rows straight into VGPRs, the next tile's
// loads issued before the current tile's arithmetic.  The ring costs the loop one add and one conditional
// subtract per key row (pos(u), for the mask); e, off and the slot of lo are formed once per workgroup,
// with the kernel's only division.  The live slots are one circular run of hi - lo <= W slots ending at e:
//   * not wrapped (slot(lo) <= e; always so while hi <= R): [slot(lo), e] -- the tiles outside it are
//     skipped, as in the linear kernel;
//   * wrapped: [0, e] and [slot(lo), R) -- only the tiles wholly inside the dead run (e, slot(lo)), at most
//     R - W slots plus what kv_start cuts off, are skipped: the loop steps over that hole.
// Both are scalar decisions, uniform over the workgroup.  A row that takes no part loads slot e instead,
// which always does: a never-written slot, or its scale, is not read, and every address is inside [0, R)
// whatever kv_len / kv_start hold.  The splits are decode_splits(B, Hkv, R), a function of the ring and not
// of the positions -- once the ring has filled every split has work.  Partials, workspace layout and
// the combine kernel are the linear kernel's (attention_combine.h); no atomics, a fixed summation order.
#include <type_traits>

#include "attention_combine.h"
#include "attention_decode_common.h"
#include "common.h"

using namespace dtd;

namespace {

// ---------------------------------------------------------------------------------- rope + append
// rope_append_kernel (attention_decode.hip) with the ring's store rule; R = the ring's slots.
template <typename T>
__global__ void __launch_bounds__(256) ring_append_kernel(T* __restrict__ qkv, const float* __restrict__ table,
                                                          T* __restrict__ kc, T* __restrict__ vc,
                                                          const int* __restrict__ kv_len, int* __restrict__ overflow,
                                                          size_t items, int Sq, int H, int Hkv, int D, size_t ld,
                                                          int R, int max_pos) {
  const int vph = D >> 4;            // 8-wide vectors per half head
  const int half = D >> 1;
  const int heads = H + 2 * Hkv;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < items; i += (size_t)gridDim.x * blockDim.x) {
    const int v = (int)(i % vph);
    const size_t hr = i / vph;
    const int hd = (int)(hr % heads);
    const size_t row = hr / heads;
    const size_t b = row / (size_t)Sq;
    const int s = (int)(row % (size_t)Sq);
    const long long pos = (long long)kv_len[b] + (long long)s;
    const bool valid = pos >= 0 && pos < (long long)max_pos;
    T* x = qkv + row * ld + (size_t)hd * D + v * 8;
    float oa[8], ob[8];
    if (hd < H + Hkv) {              // a q or k head: rotate in place (rope.hip's expression)
      int p = pos < 0 ? 0 : (pos >= (long long)max_pos ? max_pos - 1 : (int)pos);
      const float* cs = table + ((size_t)p * half + v * 8) * 2;
      float a[8], bb[8], t[16];
      vload<T, 8>(x, a);
      vload<T, 8>(x + half, bb);
      vload<float, 16>(cs, t);
#pragma unroll
      for (int j = 0; j < 8; ++j) rope_rotate(a[j], bb[j], t[2 * j], t[2 * j + 1], oa[j], ob[j]);
      vstore<T, 8>(x, oa);
      vstore<T, 8>(x + half, ob);
      if (hd < H) continue;
    } else {
      vload<T, 8>(x, oa);
      vload<T, 8>(x + half, ob);
    }
    if (!valid) {
      *overflow = 1;
      continue;
    }
    if (s < Sq - R) continue;        // not among the last R rows of the call: a later row owns the slot
    const int hk = hd < H + Hkv ? hd - H : hd - H - Hkv;
    const size_t slot = (size_t)(pos % R);
    T* dst = (hd < H + Hkv ? kc : vc) + ((b * (size_t)Hkv + hk) * (size_t)R + slot) * D + v * 8;
    vstore<T, 8>(dst, oa);
    vstore<T, 8>(dst + half, ob);
  }
}

// rope_append_fp8_kernel (attention_decode.hip) with the ring's store rule: the same rotation, row maximum,
// scale and codes; every lane, live or not, reaches the row reduction.
template <int D>
__global__ void __launch_bounds__(256) ring_append_fp8_kernel(bf16* __restrict__ qkv, const float* __restrict__ table,
                                                              uint8_t* __restrict__ kc, uint8_t* __restrict__ vc,
                                                              float* __restrict__ ks, float* __restrict__ vs,
                                                              const int* __restrict__ kv_len,
                                                              int* __restrict__ overflow, size_t items, int Sq, int H,
                                                              int Hkv, size_t ld, int R, int max_pos) {
  constexpr int LPK = D / 16;
  constexpr int half = D / 2;
  const int heads = H + 2 * Hkv;
  for (size_t i0 = blockIdx.x * (size_t)blockDim.x; i0 < items; i0 += (size_t)gridDim.x * blockDim.x) {
    const bool live = i0 + threadIdx.x < items;
    const size_t i = live ? i0 + threadIdx.x : items - 1;      // (a dead lane: the last item's indices, no access)
    const int v = (int)(i % LPK);
    const size_t hr = i / LPK;
    const int hd = (int)(hr % heads);
    const size_t row = hr / heads;
    const size_t b = row / (size_t)Sq;
    const int s = (int)(row % (size_t)Sq);
    const long long pos = (long long)kv_len[b] + (long long)s;
    const bool valid = pos >= 0 && pos < (long long)max_pos;
    const bool rot = hd < H + Hkv;
    bf16* x = qkv + row * ld + (size_t)hd * D + v * 8;
    float oa[8] = {}, ob[8] = {};
    if (live) {
      vload<bf16, 8>(x, oa);
      vload<bf16, 8>(x + half, ob);
    }
    if (live && rot) {               // a q or k head: rotate in place (rope_append_kernel's expression)
      int p = pos < 0 ? 0 : (pos >= (long long)max_pos ? max_pos - 1 : (int)pos);
      const float* cs = table + ((size_t)p * half + v * 8) * 2;
      float t[16], ra[8], rb[8];
      vload<float, 16>(cs, t);
#pragma unroll
      for (int j = 0; j < 8; ++j) rope_rotate(oa[j], ob[j], t[2 * j], t[2 * j + 1], ra[j], rb[j]);
#pragma unroll
      for (int j = 0; j < 8; ++j) {  // as rounded to bf16: what the bf16 cache would hold
        oa[j] = (float)(bf16)ra[j];
        ob[j] = (float)(bf16)rb[j];
      }
      vstore<bf16, 8>(x, oa);
      vstore<bf16, 8>(x + half, ob);
    }
    float amax = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fmaxf(fabsf(oa[j]), fabsf(ob[j])));
    amax = row_max_fp8<LPK>(amax);   // all 64 lanes are here; a row's lanes share (row, hd)
    const float scale = amax == 0.f ? 1.f : amax / 448.f;
    float ca[8], cb[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      ca[j] = oa[j] / scale;
      cb[j] = ob[j] / scale;
    }
    const uint2 wa = pack_fp8x8(ca), wb = pack_fp8x8(cb);
    if (live && hd >= H) {           // a k or v head
      if (!valid) {
        *overflow = 1;
      } else if (s >= Sq - R) {      // among the last R rows of the call
        const bool isk = hd < H + Hkv;
        const int hk = isk ? hd - H : hd - H - Hkv;
        const size_t r = (b * (size_t)Hkv + hk) * (size_t)R + (size_t)(pos % R);
        uint8_t* dst = (isk ? kc : vc) + r * D + v * 8;
        *reinterpret_cast<uint2*>(dst) = wa;
        *reinterpret_cast<uint2*>(dst + half) = wb;
        if (v == 0) (isk ? ks : vs)[r] = scale;
      }
    }
  }
}

// ---------------------------------------------------------------------------------- decode attention
// DecodeArgs with Smax = R, the ring's slots, and window = W, 1 <= W <= R.  GP, FP8, the lane layout and the
// arithmetic of a tile are decode_split_kernel's; the traversal is the ring's (file comment).
template <int D, int GP, bool FP8>
__global__ void __launch_bounds__(256) ring_split_kernel(const DecodeArgs a) {
  constexpr int EPL = FP8 ? 16 : 8;      // elements per lane: one 16-byte load
  constexpr int LPK = D / EPL;           // lanes per key row
  constexpr int GPW = 64 / LPK;          // key rows per wave and load instruction
  constexpr int NG = 4 * GPW;            // lane groups per workgroup
  constexpr int KPG = kKeyTile / NG;     // keys per lane group and tile
  constexpr int HCmax = 8192 / (NG * D); // query heads per pass of the final reduction: 32 KB of LDS
  constexpr int HC = GP < HCmax ? GP : HCmax;
  using Elem = std::conditional_t<FP8, uint8_t, bf16>;
  using Raw = std::conditional_t<FP8, uint4, bf16x8>;
  __shared__ __attribute__((aligned(16))) float so[HC][NG][D];
  __shared__ float sm[HC][NG], sl[HC][NG];

  const int split = blockIdx.x, hk = blockIdx.y, b = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int sub = lane % LPK;
  const int grp = wave * GPW + lane / LPK;
  const int G = a.G;
  const int R = a.Smax;

  const int hi = a.kv_len[b];
  int lo = a.kv_start ? a.kv_start[b] : 0;
  lo = lo > 0 ? lo : 0;
  if (hi > 0 && hi - a.window > lo) lo = hi - a.window;      // (W <= R: also the bound hi - R)
  if (hi <= 0 || lo >= hi) {             // no key at all
    write_empty<D>(a, split, b, hk);
    return;
  }
  // the circular run of live slots ends at e and begins at first, the slot of lo: lo > hi - 1 - R, so one
  // conditional add stands for lo mod R
  const int e = (hi - 1) % R;
  const int off = hi - 1 - e;            // a multiple of R: the position of slot 0 if 0 <= e
  const bool wrapped = lo < off;         // first > e: the run passes the end of the buffer
  const int first = wrapped ? lo - off + R : lo - off;
  // the tiles of this split: [tb, te) without the hole [h0, h1) of wholly dead tiles (h0 == h1: none)
  const int k0 = split * a.kps;
  const int k1 = k0 + a.kps < R ? k0 + a.kps : R;
  int tb = k0, te = k1, h0 = 0, h1 = 0;
  if (wrapped) {
    const int d0 = (e / kKeyTile + 1) * kKeyTile, d1 = first / kKeyTile * kKeyTile;
    if (d0 < d1) {
      h0 = d0;
      h1 = d1;
      if (tb >= h0 && tb < h1) tb = h1;
    }
  } else {
    const int ft = first / kKeyTile * kKeyTile;
    tb = k0 > ft ? k0 : ft;
    te = k1 < e + 1 ? k1 : e + 1;
  }
  if (tb >= te) {                        // no live slot in this split
    write_empty<D>(a, split, b, hk);
    return;
  }

  bf16x2 q[GP][EPL / 2];
#pragma unroll
  for (int g = 0; g < GP; ++g) {
    bf16x8 x0 = {}, x1 = {};             // (x1: the second 8 of an FP8 lane's 16)
    if (g < G) {
      const bf16* qp = a.q + (size_t)b * a.ldq + ((size_t)hk * G + g) * D + sub * EPL;
      x0 = *reinterpret_cast<const bf16x8*>(qp);
      if constexpr (FP8) x1 = *reinterpret_cast<const bf16x8*>(qp + 8);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      q[g][i][0] = x0[2 * i];
      q[g][i][1] = x0[2 * i + 1];
      if constexpr (FP8) {
        q[g][4 + i][0] = x1[2 * i];
        q[g][4 + i][1] = x1[2 * i + 1];
      }
    }
  }
  float m[GP], l[GP], o[GP][EPL];
#pragma unroll
  for (int g = 0; g < GP; ++g) {
    m[g] = -INFINITY;
    l[g] = 0.f;
#pragma unroll
    for (int e2 = 0; e2 < EPL; ++e2) o[g][e2] = 0.f;
  }

  const size_t rows = ((size_t)b * a.Hkv + hk) * (size_t)R;         // the head's first row: elements and scales
  const Elem* Kb = static_cast<const Elem*>(a.k) + (rows * D + sub * EPL);
  const Elem* Vb = static_cast<const Elem*>(a.v) + (rows * D + sub * EPL);
  const float* KSb = a.ks + rows;        // (not read for bf16)
  const float* VSb = a.vs + rows;

  // One tile's rows of this lane group: whether slot u = t + i * NG + grp < R takes part, and its row -- or
  // row e's, which always does -- with its scales.
  auto load = [&](int t, Raw (&kr)[KPG], Raw (&vr)[KPG], float (&kscale)[KPG], float (&vscale)[KPG], bool (&live)[KPG]) {
#pragma unroll
    for (int i = 0; i < KPG; ++i) {
      const int u = t + i * NG + grp;
      const int pos = off + (u > e ? u - R : u);     // <= hi - 1: no overflow, whatever kv_len holds
      live[i] = pos >= lo;
      const int j = live[i] ? u : e;
      kr[i] = *reinterpret_cast<const Raw*>(Kb + (size_t)j * D);
      vr[i] = *reinterpret_cast<const Raw*>(Vb + (size_t)j * D);
      if constexpr (FP8) {
        kscale[i] = KSb[j];
        vscale[i] = VSb[j];
      }
    }
  };

  Raw kk[KPG], vv[KPG];
  float ksc[KPG], vsc[KPG];              // FP8 only: the rows' scales
  bool ok[KPG];
  load(tb, kk, vv, ksc, vsc, ok);
  for (int t = tb; t < te;) {
    int nxt = t + kKeyTile;
    if (nxt == h0) nxt = h1;             // step over the dead run (h0 == h1 == 0: never)
    Raw kn[KPG], vn[KPG];
    float ksn[KPG], vsn[KPG];
    bool okn[KPG];
    load(nxt < te ? nxt : t, kn, vn, ksn, vsn, okn);         // (the last tile is loaded twice: in bounds)
    bf16x2 kb[KPG][EPL / 2];             // FP8 only: the K codes as bf16, and what turns a key's dot product into its score
    float vf[KPG][EPL], kq[KPG];
#pragma unroll
    for (int i = 0; i < KPG; ++i) {
      if constexpr (FP8) {
        float kf[EPL];
        unpack_fp8x16(kk[i], kf);
#pragma unroll
        for (int e2 = 0; e2 < EPL / 2; ++e2) {
          kb[i][e2][0] = (bf16)kf[2 * e2];
          kb[i][e2][1] = (bf16)kf[2 * e2 + 1];
        }
        unpack_fp8x16(vv[i], vf[i]);
        kq[i] = ksc[i] * a.scale2;
      } else {
#pragma unroll
        for (int e2 = 0; e2 < EPL; ++e2) vf[i][e2] = (float)vv[i][e2];
      }
    }
#pragma unroll
    for (int g = 0; g < GP; ++g) {
      float s[KPG];
      float mn = m[g];
#pragma unroll
      for (int i = 0; i < KPG; ++i) {
        float d;
        if constexpr (FP8) d = row_sum<LPK>(dot(kb[i], q[g])) * kq[i];
        else d = row_sum<LPK>(dot(pairs(kk[i]).p, q[g])) * a.scale2;
        s[i] = ok[i] ? d : -INFINITY;
        mn = fmaxf(mn, s[i]);
      }
      const float ms = mn == -INFINITY ? 0.f : mn;
      const float alpha = fexp2(m[g] - ms);
      m[g] = mn;
      float ls = l[g] * alpha;
#pragma unroll
      for (int e2 = 0; e2 < EPL; ++e2) o[g][e2] *= alpha;
#pragma unroll
      for (int i = 0; i < KPG; ++i) {
        float p = fexp2(s[i] - ms);
        ls += p;
        if constexpr (FP8) p *= vsc[i];
#pragma unroll
        for (int e2 = 0; e2 < EPL; ++e2) o[g][e2] += p * vf[i][e2];
      }
      l[g] = ls;
    }
#pragma unroll
    for (int i = 0; i < KPG; ++i) {
      kk[i] = kn[i];
      vv[i] = vn[i];
      ok[i] = okn[i];
      if constexpr (FP8) {
        ksc[i] = ksn[i];
        vsc[i] = vsn[i];
      }
    }
    t = nxt;
  }

  // the reduction over the lane groups, HC query heads per pass through LDS (decode_split_kernel's)
#pragma unroll
  for (int c = 0; c < GP; c += HC) {
    if (c) __syncthreads();
#pragma unroll
    for (int hc = 0; hc < HC; ++hc) {
      float* dst = &so[hc][grp][sub * EPL];
#pragma unroll
      for (int e2 = 0; e2 < EPL; e2 += 4)
        *reinterpret_cast<float4*>(dst + e2) = make_float4(o[c + hc][e2], o[c + hc][e2 + 1], o[c + hc][e2 + 2], o[c + hc][e2 + 3]);
      if (sub == 0) {
        sm[hc][grp] = m[c + hc];
        sl[hc][grp] = l[c + hc];
      }
    }
    __syncthreads();
    for (int idx = tid; idx < HC * D; idx += 256) {
      const int hc = idx / D, d = idx - hc * D;
      if (c + hc >= G) continue;
      float M = -INFINITY;
      for (int r = 0; r < NG; ++r) M = fmaxf(M, sm[hc][r]);
      const float Ms = M == -INFINITY ? 0.f : M;
      float L = 0.f, acc = 0.f;
      for (int r = 0; r < NG; ++r) {
        const float w = fexp2(sm[hc][r] - Ms);
        L += w * sl[hc][r];
        acc += w * so[hc][r][d];
      }
      const size_t base = (((size_t)split * a.B + b) * a.H + (size_t)hk * G + c + hc) * (D + 2);
      a.ws[base + 2 + d] = acc;
      if (d == 0) {
        a.ws[base] = M;
        a.ws[base + 1] = L;
      }
    }
  }
}

template <int D, bool FP8>
void launch_split(int GP, dim3 grid, hipStream_t s, const DecodeArgs& a) {
  switch (GP) {
    case 1: hipLaunchKernelGGL((ring_split_kernel<D, 1, FP8>), grid, dim3(256), 0, s, a); break;
    case 2: hipLaunchKernelGGL((ring_split_kernel<D, 2, FP8>), grid, dim3(256), 0, s, a); break;
    case 4: hipLaunchKernelGGL((ring_split_kernel<D, 4, FP8>), grid, dim3(256), 0, s, a); break;
    default: hipLaunchKernelGGL((ring_split_kernel<D, 8, FP8>), grid, dim3(256), 0, s, a); break;
  }
}

template <int D>
void launch_both(bool fp8, int GP, int splits, hipStream_t s, const DecodeArgs& a, void* ctx, long ldo, float* lse) {
  const dim3 grid(splits, a.Hkv, a.B);
  if (fp8) launch_split<D, true>(GP, grid, s, a);
  else launch_split<D, false>(GP, grid, s, a);
  hipLaunchKernelGGL((decode_combine_kernel<D>), dim3(a.H, a.B), dim3(D), 0, s, a.ws, splits, a.B, a.H, (bf16*)ctx,
                     (long long)ldo, lse);
}

// The two decode entry points: k_scale / v_scale are the FP8 cache's, and are checked, when fp8.
int launch_ring(bool fp8, const void* q, long ldq, const void* k, const void* v, const float* k_scale,
                const float* v_scale, const int* kv_len, const int* kv_start, void* ctx, long ldo, float* lse, float* ws,
                long ws_floats, int B, int H, int Hkv, int D, int R, int window, float scale, int splits,
                hipStream_t s) {
  if (B <= 0 || H <= 0) return 0;
  if (!q || !k || !v || !kv_len || !ctx || !lse || !ws) return (int)hipErrorInvalidValue;
  if (fp8 && (!k_scale || !v_scale || ((uintptr_t)k_scale | (uintptr_t)v_scale) % 4)) return (int)hipErrorInvalidValue;
  if (Hkv <= 0 || H % Hkv || H / Hkv > kMaxGroup) return (int)hipErrorInvalidValue;
  if (D != 64 && D != 128) return (int)hipErrorInvalidValue;
  if (ldq % 8 || ldq < (long)H * D || ldo < (long)H * D) return (int)hipErrorInvalidValue;
  if (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v) % 16) return (int)hipErrorInvalidValue;
  if (R <= 0 || R % kKeyTile || window < 1 || window > R) return (int)hipErrorInvalidValue;
  if (splits < 1 || B > 65535 || Hkv > 65535) return (int)hipErrorInvalidValue;
  const int tiles = R / kKeyTile;
  if (splits > tiles) splits = tiles;
  if (ws_floats < (long)splits * B * H * (D + 2)) return (int)hipErrorInvalidValue;
  const int G = H / Hkv;
  DecodeArgs a;
  a.q = (const bf16*)q; a.k = k; a.v = v;
  a.kv_len = kv_len; a.kv_start = kv_start; a.ws = ws; a.ldq = ldq;
  a.B = B; a.H = H; a.Hkv = Hkv; a.G = G; a.Smax = R; a.window = window;
  a.kps = kKeyTile * ((tiles + splits - 1) / splits);
  a.scale2 = scale * kLog2e;
  a.ks = fp8 ? k_scale : nullptr; a.vs = fp8 ? v_scale : nullptr;
  const int GP = G <= 1 ? 1 : (G <= 2 ? 2 : (G <= 4 ? 4 : 8));
  if (D == 64) launch_both<64>(fp8, GP, splits, s, a, ctx, ldo, lse);
  else launch_both<128>(fp8, GP, splits, s, a, ctx, ldo, lse);
  DTD_LAUNCH_CHECK();
}

}  // namespace

// dtd_attn_decode on a ring of R slots (a multiple of the key tile), 1 <= window <= R: k, v [B, Hkv, R, D].
DTD_EXPORT int dtd_attn_decode_ring(const void* q, long ldq, const void* k, const void* v, const int* kv_len,
                                    const int* kv_start, void* ctx, long ldo, float* lse, float* ws, long ws_floats,
                                    int B, int H, int Hkv, int D, int R, int window, float scale, int splits,
                                    hipStream_t s) {
  return launch_ring(false, q, ldq, k, v, nullptr, nullptr, kv_len, kv_start, ctx, ldo, lse, ws, ws_floats, B, H, Hkv, D,
                     R, window, scale, splits, s);
}

// ... on the FP8 ring: k, v [B, Hkv, R, D] e4m3 codes, k_scale, v_scale fp32 [B, Hkv, R].
DTD_EXPORT int dtd_attn_decode_ring_fp8(const void* q, long ldq, const void* k, const void* v, const float* k_scale,
                                        const float* v_scale, const int* kv_len, const int* kv_start, void* ctx,
                                        long ldo, float* lse, float* ws, long ws_floats, int B, int H, int Hkv, int D,
                                        int R, int window, float scale, int splits, hipStream_t s) {
  return launch_ring(true, q, ldq, k, v, k_scale, v_scale, kv_len, kv_start, ctx, ldo, lse, ws, ws_floats, B, H, Hkv, D,
                     R, window, scale, splits, s);
}

// dtd_rope_append on a ring: kc, vc [B, Hkv, R, D]; max_pos bounds the positions (the rotary table).
DTD_EXPORT int dtd_rope_append_ring(int dtype, void* qkv, const float* table, void* kc, void* vc, const int* kv_len,
                                    int* overflow, int B, int Sq, int H, int Hkv, int D, long ld, int R, int max_pos,
                                    hipStream_t s) {
  if (B <= 0 || Sq <= 0 || H <= 0) return 0;
  size_t items, blocks;
  if (D <= 0 || D % 16 != 0 || !append_items(qkv, table, kc, vc, kv_len, overflow, B, Sq, H, Hkv, D, ld, R, max_pos,
                                            &items, &blocks))
    return (int)hipErrorInvalidValue;
  if (dtype == kBF16)
    hipLaunchKernelGGL((ring_append_kernel<bf16>), dim3(blocks), dim3(256), 0, s, (bf16*)qkv, table, (bf16*)kc,
                       (bf16*)vc, kv_len, overflow, items, Sq, H, Hkv, D, (size_t)ld, R, max_pos);
  else
    hipLaunchKernelGGL((ring_append_kernel<float>), dim3(blocks), dim3(256), 0, s, (float*)qkv, table, (float*)kc,
                       (float*)vc, kv_len, overflow, items, Sq, H, Hkv, D, (size_t)ld, R, max_pos);
  DTD_LAUNCH_CHECK();
}

// dtd_rope_append_fp8 on a ring (bf16 qkv, D 64 or 128): kc, vc [B, Hkv, R, D] e4m3 codes, ks, vs fp32 [B, Hkv, R].
DTD_EXPORT int dtd_rope_append_ring_fp8(void* qkv, const float* table, void* kc, void* vc, float* ks, float* vs,
                                        const int* kv_len, int* overflow, int B, int Sq, int H, int Hkv, int D, long ld,
                                        int R, int max_pos, hipStream_t s) {
  if (B <= 0 || Sq <= 0 || H <= 0) return 0;
  size_t items, blocks;
  if ((D != 64 && D != 128) || !ks || !vs || ((uintptr_t)ks | (uintptr_t)vs) % 4 ||
      !append_items(qkv, table, kc, vc, kv_len, overflow, B, Sq, H, Hkv, D, ld, R, max_pos, &items, &blocks))
    return (int)hipErrorInvalidValue;
  if (D == 64)
    hipLaunchKernelGGL((ring_append_fp8_kernel<64>), dim3(blocks), dim3(256), 0, s, (bf16*)qkv, table, (uint8_t*)kc,
                       (uint8_t*)vc, ks, vs, kv_len, overflow, items, Sq, H, Hkv, (size_t)ld, R, max_pos);
  else
    hipLaunchKernelGGL((ring_append_fp8_kernel<128>), dim3(blocks), dim3(256), 0, s, (bf16*)qkv, table, (uint8_t*)kc,
                       (uint8_t*)vc, ks, vs, kv_len, overflow, items, Sq, H, Hkv, (size_t)ld, R, max_pos);
  DTD_LAUNCH_CHECK();
}
