// Incremental decoding: the KV-cache append (with the rotary embedding) and single-query attention
// against the cache.
//
// Cache layout, per layer: K, V [B, Hkv, Smax, D] -- the keys of one (sequence, key/value head) are one
// contiguous stream of D-element rows -- in one of two formats: the model's dtype, or (opt-in, bf16 models)
// OCP e4m3fn codes with one fp32 scale per row, k_scale / v_scale [B, Hkv, Smax] ("the FP8 cache", its
// quantisation law below).  Two device int32 [B] arrays are shared by all layers: kv_len (slots written)
// and kv_start (first valid slot, 0 unless the prompt was left-padded).  Nothing about the cache position
// is read back to the host: the kernels take the arrays as pointers, so their launch sequence is static
// and can be captured into a graph.
//
// dtd_rope_append: rope.hip's rotation (same table, same expression, same rounding) in place on the q
// and k heads of a packed qkv [B*Sq, (H + 2 Hkv) D] with position kv_len[b] + s, plus the copy of the
// rotated k row and of the v row of token (b, s) into slot kv_len[b] + s.  A slot outside [0, Smax) is
// not written and raises the overflow flag (a plain vector store of 1).  kv_len is not advanced here.
// dtd_rope_append_fp8 is the same on the FP8 cache (bf16 qkv): the same rotation, then the row's scale and
// codes; it is a kernel of its own, because every lane has to stay alive up to the row maximum.
//
// dtd_attn_decode / dtd_attn_decode_fp8: one query token per sequence; sequence b attends the slots
//     max(kv_start[b], hi - W) <= j < hi,   hi = min(kv_len[b], Smax)     (W = 0: no window),
// kv_len already counting the new token.  An empty range gives ctx = 0, lse = -inf.  Split-KV in two
// launches, no atomics, a fixed summation order (two calls are bitwise equal):
//   * decode_split_kernel<D, GP, FP8>, grid (splits, Hkv, B), 256 threads: one workgroup owns the keys
//     [split * kps, (split + 1) * kps) of one (sequence, key/value head), kps a multiple of the 64-key
//     tile, for all G = H / Hkv query heads of the group -- K / V are read once per group.  This is a
//     GEMV-shaped HBM stream, so K / V rows go straight into VGPRs with 16-byte loads (EPL = 8 bf16
//     elements or 16 codes per lane, D / EPL lanes per row, 64 / (D / EPL) rows per wave and load
//     instruction, the next tile's loads issued before the current tile's arithmetic) and never through
//     LDS.  The scores are packed-bf16 dot products (the codes are exact in bf16) reduced over a row's
//     lanes with DPP adds; the online-softmax state (m, l, o) is fp32 per query head and per lane group.
//     A row's two scales -- loaded by each of its lanes with the row's clamped index -- cost one multiply
//     per key and head each: k_scale[j] on the reduced score, v_scale[j] on the probability before it is
//     accumulated into o.  The format decides nothing else: the bounds and split arithmetic, the loop and
//     the reduction are one text.  LDS serves only the reduction over the lane groups at the end, which
//     writes the split's fp32 partial (m in log2 units, l, o[D]) per query head into the workspace
//     ws [splits][B][H][D + 2].  A split without a key writes (-inf, 0, 0) and returns.
//   * decode_combine_kernel, grid (H, B), D threads: merges the splits in index order, writes ctx in
//     the model's dtype and lse.
// Every load address is clamped into [lo, hi), hi <= Smax, so no slot outside the cache -- and no slot
// that was never written -- is read, whatever kv_len / kv_start hold.  All index arithmetic is 64-bit.
#include <type_traits>

#include "common.h"

using namespace dtd;

namespace {

constexpr int kKeyTile = 64;
constexpr int kMaxGroup = 8;
constexpr float kLog2e = 1.4426950408889634f;
constexpr float kLn2 = 0.6931471805599453f;

template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}

// Sum over the LPK (4, 8 or 16) aligned lanes that hold one key row; every lane gets the sum.
template <int LPK>
__device__ __forceinline__ float row_sum(float v) {
  v += dpp_f<0xB1>(v);     // quad_perm [1, 0, 3, 2]
  v += dpp_f<0x4E>(v);     // quad_perm [2, 3, 0, 1]
  if constexpr (LPK >= 8) v += dpp_f<0x141>(v);    // row_half_mirror: the other quad of the 8
  if constexpr (LPK == 16) v += dpp_f<0x140>(v);   // row_mirror: the other half of the 16
  return v;
}

// ---------------------------------------------------------------------------------- rope + append
// The rotation of one element pair (a, b) by (c, sn).  rope.hip writes a * c - b * sn and b * c + a * sn
// and its compiled form contracts the first product of each: spelled out here, so that the kernels
// round alike whatever the vectoriser makes of the loops around it.
__device__ __forceinline__ void rope_rotate(float a, float b, float c, float sn, float& oa, float& ob) {
  oa = __builtin_fmaf(a, c, -(b * sn));
  ob = __builtin_fmaf(b, c, a * sn);
}

template <typename T>
__global__ void __launch_bounds__(256) rope_append_kernel(T* __restrict__ qkv, const float* __restrict__ table,
                                                          T* __restrict__ kc, T* __restrict__ vc,
                                                          const int* __restrict__ kv_len, int* __restrict__ overflow,
                                                          size_t items, int Sq, int H, int Hkv, int D, size_t ld,
                                                          int Smax, int max_pos, float sgn) {
  const int vph = D >> 4;            // 8-wide vectors per half head
  const int half = D >> 1;
  const int heads = H + 2 * Hkv;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < items; i += (size_t)gridDim.x * blockDim.x) {
    const int v = (int)(i % vph);
    const size_t hr = i / vph;
    const int hd = (int)(hr % heads);
    const size_t row = hr / heads;
    const size_t b = row / (size_t)Sq;
    const long long slot = (long long)kv_len[b] + (long long)(row % (size_t)Sq);
    const bool fits = slot >= 0 && slot < (long long)Smax;
    T* x = qkv + row * ld + (size_t)hd * D + v * 8;
    float oa[8], ob[8];
    if (hd < H + Hkv) {              // a q or k head: rotate in place (rope.hip's expression)
      int p = slot < 0 ? 0 : (slot >= (long long)max_pos ? max_pos - 1 : (int)slot);
      const float* cs = table + ((size_t)p * half + v * 8) * 2;
      float a[8], bb[8], t[16];
      vload<T, 8>(x, a);
      vload<T, 8>(x + half, bb);
      vload<float, 16>(cs, t);
#pragma unroll
      for (int j = 0; j < 8; ++j) rope_rotate(a[j], bb[j], t[2 * j], sgn * t[2 * j + 1], oa[j], ob[j]);
      vstore<T, 8>(x, oa);
      vstore<T, 8>(x + half, ob);
      if (hd < H) continue;
    } else {
      vload<T, 8>(x, oa);
      vload<T, 8>(x + half, ob);
    }
    if (!fits) {
      *overflow = 1;
      continue;
    }
    const int hk = hd < H + Hkv ? hd - H : hd - H - Hkv;
    T* dst = (hd < H + Hkv ? kc : vc) + ((b * (size_t)Hkv + hk) * (size_t)Smax + (size_t)slot) * D + v * 8;
    vstore<T, 8>(dst, oa);
    vstore<T, 8>(dst + half, ob);
  }
}

// ---------------------------------------------------------------------------------- the FP8 cache
// K, V [B, Hkv, Smax, D] of OCP e4m3fn codes, one byte each, and k_scale, v_scale fp32 [B, Hkv, Smax]: one
// scale per D-element row.  The quantisation law (ops/kv_cache.py, quantize_kv_ref) per row x, x the
// bf16 values the bf16 cache would hold:
//     amax = max |x|;   scale = amax / 448 (1 when amax == 0);   code = e4m3(x / scale),
// both divisions IEEE fp32 (this file is built without fast-math), the conversion the hardware's
// round-to-nearest-even v_cvt_pk_fp8_f32; the dequantised value is float(code) * scale.

// Max over the LPK (4 or 8) aligned lanes that hold one row; every lane gets it.
template <int LPK>
__device__ __forceinline__ float row_max_fp8(float v) {
  v = fmaxf(v, dpp_f<0xB1>(v));     // quad_perm [1, 0, 3, 2]
  v = fmaxf(v, dpp_f<0x4E>(v));     // quad_perm [2, 3, 0, 1]
  if constexpr (LPK == 8) v = fmaxf(v, dpp_f<0x141>(v));   // row_half_mirror: the other quad of the 8
  return v;
}

// e4m3 codes of 8 floats: two dwords, element e in byte e
__device__ __forceinline__ uint2 pack_fp8x8(const float (&x)[8]) {
  uint2 w;
  int lo = __builtin_amdgcn_cvt_pk_fp8_f32(x[0], x[1], 0, false);
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(x[2], x[3], lo, true);
  int hi = __builtin_amdgcn_cvt_pk_fp8_f32(x[4], x[5], 0, false);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(x[6], x[7], hi, true);
  w.x = (unsigned)lo;
  w.y = (unsigned)hi;
  return w;
}

// dtd_rope_append_fp8: rope_append_kernel<bf16>'s rotation, bit for bit, and the quantising append.  One
// thread holds the 8 + 8 elements at v * 8 and D / 2 + v * 8 of a head row, so a row is spread over the
// LPK = D / 16 consecutive, LPK-aligned lanes of a wave (the grid stride is a multiple of 256 and the item
// count one of LPK).  The loop bound is uniform over the workgroup and nothing leaves the body early:
// every lane, live or not, reaches the row reduction.
template <int D>
__global__ void __launch_bounds__(256) rope_append_fp8_kernel(bf16* __restrict__ qkv, const float* __restrict__ table,
                                                              uint8_t* __restrict__ kc, uint8_t* __restrict__ vc,
                                                              float* __restrict__ ks, float* __restrict__ vs,
                                                              const int* __restrict__ kv_len,
                                                              int* __restrict__ overflow, size_t items, int Sq, int H,
                                                              int Hkv, size_t ld, int Smax, int max_pos) {
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
    const long long slot = (long long)kv_len[b] + (long long)(row % (size_t)Sq);
    const bool fits = slot >= 0 && slot < (long long)Smax;
    const bool rot = hd < H + Hkv;
    bf16* x = qkv + row * ld + (size_t)hd * D + v * 8;
    float oa[8] = {}, ob[8] = {};
    if (live) {
      vload<bf16, 8>(x, oa);
      vload<bf16, 8>(x + half, ob);
    }
    if (live && rot) {               // a q or k head: rotate in place (rope_append_kernel's expression)
      int p = slot < 0 ? 0 : (slot >= (long long)max_pos ? max_pos - 1 : (int)slot);
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
      if (!fits) {
        *overflow = 1;
      } else {
        const bool isk = hd < H + Hkv;
        const int hk = isk ? hd - H : hd - H - Hkv;
        const size_t r = (b * (size_t)Hkv + hk) * (size_t)Smax + (size_t)slot;
        uint8_t* dst = (isk ? kc : vc) + r * D + v * 8;
        *reinterpret_cast<uint2*>(dst) = wa;
        *reinterpret_cast<uint2*>(dst + half) = wb;
        if (v == 0) (isk ? ks : vs)[r] = scale;
      }
    }
  }
}

// ---------------------------------------------------------------------------------- decode attention
struct DecodeArgs {
  const bf16* q;      // the q block of the step's qkv: row b at q + b * ldq, head h at column h * D
  const void* k;      // [B, Hkv, Smax, D]: bf16, or e4m3 codes
  const void* v;
  const int* kv_len;
  const int* kv_start;   // or nullptr
  float* ws;          // [splits][B][H][D + 2]
  long long ldq;
  int B, H, Hkv, G, Smax, window, kps;
  float scale2;       // scale * log2(e): the scores are kept in log2 units
  const float* ks;    // the FP8 cache's row scales [B, Hkv, Smax]; nullptr for bf16
  const float* vs;
};

__device__ __forceinline__ float fexp2(float x) { return __builtin_amdgcn_exp2f(x); }

// N packed bf16 pairs: a lane's part of a K row as the dot product takes it.
template <int N>
struct Pairs {
  bf16x2 p[N];
};

__device__ __forceinline__ Pairs<4> pairs(const bf16x8 x) {
  Pairs<4> r;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    r.p[i][0] = x[2 * i];
    r.p[i][1] = x[2 * i + 1];
  }
  return r;
}

// The dot product of N packed bf16 pairs, fp32 accumulation.
template <int N>
__device__ __forceinline__ float dot(const bf16x2 (&k)[N], const bf16x2 (&q)[N]) {
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < N; ++i) {
#if __has_builtin(__builtin_amdgcn_fdot2_f32_bf16)
    s = __builtin_amdgcn_fdot2_f32_bf16(k[i], q[i], s, false);
#else
    s += (float)k[i][0] * (float)q[i][0] + (float)k[i][1] * (float)q[i][1];
#endif
  }
  return s;
}

// 16 codes -> 16 floats (v_cvt_pk_f32_fp8: exact)
__device__ __forceinline__ void unpack_fp8x16(const uint4 w, float (&f)[16]) {
  const unsigned d[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)d[i], false);
    const auto hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)d[i], true);
    f[4 * i] = lo[0];
    f[4 * i + 1] = lo[1];
    f[4 * i + 2] = hi[0];
    f[4 * i + 3] = hi[1];
  }
}

template <int D>
__device__ __forceinline__ void write_empty(const DecodeArgs& a, int split, int b, int hk) {
  for (int idx = threadIdx.x; idx < a.G * (D + 2); idx += blockDim.x) {
    const int g = idx / (D + 2), e = idx - g * (D + 2);
    const size_t base = (((size_t)split * a.B + b) * a.H + (size_t)hk * a.G + g) * (D + 2);
    a.ws[base + e] = e == 0 ? -INFINITY : 0.f;
  }
}

// GP: the group size G rounded up to a power of two (heads g >= G carry zeros and are not written).
// FP8: the cache format.  It decides the lane layout (EPL), the raw tile type, the conversion of a raw
// tile to packed bf16 pairs (K) and fp32 (V), and the two scale multiplies.  Where a format has an
// `if constexpr` arm for something the other one could share (where K's pairs are picked, the association
// of the base address, the spelling of the o stores), that arm is the spelling under which its
// instantiations compile to the code they had as a kernel of their own (profiles/attn_decode_resources.md):
// the optimiser is sensitive to it, so re-run scripts/diag/compare_kernel_asm.py after touching one.
template <int D, int GP, bool FP8>
__global__ void __launch_bounds__(256) decode_split_kernel(const DecodeArgs a) {
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

  int hi = a.kv_len[b];
  hi = hi < a.Smax ? hi : a.Smax;
  int lo = a.kv_start ? a.kv_start[b] : 0;
  lo = lo > 0 ? lo : 0;
  if (a.window > 0 && hi - a.window > lo) lo = hi - a.window;
  const int k0 = split * a.kps;
  const int k1 = k0 + a.kps < hi ? k0 + a.kps : hi;
  const int lot = lo / kKeyTile * kKeyTile;
  const int t0 = k0 > lot ? k0 : lot;    // both multiples of the tile
  if (lo >= hi || t0 >= k1) {            // no key of this split takes part
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
    for (int e = 0; e < EPL; ++e) o[g][e] = 0.f;
  }

  const size_t rows = ((size_t)b * a.Hkv + hk) * (size_t)a.Smax;    // the head's first row: elements and scales
  const Elem* K = static_cast<const Elem*>(a.k);
  const Elem* V = static_cast<const Elem*>(a.v);
  const size_t col = sub * EPL;
  const Elem* Kb = FP8 ? K + rows * D + col : K + (rows * D + col);
  const Elem* Vb = FP8 ? V + rows * D + col : V + (rows * D + col);
  const float* KSb = a.ks + rows;        // (not read for bf16)
  const float* VSb = a.vs + rows;
  const int last = hi - 1;               // lo <= last here: every address stays inside [lo, hi), hi <= Smax

  Raw kk[KPG], vv[KPG];
  float ksc[KPG], vsc[KPG];              // FP8 only: the rows' scales
#pragma unroll
  for (int i = 0; i < KPG; ++i) {
    int j = t0 + i * NG + grp;
    j = j < last ? j : last;
    j = j > lo ? j : lo;                 // a masked slot reads a live one: never-written rows and scales may hold NaN
    kk[i] = *reinterpret_cast<const Raw*>(Kb + (size_t)j * D);
    vv[i] = *reinterpret_cast<const Raw*>(Vb + (size_t)j * D);
    if constexpr (FP8) {
      ksc[i] = KSb[j];
      vsc[i] = VSb[j];
    }
  }
  for (int t = t0; t < k1; t += kKeyTile) {
    Raw kn[KPG], vn[KPG];
    float ksn[KPG], vsn[KPG];
    const int tn = t + kKeyTile < k1 ? t + kKeyTile : t;     // (the last tile is loaded twice: in bounds)
#pragma unroll
    for (int i = 0; i < KPG; ++i) {
      int j = tn + i * NG + grp;
      j = j < last ? j : last;
      j = j > lo ? j : lo;
      kn[i] = *reinterpret_cast<const Raw*>(Kb + (size_t)j * D);
      vn[i] = *reinterpret_cast<const Raw*>(Vb + (size_t)j * D);
      if constexpr (FP8) {
        ksn[i] = KSb[j];
        vsn[i] = VSb[j];
      }
    }
    bf16x2 kb[KPG][EPL / 2];             // FP8 only: the K codes as bf16, and what turns a key's dot product into its score
    float vf[KPG][EPL], kq[KPG];
    bool ok[KPG];
#pragma unroll
    for (int i = 0; i < KPG; ++i) {
      const int j = t + i * NG + grp;
      ok[i] = j >= lo && j < hi;
      if constexpr (FP8) {
        float kf[EPL];
        unpack_fp8x16(kk[i], kf);
#pragma unroll
        for (int e = 0; e < EPL / 2; ++e) {
          kb[i][e][0] = (bf16)kf[2 * e];
          kb[i][e][1] = (bf16)kf[2 * e + 1];
        }
        unpack_fp8x16(vv[i], vf[i]);
        kq[i] = ksc[i] * a.scale2;
      } else {
#pragma unroll
        for (int e = 0; e < EPL; ++e) vf[i][e] = (float)vv[i][e];
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
      for (int e = 0; e < EPL; ++e) o[g][e] *= alpha;
#pragma unroll
      for (int i = 0; i < KPG; ++i) {
        float p = fexp2(s[i] - ms);
        ls += p;
        if constexpr (FP8) p *= vsc[i];
#pragma unroll
        for (int e = 0; e < EPL; ++e) o[g][e] += p * vf[i][e];
      }
      l[g] = ls;
    }
#pragma unroll
    for (int i = 0; i < KPG; ++i) {
      kk[i] = kn[i];
      vv[i] = vn[i];
      if constexpr (FP8) {
        ksc[i] = ksn[i];
        vsc[i] = vsn[i];
      }
    }
  }

  // the reduction over the lane groups, HC query heads per pass through LDS
#pragma unroll
  for (int c = 0; c < GP; c += HC) {
    if (c) __syncthreads();
#pragma unroll
    for (int hc = 0; hc < HC; ++hc) {
      float* dst = &so[hc][grp][sub * EPL];
      if constexpr (EPL == 8) {
        *reinterpret_cast<float4*>(dst) = make_float4(o[c + hc][0], o[c + hc][1], o[c + hc][2], o[c + hc][3]);
        *reinterpret_cast<float4*>(dst + 4) = make_float4(o[c + hc][4], o[c + hc][5], o[c + hc][6], o[c + hc][7]);
      } else {
#pragma unroll
        for (int e = 0; e < EPL; e += 4)
          *reinterpret_cast<float4*>(dst + e) = make_float4(o[c + hc][e], o[c + hc][e + 1], o[c + hc][e + 2], o[c + hc][e + 3]);
      }
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

template <int D>
__global__ void __launch_bounds__(D) decode_combine_kernel(const float* __restrict__ ws, int splits, int B, int H,
                                                           bf16* __restrict__ ctx, long long ldo,
                                                           float* __restrict__ lse) {
  const int h = blockIdx.x, b = blockIdx.y, d = threadIdx.x;
  const size_t stride = (size_t)B * H * (D + 2);
  const float* p = ws + ((size_t)b * H + h) * (D + 2);
  float M = -INFINITY;
  for (int s = 0; s < splits; ++s) M = fmaxf(M, p[s * stride]);
  const float Ms = M == -INFINITY ? 0.f : M;
  float L = 0.f, acc = 0.f;
  for (int s = 0; s < splits; ++s) {
    const float w = fexp2(p[s * stride] - Ms);
    L += w * p[s * stride + 1];
    acc += w * p[s * stride + 2 + d];
  }
  const bool live = L > 0.f;
  ctx[(size_t)b * ldo + (size_t)h * D + d] = (bf16)(live ? acc / L : 0.f);
  if (d == 0) lse[(size_t)b * H + h] = live ? M * kLn2 + logf(L) : -INFINITY;
}

template <int D, bool FP8>
void launch_split(int GP, dim3 grid, hipStream_t s, const DecodeArgs& a) {
  switch (GP) {
    case 1: hipLaunchKernelGGL((decode_split_kernel<D, 1, FP8>), grid, dim3(256), 0, s, a); break;
    case 2: hipLaunchKernelGGL((decode_split_kernel<D, 2, FP8>), grid, dim3(256), 0, s, a); break;
    case 4: hipLaunchKernelGGL((decode_split_kernel<D, 4, FP8>), grid, dim3(256), 0, s, a); break;
    default: hipLaunchKernelGGL((decode_split_kernel<D, 8, FP8>), grid, dim3(256), 0, s, a); break;
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
int launch_decode(bool fp8, const void* q, long ldq, const void* k, const void* v, const float* k_scale,
                  const float* v_scale, const int* kv_len, const int* kv_start, void* ctx, long ldo, float* lse,
                  float* ws, long ws_floats, int B, int H, int Hkv, int D, int Smax, int window, float scale,
                  int splits, hipStream_t s) {
  if (B <= 0 || H <= 0) return 0;
  if (!q || !k || !v || !kv_len || !ctx || !lse || !ws) return (int)hipErrorInvalidValue;
  if (fp8 && (!k_scale || !v_scale || ((uintptr_t)k_scale | (uintptr_t)v_scale) % 4)) return (int)hipErrorInvalidValue;
  if (Hkv <= 0 || H % Hkv || H / Hkv > kMaxGroup) return (int)hipErrorInvalidValue;
  if (D != 64 && D != 128) return (int)hipErrorInvalidValue;
  if (ldq % 8 || ldq < (long)H * D || ldo < (long)H * D) return (int)hipErrorInvalidValue;
  if (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v) % 16) return (int)hipErrorInvalidValue;
  if (Smax <= 0 || window < 0 || splits < 1 || B > 65535 || Hkv > 65535) return (int)hipErrorInvalidValue;
  const int tiles = (Smax + kKeyTile - 1) / kKeyTile;
  if (splits > tiles) splits = tiles;
  if (ws_floats < (long)splits * B * H * (D + 2)) return (int)hipErrorInvalidValue;
  const int G = H / Hkv;
  DecodeArgs a;
  a.q = (const bf16*)q; a.k = k; a.v = v;
  a.kv_len = kv_len; a.kv_start = kv_start; a.ws = ws; a.ldq = ldq;
  a.B = B; a.H = H; a.Hkv = Hkv; a.G = G; a.Smax = Smax; a.window = window;
  a.kps = kKeyTile * ((tiles + splits - 1) / splits);
  a.scale2 = scale * kLog2e;
  a.ks = fp8 ? k_scale : nullptr; a.vs = fp8 ? v_scale : nullptr;
  const int GP = G <= 1 ? 1 : (G <= 2 ? 2 : (G <= 4 ? 4 : 8));
  if (D == 64) launch_both<64>(fp8, GP, splits, s, a, ctx, ldo, lse);
  else launch_both<128>(fp8, GP, splits, s, a, ctx, ldo, lse);
  DTD_LAUNCH_CHECK();
}

// The checks and the grid that dtd_rope_append and dtd_rope_append_fp8 share (each has its own rule for D, a
// positive multiple of 16 either way, and checks it first).  False: an argument error.
bool append_items(const void* qkv, const float* table, const void* kc, const void* vc, const int* kv_len,
                  const int* overflow, int B, int Sq, int H, int Hkv, int D, long ld, int Smax, int max_pos,
                  size_t* items, size_t* blocks) {
  if (!qkv || !table || !kc || !vc || !kv_len || !overflow) return false;
  if (Hkv <= 0 || H % Hkv) return false;
  if (ld % 8 != 0 || ld < (long)(H + 2 * Hkv) * D || max_pos <= 0 || Smax <= 0) return false;
  if (((uintptr_t)qkv | (uintptr_t)kc | (uintptr_t)vc) % 16) return false;
  *items = (size_t)B * Sq * (H + 2 * Hkv) * (D >> 4);
  *blocks = (*items + 255) / 256;
  if (*blocks > 8192) *blocks = 8192;
  return true;
}

}  // namespace

DTD_EXPORT int dtd_attn_decode_key_tile() { return kKeyTile; }

// ws: fp32 workspace of ws_floats >= splits * B * H * (D + 2) floats.  ldq, ldo: row strides of q and ctx
// in elements.  splits beyond the number of key tiles are cut to it.
DTD_EXPORT int dtd_attn_decode(const void* q, long ldq, const void* k, const void* v, const int* kv_len,
                               const int* kv_start, void* ctx, long ldo, float* lse, float* ws, long ws_floats, int B,
                               int H, int Hkv, int D, int Smax, int window, float scale, int splits, hipStream_t s) {
  return launch_decode(false, q, ldq, k, v, nullptr, nullptr, kv_len, kv_start, ctx, ldo, lse, ws, ws_floats, B, H, Hkv,
                       D, Smax, window, scale, splits, s);
}

// dtd_attn_decode on the FP8 cache: k, v [B, Hkv, Smax, D] e4m3 codes, k_scale, v_scale fp32 [B, Hkv, Smax];
// q / ctx bf16; everything else as dtd_attn_decode (the same workspace, the same combine kernel).
DTD_EXPORT int dtd_attn_decode_fp8(const void* q, long ldq, const void* k, const void* v, const float* k_scale,
                                   const float* v_scale, const int* kv_len, const int* kv_start, void* ctx, long ldo,
                                   float* lse, float* ws, long ws_floats, int B, int H, int Hkv, int D, int Smax,
                                   int window, float scale, int splits, hipStream_t s) {
  return launch_decode(true, q, ldq, k, v, k_scale, v_scale, kv_len, kv_start, ctx, ldo, lse, ws, ws_floats, B, H, Hkv,
                       D, Smax, window, scale, splits, s);
}

// qkv [B*Sq, (H + 2 Hkv) D] with row stride ld; kc, vc [B, Hkv, Smax, D]; overflow: one int32.
DTD_EXPORT int dtd_rope_append(int dtype, void* qkv, const float* table, void* kc, void* vc, const int* kv_len,
                               int* overflow, int B, int Sq, int H, int Hkv, int D, long ld, int Smax, int max_pos,
                               hipStream_t s) {
  if (B <= 0 || Sq <= 0 || H <= 0) return 0;
  size_t items, blocks;
  if (D <= 0 || D % 16 != 0 || !append_items(qkv, table, kc, vc, kv_len, overflow, B, Sq, H, Hkv, D, ld, Smax, max_pos,
                                            &items, &blocks))
    return (int)hipErrorInvalidValue;
  if (dtype == kBF16)
    hipLaunchKernelGGL((rope_append_kernel<bf16>), dim3(blocks), dim3(256), 0, s, (bf16*)qkv, table, (bf16*)kc,
                       (bf16*)vc, kv_len, overflow, items, Sq, H, Hkv, D, (size_t)ld, Smax, max_pos, 1.f);
  else
    hipLaunchKernelGGL((rope_append_kernel<float>), dim3(blocks), dim3(256), 0, s, (float*)qkv, table, (float*)kc,
                       (float*)vc, kv_len, overflow, items, Sq, H, Hkv, D, (size_t)ld, Smax, max_pos, 1.f);
  DTD_LAUNCH_CHECK();
}

// dtd_rope_append on the FP8 cache (bf16 qkv, D 64 or 128): kc, vc [B, Hkv, Smax, D] e4m3 codes, ks, vs fp32
// [B, Hkv, Smax].  A row that does not fit writes neither codes nor a scale and raises the flag.
DTD_EXPORT int dtd_rope_append_fp8(void* qkv, const float* table, void* kc, void* vc, float* ks, float* vs,
                                   const int* kv_len, int* overflow, int B, int Sq, int H, int Hkv, int D, long ld,
                                   int Smax, int max_pos, hipStream_t s) {
  if (B <= 0 || Sq <= 0 || H <= 0) return 0;
  size_t items, blocks;
  if ((D != 64 && D != 128) || !ks || !vs || ((uintptr_t)ks | (uintptr_t)vs) % 4 ||
      !append_items(qkv, table, kc, vc, kv_len, overflow, B, Sq, H, Hkv, D, ld, Smax, max_pos, &items, &blocks))
    return (int)hipErrorInvalidValue;
  if (D == 64)
    hipLaunchKernelGGL((rope_append_fp8_kernel<64>), dim3(blocks), dim3(256), 0, s, (bf16*)qkv, table, (uint8_t*)kc,
                       (uint8_t*)vc, ks, vs, kv_len, overflow, items, Sq, H, Hkv, (size_t)ld, Smax, max_pos);
  else
    hipLaunchKernelGGL((rope_append_fp8_kernel<128>), dim3(blocks), dim3(256), 0, s, (bf16*)qkv, table, (uint8_t*)kc,
                       (uint8_t*)vc, ks, vs, kv_len, overflow, items, Sq, H, Hkv, (size_t)ld, Smax, max_pos);
  DTD_LAUNCH_CHECK();
}
