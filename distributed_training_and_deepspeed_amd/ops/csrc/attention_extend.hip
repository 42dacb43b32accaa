// Multi-token attention against the KV cache ("extend"): T new tokens per sequence on top of a non-empty
// cache -- a further user turn, one chunk of a chunked prefill, the verification pass of speculative decoding.
//
// hipcc-flags: -Xclang -target-feature -Xclang -packed-fp32-ops
//
// Cache layout and formats are attention_decode.hip's: K, V [B, Hkv, Smax, D] in bf16, or e4m3fn codes with one
// fp32 scale per row (k_scale / v_scale [B, Hkv, Smax]).  q is the q block of the chunk's packed projection
// [B*T, (H + 2 Hkv) D], row b*T + t token t of sequence b; the chunk's own k / v rows are already in the cache
// at the slots kv_len[b] + t, kv_len counting the slots written BEFORE the chunk.  Query (b, t) sits at
// position p = kv_len[b] + t and attends
//     lo <= j < hi,   hi = min(p + 1, Smax),   lo = max(kv_start[b], 0, hi - W)     (W = 0: no window);
// T = 1 is the decode kernel's range.  A row without a key gives ctx = 0, lse = -inf.
//
// dtd_attn_extend / dtd_attn_extend_fp8 launch extend_kernel<D, FP8, KS>, grid (row blocks x splits, Hkv, B),
// 256 threads, and for splits > 1 decode_combine_kernel (attention_combine.h) over the B*T rows.
//   * Rows.  The R = T G (token, group head) pairs of one (sequence, key/value head) are the rows of one
//     product, token-major (r = t G + g): a 16-row slab spans few positions, so its causal / window edge
//     crosses few key tiles, and K / V are fetched once per row block, not once per head or token.
//   * Products.  Both are v_mfma_f32_16x16x32_bf16 with fp32 accumulators.  The scores are computed
//     transposed, S^T = K Q^T: lane (kq, i) = (lane / 16, lane % 16) holds 8 consecutive elements of key i of
//     a 16-key block as the row operand -- exactly as the key lies in memory, one 16-byte load, no LDS --
//     and the same 8 elements of query row i as the column operand.  The result leaves lane (kq, i) with
//     the scores of query i against keys 4 kq .. 4 kq + 3 of the block.  Two blocks side by side are then
//     the column operand of O^T = V^T P^T as they stand: MFMA k index 8 kq + e is key 4 kq + e of the first
//     block (e < 4) or 4 kq + e - 4 of the second.  P is never transposed; the key permutation is applied
//     to V's read instead.  V is staged through LDS (two buffers of one 64-key tile, rows padded to D + 8)
//     and read with ds_read_b64_tr_b16: the 16-lane group kq reads rows 4 kq .. 4 kq + 3 of a block, 16
//     columns wide, and gets them transposed -- two reads make the 8-deep row operand.  O^T leaves lane
//     (kq, i) with elements d = 16 db + 4 kq .. + 3 of query i: 8 bytes of bf16, or two float2 of a partial.
//     With an FP8 cache a lane's 16-byte K load holds 16 codes, which feed two MFMAs (the sum over d is
//     order-free and q is loaded in the same order); codes become bf16, exactly, in registers (K) or on
//     their way into LDS (V) with v_cvt_pk_f32_fp8.  k_scale[j] multiplies the fp32 score and v_scale[j] the
//     probability: one multiply per key and row each.  The format decides nothing else.
//   * Softmax.  The online state (m, l) per row is fp32 in log2 units, m shared by the four lanes of a
//     query (two cross-lane maxima per tile), l a per-lane partial summed at the end.
//   * The arrangement of the four waves is a rule on R alone:
//         R <= 16: "key split" (KS).  One 16-row slab per workgroup; wave w takes key block w of every
//                  64-key tile (its second MFMA half carries zero probabilities) and the four (m, l, o)
//                  are merged through LDS at the end, in wave order.
//         R  > 16: "slabs".  A workgroup owns 64 rows, wave w the slab of rows 16 w .. 16 w + 15 and all
//                  four key blocks of a tile; a wave whose slab lies beyond R only helps to stage V.
//   * Pipeline.  The K registers and the V staging registers of tile t + 1 are loaded before tile t's
//     arithmetic; V(t + 1) goes into the other LDS buffer after it: one barrier per tile.
//   * Masks.  A wave skips a tile that lies wholly outside its slab's key range, and runs the per-score
//     test (causal edge, window edge, kv_start, the end of the live range) only in tiles that an edge
//     crosses.  A (row block, split) pair without a key writes (-inf, 0, 0) -- or, with one split, ctx = 0
//     and lse = -inf -- and returns.
//   * Split-KV.  Split s owns the keys [s kps, (s + 1) kps), kps a multiple of the 64-key tile, and writes
//     fp32 partials (m, l, o[D]) to ws [splits][B*T][H][D + 2].  With splits == 1 the kernel normalises,
//     rounds and writes ctx and lse itself and touches no workspace.  No atomics: two calls are bitwise equal.
// Every load address (rows and scales) is clamped into the workgroup's live key range, which lies inside
// [kv_start, kv_len + T) and inside the cache, so a slot that was never written is never read -- dead slots
// may hold NaN.  All index arithmetic is 64-bit; all stores are plain vector stores.
#include <type_traits>

#include "attention_combine.h"
#include "common.h"

using namespace dtd;

namespace {

constexpr int kKeyTile = 64;
constexpr int kMaxGroup = 8;
constexpr int kSlab = 16;
constexpr float kLog2e = 1.4426950408889634f;

typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

struct ExtendArgs {
  const bf16* q;      // the q block of the chunk's qkv: row b*T + t at q + (b*T + t) * ldq, head h at column h * D
  const void* k;      // [B, Hkv, Smax, D]: bf16, or e4m3 codes
  const void* v;
  const float* ks;    // the FP8 cache's row scales [B, Hkv, Smax]; nullptr for bf16
  const float* vs;
  const int* kv_len;  // slots written before the chunk
  const int* kv_start;   // or nullptr
  bf16* ctx;          // [B*T, H*D], row stride ldo
  float* lse;         // [B*T, H]
  float* ws;          // [splits][B*T][H][D + 2]; not touched when splits == 1
  long long ldq, ldo;
  int B, T, H, Hkv, G, Smax, window, kps, splits;
  float scale2;       // scale * log2(e): the scores are kept in log2 units
};

// The key range of token t of a sequence (file header).
struct Bounds {
  long long len;
  int st, W, Smax;
  __device__ __forceinline__ int hi(int t) const {
    long long h = len + t + 1;
    h = h < Smax ? h : Smax;
    return (int)(h > 0 ? h : 0);
  }
  __device__ __forceinline__ int lo(int hi) const { return W > 0 && hi - W > st ? hi - W : st; }
};

__device__ __forceinline__ f32x4 mfma16(bf16x8 a, bf16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// ds_read_b64_tr_b16: lane 4q + p of each 16-lane group passes the address of row q, columns 4p .. 4p + 3 of
// a 4 x 16 block; lane i of the group receives column i (rows 0 .. 3).
__device__ __forceinline__ bf16x4 tr_read(const bf16* p) {
  const s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p));
  return __builtin_bit_cast(bf16x4, v);
}

// 8 codes (two dwords, element e in byte e) -> 8 bf16 (v_cvt_pk_f32_fp8, then the pack: exact)
__device__ __forceinline__ bf16x8 codes_bf16(unsigned lo, unsigned hi) {
  const auto a = __builtin_amdgcn_cvt_pk_f32_fp8((int)lo, false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)lo, true);
  const auto c = __builtin_amdgcn_cvt_pk_f32_fp8((int)hi, false), d = __builtin_amdgcn_cvt_pk_f32_fp8((int)hi, true);
  bf16x8 r;
  r[0] = (bf16)a[0]; r[1] = (bf16)a[1]; r[2] = (bf16)b[0]; r[3] = (bf16)b[1];
  r[4] = (bf16)c[0]; r[5] = (bf16)c[1]; r[6] = (bf16)d[0]; r[7] = (bf16)d[1];
  return r;
}

__device__ __forceinline__ int clampi(int j, int lo, int last) {
  j = j < last ? j : last;
  return j > lo ? j : lo;
}

// The final form of elements d .. d + 3 of one row (head = the lane that also writes the row's scalars): with
// one split ctx and lse, else the split's partial.
template <int D>
__device__ __forceinline__ void finish(const ExtendArgs& a, int split, int b, int hk, int row, int d, float M, float L,
                                       const f32x4 o, bool head) {
  const int t = row / a.G, g = row - t * a.G;
  const size_t qrow = (size_t)b * a.T + t;
  const size_t h = (size_t)hk * a.G + g;
  if (a.splits == 1) {
    const bool live = L > 0.f;
    bf16x4 y;
#pragma unroll
    for (int r = 0; r < 4; ++r) y[r] = (bf16)(live ? o[r] / L : 0.f);
    *reinterpret_cast<bf16x4*>(a.ctx + qrow * (size_t)a.ldo + h * D + d) = y;
    if (head) a.lse[qrow * a.H + h] = live ? M * kLn2 + logf(L) : -INFINITY;
  } else {
    float* p = a.ws + (((size_t)split * a.B * a.T + qrow) * a.H + h) * (D + 2);
    *reinterpret_cast<float2*>(p + 2 + d) = make_float2(o[0], o[1]);
    *reinterpret_cast<float2*>(p + 4 + d) = make_float2(o[2], o[3]);
    if (head) *reinterpret_cast<float2*>(p) = make_float2(M, L);
  }
}

// Rows [row0, rowN) of a (row block, split) pair without a key.
template <int D>
__device__ __forceinline__ void write_empty(const ExtendArgs& a, int split, int b, int hk, int row0, int rowN) {
  for (int idx = threadIdx.x; idx < (rowN - row0) * (D + 2); idx += blockDim.x) {
    const int row = row0 + idx / (D + 2), e = idx % (D + 2);
    const int t = row / a.G, g = row - t * a.G;
    const size_t qrow = (size_t)b * a.T + t;
    const size_t h = (size_t)hk * a.G + g;
    if (a.splits == 1) {
      if (e == 0) a.lse[qrow * a.H + h] = -INFINITY;
      else if (e >= 2) a.ctx[qrow * (size_t)a.ldo + h * D + (e - 2)] = (bf16)0.f;
    } else {
      a.ws[(((size_t)split * a.B * a.T + qrow) * a.H + h) * (D + 2) + e] = e == 0 ? -INFINITY : 0.f;
    }
  }
}

// FP8: the cache format.  KS: the key-split arrangement (R <= 16), else slabs (file header).
template <int D, bool FP8, bool KS>
__global__ void __launch_bounds__(256) extend_kernel(const ExtendArgs a) {
  constexpr int NC = D / 32;                    // score MFMAs per key block: 32 elements of d each
  constexpr int EPP = FP8 ? 16 : 8;             // elements per 16-byte piece
  constexpr int NL = D / (4 * EPP);             // 16-byte K loads per key and lane
  constexpr int NDB = D / 16;                   // 16-element blocks of d: accumulators of O^T
  constexpr int NKB = KS ? 1 : 4;               // key blocks per wave and tile
  constexpr int WGR = KS ? kSlab : 4 * kSlab;   // rows per workgroup
  constexpr int VP = D + 8;                     // LDS pitch of a V row
  constexpr int PPR = D / EPP;                  // pieces per V row
  constexpr int VPT = kKeyTile * PPR / 256;     // V pieces per thread and tile
  using Elem = std::conditional_t<FP8, uint8_t, bf16>;
  __shared__ __attribute__((aligned(16))) bf16 Vs[2][kKeyTile * VP];
  __shared__ float sm[4][kSlab], sl[4][kSlab];  // KS: the waves' (m, l)
  static_assert(sizeof(Vs) >= 4 * kSlab * D * sizeof(float), "the KS merge reuses V's buffers");

  const int rb = blockIdx.x / a.splits, split = blockIdx.x - rb * a.splits, hk = blockIdx.y, b = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 15, kq = lane >> 4;
  const int G = a.G, R = a.T * G;

  Bounds bd;
  bd.len = a.kv_len[b];
  bd.st = a.kv_start ? a.kv_start[b] : 0;
  bd.st = bd.st > 0 ? bd.st : 0;
  bd.W = a.window;
  bd.Smax = a.Smax;

  // the workgroup's rows and their key range: lo and hi do not decrease with the row
  const int row0 = rb * WGR;
  const int rowN = row0 + WGR < R ? row0 + WGR : R;
  const int wg_lo = bd.lo(bd.hi(row0 / G)), wg_hi = bd.hi((rowN - 1) / G);
  const int k0 = split * a.kps;
  const int k1 = k0 + a.kps < wg_hi ? k0 + a.kps : wg_hi;
  const int lot = wg_lo / kKeyTile * kKeyTile;
  const int t0 = k0 > lot ? k0 : lot;           // both multiples of the tile
  if (wg_lo >= wg_hi || t0 >= k1) {             // no key of this split takes part
    write_empty<D>(a, split, b, hk, row0, rowN);
    return;
  }
  const int last = wg_hi - 1;                   // wg_lo <= last: every address stays inside [wg_lo, wg_hi)

  // this wave's slab and this lane's query row (a row at or beyond R is a copy of row R - 1, never stored)
  const int srow0 = row0 + (KS ? 0 : wave * kSlab);
  const bool active = srow0 < R;                // (wave-uniform)
  const int sfirst = active ? srow0 : R - 1;
  const int slast = srow0 + kSlab - 1 < R ? srow0 + kSlab - 1 : R - 1;
  const int s_hi_min = bd.hi(sfirst / G), s_hi_max = bd.hi(slast / G);
  const int s_lo_min = bd.lo(s_hi_min), s_lo_max = bd.lo(s_hi_max);
  const int row = srow0 + col;
  const int rowc = row < R ? row : R - 1;
  const int tq = rowc / G, gq = rowc - tq * G;
  const int hi_q = bd.hi(tq), lo_q = bd.lo(hi_q);

  // q in the order of K's loads: MFMA c of a lane takes d = 32 c + 8 kq + e (bf16), or
  // 64 (c / 2) + 16 kq + 8 (c % 2) + e (codes: the two halves of one 16-byte load)
  bf16x8 qf[NC];
  {
    const bf16* qp = a.q + ((size_t)b * a.T + tq) * (size_t)a.ldq + ((size_t)hk * G + gq) * D;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int d = FP8 ? 64 * (c >> 1) + 16 * kq + 8 * (c & 1) : 32 * c + 8 * kq;
      qf[c] = *reinterpret_cast<const bf16x8*>(qp + d);
    }
  }

  const size_t rows = ((size_t)b * a.Hkv + hk) * (size_t)a.Smax;   // the head's first row: elements and scales
  const Elem* Kb = static_cast<const Elem*>(a.k) + rows * D + kq * EPP;
  const Elem* Vb = static_cast<const Elem*>(a.v) + rows * D;
  const float* KSb = a.ks + rows;               // (not read for bf16)
  const float* VSb = a.vs + rows;
  const int kb0 = KS ? wave : 0;                // this wave's first key block of a tile

  float m = -INFINITY, l = 0.f;
  f32x4 o[NDB];
#pragma unroll
  for (int db = 0; db < NDB; ++db) o[db] = f32x4{0.f, 0.f, 0.f, 0.f};

  uint4 kn[NKB][NL], vr[VPT];
  float ksn[NKB][4], vsn[NKB][4];               // FP8 only: the scales of a lane's four keys per block
#pragma unroll
  for (int kb = 0; kb < NKB; ++kb) {
    const int j = clampi(t0 + 16 * (kb0 + kb) + col, wg_lo, last);
#pragma unroll
    for (int i = 0; i < NL; ++i) kn[kb][i] = *reinterpret_cast<const uint4*>(Kb + (size_t)j * D + i * 4 * EPP);
    if constexpr (FP8) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int js = clampi(t0 + 16 * (kb0 + kb) + 4 * kq + r, wg_lo, last);
        ksn[kb][r] = KSb[js];
        vsn[kb][r] = VSb[js];
      }
    }
  }
#pragma unroll
  for (int i = 0; i < VPT; ++i) {
    const int idx = i * 256 + tid, r = idx / PPR, pc = idx - r * PPR;
    const int j = clampi(t0 + r, wg_lo, last);
    vr[i] = *reinterpret_cast<const uint4*>(Vb + (size_t)j * D + pc * EPP);
  }
#pragma unroll
  for (int i = 0; i < VPT; ++i) {
    const int idx = i * 256 + tid, r = idx / PPR, pc = idx - r * PPR;
    bf16* dst = &Vs[0][r * VP + pc * EPP];
    if constexpr (FP8) {
      *reinterpret_cast<bf16x8*>(dst) = codes_bf16(vr[i].x, vr[i].y);
      *reinterpret_cast<bf16x8*>(dst + 8) = codes_bf16(vr[i].z, vr[i].w);
    } else {
      *reinterpret_cast<uint4*>(dst) = vr[i];
    }
  }
  __syncthreads();

  int buf = 0;
  for (int t = t0; t < k1; t += kKeyTile, buf ^= 1) {
    uint4 kc[NKB][NL];
    float ksc[NKB][4], vsc[NKB][4];
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) {
#pragma unroll
      for (int i = 0; i < NL; ++i) kc[kb][i] = kn[kb][i];
      if constexpr (FP8) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          ksc[kb][r] = ksn[kb][r];
          vsc[kb][r] = vsn[kb][r];
        }
      }
    }
    const bool more = t + kKeyTile < k1;        // (uniform)
    const int tn = more ? t + kKeyTile : t;     // (the last tile is loaded twice: in bounds)
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) {
      const int j = clampi(tn + 16 * (kb0 + kb) + col, wg_lo, last);
#pragma unroll
      for (int i = 0; i < NL; ++i) kn[kb][i] = *reinterpret_cast<const uint4*>(Kb + (size_t)j * D + i * 4 * EPP);
      if constexpr (FP8) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int js = clampi(tn + 16 * (kb0 + kb) + 4 * kq + r, wg_lo, last);
          ksn[kb][r] = KSb[js];
          vsn[kb][r] = VSb[js];
        }
      }
    }
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
      const int idx = i * 256 + tid, r = idx / PPR, pc = idx - r * PPR;
      const int j = clampi(tn + r, wg_lo, last);
      vr[i] = *reinterpret_cast<const uint4*>(Vb + (size_t)j * D + pc * EPP);
    }

    const int w0 = t + 16 * kb0, w1 = w0 + 16 * NKB;       // this wave's keys of the tile
    if (active && w1 > s_lo_min && w0 < s_hi_max) {        // (wave-uniform) else: wholly outside the slab's range
      f32x4 s[NKB];
#pragma unroll
      for (int kb = 0; kb < NKB; ++kb) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          bf16x8 kf;
          if constexpr (FP8) {
            const uint4 w = kc[kb][c >> 1];
            kf = (c & 1) ? codes_bf16(w.z, w.w) : codes_bf16(w.x, w.y);
          } else {
            kf = __builtin_bit_cast(bf16x8, kc[kb][c]);
          }
          acc = mfma16(kf, qf[c], acc);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if constexpr (FP8) acc[r] *= ksc[kb][r] * a.scale2;
          else acc[r] *= a.scale2;
        }
        s[kb] = acc;
      }
      if (w0 < s_lo_max || w1 > s_hi_min) {                // an edge crosses these keys: the per-score test
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int j = w0 + 16 * kb + 4 * kq + r;
            if (j < lo_q || j >= hi_q) s[kb][r] = -INFINITY;
          }
      }
      float mx = -INFINITY;
#pragma unroll
      for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
        for (int r = 0; r < 4; ++r) mx = fmaxf(mx, s[kb][r]);
      mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float mn = fmaxf(m, mx);
      const float ms = mn == -INFINITY ? 0.f : mn;
      const float alpha = fexp2(m - ms);
      m = mn;
      float ls = l * alpha;
#pragma unroll
      for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float p = fexp2(s[kb][r] - ms);
          ls += p;
          if constexpr (FP8) p *= vsc[kb][r];
          s[kb][r] = p;
        }
      l = ls;
#pragma unroll
      for (int db = 0; db < NDB; ++db)
#pragma unroll
        for (int r = 0; r < 4; ++r) o[db][r] *= alpha;
      const bf16* vt = &Vs[buf][(16 * kb0 + 4 * kq + (col >> 2)) * VP + 4 * (col & 3)];
#pragma unroll
      for (int kg = 0; kg < (NKB + 1) / 2; ++kg) {          // 32 keys: blocks 2 kg and 2 kg + 1
        bf16x8 pf;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          pf[r] = (bf16)s[2 * kg][r];
          if constexpr (KS) pf[4 + r] = (bf16)0.f;
          else pf[4 + r] = (bf16)s[NKB > 1 ? 2 * kg + 1 : 0][r];
        }
        const bf16* vg = vt + 32 * kg * VP;
#pragma unroll
        for (int db = 0; db < NDB; ++db) {
          const bf16x4 v0 = tr_read(vg + 16 * db);
          const bf16x4 v1 = KS ? v0 : tr_read(vg + 16 * VP + 16 * db);   // (KS: times zero, any finite value)
          o[db] = mfma16(__builtin_shufflevector(v0, v1, 0, 1, 2, 3, 4, 5, 6, 7), pf, o[db]);
        }
      }
    }

    if (more) {                                 // V(t + 1) into the buffer that tile t - 1 was read from
#pragma unroll
      for (int i = 0; i < VPT; ++i) {
        const int idx = i * 256 + tid, r = idx / PPR, pc = idx - r * PPR;
        bf16* dst = &Vs[buf ^ 1][r * VP + pc * EPP];
        if constexpr (FP8) {
          *reinterpret_cast<bf16x8*>(dst) = codes_bf16(vr[i].x, vr[i].y);
          *reinterpret_cast<bf16x8*>(dst + 8) = codes_bf16(vr[i].z, vr[i].w);
        } else {
          *reinterpret_cast<uint4*>(dst) = vr[i];
        }
      }
    }
    __syncthreads();
  }

  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
  if constexpr (!KS) {
    if (active && row < R) {
#pragma unroll
      for (int db = 0; db < NDB; ++db) finish<D>(a, split, b, hk, row, 16 * db + 4 * kq, m, l, o[db], kq == 0 && db == 0);
    }
  } else {
    // the merge of the four waves' partials, in wave order (every read of V's buffers is behind the barrier)
    float* so = reinterpret_cast<float*>(&Vs[0][0]);        // [4][16][D]
#pragma unroll
    for (int db = 0; db < NDB; ++db)
      *reinterpret_cast<f32x4*>(so + ((size_t)(wave * kSlab + col)) * D + 16 * db + 4 * kq) = o[db];
    if (kq == 0) {
      sm[wave][col] = m;
      sl[wave][col] = l;
    }
    __syncthreads();
    for (int u = tid; u < kSlab * (D / 4); u += 256) {
      const int r = u / (D / 4), d = 4 * (u - r * (D / 4));
      if (row0 + r >= R) continue;
      float M = -INFINITY;
#pragma unroll
      for (int w = 0; w < 4; ++w) M = fmaxf(M, sm[w][r]);
      const float Ms = M == -INFINITY ? 0.f : M;
      float L = 0.f;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const float wt = fexp2(sm[w][r] - Ms);
        const f32x4 ow = *reinterpret_cast<const f32x4*>(so + ((size_t)(w * kSlab + r)) * D + d);
        L += wt * sl[w][r];
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] += wt * ow[e];
      }
      finish<D>(a, split, b, hk, row0 + r, d, M, L, acc, d == 0);
    }
  }
}

template <int D, bool FP8>
void launch_extend(bool ks, dim3 grid, hipStream_t s, const ExtendArgs& a) {
  if (ks) hipLaunchKernelGGL((extend_kernel<D, FP8, true>), grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL((extend_kernel<D, FP8, false>), grid, dim3(256), 0, s, a);
}

template <int D>
void launch_both(bool fp8, const ExtendArgs& a, hipStream_t s) {
  const int R = a.T * a.G;
  const bool ks = R <= kSlab;                   // the arrangement rule (file header)
  const int wgr = ks ? kSlab : 4 * kSlab;
  const dim3 grid((unsigned)((R + wgr - 1) / wgr) * a.splits, a.Hkv, a.B);
  if (fp8) launch_extend<D, true>(ks, grid, s, a);
  else launch_extend<D, false>(ks, grid, s, a);
  if (a.splits > 1)
    hipLaunchKernelGGL((decode_combine_kernel<D>), dim3(a.H, a.B * a.T), dim3(D), 0, s, a.ws, a.splits, a.B * a.T, a.H,
                       a.ctx, a.ldo, a.lse);
}

int launch(bool fp8, const void* q, long ldq, const void* k, const void* v, const float* k_scale, const float* v_scale,
           const int* kv_len, const int* kv_start, void* ctx, long ldo, float* lse, float* ws, long ws_floats, int B,
           int T, int H, int Hkv, int D, int Smax, int window, float scale, int splits, hipStream_t s) {
  if (B <= 0 || T <= 0 || H <= 0) return 0;
  if (!q || !k || !v || !kv_len || !ctx || !lse) return (int)hipErrorInvalidValue;
  if (fp8 && (!k_scale || !v_scale || ((uintptr_t)k_scale | (uintptr_t)v_scale) % 4)) return (int)hipErrorInvalidValue;
  if (Hkv <= 0 || H % Hkv || H / Hkv > kMaxGroup) return (int)hipErrorInvalidValue;
  if (D != 64 && D != 128) return (int)hipErrorInvalidValue;
  if (ldq % 8 || ldq < (long)H * D || ldo % 4 || ldo < (long)H * D) return (int)hipErrorInvalidValue;
  if (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v) % 16 || (uintptr_t)ctx % 8) return (int)hipErrorInvalidValue;
  if (Smax <= 0 || window < 0 || splits < 1 || B > 65535 || Hkv > 65535) return (int)hipErrorInvalidValue;
  if ((long long)T * (H / Hkv) > (1 << 24)) return (int)hipErrorInvalidValue;
  const int tiles = (Smax + kKeyTile - 1) / kKeyTile;
  if (splits > tiles) splits = tiles;
  if (splits > 1) {     // the combine kernel's grid is (H, B*T)
    if (!ws || (uintptr_t)ws % 8 || (long long)B * T > 65535) return (int)hipErrorInvalidValue;
    if (ws_floats < (long long)splits * B * T * H * (D + 2)) return (int)hipErrorInvalidValue;
  }
  ExtendArgs a;
  a.q = (const bf16*)q; a.k = k; a.v = v;
  a.ks = fp8 ? k_scale : nullptr; a.vs = fp8 ? v_scale : nullptr;
  a.kv_len = kv_len; a.kv_start = kv_start;
  a.ctx = (bf16*)ctx; a.lse = lse; a.ws = ws; a.ldq = ldq; a.ldo = ldo;
  a.B = B; a.T = T; a.H = H; a.Hkv = Hkv; a.G = H / Hkv; a.Smax = Smax; a.window = window;
  a.kps = kKeyTile * ((tiles + splits - 1) / splits);
  a.splits = splits;
  a.scale2 = scale * kLog2e;
  if (D == 64) launch_both<64>(fp8, a, s);
  else launch_both<128>(fp8, a, s);
  DTD_LAUNCH_CHECK();
}

}  // namespace

// q: the chunk's packed projection [B*T, ...] with row stride ldq (elements), only its q block is read; ctx
// [B*T, H*D] with row stride ldo; lse [B*T, H].  ws: fp32 workspace of ws_floats >= splits * B*T * H * (D + 2)
// floats, not touched (and may be null) when splits == 1.  splits beyond the number of key tiles are cut to it;
// splits > 1 needs B*T <= 65535.
DTD_EXPORT int dtd_attn_extend(const void* q, long ldq, const void* k, const void* v, const int* kv_len,
                               const int* kv_start, void* ctx, long ldo, float* lse, float* ws, long ws_floats, int B,
                               int T, int H, int Hkv, int D, int Smax, int window, float scale, int splits,
                               hipStream_t s) {
  return launch(false, q, ldq, k, v, nullptr, nullptr, kv_len, kv_start, ctx, ldo, lse, ws, ws_floats, B, T, H, Hkv, D,
                Smax, window, scale, splits, s);
}

// dtd_attn_extend on the FP8 cache: k, v e4m3 codes, k_scale, v_scale fp32 [B, Hkv, Smax]; q / ctx bf16.
DTD_EXPORT int dtd_attn_extend_fp8(const void* q, long ldq, const void* k, const void* v, const float* k_scale,
                                   const float* v_scale, const int* kv_len, const int* kv_start, void* ctx, long ldo,
                                   float* lse, float* ws, long ws_floats, int B, int T, int H, int Hkv, int D, int Smax,
                                   int window, float scale, int splits, hipStream_t s) {
  return launch(true, q, ldq, k, v, k_scale, v_scale, kv_len, kv_start, ctx, ldo, lse, ws, ws_floats, B, T, H, Hkv, D,
                Smax, window, scale, splits, s);
}
