// Device helpers shared by the KV-cache kernels of the linear cache (attention_decode.hip) and of the ring
// cache (attention_ring.hip): the DPP row reductions, the rotation of one element pair, the FP8 cache's row
// quantisation, the packed-bf16 dot product, and the split kernels' argument block.
#pragma once
#include "common.h"

namespace {

constexpr int kKeyTile = 64;
constexpr int kMaxGroup = 8;
constexpr float kLog2e = 1.4426950408889634f;

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

// The rotation of one element pair (a, b) by (c, sn).  rope.hip writes a * c - b * sn and b * c + a * sn
// and its compiled form contracts the first product of each: spelled out here, so that the kernels
// round alike whatever the vectoriser makes of the loops around it.
__device__ __forceinline__ void rope_rotate(float a, float b, float c, float sn, float& oa, float& ob) {
  oa = __builtin_fmaf(a, c, -(b * sn));
  ob = __builtin_fmaf(b, c, a * sn);
}

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

// The partial of a split without a key: (m, l, o) = (-inf, 0, 0) for the G query heads of the group.
template <int D>
__device__ __forceinline__ void write_empty(const DecodeArgs& a, int split, int b, int hk) {
  for (int idx = threadIdx.x; idx < a.G * (D + 2); idx += blockDim.x) {
    const int g = idx / (D + 2), e = idx - g * (D + 2);
    const size_t base = (((size_t)split * a.B + b) * a.H + (size_t)hk * a.G + g) * (D + 2);
    a.ws[base + e] = e == 0 ? -INFINITY : 0.f;
  }
}

// The checks and the grid that the append entry points share (each has its own rule for D, a positive
// multiple of 16 either way, and checks it first).  Smax: the cache's slots.  False: an argument error.
inline bool append_items(const void* qkv, const float* table, const void* kc, const void* vc, const int* kv_len,
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
