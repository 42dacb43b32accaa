// The merge of split-KV partials, shared by the cached-attention kernels (attention_decode.hip: one query
// token per sequence; attention_extend.hip: T of them).  Each split leaves an fp32 partial (m in log2 units,
// l, o[D]) per (row, head) in ws [splits][rows][H][D + 2]; decode_combine_kernel, grid (H, rows), D threads,
// merges the splits in index order -- no atomics, a fixed summation order -- and writes ctx in the model's
// dtype and lse.  A row whose every split is empty (-inf, 0, 0) gives ctx = 0, lse = -inf.
#pragma once
#include "common.h"

namespace {

constexpr float kLn2 = 0.6931471805599453f;

__device__ __forceinline__ float fexp2(float x) { return __builtin_amdgcn_exp2f(x); }

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

}  // namespace
