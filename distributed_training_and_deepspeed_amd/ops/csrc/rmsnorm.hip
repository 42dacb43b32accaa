// RMSNorm with a fused residual add (forward and backward) for gfx950 -- the normalisation of the
// Llama family (HF LlamaRMSNorm): no mean, no beta.
//
//   forward :  z    = r + y                     (y or r may be absent; z is stored only when both are given)
//              rstd = rsqrt(mean(z^2) + eps)
//              out  = z * rstd * gamma           (all in fp32, rounded once)
//   backward:  g    = (dout + dout2) * gamma,  xhat = z * rstd
//              dz   = rstd * (g - xhat * mean(g * xhat)) + dz_extra
//              column partials of (dout + dout2) * xhat (dgamma), one fp32 row per block, summed in a
//              fixed order by dtd_colsum_finalize (act.hip): bitwise deterministic, no atomics.
//
// Layout: TPR threads share a row, thread t holding the 8-element vectors t, t + TPR, ... of it (16 bytes
// of bf16, 32 of fp32 per access), so the row stays in registers between the reduction and the output.
// TPR = 64 is the wave-per-row form of norm.hip (four rows per block, rows up to 1024 wide); wider rows
// take TPR = 256, a block per row (up to 8192 wide).  h must be a multiple of 8; the grid is capped and
// strides over the rows.
#include "common.h"

using namespace dtd;

namespace {

struct RmsFwdArgs {
  const void* y; const void* r; const void* gamma; void* z; void* out; float* rstd;
  int rows, h; float eps;
};

struct RmsBwdArgs {
  const void* dout; const void* dout2; const void* dz_extra; const void* z; const float* rstd;
  const void* gamma; void* dz; float* part_gamma;
  int rows, h;
};

constexpr int kMaxBlocks = 1024;   // 4 blocks of 4 waves per CU: 4 waves per SIMD on 256 CUs

template <typename T, bool NT> __device__ __forceinline__ void ld8(const T* p, float* o) {
  if constexpr (NT) vload_nt<T, 8>(p, o); else vload<T, 8>(p, o);
}
template <typename T, bool NT> __device__ __forceinline__ void st8(T* p, const float* o) {
  if constexpr (NT) vstore_nt<T, 8>(p, o); else vstore<T, 8>(p, o);
}

// Row group of this thread inside its block.  TPR = 64: the wave index, made provably wave-uniform so
// hipcc keeps the row base in SGPRs (scalar base + 32-bit lane offset, as norm.hip's backward).
template <int TPR> __device__ __forceinline__ int wave_uniform_group() {
  if constexpr (TPR == 64) return __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  else return 0;
}

// sum over the TPR threads of a row
template <int TPR> __device__ __forceinline__ float row_total(float v, float* red) {
  if constexpr (TPR == 64) return wave_sum(v);
  else return block_sum(v, red);
}

template <typename T, int MAXC, int TPR, bool NT>
__global__ void __launch_bounds__(256) rms_fwd_kernel(RmsFwdArgs a) {
  constexpr int RPB = 256 / TPR;
  __shared__ float red[8];
  const int t = threadIdx.x % TPR, grp = wave_uniform_group<TPR>();
  const int h = a.h, nv = h >> 3;
  const bool store_z = a.z != nullptr && a.y != nullptr && a.r != nullptr;
  const T* first = (const T*)(a.y ? a.y : a.r);
  const T* second = (const T*)(a.y && a.r ? a.r : nullptr);
  for (int row0 = blockIdx.x * RPB; row0 < a.rows; row0 += gridDim.x * RPB) {
    const int row = row0 + grp;          // uniform per wave (TPR = 64) or per block (TPR = 256)
    if (row >= a.rows) continue;         // TPR = 64 only: no block barrier in that form
    const size_t base = (size_t)row * h;
    float z[MAXC * 8];
    float ss = 0.f;
    // (predicated vector rounds: measured 1-2 % ahead of the backward's branch-free clamped loads
    // here, where a round's loads feed only a sum and the z store)
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
      const int v = c * TPR + t;
      if (v < nv) {
        const int col = v << 3;
        float x[8];
        ld8<T, NT>(first + base + col, x);
        if (second) {
          float rr[8];
          ld8<T, NT>(second + base + col, rr);
#pragma unroll
          for (int j = 0; j < 8; ++j) x[j] += rr[j];
        }
        if (store_z) st8<T, NT>((T*)a.z + base + col, x);
#pragma unroll
        for (int j = 0; j < 8; ++j) { z[c * 8 + j] = x[j]; ss += x[j] * x[j]; }
      }
    }
    const float rs = rsqrtf(row_total<TPR>(ss, red) / h + a.eps);
    if (t == 0) a.rstd[row] = rs;
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
      const int v = c * TPR + t;
      if (v < nv) {
        const int col = v << 3;
        float gm[8], o[8];
        vload<T, 8>((const T*)a.gamma + col, gm);
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = z[c * 8 + j] * rs * gm[j];
        st8<T, NT>((T*)a.out + base + col, o);
      }
    }
  }
}

template <typename T, int MAXC, int TPR, bool NT>
__global__ void __launch_bounds__(256) rms_bwd_kernel(RmsBwdArgs a) {
  constexpr int RPB = 256 / TPR;
  // TPR = 64: the four waves' column partials meet in LDS (rows up to 512 * MAXC wide)
  __shared__ float sh[TPR == 64 ? 4 * 512 * MAXC : 8];
  typedef T raw8 __attribute__((ext_vector_type(8)));
  const int t = threadIdx.x % TPR, grp = wave_uniform_group<TPR>();
  const int h = a.h, nv = h >> 3;
  float pg[MAXC * 8];
#pragma unroll
  for (int i = 0; i < MAXC * 8; ++i) pg[i] = 0.f;
  // a thread owns the same columns in every row: gamma stays packed in registers (0 past the row's end,
  // which also zeroes that thread's g, so its clamped loads below add nothing)
  raw8 gmr[MAXC];
#pragma unroll
  for (int c = 0; c < MAXC; ++c) {
    const int v = c * TPR + t;
    float gm[8];
    vload<T, 8>((const T*)a.gamma + (v < nv ? v << 3 : 0), gm);
#pragma unroll
    for (int j = 0; j < 8; ++j) gmr[c][j] = (T)(v < nv ? gm[j] : 0.f);
  }
  for (int row0 = blockIdx.x * RPB; row0 < a.rows; row0 += gridDim.x * RPB) {
    const int row = row0 + grp;
    if (row >= a.rows) continue;         // TPR = 64 only (see the forward)
    const size_t base = (size_t)row * h;
    const float rs = a.rstd[row];
    float xh[MAXC * 8], g[MAXC * 8];
    float s = 0.f;
    // a thread past the end of the row (the last vector round of h = 768, 5120, ...) reads vector 0 and
    // counts it as zeros: every load of the row is issued without a branch in front of it, so the rounds'
    // round trips overlap (131072 x 768: 130 -> 107 us against predicated rounds)
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
      const bool ok = c * TPR + t < nv;
      const int col = ok ? (c * TPR + t) << 3 : 0;
      float zz[8], d[8];
      ld8<T, NT>((const T*)a.z + base + col, zz);
      ld8<T, NT>((const T*)a.dout + base + col, d);
      if (a.dout2) {
        float e[8];
        ld8<T, NT>((const T*)a.dout2 + base + col, e);
#pragma unroll
        for (int j = 0; j < 8; ++j) d[j] += e[j];
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int i = c * 8 + j;
        xh[i] = ok ? zz[j] * rs : 0.f;
        g[i] = d[j] * (float)gmr[c][j];
        s += g[i] * xh[i];
        pg[i] += d[j] * xh[i];
      }
    }
    const float m = row_total<TPR>(s, sh) / h;
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
      const bool ok = c * TPR + t < nv;
      const int col = ok ? (c * TPR + t) << 3 : 0;
      float dz[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) dz[j] = rs * (g[c * 8 + j] - xh[c * 8 + j] * m);
      if (a.dz_extra) {
        float e[8];
        ld8<T, NT>((const T*)a.dz_extra + base + col, e);
#pragma unroll
        for (int j = 0; j < 8; ++j) dz[j] += e[j];
      }
      if (ok) st8<T, NT>((T*)a.dz + base + col, dz);
    }
  }
  if (!a.part_gamma) return;
  float* out = a.part_gamma + (size_t)blockIdx.x * h;
  if constexpr (TPR == 64) {
    float* mine = sh + grp * (512 * MAXC);
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
      const int v = c * TPR + t;
      if (v < nv) {
#pragma unroll
        for (int j = 0; j < 8; ++j) mine[(v << 3) + j] = pg[c * 8 + j];
      }
    }
    __syncthreads();
    for (int col = threadIdx.x; col < h; col += 256) {
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < RPB; ++i) s += sh[i * (512 * MAXC) + col];
      out[col] = s;
    }
  } else {
    // a thread owns the same columns in every row: its partials are the block's
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
      const int v = c * TPR + t;
      if (v < nv) vstore<float, 8>(out + (v << 3), pg + c * 8);
    }
  }
}

inline bool wave_form(int h) { return h <= 1024; }

template <typename T, int MAXC, int TPR>
void launch(const RmsFwdArgs* f, const RmsBwdArgs* b, int blocks, hipStream_t s) {
  const bool nt = ew_nt_bits() == 3;
  if (f) {
    if (nt) hipLaunchKernelGGL((rms_fwd_kernel<T, MAXC, TPR, true>), dim3(blocks), dim3(256), 0, s, *f);
    else hipLaunchKernelGGL((rms_fwd_kernel<T, MAXC, TPR, false>), dim3(blocks), dim3(256), 0, s, *f);
  } else {
    if (nt) hipLaunchKernelGGL((rms_bwd_kernel<T, MAXC, TPR, true>), dim3(blocks), dim3(256), 0, s, *b);
    else hipLaunchKernelGGL((rms_bwd_kernel<T, MAXC, TPR, false>), dim3(blocks), dim3(256), 0, s, *b);
  }
}

template <typename T>
void dispatch(const RmsFwdArgs* f, const RmsBwdArgs* b, int blocks, hipStream_t s) {
  const int h = f ? f->h : b->h;
  // a row up to 1024 wide fits a wave at 4 waves per SIMD (the backward holds x-hat, g and the dgamma
  // partials: 3 x 8 x MAXC registers per lane, 114 VGPRs at MAXC = 2, about 200 at MAXC = 4); wider rows
  // are spread over a block
  if (h <= 512) launch<T, 1, 64>(f, b, blocks, s);
  else if (h <= 1024) launch<T, 2, 64>(f, b, blocks, s);
  else if (h <= 2048) launch<T, 1, 256>(f, b, blocks, s);
  else if (h <= 4096) launch<T, 2, 256>(f, b, blocks, s);
  else launch<T, 4, 256>(f, b, blocks, s);
}

inline int num_blocks(int rows, int h, int cap) {
  const int rpb = wave_form(h) ? 4 : 1;
  const int n = (rows + rpb - 1) / rpb;
  return n < cap ? n : cap;
}

}  // namespace

// 1 when the kernels take a row width (a multiple of 8, at most 8192)
DTD_EXPORT int dtd_rms_supported(int h) { return h > 0 && h % 8 == 0 && h <= 8192; }

// Number of partial rows the backward writes (callers size pgamma as [n, h] fp32).
DTD_EXPORT int dtd_rms_bwd_num_partials(int rows, int h) { return num_blocks(rows, h, kMaxBlocks); }

DTD_EXPORT int dtd_rms_fwd(int dtype, const void* y, const void* r, const void* gamma, void* z, void* out,
                           float* rstd, int rows, int h, float eps, hipStream_t s) {
  if (rows <= 0) return 0;
  if (!dtd_rms_supported(h) || (y == nullptr && r == nullptr)) return (int)hipErrorInvalidValue;
  RmsFwdArgs a{y, r, gamma, z, out, rstd, rows, h, eps};
  const int blocks = num_blocks(rows, h, 2 * kMaxBlocks);
  if (dtype == kBF16) dispatch<bf16>(&a, nullptr, blocks, s);
  else dispatch<float>(&a, nullptr, blocks, s);
  DTD_LAUNCH_CHECK();
}

DTD_EXPORT int dtd_rms_bwd(int dtype, const void* dout, const void* dout2, const void* dz_extra, const void* z,
                           const float* rstd, const void* gamma, void* dz, float* pgamma, int rows, int h,
                           hipStream_t s) {
  if (rows <= 0) return 0;
  if (!dtd_rms_supported(h) || dz == nullptr) return (int)hipErrorInvalidValue;
  RmsBwdArgs a{dout, dout2, dz_extra, z, rstd, gamma, dz, pgamma, rows, h};
  const int blocks = dtd_rms_bwd_num_partials(rows, h);
  if (dtype == kBF16) dispatch<bf16>(nullptr, &a, blocks, s);
  else dispatch<float>(nullptr, &a, blocks, s);
  DTD_LAUNCH_CHECK();
}
