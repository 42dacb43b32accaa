// SwiGLU (the gated MLP activation of the Llama family), forward and backward.
//
// gu [rows, 2f] is the output of the fused gate/up projection: gate in columns [0, f), up in [f, 2f).
//   forward :  a     = silu(gate) * up,  silu(g) = g * sigmoid(g)
//   backward:  dgate = da * up * sigmoid(g) * (1 + g * (1 - sigmoid(g)))
//              dup   = da * silu(g)
//              and, on request, a again in the same pass (the down projection's weight gradient reads
//              it; the layer then keeps no [rows, f] activation between forward and backward).
// No bias, so no column partials.  f must be a multiple of 8: every access is one 16-byte (bf16) /
// 32-byte (fp32) vector per thread, non-temporal like the other streaming passes (common.h); the grid
// is capped and strides over the vectors.  The forward and the backward's recompute share silu_mul,
// so the two a are bitwise equal.
#include "common.h"

using namespace dtd;

namespace {

// sigmoid(g) = 1 / (1 + e^-g): one v_exp and one v_rcp; saturates to 0 / 1 at -+inf
__device__ __forceinline__ float sigmoidf_fast(float g) {
  return __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(g * -1.4426950408889634f));
}
__device__ __forceinline__ float silu_mul(float g, float sg, float u) { return (g * sg) * u; }

template <typename T, bool NT> __device__ __forceinline__ void ld8(const T* p, float* o) {
  if constexpr (NT) vload_nt<T, 8>(p, o); else vload<T, 8>(p, o);
}
template <typename T, bool NT> __device__ __forceinline__ void st8(T* p, const float* o) {
  if constexpr (NT) vstore_nt<T, 8>(p, o); else vstore<T, 8>(p, o);
}

template <typename T, bool NT>
__global__ void __launch_bounds__(256) swiglu_fwd_kernel(const T* __restrict__ gu, T* __restrict__ a, size_t nvec,
                                                         int fv, size_t f) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < nvec; i += (size_t)gridDim.x * blockDim.x) {
    const size_t row = i / fv;
    const size_t col = (i - row * fv) * 8;
    const T* gp = gu + row * 2 * f + col;
    float g[8], u[8], o[8];
    ld8<T, NT>(gp, g);
    ld8<T, NT>(gp + f, u);
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = silu_mul(g[j], sigmoidf_fast(g[j]), u[j]);
    st8<T, NT>(a + row * f + col, o);
  }
}

template <typename T, bool NT>
__global__ void __launch_bounds__(256) swiglu_bwd_kernel(const T* __restrict__ da, const T* __restrict__ gu,
                                                         T* __restrict__ dgu, T* __restrict__ a, size_t nvec, int fv,
                                                         size_t f) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < nvec; i += (size_t)gridDim.x * blockDim.x) {
    const size_t row = i / fv;
    const size_t col = (i - row * fv) * 8;
    const size_t off = row * 2 * f + col;
    float g[8], u[8], d[8], dg[8], du[8], o[8];
    ld8<T, NT>(gu + off, g);
    ld8<T, NT>(gu + off + f, u);
    ld8<T, NT>(da + row * f + col, d);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float sg = sigmoidf_fast(g[j]);
      o[j] = silu_mul(g[j], sg, u[j]);
      dg[j] = d[j] * u[j] * sg * (1.f + g[j] * (1.f - sg));
      du[j] = d[j] * (g[j] * sg);
    }
    st8<T, NT>(dgu + off, dg);
    st8<T, NT>(dgu + off + f, du);
    if (a) st8<T, NT>(a + row * f + col, o);
  }
}

inline int grid_for(size_t nvec) {
  size_t blocks = (nvec + 255) / 256;
  const size_t cap = ew_mode() == 0 ? 4096 : 65536;   // as act.hip: a few vectors per thread at most
  return (int)(blocks < cap ? blocks : cap);
}

}  // namespace

DTD_EXPORT int dtd_swiglu_fwd(int dtype, const void* gu, void* a, int rows, int f, hipStream_t s) {
  if (rows <= 0 || f <= 0) return 0;
  if (f % 8 != 0) return (int)hipErrorInvalidValue;
  const size_t nvec = (size_t)rows * (f / 8);
  const dim3 grid(grid_for(nvec)), block(256);
  const bool nt = ew_nt_bits() == 3;
#define DTD_SWIGLU_FWD(T, N) \
  hipLaunchKernelGGL((swiglu_fwd_kernel<T, N>), grid, block, 0, s, (const T*)gu, (T*)a, nvec, f / 8, (size_t)f)
  if (dtype == kBF16) { if (nt) DTD_SWIGLU_FWD(bf16, true); else DTD_SWIGLU_FWD(bf16, false); }
  else { if (nt) DTD_SWIGLU_FWD(float, true); else DTD_SWIGLU_FWD(float, false); }
#undef DTD_SWIGLU_FWD
  DTD_LAUNCH_CHECK();
}

// a (may be null): also write silu(gate) * up, bitwise the forward's
DTD_EXPORT int dtd_swiglu_bwd(int dtype, const void* da, const void* gu, void* dgu, void* a, int rows, int f,
                              hipStream_t s) {
  if (rows <= 0 || f <= 0) return 0;
  if (f % 8 != 0) return (int)hipErrorInvalidValue;
  const size_t nvec = (size_t)rows * (f / 8);
  const dim3 grid(grid_for(nvec)), block(256);
  const bool nt = ew_nt_bits() == 3;
#define DTD_SWIGLU_BWD(T, N)                                                                                   \
  hipLaunchKernelGGL((swiglu_bwd_kernel<T, N>), grid, block, 0, s, (const T*)da, (const T*)gu, (T*)dgu, (T*)a, \
                     nvec, f / 8, (size_t)f)
  if (dtype == kBF16) { if (nt) DTD_SWIGLU_BWD(bf16, true); else DTD_SWIGLU_BWD(bf16, false); }
  else { if (nt) DTD_SWIGLU_BWD(float, true); else DTD_SWIGLU_BWD(float, false); }
#undef DTD_SWIGLU_BWD
  DTD_LAUNCH_CHECK();
}
