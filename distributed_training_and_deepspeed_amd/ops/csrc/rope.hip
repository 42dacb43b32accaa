// Rotary position embedding (HF Llama convention), in place on the q and k slices of the packed qkv.
//
//   for j < D/2, position p:  out[j]       = x[j]       * cos(p t_j) - x[j + D/2] * sin(p t_j)
//                             out[j + D/2] = x[j + D/2] * cos(p t_j) + x[j]       * sin(p t_j)
//
// qkv is [B*S, 3*H*D] with row stride ld: head h of q at column h*D, of k at H*D + h*D (so the 2H
// rotated heads are one contiguous run of 2*H*D columns); v is not touched.  With grouped-query
// attention (Hkv < H key/value heads) a row is [(H + 2*Hkv)*D]: the q block (H*D columns), then k
// (Hkv*D), then v (Hkv*D) -- the rotated run is the first H + Hkv heads (dtd_rope_heads).  cos / sin come from a
// table [max_pos, D/2, 2] fp32 built once per model from float64 angles -- no trigonometry here.
// inverse = 1 negates the sine: the rotation is orthogonal, so that is its inverse and its adjoint
// (the backward applies it to the attention backward's dqkv).  pos: optional int32 position of every
// token (sequence packing: they restart at each document), default row % S; a position is clamped
// into the table, never read outside it.
//
// One thread owns 8 consecutive j of one head: two 16-byte (bf16) vectors x[j..j+8), x[j+D/2..j+D/2+8)
// and the 64 bytes of (cos, sin) pairs between them; nobody else reads or writes those elements, so
// the update is in place.  The grid is capped and strides over the work items.
#include "common.h"

using namespace dtd;

namespace {

template <typename T>
__global__ void __launch_bounds__(256) rope_kernel(T* __restrict__ qkv, const float* __restrict__ table,
                                                   const int* __restrict__ pos, size_t items, int S, int heads2,
                                                   int D, size_t ld, int max_pos, float sgn) {
  const int vph = D >> 4;            // 8-wide vectors per half head
  const int half = D >> 1;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < items; i += (size_t)gridDim.x * blockDim.x) {
    const int v = (int)(i % vph);
    const size_t hr = i / vph;
    const int hd = (int)(hr % heads2);
    const size_t row = hr / heads2;
    int p = pos ? pos[row] : (int)(row % S);
    p = p < 0 ? 0 : (p >= max_pos ? max_pos - 1 : p);
    T* x = qkv + row * ld + (size_t)hd * D + v * 8;
    const float* cs = table + ((size_t)p * half + v * 8) * 2;
    float a[8], b[8], t[16];
    vload<T, 8>(x, a);
    vload<T, 8>(x + half, b);
    vload<float, 16>(cs, t);
    float oa[8], ob[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float c = t[2 * j], sn = sgn * t[2 * j + 1];
      oa[j] = a[j] * c - b[j] * sn;
      ob[j] = b[j] * c + a[j] * sn;
    }
    vstore<T, 8>(x, oa);
    vstore<T, 8>(x + half, ob);
  }
}

}  // namespace

// Rotates the first `heads` heads of every row (row stride ld): heads = H + Hkv of a grouped-query
// qkv, ld = (H + 2*Hkv)*D.
DTD_EXPORT int dtd_rope_heads(int dtype, void* qkv, const float* table, const int* pos, int B, int S, int heads, int D,
                              long ld, int max_pos, int inverse, hipStream_t s) {
  if (B <= 0 || S <= 0 || heads <= 0) return 0;
  // 16-byte vectors: D a multiple of 16, rows a multiple of 8 elements; the rotated heads inside a row
  if (D <= 0 || D % 16 != 0 || ld % 8 != 0 || ld < (long)heads * D || max_pos <= 0 || qkv == nullptr || table == nullptr)
    return (int)hipErrorInvalidValue;
  const size_t items = (size_t)B * S * heads * (D >> 4);
  size_t blocks = (items + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  const float sgn = inverse ? -1.f : 1.f;
  if (dtype == kBF16)
    hipLaunchKernelGGL((rope_kernel<bf16>), dim3(blocks), dim3(256), 0, s, (bf16*)qkv, table, pos, items, S, heads, D,
                       (size_t)ld, max_pos, sgn);
  else
    hipLaunchKernelGGL((rope_kernel<float>), dim3(blocks), dim3(256), 0, s, (float*)qkv, table, pos, items, S, heads, D,
                       (size_t)ld, max_pos, sgn);
  DTD_LAUNCH_CHECK();
}

DTD_EXPORT int dtd_rope(int dtype, void* qkv, const float* table, const int* pos, int B, int S, int H, int D, long ld,
                        int max_pos, int inverse, hipStream_t s) {
  if (H <= 0) return 0;
  return dtd_rope_heads(dtype, qkv, table, pos, B, S, 2 * H, D, ld, max_pos, inverse, s);
}
