// FP8 x FP8 GEMM for the prompt pass, and the kernel that puts activations on the FP8 grid.
//
//   Y[m, n] = bf16((acc * sx[m]) * sw[n]),   acc = sum_k float(xc[m, k]) * float(wc[n, k])   in fp32
//
// xc [M, K] and wc [N, K] are OCP e4m3fn codes, K-contiguous; sx [M] and sw [N] are arbitrary positive fp32
// scales (ops/quant.py gives powers of two, the kernel does not assume it).  The codes are multiplied exactly
// by v_mfma_scale_f32_16x16x128_f8f6f4 with format selectors 0 / 0 (e4m3 both sides) and unit block scales
// (0x7f); the only rounding is the bf16 store.  This is the product for more than 64 rows: the prompt, a chunk
// of it, a large batch -- compute-bound, where gemm_skinny.hip (M <= 64) is weight streaming.
//
// Design (what differs from gemm_w4.hip's 256 x 256 bf16 frame, and why):
// * Tile and wave split.  256 threads, waves 2 (M) x 2 (N), a wave owning TM x TN MFMA tiles of 16 x 16:
//   a workgroup tile is BM x BN = 32 TM x 32 TN.  A K-step is 128 codes = 128 bytes per row, the same LDS
//   row as gemm_w4's 64 bf16 -- but one MFMA now consumes the whole row, so a K-step is TM TN MFMAs (8 passes
//   each) against 2 (TM + TN) ds_read_b128: per MFMA a quarter of gemm_w4's issue slots for the same bytes.
//   LDS reads per MFMA are (TM + TN) / (TM TN) fragments: 1/2 at 4 x 4, 3/8 at 8 x 4, 1 at 2 x 2.  Three
//   instantiations, chosen by the shape alone (and the CU count):
//       256 x 128 (TM 8, TN 4): 32 MFMAs against 24 reads and 12 DMA pieces a wave and K-step; 128 fp32
//                               accumulators, three stages of 48 KiB -- the largest tile whose three-stage ring
//                               fits the 160 KiB of LDS (256 x 256 would leave two stages: nothing in flight
//                               while a stage is drained);
//       128 x 128 (TM 4, TN 4): 16 MFMAs, 16 reads, 8 pieces; 3 x 32 KiB;
//        64 x  64 (TM 2, TN 2):  4 MFMAs,  8 reads, 4 pieces; 3 x 16 KiB, three workgroups a CU -- the tile of
//                               64 < M <= 256: a 96-row chunk runs two row tiles of 64, not a quarter of 256,
//                               and a 2048-column projection still gives 64 workgroups.
//   The host takes the largest tile that still gives every CU a workgroup and pads M by at most a quarter.
// * Operand mapping.  W is the MFMA's row operand, X its column operand.  The sum over k is order-free and
//   both operands go through the same lane mapping, so the 32 codes of lane (q, i) = (lane / 16, lane % 16)
//   are chosen for the loads: the 16-byte chunks q and 4 + q of row i's 128 bytes, two ds_read_b128.  The
//   chunk index is XORed with (row & 7) in LDS (gemm_w4's swizzle: reads and DMA writes conflict-free).
// * Movement into LDS: LDS-DMA (buffer_load_dwordx4 ... lds), one piece = 8 rows x 128 bytes per wave
//   instruction, the swizzle carried by the source address.  A ring of three stages: at K-step s a wave waits
//   for its own pieces of s (vmcnt counted: the pieces of s + 1 stay in flight), ONE barrier (every wave's
//   pieces of s have landed, and every wave has finished reading stage s - 1), then the pieces of s + 2 are
//   issued into the stage s - 1 used, then the MFMAs of s.  Source rows are clamped into the operand (a row at
//   or above M reads row M - 1, a column at or above N reads row N - 1 of W): every load is unconditional and
//   in bounds, for the reason gemm_skinny.hip gives; what those rows produce is never stored.
// * Epilogue.  LDS row l of the W image holds weight row sigma(l) (below), so that after the MFMAs lane (q, j)
//   holds, for a pair of tiles, the 8 consecutive columns 32 jp + 8 q .. + 7 of row j: 16-byte stores straight
//   from the accumulators, a wave instruction covering 16 rows x 64 contiguous bytes.  sx for the lane's TM
//   rows and sw for its 4 TN columns are fetched once per tile.
// * Order of the sum: one workgroup per output tile walks K front to back, no K split, no atomics: two calls
//   are bitwise equal.
// * Resources: profiles/gemm_fp8_resources.md (no scratch in any instantiation).
//
// Supported: M >= 1, N % 16 == 0, K % 128 == 0, 16-byte aligned rows (dtd_gemm_fp8_supported checks the sizes,
// the launcher the rest).
//
// dtd_act_quant_fp8: bf16 x [M, K] -> codes [M, K] and scale [M] by ops/quant.py's law (amax over the row;
// the smallest power of two s with amax / s <= 448, 1 for a zero row, at least 2^-100; code = e4m3fn(x / s),
// round to nearest even).  One pass over x: TPR lanes share a row (16, 64 or 256: K <= 1024, 4096, 16384)
// and keep their up to 8 16-byte vectors in registers between the amax and the conversion; the exponent comes
// from the fp32 bits of amax (frexp by integer arithmetic), x / s is a multiplication by 2^-k, exact;
// v_cvt_pk_fp8_f32 converts, 8-byte stores.  A longer row is read twice.  No atomics; rows at and above M are
// neither read nor written.
#include <stdlib.h>

#include "common.h"

using namespace dtd;

namespace {

typedef int i32x8 __attribute__((ext_vector_type(8)));

constexpr int kStep = 128;          // codes (and bytes) per row and K-step: one MFMA deep
constexpr int kRing = 3;            // LDS stages
constexpr int kTileM[3] = {64, 128, 256};

struct Fp8Args {
  const uint8_t* x; const uint8_t* w;
  const float* sx; const float* sw;
  bf16* y;
  int M, N, K, ldx, ldw, ldy;       // leading dimensions in elements
};

template <int N>
__device__ __forceinline__ void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" :: "n"(N) : "memory"); }
__device__ __forceinline__ void barrier() { asm volatile("s_barrier" ::: "memory"); }

__device__ __forceinline__ __amdgpu_buffer_rsrc_t rsrc(const void* p, long bytes) {
  const uint64_t a = (uint64_t)p;
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)a);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32));
  const int n = __builtin_amdgcn_readfirstlane((int)(bytes < 0x7fffffffL ? bytes : 0x7fffffffL));
  return __builtin_amdgcn_make_buffer_rsrc((void*)(((uint64_t)hi << 32) | lo), (short)0, n, 0x00020000);
}

// LDS row l of the W image holds weight row sigma(l) of the tile: l = 32 jp + 16 t + i (tile pair jp, tile t of
// the pair, lane row i) -> 32 jp + 8 (i >> 2) + 4 t + (i & 3), so the accumulators of tiles 2 jp and 2 jp + 1
// give lane quad q the columns 32 jp + 8 q + 0 .. 7.  For DMA piece p (LDS rows 8 p .. 8 p + 7, lane row d):
__device__ __forceinline__ int sigma_piece(int p, int d) {
  return 32 * (p >> 2) + 16 * (p & 1) + 4 * ((p >> 1) & 1) + 8 * (d >> 2) + (d & 3);
}

// the 32 codes of a lane: chunks q and 4 + q of its row (the addresses carry the swizzle)
__device__ __forceinline__ i32x8 frag(const char* lo, const char* hi) {
  const uint4 a = *reinterpret_cast<const uint4*>(lo);
  const uint4 b = *reinterpret_cast<const uint4*>(hi);
  i32x8 r;
  r[0] = (int)a.x; r[1] = (int)a.y; r[2] = (int)a.z; r[3] = (int)a.w;
  r[4] = (int)b.x; r[5] = (int)b.y; r[6] = (int)b.z; r[7] = (int)b.w;
  return r;
}

template <int TM, int TN>
__global__ void __launch_bounds__(256) gemm_fp8_kernel(const Fp8Args g) {
  static_assert(TN % 2 == 0 && TM % 2 == 0, "the epilogue stores pairs of W tiles");
  constexpr int BM = 32 * TM, BN = 32 * TN;
  constexpr int STAGE = (BM + BN) * kStep;          // X image [BM][128 B], then W image [BN][128 B]
  constexpr int PX = BM / 32, PW = BN / 32;         // DMA pieces per wave and K-step
  static_assert(kRing * STAGE <= 160 * 1024, "the ring must fit the LDS");
  __shared__ __attribute__((aligned(1024))) char smem[kRing * STAGE];

  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = w >> 1, wn = w & 1;
  const int q = lane >> 4, i = lane & 15;
  const int ntm = (g.M + BM - 1) / BM;
  const int m0 = (blockIdx.x % ntm) * BM, n0 = (blockIdx.x / ntm) * BN;   // row tiles fastest: a W panel is shared
  const int nk = g.K / kStep;

  // ---- DMA side: this lane's source offsets of the wave's pieces (rows clamped into the operand)
  const int d = lane >> 3, sc = ((lane & 7) ^ d) * 16;
  const int mlast = g.M - 1 - m0, nlast = g.N - 1 - n0;
  int vx[PX], vw[PW];
#pragma unroll
  for (int k = 0; k < PX; ++k) {
    const int r = 8 * (w * PX + k) + d;
    vx[k] = (r < mlast ? r : mlast) * g.ldx + sc;
  }
#pragma unroll
  for (int k = 0; k < PW; ++k) {
    const int r = sigma_piece(w * PW + k, d);
    vw[k] = (r < nlast ? r : nlast) * g.ldw + sc;
  }
  const auto rx = rsrc(g.x + (size_t)m0 * g.ldx, (long)mlast * g.ldx + g.K);
  const auto rw = rsrc(g.w + (size_t)n0 * g.ldw, (long)nlast * g.ldw + g.K);
  const uint32_t lds0 = lds_addr(smem);
  auto issue = [&](int ks, int stage) {
    const uint32_t base = lds0 + stage * STAGE;
#pragma unroll
    for (int k = 0; k < PX; ++k) dma16(rx, base + (w * PX + k) * 1024, vx[k], ks * kStep);
#pragma unroll
    for (int k = 0; k < PW; ++k) dma16(rw, base + BM * kStep + (w * PW + k) * 1024, vw[k], ks * kStep);
  };

  // ---- MFMA side: this lane's two chunk addresses in row i of a tile
  const int c0 = (q ^ (i & 7)) * 16, c1 = ((4 + q) ^ (i & 7)) * 16;
  const int xrow = (wm * 16 * TM + i) * kStep, wrow = BM * kStep + (wn * 16 * TN + i) * kStep;

  f32x4 acc[TM][TN];
#pragma unroll
  for (int mi = 0; mi < TM; ++mi)
#pragma unroll
    for (int ni = 0; ni < TN; ++ni) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};

  issue(0, 0);
  if (nk > 1) issue(1, 1);
  int stage = 0;
  for (int ks = 0; ks < nk; ++ks) {
    if (ks + 1 < nk) wait_vm<PX + PW>(); else wait_vm<0>();     // (wave-uniform)
    barrier();
    if (ks + 2 < nk) issue(ks + 2, stage == 0 ? 2 : stage - 1);
    const char* buf = smem + stage * STAGE;
    i32x8 wf[TN];
#pragma unroll
    for (int ni = 0; ni < TN; ++ni) wf[ni] = frag(buf + wrow + ni * 16 * kStep + c0, buf + wrow + ni * 16 * kStep + c1);
#pragma unroll
    for (int mi = 0; mi < TM; ++mi) {
      const i32x8 xf = frag(buf + xrow + mi * 16 * kStep + c0, buf + xrow + mi * 16 * kStep + c1);
#pragma unroll
      for (int ni = 0; ni < TN; ++ni)
        acc[mi][ni] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wf[ni], xf, acc[mi][ni], 0, 0, 0, 0x7f7f7f7f, 0,
                                                                       0x7f7f7f7f);
    }
    stage = stage == kRing - 1 ? 0 : stage + 1;
  }

  // ---- epilogue: lane (q, j = i) holds row 16 mi + j, columns 32 jp + 8 q + 4 t + r of tiles 2 jp + t
  float sw[TN / 2][8];
#pragma unroll
  for (int jp = 0; jp < TN / 2; ++jp) {
    int n = n0 + wn * 16 * TN + 32 * jp + 8 * q;
    n = n < g.N - 8 ? n : g.N - 8;
    const float4 a = *reinterpret_cast<const float4*>(g.sw + n), b = *reinterpret_cast<const float4*>(g.sw + n + 4);
    sw[jp][0] = a.x; sw[jp][1] = a.y; sw[jp][2] = a.z; sw[jp][3] = a.w;
    sw[jp][4] = b.x; sw[jp][5] = b.y; sw[jp][6] = b.z; sw[jp][7] = b.w;
  }
  float sxs[TM];
#pragma unroll
  for (int mi = 0; mi < TM; ++mi) {
    const int m = m0 + wm * 16 * TM + 16 * mi + i;
    sxs[mi] = g.sx[m < g.M ? m : g.M - 1];
  }
#pragma unroll
  for (int mi = 0; mi < TM; ++mi) {
    const int m = m0 + wm * 16 * TM + 16 * mi + i;
    const float sx = sxs[mi];
#pragma unroll
    for (int jp = 0; jp < TN / 2; ++jp) {
      const int n = n0 + wn * 16 * TN + 32 * jp + 8 * q;
      bf16x8 o;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) o[4 * t + r] = (bf16)((acc[mi][2 * jp + t][r] * sx) * sw[jp][4 * t + r]);
      if (m < g.M && n < g.N) *reinterpret_cast<bf16x8*>(g.y + (size_t)m * g.ldy + n) = o;
    }
  }
}

int cu_count() {
  static int cus = 0;
  if (!cus) {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        n <= 0)
      n = 256;
    cus = n;
  }
  return cus;
}

// The M edge of the tile a shape runs on: a function of the shape (and the CU count) only.  The largest tile
// that gives every CU a workgroup and pads M by at most a quarter; the smallest when none does.
int pick_tile_m(int M, int N) {
  static const int forced = [] {
    const char* e = getenv("DTD_GEMM_FP8_TILE");
    return e ? atoi(e) : 0;
  }();
  if (forced == 64 || forced == 128 || forced == 256) return forced;
  for (int bm : {256, 128}) {
    const int bn = 128;
    const long tm = (M + bm - 1) / bm, tn = (N + bn - 1) / bn;
    if (tm * tn >= cu_count() && tm * bm * 4 <= 5L * M) return bm;
  }
  return 64;
}

template <int TM, int TN>
void launch(const Fp8Args& a, hipStream_t st) {
  const long tiles = (long)((a.M + 32 * TM - 1) / (32 * TM)) * ((a.N + 32 * TN - 1) / (32 * TN));
  hipLaunchKernelGGL((gemm_fp8_kernel<TM, TN>), dim3((unsigned)tiles), dim3(256), 0, st, a);
}

// ------------------------------------------------------------------------------------------ the quantiser
struct QuantArgs {
  const bf16* x; uint8_t* codes; float* scale;
  size_t ldx, ldc;
  int M, K;
};

// amax (>= 0, finite) -> k of the law: amax = m 2^e, m in [0.5, 1); k = e - 9 when m <= 0.875 (448 = 0.875 * 2^9),
// e - 8 otherwise; at least -100; 0 for a zero row.  A subnormal amax has e <= -126: the clamp.
__device__ __forceinline__ int scale_exponent(float amax) {
  const uint32_t u = __float_as_uint(amax);
  const int e = (int)(u >> 23) - 126;
  int k = (u & 0x7fffffu) <= 0x600000u ? e - 9 : e - 8;
  k = k < -100 ? -100 : k;
  return u == 0 ? 0 : k;
}
__device__ __forceinline__ float pow2(int k) { return __uint_as_float((uint32_t)(k + 127) << 23); }

__device__ __forceinline__ uint2 to_codes(const bf16x8& v, float inv) {
  int lo = 0, hi = 0;
  lo = __builtin_amdgcn_cvt_pk_fp8_f32((float)v[0] * inv, (float)v[1] * inv, lo, false);
  lo = __builtin_amdgcn_cvt_pk_fp8_f32((float)v[2] * inv, (float)v[3] * inv, lo, true);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32((float)v[4] * inv, (float)v[5] * inv, hi, false);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32((float)v[6] * inv, (float)v[7] * inv, hi, true);
  return make_uint2((uint32_t)lo, (uint32_t)hi);
}

__device__ __forceinline__ float amax8(const bf16x8& v, float a) {
#pragma unroll
  for (int e = 0; e < 8; ++e) a = fmaxf(a, fabsf((float)v[e]));
  return a;
}

// max over the TPR lanes of a row (TPR = 256: the workgroup, through LDS)
template <int TPR>
__device__ __forceinline__ float row_max(float a, float* sh) {
#pragma unroll
  for (int o = (TPR < 64 ? TPR : 64) / 2; o > 0; o >>= 1) a = fmaxf(a, __shfl_xor(a, o, 64));
  if constexpr (TPR == 256) {
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = a;
    __syncthreads();
    a = fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
  }
  return a;
}

// TPR lanes per row, 256 / TPR rows per workgroup, V vectors of 8 elements per lane (vector t + TPR v).
// V = 0: a row longer than 8 vectors per lane, read twice.
template <int TPR, int V>
__global__ void __launch_bounds__(256) act_quant_fp8_kernel(const QuantArgs a) {
  __shared__ float sh[4];
  const int t = threadIdx.x % TPR;
  const int row = blockIdx.x * (256 / TPR) + threadIdx.x / TPR;
  if (row >= a.M) return;                          // (TPR = 256: the whole workgroup; no barrier otherwise)
  const int nvec = a.K / 8;
  const bf16* x = a.x + (size_t)row * a.ldx;
  uint8_t* c = a.codes + (size_t)row * a.ldc;
  float amax = 0.f;
  if constexpr (V > 0) {
    bf16x8 v[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {                  // unconditional loads, clamped into the row
      const int idx = t + TPR * j;
      v[j] = *reinterpret_cast<const bf16x8*>(x + 8 * (idx < nvec ? idx : nvec - 1));
    }
#pragma unroll
    for (int j = 0; j < V; ++j) amax = amax8(v[j], amax);   // (a clamped vector is the row's own data)
    amax = row_max<TPR>(amax, sh);
    const int k = scale_exponent(amax);
    const float inv = pow2(-k);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const int idx = t + TPR * j;
      if (idx < nvec) *reinterpret_cast<uint2*>(c + 8 * idx) = to_codes(v[j], inv);
    }
    if (t == 0) a.scale[row] = pow2(k);
  } else {
    for (int idx = t; idx < nvec; idx += TPR) amax = amax8(*reinterpret_cast<const bf16x8*>(x + 8 * idx), amax);
    amax = row_max<TPR>(amax, sh);
    const int k = scale_exponent(amax);
    const float inv = pow2(-k);
    for (int idx = t; idx < nvec; idx += TPR)
      *reinterpret_cast<uint2*>(c + 8 * idx) = to_codes(*reinterpret_cast<const bf16x8*>(x + 8 * idx), inv);
    if (t == 0) a.scale[row] = pow2(k);
  }
}

template <int TPR>
void launch_quant(int vecs, const QuantArgs& a, hipStream_t st) {
  const dim3 grid((a.M + 256 / TPR - 1) / (256 / TPR));
  if (vecs <= 1) hipLaunchKernelGGL((act_quant_fp8_kernel<TPR, 1>), grid, dim3(256), 0, st, a);
  else if (vecs <= 2) hipLaunchKernelGGL((act_quant_fp8_kernel<TPR, 2>), grid, dim3(256), 0, st, a);
  else if (vecs <= 4) hipLaunchKernelGGL((act_quant_fp8_kernel<TPR, 4>), grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL((act_quant_fp8_kernel<TPR, 8>), grid, dim3(256), 0, st, a);
}

}  // namespace

DTD_EXPORT int dtd_gemm_fp8_supported(int M, int N, int K) {
  return M >= 1 && N > 0 && N % 16 == 0 && K > 0 && K % kStep == 0;
}

// The M edges of the kernel's tiles, smallest first (idx 0 .. 2); -1 past the last.
DTD_EXPORT int dtd_gemm_fp8_tile_m(int idx) { return idx >= 0 && idx < 3 ? kTileM[idx] : -1; }

// x [M, K], w [N, K]: e4m3fn codes; sx [M], sw [N] fp32; y [M, N] bf16.  ldx, ldw, ldy: row strides in elements.
// tile_m: 0 = the shape's own tile, or one of dtd_gemm_fp8_tile_m's (tests, tuning runs).
DTD_EXPORT int dtd_gemm_fp8(const void* x, int ldx, const float* sx, const void* w, int ldw, const float* sw, void* y,
                            int ldy, int M, int N, int K, int tile_m, hipStream_t s) {
  if (!dtd_gemm_fp8_supported(M, N, K)) return (int)hipErrorInvalidValue;
  if (!x || !w || !y || !sx || !sw || ((uintptr_t)x | (uintptr_t)w | (uintptr_t)y | (uintptr_t)sw) % 16 || (uintptr_t)sx % 4)
    return (int)hipErrorInvalidValue;
  // (a tile's source offsets are 32-bit: 256 rows of at most 2^22 bytes)
  if (ldx < K || ldx % 16 || ldw < K || ldw % 16 || ldy < N || ldy % 8 || ldx > (1 << 22) || ldw > (1 << 22))
    return (int)hipErrorInvalidValue;
  Fp8Args a;
  a.x = (const uint8_t*)x; a.w = (const uint8_t*)w; a.sx = sx; a.sw = sw; a.y = (bf16*)y;
  a.M = M; a.N = N; a.K = K; a.ldx = ldx; a.ldw = ldw; a.ldy = ldy;
  const int bm = tile_m ? tile_m : pick_tile_m(M, N);
  if (bm == 256) launch<8, 4>(a, s);
  else if (bm == 128) launch<4, 4>(a, s);
  else if (bm == 64) launch<2, 2>(a, s);
  else return (int)hipErrorInvalidValue;
  DTD_LAUNCH_CHECK();
}

// x bf16 [M, K] -> codes e4m3fn [M, K], scale fp32 [M].  ldx, ldc: row strides in elements.
DTD_EXPORT int dtd_act_quant_fp8(const void* x, int ldx, void* codes, int ldc, float* scale, int M, int K, hipStream_t s) {
  if (M < 1 || K < kStep || K % kStep) return (int)hipErrorInvalidValue;
  if (!x || !codes || !scale || (uintptr_t)x % 16 || (uintptr_t)codes % 8 || (uintptr_t)scale % 4) return (int)hipErrorInvalidValue;
  if (ldx < K || ldx % 8 || ldc < K || ldc % 8) return (int)hipErrorInvalidValue;
  QuantArgs a;
  a.x = (const bf16*)x; a.codes = (uint8_t*)codes; a.scale = scale;
  a.ldx = (size_t)ldx; a.ldc = (size_t)ldc; a.M = M; a.K = K;
  const int nvec = K / 8;
  if (nvec <= 16 * 8) launch_quant<16>((nvec + 15) / 16, a, s);
  else if (nvec <= 64 * 8) launch_quant<64>((nvec + 63) / 64, a, s);
  else if (nvec <= 256 * 8) launch_quant<256>((nvec + 255) / 256, a, s);
  else hipLaunchKernelGGL((act_quant_fp8_kernel<256, 0>), dim3(M), dim3(256), 0, s, a);
  DTD_LAUNCH_CHECK();
}
