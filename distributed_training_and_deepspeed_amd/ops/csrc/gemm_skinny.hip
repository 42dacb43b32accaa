// Skinny GEMM for the decode step's projections: Y[M, N] = X[M, K] . W[N, K]^T with 1 <= M <= 64.
//
// hipcc-flags: -Xclang -target-feature -Xclang -packed-fp32-ops
//
// X and Y are bf16.  W is bf16, or one-byte OCP e4m3fn codes with one fp32 scale per output feature
// (scale[N]): Y[m][n] = bf16(scale[n] * sum_k x[m][k] * float(code[n][k])).  The product is pure weight
// streaming -- every byte of W is used once, X is at most 64 rows -- so the kernel is built around W's
// loads, not around a tile of LDS:
//   * W goes straight from memory into VGPRs in 16-byte loads and is the ROW operand of
//     v_mfma_f32_16x16x32_bf16: a wave owns slabs of 16 output features, lane (q, i) = (lane / 16,
//     lane % 16) holds row i of the slab, and the instruction multiplies 16 n x 32 k of W against
//     32 k x 16 m of X^T.  A bucket of 16 MT columns (MT = 1, 2, 4 for M <= 16, 32, 64) is MT
//     accumulators per slab.  The sum over k is order-free, so which k a lane holds is chosen for the
//     loads: in a K-step of 128, load j of lane (q, i) is the 16 bytes at byte 64 j + 16 q of the row's
//     step -- bf16: 4 loads, elements 32 j + 8 q + e, one MFMA each; codes: 2 loads, codes 64 j + 16 q + e,
//     two MFMAs each (e < 8 and e >= 8) -- so that a load instruction reads 64 contiguous bytes of each
//     of the 16 rows.  The codes are converted in registers (v_cvt_pk_f32_fp8, then the pack to bf16:
//     every e4m3fn value is exact in bf16) and feed the same MFMA; scale[n] multiplies the fp32 sum once,
//     in the epilogue.  Activations are never quantised.
//   * The four waves of a workgroup split K for the SAME S slabs (S = 1, 2 or 4 consecutive slabs per
//     workgroup): wave w takes the K-steps w, w + 4, w + 8, ...  -- four times the loads in flight per
//     slab, which is what a 48-slab projection needs to pull bandwidth.  A wave without a K-step (K =
//     128 has one) keeps zero accumulators.  The next chunk's loads of W (S x 4 KiB of bf16 per wave)
//     are issued before the current chunk's MFMAs.
//   * X is staged in LDS a chunk of 4 K-steps (one per wave) at a time, already in fragment order: the
//     16-byte piece that lane l needs for K-step s, MFMA f, column tile t lies at piece index
//     ((s * 4 + f) * MT + t) * 64 + l, so a fragment read is one ds_read_b128 at consecutive addresses,
//     free of bank conflicts, and the staging writes are consecutive too.  The k permutation of W's
//     loads is applied here, once.  Rows at and above M are never read: their pieces are zeros.  The
//     pieces of chunk c + 1 are loaded into registers before chunk c's MFMAs, ahead of W's loads in
//     issue order, so waiting for them does not drain the weight stream.
//   * The four waves' fp32 partials are summed through LDS (the buffer X used) in wave order, ((p0 + p1)
//     + p2) + p3: no atomics, two calls are bitwise equal.  The accumulator of lane (q, j) holds
//     n = 4 q .. 4 q + 3 of column j: 8 bytes of bf16.  With two column tiles a lane trades one tile's
//     4 values with lane ^ 16 and stores 16 bytes (n = 8 (q / 2) .. + 7 of column 16 (q & 1) + j); the
//     16-column bucket stores its 8 bytes.  Rows at and above M are never stored.
// S depends on the shape alone (and the device's CU count): the largest of 4, 2, 1 that the bucket's
// registers allow (S MT <= 8) and that still gives every CU a workgroup.  The launch sequence of a shape
// is therefore fixed, and a captured decode step replays it.  DTD_GEMM_SKINNY_SLABS overrides S in
// tuning runs.
//
// Supported: 1 <= M <= 64, N % 16 == 0, K % 128 == 0, 16-byte aligned rows (dtd_gemm_skinny_supported
// checks the three sizes, the launcher the rest).
#include <stdlib.h>

#include "common.h"

using namespace dtd;

namespace {

constexpr int kStep = 128;     // k per K-step: 4 MFMAs of 32
constexpr int kWaves = 4;      // K-steps per chunk: one per wave

enum Format : int { kFmtBF16 = 0, kFmtFP8 = 1 };

struct SkinnyArgs {
  const bf16* x;
  const void* w;
  const float* scale;    // FP8 only
  bf16* y;
  size_t ldx, ldw, ldy;  // row strides in elements
  int M, N, K;
};

// workgroup barrier that waits for this wave's LDS traffic only: the weight loads stay in flight across it
__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// 8 codes (two dwords, element e in byte e) as bf16: exact
__device__ __forceinline__ bf16x8 codes_to_bf16(unsigned lo, unsigned hi) {
  const auto a = __builtin_amdgcn_cvt_pk_f32_fp8((int)lo, false);
  const auto b = __builtin_amdgcn_cvt_pk_f32_fp8((int)lo, true);
  const auto c = __builtin_amdgcn_cvt_pk_f32_fp8((int)hi, false);
  const auto d = __builtin_amdgcn_cvt_pk_f32_fp8((int)hi, true);
  bf16x8 r;
  r[0] = (bf16)a[0]; r[1] = (bf16)a[1]; r[2] = (bf16)b[0]; r[3] = (bf16)b[1];
  r[4] = (bf16)c[0]; r[5] = (bf16)c[1]; r[6] = (bf16)d[0]; r[7] = (bf16)d[1];
  return r;
}

// 4 floats -> 4 bf16 in two dwords
__device__ __forceinline__ uint2 pack4(const float (&v)[4]) {
  bf16x4 p;
#pragma unroll
  for (int r = 0; r < 4; ++r) p[r] = (bf16)v[r];
  return __builtin_bit_cast(uint2, p);
}

// Every load below is unconditional, at an address clamped into the operand: a load under a branch makes
// the compiler give up counting the loads in flight and drain the queue (s_waitcnt vmcnt(0)) at the next
// use, which would serialise the weight stream.

// Chunk c's X pieces of one thread, in registers: piece r is LDS piece tid + 256 r =
// ((ksl * 4 + f) * MT + t) * 64 + lane, the 8 elements that lane (q, i) feeds to MFMA f of K-step ksl for
// column tile t.  A row at or above M is not read (the lane reads row M - 1 and store_x writes zeros); a
// K-step past the last reads the last one, and no wave reads that piece.
template <int MT, bool FP8>
__device__ __forceinline__ void load_x(const SkinnyArgs& a, int c, int nsteps, int wave, int q, int i,
                                       bf16x8 (&xr)[4 * MT]) {
#pragma unroll
  for (int r = 0; r < 4 * MT; ++r) {
    const int rest = wave + 4 * r;
    const int t = rest % MT, f = (rest / MT) & 3, ksl = rest / (4 * MT);
    int m = 16 * t + i;
    m = m < a.M ? m : a.M - 1;
    int ks = c * kWaves + ksl;
    ks = ks < nsteps ? ks : nsteps - 1;
    const int ko = FP8 ? (f >> 1) * 64 + q * 16 + (f & 1) * 8 : f * 32 + q * 8;
    xr[r] = *reinterpret_cast<const bf16x8*>(a.x + (size_t)m * a.ldx + (size_t)ks * kStep + ko);
  }
}

// The pieces into LDS, zeros for the rows at and above M.
template <int MT>
__device__ __forceinline__ void store_x(uint4* lds, int tid, int wave, int i, int M, const bf16x8 (&xr)[4 * MT]) {
#pragma unroll
  for (int r = 0; r < 4 * MT; ++r) {
    const int t = (wave + 4 * r) % MT;
    const uint4 v = __builtin_bit_cast(uint4, xr[r]);
    lds[tid + 256 * r] = 16 * t + i < M ? v : make_uint4(0u, 0u, 0u, 0u);
  }
}

// This wave's K-step of chunk c, all slabs: LPS 16-byte loads per slab (a K-step past the last reads the
// last one, and its MFMAs are skipped).
template <bool FP8, int S>
__device__ __forceinline__ void load_w(const uint8_t* const (&wrow)[S], int c, int nsteps, int wave,
                                       uint4 (&dst)[S][FP8 ? 2 : 4]) {
  int ks = c * kWaves + wave;
  ks = ks < nsteps ? ks : nsteps - 1;
  const size_t off = (size_t)ks * kStep * (FP8 ? 1 : 2);
#pragma unroll
  for (int s = 0; s < S; ++s)
#pragma unroll
    for (int j = 0; j < (FP8 ? 2 : 4); ++j) dst[s][j] = *reinterpret_cast<const uint4*>(wrow[s] + off + j * 64);
}

// One K-step: 4 MFMAs per slab and column tile, X's fragments from LDS.
template <int MT, bool FP8, int S>
__device__ __forceinline__ void mma_step(const uint4* lds, int wave, int lane, const uint4 (&w)[S][FP8 ? 2 : 4],
                                         f32x4 (&acc)[S][MT]) {
#pragma unroll
  for (int f = 0; f < 4; ++f) {
    bf16x8 xb[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) xb[t] = __builtin_bit_cast(bf16x8, lds[((wave * 4 + f) * MT + t) * 64 + lane]);
#pragma unroll
    for (int s = 0; s < S; ++s) {
      bf16x8 wf;
      if constexpr (FP8) {
        const uint4 raw = w[s][f >> 1];
        wf = (f & 1) ? codes_to_bf16(raw.z, raw.w) : codes_to_bf16(raw.x, raw.y);
      } else {
        wf = __builtin_bit_cast(bf16x8, w[s][f]);
      }
#pragma unroll
      for (int t = 0; t < MT; ++t) acc[s][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, xb[t], acc[s][t], 0, 0, 0);
    }
  }
}

// MT: column tiles of 16 (the M bucket); FP8: the weight format; S: slabs per workgroup.
template <int MT, bool FP8, int S>
__global__ void __launch_bounds__(256) gemm_skinny_kernel(const SkinnyArgs a) {
  constexpr int LPS = FP8 ? 2 : 4;                 // 16-byte loads per lane, slab and K-step
  constexpr int XP = 4 * MT;                       // X pieces per thread and chunk
  static_assert(S <= 4 && S * MT <= 8, "the partials reuse the X buffer; the registers are sized for S * MT <= 8");
  // X chunk [4 K-steps][4 MFMAs][MT][64 lanes] x 16 bytes; then the partials [4 waves][S][MT][64] x 16 bytes
  __shared__ uint4 lds[kWaves * 4 * MT * 64];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int q = lane >> 4, i = lane & 15;
  const int nslabs = a.N >> 4;
  const int nsteps = a.K / kStep;
  const int nchunks = (nsteps + kWaves - 1) / kWaves;

  // this lane's row of each slab (a slab past the last reads the last one and is never stored)
  const uint8_t* wrow[S];
#pragma unroll
  for (int s = 0; s < S; ++s) {
    int slab = blockIdx.x * S + s;
    slab = slab < nslabs ? slab : nslabs - 1;
    wrow[s] = static_cast<const uint8_t*>(a.w) + ((size_t)slab * 16 + i) * a.ldw * (FP8 ? 1 : 2) + q * 16;
  }

  uint4 cur[S][LPS], nxt[S][LPS];
  bf16x8 xr[XP];
  f32x4 acc[S][MT];
#pragma unroll
  for (int s = 0; s < S; ++s)
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[s][t] = f32x4{0.f, 0.f, 0.f, 0.f};

  load_x<MT, FP8>(a, 0, nsteps, wave, q, i, xr);
  load_w<FP8, S>(wrow, 0, nsteps, wave, cur);
  for (int c = 0; c + 1 < nchunks; ++c) {          // the full chunks: every wave has a K-step
    if (c) lds_barrier();                          // chunk c - 1 has been read
    store_x<MT>(lds, tid, wave, i, a.M, xr);
    lds_barrier();
    load_x<MT, FP8>(a, c + 1, nsteps, wave, q, i, xr);
    load_w<FP8, S>(wrow, c + 1, nsteps, wave, nxt);
    mma_step<MT, FP8, S>(lds, wave, lane, cur, acc);
#pragma unroll
    for (int s = 0; s < S; ++s)
#pragma unroll
      for (int j = 0; j < LPS; ++j) cur[s][j] = nxt[s][j];
  }
  if (nchunks > 1) lds_barrier();
  store_x<MT>(lds, tid, wave, i, a.M, xr);         // the last chunk: 1 to 4 K-steps
  lds_barrier();
  if ((nchunks - 1) * kWaves + wave < nsteps) mma_step<MT, FP8, S>(lds, wave, lane, cur, acc);

  // the sum over the waves, in wave order, and the stores
  lds_barrier();
#pragma unroll
  for (int s = 0; s < S; ++s)
#pragma unroll
    for (int t = 0; t < MT; ++t) lds[((wave * S + s) * MT + t) * 64 + lane] = __builtin_bit_cast(uint4, acc[s][t]);
  lds_barrier();
  constexpr int TP = MT >= 2 ? 2 : 1;              // column tiles per store
  constexpr int UPS = MT / TP;                     // store units per slab
  for (int u = wave; u < S * UPS; u += kWaves) {
    const int s = u / UPS, tp = u % UPS;
    const int slab = blockIdx.x * S + s;
    if (slab >= nslabs) continue;                  // (wave-uniform)
    const int n = slab * 16 + 4 * q;
    float sc[4] = {1.f, 1.f, 1.f, 1.f};
    if constexpr (FP8) {
#pragma unroll
      for (int r = 0; r < 4; ++r) sc[r] = a.scale[n + r];
    }
    uint2 pk[TP];
#pragma unroll
    for (int h = 0; h < TP; ++h) {
      const int t = tp * TP + h;
      f32x4 p[kWaves];
#pragma unroll
      for (int w = 0; w < kWaves; ++w) p[w] = __builtin_bit_cast(f32x4, lds[((w * S + s) * MT + t) * 64 + lane]);
      float v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        v[r] = ((p[0][r] + p[1][r]) + p[2][r]) + p[3][r];
        if constexpr (FP8) v[r] *= sc[r];
      }
      pk[h] = pack4(v);
    }
    if constexpr (TP == 2) {
      // lanes q and q ^ 1 hold the two halves of 8 consecutive n of both tiles: an even q keeps the
      // first tile, an odd q the second, and each takes the other half from its partner
      const bool odd = q & 1;
      const uint2 give = odd ? pk[0] : pk[1];
      uint2 take;
      take.x = __shfl_xor(give.x, 16, 64);
      take.y = __shfl_xor(give.y, 16, 64);
      const uint4 out = odd ? make_uint4(take.x, take.y, pk[1].x, pk[1].y) : make_uint4(pk[0].x, pk[0].y, take.x, take.y);
      const int m = 16 * (tp * 2 + (odd ? 1 : 0)) + i;
      if (m < a.M) *reinterpret_cast<uint4*>(a.y + (size_t)m * a.ldy + slab * 16 + 4 * (q & ~1)) = out;
    } else {
      if (i < a.M) *reinterpret_cast<uint2*>(a.y + (size_t)i * a.ldy + n) = pk[0];
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

// Slabs per workgroup: a function of the shape (and the CU count) only.
int pick_slabs(int MT, int N) {
  static const int forced = [] {
    const char* e = getenv("DTD_GEMM_SKINNY_SLABS");
    return e ? atoi(e) : 0;
  }();
  const int smax = MT == 4 ? 2 : 4;
  if (forced == 1 || forced == 2 || forced == 4) return forced < smax ? forced : smax;
  const int nslabs = N / 16;
  int S = smax;
  while (S > 1 && (nslabs + S - 1) / S < cu_count()) S >>= 1;
  return S;
}

template <int MT, bool FP8>
void launch_s(int S, int N, hipStream_t st, const SkinnyArgs& a) {
  const int nslabs = N / 16;
  const dim3 grid((nslabs + S - 1) / S);
  if (S == 1) hipLaunchKernelGGL((gemm_skinny_kernel<MT, FP8, 1>), grid, dim3(256), 0, st, a);
  else if (S == 2) hipLaunchKernelGGL((gemm_skinny_kernel<MT, FP8, 2>), grid, dim3(256), 0, st, a);
  else if constexpr (MT < 4) hipLaunchKernelGGL((gemm_skinny_kernel<MT, FP8, 4>), grid, dim3(256), 0, st, a);
}

template <bool FP8>
void launch_mt(int MT, int N, hipStream_t st, const SkinnyArgs& a) {
  const int S = pick_slabs(MT, N);
  if (MT == 1) launch_s<1, FP8>(S, N, st, a);
  else if (MT == 2) launch_s<2, FP8>(S, N, st, a);
  else launch_s<4, FP8>(S, N, st, a);
}

}  // namespace

DTD_EXPORT int dtd_gemm_skinny_supported(int M, int N, int K) {
  return M >= 1 && M <= 64 && N > 0 && N % 16 == 0 && K > 0 && K % kStep == 0;
}

// fmt 0: w bf16 [N, K]; fmt 1: w e4m3fn codes [N, K] with scale fp32 [N].  ldx, ldw, ldy: row strides in
// elements.  x [M, K] and y [M, N] bf16.
DTD_EXPORT int dtd_gemm_skinny(int fmt, const void* x, int ldx, const void* w, int ldw, const float* scale, void* y,
                               int ldy, int M, int N, int K, hipStream_t s) {
  if (!dtd_gemm_skinny_supported(M, N, K) || (fmt != kFmtBF16 && fmt != kFmtFP8)) return (int)hipErrorInvalidValue;
  if (!x || !w || !y || ((uintptr_t)x | (uintptr_t)w | (uintptr_t)y) % 16) return (int)hipErrorInvalidValue;
  if (ldx < K || ldx % 8 || ldw < K || ldw % (fmt == kFmtFP8 ? 16 : 8) || ldy < N || ldy % 8) return (int)hipErrorInvalidValue;
  if (fmt == kFmtFP8 && (!scale || (uintptr_t)scale % 4)) return (int)hipErrorInvalidValue;
  SkinnyArgs a;
  a.x = (const bf16*)x; a.w = w; a.scale = scale; a.y = (bf16*)y;
  a.ldx = (size_t)ldx; a.ldw = (size_t)ldw; a.ldy = (size_t)ldy;
  a.M = M; a.N = N; a.K = K;
  const int MT = M <= 16 ? 1 : (M <= 32 ? 2 : 4);
  if (fmt == kFmtFP8) launch_mt<true>(MT, N, s, a);
  else launch_mt<false>(MT, N, s, a);
  DTD_LAUNCH_CHECK();
}
