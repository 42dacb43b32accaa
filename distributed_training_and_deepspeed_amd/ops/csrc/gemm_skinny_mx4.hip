// Skinny GEMM on OCP MXFP4 weights: Y[M, N] = bf16(sum_k x[m][k] * deq(W)[n][k]) with 1 <= M <= 64.
//
// hipcc-flags: -Xclang -target-feature -Xclang -packed-fp32-ops
//
// X and Y are bf16.  W is stored by ops/quant.py's MX4 law: codes uint8 [N, K/2], two e2m1 elements per
// byte (element 2 j in the low nibble of byte j), and scales uint8 [N, K/32], one e8m0 exponent byte per
// block of 32 consecutive k: deq(W)[n][k] = e2m1(code) * 2^(byte - 127), exact in bf16.  That is 4.25 bits
// per weight, so the kernel is gemm_skinny.hip's weight streamer with every decision that depended on the
// bytes per weight taken again.  What it keeps, because that kernel proved it: W goes from memory into
// VGPRs and is the ROW operand of v_mfma_f32_16x16x32_bf16 (a wave owns slabs of 16 output features, lane
// (q, i) = (lane / 16, lane % 16) holds row i), no LDS on W's way; X is staged in LDS in fragment order; the
// four waves of a workgroup split K for the same slabs and sum their fp32 partials through LDS in wave
// order, ((p0 + p1) + p2) + p3 -- no atomics, two calls are bitwise equal; every load is unconditional at an
// address clamped into its operand.  What is new:
//   * Load mapping.  One 16-byte load of a lane is exactly one MX block: the 32 codes of block q of row i
//     in the K-step (128 k = 64 bytes of codes per row), so a load instruction still reads 64 contiguous
//     bytes of each of 16 rows, and ONE load per lane, slab and K-step feeds all four MFMAs: dword f holds
//     the elements 8 f .. 8 f + 7 of the block.  MFMA f of lane (q, .) therefore multiplies k = 32 q + 8 f +
//     e (e < 8), and X's staging applies that permutation once (load_x: ko = 32 q + 8 f).
//   * Scale.  It differs per block, so it cannot wait for the epilogue as scale[n] does: it goes onto the
//     weights.  v_cvt_scalef32_pk_bf16_fp4 takes it as an fp32 operand (byte << 23 is 2^(byte - 127)) and
//     yields two bf16 from one byte of codes, 16 conversions per block, the product exact.  A lane's block
//     has ONE scale: byte 4 ks + q of row i's scales, fetched as one byte load beside the codes' load, in
//     the same stage of the ring, clamped by the same K-step index -- never a dependent load in front of a
//     conversion.  (The 16 scale bytes of a row's chunk are the four waves' 4 x 4 blocks; each wave takes
//     its own four, one per q.)
//   * Bytes in flight.  A K-step of a slab is 1 KiB per wave where bf16 has 4 KiB, so "the next chunk" of
//     the bf16 schedule keeps a quarter of the bytes in flight.  The register file decides how to win them
//     back: a stage (one K-step of one slab) is 5 VGPRs, codes and scale, so the ring is D chunks deep with
//     D = 2 at S >= 4 and D = 4 at S <= 2 -- at S = 8, D = 2 a wave has 16 KiB in flight, what bf16 has at
//     S = 4 -- and the X chunk in LDS stays 4 K-steps (one per wave), which keeps LDS at 16 KiB per column
//     tile.  More K-steps per wave and chunk instead would have multiplied the X buffer (64 KiB per column
//     tile at 16 K-steps).  The ring has D + 1 stages and the loop is unrolled by D + 1, so a stage is a fixed
//     set of registers and nothing is moved while its load is in flight.  The chunks past the last re-read
//     the last K-step (clamped; they hit the cache and are never used).
//   * X against W.  A workgroup stages 4 KiB of X per K-step and column tile for 1 KiB of W per slab: at
//     the bf16 kernel's S <= 4 X's traffic from L2 would equal the weight stream.  The quarter-size stages
//     make room for S = 8 at MT = 1, 4 at MT = 2, 2 at MT = 4 (S MT <= 8: the accumulators and the partials'
//     32 KiB of LDS).
// S depends on the shape alone (and the device's CU count): the largest power of two up to 8 / MT that still
// gives every CU a workgroup, so a captured decode step replays one launch sequence.
// DTD_GEMM_SKINNY_MX4_SLABS overrides S in tuning runs.  Scale byte 255 (e8m0's NaN) is never written by the
// law; what comes out of it here is unspecified.
//
// Supported: 1 <= M <= 64, N % 16 == 0, K % 128 == 0, 16-byte aligned rows of x, codes and y
// (dtd_gemm_skinny_mx4_supported checks the three sizes, the launcher the rest).
#include <stdlib.h>

#include "common.h"

using namespace dtd;

namespace {

constexpr int kStep = 128;     // k per K-step: 4 MFMAs of 32, one MX block per lane
constexpr int kWaves = 4;      // K-steps per chunk: one per wave
constexpr int kMaxSlabs = 8;

struct Mx4Args {
  const bf16* x;
  const uint8_t* codes;
  const uint8_t* scales;
  bf16* y;
  size_t ldx, ldy;       // row strides in elements
  size_t ldc, lds;       // row strides of codes and scales in bytes
  int M, N, K;
};

// one K-step of one slab in a lane's registers: its block's 32 codes and the block's scale byte
struct Stage {
  uint4 c;
  unsigned s;
};

// workgroup barrier that waits for this wave's LDS traffic only: the weight loads stay in flight across it
__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// 8 codes (one dword, element e in nibble e) times the block's scale, as bf16: exact
__device__ __forceinline__ bf16x8 codes_to_bf16(unsigned dw, float scale) {
  const bf16x2 a = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(dw, scale, 0);
  const bf16x2 b = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(dw, scale, 1);
  const bf16x2 c = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(dw, scale, 2);
  const bf16x2 d = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(dw, scale, 3);
  bf16x8 r;
  r[0] = a[0]; r[1] = a[1]; r[2] = b[0]; r[3] = b[1];
  r[4] = c[0]; r[5] = c[1]; r[6] = d[0]; r[7] = d[1];
  return r;
}

// 4 floats -> 4 bf16 in two dwords
__device__ __forceinline__ uint2 pack4(const float (&v)[4]) {
  bf16x4 p;
#pragma unroll
  for (int r = 0; r < 4; ++r) p[r] = (bf16)v[r];
  return __builtin_bit_cast(uint2, p);
}

// Chunk c's X pieces of one thread, in registers: piece r is LDS piece tid + 256 r = ((ksl * 4 + f) * MT + t)
// * 64 + lane, the 8 elements k = 32 q + 8 f + e that lane (q, i) feeds to MFMA f of K-step ksl for column
// tile t.  A row at or above M is not read (the lane reads row M - 1 and store_x writes zeros); a K-step past
// the last reads the last one, and no wave reads that piece.
template <int MT>
__device__ __forceinline__ void load_x(const Mx4Args& a, int c, int nsteps, int wave, int q, int i,
                                       bf16x8 (&xr)[4 * MT]) {
#pragma unroll
  for (int r = 0; r < 4 * MT; ++r) {
    const int rest = wave + 4 * r;
    const int t = rest % MT, f = (rest / MT) & 3, ksl = rest / (4 * MT);
    int m = 16 * t + i;
    m = m < a.M ? m : a.M - 1;
    int ks = c * kWaves + ksl;
    ks = ks < nsteps ? ks : nsteps - 1;
    xr[r] = *reinterpret_cast<const bf16x8*>(a.x + (size_t)m * a.ldx + (size_t)ks * kStep + q * 32 + f * 8);
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

// This wave's K-step of chunk c, all slabs: one 16-byte load of codes and one byte of scale per slab (a K-step
// past the last reads the last one, and its MFMAs are skipped or its stage is never reached).  cbase / sbase:
// the slabs' first rows (wave-uniform); coff / soff: this lane's row and block inside a slab.
template <int S>
__device__ __forceinline__ void load_w(const uint8_t* const (&cbase)[S], const uint8_t* const (&sbase)[S], unsigned coff,
                                       unsigned soff, int c, int nsteps, int wave, Stage (&dst)[S]) {
  int ks = c * kWaves + wave;
  ks = ks < nsteps ? ks : nsteps - 1;
#pragma unroll
  for (int s = 0; s < S; ++s) {
    dst[s].c = *reinterpret_cast<const uint4*>(cbase[s] + (size_t)ks * (kStep / 2) + coff);
    dst[s].s = sbase[s][(size_t)ks * (kStep / 32) + soff];
  }
}

// One K-step: 4 MFMAs per slab and column tile, X's fragments from LDS, the codes converted on the way.
template <int MT, int S>
__device__ __forceinline__ void mma_step(const uint4* lds, int wave, int lane, const Stage (&w)[S], f32x4 (&acc)[S][MT]) {
  float sc[S];
#pragma unroll
  for (int s = 0; s < S; ++s) sc[s] = __builtin_bit_cast(float, w[s].s << 23);
#pragma unroll
  for (int f = 0; f < 4; ++f) {
    bf16x8 xb[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) xb[t] = __builtin_bit_cast(bf16x8, lds[((wave * 4 + f) * MT + t) * 64 + lane]);
#pragma unroll
    for (int s = 0; s < S; ++s) {
      const unsigned dw = f == 0 ? w[s].c.x : (f == 1 ? w[s].c.y : (f == 2 ? w[s].c.z : w[s].c.w));
      const bf16x8 wf = codes_to_bf16(dw, sc[s]);
#pragma unroll
      for (int t = 0; t < MT; ++t) acc[s][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, xb[t], acc[s][t], 0, 0, 0);
    }
  }
}

// MT: column tiles of 16 (the M bucket); S: slabs per workgroup; D: chunks of W in flight ahead of the MFMAs.
template <int MT, int S, int D>
__global__ void __launch_bounds__(256) gemm_skinny_mx4_kernel(const Mx4Args a) {
  constexpr int XP = 4 * MT;                       // X pieces per thread and chunk
  static_assert(S <= kMaxSlabs && S * MT <= 8, "the registers and the partials' LDS are sized for S * MT <= 8");
  // X chunk [4 K-steps][4 MFMAs][MT][64 lanes] x 16 bytes; then the partials [4 waves][S][MT][64] x 16 bytes
  __shared__ uint4 lds[kWaves * (S > 4 ? S : 4) * MT * 64];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int q = lane >> 4, i = lane & 15;
  const int nslabs = a.N >> 4;
  const int nsteps = a.K / kStep;
  const int nchunks = (nsteps + kWaves - 1) / kWaves;

  // the slabs' first rows (a slab past the last reads the last one and is never stored)
  const uint8_t* cbase[S];
  const uint8_t* sbase[S];
#pragma unroll
  for (int s = 0; s < S; ++s) {
    int slab = blockIdx.x * S + s;
    slab = slab < nslabs ? slab : nslabs - 1;
    cbase[s] = a.codes + (size_t)slab * 16 * a.ldc;
    sbase[s] = a.scales + (size_t)slab * 16 * a.lds;
  }
  const unsigned coff = (unsigned)i * (unsigned)a.ldc + q * 16;   // (15 rows of K / 2 bytes: far below 2^32)
  const unsigned soff = (unsigned)i * (unsigned)a.lds + q;

  constexpr int R = D + 1;
  Stage ring[R][S];                                // chunk c lives in ring[c % R]
  Stage last[S];
  bf16x8 xr[XP];
  f32x4 acc[S][MT];
#pragma unroll
  for (int s = 0; s < S; ++s)
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[s][t] = f32x4{0.f, 0.f, 0.f, 0.f};

  load_x<MT>(a, 0, nsteps, wave, q, i, xr);
#pragma unroll
  for (int d = 0; d < D; ++d) load_w<S>(cbase, sbase, coff, soff, d, nsteps, wave, ring[d]);
  // The loop is unrolled by R so that every ring index is a constant: no register is moved while its load
  // is in flight (a move would wait for the load and empty the ring).
  for (int c0 = 0;; c0 += R) {
#pragma unroll
    for (int p = 0; p < R; ++p) {
      const int c = c0 + p;
      if (c + 1 >= nchunks) {                      // the last chunk: below
#pragma unroll
        for (int s = 0; s < S; ++s) last[s] = ring[p][s];
        goto tail;
      }
      if (c) lds_barrier();                        // chunk c - 1 has been read
      store_x<MT>(lds, tid, wave, i, a.M, xr);
      lds_barrier();
      load_x<MT>(a, c + 1, nsteps, wave, q, i, xr);
      load_w<S>(cbase, sbase, coff, soff, c + D, nsteps, wave, ring[(p + D) % R]);
      mma_step<MT, S>(lds, wave, lane, ring[p], acc);   // a full chunk: every wave has a K-step
    }
  }
tail:
  if (nchunks > 1) lds_barrier();
  store_x<MT>(lds, tid, wave, i, a.M, xr);         // the last chunk: 1 to 4 K-steps
  lds_barrier();
  if ((nchunks - 1) * kWaves + wave < nsteps) mma_step<MT, S>(lds, wave, lane, last, acc);

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
    uint2 pk[TP];
#pragma unroll
    for (int h = 0; h < TP; ++h) {
      const int t = tp * TP + h;
      f32x4 p[kWaves];
#pragma unroll
      for (int w = 0; w < kWaves; ++w) p[w] = __builtin_bit_cast(f32x4, lds[((w * S + s) * MT + t) * 64 + lane]);
      float v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = ((p[0][r] + p[1][r]) + p[2][r]) + p[3][r];
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
    const char* e = getenv("DTD_GEMM_SKINNY_MX4_SLABS");
    return e ? atoi(e) : 0;
  }();
  const int smax = kMaxSlabs / MT;
  if (forced == 1 || forced == 2 || forced == 4 || forced == 8) return forced < smax ? forced : smax;
  const int nslabs = N / 16;
  int S = smax;
  while (S > 1 && (nslabs + S - 1) / S < cu_count()) S >>= 1;
  return S;
}

template <int MT>
void launch_s(int S, int N, hipStream_t st, const Mx4Args& a) {
  const int nslabs = N / 16;
  const dim3 grid((nslabs + S - 1) / S);
  if (S == 1) hipLaunchKernelGGL((gemm_skinny_mx4_kernel<MT, 1, 4>), grid, dim3(256), 0, st, a);
  else if (S == 2) hipLaunchKernelGGL((gemm_skinny_mx4_kernel<MT, 2, 4>), grid, dim3(256), 0, st, a);
  else if constexpr (MT <= 2) {
    if (S == 4) hipLaunchKernelGGL((gemm_skinny_mx4_kernel<MT, 4, 2>), grid, dim3(256), 0, st, a);
    else if constexpr (MT == 1) hipLaunchKernelGGL((gemm_skinny_mx4_kernel<MT, 8, 2>), grid, dim3(256), 0, st, a);
  }
}

}  // namespace

DTD_EXPORT int dtd_gemm_skinny_mx4_supported(int M, int N, int K) {
  return M >= 1 && M <= 64 && N > 0 && N % 16 == 0 && K > 0 && K % kStep == 0;
}

// x [M, K] and y [M, N] bf16 with row strides ldx, ldy in elements; codes uint8 [N, K / 2] with row stride ldc
// bytes; scales uint8 [N, K / 32] with row stride lds bytes.
DTD_EXPORT int dtd_gemm_skinny_mx4(const void* x, int ldx, const void* codes, int ldc, const void* scales, int lds, void* y,
                                   int ldy, int M, int N, int K, hipStream_t s) {
  if (!dtd_gemm_skinny_mx4_supported(M, N, K)) return (int)hipErrorInvalidValue;
  if (!x || !codes || !scales || !y || ((uintptr_t)x | (uintptr_t)codes | (uintptr_t)y) % 16) return (int)hipErrorInvalidValue;
  if (ldx < K || ldx % 8 || ldc < K / 2 || ldc % 16 || lds < K / 32 || ldy < N || ldy % 8) return (int)hipErrorInvalidValue;
  Mx4Args a;
  a.x = (const bf16*)x; a.codes = (const uint8_t*)codes; a.scales = (const uint8_t*)scales; a.y = (bf16*)y;
  a.ldx = (size_t)ldx; a.ldy = (size_t)ldy; a.ldc = (size_t)ldc; a.lds = (size_t)lds;
  a.M = M; a.N = N; a.K = K;
  const int MT = M <= 16 ? 1 : (M <= 32 ? 2 : 4);
  const int S = pick_slabs(MT, N);
  if (MT == 1) launch_s<1>(S, N, s, a);
  else if (MT == 2) launch_s<2>(S, N, s, a);
  else launch_s<4>(S, N, s, a);
  DTD_LAUNCH_CHECK();
}
