// LM-head cross-entropy without the logits ("chunked LM-head+CE fusion").
//
// The unfused causal-LM head writes the bf16 logits [T, V], reads them for the row LSE, keeps them
// for the backward and writes a second [T, V] tensor there.  Here the logit tiles only ever live in
// MFMA accumulators:
//   dtd_head_lse     : z = x . w^T per (128-token tile, vocabulary range) -> a running per-token
//                      (max, sum exp) over the range, one fp32 partial per (token, range); the tile
//                      that holds a token's label column also writes the fp32 label logit.  A second
//                      kernel combines the partials of a row in a fixed order (lse, loss per row) and a
//                      one-block kernel reduces them to (mean, count).  No atomics: bitwise
//                      reproducible.
//   dtd_head_dlogits : recomputes z for the vocabulary columns [v0, v1) and writes
//                      (exp(z - lse) - onehot) * grad_out / count as bf16 into a chunk buffer.
//
// Both kernels share one 128 x 128 x h tile product on v_mfma_f32_32x32x16_bf16 (fragment maps in
// attention.hip): "P" rows land in the accumulator registers, "Q" rows on the lanes.  The forward
// takes P = weight rows, Q = tokens: a lane owns one token and 2 x 16 of its logits, so the softmax
// reduction over the vocabulary is in-register, and the four partials of a token (2 waves x 2 lane
// halves) meet once per workgroup in LDS.  The backward takes P = tokens, Q = weight rows: the
// vocabulary is on the lane and the 32 lanes of a half-wave store 64 contiguous bytes of a row.
// Global -> register -> LDS staging, two LDS stages, one barrier per 64-wide K step.
//
// Bounds: operand rows are clamped to the last valid row on load (tokens >= T, weight rows >= V
// are read from valid memory and never reach a result: columns >= V are -inf in the forward and
// are not stored in the backward).  x and w are addressed from 64-bit bases; the chunk buffer is
// addressed with 32-bit element offsets (T * ldd < 2^30, checked on the host -- the Python plan
// splits rows above that).
#include "common.h"

using namespace dtd;

typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

constexpr int TILE = 128;           // rows of P and of Q per workgroup tile
constexpr int KT = 64;              // K elements per LDS stage
constexpr int LROW = KT + 8;        // LDS row of 144 bytes: conflict-free 16-byte fragment reads
constexpr int OPER = TILE * LROW;   // one operand of one stage (elements)
constexpr int THREADS = 256;        // 4 waves: 2 (P halves) x 2 (Q halves), 64 x 64 per wave
constexpr int MAX_RANGES = 512;

__device__ __forceinline__ f32x16 mfma32(bf16x8 a, bf16x8 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ int crow(int i, int h) { return (i & 3) + 8 * (i >> 2) + 4 * h; }

// rows [row0, row0 + 128) x columns [k0, k0 + 64) of a row-major operand: 4 x 16 bytes per thread;
// rows past the end re-read the last valid row
__device__ __forceinline__ void load_tile(const bf16* __restrict__ base, size_t ld, int row0, int nrows, int k0,
                                          bf16x8 (&r)[4]) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int row = min(row0 + (tid >> 3) + 32 * j, nrows - 1);
    r[j] = *reinterpret_cast<const bf16x8*>(base + (size_t)row * ld + k0 + (tid & 7) * 8);
  }
}
__device__ __forceinline__ void store_tile(bf16* lds, const bf16x8 (&r)[4]) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    *reinterpret_cast<bf16x8*>(lds + ((tid >> 3) + 32 * j) * LROW + (tid & 7) * 8) = r[j];
}

// acc[ps][qs] = P[prow0 + wp*64 + ps*32 + ..] . Q[qrow0 + wq*64 + qs*32 + ..]^T over K = h.
// Every thread of the workgroup calls it; it ends on a barrier, so `smem` is free afterwards.
__device__ __forceinline__ void tile_product(bf16* smem, const bf16* __restrict__ P, size_t ldp, int prow0, int prows,
                                             const bf16* __restrict__ Q, size_t ldq, int qrow0, int qrows, int h,
                                             f32x16 (&acc)[2][2]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wp = wave >> 1, wq = wave & 1;
  const int fo = (lane & 31) * LROW + (lane >> 5) * 8;   // this lane's fragment inside a 32-row subtile
  bf16x8 rp[4], rq[4];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[a][b][i] = 0.f;
  const int nk = h / KT;
  load_tile(P, ldp, prow0, prows, 0, rp);
  load_tile(Q, ldq, qrow0, qrows, 0, rq);
  store_tile(smem, rp);
  store_tile(smem + OPER, rq);
  __syncthreads();
  for (int i = 0; i < nk; ++i) {
    const bf16* sp = smem + (i & 1) * 2 * OPER;
    const bf16* sq = sp + OPER;
    const bool more = i + 1 < nk;
    if (more) {
      load_tile(P, ldp, prow0, prows, (i + 1) * KT, rp);
      load_tile(Q, ldq, qrow0, qrows, (i + 1) * KT, rq);
    }
#pragma unroll
    for (int ks = 0; ks < KT / 16; ++ks) {
      bf16x8 a[2], b[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        a[t] = *reinterpret_cast<const bf16x8*>(sp + (wp * 64 + t * 32) * LROW + fo + ks * 16);
        b[t] = *reinterpret_cast<const bf16x8*>(sq + (wq * 64 + t * 32) * LROW + fo + ks * 16);
      }
#pragma unroll
      for (int ps = 0; ps < 2; ++ps)
#pragma unroll
        for (int qs = 0; qs < 2; ++qs) acc[ps][qs] = mfma32(a[ps], b[qs], acc[ps][qs]);
    }
    if (more) {   // the other stage: last read before the barrier that ended step i - 1
      bf16* np = smem + ((i + 1) & 1) * 2 * OPER;
      store_tile(np, rp);
      store_tile(np + OPER, rq);
    }
    __syncthreads();
  }
}

// grid (token tiles, ranges).  part[T][R][2] = (max, sum exp(z - max)) of the token's logits in the
// range; zlab[T] = the label logit (written by the one workgroup whose range holds the label).
__global__ void __launch_bounds__(THREADS) head_lse_kernel(const bf16* __restrict__ x, size_t ldx,
                                                           const bf16* __restrict__ w, size_t ldw,
                                                           const int64_t* __restrict__ labels,
                                                           float* __restrict__ part, float* __restrict__ zlab, int T,
                                                           int V, int h, int R, int tiles_per) {
  __shared__ __attribute__((aligned(16))) bf16 smem[4 * OPER];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wp = wave >> 1, wq = wave & 1, half = lane >> 5;
  const int t0 = blockIdx.x * TILE, r = blockIdx.y;
  const int nvt = (V + TILE - 1) / TILE;
  const int vt_end = min(nvt, (r + 1) * tiles_per);
  int tok[2], lab[2];
  float m[2], s[2];
#pragma unroll
  for (int qs = 0; qs < 2; ++qs) {
    tok[qs] = t0 + wq * 64 + qs * 32 + (lane & 31);
    const int64_t y = tok[qs] < T ? labels[tok[qs]] : -1;
    lab[qs] = (y >= 0 && y < V) ? (int)y : -1;
    m[qs] = -INFINITY;
    s[qs] = 0.f;
  }
  for (int vt = r * tiles_per; vt < vt_end; ++vt) {
    f32x16 acc[2][2];
    tile_product(smem, w, ldw, vt * TILE, V, x, ldx, t0, T, h, acc);
    const int vrow = vt * TILE + wp * 64;
#pragma unroll
    for (int qs = 0; qs < 2; ++qs) {
      float tm = -INFINITY;
#pragma unroll
      for (int ps = 0; ps < 2; ++ps)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int row = vrow + ps * 32 + crow(i, half);
          const float z = row < V ? acc[ps][qs][i] : -INFINITY;
          acc[ps][qs][i] = z;
          tm = fmaxf(tm, z);
          if (row == lab[qs]) zlab[tok[qs]] = z;   // lab >= 0 only for tokens < T
        }
      if (tm > -INFINITY) {   // else: every column of this lane is past V
        if (tm > m[qs]) {
          s[qs] *= __expf(m[qs] - tm);   // exp(-inf) = 0 on the first tile
          m[qs] = tm;
        }
        float e = 0.f;
#pragma unroll
        for (int ps = 0; ps < 2; ++ps)
#pragma unroll
          for (int i = 0; i < 16; ++i) e += __expf(acc[ps][qs][i] - m[qs]);
        s[qs] += e;
      }
    }
  }
  // the four partials of a token, combined in a fixed order; smem is free (tile_product's barrier)
  float* comb = reinterpret_cast<float*>(smem);   // [4][TILE][2]
#pragma unroll
  for (int qs = 0; qs < 2; ++qs) {
    const int c = ((wp * 2 + half) * TILE + wq * 64 + qs * 32 + (lane & 31)) * 2;
    comb[c] = m[qs];
    comb[c + 1] = s[qs];
  }
  __syncthreads();
  const int tid = threadIdx.x;
  if (tid < TILE && t0 + tid < T) {
    float M = -INFINITY;
#pragma unroll
    for (int k = 0; k < 4; ++k) M = fmaxf(M, comb[(k * TILE + tid) * 2]);
    float S = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float mk = comb[(k * TILE + tid) * 2];
      if (mk > -INFINITY) S += comb[(k * TILE + tid) * 2 + 1] * __expf(mk - M);
    }
    float* o = part + ((size_t)(t0 + tid) * R + r) * 2;
    o[0] = M;
    o[1] = S;
  }
}

// lse / loss per row from the R partials: one wave per row (a thread per row walked its R partials
// in 43 us at 512 rows x 64 ranges), lane l takes ranges l, l + 64, ... and the butterfly
// reductions combine the lanes in a fixed order
__global__ void __launch_bounds__(256) head_combine_kernel(const float* __restrict__ part,
                                                           const float* __restrict__ zlab,
                                                           const int64_t* __restrict__ labels,
                                                           float* __restrict__ lse_row, float* __restrict__ loss_row,
                                                           int T, int R, int ignore_index) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= T) return;   // wave-uniform; no barrier below
  if (labels[row] == ignore_index) {
    if (lane == 0) { lse_row[row] = 0.f; loss_row[row] = 0.f; }
    return;
  }
  const float* p = part + (size_t)row * R * 2;
  float M = -INFINITY;
  for (int k = lane; k < R; k += 64) M = fmaxf(M, p[2 * k]);
  M = wave_max(M);
  float S = 0.f;
  for (int k = lane; k < R; k += 64) S += p[2 * k + 1] * expf(p[2 * k] - M);
  S = wave_sum(S);
  if (lane == 0) {
    const float lse = M + logf(S);
    lse_row[row] = lse;
    loss_row[row] = lse - zlab[row];
  }
}

// stats[0] = sum(loss_row) / count, stats[1] = count of rows with a label (xent.hip's layout)
__global__ void __launch_bounds__(1024) head_reduce_kernel(const float* __restrict__ loss_row,
                                                           const int64_t* __restrict__ labels, int T,
                                                           int ignore_index, float* __restrict__ stats) {
  __shared__ float sh[16];
  float s = 0.f, c = 0.f;
  for (int r = threadIdx.x; r < T; r += blockDim.x)
    if (labels[r] != ignore_index) { s += loss_row[r]; c += 1.f; }
  s = block_sum(s, sh);
  c = block_sum(c, sh);
  if (threadIdx.x == 0) { stats[0] = c > 0.f ? s / c : NAN; stats[1] = c; }
}

// grid (token tiles, vocabulary tiles of [v0, v1)).  d[T][ldd], column c - v0.
__global__ void __launch_bounds__(THREADS) head_dlogits_kernel(const bf16* __restrict__ x, size_t ldx,
                                                               const bf16* __restrict__ w, size_t ldw,
                                                               const int64_t* __restrict__ labels,
                                                               const float* __restrict__ lse_row,
                                                               const float* __restrict__ stats,
                                                               const float* __restrict__ grad_out,
                                                               bf16* __restrict__ d, int ldd, int T, int V, int h,
                                                               int v0, int v1, int ignore_index) {
  __shared__ __attribute__((aligned(16))) bf16 smem[4 * OPER];
  __shared__ float s_lse[TILE], s_g[TILE];
  __shared__ int s_lab[TILE];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wp = wave >> 1, wq = wave & 1, half = lane >> 5;
  const int t0 = blockIdx.x * TILE, c0 = v0 + blockIdx.y * TILE;
  if (threadIdx.x < TILE) {
    const int t = t0 + threadIdx.x;
    const int64_t y = t < T ? labels[t] : (int64_t)ignore_index;
    const bool valid = y != ignore_index;
    // an unlabelled row: exp(z - inf) = 0 and scale 0, an exact zero gradient
    s_lse[threadIdx.x] = valid ? lse_row[t] : INFINITY;
    s_g[threadIdx.x] = valid ? grad_out[0] / stats[1] : 0.f;
    s_lab[threadIdx.x] = valid ? (int)y : -1;
  }
  f32x16 acc[2][2];
  tile_product(smem, x, ldx, t0, T, w, ldw, c0, V, h, acc);   // its barriers publish s_lse / s_g / s_lab
#pragma unroll
  for (int qs = 0; qs < 2; ++qs) {
    const int col = c0 + wq * 64 + qs * 32 + (lane & 31);
    if (col >= v1) continue;
#pragma unroll
    for (int ps = 0; ps < 2; ++ps)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int tr = wp * 64 + ps * 32 + crow(i, half);
        if (t0 + tr < T) {
          float p = __expf(acc[ps][qs][i] - s_lse[tr]);
          if (col == s_lab[tr]) p -= 1.f;
          d[(t0 + tr) * ldd + (col - v0)] = (bf16)(p * s_g[tr]);
        }
      }
  }
}

bool aligned16(const void* p, long ld) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0 && ld % 8 == 0; }

}  // namespace

// Shapes the kernels take: any T >= 1 and V >= 1, h a multiple of the 64-wide K step.
DTD_EXPORT int dtd_head_xent_supported(int T, int V, int h) {
  return T >= 1 && V >= 1 && h >= KT && h % KT == 0 && (T + TILE - 1) / TILE <= 65535 * 16;
}

// Number of vocabulary ranges R of the forward (part is [T][R][2] floats): enough workgroups for two
// per CU at 256 CUs, every range non-empty.
DTD_EXPORT int dtd_head_lse_ranges(int T, int V) {
  if (T < 1 || V < 1) return 0;
  const int ntt = (T + TILE - 1) / TILE, nvt = (V + TILE - 1) / TILE;
  int want = (512 + ntt - 1) / ntt;
  want = want < 1 ? 1 : want > MAX_RANGES ? MAX_RANGES : want;
  if (want > nvt) want = nvt;
  const int per = (nvt + want - 1) / want;
  return (nvt + per - 1) / per;
}

DTD_EXPORT int dtd_head_lse(const void* x, long ldx, const void* w, long ldw, const int64_t* labels, float* part,
                            float* zlab, float* lse_row, float* loss_row, float* stats, int T, int V, int h,
                            int ignore_index, hipStream_t s) {
  if (!dtd_head_xent_supported(T, V, h) || !aligned16(x, ldx) || !aligned16(w, ldw) || ldx < h || ldw < h)
    return (int)hipErrorInvalidValue;
  const int ntt = (T + TILE - 1) / TILE, nvt = (V + TILE - 1) / TILE;
  const int R = dtd_head_lse_ranges(T, V), per = (nvt + R - 1) / R;
  hipLaunchKernelGGL(head_lse_kernel, dim3(ntt, R), dim3(THREADS), 0, s, (const bf16*)x, (size_t)ldx, (const bf16*)w,
                     (size_t)ldw, labels, part, zlab, T, V, h, R, per);
  hipLaunchKernelGGL(head_combine_kernel, dim3((T + 3) / 4), dim3(256), 0, s, (const float*)part,
                     (const float*)zlab, labels, lse_row, loss_row, T, R, ignore_index);
  hipLaunchKernelGGL(head_reduce_kernel, dim3(1), dim3(1024), 0, s, (const float*)loss_row, labels, T, ignore_index,
                     stats);
  DTD_LAUNCH_CHECK();
}

// Largest T * ldd of a chunk buffer (32-bit element offsets, byte offsets below 2^31).
DTD_EXPORT long dtd_head_dlogits_max_elems() { return 1L << 30; }

DTD_EXPORT int dtd_head_dlogits(const void* x, long ldx, const void* w, long ldw, const int64_t* labels,
                                const float* lse_row, const float* stats, const float* grad_out, void* d, long ldd,
                                int T, int V, int h, int v0, int v1, int ignore_index, hipStream_t s) {
  if (!dtd_head_xent_supported(T, V, h) || !aligned16(x, ldx) || !aligned16(w, ldw) || ldx < h || ldw < h ||
      v0 < 0 || v1 > V || v0 >= v1 || ldd < v1 - v0 || (long)T * ldd > dtd_head_dlogits_max_elems() ||
      (v1 - v0 + TILE - 1) / TILE > 65535)
    return (int)hipErrorInvalidValue;
  const int ntt = (T + TILE - 1) / TILE, nct = (v1 - v0 + TILE - 1) / TILE;
  hipLaunchKernelGGL(head_dlogits_kernel, dim3(ntt, nct), dim3(THREADS), 0, s, (const bf16*)x, (size_t)ldx,
                     (const bf16*)w, (size_t)ldw, labels, lse_row, stats, grad_out, (bf16*)d, (int)ldd, T, V, h, v0,
                     v1, ignore_index);
  DTD_LAUNCH_CHECK();
}
