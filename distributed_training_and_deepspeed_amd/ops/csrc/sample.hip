// Token sampling on the device: temperature, top-k, top-p (nucleus) and the draw in one launch.
//
// The law (ops/functional.py::sample_tokens_ref states it in PyTorch):
//   z_i = float(logit_i) * inv_t; a -inf (or NaN) entry is never kept;
//   top-k keeps the k largest z, ties to the lower index;
//   top-p keeps, of those in descending z (ties to the lower index), the shortest prefix whose softmax
//   mass reaches top_p;
//   the draw returns the first kept index, in ascending index order, whose running mass exceeds u * Z
//   (Z the kept mass, u 24 bits of the counter hash of common.h over (seed, step, kSampleSid, row)).
//
// Design.  One workgroup of 1024 threads per row; rows are independent.
//  * The row is read ONCE, with 16-byte loads (vector it * 1024 + tid of the 16-byte grid the row lies on;
//    the two ragged edge vectors element by element), and stays in registers as the raw words, where the
//    register budget allows: 128 VGPRs a thread at 1024 threads, of which the passes' own temporaries (the
//    fp64 exponential, 64-bit sums) take about 70.  That leaves 4 vectors a thread for bf16 (V <= 32760) and
//    12 for fp32 (V <= 49148); these kernels use no scratch memory.  Held at 16 vectors (V = 128256 in bf16) the
//    compiler spilled 66 to 80 registers, so that size is not built: a longer row (up to kMaxV) runs the same
//    passes re-reading the row from memory, where the head's GEMM left it in L2 (72 VGPRs, no scratch).
//  * No sort.  Both thresholds come from a radix descent over the order-preserving key, 8 bits a pass, each
//    pass one 256-bin histogram in LDS: of counts for top-k, of masses for top-p.  bf16 logits are keyed by
//    their own 16 bits (the scaling by inv_t > 0 keeps their order and, within fp32's normal range, their
//    distinctness): two passes; fp32 logits by the 32 bits of z: four.
//  * Determinism.  No float atomics: a mass is the integer round(2^40 exp(z - max)) (exp in fp64, so a mass
//    is exact to half a unit), histograms and sums are 64-bit integer adds, whose order does not matter.
//    V <= 2^20 keeps every sum below 2^61.
//  * A threshold's ties are equal keys, hence equal masses: the descent returns how many of them are still
//    needed, and the lowest indices fill that count.
//  * Index order.  A wave's vector in iteration `it` covers 64 consecutive vectors, so (it, wave) numbers
//    contiguous segments of the row in ascending order.  "First index whose running sum exceeds t" is:
//    segment sums (a wave reduction each), one scan over the segments by wave 0, then a lane scan and an
//    element walk inside the one segment that holds t.  The tie cut-offs and the draw all use it.
//  * EOS: a finished row (done[b]) emits pad without reading its logits; a row that emits eos sets done[b].
// LDS: the histogram and the segment sums (2.7 or 3.7 KiB; 34 KiB for the rows re-read from memory).  No workspace
// and no allocation: the call writes out[B] (and done[B]) only.
#include "common.h"

namespace {
using namespace dtd;

constexpr int kThreads = 1024, kWaves = kThreads / kWave;
constexpr int kFrac = 40;                       // fractional bits of a mass
constexpr uint32_t kSampleSid = 0x53414D50u;    // ops/functional.py SAMPLE_SID (above every dropout stream id)
constexpr int kMaxV = 1 << 20;
typedef unsigned long long u64;

template <typename T> struct Fmt;
template <> struct Fmt<bf16> {
  static constexpr int kEpv = 8, kKeyBits = 16;
  static constexpr int kMoreVecs = 0;           // no second in-register size: 8 vectors already spill
  static constexpr uint32_t kNegInfWord = 0xFF80FF80u;
  static __device__ __forceinline__ void put(uint32_t* w, int j, const bf16* p) {
    const uint32_t h = *reinterpret_cast<const uint16_t*>(p), sh = (j & 1) * 16;
    w[j >> 1] = (w[j >> 1] & ~(0xFFFFu << sh)) | (h << sh);
  }
  static __device__ __forceinline__ void get(const uint32_t* w, int j, float inv_t, float& z, uint32_t& key) {
    uint32_t h = (w[j >> 1] >> ((j & 1) * 16)) & 0xFFFFu;
    if (h == 0x8000u) h = 0;                    // -0 ties with +0
    z = __uint_as_float(h << 16) * inv_t;
    key = (h & 0x8000u) ? (~h & 0xFFFFu) : (h | 0x8000u);
  }
  static __device__ __forceinline__ float z_of_key(uint32_t key, float inv_t) {
    const uint32_t h = (key & 0x8000u) ? (key ^ 0x8000u) : (~key & 0xFFFFu);
    return __uint_as_float(h << 16) * inv_t;
  }
};
template <> struct Fmt<float> {
  static constexpr int kEpv = 4, kKeyBits = 32;
  static constexpr int kMoreVecs = 12;
  static constexpr uint32_t kNegInfWord = 0xFF800000u;
  static __device__ __forceinline__ void put(uint32_t* w, int j, const float* p) {
    w[j] = *reinterpret_cast<const uint32_t*>(p);
  }
  static __device__ __forceinline__ void get(const uint32_t* w, int j, float inv_t, float& z, uint32_t& key) {
    z = __uint_as_float(w[j]) * inv_t + 0.0f;   // -0 ties with +0
    const uint32_t b = __float_as_uint(z);
    key = (b >> 31) ? ~b : (b | 0x80000000u);
  }
  static __device__ __forceinline__ float z_of_key(uint32_t key, float) {
    return __uint_as_float((key >> 31) ? (key ^ 0x80000000u) : ~key);
  }
};

// NV > 0: the row's vectors in registers; NV == 0: read again from memory by every pass.
template <typename T, int NV> struct Row {
  uint32_t r[NV > 0 ? NV * 4 : 4];
  const T* pa;     // the row's pointer rounded down to 16 bytes
  int off, V, nit; // the row's first element within its vector; length; vectors per thread
  float inv_t;
};

template <int NV> struct Smem {
  static constexpr int kSegs = NV > 0 ? NV * kWaves : (kMaxV / 4 / kThreads + 1) * kWaves;
  u64 hist[256];
  u64 seg[kSegs];
  u64 red[kWaves];
  float redf[kWaves];
  u64 above, tie, target, seg_base;
  int digit, seg_found, result;
};

// Vector vg of the row's 16-byte grid as four raw words; elements outside the row read as -inf (and are not loaded).
template <typename T>
__device__ __forceinline__ void load_vec(const T* pa, int vg, int off, int V, uint32_t* w) {
  constexpr int E = Fmt<T>::kEpv;
  const int i0 = vg * E - off;
  if (i0 >= 0 && i0 + E <= V) {
    const uint4 v = *reinterpret_cast<const uint4*>(pa + (size_t)vg * E);
    w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q) w[q] = Fmt<T>::kNegInfWord;
#pragma unroll
    for (int j = 0; j < E; ++j)
      if (i0 + j >= 0 && i0 + j < V) Fmt<T>::put(w, j, pa + (size_t)vg * E + j);
  }
}

// f(it, words) for the thread's vectors (all of them, or iteration `only` alone)
template <typename T, int NV, typename F>
__device__ __forceinline__ void for_each_vec(const Row<T, NV>& row, int only, F&& f) {
  if constexpr (NV > 0) {
#pragma unroll
    for (int v = 0; v < NV; ++v)
      if (only < 0 || only == v) {
        // an opaque copy: the decoded keys and z of every held element are loop invariants of every pass loop, and
        // hoisted out of one they would all have to live in registers at once
        uint32_t w[4] = {row.r[v * 4], row.r[v * 4 + 1], row.r[v * 4 + 2], row.r[v * 4 + 3]};
        asm volatile("" : "+v"(w[0]), "+v"(w[1]), "+v"(w[2]), "+v"(w[3]));
        f(v, w);
      }
  } else {
    const int lo = only < 0 ? 0 : only, hi = only < 0 ? row.nit : only + 1;
    for (int it = lo; it < hi; ++it) {
      uint32_t w[4];
      load_vec<T>(row.pa, it * kThreads + (int)threadIdx.x, row.off, row.V, w);
      f(it, w);
    }
  }
}

// f(j, index, z, key, valid) for the elements of one vector
template <typename T, int NV, typename F>
__device__ __forceinline__ void for_each_in_vec(const Row<T, NV>& row, int it, const uint32_t* w, F&& f) {
  constexpr int E = Fmt<T>::kEpv;
  const int i0 = (it * kThreads + (int)threadIdx.x) * E - row.off;
#pragma unroll
  for (int j = 0; j < E; ++j) {
    float z; uint32_t key;
    Fmt<T>::get(w, j, row.inv_t, z, key);
    f(j, i0 + j, z, key, z > -INFINITY);
  }
}

template <typename T, int NV, typename F>
__device__ __forceinline__ void for_each_elem(const Row<T, NV>& row, F&& f) {
  for_each_vec(row, -1, [&](int it, const uint32_t* w) {
    for_each_in_vec(row, it, w, [&](int, int idx, float z, uint32_t key, bool valid) { f(idx, z, key, valid); });
  });
}

__device__ __forceinline__ u64 wave_sum_u64(u64 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ u64 wave_scan_u64(u64 v, int lane) {   // inclusive, ascending lanes
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const u64 t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}

__device__ __forceinline__ u64 mass(float z, float m) {
  const double d = (double)z - (double)m;
  if (!(d > -29.0)) return 0;                   // below half a unit (2^-41 = e^-28.4), or NaN
  return (u64)(exp(d) * (double)(1ull << kFrac) + 0.5);
}

// Radix descent.  Over the elements with wt(...) participating (valid ones), find the key T with
//   S(key > T) < target <= S(key >= T),   S = sum of weights,   target = target_of(S(all)).
// Returns T, with above = S(key > T), tie = S(key == T) and the target.
template <typename T, int NV, typename W, typename TF>
__device__ __forceinline__ uint32_t descend(const Row<T, NV>& row, Smem<NV>& sm, W&& wt, TF&& target_of, u64& above,
                                            u64& tie, u64& target) {
  const int tid = threadIdx.x, lane = tid & 63;
  uint32_t prefix = 0;
  above = tie = target = 0;
  for (int shift = Fmt<T>::kKeyBits - 8; shift >= 0; shift -= 8) {
    __syncthreads();                             // (every thread has read the previous pass's result)
    if (tid < 256) sm.hist[tid] = 0;
    if (tid == 0) { sm.digit = 0; sm.tie = 0; sm.above = above; }
    __syncthreads();
    const uint32_t hi_mask = shift + 8 >= 32 ? 0u : (0xFFFFFFFFu << (shift + 8));
    for_each_elem(row, [&](int idx, float z, uint32_t key, bool valid) {
      if (valid && ((key ^ prefix) & hi_mask) == 0) {
        const u64 w = wt(idx, z, key);
        if (w) atomicAdd(&sm.hist[(key >> shift) & 255u], w);
      }
    });
    __syncthreads();
    if (tid < 64) {                              // lane l owns bins 4l .. 4l+3; suffix sums from the top bin down
      u64 h[4], s = 0;
#pragma unroll
      for (int q = 0; q < 4; ++q) { h[q] = sm.hist[4 * lane + q]; s += h[q]; }
      u64 suf = s;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const u64 t = __shfl_down(suf, o, 64);
        if (lane + o < 64) suf += t;
      }
      if (shift == Fmt<T>::kKeyBits - 8) {
        target = target_of(__shfl(suf, 0, 64));
        if (lane == 0) sm.target = target;
      }
      u64 gt = above + suf - s;
#pragma unroll
      for (int q = 3; q >= 0; --q) {
        const u64 ge = gt + h[q];
        if (gt < target && target <= ge) { sm.digit = 4 * lane + q; sm.above = gt; sm.tie = h[q]; }
        gt = ge;
      }
    }
    __syncthreads();
    prefix |= (uint32_t)sm.digit << shift;
    above = sm.above;
    tie = sm.tie;
    target = sm.target;
  }
  return prefix;
}

// Segment sums of wt in index order into sm.seg; returns their total.
template <typename T, int NV, typename W>
__device__ __forceinline__ u64 seg_totals(const Row<T, NV>& row, Smem<NV>& sm, W&& wt) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  u64 mine = 0;
  __syncthreads();                               // (the previous readers of sm.seg are done)
  for_each_vec(row, -1, [&](int it, const uint32_t* w) {
    u64 s = 0;
    for_each_in_vec(row, it, w, [&](int, int idx, float z, uint32_t key, bool valid) { s += wt(idx, z, key, valid); });
    s = wave_sum_u64(s);
    if (lane == 0) sm.seg[it * kWaves + wave] = s;
    mine += s;
  });
  if (lane == 0) sm.red[wave] = mine;
  __syncthreads();
  u64 total = 0;
#pragma unroll
  for (int i = 0; i < kWaves; ++i) total += sm.red[i];
  return total;
}

// After seg_totals(wt): the first index whose inclusive running sum of wt exceeds tgt; -1 when none does.
template <typename T, int NV, typename W>
__device__ __forceinline__ int locate(const Row<T, NV>& row, Smem<NV>& sm, W&& wt, u64 tgt) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nseg = row.nit * kWaves;
  if (wave == 0) {
    u64 carry = 0, base = 0;
    int found = -1;
    for (int c = 0; c < nseg && found < 0; c += 64) {
      const u64 v = c + lane < nseg ? sm.seg[c + lane] : 0;
      const u64 inc = wave_scan_u64(v, lane);
      const u64 hit = __ballot(carry + inc > tgt);
      if (hit) {
        const int l = __ffsll((long long)hit) - 1;
        found = c + l;
        base = carry + __shfl(inc - v, l, 64);
      }
      carry += __shfl(inc, 63, 64);
    }
    if (lane == 0) { sm.seg_found = found; sm.seg_base = base; sm.result = -1; }
  }
  __syncthreads();
  const int fs = sm.seg_found;
  if (fs >= 0 && (fs % kWaves) == wave) {        // the wave that holds the segment: lane scan, then the element walk
    const u64 base = sm.seg_base;
    for_each_vec(row, fs / kWaves, [&](int it, const uint32_t* w) {
      u64 s = 0;
      for_each_in_vec(row, it, w, [&](int, int idx, float z, uint32_t key, bool valid) { s += wt(idx, z, key, valid); });
      const u64 inc = wave_scan_u64(s, lane);
      const u64 hit = __ballot(base + inc > tgt);
      if (hit && lane == __ffsll((long long)hit) - 1) {
        u64 run = base + inc - s;
        int res = -1;
        for_each_in_vec(row, it, w, [&](int, int idx, float z, uint32_t key, bool valid) {
          run += wt(idx, z, key, valid);
          if (res < 0 && run > tgt) res = idx;
        });
        sm.result = res;
      }
    });
  }
  __syncthreads();
  return sm.result;
}

template <typename T, int NV>
__device__ __forceinline__ int sample_row(Row<T, NV>& row, Smem<NV>& sm, int top_k, double top_p, uint32_t u24) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if constexpr (NV > 0) {
#pragma unroll
    for (int v = 0; v < NV; ++v) load_vec<T>(row.pa, v * kThreads + tid, row.off, row.V, &row.r[v * 4]);
  }
  // the row's maximum and its number of finite entries
  float m = -INFINITY;
  u64 nv = 0;
  for_each_elem(row, [&](int, float z, uint32_t, bool valid) { if (valid) { m = fmaxf(m, z); ++nv; } });
  m = wave_max(m);
  nv = wave_sum_u64(nv);
  if (lane == 0) { sm.redf[wave] = m; sm.red[wave] = nv; }
  __syncthreads();
  m = -INFINITY; nv = 0;
#pragma unroll
  for (int i = 0; i < kWaves; ++i) { m = fmaxf(m, sm.redf[i]); nv += sm.red[i]; }
  if (nv == 0) return 0;

  // top-k: keys above Tk, and the ties at Tk up to index Ik
  const bool usek = top_k > 0 && (u64)top_k < nv;
  uint32_t Tk = 0;
  int Ik = INT_MAX;
  u64 above, ties, target;
  if (usek) {
    Tk = descend(row, sm, [](int, float, uint32_t) -> u64 { return 1; }, [&](u64) -> u64 { return (u64)top_k; },
                 above, ties, target);
    const u64 need = target - above;
    if (need < ties) {
      auto tie = [&](int, float, uint32_t key, bool valid) -> u64 { return valid && key == Tk; };
      seg_totals(row, sm, tie);
      const int i = locate(row, sm, tie, need - 1);
      if (i >= 0) Ik = i;
    }
  }
  auto kept1 = [&](int idx, uint32_t key) { return !usek || key > Tk || (key == Tk && idx <= Ik); };

  // top-p: of those, keys above Tp and the ties at Tp up to index Ip
  const bool usep = top_p < 1.0;
  uint32_t Tp = 0;
  int Ip = INT_MAX;
  if (usep) {
    Tp = descend(row, sm, [&](int idx, float z, uint32_t key) -> u64 { return kept1(idx, key) ? mass(z, m) : 0; },
                 [&](u64 total) -> u64 {
                   const u64 t = (u64)ceil(top_p * (double)total);
                   return t < 1 ? 1 : (t > total ? total : t);
                 }, above, ties, target);
    u64 wt = mass(Fmt<T>::z_of_key(Tp, row.inv_t), m);
    if (wt == 0) wt = 1;
    const u64 need = (target - above + wt - 1) / wt;
    if (need < ties / wt) {
      auto tie = [&](int idx, float, uint32_t key, bool valid) -> u64 { return valid && key == Tp && kept1(idx, key); };
      seg_totals(row, sm, tie);
      const int i = locate(row, sm, tie, need - 1);
      if (i >= 0) Ip = i;
    }
  }

  // the draw, over the kept masses in index order
  auto kept_mass = [&](int idx, float z, uint32_t key, bool valid) -> u64 {
    const bool keep = valid && kept1(idx, key) && (!usep || key > Tp || (key == Tp && idx <= Ip));
    return keep ? mass(z, m) : 0;
  };
  const u64 Z = seg_totals(row, sm, kept_mass);
  const u64 tgt = (__umul64hi(Z, (u64)u24) << 40) | ((Z * (u64)u24) >> 24);    // floor(u Z), exact
  const int tok = locate(row, sm, kept_mass, tgt);
  return tok < 0 ? 0 : tok;
}

template <typename T, int NV>
__global__ __launch_bounds__(kThreads) void sample_kernel(const T* __restrict__ logits, long ld, int V, float inv_t,
                                                          int top_k, double top_p, u64 seed,
                                                          const u64* __restrict__ step, uint8_t* __restrict__ done,
                                                          long eos, long pad, long* __restrict__ out) {
  __shared__ Smem<NV> sm;
  const int b = blockIdx.x;
  if (done != nullptr && done[b]) {              // block-uniform
    if (threadIdx.x == 0) out[b] = pad;
    return;
  }
  constexpr int E = Fmt<T>::kEpv;
  const T* p = logits + (size_t)b * ld;
  Row<T, NV> row;
  row.off = (int)(((uintptr_t)p & 15) / sizeof(T));
  row.pa = p - row.off;
  row.V = V;
  row.inv_t = inv_t;
  row.nit = NV > 0 ? NV : ((row.off + V + E - 1) / E + kThreads - 1) / kThreads;
  // 24 uniform bits for this row: DropoutRng's keys (common.h) with the sampler's stream id
  const u64 st = step[0];
  const uint32_t k0 = mix32((uint32_t)seed ^ mix32((uint32_t)(seed >> 32) + 0x9e3779b9U));
  const uint32_t k1 = mix32((uint32_t)st * 0x85ebca6bU ^ mix32(kSampleSid + 0x632be5abU) ^ k0);
  const uint32_t u24 = mix32(((uint32_t)b ^ k0) + k1) >> 8;
  const int tok = sample_row(row, sm, top_k, top_p, u24);
  if (threadIdx.x == 0) {
    out[b] = tok;
    if (done != nullptr && tok == eos) done[b] = 1;
  }
}

template <typename T>
int launch(const void* logits, long ld, int B, int V, float inv_t, int top_k, double top_p, u64 seed, const void* step,
           void* done, long eos, long pad, void* out, hipStream_t s) {
  constexpr int E = Fmt<T>::kEpv;
  const int nvec = (V + 2 * (E - 1)) / E;       // vectors of the 16-byte grid a row can touch, at any alignment
  auto go = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3(B), dim3(kThreads), 0, s, (const T*)logits, ld, V, inv_t, top_k, top_p, seed,
                       (const u64*)step, (uint8_t*)done, eos, pad, (long*)out);
  };
  constexpr int M = Fmt<T>::kMoreVecs;
  if (nvec <= 4 * kThreads) {
    go(sample_kernel<T, 4>);
  } else if (M > 0 && nvec <= M * kThreads) {
    if constexpr (M > 0) go(sample_kernel<T, M>);
  } else {
    go(sample_kernel<T, 0>);
  }
  DTD_LAUNCH_CHECK();
}
}  // namespace

// logits [B, V] (row stride ld elements, unit column stride), inv_t > 0, top_k (<= 0: off), 0 < top_p <= 1,
// seed, step (device int64 [1]), done (device uint8 [B] or null) with eos / pad, out (device int64 [B]).
DTD_EXPORT int dtd_sample_tokens(int dtype, const void* logits, long ld, int B, int V, float inv_t, int top_k,
                                 double top_p, unsigned long long seed, const void* step, void* done, long eos,
                                 long pad, void* out, hipStream_t s) {
  if (B <= 0) return 0;
  if (V <= 0 || V > kMaxV || !(inv_t > 0.f) || !(top_p > 0.0 && top_p <= 1.0)) return (int)hipErrorInvalidValue;
  if (dtype == kBF16) return launch<bf16>(logits, ld, B, V, inv_t, top_k, top_p, seed, step, done, eos, pad, out, s);
  if (dtype == kF32) return launch<float>(logits, ld, B, V, inv_t, top_k, top_p, seed, step, done, eos, pad, out, s);
  return (int)hipErrorInvalidValue;
}
