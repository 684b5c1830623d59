// sample.hip -- the one-read sampler (ops.sample_tokens) and its counter-based uniforms
// (ops.seeded_uniform).
//
//  * seeded_uniform : Philox4x32-10, key (seed & 0xffffffff, seed >> 32), counter
//                     (index, 0, 0, 0); u = float(w0 >> 8) * 2^-24, exact in fp32 and < 1.
//  * sample_tokens  : temperature / top-k / top-p / min-p sampling, the contract of
//                     sample_kernel (embed_sample.hip) plus min_p, from bf16 or fp32 logits as
//                     the LM head wrote them.  One 1024-thread workgroup per row.  A bf16 row of
//                     up to 131072 logits is read from memory ONCE, 16 bytes a lane, and stays
//                     packed in <= 64 registers per thread: the 24-round threshold searches,
//                     the masses and the draw all run on those registers, wave shuffles and LDS.
//                     fp32 rows and bf16 rows the vector loads cannot take (stride or base not
//                     16-byte aligned, longer rows) run the same code over memory.
//
// Per row, with x = float32(logit) * inv_temp over the columns below n_valid:
//   top_k == 1           -> the lowest index of the maximum, whatever else is set
//   0 < top_k < n_valid  -> keep x >= k-th largest (bisection over [min, max], ties kept)
//   0 < top_p < 1        -> of those, the shortest descending prefix with mass >= top_p
//                           (bisection on the mass; ties at the cutoff kept).  When the top-k
//                           survivors fit the LDS list (<= 2048) the search runs on the list.
//   min_p > 0            -> and x >= max + log(min_p), i.e. p_i >= min_p * p_max
// then the inverse CDF of the kept tokens in index order at u, the row's uniform: the caller's
// or seeded_uniform(seed, index) computed here.  Rows with valid == 0 write 0 and read nothing.
// Logits are expected finite, inv_temp positive.
#include "docqa_common.h"
#include <float.h>
#include <math.h>

using namespace docqa;

namespace {

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxVec = 16;           // vectors (of Row::span logits) a thread owns at most
constexpr int kCand = 2 * kThreads;   // top-k survivors the LDS list holds

__device__ __forceinline__ float seeded_u01(long long seed, int index) {
  uint32_t k0 = (uint32_t)(unsigned long long)seed, k1 = (uint32_t)((unsigned long long)seed >> 32);
  uint32_t c0 = (uint32_t)index, c1 = 0, c2 = 0, c3 = 0;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
    const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
    c0 = h1 ^ c1 ^ k0; c1 = l1; c2 = h0 ^ c3 ^ k1; c3 = l0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return (float)(c0 >> 8) * 0x1p-24f;
}

__global__ __launch_bounds__(256) void seeded_uniform_kernel(const long long* __restrict__ seed,
                                                             const int* __restrict__ index,
                                                             float* __restrict__ out, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = seeded_u01(seed[i], index[i]);
}

// A row's logits as the workgroup's threads own them: vector (u, thread) covers `span`
// consecutive columns from (u * 1024 + thread) * span, so index order is (u, wave, lane, j).
// each(f, g, only): f(logit, column) for the thread's columns, g(u) after each vector -- every
// lane of a wave reaches g(u) together; `only` >= 0 visits that vector alone.

// NV x 8 bf16 in registers; columns at or past n_valid hold -inf
template <int NV>
struct RegRow {
  uint4 v[NV];
  __device__ __forceinline__ RegRow(const void* base, size_t off, int V) {
    const uint16_t* r = reinterpret_cast<const uint16_t*>(base) + off;
    const uint4 ninf{0xff80ff80u, 0xff80ff80u, 0xff80ff80u, 0xff80ff80u};
#pragma unroll
    for (int u = 0; u < NV; ++u) {
      const int c = (u * kThreads + (int)threadIdx.x) * 8;
      v[u] = c + 8 <= V ? *reinterpret_cast<const uint4*>(r + c) : ninf;
    }
    // n_valid % 8 != 0: the one vector that straddles the end, column by column
    const int pv = V / 8;
    if (V % 8 != 0 && pv % kThreads == (int)threadIdx.x) {
      uint32_t w[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t a = pv * 8 + 2 * j < V ? r[pv * 8 + 2 * j] : 0xff80u;
        const uint32_t b = pv * 8 + 2 * j + 1 < V ? r[pv * 8 + 2 * j + 1] : 0xff80u;
        w[j] = a | (b << 16);
      }
#pragma unroll
      for (int u = 0; u < NV; ++u)
        if (u == pv / kThreads) v[u] = uint4{w[0], w[1], w[2], w[3]};
    }
  }
  template <class F, class G>
  __device__ __forceinline__ void each(F&& f, G&& g, int only = -1) {
#pragma unroll
    for (int u = 0; u < NV; ++u) {
      if (only >= 0 && u != only) continue;
      // the packed words are the loop-invariant state: without this the compiler keeps the 8 NV
      // unpacked products alive across the search rounds and spills them
      asm volatile("" : "+v"(v[u].x), "+v"(v[u].y), "+v"(v[u].z), "+v"(v[u].w));
      float x[8];
      unpack8(v[u], x);
      const int c = (u * kThreads + (int)threadIdx.x) * 8;
#pragma unroll
      for (int j = 0; j < 8; ++j) f(x[j], c + j);
      g(u);
    }
  }
};

__device__ __forceinline__ float to_f32(float v) { return v; }
__device__ __forceinline__ float to_f32(uint16_t v) { return bf2f(v); }

// the row where it lies (fp32, or bf16 the vector loads cannot take): span = ceil(V / 16384)
template <class T>
struct MemRow {
  const T* r;
  int V, span, nv;
  __device__ __forceinline__ MemRow(const void* base, size_t off, int V_)
      : r(reinterpret_cast<const T*>(base) + off), V(V_) {
    span = (int)(((long long)V + kThreads * kMaxVec - 1) / (kThreads * kMaxVec));
    nv = (int)(((long long)V + (long long)kThreads * span - 1) / ((long long)kThreads * span));
  }
  template <class F, class G>
  __device__ __forceinline__ void each(F&& f, G&& g, int only = -1) const {
    for (int u = 0; u < nv; ++u) {
      if (only >= 0 && u != only) continue;
      const long long c = ((long long)u * kThreads + threadIdx.x) * span;
      for (int j = 0; j < span; ++j)   // past the end: -inf like RegRow, so every lane calls f
        f(c + j < V ? to_f32(r[c + j]) : -INFINITY, (int)(c + j));
      g(u);
    }
  }
};

struct Shared {
  uint32_t red[2][kWaves];     // block reductions, double buffered: one barrier each
  int ridx[kWaves];
  float part[kMaxVec * kWaves];   // kept mass per (vector, wave), the index order of the row
  float cand[kCand];
  int ncand;
  int sel;                     // the (vector, wave) entry the draw falls in
  float sel_base;              // kept mass in front of it
  float target;
};

__device__ __forceinline__ float block_sum(float v, Shared& sh, int& buf) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) sh.red[buf][threadIdx.x >> 6] = __float_as_uint(v);
  __syncthreads();
  float s = 0.f;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) s += __uint_as_float(sh.red[buf][w]);
  buf ^= 1;
  return s;
}
__device__ __forceinline__ float block_max(float v, Shared& sh, int& buf) {
  v = wave_max(v);
  if ((threadIdx.x & 63) == 0) sh.red[buf][threadIdx.x >> 6] = __float_as_uint(v);
  __syncthreads();
  float s = -INFINITY;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) s = fmaxf(s, __uint_as_float(sh.red[buf][w]));
  buf ^= 1;
  return s;
}
__device__ __forceinline__ uint32_t block_count(uint32_t c, Shared& sh, int& buf) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  if ((threadIdx.x & 63) == 0) sh.red[buf][threadIdx.x >> 6] = c;
  __syncthreads();
  uint32_t s = 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) s += sh.red[buf][w];
  buf ^= 1;
  return s;
}

__device__ __forceinline__ float wave_scan(float v) {   // inclusive, lane order
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}

// lane of the first set bit of `hit`, or of the last set bit of `any` when `hit` is empty
// (a target the rounded masses fall short of takes the last kept entry), or 0
__device__ __forceinline__ int first_or_last(unsigned long long hit, unsigned long long any) {
  if (hit) return __ffsll((long long)hit) - 1;
  if (any) return 63 - __clzll((long long)any);
  return 0;
}

template <class Row>
__device__ __forceinline__ void sample_row(Row& row, Shared& sh, int V, float it, int k, float p,
                                           float mp, float u01, int64_t* out) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const auto none = [](int) {};
  int buf = 0;
  if (k == 1) {
    // greedy row inside a sampled batch: the lowest index of the maximum (k is per row, so
    // the branch is uniform)
    float bv = -FLT_MAX;
    int bi = 0x7fffffff;
    row.each([&](float l, int i) { const float x = l * it; if (x > bv || (x == bv && i < bi)) { bv = x; bi = i; } },
             none);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    if (lane == 0) { sh.red[0][wave] = __float_as_uint(bv); sh.ridx[wave] = bi; }
    __syncthreads();
    if (tid == 0) {
      for (int w = 1; w < kWaves; ++w) {
        const float ov = __uint_as_float(sh.red[0][w]);
        const int oi = sh.ridx[w];
        if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
      }
      *out = bi == 0x7fffffff ? 0 : bi;   // all-NaN row: a valid id
    }
    return;
  }
  if (tid < kMaxVec * kWaves) sh.part[tid] = 0.f;
  if (tid == 0) sh.ncand = 0;
  float mx = -INFINITY, mn = INFINITY;
  row.each([&](float l, int) { const float x = l * it; mx = fmaxf(mx, x); mn = fminf(mn, x == -INFINITY ? INFINITY : x); },
           none);
  mx = block_max(mx, sh, buf);
  mn = -block_max(-mn, sh, buf);
  // top-k threshold: the largest th of the search with count(x >= th) >= k
  float th = -FLT_MAX;
  const bool kon = k > 0 && k < V;
  if (kon) {
    float lo = mn, hi = mx;
    _Pragma("unroll 1") for (int r = 0; r < 24; ++r) {
      const float mid = 0.5f * (lo + hi);
      uint32_t c = 0;
      row.each([&](float l, int) { c += l * it >= mid ? 1u : 0u; }, none);
      c = block_count(c, sh, buf);
      if (c >= (uint32_t)k) lo = mid; else hi = mid;
    }
    th = lo;
  }
  if (p > 0.f && p < 1.f) {
    // mass of the top-k survivors, and the survivors into the LDS list where they can fit
    const bool list = kon ? k <= kCand : V <= kCand;
    float z = 0.f;
    row.each([&](float l, int) {
      const float x = l * it;
      if (x >= th) {
        z += __expf(x - mx);
        if (list) {
          const int s = atomicAdd(&sh.ncand, 1);
          if (s < kCand) sh.cand[s] = x;
        }
      }
    }, none);
    z = block_sum(z, sh, buf);
    const int n = sh.ncand;
    // smallest threshold set whose mass >= p * z: bisection on th2 in [th, mx]
    float lo = fmaxf(th, mn), hi = mx;
    if (list && n <= kCand) {
      float cx[kCand / kThreads], ce[kCand / kThreads];
#pragma unroll
      for (int j = 0; j < kCand / kThreads; ++j) {
        cx[j] = j * kThreads + tid < n ? sh.cand[j * kThreads + tid] : -INFINITY;
        ce[j] = __expf(cx[j] - mx);
      }
      _Pragma("unroll 1") for (int r = 0; r < 24; ++r) {
        const float mid = 0.5f * (lo + hi);
        float m = 0.f;
#pragma unroll
        for (int j = 0; j < kCand / kThreads; ++j) m += cx[j] >= mid ? ce[j] : 0.f;
        m = block_sum(m, sh, buf);
        if (m >= p * z) lo = mid; else hi = mid;
      }
    } else {
      _Pragma("unroll 1") for (int r = 0; r < 24; ++r) {
        const float mid = 0.5f * (lo + hi);
        float m = 0.f;
        row.each([&](float l, int) { const float x = l * it; if (x >= mid) m += __expf(x - mx); }, none);
        m = block_sum(m, sh, buf);
        if (m >= p * z) lo = mid; else hi = mid;
      }
    }
    th = fmaxf(th, lo);
  }
  if (mp > 0.f) th = fmaxf(th, mx + logf(fminf(mp, 1.f)));
  // kept mass per (vector, wave) in index order
  {
    float acc = 0.f;
    row.each([&](float l, int) { const float x = l * it; if (x >= th) acc += __expf(x - mx); },
             [&](int u) {
               const float s = wave_sum(acc);
               if (lane == 0) sh.part[u * kWaves + wave] = s;
               acc = 0.f;
             });
  }
  __syncthreads();
  if (wave == 0) {
    // the entry the draw falls in: lane l scans entries 4 l .. 4 l + 3
    constexpr int E = kMaxVec * kWaves / 64;
    float e[E], ls = 0.f;
#pragma unroll
    for (int j = 0; j < E; ++j) { e[j] = sh.part[lane * E + j]; ls += e[j]; }
    const float incl = wave_scan(ls);
    const float z = __shfl(incl, 63, 64);
    const float target = u01 * z;
    const int L = first_or_last(__ballot(incl > target), __ballot(ls > 0.f));
    if (lane == L) {
      float acc = incl - ls;
      int pick = 0;
      float base = acc;
      bool done = false;
#pragma unroll
      for (int j = 0; j < E; ++j) {
        if (!done && e[j] > 0.f) {
          pick = lane * E + j;
          base = acc;
          acc += e[j];
          if (acc > target) done = true;
        }
      }
      sh.sel = pick;
      sh.sel_base = base;
      sh.target = target;
    }
  }
  __syncthreads();
  const int sel = sh.sel;
  if (wave != sel % kWaves) return;
  const int us = sel / kWaves;
  const float rem = sh.target - sh.sel_base;
  float lm = 0.f;
  row.each([&](float l, int) { const float x = l * it; if (x >= th) lm += __expf(x - mx); }, none, us);
  const float incl = wave_scan(lm);
  const int L = first_or_last(__ballot(incl > rem), __ballot(lm > 0.f));
  if (lane == L) {
    float acc = incl - lm;
    int pick = 0;
    bool done = false;
    row.each([&](float l, int i) {
      const float x = l * it;
      if (!done && x >= th) {
        acc += __expf(x - mx);
        pick = i;
        if (acc > rem) done = true;
      }
    }, none, us);
    *out = pick;
  }
}

// MODE 0: bf16 in registers (NV vectors a thread), 1: bf16 from memory, 2: fp32 from memory
template <int MODE, int NV>
__global__ __launch_bounds__(kThreads) void sample_tokens_kernel(
    const void* __restrict__ logits, int V, int ld, const float* __restrict__ inv_temp,
    const int* __restrict__ top_k, const float* __restrict__ top_p, const float* __restrict__ min_p,
    const float* __restrict__ u, const long long* __restrict__ seed, const int* __restrict__ index,
    const int* __restrict__ valid, int64_t* __restrict__ out) {
  __shared__ Shared sh;
  const int row = blockIdx.x;
  if (valid != nullptr && valid[row] == 0) {
    if (threadIdx.x == 0) out[row] = 0;
    return;
  }
  const float u01 = u != nullptr ? u[row] : seeded_u01(seed[row], index[row]);
  const float mp = min_p != nullptr ? min_p[row] : 0.f;
  const size_t off = (size_t)row * ld;
  if constexpr (MODE == 0) {
    RegRow<NV> r(logits, off, V);
    sample_row(r, sh, V, inv_temp[row], top_k[row], top_p[row], mp, u01, out + row);
  } else if constexpr (MODE == 1) {
    MemRow<uint16_t> r(logits, off, V);
    sample_row(r, sh, V, inv_temp[row], top_k[row], top_p[row], mp, u01, out + row);
  } else {
    MemRow<float> r(logits, off, V);
    sample_row(r, sh, V, inv_temp[row], top_k[row], top_p[row], mp, u01, out + row);
  }
}

}  // namespace

int docqa_seeded_uniform(const int64_t* seed, const int* index, float* out, int n, hipStream_t s) {
  if (n == 0) return 0;
  seeded_uniform_kernel<<<(n + 255) / 256, 256, 0, s>>>(reinterpret_cast<const long long*>(seed), index, out, n);
  DOCQA_CHECK_LAUNCH();
  return 0;
}

// logits [rows, ld] bf16 / fp32, columns < n_valid take part; exactly one of u / (seed, index);
// min_p and valid may be null.  Any stride and alignment is served (see the file header).
int docqa_sample_tokens(const void* logits, int rows, int n_valid, int ld, int is_bf16, const float* inv_temp,
                        const int* top_k, const float* top_p, const float* min_p, const float* u,
                        const int64_t* seed, const int* index, const int* valid, int64_t* out, hipStream_t s) {
  if (rows == 0) return 0;
  if (n_valid <= 0 || (rows > 1 && ld < n_valid)) return -1;
  if ((u == nullptr) == (seed == nullptr) || (seed != nullptr && index == nullptr)) return -1;
  const long long* sd = reinterpret_cast<const long long*>(seed);
#define ST(MODE, NV) \
  sample_tokens_kernel<MODE, NV><<<rows, kThreads, 0, s>>>(logits, n_valid, ld, inv_temp, top_k, top_p, min_p, u, \
                                                           sd, index, valid, out)
  if (!is_bf16) {
    ST(2, 1);
  } else if (ld % 8 != 0 || !docqa_aligned16(logits) || n_valid > kThreads * 8 * kMaxVec) {
    ST(1, 1);
  } else {
    const int nv = (n_valid + kThreads * 8 - 1) / (kThreads * 8);
    if (nv <= 1) ST(0, 1);
    else if (nv <= 2) ST(0, 2);
    else if (nv <= 4) ST(0, 4);
    else if (nv <= 8) ST(0, 8);
    else ST(0, 16);
  }
#undef ST
  DOCQA_CHECK_LAUNCH();
  return 0;
}
