// logprobs.hip -- per-token log-probabilities of the LM-head logits (the Ollama API's
// "logprobs" / "top_logprobs"):  logprob(t) = logit[t] - logsumexp(logit[0:n_valid]).
//
//  * logprobs_pass1 : one workgroup per (row, vocab split).  The split's <= 8192 logits are
//                     read ONCE (16-byte loads) into 32 registers per thread; the workgroup
//                     leaves (max, sum exp(x - max)) in fp32 and, for rows that ask for
//                     alternatives, its own top-n as (value, id) pairs: n rounds of "best
//                     element after the previous winner" -- every thread caches its local
//                     best, only the winner's thread rescans its registers, one barrier a round.
//  * logprobs_pass2 : one workgroup per row merges the splits' (max, sum) into the row's
//                     logsumexp, writes the chosen token's logprob and extracts the top-n of
//                     the splits' candidates the same way.
//
// Order: descending value, ties to the lower token id (docqa::argmax_better).  Values are kept
// as (x - max) - log(sum) so that logits of large magnitude lose nothing to the addition
// max + log(sum).  Rows with top_n < 0 are skipped (nothing of theirs is written), top_n == 0
// skips the top-n work.  Logits are expected finite.
#include "docqa_argmax.h"
#include "docqa_common.h"
#include <math.h>

using namespace docqa;

namespace {

constexpr int kTop = 20;            // ops.TOP_LOGPROBS_MAX
constexpr int kPerThread = 32;      // logits a thread of pass 1 holds
constexpr int kChunkMax = 256 * kPerThread;
constexpr int kChunkMin = 1024;
constexpr int kSplitsMax = 128;
constexpr int kCandPerThread = (kSplitsMax * kTop + 255) / 256;
constexpr int kNone = 0x7fffffff;   // id of "no entry" (value -inf)

// (value, id) a comes strictly after (bv, bi) in the output order
__device__ __forceinline__ bool after(float v, int i, float bv, int bi) {
  return v < bv || (v == bv && i > bi);
}

// best (value, id) over the workgroup's 256 threads, returned to every thread.  `buf`
// alternates between rounds, so one barrier per call is enough.
__device__ __forceinline__ void block_best(float& bv, int& bi, float (*sv)[4], int (*si)[4], int buf) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    argmax_better(bv, bi, ov, oi);
  }
  if ((threadIdx.x & 63) == 0) { sv[buf][threadIdx.x >> 6] = bv; si[buf][threadIdx.x >> 6] = bi; }
  __syncthreads();
  bv = sv[buf][0]; bi = si[buf][0];
#pragma unroll
  for (int w = 1; w < 4; ++w) argmax_better(bv, bi, sv[buf][w], si[buf][w]);
}

template <bool BF16>
__global__ __launch_bounds__(256) void logprobs_pass1(const void* __restrict__ logits, int V, int ld, int chunk,
                                                      int splits, const int* __restrict__ top_n,
                                                      float* __restrict__ pm, float* __restrict__ ps,
                                                      float* __restrict__ ptv, int* __restrict__ pti) {
  constexpr int VEC = BF16 ? 8 : 4, U = kPerThread / VEC;
  __shared__ float sv[2][4];
  __shared__ int si[2][4];
  __shared__ float red[8];
  const int row = blockIdx.y, sp = blockIdx.x, tid = threadIdx.x;
  int tn = top_n[row];
  if (tn < 0) return;                      // row-uniform: the whole workgroup leaves
  tn = tn > kTop ? kTop : tn;
  const int lo = sp * chunk, hi = min(V, lo + chunk);
  float v[kPerThread];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int i = lo + (u * 256 + tid) * VEC;
    if constexpr (BF16) {
      // V, ld and chunk are multiples of 8: a vector is wholly inside [lo, hi) or outside
      if (i + VEC <= hi) {
        const uint16_t* r = reinterpret_cast<const uint16_t*>(logits) + (size_t)row * ld;
        unpack8(*reinterpret_cast<const uint4*>(r + i), &v[u * VEC]);
      } else {
#pragma unroll
        for (int j = 0; j < VEC; ++j) v[u * VEC + j] = -INFINITY;
      }
    } else {
      const float* r = reinterpret_cast<const float*>(logits) + (size_t)row * ld;
      if (i + VEC <= hi) {
        const float4 f = *reinterpret_cast<const float4*>(r + i);
        v[u * VEC] = f.x; v[u * VEC + 1] = f.y; v[u * VEC + 2] = f.z; v[u * VEC + 3] = f.w;
      } else {
#pragma unroll
        for (int j = 0; j < VEC; ++j) v[u * VEC + j] = i + j < hi ? r[i + j] : -INFINITY;
      }
    }
  }
  // (max, sum exp(x - max)) of the split; every split holds at least one logit
  float m = -INFINITY;
#pragma unroll
  for (int e = 0; e < kPerThread; ++e) m = fmaxf(m, v[e]);
  m = wave_max(m);
  if ((tid & 63) == 0) red[tid >> 6] = m;
  __syncthreads();
  m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  float s = 0.f;
#pragma unroll
  for (int e = 0; e < kPerThread; ++e) s += __expf(v[e] - m);   // exp(-inf) = 0 past the end
  s = wave_sum(s);
  if ((tid & 63) == 0) red[4 + (tid >> 6)] = s;
  __syncthreads();
  if (tid == 0) {
    pm[row * splits + sp] = m;
    ps[row * splits + sp] = red[4] + red[5] + red[6] + red[7];
  }
  if (tn == 0) return;
  // the split's top-n.  A thread's ids ascend with its register index, so a strict compare
  // keeps the lowest id among equal values.
  float lv = -INFINITY;
  int li = kNone;
#pragma unroll
  for (int e = 0; e < kPerThread; ++e) {
    if (v[e] > lv) { lv = v[e]; li = lo + ((e / VEC) * 256 + tid) * VEC + (e % VEC); }
  }
  // winners wait in LDS and leave in one go, tn threads storing one entry each
  __shared__ float wv[kTop];
  __shared__ int wi[kTop];
  for (int k = 0; k < tn; ++k) {
    float bv = lv;
    int bi = li;
    block_best(bv, bi, sv, si, k & 1);
    if (tid == 0) { wv[k] = bv; wi[k] = bi; }
    if (li == bi && bi != kNone) {         // this thread held the winner: its next best
      lv = -INFINITY;
      li = kNone;
#pragma unroll
      for (int e = 0; e < kPerThread; ++e) {
        const int id = lo + ((e / VEC) * 256 + tid) * VEC + (e % VEC);
        if (after(v[e], id, bv, bi) && v[e] > lv) { lv = v[e]; li = id; }
      }
    }
  }
  __syncthreads();
  if (tid < tn) {
    const size_t o = ((size_t)row * splits + sp) * kTop + tid;
    ptv[o] = wv[tid];
    pti[o] = wi[tid];
  }
}

template <bool BF16>
__global__ __launch_bounds__(256) void logprobs_pass2(const void* __restrict__ logits, int V, int ld, int splits,
                                                      const int64_t* __restrict__ chosen,
                                                      const int* __restrict__ top_n, const float* __restrict__ pm,
                                                      const float* __restrict__ ps, const float* __restrict__ ptv,
                                                      const int* __restrict__ pti, float* __restrict__ lp,
                                                      int* __restrict__ top_ids, float* __restrict__ top_lp) {
  __shared__ float sv[2][4];
  __shared__ int si[2][4];
  __shared__ float red[8];
  const int row = blockIdx.x, tid = threadIdx.x;
  int tn = top_n[row];
  if (tn < 0) return;
  tn = tn > kTop ? kTop : tn;
  // logsumexp of the row from the splits' (max, sum): splits <= kSplitsMax <= 256
  const float mine_m = tid < splits ? pm[row * splits + tid] : -INFINITY;
  float M = wave_max(mine_m);
  if ((tid & 63) == 0) red[tid >> 6] = M;
  __syncthreads();
  M = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  float S = tid < splits ? ps[row * splits + tid] * __expf(mine_m - M) : 0.f;
  S = wave_sum(S);
  if ((tid & 63) == 0) red[4 + (tid >> 6)] = S;
  __syncthreads();
  const float logS = logf(red[4] + red[5] + red[6] + red[7]);
  if (tid == 0) {
    const int64_t c = chosen[row];
    float x = -INFINITY;                   // an id outside [0, V) is never read
    if (c >= 0 && c < (int64_t)V) {
      if constexpr (BF16) x = bf2f(reinterpret_cast<const uint16_t*>(logits)[(size_t)row * ld + c]);
      else x = reinterpret_cast<const float*>(logits)[(size_t)row * ld + c];
    }
    lp[row] = (x - M) - logS;
  }
  if (tid >= tn && tid < kTop) {           // entries past top_n: no entry
    top_ids[(size_t)row * kTop + tid] = -1;
    top_lp[(size_t)row * kTop + tid] = -INFINITY;
  }
  if (tn == 0) return;
  // the splits' candidates, splits x tn of them, kCandPerThread per thread
  const int ncand = splits * tn;
  float cv[kCandPerThread];
  int ci[kCandPerThread];
  float lv = -INFINITY;
  int li = kNone;
#pragma unroll
  for (int c = 0; c < kCandPerThread; ++c) {
    const int q = c * 256 + tid;
    cv[c] = -INFINITY;
    ci[c] = kNone;
    if (q < ncand) {
      const size_t a = ((size_t)row * splits + q / tn) * kTop + q % tn;
      cv[c] = ptv[a];
      ci[c] = pti[a];
    }
    argmax_better(lv, li, cv[c], ci[c]);
  }
  __shared__ float wv[kTop];               // as in pass 1: the winners leave together
  __shared__ int wi[kTop];
  for (int k = 0; k < tn; ++k) {
    float bv = lv;
    int bi = li;
    block_best(bv, bi, sv, si, k & 1);
    if (tid == 0) {
      wi[k] = bi == kNone ? -1 : bi;
      wv[k] = bi == kNone ? -INFINITY : (bv - M) - logS;
    }
    if (li == bi && bi != kNone) {
      lv = -INFINITY;
      li = kNone;
#pragma unroll
      for (int c = 0; c < kCandPerThread; ++c)
        if (after(cv[c], ci[c], bv, bi)) argmax_better(lv, li, cv[c], ci[c]);
    }
  }
  __syncthreads();
  if (tid < tn) {
    top_ids[(size_t)row * kTop + tid] = wi[tid];
    top_lp[(size_t)row * kTop + tid] = wv[tid];
  }
}

}  // namespace

// Vocab splits of a [rows, V] launch and the logits per split (a multiple of 8): 8192-logit
// splits, halved down to 1024 while the grid would leave the 256 CUs short of two workgroups
// each (1 row of 128256: 126 splits; 32 rows: 16 each; 256 rows: 16 each).  0: V too large.
int docqa_token_logprobs_splits(int rows, int V, int* chunk_out) {
  if (rows <= 0 || V <= 0) return 0;
  int chunk = kChunkMax;
  while (chunk > kChunkMin && (int64_t)rows * ((V + chunk - 1) / chunk) < 512 &&
         (V + chunk / 2 - 1) / (chunk / 2) <= kSplitsMax)
    chunk >>= 1;
  const int splits = (V + chunk - 1) / chunk;
  if (splits > kSplitsMax) return 0;
  if (chunk_out) *chunk_out = chunk;
  return splits;
}

int docqa_top_logprobs_max() { return kTop; }

// lp [rows] fp32, top_ids / top_lp [rows, 20]; workspaces pm / ps >= rows * splits floats,
// ptv / pti >= rows * splits * 20, splits from docqa_token_logprobs_splits(rows, n_valid).
int docqa_token_logprobs(const void* logits, int rows, int n_valid, int ld, int is_bf16, const int64_t* chosen,
                         const int* top_n, float* pm, float* ps, float* ptv, int* pti, float* lp, int* top_ids,
                         float* top_lp, hipStream_t s) {
  if (rows == 0) return 0;
  if (n_valid <= 0 || ld < n_valid) return -1;
  if (is_bf16 && (n_valid % 8 != 0 || ld % 8 != 0)) return -1;
  if (!is_bf16 && ld % 4 != 0) return -1;
  if (!docqa_aligned16(logits)) return -1;
  int chunk = 0;
  const int splits = docqa_token_logprobs_splits(rows, n_valid, &chunk);
  if (splits <= 0 || rows > 65535) return -1;
  dim3 g1(splits, rows);
  if (is_bf16) {
    logprobs_pass1<true><<<g1, 256, 0, s>>>(logits, n_valid, ld, chunk, splits, top_n, pm, ps, ptv, pti);
    logprobs_pass2<true><<<rows, 256, 0, s>>>(logits, n_valid, ld, splits, chosen, top_n, pm, ps, ptv, pti, lp,
                                              top_ids, top_lp);
  } else {
    logprobs_pass1<false><<<g1, 256, 0, s>>>(logits, n_valid, ld, chunk, splits, top_n, pm, ps, ptv, pti);
    logprobs_pass2<false><<<rows, 256, 0, s>>>(logits, n_valid, ld, splits, chosen, top_n, pm, ps, ptv, pti, lp,
                                               top_ids, top_lp);
  }
  DOCQA_CHECK_LAUNCH();
  return 0;
}
