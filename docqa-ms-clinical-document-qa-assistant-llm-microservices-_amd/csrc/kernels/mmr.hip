// mmr.hip -- maximal marginal relevance re-selection of a ranked candidate list, one launch
// for a batch (LangChain's `search_type="mmr"` over the retriever of llm-qa/main.py:101;
// the selection rule is langchain_core.vectorstores.utils.maximal_marginal_relevance).
//
// Per query: F <= 64 candidate row ids (best first), of which the first ncand count and
// entries outside [0, N) do not; lam in [0, 1] (negative: the row passes its first k entries
// through).  Similarity is the cosine, all fp32:
//
//   cos(a, b) = dot(a, b) / sqrtf(|a|^2 * |b|^2), 0 when that root is 0
//
// pick 0 maximises cos(q, c); pick t > 0 maximises lam * cos(q, c) - (1 - lam) * red(c) over
// the unpicked candidates, red(c) = max over the picks so far of cos(c, pick); every product
// and the difference rounded on its own; ties to the earlier position.
//
// mmr_kernel (one 256-thread workgroup per query), the mapping:
//   * gather: the candidate rows and the query are staged by 64-column chunks of d into LDS
//     as fp32 (bf16 rows widened), 65 rows of 68 words (a row step of 4 banks: the b128
//     operand reads of 16 lanes cover the 64 banks once).  Thread t loads 8 columns of rows
//     t / 8 and 32 + t / 8; the loads of chunk c + 1 are in flight while chunk c multiplies,
//     two LDS buffers, one barrier per chunk.  Rows that are no candidates stay zero.
//   * products on v_mfma_f32_32x32x2_f32 (an exact fp32 fma chain in k order): wave 0 the
//     Gram tile of candidates (0..31, 0..31), wave 1 (0..31, 32..63), wave 2 (32..63, 32..63)
//     -- the fourth tile is the second one transposed, bit for bit, since both chains run
//     over the same products in the same order -- and wave 3 the query dots, as two tiles
//     whose B operand holds the query in column 0.  One accumulator per tile: the 32x32x2
//     form issues every 64 cycles and its dependent latency is those 64 cycles.  With
//     F <= 32 only wave 0 and the first tile of wave 3 multiply.
//   * the tiles are written as cosines into a [64][65] LDS matrix (both orientations), then
//     wave 0 runs the k greedy rounds: lane i owns candidate i, keeps cos(q, i) and red[i],
//     the argmax over (score, -position) is a 6-step shuffle butterfly.
//   LDS 52.6 KiB static.
#include "docqa_common.h"
#include <math.h>

using namespace docqa;

namespace {

constexpr int MF = 64;                 // candidates per query
constexpr int DC = 64;                 // columns of d per chunk
constexpr int CS = DC + 4;             // chunk row stride (words)
constexpr int GS = MF + 1;             // cosine matrix row stride (words)

// 8 columns of one row: fp32 two 16-byte loads, bf16 one, widened exactly
template <bool BF16>
__device__ __forceinline__ void load8(const void* base, size_t elem, float* v) {
  if constexpr (BF16) {
    unpack8(*reinterpret_cast<const uint4*>(static_cast<const uint16_t*>(base) + elem), v);
  } else {
    const float4* p = reinterpret_cast<const float4*>(static_cast<const float*>(base) + elem);
    const float4 a = p[0], b = p[1];
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
  }
}

__device__ __forceinline__ void zero8(float* v) {
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = 0.f;
}

__device__ __forceinline__ void store8(float* dst, const float* v) {
  *reinterpret_cast<float4*>(dst) = float4{v[0], v[1], v[2], v[3]};
  *reinterpret_cast<float4*>(dst + 4) = float4{v[4], v[5], v[6], v[7]};
}

__device__ __forceinline__ float cosine(float dot, float na, float nb) {
  const float den = sqrtf(na * nb);
  return den > 0.f ? dot / den : 0.f;
}

template <bool BF16>
__global__ __launch_bounds__(256) void mmr_kernel(
    const void* __restrict__ xb, const float* __restrict__ norms, int64_t N, int d,
    const float* __restrict__ xq, const int64_t* __restrict__ cand, int F,
    const int* __restrict__ ncand, const float* __restrict__ lam, int k, float* __restrict__ out_s,
    int64_t* __restrict__ out_i, int* __restrict__ out_p) {
  __shared__ __attribute__((aligned(16))) float sbuf[2][(MF + 1) * CS];
  __shared__ float scos[MF * GS];
  __shared__ float snrm[MF], sqd[MF], sqn[8];
  __shared__ int64_t sid[MF];
  __shared__ int sok[MF];
  const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l32 = lane & 31, hh = lane >> 5;
  const float lm = lam[q];
  float* os = out_s + (size_t)q * k;
  int64_t* oi = out_i + (size_t)q * k;
  int* op = out_p + (size_t)q * k;
  const int64_t* cq = cand + (size_t)q * F;
  if (lm < 0.f) {                      // off: the untouched prefix (k <= F)
    if (tid < k) { os[tid] = 0.f; oi[tid] = cq[tid]; op[tid] = tid; }
    return;
  }
  if (tid < MF) {
    const int nc = min(max(ncand[q], 0), F);
    const int64_t id = tid < F ? cq[tid] : -1;
    const bool ok = tid < nc && id >= 0 && id < N;
    sid[tid] = id;
    sok[tid] = ok;
    snrm[tid] = ok ? norms[id] : 0.f;
  }
  __syncthreads();

  // gather roles: 8 columns (c8) of candidate rows r0 and r0 + 32; threads 0..7 also the query
  const int c8 = (tid & 7) * 8, r0 = tid >> 3;
  const bool ok0 = sok[r0] != 0, ok1 = sok[r0 + 32] != 0;
  const size_t e0 = ok0 ? (size_t)sid[r0] * (size_t)d : 0, e1 = ok1 ? (size_t)sid[r0 + 32] * (size_t)d : 0;
  const float* qrow = xq + (size_t)q * d;
  const bool wide = F > 32;            // candidates 32..63 exist
  float v0[8], v1[8], vq[8], qn = 0.f;
  auto fetch = [&](int c0) {
    const int col = c0 + c8;
    if (ok0 && col < d) load8<BF16>(xb, e0 + col, v0); else zero8(v0);
    if (ok1 && col < d) load8<BF16>(xb, e1 + col, v1); else zero8(v1);
    if (tid < 8) {
      if (col < d) load8<false>(qrow, col, vq); else zero8(vq);
    }
  };
  auto stage = [&](float* buf) {
    store8(buf + r0 * CS + c8, v0);
    store8(buf + (r0 + 32) * CS + c8, v1);
    if (tid < 8) {
      store8(buf + MF * CS + c8, vq);
#pragma unroll
      for (int j = 0; j < 8; ++j) qn = fmaf(vq[j], vq[j], qn);
    }
  };

  f32x16 acc0, acc1;
#pragma unroll
  for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; }
  // operand rows of this wave's tile(s): A rows ra (and ra + 32 for the second query tile)
  const int ra = (wave == 2 ? 32 : 0) + l32;
  const int rb = wave == 3 ? MF : (wave >= 1 ? 32 : 0) + l32;
  const bool active = wave == 0 || wave == 3 || wide;
  const bool bcol = wave != 3 || l32 == 0;        // the query sits in column 0 alone

  const int nchunk = (d + DC - 1) / DC;
  fetch(0);
  stage(sbuf[0]);
  __syncthreads();
  for (int c = 0; c < nchunk; ++c) {
    const bool more = c + 1 < nchunk;
    if (more) fetch((c + 1) * DC);
    if (active) {
      const float* buf = sbuf[c & 1];
      const float* a_row = buf + ra * CS + 4 * hh;
      const float* a2_row = a_row + 32 * CS;
      const float* b_row = buf + rb * CS + 4 * hh;
      const int kend = min(DC, d - c * DC);        // a multiple of 8
      for (int u = 0; u < kend; u += 8) {
        const float4 a4 = *reinterpret_cast<const float4*>(a_row + u);
        float4 b4 = *reinterpret_cast<const float4*>(b_row + u);
        if (!bcol) b4 = float4{0.f, 0.f, 0.f, 0.f};
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.x, b4.x, acc0, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.y, b4.y, acc0, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.z, b4.z, acc0, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.w, b4.w, acc0, 0, 0, 0);
        if (wave == 3 && wide) {
          const float4 c4 = *reinterpret_cast<const float4*>(a2_row + u);
          acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(c4.x, b4.x, acc1, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(c4.y, b4.y, acc1, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(c4.z, b4.z, acc1, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(c4.w, b4.w, acc1, 0, 0, 0);
        }
      }
    }
    if (more) stage(sbuf[(c + 1) & 1]);
    __syncthreads();
  }

  // tiles -> cosines.  acc[r] is (A row (r & 3) + 8 (r >> 2) + 4 hh, B column l32)
  if (tid < 8) sqn[tid] = qn;
  if (wave == 3) {
    if (l32 == 0) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * hh;
        sqd[row] = acc0[r];
        sqd[row + 32] = acc1[r];
      }
    }
  } else if (active) {
    const int ib = wave == 2 ? 32 : 0, jb = wave >= 1 ? 32 : 0;
    const int j = jb + l32;
    const float nj = snrm[j];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int i = ib + (r & 3) + 8 * (r >> 2) + 4 * hh;
      const float cs = cosine(acc0[r], snrm[i], nj);
      scos[i * GS + j] = cs;
      if (wave == 1) scos[j * GS + i] = cs;
    }
  }
  __syncthreads();
  if (wave != 0) return;

  // greedy rounds: lane = candidate position
  float qn2 = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) qn2 += sqn[j];
  bool avail = sok[lane] != 0;
  const float rel = cosine(sqd[lane], qn2, snrm[lane]);
  const float oml = __fsub_rn(1.f, lm);
  const int np = min(k, (int)__popcll(__ballot(avail)));
  float red = 0.f;
  for (int t = 0; t < np; ++t) {
    const float sc = t == 0 ? rel : __fsub_rn(__fmul_rn(lm, rel), __fmul_rn(oml, red));
    bool ba = avail;
    float bs = sc;
    int bi = lane;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const bool xa = __shfl_xor((int)ba, o, 64) != 0;
      const float xs = __shfl_xor(bs, o, 64);
      const int xi = __shfl_xor(bi, o, 64);
      if (xa && (!ba || xs > bs || (xs == bs && xi < bi))) { ba = xa; bs = xs; bi = xi; }
    }
    const int p = __builtin_amdgcn_readfirstlane(bi);
    const float ps = __shfl(sc, p, 64);
    if (lane == 0) { os[t] = ps; oi[t] = sid[p]; op[t] = p; }
    if (lane == p) avail = false;
    const float cp = scos[p * GS + lane];
    red = t == 0 ? cp : fmaxf(red, cp);
  }
  for (int i = np + lane; i < k; i += 64) { os[i] = 0.f; oi[i] = -1; op[i] = -1; }
}

}  // namespace

// xb [N, d] fp32 or bf16 (is_bf16), norms fp32 [N], xq fp32 [nq, d], cand int64 [nq, F], ncand
// int32 [nq], lam fp32 [nq] -> out_s fp32 / out_i int64 / out_p int32 [nq, k].  -1: outside
// 1 <= k <= F <= 64, d % 8 (fp32) / d % 16 (bf16), 16-byte aligned xb and xq.
int docqa_mmr_select(const void* xb, const float* norms, int64_t N, int d, int is_bf16, const float* xq,
                     const int64_t* cand, int F, const int* ncand, const float* lam, int nq, int k,
                     float* out_s, int64_t* out_i, int* out_p, hipStream_t s) {
  if (nq == 0) return 0;
  if (k < 1 || k > F || F > MF || d <= 0 || d % (is_bf16 ? 16 : 8) != 0 || N < 0) return -1;
  if ((N > 0 && !docqa_aligned16(xb)) || !docqa_aligned16(xq)) return -1;
  if (is_bf16)
    mmr_kernel<true><<<nq, 256, 0, s>>>(xb, norms, N, d, xq, cand, F, ncand, lam, k, out_s, out_i, out_p);
  else
    mmr_kernel<false><<<nq, 256, 0, s>>>(xb, norms, N, d, xq, cand, F, ncand, lam, k, out_s, out_i, out_p);
  DOCQA_CHECK_LAUNCH();
  return 0;
}
