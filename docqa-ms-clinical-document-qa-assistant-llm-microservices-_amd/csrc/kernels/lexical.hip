// lexical.hip -- brute-force BM25 scan over CSR term columns with the top-k fused into it,
// and the rank fusion of a dense and a lexical hit list (reciprocal rank fusion).
//
// Extension: the reference has no keyword search.  Columns: index/lexical.py (row_ptr int64
// [N+1], terms int32 [E] = 32-bit term hashes, unique and ascending (unsigned) within a row,
// tfs uint8 [E], dl int32 [N]); query rows: 32 (term, weight) slots, 0xFFFFFFFF pads.
//
//   K_r   = k1 * ((1 - b) + (b * dl_r) / avgdl)
//   s_q,r = sum over the row's entries, in entry order, of  w_q,t * (tf / (tf + K_r))
//
// all fp32, every operation rounded on its own (no fused multiply-add), Lucene >= 8 BM25
// (no (k1 + 1) factor).  A row competes for query q iff it holds one of q's terms and
// passes q's scope row (docqa_scope.h); score descending, ties towards the lower row.
// A term repeated inside one query row counts once (its first slot).
//
// bm25_tile_kernel (grid: row blocks x groups of 32 queries, 256 threads), the mapping:
//   * setup: the group's <= 1024 (query, slot) pairs go into an open-addressing LDS table
//     term -> chain of pairs (2048 keys, the padding key = empty, so a row entry equal to
//     the padding key misses); a pair's weight sits beside it.
//   * per 256-row tile, phase 1: one lane owns one row and walks its entries in order; a
//     table hit walks the term's chain and adds w * tf/(tf+K) into cell [query][row] of a
//     [32][256] fp32 LDS tile.  One writer per cell, the first hit stores instead of adds:
//     no atomics, no zeroing, and the sum order of a (query, row) pair is the row's entry
//     order -- rows with identical entries and dl get bit-identical scores.  The lane
//     then clears the bits of the queries whose scope its row fails (hit queries only).
//   * phase 2: thread (q = tid & 31, s = tid >> 5) scans rows 32 s .. 32 s + 31 of the
//     tile for query q (row stride 257 words: conflict-free for both phases) into its
//     register top-K list (negated scores, topk_insert).
//   * end: the 8 lists of a query merge through LDS (a few queries per round, the tile's
//     space reused) into one top-K per (query, row block) -> workspace; the second launch
//     is topk_merge_kernel<K, true> unchanged (it flips the sign back, -FLT_MAX / -1 pad).
//   LDS 63104 B (61.6 KiB) static: two workgroups per CU.
//
// rank_fuse_kernel: one wave per query; each lane holds one entry of either list, finds its
// partner in the other list by shuffles, and ranks itself among all candidates with exact
// rational compares (cross-multiplied in int64).
#include "docqa_common.h"
#include "docqa_scope.h"
#include "docqa_topk.h"
#include <float.h>

using namespace docqa;

int docqa_knn_kpad(int k);             // knn.hip: k padded to 4 / 8 / 16 / 32 / 64, -1 above

namespace {

constexpr int QG = 32;                // queries per workgroup
constexpr int QT = 32;                 // term slots per query
constexpr int TR = 256;                // rows per tile = threads
constexpr int TSTRIDE = TR + 1;        // tile row stride (words)
constexpr int HSLOTS = 2048;           // hash table keys (>= 2 x QG x QT)
constexpr uint32_t EMPTY = 0xffffffffu;

__device__ __forceinline__ int term_slot(uint32_t t) { return (int)((t * 0x9E3779B1u) >> 21); }

template <int K, bool SCOPED>
__global__ __launch_bounds__(256) void bm25_tile_kernel(
    const int64_t* __restrict__ row_ptr, const uint32_t* __restrict__ terms,
    const uint8_t* __restrict__ tfs, const int* __restrict__ dl, int N,
    const uint32_t* __restrict__ qterms, const float* __restrict__ qweights, int nq, float k1,
    float b, float one_minus_b, float avgdl, int rows_per_block, float* __restrict__ ws_d,
    int* __restrict__ ws_i, int nblk, const int* __restrict__ tags, const int* __restrict__ days,
    const int4* __restrict__ scope) {
  __shared__ uint32_t s_key[HSLOTS];
  __shared__ int s_head[HSLOTS];
  __shared__ int s_next[QG * QT];
  __shared__ uint32_t s_term[QG * QT];
  __shared__ float s_w[QG * QT];
  __shared__ int4 s_scope[QG];
  __shared__ uint32_t s_mask[TR];
  __shared__ float s_tile[QG * TSTRIDE];

  const int blk = blockIdx.x, q0 = blockIdx.y * QG, tid = threadIdx.x;

  // ---- setup: the group's (query, slot) pairs -> hash table with chains
  for (int i = tid; i < HSLOTS; i += 256) { s_key[i] = EMPTY; s_head[i] = -1; }
  for (int p = tid; p < QG * QT; p += 256) {
    const int q = q0 + (p >> 5);
    s_term[p] = q < nq ? qterms[(size_t)q * QT + (p & 31)] : EMPTY;
    s_w[p] = q < nq ? qweights[(size_t)q * QT + (p & 31)] : 0.f;
  }
  if constexpr (SCOPED) {
    if (tid < QG) s_scope[tid] = (q0 + tid < nq) ? scope[q0 + tid] : make_int4(0, 0, 0, 0);
  }
  __syncthreads();
  for (int p = tid; p < QG * QT; p += 256) {
    const uint32_t t = s_term[p];
    bool use = t != EMPTY;
    for (int j = p & ~31; j < p && use; ++j) use = s_term[j] != t;   // a repeated term counts once
    if (use) {
      int h = term_slot(t);
      for (;;) {
        const uint32_t prev = atomicCAS(&s_key[h], EMPTY, t);
        if (prev == EMPTY || prev == t) break;
        h = (h + 1) & (HSLOTS - 1);
      }
      // chain order is arbitrary: the pairs of one term belong to different queries
      s_next[p] = atomicExch(&s_head[h], p);
    }
  }
  __syncthreads();

  float td[K];
  int ti[K];
#pragma unroll
  for (int i = 0; i < K; ++i) { td[i] = FLT_MAX; ti[i] = -1; }

  // in 64 bits: at N near 2^31 the last blocks' blk * rows_per_block (+ rows_per_block) pass 2^31
  const int64_t rb64 = (int64_t)blk * rows_per_block;
  const int row_begin = (int)(rb64 < N ? rb64 : N);
  const int row_end = (int)(rb64 + rows_per_block < N ? rb64 + rows_per_block : N);
  const int pq = tid & 31, ps = tid >> 5;        // phase 2: query, 32-row slice

  for (int tile = row_begin; tile < row_end; tile += TR) {
    // ---- phase 1: this lane's row
    const int row = tile + tid;
    uint32_t mask = 0;
    if (row < row_end) {
      const int64_t e0 = row_ptr[row], e1 = row_ptr[row + 1];
      if (e1 > e0) {
        const float Kr = __fmul_rn(k1, __fadd_rn(one_minus_b, __fdiv_rn(__fmul_rn(b, (float)dl[row]), avgdl)));
        for (int64_t e = e0; e < e1; ++e) {
          const uint32_t t = terms[e];
          int h = term_slot(t);
          uint32_t kk;
          while ((kk = s_key[h]) != t && kk != EMPTY) h = (h + 1) & (HSLOTS - 1);
          if (kk == t && t != EMPTY) {
            const float tf = (float)tfs[e];
            const float x = __fdiv_rn(tf, __fadd_rn(tf, Kr));
            for (int p = s_head[h]; p >= 0; p = s_next[p]) {
              const int q = p >> 5;
              const float c = __fmul_rn(s_w[p], x);
              float* cell = &s_tile[q * TSTRIDE + tid];
              *cell = ((mask >> q) & 1u) ? __fadd_rn(*cell, c) : c;
              mask |= 1u << q;
            }
          }
        }
        if constexpr (SCOPED) {
          if (mask) {
            const int rt = tags[row], rd = days[row];
            for (uint32_t m = mask; m; m &= m - 1) {
              const int q = __ffs(m) - 1;
              if (!scope_match(s_scope[q], rt, rd)) mask &= ~(1u << q);
            }
          }
        }
      }
    }
    s_mask[tid] = mask;
    __syncthreads();
    // ---- phase 2: query pq over rows 32 ps .. 32 ps + 31 of the tile, ascending
    for (int i = 0; i < 32; ++i) {
      const int r = ps * 32 + i;
      if ((s_mask[r] >> pq) & 1u) {
        const float v = -s_tile[pq * TSTRIDE + r];
        if (v < td[K - 1]) topk_insert<K>(td, ti, v, tile + r);
      }
    }
    __syncthreads();
  }

  // ---- merge the 8 lists per query through LDS (the tile's space), QPR queries per round
  constexpr int QPR = (QG * TSTRIDE) / (16 * K) >= QG ? QG : (QG * TSTRIDE) / (16 * K);
  static_assert(QPR >= 1 && QG % QPR == 0, "merge rounds");
  float* md = s_tile;                                           // [QPR][8 lists][K]
  int* mi = reinterpret_cast<int*>(s_tile) + QPR * 8 * K;
  for (int base = 0; base < QG; base += QPR) {
    if (pq >= base && pq < base + QPR) {
#pragma unroll
      for (int i = 0; i < K; ++i) {
        md[((pq - base) * 8 + ps) * K + i] = td[i];
        mi[((pq - base) * 8 + ps) * K + i] = ti[i];
      }
    }
    __syncthreads();
    if (tid < QPR && q0 + base + tid < nq) {
      const int q = tid;
      int head[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) head[j] = 0;
      const size_t ob = ((size_t)(q0 + base + q) * nblk + blk) * K;
      for (int i = 0; i < K; ++i) {
        int best = 0;
        float bd = FLT_MAX;
        int bi = 0x7fffffff;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          if (head[j] < K) {
            const float v = md[(q * 8 + j) * K + head[j]];
            const int id = mi[(q * 8 + j) * K + head[j]];
            if (v < bd || (v == bd && id < bi)) { bd = v; bi = id; best = j; }
          }
        }
        head[best]++;
        ws_d[ob + i] = bd;
        ws_i[ob + i] = bd == FLT_MAX ? -1 : bi;
      }
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------ rank fusion
// a candidate: score num / den (den > 0; num = 0: none) and id
struct Cand { int64_t num, den, id; };

__device__ __forceinline__ int64_t shfl64(int64_t v, int src) {
  const int lo = __shfl((int)(uint32_t)(uint64_t)v, src, 64);
  const int hi = __shfl((int)(uint32_t)((uint64_t)v >> 32), src, 64);
  return (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
}

// does `o` come before `m`?  score descending (exact rationals), ties to the lower id
__device__ __forceinline__ bool cand_before(const Cand& o, const Cand& m) {
  const int64_t l = o.num * m.den, r = m.num * o.den;
  return l > r || (l == r && o.id < m.id);
}

__global__ __launch_bounds__(64) void rank_fuse_kernel(
    const int64_t* __restrict__ i_dense, int ld, const int64_t* __restrict__ i_lex, int ll,
    const int* __restrict__ mode, int k, int c, float* __restrict__ out_f,
    int64_t* __restrict__ out_i) {
  const int q = blockIdx.x, lane = threadIdx.x;
  const int md = mode[q];
  int64_t a_id = (lane < ld && md != 1) ? i_dense[(size_t)q * ld + lane] : -1;
  int64_t b_id = (lane < ll && md != 0) ? i_lex[(size_t)q * ll + lane] : -1;
  if (a_id < 0) a_id = -1;
  if (b_id < 0) b_id = -1;
  const int64_t rk = (int64_t)c + lane + 1;      // this lane's rank term in either list
  // partner of the dense entry in the lexical list (first occurrence), repeats within a list
  int a_partner = -1;
  bool a_dup = false, b_dup = false, b_in_a = false;
  for (int j = 0; j < 64; ++j) {
    const int64_t oa = shfl64(a_id, j), ob = shfl64(b_id, j);
    if (a_id >= 0) {
      if (ob == a_id && a_partner < 0) a_partner = j;
      if (oa == a_id && j < lane) a_dup = true;
    }
    if (b_id >= 0) {
      if (oa == b_id) b_in_a = true;
      if (ob == b_id && j < lane) b_dup = true;
    }
  }
  Cand ca{0, 1, -1}, cb{0, 1, -1};
  if (a_id >= 0 && !a_dup) {
    if (a_partner >= 0) {
      const int64_t rb = (int64_t)c + a_partner + 1;
      ca = Cand{rk + rb, rk * rb, a_id};
    } else {
      ca = Cand{1, rk, a_id};
    }
  }
  if (b_id >= 0 && !b_dup && !b_in_a) cb = Cand{1, rk, b_id};
  int ra = 0, rb = 0, total = 0;
  for (int j = 0; j < 64; ++j) {
    Cand oa{shfl64(ca.num, j), shfl64(ca.den, j), shfl64(ca.id, j)};
    Cand ob{shfl64(cb.num, j), shfl64(cb.den, j), shfl64(cb.id, j)};
    if (oa.num > 0) { ++total; ra += cand_before(oa, ca); rb += cand_before(oa, cb); }
    if (ob.num > 0) { ++total; ra += cand_before(ob, ca); rb += cand_before(ob, cb); }
  }
  float* of = out_f + (size_t)q * k;
  int64_t* oi = out_i + (size_t)q * k;
  if (ca.num > 0 && ra < k) { of[ra] = (float)ca.num / (float)ca.den; oi[ra] = ca.id; }
  if (cb.num > 0 && rb < k) { of[rb] = (float)cb.num / (float)cb.den; oi[rb] = cb.id; }
  for (int i = total + lane; i < k; i += 64) { of[i] = 0.f; oi[i] = -1; }
}

template <int K>
int launch_bm25(const int64_t* row_ptr, const int* terms, const uint8_t* tfs, const int* dl, int N,
                const int* qterms, const float* qweights, int nq, int k, float k1, float b,
                float one_minus_b, float avgdl, const int* tags, const int* days, const int* scope,
                float* ws_d, int* ws_i, int nblk, float* out_s, int64_t* out_i, int64_t id_offset,
                hipStream_t s) {
  int rpb = (N + nblk - 1) / nblk;
  rpb = (rpb + TR - 1) / TR * TR;
  dim3 g1(nblk, (nq + QG - 1) / QG);
  const uint32_t* t = reinterpret_cast<const uint32_t*>(terms);
  const uint32_t* qt = reinterpret_cast<const uint32_t*>(qterms);
  if (scope)
    bm25_tile_kernel<K, true><<<g1, 256, 0, s>>>(row_ptr, t, tfs, dl, N, qt, qweights, nq, k1, b, one_minus_b,
                                                 avgdl, rpb, ws_d, ws_i, nblk, tags, days,
                                                 reinterpret_cast<const int4*>(scope));
  else
    bm25_tile_kernel<K, false><<<g1, 256, 0, s>>>(row_ptr, t, tfs, dl, N, qt, qweights, nq, k1, b, one_minus_b,
                                                  avgdl, rpb, ws_d, ws_i, nblk, nullptr, nullptr, nullptr);
  topk_merge_kernel<K, true><<<nq, 256, topk_merge_lds(K), s>>>(ws_d, ws_i, nblk, nullptr, 0, k, out_s, out_i,
                                                                id_offset, nullptr);
  DOCQA_CHECK_LAUNCH();
  return 0;
}

}  // namespace

// one workspace list per (query, row block): >= 256 rows per block, at most 1024 blocks
int docqa_bm25_workspace_blocks(int N) {
  int nblk = (N + TR - 1) / TR;
  if (nblk > 1024) nblk = 1024;
  return nblk < 1 ? 1 : nblk;
}

// ws_d / ws_i: [nq, nblk, docqa_knn_kpad(k)]; scope (with tags, days) may be null; scope is
// 16-byte aligned.  -1: k outside 1..64 or no rows.
int docqa_bm25_topk(const int64_t* row_ptr, const int* terms, const uint8_t* tfs, const int* dl, int N,
                    const int* qterms, const float* qweights, int nq, int k, float k1, float b,
                    float one_minus_b, float avgdl, const int* tags, const int* days, const int* scope,
                    float* ws_d, int* ws_i, int nblk, float* out_s, int64_t* out_i, int64_t id_offset,
                    hipStream_t s) {
  if (nq == 0) return 0;
  if (N <= 0) return -1;
#define BM25_CASE(KK)                                                                                  \
  case KK:                                                                                             \
    return launch_bm25<KK>(row_ptr, terms, tfs, dl, N, qterms, qweights, nq, k, k1, b, one_minus_b,    \
                           avgdl, tags, days, scope, ws_d, ws_i, nblk, out_s, out_i, id_offset, s);
  switch (docqa_knn_kpad(k)) {
    BM25_CASE(4)
    BM25_CASE(8)
    BM25_CASE(16)
    BM25_CASE(32)
    BM25_CASE(64)
    default: return -1;
  }
#undef BM25_CASE
}

// i_dense [nq, ld], i_lex [nq, ll] (ld, ll <= 64; negative ids are ignored), mode int32 [nq]
// (0 dense, 1 lexical, 2 reciprocal rank fusion), out_f / out_i [nq, k].  -1: outside that.
int docqa_rank_fuse(const int64_t* i_dense, int ld, const int64_t* i_lex, int ll, const int* mode, int nq,
                    int k, int c, float* out_f, int64_t* out_i, hipStream_t s) {
  if (nq == 0) return 0;
  if (ld < 0 || ld > 64 || ll < 0 || ll > 64 || k < 1 || c < 0 || c > 100000) return -1;
  rank_fuse_kernel<<<nq, 64, 0, s>>>(i_dense, ld, i_lex, ll, mode, k, c, out_f, out_i);
  DOCQA_CHECK_LAUNCH();
  return 0;
}
