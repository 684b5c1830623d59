// compact.hip -- exact, deterministic compaction kernels for deleting rows from the vector
// store (index/flat.py remove_ids and the columns kept beside the vectors).
//
//   masked scan    pos[r] = sum_{i<r} (keep[i] ? w[i] : 0), int64 [n+1], w = 1 without weights
//   row gather     dst[pos[r]] = src[r] for kept rows of W bytes, out of place
//   CSR gather     new row_ptr + the entries of kept rows (terms 4 B, tfs 1 B per entry)
//   id remap       ids'[j] = pos[ids[j]] over an id list that is already compacted
//
// Everything is copying and integer sums: bit-exact, no atomics, no float, the same result on
// every run.  All index arithmetic is int64 (a 10M x 384 fp32 store is 15 GB; the CSR of a
// large corpus passes 2^31 bytes long before it passes 2^31 entries).
//
// The scan is reduce-then-scan: per-tile sums, a scan of the tile sums, per-tile
// finalisation, with one more level of the same two kernels whenever the tile sums outgrow
// one workgroup (three levels cover kScanTile^3 = 2^30 rows).  It costs 1 / 3 / 5 launches
// where a decoupled look-back scan costs one, and that is deliberate: NO WORKGROUP WAITS ON
// ANOTHER WORKGROUP here -- no flag spin, no cooperative launch -- so nothing in this file
// can hang, whatever the scheduler does.  The extra launches are microseconds against a move
// of milliseconds.
//
// The gather is a pure streaming copy, bound by HBM (MI355X_MICROARCH.md: ~10 B/cycle/CU for
// global_load_dwordx4).  Load / store forms chosen, and why:
//   * plain 16-byte global_load_dwordx4 / global_store_dwordx4 per lane whenever W and both
//     bases are multiples of 16 (vectors, PQ codes with M % 16 == 0): the widest form, 4x
//     fewer memory instructions than dwords, and a wave-instruction covers 1 KiB contiguous
//     in the source (the destination is contiguous too, except across a removed run);
//   * else 4-byte lanes (norms, tags, days, dl, ids as two lanes, W = 6 falls through), else
//     bytes.  Narrow rows move 1000x fewer bytes than the vectors, so their rate is noise;
//   * no nt / sc1 modifiers: on this chip nt loads only bypass the L1 (0-3 % slower at 16 B)
//     and every store flavour leaves L2 at the same rate, so there is nothing to gain; the
//     keep / pos words, which the lanes of a row share, do hit the L1 with plain loads;
//   * no LDS staging: nothing is reused or transposed;
//   * each thread issues kUnroll independent loads before its stores, a grid capped at
//     kMaxBlocks workgroups strides over the rest (cdna_hip_programming.md Guideline 11).
// A destination index is written only when it is inside the destination (`dst_rows`,
// `e_cap`), so a wrong `pos` from a caller cannot write out of bounds.
#include "docqa_common.h"
#include "docqa_kernels.h"

namespace {

constexpr int kBlock = 256;
constexpr int kScanItems = 4;
constexpr int kScanTile = kBlock * kScanItems;        // 1024 values per workgroup
constexpr int kUnroll = 4;
constexpr int kChunk = kBlock * kUnroll;              // lane units per workgroup iteration
constexpr int kMaxBlocks = 8192;

// value r of a scan level: level 0 reads the mask (and weights), upper levels int64 sums
template <bool MASK>
__device__ __forceinline__ int64_t scan_value(const uint8_t* keep, const int64_t* w, int64_t r) {
  if constexpr (MASK) return keep[r] ? (w ? w[r] : int64_t(1)) : int64_t(0);
  else return w[r];
}

// block-wide sum of one int64 per thread; the result is valid in every thread
__device__ __forceinline__ int64_t block_sum(int64_t v, int64_t* sm) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  __syncthreads();
  if (lane == 0) sm[wave] = v;
  __syncthreads();
  return sm[0] + sm[1] + sm[2] + sm[3];
}

// sums[t] = sum of the values of tile t
template <bool MASK>
__global__ __launch_bounds__(kBlock) void scan_reduce_kernel(const uint8_t* __restrict__ keep,
                                                             const int64_t* __restrict__ w, int64_t n,
                                                             int64_t* __restrict__ sums) {
  __shared__ int64_t sm[kBlock / 64];
  const int64_t base = int64_t(blockIdx.x) * kScanTile + int64_t(threadIdx.x) * kScanItems;
  int64_t v = 0;
#pragma unroll
  for (int i = 0; i < kScanItems; ++i)
    if (base + i < n) v += scan_value<MASK>(keep, w, base + i);
  v = block_sum(v, sm);
  if (threadIdx.x == 0) sums[blockIdx.x] = v;
}

// out[r] = offs[tile] + exclusive prefix inside the tile (offs == nullptr: 0); the workgroup of
// the last tile also writes out[n] = the total.  n == 0: one workgroup writes out[0] = 0.
template <bool MASK>
__global__ __launch_bounds__(kBlock) void scan_tile_kernel(const uint8_t* __restrict__ keep,
                                                           const int64_t* __restrict__ w, int64_t n,
                                                           const int64_t* __restrict__ offs,
                                                           int64_t* __restrict__ out) {
  __shared__ int64_t sm[kBlock / 64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t base = int64_t(blockIdx.x) * kScanTile + int64_t(threadIdx.x) * kScanItems;
  int64_t x[kScanItems];
  int64_t t = 0;
#pragma unroll
  for (int i = 0; i < kScanItems; ++i) {
    x[i] = base + i < n ? scan_value<MASK>(keep, w, base + i) : int64_t(0);
    t += x[i];
  }
  // inclusive scan of the thread sums inside the wave, then the wave totals through LDS
  int64_t inc = t;
  for (int o = 1; o < 64; o <<= 1) {
    const int64_t y = __shfl_up(inc, o, 64);
    if (lane >= o) inc += y;
  }
  if (lane == 63) sm[wave] = inc;
  __syncthreads();
  int64_t run = offs ? offs[blockIdx.x] : int64_t(0);
  for (int i = 0; i < wave; ++i) run += sm[i];
  run += inc - t;
#pragma unroll
  for (int i = 0; i < kScanItems; ++i) {
    if (base + i < n) out[base + i] = run;
    run += x[i];
  }
  // the thread whose items end the array holds the grand total
  const int64_t last = n > 0 ? n - 1 : 0;
  if (n == 0) {
    if (blockIdx.x == 0 && threadIdx.x == 0) out[0] = 0;
  } else if (base <= last && last < base + kScanItems) {
    out[n] = run;
  }
}

// lane units of T (16 / 4 / 1 bytes), L per row: unit u of the flattened source belongs to row
// u / L.  A workgroup iteration covers kChunk consecutive units: one 64-bit division per
// workgroup iteration (uniform), 32-bit divisions per lane.
template <typename T>
__global__ __launch_bounds__(kBlock) void gather_rows_kernel(const T* __restrict__ src, T* __restrict__ dst,
                                                             const uint8_t* __restrict__ keep,
                                                             const int64_t* __restrict__ pos, int64_t n,
                                                             uint32_t L, int64_t dst_rows) {
  const int64_t total = n * int64_t(L);
  const int64_t nchunks = (total + kChunk - 1) / kChunk;
  for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const int64_t u0 = c * kChunk;
    const int64_t r0 = u0 / L;
    const uint32_t l0 = uint32_t(u0 - r0 * L);
    T v[kUnroll];
    int64_t d[kUnroll];
#pragma unroll
    for (int i = 0; i < kUnroll; ++i) {
      const uint32_t j = uint32_t(i) * kBlock + threadIdx.x;        // unit inside the chunk
      d[i] = -1;
      if (u0 + j < total) {
        const uint32_t q = l0 + j;                                  // < L + kChunk < 2^32
        const uint32_t dr = q / L, l = q - dr * L;
        const int64_t r = r0 + dr;
        if (keep[r]) {
          const int64_t p = pos[r];
          if (p >= 0 && p < dst_rows) {
            d[i] = p * int64_t(L) + l;
            v[i] = src[u0 + j];
          }
        }
      }
    }
#pragma unroll
    for (int i = 0; i < kUnroll; ++i)
      if (d[i] >= 0) dst[d[i]] = v[i];
  }
}

// 16 lanes per row: new_ptr[pos[r]] = epos[r], entries row_ptr[r] .. row_ptr[r+1] copied to
// epos[r] ..; row n (one past the end) closes the new row_ptr.  terms / tfs may be null.
constexpr int kRowLanes = 16;
__global__ __launch_bounds__(kBlock) void csr_gather_kernel(const int64_t* __restrict__ row_ptr,
                                                            const uint8_t* __restrict__ keep,
                                                            const int64_t* __restrict__ pos,
                                                            const int64_t* __restrict__ epos, int64_t n,
                                                            const int* __restrict__ terms,
                                                            const uint8_t* __restrict__ tfs, int64_t e_in,
                                                            int64_t* __restrict__ new_ptr, int64_t ptr_rows,
                                                            int* __restrict__ new_terms,
                                                            uint8_t* __restrict__ new_tfs, int64_t e_cap) {
  const int sub = threadIdx.x % kRowLanes;
  const int64_t rows_per_block = kBlock / kRowLanes;
  const int64_t nb = (n + 1 + rows_per_block - 1) / rows_per_block;
  for (int64_t b = blockIdx.x; b < nb; b += gridDim.x) {
    const int64_t r = b * rows_per_block + threadIdx.x / kRowLanes;
    if (r > n) continue;
    if (r == n) {
      const int64_t p = pos[n];
      if (sub == 0 && p >= 0 && p < ptr_rows) new_ptr[p] = epos[n];
      continue;
    }
    if (!keep[r]) continue;
    const int64_t p = pos[r], e0 = epos[r];
    if (sub == 0 && p >= 0 && p < ptr_rows) new_ptr[p] = e0;
    const int64_t a = row_ptr[r], z = row_ptr[r + 1];
    if (a < 0 || z > e_in || e0 < 0) continue;
    for (int64_t i = a + sub; i < z; i += kRowLanes) {
      const int64_t o = e0 + (i - a);
      if (o < e_cap) {
        if (terms) new_terms[o] = terms[i];
        if (tfs) new_tfs[o] = tfs[i];
      }
    }
  }
}

__global__ __launch_bounds__(kBlock) void remap_ids_kernel(const int64_t* __restrict__ ids, int64_t m,
                                                           const int64_t* __restrict__ pos, int64_t n,
                                                           int64_t* __restrict__ out) {
  for (int64_t j = int64_t(blockIdx.x) * kBlock + threadIdx.x; j < m; j += int64_t(gridDim.x) * kBlock) {
    const int64_t i = ids[j];
    out[j] = (i >= 0 && i < n) ? pos[i] : int64_t(-1);
  }
}

inline int64_t tiles(int64_t n) { return (n + kScanTile - 1) / kScanTile; }
inline int grid_for(int64_t blocks) { return int(blocks < 1 ? 1 : (blocks > kMaxBlocks ? kMaxBlocks : blocks)); }

template <typename T>
int launch_gather(const void* src, void* dst, const uint8_t* keep, const int64_t* pos, int64_t n, int64_t W,
                  int64_t dst_rows, hipStream_t s) {
  const uint32_t L = uint32_t(W / int64_t(sizeof(T)));
  const int64_t chunks = (n * int64_t(L) + kChunk - 1) / kChunk;
  gather_rows_kernel<T><<<grid_for(chunks), kBlock, 0, s>>>(static_cast<const T*>(src), static_cast<T*>(dst), keep,
                                                            pos, n, L, dst_rows);
  DOCQA_CHECK_LAUNCH();
  return 0;
}

}  // namespace

int docqa_compact_scan_tile() { return kScanTile; }
int docqa_compact_scan_levels() { return 3; }

// int64 words of workspace the scan of n values needs (the tile sums and their scans)
int64_t docqa_masked_scan_workspace(int64_t n) {
  const int64_t t1 = tiles(n), t2 = tiles(t1);
  return 2 * (t1 + 1) + 2 * (t2 + 1);
}

// keep uint8 [n], w int64 [n] or null -> pos int64 [n+1].  -1: n outside [0, kScanTile^3].
int docqa_masked_scan(const uint8_t* keep, const int64_t* w, int64_t n, int64_t* pos, int64_t* ws,
                      hipStream_t s) {
  const int64_t cap = int64_t(kScanTile) * kScanTile * kScanTile;
  if (n < 0 || n > cap) return -1;
  const int64_t t1 = tiles(n), t2 = tiles(t1);
  if (t1 <= 1) {
    scan_tile_kernel<true><<<1, kBlock, 0, s>>>(keep, w, n, nullptr, pos);
    DOCQA_CHECK_LAUNCH();
    return 0;
  }
  int64_t* s1 = ws;                  // [t1] tile sums
  int64_t* e1 = s1 + (t1 + 1);       // [t1 + 1] their exclusive scan
  int64_t* s2 = e1 + (t1 + 1);       // [t2]
  int64_t* e2 = s2 + (t2 + 1);       // [t2 + 1]
  scan_reduce_kernel<true><<<int(t1), kBlock, 0, s>>>(keep, w, n, s1);
  DOCQA_CHECK_LAUNCH();
  if (t2 <= 1) {
    scan_tile_kernel<false><<<1, kBlock, 0, s>>>(nullptr, s1, t1, nullptr, e1);
    DOCQA_CHECK_LAUNCH();
  } else {
    scan_reduce_kernel<false><<<int(t2), kBlock, 0, s>>>(nullptr, s1, t1, s2);
    DOCQA_CHECK_LAUNCH();
    scan_tile_kernel<false><<<1, kBlock, 0, s>>>(nullptr, s2, t2, nullptr, e2);     // t2 <= kScanTile
    DOCQA_CHECK_LAUNCH();
    scan_tile_kernel<false><<<int(t2), kBlock, 0, s>>>(nullptr, s1, t1, e2, e1);
    DOCQA_CHECK_LAUNCH();
  }
  scan_tile_kernel<true><<<int(t1), kBlock, 0, s>>>(keep, w, n, e1, pos);
  DOCQA_CHECK_LAUNCH();
  return 0;
}

// dst[pos[r]] = src[r] for kept rows of W bytes; dst holds dst_rows rows and never aliases src.
// -1: W outside [1, 2^20] or n < 0.
int docqa_gather_rows(const void* src, void* dst, const uint8_t* keep, const int64_t* pos, int64_t n,
                      int64_t W, int64_t dst_rows, hipStream_t s) {
  if (n < 0 || W < 1 || W > (int64_t(1) << 20) || dst_rows < 0) return -1;
  if (n == 0 || dst_rows == 0) return 0;
  const uintptr_t a = reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst) | uintptr_t(W);
  if (a % 16 == 0) return launch_gather<uint4>(src, dst, keep, pos, n, W, dst_rows, s);
  if (a % 4 == 0) return launch_gather<uint32_t>(src, dst, keep, pos, n, W, dst_rows, s);
  return launch_gather<uint8_t>(src, dst, keep, pos, n, W, dst_rows, s);
}

int docqa_csr_gather(const int64_t* row_ptr, const uint8_t* keep, const int64_t* pos, const int64_t* epos,
                     int64_t n, const int* terms, const uint8_t* tfs, int64_t e_in, int64_t* new_ptr,
                     int64_t ptr_rows, int* new_terms, uint8_t* new_tfs, int64_t e_cap, hipStream_t s) {
  if (n < 0 || e_in < 0 || ptr_rows < 1 || e_cap < 0) return -1;
  const int64_t blocks = (n + 1 + kBlock / kRowLanes - 1) / (kBlock / kRowLanes);
  csr_gather_kernel<<<grid_for(blocks), kBlock, 0, s>>>(row_ptr, keep, pos, epos, n, terms, tfs, e_in, new_ptr,
                                                        ptr_rows, new_terms, new_tfs, e_cap);
  DOCQA_CHECK_LAUNCH();
  return 0;
}

int docqa_remap_ids(const int64_t* ids, int64_t m, const int64_t* pos, int64_t n, int64_t* out, hipStream_t s) {
  if (m < 0 || n < 0) return -1;
  if (m == 0) return 0;
  remap_ids_kernel<<<grid_for((m + kBlock - 1) / kBlock), kBlock, 0, s>>>(ids, m, pos, n, out);
  DOCQA_CHECK_LAUNCH();
  return 0;
}
