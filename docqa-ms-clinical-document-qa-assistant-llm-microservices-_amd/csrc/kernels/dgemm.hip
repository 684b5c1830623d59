// dgemm.hip -- skinny "decode GEMM" for the Llama generator's per-token projections:
//   Y[M, N] = X[M, K] . W[N, K]^T,   M = decode batch (<= 128), weights streamed once.
//
// At M <= 64 a projection is a weight-streaming problem (<= 64 FLOP per weight byte, far
// below the MFMA roof), so the design is about HBM bytes in flight (Little's law: ~8 TB/s x
// a few us of loaded latency = tens of KB per CU), not about tiles:
//   * workgroup = 64 weight rows x all M rows x one K slice.  W streams HBM -> LDS through
//     a 4-stage ring of 128-deep k-blocks filled by LDS-DMA (global_load_lds 16 B, source
//     XOR swizzle so the 16-row B-fragment reads are bank-conflict-free).  In-flight bytes
//     then cost LDS, not VGPRs: 2 workgroups x 3 stages x 16 KB per CU, while a register
//     double buffer (the first version of this kernel) capped M=64 at ~4.2 TB/s;
//   * X (tiny, L2-resident) goes straight to VGPRs, one k-block ahead; each wave owns a
//     disjoint (16 X rows x k-range) piece: 4 m-tiles at M=64, or 1-2 m-tiles with the
//     k-range split across waves (partials summed through LDS at the end);
//   * v_mfma_f32_16x16x32_bf16: A = X fragment, B = 4 weight n-tiles from the ring;
//   * split-K over the grid's y dimension gives >= 256 workgroups for the narrow
//     projections (O: N=4096); slices write fp32 partials reduced by a tiny second kernel,
//     S = 1 writes bf16 directly (gate|up, LM head).
//   * EPI_GLU: the Llama gate|up projection with SwiGLU fused into the epilogue.  The
//     weight rows are interleaved in blocks of 8 (gate 8b..8b+7, then up 8b..8b+7), so one
//     16-wide MFMA n-tile holds matching gate and up columns 8 lanes apart: a DPP row
//     rotate by 8 pairs them and silu(g) * u is written directly -- no [M, 2I] round trip
//     and no separate silu_mul launch.  7 n-tiles per workgroup (112 rows) make the Llama-3-8B
//     shape exactly 256 workgroups = one per CU, and halve the L2 traffic of re-reading X
//     per workgroup (at M = 64 that X traffic, not HBM, was the limiter).
//   * 65..128 rows: each wave owns two 16-row m-tiles over the whole k-block, so every
//     B fragment read from the LDS ring feeds two MFMAs and the weights still stream from
//     HBM exactly once (a second pass over 64-row halves would read them twice).
// Shapes: N % (16 NT) == 0, (K / S) % 512 == 0 (whole 4-stage ring turns), M <= 128
// (M <= 192 with 64-row weight tiles: three m-tiles per wave, no fused SwiGLU).
#include "docqa_common.h"
#include "docqa_asm.h"
#include "docqa_argmax.h"
#include "docqa_norm_row.h"
#include <stdlib.h>
#include <type_traits>

using namespace docqa;

namespace {
constexpr int BN = 64, BKD = 128, NS = 4, MR = 192;   // NS: default ring slots, K granule 4 stages
constexpr int KSTEPS = BKD / 32;               // 16x16x32 k-steps per stage
enum { EPI_BF16 = 0, EPI_PARTIAL = 1, EPI_GLU = 2, EPI_ARGMAX = 3 };
typedef __attribute__((address_space(3))) void lds_void;

// The ring's DMA / X loads are inline asm (docqa_asm.h): the counted waits below are the
// only vmcnt waits of the main loop.

template <int OFF>
__device__ __forceinline__ void gload16(bf16x8& d, const void* p) {
  asm volatile("global_load_dwordx4 %0, %1, off offset:%2" : "=v"(d) : "v"(p), "i"(OFF) : "memory");
}

// wait until at most N vector-memory ops are outstanding, naming the registers that
// become valid so nothing reading them is scheduled above the wait
// the same with the non-temporal hint: once-read weight streams (nt: aux = 2,
// MI355X_MICROARCH.md nt-weights) do not displace the L2 lines the next launch re-reads
template <int OFF>
__device__ __forceinline__ void gload16_nt(bf16x8& d, const void* p) {
  asm volatile("global_load_dwordx4 %0, %1, off offset:%2 nt" : "=v"(d) : "v"(p), "i"(OFF) : "memory");
}

template <int N, int SPW>
__device__ __forceinline__ void wait_vm_n(bf16x8 (&x)[SPW]) {
  if constexpr (SPW == 1)
    asm volatile("s_waitcnt vmcnt(%1)" : "+v"(x[0]) : "i"(N) : "memory");
  else if constexpr (SPW == 2)
    asm volatile("s_waitcnt vmcnt(%2)" : "+v"(x[0]), "+v"(x[1]) : "i"(N) : "memory");
  else if constexpr (SPW == 4)
    asm volatile("s_waitcnt vmcnt(%4)" : "+v"(x[0]), "+v"(x[1]), "+v"(x[2]), "+v"(x[3]) : "i"(N) : "memory");
  else if constexpr (SPW == 8)
    asm volatile("s_waitcnt vmcnt(%8)" : "+v"(x[0]), "+v"(x[1]), "+v"(x[2]), "+v"(x[3]), "+v"(x[4]), "+v"(x[5]),
                 "+v"(x[6]), "+v"(x[7]) : "i"(N) : "memory");
  else {
    static_assert(SPW == 12, "X fragment sets of 1, 2, 4, 8 or 12");
    asm volatile("s_waitcnt vmcnt(%12)" : "+v"(x[0]), "+v"(x[1]), "+v"(x[2]), "+v"(x[3]), "+v"(x[4]), "+v"(x[5]),
                 "+v"(x[6]), "+v"(x[7]), "+v"(x[8]), "+v"(x[9]), "+v"(x[10]), "+v"(x[11]) : "i"(N) : "memory");
  }
}

// keep x's registers allocated up to this point (for loads that are drained, never read)
template <int SPW>
__device__ __forceinline__ void keep_live(bf16x8 (&x)[SPW]) {
#pragma unroll
  for (int s = 0; s < SPW; ++s) asm volatile("" : "+v"(x[s]));
}

__device__ __forceinline__ int w_off(int row, int ch) {  // [rows][128] stage, 16 chunks per row
  return row * BKD + ((ch ^ (row & 15)) << 3);
}


// value of the lane 8 positions away inside each 16-lane row (DPP row_ror:8)
__device__ __forceinline__ float row_swap8(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x128, 0xf, 0xf, false));
}

// Wave roles: MT m-tiles of 16 X rows.  MT <= 4: the 4 waves split as (m-tile = wave % MT,
// k-group = wave / MT) so every wave owns a disjoint (rows x k) piece of the product and
// the W stage in LDS (NT 16-row n-tiles) is shared by all of them; KW = 4 / MT k-groups
// are summed through LDS at the end.  MT = 8: wave w owns m-tiles 2w, 2w+1 (MPW = 2) over
// the whole k-block (KW = 1).
// NormArgs (EPI_PARTIAL, few rows): the split-K slabs go out write-through and the LAST
// workgroup of the grid to finish (one ticket word, re-armed by it) runs the residual add +
// RMSNorm over them (docqa_norm_row.h, the add_rmsnorm_splitk arithmetic) -- the batch-1
// O / down projection then needs no add_rmsnorm_splitk launch (4.6 us each at M = 1,
// profiles/r4_batch1_kernel_stats.txt).
struct NormArgs {
  int* tick = nullptr;             // null: plain partial slabs
  uint16_t* residual = nullptr;    // [M, N] bf16, updated in place
  const uint16_t* gamma = nullptr; // [N]
  uint16_t* out = nullptr;         // [M, N] bf16 normed rows
  float eps = 0.f;
};

// XNormIn (batch 1, XN mode): the projection's input row is not read from X but built by
// the workgroup itself from the PREVIOUS projection's split-K slabs -- residual add + RMSNorm
// (the add_rmsnorm_splitk arithmetic, same thread -> chunk map, so the same bits) into LDS,
// while the first weight stages are already streaming.  One workgroup writes the updated
// residual to res_out (a second buffer: the others still read res_in), so the norm launch
// between two decode projections disappears.
struct XNormIn {
  const float* P = nullptr;          // [S, 1, K] fp32 slabs of the previous projection
  int S = 0;                         // 1..64 (up to 4 loaded in parallel)
  const uint16_t* res_in = nullptr;  // [1, K]
  uint16_t* res_out = nullptr;       // [1, K] = res_in + bf16(sum P)
  const uint16_t* gamma = nullptr;   // [K]
  float eps = 0.f;
};
constexpr int kXnMaxK = 4096;

// residual add + RMSNorm of the one input row into sx[0 .. Ks) (k slice [kbeg, kbeg + Ks))
__device__ __forceinline__ void xnorm_prologue(const XNormIn& xn, int K, int kbeg, int Ks, bool writer,
                                               uint16_t* sx, float* red) {
  constexpr int NV = kXnMaxK / 8 / 256;
  const int tid = threadIdx.x, nchunk = K >> 3;
  const uint4* rr = reinterpret_cast<const uint4*>(xn.res_in);
  const uint4* wr = reinterpret_cast<const uint4*>(xn.gamma);
  float v[NV][8];
  uint4 rres[NV], wres[NV];
  float4 pa[NV][4], pb[NV][4];
  // every load (residual, gamma, up to 4 slabs; clamped slabs loaded, not added) before the
  // first use: one memory latency, overlapped with the weight stages issued before
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = min(tid + 256 * i, nchunk - 1);
    rres[i] = rr[c];
    wres[i] = wr[c];
#pragma unroll
    for (int sl = 0; sl < 4; ++sl) {
      const float* q = xn.P + (size_t)min(sl, xn.S - 1) * K + c * 8;
      pa[i][sl] = *reinterpret_cast<const float4*>(q);
      pb[i][sl] = *reinterpret_cast<const float4*>(q + 4);
    }
  }
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = tid + 256 * i;
    if (c < nchunk) {
      float4 a = pa[i][0], b = pb[i][0];
#pragma unroll
      for (int sl = 1; sl < 4; ++sl)
        if (sl < xn.S) {
          a.x += pa[i][sl].x; a.y += pa[i][sl].y; a.z += pa[i][sl].z; a.w += pa[i][sl].w;
          b.x += pb[i][sl].x; b.y += pb[i][sl].y; b.z += pb[i][sl].z; b.w += pb[i][sl].w;
        }
      for (int sl = 4; sl < xn.S; ++sl) {   // more than 4 slabs (small models): in order, serial
        const float* q = xn.P + (size_t)sl * K + c * 8;
        const float4 a2 = *reinterpret_cast<const float4*>(q), b2 = *reinterpret_cast<const float4*>(q + 4);
        a.x += a2.x; a.y += a2.y; a.z += a2.z; a.w += a2.w;
        b.x += b2.x; b.y += b2.y; b.z += b2.z; b.w += b2.w;
      }
      const float x8[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
      float r[8];
      unpack8(rres[i], r);
#pragma unroll
      for (int j = 0; j < 8; ++j) v[i][j] = bf2f(f2bf(bf2f(f2bf(x8[j])) + r[j]));
      if (writer) reinterpret_cast<uint4*>(xn.res_out)[c] = pack8(v[i]);
#pragma unroll
      for (int j = 0; j < 8; ++j) ss += v[i][j] * v[i][j];
    }
  }
  ss = wave_sum(ss);
  if ((tid & 63) == 0) red[tid >> 6] = ss;
  __syncthreads();
  ss = red[0] + red[1] + red[2] + red[3];
  const float inv = rsqrtf(ss / (float)K + xn.eps);
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = tid + 256 * i;
    if (c < nchunk && c * 8 >= kbeg && c * 8 < kbeg + Ks) {
      float g[8], o[8];
      unpack8(wres[i], g);
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = v[i][j] * inv * g[j];
      *reinterpret_cast<uint4*>(sx + c * 8 - kbeg) = pack8(o);
    }
  }
  __syncthreads();
}

template <int EPI, int MT, int NT, int NSR, int XA = 2, bool NORM = false, bool XN = false>
__global__ __launch_bounds__(256) void dgemm_kernel(const uint16_t* __restrict__ X,
                                                    const uint16_t* __restrict__ W,
                                                    uint16_t* __restrict__ Y,
                                                    float* __restrict__ P, int M, int N, int K,
                                                    int Ks, int xcd_remap, float* __restrict__ pv = nullptr,
                                                    int* __restrict__ pi = nullptr, int n_valid = 0,
                                                    NormArgs na = NormArgs{}, XNormIn xn = XNormIn{}) {
  static_assert(!NORM || EPI == EPI_PARTIAL, "the fused norm consumes split-K slabs");
  static_assert(!XN || (MT == 1 && XA == 2), "the in-LDS input row is the one-row (batch-1) case");
  constexpr int MPW = MT > 4 ? MT / 4 : 1;       // m-tiles per wave
  constexpr int MTW = MT > 4 ? 4 : MT;           // wave groups along m
  constexpr int KW = 4 / MTW, SPW = KSTEPS / KW;
  constexpr int XR = MPW * SPW;                  // X fragments per wave per stage
  constexpr int XV = XN ? 0 : XR;                // ... of them vector-memory loads
  // vector-memory ops allowed in flight at the top of a step: XN counts exactly the NSR - 2
  // weight stages issued after this step's (deeper XN rings hide the input-row prologue);
  // the X-streaming variants keep the tuned 4-slot count
  constexpr int VW = XN ? (NSR - 2) * NT : 2 * NT + XV;
  constexpr int STAGE = NT * 16 * BKD;           // elements of one W stage (NT x 4 KB)
  static_assert(NSR >= 4, "ring needs >= 4 slots");
  static_assert(MT <= 4 || MT == 8 || MT == 12, "MT in {1, 2, 4, 8, 12}");
  __shared__ __attribute__((aligned(16))) uint16_t sw[NSR * STAGE];   // W ring
  __shared__ __attribute__((aligned(16))) uint16_t sx[XN ? kXnMaxK : 8];  // XN: the input row slice
  __shared__ float xred[4];
  // XCD-aware split-K placement: workgroups are dealt to the 8 XCDs round-robin by linear
  // id, so with the plain (tile, slice) grid every XCD sees every K slice and its 4 MB L2
  // must hold all of X next to the weight stream.  Remapped, XCD x only runs slice x % S:
  // its L2 holds 1/S of X and the re-reads of X by its workgroups hit there.
  int tile = blockIdx.x, slice = blockIdx.y;
  if (xcd_remap) {
    const int S = gridDim.y;
    const int L = blockIdx.x + blockIdx.y * gridDim.x;
    const int xcd = L & 7, j = L >> 3;
    slice = xcd % S;
    tile = j * (8 / S) + xcd / S;
  }
  const int n0 = tile * NT * 16;
  const int kbeg = slice * Ks;
  const int nkb = Ks / BKD;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fq = lane >> 4;
  const int mt = wave % MTW, kg = wave / MTW;
  const uint16_t* xrow[MPW];
#pragma unroll
  for (int mi = 0; mi < MPW; ++mi) {
    const int xr = min((mt * MPW + mi) * 16 + fr, M - 1);
    xrow[mi] = X + (size_t)xr * K + kbeg + kg * SPW * 32 + fq * 8;
  }
  const uint32_t ring = lds_u32(sw);

  f32x4 acc[MPW][NT];
#pragma unroll
  for (int mi = 0; mi < MPW; ++mi)
#pragma unroll
    for (int i = 0; i < NT; ++i) acc[mi][i] = f32x4{0.f, 0.f, 0.f, 0.f};

  // W stage j -> ring slot j % NS: 4 NT wave-instructions of 64 lanes x 16 B, NT per wave,
  // source XOR-swizzled (the DMA destination is lane-linear).  Past the last stage the
  // sources are clamped (L2 hits into free slots / dead X buffers) so that every step
  // issues the same loads unconditionally: a load whose destination is live on one path
  // and not on another lets hipcc hand its registers to other values while the data is
  // still in flight.
  const uint16_t* wsrc[NT];
#pragma unroll
  for (int i = 0; i < NT; ++i) {
    const int p = (i * 4 + wave) * 64 + lane;
    const int r = p >> 4;
    wsrc[i] = W + (size_t)(n0 + r) * K + kbeg + (((p & 15) ^ (r & 15)) << 3);
  }
  auto stage_w = [&](int j) {
    const int koff = min(j, nkb - 1) * BKD;
    const uint32_t dst = ring + (uint32_t)((j % NSR) * STAGE * 2);
#pragma unroll
    for (int i = 0; i < NT; ++i) glds16<true>(wsrc[i] + koff, dst + (uint32_t)((i * 4 + wave) * 1024));
  };
  auto load_x = [&](bf16x8 (&x)[XR], int j) {
    if constexpr (XN) {   // one row, from the prologue's LDS slice (a broadcast read)
      x[0] = *reinterpret_cast<const bf16x8*>(sx + min(j, nkb - 1) * BKD + kg * SPW * 32 + fq * 8);
      return;
    }
#pragma unroll
    for (int mi = 0; mi < MPW; ++mi) {
      const uint16_t* src = xrow[mi] + min(j, nkb - 1) * BKD;
      gload16<0>(x[mi * SPW], src);
      if constexpr (SPW > 1) gload16<64>(x[mi * SPW + 1], src);
      if constexpr (SPW > 2) { gload16<128>(x[mi * SPW + 2], src); gload16<192>(x[mi * SPW + 3], src); }
    }
  };
  auto mma = [&](const bf16x8 (&x)[XR], int j) {
    const uint16_t* src = sw + (j % NSR) * STAGE;
#pragma unroll
    for (int s = 0; s < SPW; ++s) {
      const int ch = (kg * SPW + s) * 4 + fq;
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const bf16x8 b = *reinterpret_cast<const bf16x8*>(src + w_off(nt * 16 + fr, ch));
#pragma unroll
        for (int mi = 0; mi < MPW; ++mi)
          acc[mi][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(x[mi * SPW + s], b, acc[mi][nt], 0, 0, 0);
      }
    }
  };
  // Issue order per wave (R = NSR): W0 .. W(R-4) X0 W(R-3) X1 W(R-2) | step i: X(i+2)
  // W(i+R-1).  At the top of step i the ops issued after X(i) are one W group, X(i+1) and
  // one more W group, so vmcnt(2 NT + XR) retires X(i) and (issued before it) W(i)
  // while R-2 W stages stay in flight; the barrier then publishes stage i to every wave
  // and frees slot (i-1) % R for W(i+R-1).
  bf16x8 x0[XR], x1[XR], x2[XR], x3[XR];
#define RING_STEP(I, XC, XN, NW)                                                        \
  wait_vm_n<NW>(XC);                                                                    \
  ring_barrier();                                                                       \
  load_x(XN, (I) + XA);                                                                 \
  stage_w((I) + NSR - 1);                                                               \
  mma(XC, I);
  if constexpr (XA == 2) {
    if constexpr (XN) {
      // weight stages first, then the input row (its loads overlap theirs; waiting for them
      // retires the stages too -- vmcnt is in order), then the first two X fragments
#pragma unroll
      for (int j = 0; j <= NSR - 2; ++j) stage_w(j);
      xnorm_prologue(xn, K, kbeg, Ks, blockIdx.x == 0 && blockIdx.y == 0, sx, xred);
      load_x(x0, 0);
      load_x(x1, 1);
    } else {
#pragma unroll
      for (int j = 0; j <= NSR - 4; ++j) stage_w(j);
      load_x(x0, 0);
      stage_w(NSR - 3);
      load_x(x1, 1);
      stage_w(NSR - 2);
    }
    // nkb % 4 == 0: a break-free 4-step body keeps each X buffer in one register set (an
    // early exit makes hipcc merge buffers with register copies that read in-flight data)
    for (int i = 0; i < nkb; i += 4) {
      RING_STEP(i, x0, x2, VW)
      RING_STEP(i + 1, x1, x3, VW)
      RING_STEP(i + 2, x2, x0, VW)
      RING_STEP(i + 3, x3, x1, VW)
    }
  } else {
    // X three k-blocks ahead (the 65-128-row case, where X -- not W -- is the longer
    // pole): issue W0 X0 W1 X1 W2 X2 | step i: X(i+3) W(i+3).  W(i) now follows X(i), and
    // the ops after W(i) are X(i+1) W(i+1) X(i+2) W(i+2): vmcnt(2 (NT + XR)) retires both.
    static_assert(NSR == 4, "X-ahead-3 schedule is written for a 4-slot ring");
    stage_w(0);
    load_x(x0, 0);
    stage_w(1);
    load_x(x1, 1);
    stage_w(2);
    load_x(x2, 2);
    for (int i = 0; i < nkb; i += 4) {
      RING_STEP(i, x0, x3, 2 * (NT + XR))
      RING_STEP(i + 1, x1, x0, 2 * (NT + XR))
      RING_STEP(i + 2, x2, x1, 2 * (NT + XR))
      RING_STEP(i + 3, x3, x2, 2 * (NT + XR))
    }
  }
#undef RING_STEP
  // drain the clamped tail loads; naming every X buffer keeps their registers reserved
  // until the data has landed
  wait_vm_n<0>(x0);
  keep_live(x1);
  keep_live(x2);
  keep_live(x3);

  // C/D map of 16x16x32: col = lane & 15 (weight row), row = 4 * (lane >> 4) + r (X row)
  auto store = [&](int row, int col, float v) {
    if constexpr (NORM)
      __hip_atomic_store(P + ((size_t)slice * M + row) * N + col, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else if constexpr (EPI == EPI_PARTIAL) P[((size_t)slice * M + row) * N + col] = v;
    else Y[(size_t)row * N + col] = f2bf(v);
  };
  // SwiGLU pair: gate value at an 8-block's low half, up value 8 columns later
  float glu_lo = 0.f;   // the smallest gate this lane has seen (silu_times_first)
  auto store_glu = [&](int row, int col, float g, float u, auto second) {
    const float gb = bf2f(f2bf(g)), ub = bf2f(f2bf(u));   // as the unfused bf16 GEMM output
    Y[(size_t)row * (N >> 1) + ((col >> 4) << 3) + (col & 7)] = f2bf(silu_times_pass(gb, ub, glu_lo, second));
  };
  if constexpr (EPI == EPI_ARGMAX) {
    // LM head + greedy pick: the [rows, 64] logit tile through LDS (past the k-group
    // reduction area), 4 lanes per row -> one (value, id) partial per (row, tile)
    constexpr int TP = NT * 16 + 1;
    __syncthreads();                                  // every wave done reading the ring
    float* tl = reinterpret_cast<float*>(sw) + (KW == 1 ? 0 : 4 * NT * 64 * 4);
    if constexpr (KW == 1) {
#pragma unroll
      for (int mi = 0; mi < MPW; ++mi)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
          for (int r = 0; r < 4; ++r) tl[((mt * MPW + mi) * 16 + fq * 4 + r) * TP + nt * 16 + fr] = acc[mi][nt][r];
    } else {
      f32x4* red = reinterpret_cast<f32x4*>(sw);      // [wave][nt][lane] = one slot
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) red[(wave * NT + nt) * 64 + lane] = acc[0][nt];
      __syncthreads();
      const float* rf = reinterpret_cast<const float*>(sw);
      for (int idx = tid; idx < MT * NT * 256; idx += 256) {
        const int r = idx & 3, ln = (idx >> 2) & 63, q = idx >> 8;
        const int nt = q % NT, m = q / NT;
        float v = 0.f;
#pragma unroll
        for (int g = 0; g < KW; ++g) v += rf[(((g * MT + m) * NT + nt) * 64 + ln) * 4 + r];
        tl[(m * 16 + (ln >> 4) * 4 + r) * TP + nt * 16 + (ln & 15)] = v;
      }
    }
    __syncthreads();
    const int ntiles = N / (NT * 16);
    for (int rr = tid >> 2; rr < MT * 16; rr += 64) {
      float bv = -FLT_MAX;
      int bi = 0x7fffffff;
      const int c0 = (tid & 3) * (NT * 4);
#pragma unroll 4
      for (int c = c0; c < c0 + NT * 4; ++c) {
        const int col = n0 + c;
        if (col < n_valid) argmax_better(bv, bi, bf2f(f2bf(tl[rr * TP + c])), col);
      }
#pragma unroll
      for (int o = 1; o <= 2; o <<= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        argmax_better(bv, bi, ov, oi);
      }
      if ((tid & 3) == 0 && rr < M) {
        pv[(size_t)rr * ntiles + tile] = bv;
        pi[(size_t)rr * ntiles + tile] = bi;
      }
    }
    return;
  }
  if constexpr (KW == 1) {
    auto sweep = [&](auto second) {
#pragma unroll
      for (int mi = 0; mi < MPW; ++mi)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int row = (mt * MPW + mi) * 16 + fq * 4 + r, col = n0 + nt * 16 + fr;
            if constexpr (EPI == EPI_GLU) {
              const float u = row_swap8(acc[mi][nt][r]);
              if (row < M && (fr & 8) == 0) store_glu(row, col, acc[mi][nt][r], u, second);
            } else if (row < M) {
              store(row, col, acc[mi][nt][r]);
            }
          }
    };
    sweep(std::false_type{});
    if constexpr (EPI == EPI_GLU) {
      if (silu_second_pass(glu_lo)) sweep(std::true_type{});   // a gate below -80: silu_times for the wave's pairs
    }
  } else {
    // sum the KW k-groups through LDS (ring is free after the last barrier + wait)
    __syncthreads();
    f32x4* red = reinterpret_cast<f32x4*>(sw);        // [wave][nt][lane] = one slot
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) red[(wave * NT + nt) * 64 + lane] = acc[0][nt];
    __syncthreads();
    const float* rf = reinterpret_cast<const float*>(sw);
    auto sum_k = [&](int m, int nt, int ln, int r) {
      float v = 0.f;
#pragma unroll
      for (int g = 0; g < KW; ++g) v += rf[(((g * MT + m) * NT + nt) * 64 + ln) * 4 + r];
      return v;
    };
    auto sweep = [&](auto second) {
#pragma unroll
      for (int e = 0; e < MT * NT; ++e) {
        const int idx = e * 256 + tid;                 // (m-tile, nt, lane, r)
        const int r = idx & 3, ln = (idx >> 2) & 63, q = idx >> 8;
        const int nt = q % NT, m = q / NT;
        const int row = m * 16 + (ln >> 4) * 4 + r, col = n0 + nt * 16 + (ln & 15);
        if (row >= M) continue;
        if constexpr (EPI == EPI_GLU) {
          if ((ln & 8) == 0) store_glu(row, col, sum_k(m, nt, ln, r), sum_k(m, nt, ln + 8, r), second);
        } else {
          store(row, col, sum_k(m, nt, ln, r));
        }
      }
    };
    sweep(std::false_type{});
    if constexpr (EPI == EPI_GLU) {
      if (silu_second_pass(glu_lo)) sweep(std::true_type{});   // a gate below -80: silu_times for the wave's pairs
    }
  }
  if constexpr (NORM) {
    __shared__ int s_last;
    __shared__ float red[4];
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this workgroup's slab pieces landed
    __syncthreads();
    if (tid == 0) {
      const int old = __hip_atomic_fetch_add(na.tick, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      s_last = old == (int)(gridDim.x * gridDim.y) - 1;
      if (s_last) __hip_atomic_store(na.tick, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    if (!s_last) return;
    const int S = gridDim.y;
    for (int row = 0; row < M; ++row) {
      if (S == 4)
        add_rmsnorm_splitk_row<4, 4, false, true>(P, S, (size_t)M * N, na.residual, na.gamma, na.out, N, na.eps,
                                                  row, tid, red);
      else
        add_rmsnorm_splitk_row<4, 0, false, true>(P, S, (size_t)M * N, na.residual, na.gamma, na.out, N, na.eps,
                                                  row, tid, red);
      __syncthreads();   // red reused by the next row
    }
  }
}

__global__ __launch_bounds__(256) void splitk_reduce_kernel(const float* __restrict__ P,
                                                            uint16_t* __restrict__ Y, int MN, int S) {
  const int i = (blockIdx.x * 256 + threadIdx.x) * 4;
  if (i >= MN) return;
  float4 acc = *reinterpret_cast<const float4*>(P + i);
  for (int s = 1; s < S; ++s) {
    const float4 v = *reinterpret_cast<const float4*>(P + (size_t)s * MN + i);
    acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
  }
  uint2 o;
  o.x = pack2(acc.x, acc.y);
  o.y = pack2(acc.z, acc.w);
  *reinterpret_cast<uint2*>(Y + i) = o;
}
}  // namespace

// split count: enough workgroups for the chip (>= 256), K slices of whole ring turns
int docqa_dgemm_splits(int N, int K) {
  const int tiles = N / BN;
  int s = 1;
  while (tiles * s < 256 && K % (s * 2) == 0 && (K / (s * 2)) % (NS * BKD) == 0)
    s *= 2;
  return s;
}

static int xa_knob() {   // X prefetch distance for 65-128 rows (tuning experiments)
  static const int v = [] {
    const char* e = getenv("DOCQA_DGEMM_XA");
    return e ? atoi(e) : 0;
  }();
  return v;
}

static int xcd_knob() {   // XCD-aware slice placement (A/B experiments): 1 on, 0 off
  static const int v = [] {
    const char* e = getenv("DOCQA_DGEMM_XCD");
    return e ? atoi(e) : 1;
  }();
  return v;
}

template <int EPI, int NT, int NSR = NS>
static void launch_mt(int mt, dim3 grid, hipStream_t s, const uint16_t* x, const uint16_t* w,
                      uint16_t* y, float* p, int M, int N, int K, int Ks, float* pv = nullptr,
                      int* pi = nullptr, int nv = 0) {
  const int S = grid.y;
  const int xr = (xcd_knob() && S > 1 && 8 % S == 0 && (grid.x * S) % 8 == 0) ? 1 : 0;
  if (mt == 1) dgemm_kernel<EPI, 1, NT, NSR><<<grid, 256, 0, s>>>(x, w, y, p, M, N, K, Ks, xr, pv, pi, nv);
  else if (mt == 2) dgemm_kernel<EPI, 2, NT, NSR><<<grid, 256, 0, s>>>(x, w, y, p, M, N, K, Ks, xr, pv, pi, nv);
  else if (mt <= 4) dgemm_kernel<EPI, 4, NT, NSR><<<grid, 256, 0, s>>>(x, w, y, p, M, N, K, Ks, xr, pv, pi, nv);
  else if (mt <= 8) {
    if constexpr (NSR == 4) {
      if (xa_knob() == 3)
        dgemm_kernel<EPI, 8, NT, NSR, 3><<<grid, 256, 0, s>>>(x, w, y, p, M, N, K, Ks, xr, pv, pi, nv);
      else dgemm_kernel<EPI, 8, NT, NSR><<<grid, 256, 0, s>>>(x, w, y, p, M, N, K, Ks, xr, pv, pi, nv);
    } else {
      dgemm_kernel<EPI, 8, NT, NSR><<<grid, 256, 0, s>>>(x, w, y, p, M, N, K, Ks, xr, pv, pi, nv);
    }
  } else if constexpr (NT <= 8 && EPI != EPI_GLU) {
    // 129-192 rows: three m-tiles per wave
    dgemm_kernel<EPI, 12, NT, NSR><<<grid, 256, 0, s>>>(x, w, y, p, M, N, K, Ks, xr, pv, pi, nv);
  }
}

static bool shape_ok(int M, int N, int K, int S, int bn) {
  return M <= MR && N % bn == 0 && S >= 1 && K % S == 0 && (K / S) % (NS * BKD) == 0;
}

int docqa_dgemm(const void* X, const void* W, void* Y, float* partial, int M, int N, int K,
                int S, hipStream_t s) {
  if (M == 0) return 0;
  if (!shape_ok(M, N, K, S, BN) || (S > 1 && !partial)) return -1;
  dim3 grid(N / BN, S);
  const int mt = (M + 15) / 16;
  const uint16_t* x = (const uint16_t*)X;
  const uint16_t* w = (const uint16_t*)W;
  if (S == 1) {
    launch_mt<EPI_BF16, 4>(mt, grid, s, x, w, (uint16_t*)Y, nullptr, M, N, K, K);
  } else {
    launch_mt<EPI_PARTIAL, 4>(mt, grid, s, x, w, nullptr, partial, M, N, K, K / S);
    const int MN = M * N;  // multiple of 4 (N % 64 == 0)
    splitk_reduce_kernel<<<(MN / 4 + 255) / 256, 256, 0, s>>>(partial, (uint16_t*)Y, MN, S);
  }
  DOCQA_CHECK_LAUNCH();
  return 0;
}

// split-K partial slabs only (S >= 1, P: [S, M, N] fp32): the combine is fused into the
// consumer (add_rmsnorm_splitk / rope_cache_splitk)
int docqa_dgemm_partial(const void* X, const void* W, float* P, int M, int N, int K, int S,
                        int tile_rows, hipStream_t s) {
  if (M == 0) return 0;
  if (!P || (tile_rows != 64 && tile_rows != 128) || !shape_ok(M, N, K, S, tile_rows)) return -1;
  const int mt = (M + 15) / 16;
  const uint16_t* x = (const uint16_t*)X;
  const uint16_t* w = (const uint16_t*)W;
  static const int ns_env = [] {   // ring depth knob (tuning experiments)
    const char* e = getenv("DOCQA_DGEMM_NS");
    return e ? atoi(e) : 0;
  }();
  if (tile_rows == 128)   // 1 workgroup per CU (128 KB ring), X re-read half as often
    launch_mt<EPI_PARTIAL, 8>(mt, dim3(N / 128, S), s, x, w, nullptr, P, M, N, K, K / S);
  else if (ns_env == 6)
    launch_mt<EPI_PARTIAL, 4, 6>(mt, dim3(N / 64, S), s, x, w, nullptr, P, M, N, K, K / S);
  else if (ns_env == 8)
    launch_mt<EPI_PARTIAL, 4, 8>(mt, dim3(N / 64, S), s, x, w, nullptr, P, M, N, K, K / S);
  else
    launch_mt<EPI_PARTIAL, 4>(mt, dim3(N / 64, S), s, x, w, nullptr, P, M, N, K, K / S);
  DOCQA_CHECK_LAUNCH();
  return 0;
}

// Few-row split-K projection with the residual add + RMSNorm fused in (NormArgs): P [S, M, N]
// fp32 slabs (scratch), residual [M, N] updated, out [M, N] = rmsnorm(residual) * gamma.
// M <= kNormRows, N <= 8192 (4 chunks of 8 per lane), 64-row weight tiles.
constexpr int kNormRows = 4;
int docqa_dgemm_add_rmsnorm(const void* X, const void* W, float* P, int M, int N, int K, int S, void* residual,
                            const void* gamma, void* out, float eps, int* tick, hipStream_t s) {
  if (M == 0) return 0;
  if (M > kNormRows || N > 8192 || N % 8 || !tick || !P || !shape_ok(M, N, K, S, BN)) return -1;
  NormArgs na{tick, (uint16_t*)residual, (const uint16_t*)gamma, (uint16_t*)out, eps};
  const dim3 grid(N / BN, S);
  const int xr = (xcd_knob() && S > 1 && 8 % S == 0 && (grid.x * S) % 8 == 0) ? 1 : 0;
  dgemm_kernel<EPI_PARTIAL, 1, 4, NS, 2, true><<<grid, 256, 0, s>>>((const uint16_t*)X, (const uint16_t*)W, nullptr,
                                                                    P, M, N, K, K / S, xr, nullptr, nullptr, 0, na);
  DOCQA_CHECK_LAUNCH();
  return 0;
}

// Batch-1 projections whose input row is rmsnorm(res_in + bf16(sum of the previous
// projection's slabs)) * gamma, built in LDS by each workgroup (XNormIn): split-K slabs out
// (the next layer's QKV) or the fused SwiGLU (gate|up).  res_out <- res_in + bf16(sum Pin).
static bool xn_ok(int N, int K, int S, int bn, const XNormIn& xn) {
  return K <= kXnMaxK && xn.S >= 1 && xn.S <= 64 && xn.P && xn.res_in && xn.res_out &&
         xn.gamma && xn.res_in != xn.res_out && shape_ok(1, N, K, S, bn);
}

int docqa_dgemm_partial_xn(const float* Pin, int Sin, const void* res_in, void* res_out, const void* gamma,
                           float eps, const void* W, float* P, int N, int K, int S, hipStream_t s) {
  const XNormIn xn{Pin, Sin, (const uint16_t*)res_in, (uint16_t*)res_out, (const uint16_t*)gamma, eps};
  if (!P || !xn_ok(N, K, S, BN, xn)) return -1;
  const dim3 grid(N / BN, S);
  const int xr = (xcd_knob() && S > 1 && 8 % S == 0 && (grid.x * S) % 8 == 0) ? 1 : 0;
  // (an 8-slot ring to stream on under the input-row prologue measured slower: QKV 17.7 vs
  // 16.4 us, profiles/r4_b1_ab.log)
  dgemm_kernel<EPI_PARTIAL, 1, 4, NS, 2, false, true><<<grid, 256, 0, s>>>(
      nullptr, (const uint16_t*)W, nullptr, P, 1, N, K, K / S, xr, nullptr, nullptr, 0, NormArgs{}, xn);
  DOCQA_CHECK_LAUNCH();
  return 0;
}

int docqa_dgemm_glu_xn(const float* Pin, int Sin, const void* res_in, void* res_out, const void* gamma, float eps,
                       const void* W, void* Y, int N, int K, hipStream_t s) {
  const XNormIn xn{Pin, Sin, (const uint16_t*)res_in, (uint16_t*)res_out, (const uint16_t*)gamma, eps};
  if (xn_ok(N, K, 1, 112, xn) && N / 112 >= 192)
    dgemm_kernel<EPI_GLU, 1, 7, NS, 2, false, true><<<dim3(N / 112), 256, 0, s>>>(
        nullptr, (const uint16_t*)W, (uint16_t*)Y, nullptr, 1, N, K, K, 0, nullptr, nullptr, 0, NormArgs{}, xn);
  else if (xn_ok(N, K, 1, 64, xn))
    dgemm_kernel<EPI_GLU, 1, 4, NS, 2, false, true><<<dim3(N / 64), 256, 0, s>>>(
        nullptr, (const uint16_t*)W, (uint16_t*)Y, nullptr, 1, N, K, K, 0, nullptr, nullptr, 0, NormArgs{}, xn);
  else
    return -1;
  DOCQA_CHECK_LAUNCH();
  return 0;
}

// Y[M, N/2] = silu(gate) * up for the 8-interleaved gate|up weight W [N, K] (N = 2 I)
int docqa_dgemm_glu(const void* X, const void* W, void* Y, int M, int N, int K, hipStream_t s) {
  if (M == 0) return 0;
  if (M > 128) return -1;
  const int mt = (M + 15) / 16;
  const uint16_t* x = (const uint16_t*)X;
  const uint16_t* w = (const uint16_t*)W;
  static const int glu_nt = [] {   // tile-width knob (tuning experiments): 4 -> 64-row tiles
    const char* e = getenv("DOCQA_GLU_NT");
    return e ? atoi(e) : 0;
  }();
  if (glu_nt != 4 && shape_ok(M, N, K, 1, 112) && N / 112 >= 192) {
    launch_mt<EPI_GLU, 7>(mt, dim3(N / 112), s, x, w, (uint16_t*)Y, nullptr, M, N, K, K);
  } else if (shape_ok(M, N, K, 1, 64)) {
    launch_mt<EPI_GLU, 4>(mt, dim3(N / 64), s, x, w, (uint16_t*)Y, nullptr, M, N, K, K);
  } else {
    return -1;
  }
  DOCQA_CHECK_LAUNCH();
  return 0;
}

// LM head + greedy pick at <= 192 rows (batch-1 decode included): out[M] = argmax over the
// first n_valid columns of bf16(X . W^T), outv[M] (optional) the picked value; ws_v / ws_i:
// [M, N / 64] per-tile partials.  The [M, vocab] logits never reach HBM.
int docqa_dgemm_argmax(const void* X, const void* W, int64_t* out, float* outv, float* ws_v, int* ws_i, int M,
                       int N, int K, int n_valid, hipStream_t s) {
  if (M == 0) return 0;
  if (!shape_ok(M, N, K, 1, BN) || n_valid <= 0 || n_valid > N) return -1;
  const int mt = (M + 15) / 16;
  launch_mt<EPI_ARGMAX, 4>(mt, dim3(N / BN), s, (const uint16_t*)X, (const uint16_t*)W, nullptr, nullptr, M, N, K,
                           K, ws_v, ws_i, n_valid);
  argmax_merge_kernel<<<M, 256, 0, s>>>(ws_v, ws_i, N / BN, out, outv);
  DOCQA_CHECK_LAUNCH();
  return 0;
}

// ---------------------------------------------------------------------------------------
// Batch-1 GEMV (one decode row): y[N] = x[K] . W[N, K]^T with NO MFMA and NO LDS ring.  At
// M = 1 the projection is a pure weight stream, and the ring kernel above tops out at
// ~4.3 TB/s there (profiles/r4_b1_decode_gemm_split_probe.log) with two 16-KB stages in
// flight per workgroup.  Here every lane issues ALL of its weight loads at once, straight
// into VGPRs (R weight rows x C 16-B chunks: 32 loads = 128 KB per 256-thread workgroup in
// flight for the 4096-wide projections), then retires them row by row in issue order
// (vmcnt counts loads back in order) into v_dot2_f32_bf16 dot products against the input
// row; the 4 waves split K and meet in LDS.  Workgroup = R output rows x one K slice.
//   * EPI_PARTIAL: fp32 slab P[slice][n] for the split-K consumers (same layout as dgemm);
//   * EPI_GLU: R = 16 rows = one 8-interleaved gate|up group -> 8 SwiGLU outputs, bf16;
//   * XN: the input row is built in LDS from the previous projection's slabs (XNormIn),
//     its loads queued behind the weight loads (the stream is already in flight).
// Shapes: N % R == 0, Ks = K / S with Ks % 2048 == 0 (C = Ks / 2048 chunks per lane), and
// R x C <= 32 loads per lane (the 6-bit vmcnt counter holds at most 63 outstanding).
template <int I, int N, typename F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    static_for<I + 1, N>(f);
  }
}

template <int R, int C, int EPI, bool XN, bool NTW>
__global__ __launch_bounds__(256) void gemv_kernel(const uint16_t* __restrict__ X, const uint16_t* __restrict__ W,
                                                   uint16_t* __restrict__ Y, float* __restrict__ P, int N, int K,
                                                   int Ks, XNormIn xn, int* __restrict__ pi = nullptr,
                                                   int n_valid = 0) {
  static_assert(EPI == EPI_PARTIAL || (EPI == EPI_GLU && R == 16) || (EPI == EPI_ARGMAX && R == 16),
                "GLU: one 16-row gate|up group; ARGMAX: 16 logits per workgroup");
  static_assert(R * C <= 32, "loads in flight per lane must fit the vmcnt counter");
  __shared__ __attribute__((aligned(16))) uint16_t sx[XN ? kXnMaxK : 8];
  __shared__ float red[4][R];
  __shared__ float xred[4];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n0 = blockIdx.x * R, slice = blockIdx.y, kbeg = slice * Ks;
  const int kq = Ks >> 2;                         // k per wave
  const int kw = kbeg + wave * kq;                // this wave's k range
  // weight chunk (r, c) of this lane: row n0 + r, k = kw + c * 512 + lane * 8
  bf16x8 w[R][C];
  const uint16_t* wb = W + (size_t)n0 * K + kw + lane * 8;
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int c = 0; c < C; ++c) {
      if constexpr (NTW) gload16_nt<0>(w[r][c], wb + (size_t)r * K + c * 512);
      else gload16<0>(w[r][c], wb + (size_t)r * K + c * 512);
    }
  bf16x8 x[C];
  if constexpr (XN) {
    xnorm_prologue(xn, K, kbeg, Ks, blockIdx.x == 0 && blockIdx.y == 0, sx, xred);
#pragma unroll
    for (int c = 0; c < C; ++c) x[c] = *reinterpret_cast<const bf16x8*>(sx + (kw - kbeg) + c * 512 + lane * 8);
  } else {
#pragma unroll
    for (int c = 0; c < C; ++c) x[c] = *reinterpret_cast<const bf16x8*>(X + kw + c * 512 + lane * 8);
  }
  float acc[R];
  static_for<0, R>([&](auto rc) {
    constexpr int r = decltype(rc)::value;
    // row r's chunks landed: everything issued after them is the later rows' C chunks each
    constexpr int LEFT = (R - 1 - r) * C;
    if constexpr (C == 1) wait_vm_n<LEFT, 1>(*reinterpret_cast<bf16x8(*)[1]>(&w[r][0]));
    else if constexpr (C == 2) wait_vm_n<LEFT, 2>(*reinterpret_cast<bf16x8(*)[2]>(&w[r][0]));
    else if constexpr (C == 4) wait_vm_n<LEFT, 4>(*reinterpret_cast<bf16x8(*)[4]>(&w[r][0]));
    else {
      static_assert(C == 7, "C in {1, 2, 4, 7}");
      asm volatile("s_waitcnt vmcnt(%7)" : "+v"(w[r][0]), "+v"(w[r][1]), "+v"(w[r][2]), "+v"(w[r][3]), "+v"(w[r][4]),
                   "+v"(w[r][5]), "+v"(w[r][6]) : "i"(LEFT) : "memory");
    }
    float a = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const bf16x8 wv = w[r][c], xv = x[c];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bf16x2 wa = {wv[2 * j], wv[2 * j + 1]}, xa = {xv[2 * j], xv[2 * j + 1]};
        a = __builtin_amdgcn_fdot2_f32_bf16(wa, xa, a, false);
      }
    }
    acc[r] = wave_sum(a);
  });
  if (lane == 0) {
#pragma unroll
    for (int r = 0; r < R; ++r) red[wave][r] = acc[r];
  }
  __syncthreads();
  if constexpr (EPI == EPI_PARTIAL) {
    if (tid < R) P[(size_t)slice * N + n0 + tid] = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
  } else if constexpr (EPI == EPI_ARGMAX) {
    // LM head + greedy pick: the 16 logits (bf16-rounded, as the unfused logits) -> one
    // (value, id) partial per workgroup at P / pi [blockIdx.x] for argmax_merge_kernel
    if (tid < 64) {
      float bv = -FLT_MAX;
      int bi = 0x7fffffff;
      if (tid < R && n0 + tid < n_valid) {
        bv = bf2f(f2bf(red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid]));
        bi = n0 + tid;
      }
#pragma unroll
      for (int o = 1; o < R; o <<= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        argmax_better(bv, bi, ov, oi);
      }
      if (tid == 0) {
        P[blockIdx.x] = bv;
        pi[blockIdx.x] = bi;
      }
    }
  } else {
    // gate rows n0 .. n0 + 7, up rows n0 + 8 .. n0 + 15 -> outputs n0 / 2 .. n0 / 2 + 7
    if (tid < 8) {
      const float g = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
      const float u = red[0][tid + 8] + red[1][tid + 8] + red[2][tid + 8] + red[3][tid + 8];
      const float gv = bf2f(f2bf(g)), uv = bf2f(f2bf(u));   // as the bf16 GEMM output
      Y[(n0 >> 1) + tid] = f2bf(silu(gv) * uv);
      // a gate below -80 (never in a real model): the store repeated with silu_times, behind a
      // branch of its own so that its second exp stays off every other workgroup's tail
      if (silu_second_pass(gv)) Y[(n0 >> 1) + tid] = f2bf(silu_times(gv, uv));
    }
  }
}

// weight-load policy: nt by default (batch-1 p50 454 -> 439 ms, profiles/r6_b1_nt_down_ab.log);
// DOCQA_GEMV_NT=0 for the default policy
static bool gemv_nt() {
  static const bool v = [] {
    const char* e = getenv("DOCQA_GEMV_NT");
    return e ? atoi(e) != 0 : true;
  }();
  return v;
}

template <int EPI, bool XN>
static int launch_gemv(int R, int C, dim3 grid, hipStream_t s, const uint16_t* x, const uint16_t* w, uint16_t* y,
                       float* p, int N, int K, int Ks, const XNormIn& xn) {
  const bool nt = gemv_nt();
#define GEMV_CASE(RR, CC)                                                                                    \
  if (R == RR && C == CC) {                                                                                  \
    if (nt) gemv_kernel<RR, CC, EPI, XN, true><<<grid, 256, 0, s>>>(x, w, y, p, N, K, Ks, xn);               \
    else gemv_kernel<RR, CC, EPI, XN, false><<<grid, 256, 0, s>>>(x, w, y, p, N, K, Ks, xn);                 \
    return 0;                                                                                                \
  }
  if constexpr (EPI == EPI_GLU) {
    GEMV_CASE(16, 1) GEMV_CASE(16, 2)
  } else if constexpr (EPI == EPI_ARGMAX) {
    return -1;   // docqa_gemv_argmax launches its own instantiations
  } else {
    GEMV_CASE(16, 1) GEMV_CASE(16, 2) GEMV_CASE(8, 2) GEMV_CASE(8, 4) GEMV_CASE(4, 4) GEMV_CASE(4, 7)
    GEMV_CASE(8, 1) GEMV_CASE(4, 2) GEMV_CASE(4, 1)
  }
#undef GEMV_CASE
  return -1;
}

// Batch-1 GEMV (see gemv_kernel).  epi 0: fp32 slabs P [S, 1, N]; epi 1: SwiGLU Y [1, N / 2]
// (R = 16, S = 1).  xn (nullable): the input row from the previous projection's slabs.
int docqa_gemv(const void* X, const void* W, void* Y, float* P, int N, int K, int S, int R, int epi,
               const float* Pin, int Sin, const void* res_in, void* res_out, const void* gamma, float eps,
               hipStream_t s) {
  if (S < 1 || K % S || (K / S) % 2048 || N % R || R < 1) return -1;
  const int Ks = K / S, C = Ks / 2048;
  const bool xnm = Pin != nullptr;
  const XNormIn xn{Pin, Sin, (const uint16_t*)res_in, (uint16_t*)res_out, (const uint16_t*)gamma, eps};
  if (xnm && !xn_ok(N, K, 1, R, xn)) return -1;
  if (!xnm && !X) return -1;
  if (epi == 1 ? (R != 16 || S != 1 || !Y) : !P) return -1;
  const dim3 grid(N / R, S);
  const uint16_t* x = (const uint16_t*)X;
  const uint16_t* w = (const uint16_t*)W;
  int rc;
  if (epi == 1)
    rc = xnm ? launch_gemv<EPI_GLU, true>(R, C, grid, s, x, w, (uint16_t*)Y, nullptr, N, K, Ks, xn)
             : launch_gemv<EPI_GLU, false>(R, C, grid, s, x, w, (uint16_t*)Y, nullptr, N, K, Ks, xn);
  else
    rc = xnm ? launch_gemv<EPI_PARTIAL, true>(R, C, grid, s, x, w, nullptr, P, N, K, Ks, xn)
             : launch_gemv<EPI_PARTIAL, false>(R, C, grid, s, x, w, nullptr, P, N, K, Ks, xn);
  if (rc) return rc;
  DOCQA_CHECK_LAUNCH();
  return 0;
}

// Batch-1 LM head + greedy pick on the GEMV: 16 vocabulary rows per workgroup (C = K / 2048
// chunks per lane, nt weight loads), one (value, id) partial each, merged by
// argmax_merge_kernel.  ws_v / ws_i: N / 16 entries.
int docqa_gemv_argmax(const void* X, const void* W, int64_t* out, float* outv, float* ws_v, int* ws_i, int N, int K,
                      int n_valid, hipStream_t s) {
  if (N % 16 || K % 2048 || K / 2048 > 2 || n_valid <= 0 || n_valid > N) return -1;
  const dim3 grid(N / 16);
  const XNormIn xn{};
  const uint16_t* x = (const uint16_t*)X;
  const uint16_t* w = (const uint16_t*)W;
  if (K == 2048)
    gemv_kernel<16, 1, EPI_ARGMAX, false, true><<<grid, 256, 0, s>>>(x, w, nullptr, ws_v, N, K, K, xn, ws_i, n_valid);
  else
    gemv_kernel<16, 2, EPI_ARGMAX, false, true><<<grid, 256, 0, s>>>(x, w, nullptr, ws_v, N, K, K, xn, ws_i, n_valid);
  argmax_merge_kernel<<<1, 256, 0, s>>>(ws_v, ws_i, N / 16, out, outv);
  DOCQA_CHECK_LAUNCH();
  return 0;
}

// ---------------------------------------------------------------------------------------
// FP8 weight stream for the batch-1 GEMV: the same register-streaming design over weights
// stored as OCP e4m3fn codes Wq [N, K] (one byte each) with one power-of-two fp32 scale per
// output row, W'[n, k] = Wq[n, k] * scale[n] (exactly the model's resident bf16 weights), so
// a projection moves half the bytes.  Each lane issues all its loads at once -- its row
// scale, the input row (bf16, unless XN builds it in LDS), then R rows x C chunks of LB = 8 or
// 16 codes, non-temporal -- and retires them in issue order with counted vmcnt waits;
// v_cvt_pk_f32_fp8 widens two codes per instruction, fp32 FMAs against the widened input
// row accumulate, the 4 waves split K and meet in LDS.  The row scale multiplies the fp32 sum
// once, before any bf16 rounding of an epilogue (exact: a power of two).
//   * EPI_PARTIAL: fp32 slab P[slice][n], scaled;
//   * EPI_GLU: R / 16 8-interleaved gate|up groups -> R / 2 SwiGLU outputs, bf16;
//   * EPI_ARGMAX: R logits -> one (value, id) partial per workgroup for argmax_merge_kernel.
// Shapes: N % R == 0, Ks = K / S with Ks % (256 LB) == 0 (C = Ks / (256 LB) chunks per lane),
// and 1 + C LB / 8 + R C <= 63 loads per lane (the 6-bit vmcnt counter).
namespace {
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
template <int LB> struct Fp8Chunk { typedef u32x2 T; };
template <> struct Fp8Chunk<16> { typedef u32x4 T; };

template <int LB>
__device__ __forceinline__ void gload_fp8_nt(typename Fp8Chunk<LB>::T& d, const void* p) {
  if constexpr (LB == 8) asm volatile("global_load_dwordx2 %0, %1, off nt" : "=v"(d) : "v"(p) : "memory");
  else asm volatile("global_load_dwordx4 %0, %1, off nt" : "=v"(d) : "v"(p) : "memory");
}

__device__ __forceinline__ void gload4(float& d, const void* p) {
  asm volatile("global_load_dword %0, %1, off" : "=v"(d) : "v"(p) : "memory");
}

// at most LEFT vector-memory ops outstanding; names the registers that become valid
template <int LEFT, typename T>
__device__ __forceinline__ void wait_vm_reg(T& v) {
  asm volatile("s_waitcnt vmcnt(%1)" : "+v"(v) : "i"(LEFT) : "memory");
}

template <int LEFT, int C, typename T>
__device__ __forceinline__ void wait_vm_row(T (&w)[C]) {
  if constexpr (C == 1)
    asm volatile("s_waitcnt vmcnt(%1)" : "+v"(w[0]) : "i"(LEFT) : "memory");
  else if constexpr (C == 2)
    asm volatile("s_waitcnt vmcnt(%2)" : "+v"(w[0]), "+v"(w[1]) : "i"(LEFT) : "memory");
  else if constexpr (C == 4)
    asm volatile("s_waitcnt vmcnt(%4)" : "+v"(w[0]), "+v"(w[1]), "+v"(w[2]), "+v"(w[3]) : "i"(LEFT) : "memory");
  else {
    static_assert(C == 7, "C in {1, 2, 4, 7}");
    asm volatile("s_waitcnt vmcnt(%7)" : "+v"(w[0]), "+v"(w[1]), "+v"(w[2]), "+v"(w[3]), "+v"(w[4]), "+v"(w[5]),
                 "+v"(w[6]) : "i"(LEFT) : "memory");
  }
}

template <int R, int C, int LB, int EPI, bool XN>
__global__ __launch_bounds__(256) void gemv8_kernel(const uint16_t* __restrict__ X, const uint8_t* __restrict__ W,
                                                    const float* __restrict__ SC, uint16_t* __restrict__ Y,
                                                    float* __restrict__ P, int N, int K, int Ks, XNormIn xn,
                                                    int* __restrict__ pi = nullptr, int n_valid = 0) {
  typedef typename Fp8Chunk<LB>::T WT;
  constexpr int XL = C * LB / 8;      // 16-byte input-row loads per lane
  constexpr int CK = 64 * LB;         // k covered by one wave-wide chunk
  static_assert((R & (R - 1)) == 0, "R a power of two");
  static_assert(EPI == EPI_PARTIAL || R % 16 == 0, "GLU / ARGMAX: whole 16-row groups");
  static_assert(R <= 64 && 1 + XL + R * C <= 63, "loads in flight per lane must fit the vmcnt counter");
  __shared__ __attribute__((aligned(16))) uint16_t sx[XN ? kXnMaxK : 8];
  __shared__ float red[4][R];
  __shared__ float xred[4];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n0 = blockIdx.x * R, slice = blockIdx.y, kbeg = slice * Ks;
  const int kw = kbeg + wave * (Ks >> 2);           // this wave's k range
  // issue order: row scale, input row, weights (row-major) -- retired in that order
  float sc;
  gload4(sc, SC + n0 + (tid & (R - 1)));
  bf16x8 xr[XL];
  if constexpr (!XN) {
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
      for (int h = 0; h < LB / 8; ++h) gload16<0>(xr[c * (LB / 8) + h], X + kw + c * CK + lane * LB + h * 8);
  }
  // weight chunk (r, c) of this lane: row n0 + r, k = kw + c * CK + lane * LB
  WT w[R][C];
  const uint8_t* wb = W + (size_t)n0 * K + kw + lane * LB;
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int c = 0; c < C; ++c) gload_fp8_nt<LB>(w[r][c], wb + (size_t)r * K + c * CK);
  float xf[XL][8];
  if constexpr (XN) {
    xnorm_prologue(xn, K, kbeg, Ks, blockIdx.x == 0 && blockIdx.y == 0, sx, xred);
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
      for (int h = 0; h < LB / 8; ++h)
        unpack8(*reinterpret_cast<const uint4*>(sx + (kw - kbeg) + c * CK + lane * LB + h * 8), xf[c * (LB / 8) + h]);
  } else {
#pragma unroll
    for (int i = 0; i < XL; ++i) {
      wait_vm_reg<R * C>(xr[i]);
      unpack8(__builtin_bit_cast(uint4, xr[i]), xf[i]);
    }
  }
  wait_vm_reg<R * C>(sc);
  float acc[R];
  static_for<0, R>([&](auto rc) {
    constexpr int r = decltype(rc)::value;
    // row r's chunks landed: everything issued after them is the later rows' C chunks each
    wait_vm_row<(R - 1 - r) * C, C>(w[r]);
    float a = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
      for (int d = 0; d < LB / 4; ++d) {
        const float* xv = &xf[c * (LB / 8) + (d >> 1)][(d & 1) * 4];
        const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[r][c][d], false);
        const f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[r][c][d], true);
        a = fmaf(lo[0], xv[0], a);
        a = fmaf(lo[1], xv[1], a);
        a = fmaf(hi[0], xv[2], a);
        a = fmaf(hi[1], xv[3], a);
      }
    acc[r] = wave_sum(a);
  });
  if (lane == 0) {
#pragma unroll
    for (int r = 0; r < R; ++r) red[wave][r] = acc[r];
  }
  __syncthreads();
  if (tid >= 64) return;
  // lane r < R of wave 0: output row n0 + r, scaled
  const int rr = tid & (R - 1);
  const float v = (red[0][rr] + red[1][rr] + red[2][rr] + red[3][rr]) * sc;
  if constexpr (EPI == EPI_PARTIAL) {
    if (tid < R) P[(size_t)slice * N + n0 + tid] = v;
  } else if constexpr (EPI == EPI_ARGMAX) {
    // the R logits (bf16-rounded, as the unfused logits) -> one (value, id) partial per
    // workgroup at P / pi [blockIdx.x]
    float bv = -FLT_MAX;
    int bi = 0x7fffffff;
    if (tid < R && n0 + tid < n_valid) {
      bv = bf2f(f2bf(v));
      bi = n0 + tid;
    }
#pragma unroll
    for (int o = 1; o < R; o <<= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      argmax_better(bv, bi, ov, oi);
    }
    if (tid == 0) {
      P[blockIdx.x] = bv;
      pi[blockIdx.x] = bi;
    }
  } else {
    // group g: gate rows 16 g .. 16 g + 7, up rows 16 g + 8 .. 16 g + 15 -> outputs 8 g .. 8 g + 7
    const int t = tid & (R / 2 - 1), gi = (t >> 3) * 16 + (t & 7);
    const float g = __shfl(v, gi, 64), u = __shfl(v, gi + 8, 64);
    if (tid < R / 2) {
      const float gv = bf2f(f2bf(g)), uv = bf2f(f2bf(u));   // as the bf16 GEMM output
      Y[(n0 >> 1) + tid] = f2bf(silu(gv) * uv);
      // a gate below -80 (never in a real model): the store repeated with silu_times, behind a
      // branch of its own so that its second exp stays off every other workgroup's tail
      if (silu_second_pass(gv)) Y[(n0 >> 1) + tid] = f2bf(silu_times(gv, uv));
    }
  }
}

template <int EPI, bool XN>
int launch_gemv8(int R, int C, int LB, dim3 grid, hipStream_t s, const uint16_t* x, const uint8_t* w, const float* sc,
                 uint16_t* y, float* p, int N, int K, int Ks, const XNormIn& xn, int* pi = nullptr, int nv = 0) {
#define GEMV8_CASE(RR, CC, LL)                                                                           \
  if (R == RR && C == CC && LB == LL) {                                                                  \
    gemv8_kernel<RR, CC, LL, EPI, XN><<<grid, 256, 0, s>>>(x, w, sc, y, p, N, K, Ks, xn, pi, nv);        \
    return 0;                                                                                            \
  }
  if constexpr (EPI == EPI_PARTIAL) {
    GEMV8_CASE(8, 1, 8) GEMV8_CASE(16, 1, 8) GEMV8_CASE(8, 2, 8) GEMV8_CASE(16, 2, 8)
    GEMV8_CASE(8, 1, 16) GEMV8_CASE(16, 1, 16) GEMV8_CASE(32, 1, 16)
    if constexpr (!XN) {   // K > kXnMaxK: never the in-kernel input row
      GEMV8_CASE(4, 4, 8) GEMV8_CASE(8, 4, 8) GEMV8_CASE(4, 7, 8) GEMV8_CASE(8, 2, 16) GEMV8_CASE(16, 2, 16)
    }
  } else {
    GEMV8_CASE(16, 1, 8) GEMV8_CASE(32, 1, 8) GEMV8_CASE(16, 2, 8) GEMV8_CASE(16, 1, 16) GEMV8_CASE(32, 1, 16)
  }
#undef GEMV8_CASE
  return -1;
}

// shared shape rules of the FP8 GEMV entry points; C (chunks per lane) out
bool gemv8_shape(int N, int K, int S, int R, int LB, int* C) {
  if (N < 1 || K < 1 || S < 1 || R < 1 || (LB != 8 && LB != 16) || K % S || N % R) return false;
  const int Ks = K / S;
  if (Ks % (256 * LB)) return false;
  *C = Ks / (256 * LB);
  return true;
}
}  // namespace

// Batch-1 GEMV over FP8 weights (see gemv8_kernel): Wq [N, K] e4m3fn codes, scale [N] fp32.
// epi 0: fp32 slabs P [S, 1, N]; epi 1: SwiGLU Y [1, N / 2] (R % 16 == 0, S = 1).  LB: codes per
// lane per load (8 or 16).  Pin != null: the input row from the previous projection's slabs.
// -1 for any shape / (R, C, LB) without an instantiation: nothing is launched.
int docqa_gemv8(const void* X, const void* Wq, const float* scale, void* Y, float* P, int N, int K, int S, int R,
                int LB, int epi, const float* Pin, int Sin, const void* res_in, void* res_out, const void* gamma,
                float eps, hipStream_t s) {
  int C = 0;
  if (!gemv8_shape(N, K, S, R, LB, &C) || !Wq || !scale || !docqa_aligned16(Wq)) return -1;
  const int Ks = K / S;
  const bool xnm = Pin != nullptr;
  const XNormIn xn{Pin, Sin, (const uint16_t*)res_in, (uint16_t*)res_out, (const uint16_t*)gamma, eps};
  if (xnm && !xn_ok(N, K, 1, R, xn)) return -1;
  if (!xnm && (!X || !docqa_aligned16(X))) return -1;
  if (epi == 1 ? (R % 16 || S != 1 || !Y) : !P) return -1;
  const dim3 grid(N / R, S);
  const uint16_t* x = (const uint16_t*)X;
  const uint8_t* w = (const uint8_t*)Wq;
  int rc;
  if (epi == 1)
    rc = xnm ? launch_gemv8<EPI_GLU, true>(R, C, LB, grid, s, x, w, scale, (uint16_t*)Y, nullptr, N, K, Ks, xn)
             : launch_gemv8<EPI_GLU, false>(R, C, LB, grid, s, x, w, scale, (uint16_t*)Y, nullptr, N, K, Ks, xn);
  else
    rc = xnm ? launch_gemv8<EPI_PARTIAL, true>(R, C, LB, grid, s, x, w, scale, nullptr, P, N, K, Ks, xn)
             : launch_gemv8<EPI_PARTIAL, false>(R, C, LB, grid, s, x, w, scale, nullptr, P, N, K, Ks, xn);
  if (rc) return rc;
  DOCQA_CHECK_LAUNCH();
  return 0;
}

// Batch-1 LM head + greedy pick over FP8 weights: R (16 or 32) vocabulary rows per workgroup,
// one (value, id) partial each, merged by argmax_merge_kernel.  ws_v / ws_i: N / R entries.
int docqa_gemv8_argmax(const void* X, const void* Wq, const float* scale, int64_t* out, float* outv, float* ws_v,
                       int* ws_i, int N, int K, int R, int LB, int n_valid, hipStream_t s) {
  int C = 0;
  if (!gemv8_shape(N, K, 1, R, LB, &C) || R % 16 || !X || !Wq || !scale || !out || !ws_v || !ws_i ||
      !docqa_aligned16(X) || !docqa_aligned16(Wq) || n_valid <= 0 || n_valid > N)
    return -1;
  const int rc = launch_gemv8<EPI_ARGMAX, false>(R, C, LB, dim3(N / R), s, (const uint16_t*)X, (const uint8_t*)Wq,
                                                 scale, nullptr, ws_v, N, K, K, XNormIn{}, ws_i, n_valid);
  if (rc) return rc;
  argmax_merge_kernel<<<1, 256, 0, s>>>(ws_v, ws_i, N / R, out, outv);
  DOCQA_CHECK_LAUNCH();
  return 0;
}

// ---------------------------------------------------------------------------------------
// MXFP4 weight stream for the batch-1 GEMV: the register-streaming design of gemv8_kernel over
// OCP microscaling weights -- Wq [N, K / 2] bytes of two e2m1 codes (element 2j in bits 0..3,
// 2j + 1 in bits 4..7) and E [N, K / 32] e8m0 block scales, W'[n, k] = code * 2^(E[n, k / 32] - 127)
// (exactly the model's resident bf16 weights), so a projection moves 4.25 bits per weight.
//   * Lane-to-block map: a lane's load is LB = 32 codes (16 B: exactly one scale block) or 16
//     codes (8 B: two lanes share a block), and KW of the 4 waves split K while the other
//     4 / KW split the R rows (RW = R KW / 4 rows per wave).  Four bits per weight leave a wave
//     too few bytes when all four split a 2048..4096-long K, so the short K run KW = 1 | 2 with
//     whole-block 16-byte loads; a wave's 64 scale bytes of one chunk are contiguous in E
//     (one byte load per chunk, 64 B per wave).
//   * Issue order: block scales, the input row (bf16, unless XN builds it in LDS), then RW rows
//     x C chunks of codes, non-temporal; retired in that order with counted vmcnt waits.
//   * v_cvt_scalef32_pk_bf16_fp4 widens two codes per instruction with the block scale applied
//     (the scale operand is the fp32 E << 23: no multiply, nothing left for the epilogue; a code
//     times a power of two is exact in bf16), v_dot2_f32_bf16 against the packed bf16 input row
//     accumulates in fp32 -- one conversion and one dot per two weights, the input row never
//     unpacked; the waves meet in LDS.
// Epilogues as gemv8_kernel (EPI_PARTIAL slabs, EPI_GLU, EPI_ARGMAX).
// Shapes: N % R == 0, Ks = K / S = KW C 64 LB, and 2 RW C + C LB / 8 <= 63 loads per lane.
namespace {
__device__ __forceinline__ void gload_ubyte(uint32_t& d, const void* p) {
  asm volatile("global_load_ubyte %0, %1, off" : "=v"(d) : "v"(p) : "memory");
}

template <int R, int C, int LB, int KW, int EPI, bool XN>
__global__ __launch_bounds__(256) void gemv4_kernel(const uint16_t* __restrict__ X, const uint8_t* __restrict__ W,
                                                    const uint8_t* __restrict__ E, uint16_t* __restrict__ Y,
                                                    float* __restrict__ P, int N, int K, int Ks, XNormIn xn,
                                                    int* __restrict__ pi = nullptr, int n_valid = 0) {
  typedef typename Fp8Chunk<LB / 2>::T WT;   // LB / 2 bytes of codes per load
  constexpr int RW = R * KW / 4;      // rows per wave
  constexpr int XH = LB / 8;          // 16-byte input-row loads per chunk
  constexpr int XL = C * XH;
  constexpr int CK = 64 * LB;         // k covered by one wave-wide chunk
  static_assert(LB == 16 || LB == 32, "8- or 16-byte code loads");
  static_assert(KW == 1 || KW == 2 || KW == 4, "waves along K");
  static_assert((R & (R - 1)) == 0 && R <= 64 && RW >= 1 && RW * 4 == R * KW, "R a power of two, whole rows per wave");
  static_assert(EPI == EPI_PARTIAL || R % 16 == 0, "GLU / ARGMAX: whole 16-row groups");
  static_assert(2 * RW * C + XL <= 63, "loads in flight per lane must fit the vmcnt counter");
  __shared__ __attribute__((aligned(16))) uint16_t sx[XN ? kXnMaxK : 8];
  __shared__ float red[KW][R];
  __shared__ float xred[4];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kg = wave % KW, rg = wave / KW;          // this wave's k group and row group
  const int n0 = blockIdx.x * R, slice = blockIdx.y, kbeg = slice * Ks;
  const int kw = kbeg + kg * (Ks / KW);              // this wave's k range
  const int nw = n0 + rg * RW;                       // this wave's first row
  // issue order: block scales, input row, codes (row-major) -- retired in that order
  // chunk (r, c) of this lane: row nw + r, k = kw + c * CK + lane * LB .. + LB
  uint32_t sc[RW][C];
  const uint8_t* eb = E + (size_t)nw * (K >> 5) + ((kw + lane * LB) >> 5);
#pragma unroll
  for (int r = 0; r < RW; ++r)
#pragma unroll
    for (int c = 0; c < C; ++c) gload_ubyte(sc[r][c], eb + (size_t)r * (K >> 5) + c * (CK >> 5));
  bf16x8 xr[XL];
  if constexpr (!XN) {
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
      for (int h = 0; h < XH; ++h) gload16<0>(xr[c * XH + h], X + kw + c * CK + lane * LB + h * 8);
  }
  WT w[RW][C];
  const uint8_t* wb = W + (size_t)nw * (K >> 1) + ((kw + lane * LB) >> 1);
#pragma unroll
  for (int r = 0; r < RW; ++r)
#pragma unroll
    for (int c = 0; c < C; ++c) gload_fp8_nt<LB / 2>(w[r][c], wb + (size_t)r * (K >> 1) + c * (CK >> 1));
  if constexpr (XN) {
    xnorm_prologue(xn, K, kbeg, Ks, blockIdx.x == 0 && blockIdx.y == 0, sx, xred);
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
      for (int h = 0; h < XH; ++h)
        xr[c * XH + h] = *reinterpret_cast<const bf16x8*>(sx + (kw - kbeg) + c * CK + lane * LB + h * 8);
  } else {
#pragma unroll
    for (int i = 0; i < XL; ++i) wait_vm_reg<RW * C>(xr[i]);
  }
  float acc[RW];
  static_for<0, RW>([&](auto rc) {
    constexpr int r = decltype(rc)::value;
    // row r's chunks (and, issued before them, every scale) landed: everything issued after
    // them is the later rows' C chunks each
    wait_vm_row<(RW - 1 - r) * C, C>(w[r]);
    float a = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      wait_vm_reg<(RW - 1 - r) * C>(sc[r][c]);
      const float scale = __uint_as_float(sc[r][c] << 23);   // e8m0 -> fp32 2^(e - 127)
#pragma unroll
      for (int d = 0; d < LB / 8; ++d) {
        const uint32_t cw = w[r][c][d];                      // 8 codes: k = 8 d .. 8 d + 7 of the chunk
        const bf16x8 xv = xr[c * XH + d];
        const bf16x2 w0 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(cw, scale, 0);
        const bf16x2 w1 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(cw, scale, 1);
        const bf16x2 w2 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(cw, scale, 2);
        const bf16x2 w3 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(cw, scale, 3);
        a = __builtin_amdgcn_fdot2_f32_bf16(w0, bf16x2{xv[0], xv[1]}, a, false);
        a = __builtin_amdgcn_fdot2_f32_bf16(w1, bf16x2{xv[2], xv[3]}, a, false);
        a = __builtin_amdgcn_fdot2_f32_bf16(w2, bf16x2{xv[4], xv[5]}, a, false);
        a = __builtin_amdgcn_fdot2_f32_bf16(w3, bf16x2{xv[6], xv[7]}, a, false);
      }
    }
    acc[r] = wave_sum(a);
  });
  if (lane == 0) {
#pragma unroll
    for (int r = 0; r < RW; ++r) red[kg][rg * RW + r] = acc[r];
  }
  __syncthreads();
  if (tid >= 64) return;
  // lane r < R of wave 0: output row n0 + r
  const int rr = tid & (R - 1);
  float v = red[0][rr];
#pragma unroll
  for (int g = 1; g < KW; ++g) v += red[g][rr];
  if constexpr (EPI == EPI_PARTIAL) {
    if (tid < R) P[(size_t)slice * N + n0 + tid] = v;
  } else if constexpr (EPI == EPI_ARGMAX) {
    // the R logits (bf16-rounded, as the unfused logits) -> one (value, id) partial per
    // workgroup at P / pi [blockIdx.x]
    float bv = -FLT_MAX;
    int bi = 0x7fffffff;
    if (tid < R && n0 + tid < n_valid) {
      bv = bf2f(f2bf(v));
      bi = n0 + tid;
    }
#pragma unroll
    for (int o = 1; o < R; o <<= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      argmax_better(bv, bi, ov, oi);
    }
    if (tid == 0) {
      P[blockIdx.x] = bv;
      pi[blockIdx.x] = bi;
    }
  } else {
    // group g: gate rows 16 g .. 16 g + 7, up rows 16 g + 8 .. 16 g + 15 -> outputs 8 g .. 8 g + 7
    const int t = tid & (R / 2 - 1), gi = (t >> 3) * 16 + (t & 7);
    const float g = __shfl(v, gi, 64), u = __shfl(v, gi + 8, 64);
    if (tid < R / 2) {
      const float gv = bf2f(f2bf(g)), uv = bf2f(f2bf(u));   // as the bf16 GEMM output
      Y[(n0 >> 1) + tid] = f2bf(silu(gv) * uv);
      // a gate below -80 (never in a real model): the store repeated with silu_times, behind a
      // branch of its own so that its second exp stays off every other workgroup's tail
      if (silu_second_pass(gv)) Y[(n0 >> 1) + tid] = f2bf(silu_times(gv, uv));
    }
  }
}

template <int EPI, bool XN>
int launch_gemv4(int R, int C, int LB, int KW, dim3 grid, hipStream_t s, const uint16_t* x, const uint8_t* w,
                 const uint8_t* e, uint16_t* y, float* p, int N, int K, int Ks, const XNormIn& xn, int* pi = nullptr,
                 int nv = 0) {
#define GEMV4_CASE(RR, CC, LL, WW)                                                                        \
  if (R == RR && C == CC && LB == LL && KW == WW) {                                                      \
    gemv4_kernel<RR, CC, LL, WW, EPI, XN><<<grid, 256, 0, s>>>(x, w, e, y, p, N, K, Ks, xn, pi, nv);     \
    return 0;                                                                                            \
  }
  if constexpr (EPI == EPI_PARTIAL) {
    GEMV4_CASE(16, 1, 32, 1) GEMV4_CASE(32, 1, 32, 1) GEMV4_CASE(8, 1, 32, 2) GEMV4_CASE(16, 1, 32, 2)
    GEMV4_CASE(16, 2, 32, 1) GEMV4_CASE(8, 1, 16, 4) GEMV4_CASE(8, 1, 16, 2)
    if constexpr (!XN) {   // K > kXnMaxK: never the in-kernel input row
      GEMV4_CASE(8, 1, 32, 4) GEMV4_CASE(16, 1, 32, 4) GEMV4_CASE(4, 7, 32, 1) GEMV4_CASE(8, 7, 32, 1)
      GEMV4_CASE(4, 7, 16, 2)
    }
  } else {
    GEMV4_CASE(16, 1, 32, 1) GEMV4_CASE(32, 1, 32, 1) GEMV4_CASE(16, 1, 32, 2) GEMV4_CASE(32, 1, 32, 2)
    GEMV4_CASE(16, 2, 32, 1) GEMV4_CASE(16, 1, 16, 4)
  }
#undef GEMV4_CASE
  return -1;
}

// shared shape rules of the MXFP4 GEMV entry points; C (chunks per lane) out
bool gemv4_shape(int N, int K, int S, int R, int LB, int KW, int* C) {
  if (N < 1 || K < 1 || S < 1 || R < 1 || (LB != 16 && LB != 32) || (KW != 1 && KW != 2 && KW != 4) || K % 32 ||
      K % S || N % R)
    return false;
  const int Ks = K / S;
  if (Ks % (64 * LB * KW)) return false;
  *C = Ks / (64 * LB * KW);
  return true;
}
}  // namespace

// Batch-1 GEMV over MXFP4 weights (see gemv4_kernel): Wq [N, K / 2] e2m1 code pairs, E [N, K / 32]
// e8m0 block scales.  epi 0: fp32 slabs P [S, 1, N]; epi 1: SwiGLU Y [1, N / 2] (R % 16 == 0,
// S = 1).  LB: codes per lane per load (16 | 32), KW: waves along K (1 | 2 | 4).  Pin != null: the
// input row from the previous projection's slabs.
// -1 for any shape / (R, C, LB, KW) without an instantiation: nothing is launched.
int docqa_gemv4(const void* X, const void* Wq, const void* E, void* Y, float* P, int N, int K, int S, int R, int LB,
                int KW, int epi, const float* Pin, int Sin, const void* res_in, void* res_out, const void* gamma,
                float eps, hipStream_t s) {
  int C = 0;
  if (!gemv4_shape(N, K, S, R, LB, KW, &C) || !Wq || !E || !docqa_aligned16(Wq)) return -1;
  const int Ks = K / S;
  const bool xnm = Pin != nullptr;
  const XNormIn xn{Pin, Sin, (const uint16_t*)res_in, (uint16_t*)res_out, (const uint16_t*)gamma, eps};
  if (xnm && !xn_ok(N, K, 1, R, xn)) return -1;
  if (!xnm && (!X || !docqa_aligned16(X))) return -1;
  if (epi == 1 ? (R % 16 || S != 1 || !Y) : !P) return -1;
  const dim3 grid(N / R, S);
  const uint16_t* x = (const uint16_t*)X;
  const uint8_t* w = (const uint8_t*)Wq;
  const uint8_t* e = (const uint8_t*)E;
  int rc;
  if (epi == 1)
    rc = xnm ? launch_gemv4<EPI_GLU, true>(R, C, LB, KW, grid, s, x, w, e, (uint16_t*)Y, nullptr, N, K, Ks, xn)
             : launch_gemv4<EPI_GLU, false>(R, C, LB, KW, grid, s, x, w, e, (uint16_t*)Y, nullptr, N, K, Ks, xn);
  else
    rc = xnm ? launch_gemv4<EPI_PARTIAL, true>(R, C, LB, KW, grid, s, x, w, e, nullptr, P, N, K, Ks, xn)
             : launch_gemv4<EPI_PARTIAL, false>(R, C, LB, KW, grid, s, x, w, e, nullptr, P, N, K, Ks, xn);
  if (rc) return rc;
  DOCQA_CHECK_LAUNCH();
  return 0;
}

// Batch-1 LM head + greedy pick over MXFP4 weights: R (16 or 32) vocabulary rows per workgroup,
// one (value, id) partial each, merged by argmax_merge_kernel.  ws_v / ws_i: N / R entries.
int docqa_gemv4_argmax(const void* X, const void* Wq, const void* E, int64_t* out, float* outv, float* ws_v,
                       int* ws_i, int N, int K, int R, int LB, int KW, int n_valid, hipStream_t s) {
  int C = 0;
  if (!gemv4_shape(N, K, 1, R, LB, KW, &C) || R % 16 || !X || !Wq || !E || !out || !ws_v || !ws_i ||
      !docqa_aligned16(X) || !docqa_aligned16(Wq) || n_valid <= 0 || n_valid > N)
    return -1;
  const int rc = launch_gemv4<EPI_ARGMAX, false>(R, C, LB, KW, dim3(N / R), s, (const uint16_t*)X, (const uint8_t*)Wq,
                                                 (const uint8_t*)E, nullptr, ws_v, N, K, K, XNormIn{}, ws_i, n_valid);
  if (rc) return rc;
  argmax_merge_kernel<<<1, 256, 0, s>>>(ws_v, ws_i, N / R, out, outv);
  DOCQA_CHECK_LAUNCH();
  return 0;
}

// ---------------------------------------------------------------------------------------
// FP8 weight stream for decode steps of 2..32 rows: dgemm_kernel's ring pipeline (256 threads,
// workgroup = NT x 16 weight rows x all M rows x one K slice, X fragments straight to VGPRs
// one k-block ahead, counted vmcnt waits, ring_barrier, XCD-aware slice remap,
// v_mfma_f32_16x16x32_bf16) over the e4m3fn codes Wq [N, K] + scale [N] of gemv8_kernel.
//   * Ring depth: bytes in flight per CU are what the design is about, so a stage keeps the
//     bf16 kernel's BYTES, not its k-depth: 256 codes (256 B) per weight row = twice the k per
//     stage, 4 slots, the same NT LDS-DMA wave-instructions (glds16<true>, 16 B per lane, nt)
//     per wave per stage and therefore the same issue order and vmcnt counts.  K granule: one
//     ring turn = 4 x 256 = 1024 (Ks % 1024 == 0).
//   * LDS layout: stage = [NT 16][256 B], i.e. 16 chunks of 16 B per row -- byte for byte the
//     bf16 stage, so the bf16 kernel's source swizzle carries over with chunks counted in bytes:
//     chunk c of row r lands at chunk position c ^ (r & 15).  The B fragment of k-step ks (32
//     codes) for lane (fr = lane & 15, fq = lane >> 4) is the 8 codes k = 32 ks + 8 fq .. + 7 of
//     row 16 nt + fr: chunk c = 2 ks + (fq >> 1), half (fq & 1), one ds_read_b64 at
//       row * 256 + ((c ^ fr) << 4) + (fq & 1) * 8.
//     ds_read_b64 is served in two 32-lane groups {0..31}, {32..63}, bank = (addr / 4) % 64
//     (MI355X_MICROARCH.md, LDS): a group is conflict-free iff its 32 lanes hit 32 distinct 8-B
//     slots of the 256-B bank row.  Inside a group fq >> 1 is constant, so c is one value, and
//     row * 256 == 0 (mod 256): the slot is ((c ^ fr) << 1) + (fq & 1); fr = 0..15 makes c ^ fr
//     a permutation of the 16 chunk positions and fq & 1 picks the half -- 32 distinct slots.
//   * B fragment: v_cvt_scalef32_pk_bf16_fp8 (scale 1.0) widens two codes per instruction,
//     four per fragment; exact (every e4m3fn value is a bf16 value; quantize_fp8_rows
//     saturates, so no NaN codes).
//   * Accumulators fp32; the row scale (the C/D column = weight row: one value per lane per
//     n-tile) multiplies them once after the k loop, before the k-group sum and any bf16
//     rounding (exact: a power of two).
//   * MT = 1 (2..16 rows, the four waves split k) and MT = 2 (17..32 rows, two k-groups).  At
//     33+ rows every wave of this mapping would widen every fragment (4x redundant VALU work per
//     byte): 33..128 rows take dgemm8w_kernel below, whose waves own n-tiles instead.
//   * Epilogues: EPI_PARTIAL / EPI_GLU / EPI_ARGMAX as dgemm_kernel's k-group (KW > 1) paths.
namespace {
constexpr int BK8 = 256;                  // codes (= bytes) per weight row per stage
constexpr int KSTEPS8 = BK8 / 32;         // 16x16x32 k-steps per stage

__device__ __forceinline__ int w8_off(int row, int ch, int half) {   // byte offset in a stage
  return row * BK8 + ((ch ^ (row & 15)) << 4) + half * 8;
}

// 8 e4m3fn codes -> the bf16x8 B fragment
__device__ __forceinline__ bf16x8 widen8(u32x2 c) {
  const bf16x2 a = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c[0], 1.0f, false);
  const bf16x2 b = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c[0], 1.0f, true);
  const bf16x2 d = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c[1], 1.0f, false);
  const bf16x2 e = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c[1], 1.0f, true);
  return bf16x8{a[0], a[1], b[0], b[1], d[0], d[1], e[0], e[1]};
}

template <int EPI, int MT, int NT>
__global__ __launch_bounds__(256) void dgemm8_kernel(const uint16_t* __restrict__ X, const uint8_t* __restrict__ W,
                                                     const float* __restrict__ SC, uint16_t* __restrict__ Y,
                                                     float* __restrict__ P, int M, int N, int K, int Ks,
                                                     int xcd_remap, float* __restrict__ pv = nullptr,
                                                     int* __restrict__ pi = nullptr, int n_valid = 0) {
  static_assert(MT == 1 || MT == 2, "2..16 rows (MT = 1) or 17..32 rows (MT = 2)");
  static_assert(EPI == EPI_PARTIAL || EPI == EPI_GLU || EPI == EPI_ARGMAX, "slabs, SwiGLU or argmax");
  constexpr int NSR = NS;                        // ring slots
  constexpr int KW = 4 / MT, SPW = KSTEPS8 / KW; // k-groups; k-steps (= X fragments) per wave per stage
  constexpr int VW = 2 * NT + SPW;               // vector-memory ops in flight at the top of a step
  constexpr int STAGE = NT * 16 * BK8;           // bytes of one W stage (NT x 4 KB)
  __shared__ __attribute__((aligned(16))) uint8_t sw[NSR * STAGE];   // W ring
  int tile = blockIdx.x, slice = blockIdx.y;
  if (xcd_remap) {   // XCD x only runs slice x % S (see dgemm_kernel)
    const int S = gridDim.y;
    const int L = blockIdx.x + blockIdx.y * gridDim.x;
    const int xcd = L & 7, j = L >> 3;
    slice = xcd % S;
    tile = j * (8 / S) + xcd / S;
  }
  const int n0 = tile * NT * 16;
  const int kbeg = slice * Ks;
  const int nkb = Ks / BK8;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fq = lane >> 4;
  const int mt = wave % MT, kg = wave / MT;
  // this lane's row scales, first in the queue: retired by the first counted wait
  float sc[NT];
#pragma unroll
  for (int i = 0; i < NT; ++i) gload4(sc[i], SC + n0 + i * 16 + fr);
  const uint16_t* xrow = X + (size_t)min(mt * 16 + fr, M - 1) * K + kbeg + kg * SPW * 32 + fq * 8;
  const uint32_t ring = lds_u32(sw);

  f32x4 acc[NT];
#pragma unroll
  for (int i = 0; i < NT; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};

  // W stage j -> ring slot j % NSR: 4 NT wave-instructions of 64 lanes x 16 B (4 rows each), NT
  // per wave, source XOR-swizzled; clamped past the last stage (see dgemm_kernel)
  const uint8_t* wsrc[NT];
#pragma unroll
  for (int i = 0; i < NT; ++i) {
    const int p = (i * 4 + wave) * 64 + lane;
    const int r = p >> 4;
    wsrc[i] = W + (size_t)(n0 + r) * K + kbeg + (((p & 15) ^ (r & 15)) << 4);
  }
  auto stage_w = [&](int j) {
    const int koff = min(j, nkb - 1) * BK8;
    const uint32_t dst = ring + (uint32_t)((j % NSR) * STAGE);
#pragma unroll
    for (int i = 0; i < NT; ++i) glds16<true>(wsrc[i] + koff, dst + (uint32_t)((i * 4 + wave) * 1024));
  };
  auto load_x = [&](bf16x8 (&x)[SPW], int j) {
    const uint16_t* src = xrow + min(j, nkb - 1) * BK8;
    gload16<0>(x[0], src);
    gload16<64>(x[1], src);
    if constexpr (SPW > 2) { gload16<128>(x[2], src); gload16<192>(x[3], src); }
  };
  // n-tile byte offsets, opaque to hipcc: with constant distances it merges the reads of two
  // n-tiles into ds_read2st64_b64, which is banked mod 32 in 16-lane groups -- there this
  // layout is 2-way conflicted, at half the bytes per clock of ds_read_b64
  int ntoff[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    ntoff[nt] = nt * 16 * BK8;
    asm volatile("" : "+v"(ntoff[nt]));
  }
  auto mma = [&](const bf16x8 (&x)[SPW], int j) {
    const uint8_t* src = sw + (j % NSR) * STAGE;
#pragma unroll
    for (int s = 0; s < SPW; ++s) {
      const int ch = (kg * SPW + s) * 2 + (fq >> 1);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const u32x2 c = *reinterpret_cast<const u32x2*>(src + ntoff[nt] + w8_off(fr, ch, fq & 1));
        acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(x[s], widen8(c), acc[nt], 0, 0, 0);
      }
    }
  };
  // issue order and counted waits: dgemm_kernel's XA = 2 schedule (W0 X0 W1 X1 W2 | step i:
  // X(i+2) W(i+3)); nkb % 4 == 0
  bf16x8 x0[SPW], x1[SPW], x2[SPW], x3[SPW];
  // the row scales are the oldest loads in the queue: every counted wait has retired them, and
  // naming their registers right there (no instruction) keeps anything that reads or moves them
  // below the first wait
  auto name_sc = [&] {
#pragma unroll
    for (int i = 0; i < NT; ++i) asm volatile("" : "+v"(sc[i]));
  };
#define RING_STEP8(I, XC, XNX)                                                          \
  wait_vm_n<VW>(XC);                                                                    \
  name_sc();                                                                            \
  ring_barrier();                                                                       \
  load_x(XNX, (I) + 2);                                                                 \
  stage_w((I) + NSR - 1);                                                               \
  mma(XC, I);
  stage_w(0);
  load_x(x0, 0);
  stage_w(1);
  load_x(x1, 1);
  stage_w(2);
  for (int i = 0; i < nkb; i += 4) {
    RING_STEP8(i, x0, x2)
    RING_STEP8(i + 1, x1, x3)
    RING_STEP8(i + 2, x2, x0)
    RING_STEP8(i + 3, x3, x1)
  }
#undef RING_STEP8
  wait_vm_n<0>(x0);
  keep_live(x1);
  keep_live(x2);
  keep_live(x3);
#pragma unroll
  for (int i = 0; i < NT; ++i) acc[i] *= sc[i];

  // sum the KW k-groups through LDS (ring is free after the last barrier + wait)
  __syncthreads();
  f32x4* red = reinterpret_cast<f32x4*>(sw);        // [wave][nt][lane] = one slot
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) red[(wave * NT + nt) * 64 + lane] = acc[nt];
  __syncthreads();
  const float* rf = reinterpret_cast<const float*>(sw);
  auto sum_k = [&](int m, int nt, int ln, int r) {
    float v = 0.f;
#pragma unroll
    for (int g = 0; g < KW; ++g) v += rf[(((g * MT + m) * NT + nt) * 64 + ln) * 4 + r];
    return v;
  };
  // C/D map of 16x16x32: col = lane & 15 (weight row), row = 4 * (lane >> 4) + r (X row)
  if constexpr (EPI == EPI_ARGMAX) {
    // the [rows, NT 16] logit tile through LDS (past the k-group reduction area), 4 lanes per
    // row -> one (value, id) partial per (row, tile)
    constexpr int TP = NT * 16 + 1;
    float* tl = reinterpret_cast<float*>(sw) + 4 * NT * 64 * 4;
    for (int idx = tid; idx < MT * NT * 256; idx += 256) {
      const int r = idx & 3, ln = (idx >> 2) & 63, q = idx >> 8;
      const int nt = q % NT, m = q / NT;
      tl[(m * 16 + (ln >> 4) * 4 + r) * TP + nt * 16 + (ln & 15)] = sum_k(m, nt, ln, r);
    }
    __syncthreads();
    const int ntiles = N / (NT * 16);
    for (int rr = tid >> 2; rr < MT * 16; rr += 64) {
      float bv = -FLT_MAX;
      int bi = 0x7fffffff;
      const int c0 = (tid & 3) * (NT * 4);
#pragma unroll 4
      for (int c = c0; c < c0 + NT * 4; ++c) {
        const int col = n0 + c;
        if (col < n_valid) argmax_better(bv, bi, bf2f(f2bf(tl[rr * TP + c])), col);
      }
#pragma unroll
      for (int o = 1; o <= 2; o <<= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        argmax_better(bv, bi, ov, oi);
      }
      if ((tid & 3) == 0 && rr < M) {
        pv[(size_t)rr * ntiles + tile] = bv;
        pi[(size_t)rr * ntiles + tile] = bi;
      }
    }
    return;
  }
  float glu_lo = 0.f;   // EPI_GLU: the smallest gate this lane has seen (silu_times_first)
  auto sweep = [&](auto second) {
#pragma unroll
    for (int e = 0; e < MT * NT; ++e) {
      const int idx = e * 256 + tid;                 // (m-tile, nt, lane, r)
      const int r = idx & 3, ln = (idx >> 2) & 63, q = idx >> 8;
      const int nt = q % NT, m = q / NT;
      const int row = m * 16 + (ln >> 4) * 4 + r, col = n0 + nt * 16 + (ln & 15);
      if (row >= M) continue;
      if constexpr (EPI == EPI_GLU) {
        // SwiGLU pair: gate value at an 8-block's low half, up value 8 columns later, both
        // rounded to bf16 first, as the unfused bf16 GEMM output
        if ((ln & 8) == 0) {
          const float gb = bf2f(f2bf(sum_k(m, nt, ln, r))), ub = bf2f(f2bf(sum_k(m, nt, ln + 8, r)));
          Y[(size_t)row * (N >> 1) + ((col >> 4) << 3) + (col & 7)] = f2bf(silu_times_pass(gb, ub, glu_lo, second));
        }
      } else {
        P[((size_t)slice * M + row) * N + col] = sum_k(m, nt, ln, r);
      }
    }
  };
  sweep(std::false_type{});
  if constexpr (EPI == EPI_GLU) {
    if (silu_second_pass(glu_lo)) sweep(std::true_type{});   // a gate below -80: silu_times for the wave's pairs
  }
}

constexpr int MR8 = 32;   // rows of the FP8 ring kernel (MT <= 2)

bool shape8_ok(int M, int N, int K, int S, int bn) {
  return M >= 1 && M <= MR8 && N >= bn && N % bn == 0 && S >= 1 && K % S == 0 && (K / S) >= NS * BK8 &&
         (K / S) % (NS * BK8) == 0;
}

template <int EPI, int NT>
void launch8(dim3 grid, hipStream_t s, const void* x, const void* w, const float* sc, uint16_t* y, float* p, int M,
             int N, int K, int Ks, float* pv = nullptr, int* pi = nullptr, int nv = 0) {
  const int S = grid.y;
  const int xr = (xcd_knob() && S > 1 && 8 % S == 0 && (grid.x * S) % 8 == 0) ? 1 : 0;
  const uint16_t* xp = (const uint16_t*)x;
  const uint8_t* wp = (const uint8_t*)w;
  if (M <= 16) dgemm8_kernel<EPI, 1, NT><<<grid, 256, 0, s>>>(xp, wp, sc, y, p, M, N, K, Ks, xr, pv, pi, nv);
  else dgemm8_kernel<EPI, 2, NT><<<grid, 256, 0, s>>>(xp, wp, sc, y, p, M, N, K, Ks, xr, pv, pi, nv);
}
}  // namespace

// 2..32-row decode projections over FP8 weights (see dgemm8_kernel; one row works too, the
// plans send it to the GEMV): Wq [N, K] e4m3fn codes, scale [N] fp32 powers of two.  All
// return -1, launching nothing, for a shape without an instantiation: more than 32 rows,
// N % tile, a K slice that is not whole 1024-deep ring turns, pointers off 16 B.
// fp32 slabs P [S, M, N]; tile_rows: 64
int docqa_dgemm8_partial(const void* X, const void* Wq, const float* scale, float* P, int M, int N, int K, int S,
                         int tile_rows, hipStream_t s) {
  if (M == 0) return 0;
  if (!X || !Wq || !scale || !P || tile_rows != 64 || !shape8_ok(M, N, K, S, 64) || !docqa_aligned16(X) ||
      !docqa_aligned16(Wq))
    return -1;
  launch8<EPI_PARTIAL, 4>(dim3(N / 64, S), s, X, Wq, scale, nullptr, P, M, N, K, K / S);
  DOCQA_CHECK_LAUNCH();
  return 0;
}

// Y [M, N / 2] = silu(gate) * up for the 8-interleaved gate|up codes Wq [N, K] (N = 2 I); 112-row
// tiles where they give >= 192 workgroups (as docqa_dgemm_glu), else 64-row tiles
int docqa_dgemm8_glu(const void* X, const void* Wq, const float* scale, void* Y, int M, int N, int K, hipStream_t s) {
  if (M == 0) return 0;
  if (!X || !Wq || !scale || !Y || !docqa_aligned16(X) || !docqa_aligned16(Wq)) return -1;
  if (shape8_ok(M, N, K, 1, 112) && N / 112 >= 192)
    launch8<EPI_GLU, 7>(dim3(N / 112), s, X, Wq, scale, (uint16_t*)Y, nullptr, M, N, K, K);
  else if (shape8_ok(M, N, K, 1, 64))
    launch8<EPI_GLU, 4>(dim3(N / 64), s, X, Wq, scale, (uint16_t*)Y, nullptr, M, N, K, K);
  else
    return -1;
  DOCQA_CHECK_LAUNCH();
  return 0;
}

// LM head + greedy pick: out[M] = argmax over the first n_valid columns of bf16(X . W'^T), outv[M]
// the picked value; ws_v / ws_i: [M, N / 64] per-tile partials
int docqa_dgemm8_argmax(const void* X, const void* Wq, const float* scale, int64_t* out, float* outv, float* ws_v,
                        int* ws_i, int M, int N, int K, int n_valid, hipStream_t s) {
  if (M == 0) return 0;
  if (!X || !Wq || !scale || !out || !ws_v || !ws_i || !shape8_ok(M, N, K, 1, 64) || n_valid <= 0 || n_valid > N ||
      !docqa_aligned16(X) || !docqa_aligned16(Wq))
    return -1;
  launch8<EPI_ARGMAX, 4>(dim3(N / 64), s, X, Wq, scale, nullptr, nullptr, M, N, K, K, ws_v, ws_i, n_valid);
  argmax_merge_kernel<<<M, 256, 0, s>>>(ws_v, ws_i, N / 64, out, outv);
  DOCQA_CHECK_LAUNCH();
  return 0;
}

// ---------------------------------------------------------------------------------------
// FP8 weight stream for decode steps of 33..128 rows (dgemm8w_kernel): the codes Wq [N, K] + scale
// [N] of dgemm8_kernel, the same arithmetic (codes widened exactly by
// v_cvt_scalef32_pk_bf16_fp8 at scale 1.0, v_mfma_f32_16x16x32_bf16 into fp32, the power-of-two
// row scale applied once after the k loop), another split of the work.  dgemm8_kernel's waves own
// (m-tile, k-group) pieces and share every B fragment, so with MT = 4 / 8 m-tiles each code would
// be widened 4 times per workgroup.  Here the WAVES OWN N-TILES:
//   * workgroup = 128 weight rows (NT = 8 n-tiles) x all M rows (MT = 4: 33..64, MT = 8:
//     65..128) x one K slice; wave w owns n-tiles 2w, 2w + 1 and runs every m-tile against them.
//     A B fragment is read and widened by exactly one wave, once, and then feeds MT MFMAs from
//     registers: one conversion per code per workgroup.
//   * X goes through LDS, staged once per workgroup per k-block next to the codes (all X fragments
//     of a stage in every wave's registers would be MT x 4 k-steps x 4 VGPRs per buffer).  A
//     workgroup therefore fetches its X slice from L2 once, like dgemm_kernel's, and covers 128
//     weight rows with it: per weight BYTE the X traffic equals the bf16 kernel's 64-row tiles
//     (and is half of it per weight row).
//   * Ring: stages of 128 k.  One slot = the X stage [MT 16][128] bf16 (MT x 4 KB) + the code
//     stage [128][128 B] (16 KB); MT = 4: 4 slots = 128 KB, MT = 8: 3 slots = 144 KB -- one
//     workgroup per CU either way, 32..48 KB of codes in flight per CU.  Both stages are filled by
//     LDS-DMA (glds16, 16 B per lane): no vector-memory result ever lands in a VGPR inside the
//     loop, so the counted vmcnt waits below are exact and no X register buffers exist.  Step i:
//     wait for stage i (the NSR - 2 younger stages stay in flight), s_barrier (publishes stage i,
//     frees slot (i - 1) % NSR), issue stage i + NSR - 1, MFMA over stage i.  Past the last stage
//     nothing is issued and the waits drain to 0 (wave-uniform branches), so K slices are any
//     multiple of one stage; the entry points ask for whole 512-deep turns (DGEMM8W_K).
//   * LDS layout and banks (MI355X_MICROARCH.md, LDS: 64 banks x 4 B = one 256-B bank row).
//     X stage: 256 B per row = 16 chunks of 16 B, chunk c of row r stored at chunk position
//     c ^ (r & 15) (the DMA destination is lane-linear, so the SOURCE is swizzled -- as
//     dgemm_kernel's weight stage).  The A fragment of k-step ks, lane (fr = lane & 15, fq =
//     lane >> 4) is chunk c = 4 ks + fq of row 16 mi + fr: one ds_read_b128 at
//     row * 256 + ((c ^ fr) << 4).  ds_read_b128 is served in four 16-lane groups, the first
//     {0-3, 12-15, 20-27}: fq = 0 with fr in {0..3, 12..15} and fq = 1 with fr in {4..11}.  A
//     row is one bank row, so a lane's 16-B slot is its chunk position: (4 ks) ^ fr for the
//     first eight lanes and (4 ks + 1) ^ fr = (4 ks) ^ (fr ^ 1) for the others -- fr ^ 1 maps
//     {4..11} onto itself, so the 16 lanes cover (4 ks) ^ {0..15}: 16 distinct slots, no
//     conflict.  The other three groups are the same sets shifted by fq pairs (2, 3) or with the
//     roles of the fr ranges exchanged.
//     Code stage: 128 B per row = 8 chunks, two rows per bank row; chunk c of row r is stored at
//     position c ^ ((r >> 1) & 7).  The B fragment (8 codes, k = 32 ks + 8 fq ..) is chunk c =
//     2 ks + (fq >> 1), half fq & 1: one ds_read_b64 at row * 128 + ((c ^ (fr >> 1)) << 4) +
//     (fq & 1) * 8.  ds_read_b64 is served in two 32-lane groups, in each fq >> 1 (so c) is
//     constant: the 8-B slot inside the bank row is (fr & 1) * 16 + (c ^ (fr >> 1)) * 2 +
//     (fq & 1); fr >> 1 = 0..7 makes c ^ (fr >> 1) a permutation of the 8 positions, fr & 1 picks
//     the row of the pair, fq & 1 the half -- 32 distinct slots, no conflict.
//   * Epilogues as dgemm_kernel's one-k-group paths: EPI_PARTIAL fp32 slabs, EPI_GLU (DPP row
//     rotate pairs gate and up, both rounded to bf16 first), EPI_ARGMAX through the drained ring.
namespace {
constexpr int BKW = 128;                  // k per stage: 128 codes (128 B) per weight row
constexpr int NTW8 = 8;                   // n-tiles per workgroup: 128 weight rows
constexpr int KGW = 512;                  // K-slice granule the entry points accept

template <int EPI, int MT>
__global__ __launch_bounds__(256) void dgemm8w_kernel(const uint16_t* __restrict__ X, const uint8_t* __restrict__ W,
                                                      const float* __restrict__ SC, uint16_t* __restrict__ Y,
                                                      float* __restrict__ P, int M, int N, int K, int Ks,
                                                      int xcd_remap, float* __restrict__ pv = nullptr,
                                                      int* __restrict__ pi = nullptr, int n_valid = 0) {
  static_assert(MT == 4 || MT == 8, "33..64 rows (MT = 4) or 65..128 rows (MT = 8)");
  static_assert(EPI == EPI_PARTIAL || EPI == EPI_GLU || EPI == EPI_ARGMAX, "slabs, SwiGLU or argmax");
  constexpr int NT = NTW8, NPW = NT / 4;         // n-tiles per workgroup / per wave
  constexpr int NSR = MT == 8 ? 3 : 4;           // ring slots
  constexpr int XB = MT * 16 * BKW * 2;          // bytes of one X stage
  constexpr int WB = NT * 16 * BKW;              // bytes of one code stage
  constexpr int SLOT = XB + WB;
  constexpr int XOPS = MT, WOPS = NT / 2;        // LDS-DMA wave-instructions per wave per stage
  constexpr int OPS = XOPS + WOPS;
  static_assert((NSR - 2) * OPS <= 63, "vmcnt is a 6-bit counter");
  __shared__ __attribute__((aligned(16))) uint8_t sw[NSR * SLOT];
  int tile = blockIdx.x, slice = blockIdx.y;
  if (xcd_remap) {   // XCD x only runs slice x % S (see dgemm_kernel)
    const int S = gridDim.y;
    const int L = blockIdx.x + blockIdx.y * gridDim.x;
    const int xcd = L & 7, j = L >> 3;
    slice = xcd % S;
    tile = j * (8 / S) + xcd / S;
  }
  const int n0 = tile * NT * 16;
  const int kbeg = slice * Ks;
  const int nkb = Ks / BKW;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fq = lane >> 4;
  const uint32_t ring = lds_u32(sw);

  // this lane's row scales (C/D column = weight row): read long before their use after the loop
  float sc[NPW];
#pragma unroll
  for (int j = 0; j < NPW; ++j) sc[j] = SC[n0 + (wave * NPW + j) * 16 + fr];

  // X stage: MT 4 pieces of 4 rows (1 KB), piece q = 4 t + wave; rows past M read row M - 1
  const uint16_t* xsrc[XOPS];
#pragma unroll
  for (int t = 0; t < XOPS; ++t) {
    const int r = (t * 4 + wave) * 4 + (lane >> 4);
    xsrc[t] = X + (size_t)min(r, M - 1) * K + kbeg + (((lane & 15) ^ (r & 15)) << 3);
  }
  // code stage: 16 pieces of 8 rows (1 KB), piece q = 4 t + wave
  const uint8_t* wsrc[WOPS];
#pragma unroll
  for (int t = 0; t < WOPS; ++t) {
    const int r = (t * 4 + wave) * 8 + (lane >> 3);
    wsrc[t] = W + (size_t)(n0 + r) * K + kbeg + (((lane & 7) ^ ((r >> 1) & 7)) << 4);
  }
  auto stage = [&](int j) {   // j < nkb
    const uint32_t dst = ring + (uint32_t)((j % NSR) * SLOT);
#pragma unroll
    for (int t = 0; t < WOPS; ++t) glds16<true>(wsrc[t] + j * BKW, dst + XB + (uint32_t)((t * 4 + wave) * 1024));
#pragma unroll
    for (int t = 0; t < XOPS; ++t) glds16<false>(xsrc[t] + j * BKW, dst + (uint32_t)((t * 4 + wave) * 1024));
  };

  f32x4 acc[MT][NPW];
#pragma unroll
  for (int mi = 0; mi < MT; ++mi)
#pragma unroll
    for (int j = 0; j < NPW; ++j) acc[mi][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // byte offsets of this lane's fragments inside a stage (k-step 0); the n-tile offsets opaque to
  // hipcc so that it keeps one ds_read_b64 per fragment (see dgemm8_kernel)
  const int aoff = fr * (BKW * 2), boff0 = (wave * NPW * 16 + fr) * BKW + (fq & 1) * 8;
  int ntoff[NPW];
#pragma unroll
  for (int j = 0; j < NPW; ++j) {
    ntoff[j] = j * 16 * BKW;
    asm volatile("" : "+v"(ntoff[j]));
  }
  // one wave per SIMD: nothing else hides the LDS latency, so the fragments of k-step ks + 1 are
  // read (into a second register set) before the MFMAs of k-step ks
  auto mma = [&](int i) {
    const uint8_t* xs = sw + (i % NSR) * SLOT;
    const uint8_t* ws = xs + XB;
    bf16x8 a[2][MT];
    u32x2 bc[2][NPW];
    auto frags = [&](int ks) {
#pragma unroll
      for (int j = 0; j < NPW; ++j) {
        const int c = 2 * ks + (fq >> 1);
        bc[ks & 1][j] = *reinterpret_cast<const u32x2*>(ws + boff0 + ntoff[j] + ((c ^ (fr >> 1)) << 4));
      }
#pragma unroll
      for (int mi = 0; mi < MT; ++mi) {
        const int c = 4 * ks + fq;
        a[ks & 1][mi] = *reinterpret_cast<const bf16x8*>(xs + mi * 16 * BKW * 2 + aoff + ((c ^ fr) << 4));
      }
    };
    frags(0);
#pragma unroll
    for (int ks = 0; ks < BKW / 32; ++ks) {
      if (ks + 1 < BKW / 32) frags(ks + 1);
      __builtin_amdgcn_sched_barrier(0);   // hipcc otherwise sinks each read to just before its MFMA
      bf16x8 b[NPW];
#pragma unroll
      for (int j = 0; j < NPW; ++j) b[j] = widen8(bc[ks & 1][j]);
#pragma unroll
      for (int mi = 0; mi < MT; ++mi)
#pragma unroll
        for (int j = 0; j < NPW; ++j)
          acc[mi][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[ks & 1][mi], b[j], acc[mi][j], 0, 0, 0);
    }
  };

  for (int j = 0; j < NSR - 1; ++j)
    if (j < nkb) stage(j);
  for (int i = 0; i < nkb; ++i) {
    // stages issued after stage i so far: min(NSR - 2, nkb - 1 - i); the tail drains
    if (i + NSR - 2 < nkb) wait_vmcnt<(NSR - 2) * OPS>();
    else wait_vmcnt<0>();
    ring_barrier();
    if (i + NSR - 1 < nkb) stage(i + NSR - 1);
    mma(i);
  }

  // C/D map of 16x16x32: col = lane & 15 (weight row), row = 4 * (lane >> 4) + r (X row)
  if constexpr (EPI == EPI_ARGMAX) {
    // the [MT 16, 128] logit tile through LDS (the ring: every DMA has landed -- the last step
    // waited for vmcnt 0 -- and the barrier says every wave is done reading it), 4 lanes per
    // row -> one (value, id) partial per (row, tile)
    constexpr int TP = NT * 16 + 1;
    static_assert(MT * 16 * TP * 4 <= NSR * SLOT, "logit tile fits the ring");
    __syncthreads();
    float* tl = reinterpret_cast<float*>(sw);
#pragma unroll
    for (int mi = 0; mi < MT; ++mi)
#pragma unroll
      for (int j = 0; j < NPW; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          tl[(mi * 16 + fq * 4 + r) * TP + (wave * NPW + j) * 16 + fr] = acc[mi][j][r] * sc[j];
    __syncthreads();
    const int ntiles = N / (NT * 16);
    for (int rr = tid >> 2; rr < MT * 16; rr += 64) {
      float bv = -FLT_MAX;
      int bi = 0x7fffffff;
      const int c0 = (tid & 3) * (NT * 4);
#pragma unroll 4
      for (int c = c0; c < c0 + NT * 4; ++c) {
        const int col = n0 + c;
        if (col < n_valid) argmax_better(bv, bi, bf2f(f2bf(tl[rr * TP + c])), col);
      }
#pragma unroll
      for (int o = 1; o <= 2; o <<= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        argmax_better(bv, bi, ov, oi);
      }
      if ((tid & 3) == 0 && rr < M) {
        pv[(size_t)rr * ntiles + tile] = bv;
        pi[(size_t)rr * ntiles + tile] = bi;
      }
    }
    return;
  }
  float glu_lo = 0.f;   // EPI_GLU: the smallest gate this lane has seen (silu_times_first)
  auto sweep = [&](auto second) {
#pragma unroll
    for (int mi = 0; mi < MT; ++mi)
#pragma unroll
      for (int j = 0; j < NPW; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = mi * 16 + fq * 4 + r, col = n0 + (wave * NPW + j) * 16 + fr;
          const float v = acc[mi][j][r] * sc[j];
          if constexpr (EPI == EPI_GLU) {
            // SwiGLU pair: gate value at an 8-block's low half, up value 8 columns (lanes) later,
            // both rounded to bf16 first, as the unfused bf16 GEMM output
            const float u = row_swap8(v);
            if (row < M && (fr & 8) == 0) {
              const float gb = bf2f(f2bf(v)), ub = bf2f(f2bf(u));
              Y[(size_t)row * (N >> 1) + ((col >> 4) << 3) + (col & 7)] = f2bf(silu_times_pass(gb, ub, glu_lo, second));
            }
          } else if (row < M) {
            P[((size_t)slice * M + row) * N + col] = v;
          }
        }
  };
  sweep(std::false_type{});
  if constexpr (EPI == EPI_GLU) {
    if (silu_second_pass(glu_lo)) sweep(std::true_type{});   // a gate below -80: silu_times for the wave's pairs
  }
}

constexpr int MR8W_LO = MR8 + 1, MR8W_HI = 128;   // rows of the wide FP8 kernel

bool shape8w_ok(int M, int N, int K, int S) {
  return M >= MR8W_LO && M <= MR8W_HI && N >= NTW8 * 16 && N % (NTW8 * 16) == 0 && S >= 1 && K % S == 0 &&
         (K / S) >= KGW && (K / S) % KGW == 0;
}

template <int EPI>
void launch8w(dim3 grid, hipStream_t s, const void* x, const void* w, const float* sc, uint16_t* y, float* p, int M,
              int N, int K, int Ks, float* pv = nullptr, int* pi = nullptr, int nv = 0) {
  const int S = grid.y;
  const int xr = (xcd_knob() && S > 1 && 8 % S == 0 && (grid.x * S) % 8 == 0) ? 1 : 0;
  const uint16_t* xp = (const uint16_t*)x;
  const uint8_t* wp = (const uint8_t*)w;
  if (M <= 64) dgemm8w_kernel<EPI, 4><<<grid, 256, 0, s>>>(xp, wp, sc, y, p, M, N, K, Ks, xr, pv, pi, nv);
  else dgemm8w_kernel<EPI, 8><<<grid, 256, 0, s>>>(xp, wp, sc, y, p, M, N, K, Ks, xr, pv, pi, nv);
}
}  // namespace

// 33..128-row decode projections over FP8 weights (see dgemm8w_kernel): Wq [N, K] e4m3fn codes,
// scale [N] fp32 powers of two; 128-row weight tiles.  All return -1, launching nothing, for a
// shape without an instantiation: M outside 33..128, N % 128, a K slice that is not whole
// 512-deep turns, pointers off 16 B, n_valid outside 1..N.
// fp32 slabs P [S, M, N]
int docqa_dgemm8w_partial(const void* X, const void* Wq, const float* scale, float* P, int M, int N, int K, int S,
                          int tile_rows, hipStream_t s) {
  if (!X || !Wq || !scale || !P || tile_rows != 128 || !shape8w_ok(M, N, K, S) || !docqa_aligned16(X) ||
      !docqa_aligned16(Wq))
    return -1;
  launch8w<EPI_PARTIAL>(dim3(N / 128, S), s, X, Wq, scale, nullptr, P, M, N, K, K / S);
  DOCQA_CHECK_LAUNCH();
  return 0;
}

// Y [M, N / 2] = silu(gate) * up for the 8-interleaved gate|up codes Wq [N, K] (N = 2 I)
int docqa_dgemm8w_glu(const void* X, const void* Wq, const float* scale, void* Y, int M, int N, int K, hipStream_t s) {
  if (!X || !Wq || !scale || !Y || !shape8w_ok(M, N, K, 1) || !docqa_aligned16(X) || !docqa_aligned16(Wq)) return -1;
  launch8w<EPI_GLU>(dim3(N / 128), s, X, Wq, scale, (uint16_t*)Y, nullptr, M, N, K, K);
  DOCQA_CHECK_LAUNCH();
  return 0;
}

// LM head + greedy pick: out[M] = argmax over the first n_valid columns of bf16(X . W'^T), outv[M]
// the picked value; ws_v / ws_i: [M, N / 128] per-tile partials
int docqa_dgemm8w_argmax(const void* X, const void* Wq, const float* scale, int64_t* out, float* outv, float* ws_v,
                         int* ws_i, int M, int N, int K, int n_valid, hipStream_t s) {
  if (!X || !Wq || !scale || !out || !ws_v || !ws_i || !shape8w_ok(M, N, K, 1) || n_valid <= 0 || n_valid > N ||
      !docqa_aligned16(X) || !docqa_aligned16(Wq))
    return -1;
  launch8w<EPI_ARGMAX>(dim3(N / 128), s, X, Wq, scale, nullptr, nullptr, M, N, K, K, ws_v, ws_i, n_valid);
  argmax_merge_kernel<<<M, 256, 0, s>>>(ws_v, ws_i, N / 128, out, outv);
  DOCQA_CHECK_LAUNCH();
  return 0;
}

// ---------------------------------------------------------------------------------------
// MXFP4 weight stream for decode steps of 2..32 rows: dgemm8_kernel's ring pipeline (256 threads,
// workgroup = NT x 16 weight rows x all M rows x one K slice, X fragments straight to VGPRs two
// stages ahead, counted vmcnt waits, ring_barrier, XCD-aware slice remap,
// v_mfma_f32_16x16x32_bf16) over the (Wq, E) copies of gemv4_kernel: Wq [N, K / 2] bytes of two
// e2m1 codes (element 2j in bits 0..3), E [N, K / 32] e8m0 block scales.
//   * Ring depth: a stage keeps the bf16 / FP8 stage's BYTES -- 256 B per weight row, now 512
//     codes = 16 scale blocks -- in 4 slots, so the NT LDS-DMA wave-instructions (glds16<true>,
//     16 B per lane, nt) per wave per stage, the issue order and the counted waits carry over.
//     K granule: one ring turn = 4 x 512 = 2048 (Ks % 2048 == 0: 4096 is 2 turns, 14336 is 7).
//     The 128-B-per-row stage (granule 1024) was not built.  What the narrow projections lack
//     at this granule is workgroups (O 4096 x 4096: 64 tiles x 2 slices for 256 CUs), and fewer
//     n-tiles per workgroup give them without touching the stage: NT = 2 | 1 (32 | 16 weight
//     rows, a 32 | 16 KB ring, more workgroups per CU) for the slab epilogue -- O at 8 rows 6.7 us
//     at NT = 2, S = 2 against 8.5 at NT = 4 (profiles/mxfp4_dgemm_probe.log).  X is re-read per
//     workgroup, so the wide projections keep NT = 4 | 7.
//   * LDS layout: stage = [NT 16][256 B], 16 chunks of 16 B per row, byte for byte the FP8 stage
//     with the same source swizzle: chunk c of row r lands at chunk position c ^ (r & 15).  A
//     chunk is exactly one scale block (32 codes).
//   * B fragment: the k order inside an MFMA is free as long as A and B agree, so lane (fr =
//     lane & 15, fq = lane >> 4) owns a WHOLE block: block c = 4 g + fq of its wave's 4 G blocks
//     of the stage (G = 1 at MT = 1, 2 at MT = 2), row 16 nt + fr -- one ds_read_b128 at
//       row * 256 + ((c ^ fr) << 4)
//     and one scale byte feed the lane's B operand of four MFMAs (dword t = codes 8 t .. 8 t + 7
//     for MFMA t).  The matching A operands are the 64 contiguous bytes X[row][32 c + 8 t ..]:
//     MFMA t of group g contracts k = 32 (4 g + fq) + 8 t + e over (fq, e), the four of them all
//     128 k of the group.
//     ds_read_b128 is served in four 16-lane groups {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and
//     the same + 32, bank = (addr / 4) % 64 (MI355X_MICROARCH.md, LDS): a group is conflict-free
//     iff its 16 lanes hit 16 distinct 16-B slots of the 256-B bank row.  row * 256 == 0 (mod
//     256), so the slot is c ^ fr.  The first group holds fq = 0 with fr in {0-3, 12-15} and
//     fq = 1 with fr in {4-11}; with c0 the (even) block of fq = 0 its slots are c0 ^ {0-3, 12-15}
//     and (c0 ^ 1) ^ {4-11} = c0 ^ {4-11} (x ^ 1 maps {4-11} onto itself): all 16.  The second
//     group swaps the two fr sets, the upper two have fq = 2 | 3 (x ^ 2 and x ^ 3 map both sets
//     onto themselves): every group is conflict-free.
//   * Widening: v_cvt_scalef32_pk_bf16_fp4 (two codes per instruction, four per 8-code fragment)
//     with the block scale as its fp32 operand E << 23 -- exact (a code times a power of two is
//     a bf16 value), so the fp32 accumulators need no scaling afterwards.  No scaled MFMA: it
//     would need quantized activations, i.e. another model.
//   * Block scales: per-lane global loads into VGPRs, not one more LDS-DMA piece.  A lane needs
//     one byte per n-tile per group; the four fq lanes' bytes are one aligned dword (G = 2: two
//     dwords 4 B apart, one dwordx2), so each lane loads that word (the 4 fq lanes coalesce) and
//     picks byte fq with a shift and a mask.  That is NT loads per stage, issued FIRST in the stage's X
//     set and therefore retired by the wait that retires the stage's X fragments; a DMA piece of
//     NT x 256 B is not a whole number of 1-KB wave-instructions at NT = 7, would be issued by
//     some waves only (unequal vmcnt counts per wave) and costs a ds_read per n-tile.
//   * vmcnt: the per-stage vector-memory set of a lane is XV = NT scale loads + SPW X fragments
//     (SPW = 4 G), issued as one group "X(j)".  Issue order W0 X0 W1 X1 W2 | step i: X(i+2)
//     W(i+3); the ops issued after X(i) are W(i+1) X(i+1) W(i+2), so vmcnt(2 NT + XV) retires
//     X(i) and, issued before it, W(i).  At most 2 NT + XV + NT + XV <= 51 in flight (NT = 7,
//     MT = 2), inside the 6-bit counter.
//   * MT = 1 (2..16 rows: four waves split the stage's 16 blocks, 4 each) and MT = 2 (17..32
//     rows: two k-groups of 8 blocks).  33+ rows stay on W' (dgemm8w_kernel is FP8 only): every wave
//     would widen every fragment and the bf16 kernel is no longer bound by weight bytes alone.
//   * Where the time goes: a stage holds twice the FP8 stage's k, so twice its conversions, MFMAs
//     and X bytes per weight byte.  The kernel is bound by that per-k work, not by HBM: 3.2-4.0
//     TB/s of codes and scales at 2 rows (FP8: 4.4-5.7), and the time grows with the rows (LM
//     head 70 / 84 / 107 / 145 us at 2 / 8 / 16 / 32 rows) as the X fragments stop hitting the
//     same cache lines.  It beats W' by 2.2-2.7 x on the wide projections at 2..8 rows and still
//     by 1.3-1.6 x at 32; against FP8 it wins up to 8 rows and loses from 16.
//   * Epilogues: EPI_PARTIAL / EPI_GLU / EPI_ARGMAX exactly as dgemm8_kernel.
namespace {
constexpr int BK4 = 512;                  // codes per weight row per stage (256 B)
constexpr int BKB4 = BK4 / 2;             // ... bytes

__device__ __forceinline__ void gload_u32(uint32_t& d, const void* p) {
  asm volatile("global_load_dword %0, %1, off" : "=v"(d) : "v"(p) : "memory");
}
__device__ __forceinline__ void gload_u32(u32x2& d, const void* p) {
  asm volatile("global_load_dwordx2 %0, %1, off" : "=v"(d) : "v"(p) : "memory");
}
__device__ __forceinline__ uint32_t word_of(uint32_t v, int) { return v; }
__device__ __forceinline__ uint32_t word_of(u32x2 v, int g) { return v[g]; }

// 8 e2m1 codes (one dword) times the block scale -> the bf16x8 B fragment
__device__ __forceinline__ bf16x8 widen4(uint32_t c, float scale) {
  const bf16x2 a = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(c, scale, 0);
  const bf16x2 b = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(c, scale, 1);
  const bf16x2 d = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(c, scale, 2);
  const bf16x2 e = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(c, scale, 3);
  return bf16x8{a[0], a[1], b[0], b[1], d[0], d[1], e[0], e[1]};
}

template <int EPI, int MT, int NT>
__global__ __launch_bounds__(256) void dgemm4_kernel(const uint16_t* __restrict__ X, const uint8_t* __restrict__ W,
                                                     const uint8_t* __restrict__ E, uint16_t* __restrict__ Y,
                                                     float* __restrict__ P, int M, int N, int K, int Ks,
                                                     int xcd_remap, float* __restrict__ pv = nullptr,
                                                     int* __restrict__ pi = nullptr, int n_valid = 0) {
  static_assert(MT == 1 || MT == 2, "2..16 rows (MT = 1) or 17..32 rows (MT = 2)");
  static_assert(EPI == EPI_PARTIAL || EPI == EPI_GLU || EPI == EPI_ARGMAX, "slabs, SwiGLU or argmax");
  constexpr int NSR = NS;                        // ring slots
  constexpr int KW = 4 / MT;                     // k-groups
  constexpr int G = 4 / KW;                      // 4-block groups per wave per stage
  constexpr int SPW = 4 * G;                     // k-steps (= X fragments) per wave per stage
  constexpr int XV = NT + SPW;                   // scale words + X fragments per stage
  constexpr int VW = 2 * NT + XV;                // vector-memory ops in flight at the top of a step
  constexpr int STAGE = NT * 16 * BKB4;          // bytes of one W stage (NT x 4 KB)
  static_assert(3 * NT + 2 * XV <= 63, "loads in flight per lane must fit the vmcnt counter");
  typedef std::conditional_t<G == 1, uint32_t, u32x2> ST;   // a lane's scale bytes of one stage and n-tile
  __shared__ __attribute__((aligned(16))) uint8_t sw[NSR * STAGE];   // W ring
  int tile = blockIdx.x, slice = blockIdx.y;
  if (xcd_remap) {   // XCD x only runs slice x % S (see dgemm_kernel)
    const int S = gridDim.y;
    const int L = blockIdx.x + blockIdx.y * gridDim.x;
    const int xcd = L & 7, j = L >> 3;
    slice = xcd % S;
    tile = j * (8 / S) + xcd / S;
  }
  const int n0 = tile * NT * 16;
  const int kbeg = slice * Ks;
  const int nkb = Ks / BK4;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fq = lane >> 4;
  const int mt = wave % MT, kg = wave / MT;
  // this lane's 64 X bytes per group: k = 128 (G kg + g) + 32 fq + 8 t of the stage
  const uint16_t* xrow = X + (size_t)min(mt * 16 + fr, M - 1) * K + kbeg + kg * SPW * 32 + fq * 32;
  // ... and its scale word: blocks 4 (G kg + g) .. + 3 of the stage, row 16 nt + fr
  const uint8_t* erow = E + (size_t)(n0 + fr) * (K >> 5) + (kbeg >> 5) + kg * SPW;
  const uint32_t ring = lds_u32(sw);

  f32x4 acc[NT];
#pragma unroll
  for (int i = 0; i < NT; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};

  // W stage j -> ring slot j % NSR: 4 NT wave-instructions of 64 lanes x 16 B (4 rows each), NT
  // per wave, source XOR-swizzled; clamped past the last stage (see dgemm_kernel)
  const uint8_t* wsrc[NT];
#pragma unroll
  for (int i = 0; i < NT; ++i) {
    const int p = (i * 4 + wave) * 64 + lane;
    const int r = p >> 4;
    wsrc[i] = W + (size_t)(n0 + r) * (K >> 1) + (kbeg >> 1) + (((p & 15) ^ (r & 15)) << 4);
  }
  auto stage_w = [&](int j) {
    const int koff = min(j, nkb - 1) * BKB4;
    const uint32_t dst = ring + (uint32_t)((j % NSR) * STAGE);
#pragma unroll
    for (int i = 0; i < NT; ++i) glds16<true>(wsrc[i] + koff, dst + (uint32_t)((i * 4 + wave) * 1024));
  };
  // X(j): the stage's scale words first, then its X fragments
  auto load_x = [&](ST (&sc)[NT], bf16x8 (&x)[SPW], int j) {
    const int jj = min(j, nkb - 1);
    const uint8_t* es = erow + jj * (BK4 / 32);
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) gload_u32(sc[nt], es + (size_t)nt * 16 * (K >> 5));
    const uint16_t* src = xrow + jj * BK4;
    gload16<0>(x[0], src);
    gload16<16>(x[1], src);
    gload16<32>(x[2], src);
    gload16<48>(x[3], src);
    if constexpr (G == 2) {
      gload16<256>(x[4], src);
      gload16<272>(x[5], src);
      gload16<288>(x[6], src);
      gload16<304>(x[7], src);
    }
  };
  auto name_sc = [&](ST (&sc)[NT]) {   // retired by the wait just before: see dgemm8_kernel
#pragma unroll
    for (int i = 0; i < NT; ++i) asm volatile("" : "+v"(sc[i]));
  };
  auto mma = [&](const ST (&sc)[NT], const bf16x8 (&x)[SPW], int j) {
    const uint8_t* src = sw + (j % NSR) * STAGE + fr * BKB4;
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const int c = (kg * G + g) * 4 + fq;
      const int off = (c ^ fr) << 4;
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const u32x4 cw = *reinterpret_cast<const u32x4*>(src + nt * 16 * BKB4 + off);
        // e8m0 byte fq of the word -> fp32 2^(e - 127)
        const float scale = __uint_as_float(((word_of(sc[nt], g) >> (fq * 8)) & 0xffu) << 23);
#pragma unroll
        for (int t = 0; t < 4; ++t)
          acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(x[g * 4 + t], widen4(cw[t], scale), acc[nt], 0, 0, 0);
      }
    }
  };
  bf16x8 x0[SPW], x1[SPW], x2[SPW], x3[SPW];
  ST s0[NT], s1[NT], s2[NT], s3[NT];
#define RING_STEP4(I, SC, XC, SNX, XNX)                                                 \
  wait_vm_n<VW>(XC);                                                                    \
  name_sc(SC);                                                                          \
  ring_barrier();                                                                       \
  load_x(SNX, XNX, (I) + 2);                                                            \
  stage_w((I) + NSR - 1);                                                               \
  mma(SC, XC, I);
  stage_w(0);
  load_x(s0, x0, 0);
  stage_w(1);
  load_x(s1, x1, 1);
  stage_w(2);
  for (int i = 0; i < nkb; i += 4) {
    RING_STEP4(i, s0, x0, s2, x2)
    RING_STEP4(i + 1, s1, x1, s3, x3)
    RING_STEP4(i + 2, s2, x2, s0, x0)
    RING_STEP4(i + 3, s3, x3, s1, x1)
  }
#undef RING_STEP4
  // drain the clamped tail loads; naming every buffer keeps its registers reserved until then
  wait_vm_n<0>(x0);
  keep_live(x1);
  keep_live(x2);
  keep_live(x3);
  name_sc(s0);
  name_sc(s1);
  name_sc(s2);
  name_sc(s3);

  // sum the KW k-groups through LDS (ring is free after the last barrier + wait)
  __syncthreads();
  f32x4* red = reinterpret_cast<f32x4*>(sw);        // [wave][nt][lane] = one slot
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) red[(wave * NT + nt) * 64 + lane] = acc[nt];
  __syncthreads();
  const float* rf = reinterpret_cast<const float*>(sw);
  auto sum_k = [&](int m, int nt, int ln, int r) {
    float v = 0.f;
#pragma unroll
    for (int g = 0; g < KW; ++g) v += rf[(((g * MT + m) * NT + nt) * 64 + ln) * 4 + r];
    return v;
  };
  // C/D map of 16x16x32: col = lane & 15 (weight row), row = 4 * (lane >> 4) + r (X row)
  if constexpr (EPI == EPI_ARGMAX) {
    // the [rows, NT 16] logit tile through LDS (past the k-group reduction area), 4 lanes per
    // row -> one (value, id) partial per (row, tile)
    constexpr int TP = NT * 16 + 1;
    float* tl = reinterpret_cast<float*>(sw) + 4 * NT * 64 * 4;
    for (int idx = tid; idx < MT * NT * 256; idx += 256) {
      const int r = idx & 3, ln = (idx >> 2) & 63, q = idx >> 8;
      const int nt = q % NT, m = q / NT;
      tl[(m * 16 + (ln >> 4) * 4 + r) * TP + nt * 16 + (ln & 15)] = sum_k(m, nt, ln, r);
    }
    __syncthreads();
    const int ntiles = N / (NT * 16);
    for (int rr = tid >> 2; rr < MT * 16; rr += 64) {
      float bv = -FLT_MAX;
      int bi = 0x7fffffff;
      const int c0 = (tid & 3) * (NT * 4);
#pragma unroll 4
      for (int c = c0; c < c0 + NT * 4; ++c) {
        const int col = n0 + c;
        if (col < n_valid) argmax_better(bv, bi, bf2f(f2bf(tl[rr * TP + c])), col);
      }
#pragma unroll
      for (int o = 1; o <= 2; o <<= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        argmax_better(bv, bi, ov, oi);
      }
      if ((tid & 3) == 0 && rr < M) {
        pv[(size_t)rr * ntiles + tile] = bv;
        pi[(size_t)rr * ntiles + tile] = bi;
      }
    }
    return;
  }
  float glu_lo = 0.f;   // EPI_GLU: the smallest gate this lane has seen (silu_times_first)
  auto sweep = [&](auto second) {
#pragma unroll
    for (int e = 0; e < MT * NT; ++e) {
      const int idx = e * 256 + tid;                 // (m-tile, nt, lane, r)
      const int r = idx & 3, ln = (idx >> 2) & 63, q = idx >> 8;
      const int nt = q % NT, m = q / NT;
      const int row = m * 16 + (ln >> 4) * 4 + r, col = n0 + nt * 16 + (ln & 15);
      if (row >= M) continue;
      if constexpr (EPI == EPI_GLU) {
        // SwiGLU pair: gate value at an 8-block's low half, up value 8 columns later, both
        // rounded to bf16 first, as the unfused bf16 GEMM output
        if ((ln & 8) == 0) {
          const float gb = bf2f(f2bf(sum_k(m, nt, ln, r))), ub = bf2f(f2bf(sum_k(m, nt, ln + 8, r)));
          Y[(size_t)row * (N >> 1) + ((col >> 4) << 3) + (col & 7)] = f2bf(silu_times_pass(gb, ub, glu_lo, second));
        }
      } else {
        P[((size_t)slice * M + row) * N + col] = sum_k(m, nt, ln, r);
      }
    }
  };
  sweep(std::false_type{});
  if constexpr (EPI == EPI_GLU) {
    if (silu_second_pass(glu_lo)) sweep(std::true_type{});   // a gate below -80: silu_times for the wave's pairs
  }
}

constexpr int MR4 = 32;   // rows of the MXFP4 ring kernel (MT <= 2)

bool shape4_ok(int M, int N, int K, int S, int bn) {
  return M >= 1 && M <= MR4 && N >= bn && N % bn == 0 && S >= 1 && K % S == 0 && (K / S) >= NS * BK4 &&
         (K / S) % (NS * BK4) == 0;
}

bool ptrs4_ok(const void* X, const void* Wq, const void* E) {
  return X && Wq && E && docqa_aligned16(X) && docqa_aligned16(Wq) && docqa_aligned16(E);
}

template <int EPI, int NT>
void launch4(dim3 grid, hipStream_t s, const void* x, const void* w, const void* e, uint16_t* y, float* p, int M,
             int N, int K, int Ks, float* pv = nullptr, int* pi = nullptr, int nv = 0) {
  const int S = grid.y;
  const int xr = (xcd_knob() && S > 1 && 8 % S == 0 && (grid.x * S) % 8 == 0) ? 1 : 0;
  const uint16_t* xp = (const uint16_t*)x;
  const uint8_t* wp = (const uint8_t*)w;
  const uint8_t* ep = (const uint8_t*)e;
  if (M <= 16) dgemm4_kernel<EPI, 1, NT><<<grid, 256, 0, s>>>(xp, wp, ep, y, p, M, N, K, Ks, xr, pv, pi, nv);
  else dgemm4_kernel<EPI, 2, NT><<<grid, 256, 0, s>>>(xp, wp, ep, y, p, M, N, K, Ks, xr, pv, pi, nv);
}
}  // namespace

// 2..32-row decode projections over MXFP4 weights (see dgemm4_kernel; one row works too, the
// plans send it to the GEMV): Wq [N, K / 2] e2m1 code pairs, E [N, K / 32] e8m0 block scales.
// All return -1, launching nothing, for a shape without an instantiation: more than 32 rows,
// N % tile, a K slice that is not whole 2048-deep ring turns, pointers off 16 B.
// fp32 slabs P [S, M, N]; tile_rows: 64, or 32 | 16 (NT = 2 | 1: the same stage per weight row in
// a ring of 32 | 16 KB) for the narrow projections, whose 64-row tiles times the few slices a
// 2048-deep granule allows leave CUs idle (O 4096 x 4096: 64 x 2 workgroups)
int docqa_dgemm4_partial(const void* X, const void* Wq, const void* E, float* P, int M, int N, int K, int S,
                         int tile_rows, hipStream_t s) {
  if (M == 0) return 0;
  if (!P || (tile_rows != 64 && tile_rows != 32 && tile_rows != 16) || !shape4_ok(M, N, K, S, tile_rows) ||
      !ptrs4_ok(X, Wq, E))
    return -1;
  const dim3 grid(N / tile_rows, S);
  if (tile_rows == 64) launch4<EPI_PARTIAL, 4>(grid, s, X, Wq, E, nullptr, P, M, N, K, K / S);
  else if (tile_rows == 32) launch4<EPI_PARTIAL, 2>(grid, s, X, Wq, E, nullptr, P, M, N, K, K / S);
  else launch4<EPI_PARTIAL, 1>(grid, s, X, Wq, E, nullptr, P, M, N, K, K / S);
  DOCQA_CHECK_LAUNCH();
  return 0;
}

// Y [M, N / 2] = silu(gate) * up for the 8-interleaved gate|up codes (N = 2 I); 112-row tiles
// where they give >= 192 workgroups (as docqa_dgemm_glu), else 64-row tiles
int docqa_dgemm4_glu(const void* X, const void* Wq, const void* E, void* Y, int M, int N, int K, hipStream_t s) {
  if (M == 0) return 0;
  if (!Y || !ptrs4_ok(X, Wq, E)) return -1;
  if (shape4_ok(M, N, K, 1, 112) && N / 112 >= 192)
    launch4<EPI_GLU, 7>(dim3(N / 112), s, X, Wq, E, (uint16_t*)Y, nullptr, M, N, K, K);
  else if (shape4_ok(M, N, K, 1, 64))
    launch4<EPI_GLU, 4>(dim3(N / 64), s, X, Wq, E, (uint16_t*)Y, nullptr, M, N, K, K);
  else
    return -1;
  DOCQA_CHECK_LAUNCH();
  return 0;
}

// LM head + greedy pick: out[M] = argmax over the first n_valid columns of bf16(X . W'^T), outv[M]
// the picked value; ws_v / ws_i: [M, N / 64] per-tile partials
int docqa_dgemm4_argmax(const void* X, const void* Wq, const void* E, int64_t* out, float* outv, float* ws_v,
                        int* ws_i, int M, int N, int K, int n_valid, hipStream_t s) {
  if (M == 0) return 0;
  if (!out || !ws_v || !ws_i || !shape4_ok(M, N, K, 1, 64) || n_valid <= 0 || n_valid > N || !ptrs4_ok(X, Wq, E))
    return -1;
  launch4<EPI_ARGMAX, 4>(dim3(N / 64), s, X, Wq, E, nullptr, nullptr, M, N, K, K, ws_v, ws_i, n_valid);
  argmax_merge_kernel<<<M, 256, 0, s>>>(ws_v, ws_i, N / 64, out, outv);
  DOCQA_CHECK_LAUNCH();
  return 0;
}
