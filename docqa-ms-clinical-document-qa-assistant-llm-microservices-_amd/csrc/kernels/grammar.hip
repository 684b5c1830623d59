// grammar.hip -- grammar-constrained decoding (the Ollama API's format: "json") on the device.
//
// The automaton is the one of ops/grammar.py: a lexer table  state x byte -> next | op << 8
// (int16 [n_states, 256], built on the host and handed in) and a pushdown stack of one bit per
// nesting level.  Only the op semantics below are written twice; the host's copy is
// ops.grammar.step and the two must stay the same, line for line.
//
//  * grammar_mask_kernel    : one workgroup per (row, 4096 tokens).  A constrained row's
//                             workgroups stage the table in LDS (<= 32 KiB), compute the row's
//                             256-bit "first byte accepted" set (thread b walks byte b) and then
//                             walk each token's bytes from the row's state, 16 tokens a thread;
//                             most tokens die on the set.  A token that is not allowed gets -inf
//                             in its logit; nothing else is written and no logit is read.
//                             Rows with state 0 / valid 0 leave at once, and a DONE row needs no
//                             table: everything but EOS is masked.
//  * grammar_advance_kernel : one thread per row walks the picked token from the table in
//                             global memory and stores the new state.
//
// Per-row state word (int64, 0: row not constrained): bits 0..7 lexer state, 8..12 whitespace
// run, 13..18 depth, 19..50 stack (bit 19 + level: 1 array, 0 object).
#include "docqa_common.h"
#include <stdint.h>
#include <string.h>

namespace {

constexpr int kMaxStates = 64;       // ops.grammar.MAX_STATES: rows of the LDS table
constexpr int kWsCap = 16;           // ops.grammar.WS_CAP
constexpr int kDepthCap = 32;        // ops.grammar.DEPTH_CAP
constexpr int kTokPerThread = 16;
constexpr int kChunk = 256 * kTokPerThread;
// lexer states the ops name (ops.grammar)
constexpr int kDone = 1, kAfterValue = 2, kExpectKey = 3, kExpectValue = 4;
enum : int { OP_NONE, OP_WS, OP_PUSH_OBJ, OP_PUSH_ARR, OP_POP_OBJ, OP_POP_ARR, OP_COMMA, OP_REJECT };

struct GState {
  int lex, ws, depth;
  unsigned stack;
};

__device__ __forceinline__ GState g_unpack(int64_t w) {
  GState s;
  s.lex = (int)(w & 0xff);
  s.ws = (int)(w >> 8) & 0x1f;
  s.depth = (int)(w >> 13) & 0x3f;
  s.stack = (unsigned)(w >> 19);
  return s;
}

__device__ __forceinline__ int64_t g_pack(const GState& s) {
  return (int64_t)s.lex | (int64_t)s.ws << 8 | (int64_t)s.depth << 13 | (int64_t)s.stack << 19;
}

// one byte: `e` is the table entry of (s.lex, byte).  False: rejected (s is then undefined).
__device__ __forceinline__ bool g_step(GState& s, unsigned e) {
  const int nxt = e & 0xff, op = (e >> 8) & 0xff;
  if (op == OP_REJECT) return false;
  if (op == OP_WS) {
    if (s.ws >= kWsCap) return false;
    s.ws += 1;
    s.lex = nxt;
    return true;
  }
  s.ws = 0;
  if (op == OP_PUSH_OBJ || op == OP_PUSH_ARR) {
    if (s.depth >= kDepthCap) return false;
    if (op == OP_PUSH_ARR) s.stack |= 1u << s.depth;
    s.depth += 1;
    s.lex = nxt;
    return true;
  }
  if (op == OP_POP_OBJ || op == OP_POP_ARR) {
    if (s.depth == 0 || ((s.stack >> (s.depth - 1)) & 1u) != (op == OP_POP_ARR ? 1u : 0u)) return false;
    s.depth -= 1;
    s.stack &= ~(1u << s.depth);
    s.lex = s.depth == 0 ? kDone : kAfterValue;
    return true;
  }
  if (op == OP_COMMA) {
    if (s.depth == 0) return false;
    s.lex = ((s.stack >> (s.depth - 1)) & 1u) ? kExpectValue : kExpectKey;
    return true;
  }
  s.lex = nxt;
  return true;
}

template <typename T>
__device__ __forceinline__ T neg_inf();
template <>
__device__ __forceinline__ uint16_t neg_inf<uint16_t>() { return 0xff80u; }        // bf16 -inf
template <>
__device__ __forceinline__ uint32_t neg_inf<uint32_t>() { return 0xff800000u; }    // fp32 -inf

// T: the logits' storage word (uint16_t bf16, uint32_t fp32)
template <typename T>
__global__ __launch_bounds__(256) void grammar_mask_kernel(
    T* __restrict__ logits, int n_valid, long ld, const int64_t* __restrict__ state,
    const int* __restrict__ valid, const int* __restrict__ tok_off, int n_tok,
    const uint8_t* __restrict__ tok_bytes, int total, const uint16_t* __restrict__ table, int n_states,
    int eos_id) {
  __shared__ __attribute__((aligned(16))) uint16_t tab[kMaxStates * 256];
  __shared__ unsigned first[8];
  const int row = blockIdx.y, tid = threadIdx.x;
  if (valid != nullptr && valid[row] == 0) return;     // row-uniform: the whole workgroup leaves
  const int64_t word = state[row];
  if (word == 0) return;
  const GState s0 = g_unpack(word);
  const int lo = blockIdx.x * kChunk, hi = min(n_valid, lo + kChunk);
  T* out = logits + (size_t)row * (size_t)ld;
  if (s0.lex == kDone || s0.lex >= n_states) {
    // DONE: EOS alone (a lexer state the table does not have allows nothing)
    for (int t = lo + tid; t < hi; t += 256)
      if (!(t == eos_id && s0.lex == kDone)) out[t] = neg_inf<T>();
    return;
  }
  {
    const uint4* src = reinterpret_cast<const uint4*>(table);
    uint4* dst = reinterpret_cast<uint4*>(tab);
    for (int i = tid; i < n_states * 32; i += 256) dst[i] = src[i];     // 512 B per table row
  }
  __syncthreads();
  {
    GState s = s0;
    const bool ok = g_step(s, tab[s0.lex * 256 + tid]);
    const unsigned long long m = __ballot(ok);
    if ((tid & 63) == 0) {
      first[(tid >> 6) * 2] = (unsigned)m;
      first[(tid >> 6) * 2 + 1] = (unsigned)(m >> 32);
    }
  }
  __syncthreads();
  for (int t = lo + tid; t < hi; t += 256) {
    bool allowed = false;
    if (t != eos_id && t < n_tok) {
      const int a = tok_off[t], b = tok_off[t + 1];
      if (a >= 0 && b > a && b <= total) {
        // the token's first 8 bytes in one load where the buffer has them
        unsigned long long w = 0;
        const int n8 = min(b - a, 8);
        if (a + 8 <= total) {
          memcpy(&w, tok_bytes + a, 8);
        } else {
          for (int i = 0; i < n8; ++i) w |= (unsigned long long)tok_bytes[a + i] << (8 * i);
        }
        const unsigned b0 = (unsigned)(w & 0xff);
        if ((first[b0 >> 5] >> (b0 & 31)) & 1u) {
          GState s = s0;
          allowed = true;
          for (int i = 0; i < n8 && allowed; ++i)
            allowed = g_step(s, tab[(s.lex & (kMaxStates - 1)) * 256 + (unsigned)((w >> (8 * i)) & 0xff)]);
          for (int p = a + 8; p < b && allowed; ++p)
            allowed = g_step(s, tab[(s.lex & (kMaxStates - 1)) * 256 + tok_bytes[p]]);
        }
      }
    }
    if (!allowed) out[t] = neg_inf<T>();
  }
}

__global__ __launch_bounds__(256) void grammar_advance_kernel(
    int64_t* __restrict__ state, const int64_t* __restrict__ nxt, const int* __restrict__ valid,
    const int* __restrict__ tok_off, int n_tok, const uint8_t* __restrict__ tok_bytes, int total,
    const uint16_t* __restrict__ table, int n_states, int eos_id, int rows) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= rows) return;
  if (valid != nullptr && valid[r] == 0) return;
  const int64_t word = state[r];
  if (word == 0) return;
  GState s = g_unpack(word);
  if (s.lex == kDone || s.lex >= n_states) return;
  const int64_t t = nxt[r];
  if (t == eos_id || t < 0 || t >= n_tok) return;
  const int a = tok_off[t], b = tok_off[t + 1];
  if (a < 0 || b <= a || b > total) return;
  for (int p = a; p < b; ++p) {
    if (s.lex >= n_states) return;
    if (!g_step(s, table[s.lex * 256 + tok_bytes[p]])) return;     // rejected: the state stays
  }
  state[r] = g_pack(s);
}

}  // namespace

int docqa_grammar_max_states() { return kMaxStates; }

// logits [rows, ld] bf16 / fp32; state int64 [rows]; valid int32 [rows] or null; tok_off int32
// [n_tok + 1] into tok_bytes [total]; table int16 [n_states, 256], 16-byte aligned
int docqa_grammar_mask(void* logits, int rows, int n_valid, long ld, int is_bf16, const int64_t* state,
                       const int* valid, const int* tok_off, int n_tok, const uint8_t* tok_bytes, int total,
                       const void* table, int n_states, int eos_id, hipStream_t s) {
  if (rows == 0 || n_valid <= 0) return 0;
  if (rows > 65535 || n_states < 1 || n_states > kMaxStates || n_tok < 0 || !docqa_aligned16(table)) return -1;
  dim3 grid((n_valid + kChunk - 1) / kChunk, rows);
  const uint16_t* tab = static_cast<const uint16_t*>(table);
  if (is_bf16)
    grammar_mask_kernel<uint16_t><<<grid, 256, 0, s>>>(static_cast<uint16_t*>(logits), n_valid, ld, state, valid,
                                                       tok_off, n_tok, tok_bytes, total, tab, n_states, eos_id);
  else
    grammar_mask_kernel<uint32_t><<<grid, 256, 0, s>>>(static_cast<uint32_t*>(logits), n_valid, ld, state, valid,
                                                       tok_off, n_tok, tok_bytes, total, tab, n_states, eos_id);
  DOCQA_CHECK_LAUNCH();
  return 0;
}

int docqa_grammar_advance(int64_t* state, const int64_t* nxt, int rows, const int* valid, const int* tok_off,
                          int n_tok, const uint8_t* tok_bytes, int total, const void* table, int n_states,
                          int eos_id, hipStream_t s) {
  if (rows == 0) return 0;
  if (n_states < 1 || n_states > kMaxStates || n_tok < 0) return -1;
  grammar_advance_kernel<<<(rows + 255) / 256, 256, 0, s>>>(state, nxt, valid, tok_off, n_tok, tok_bytes, total,
                                                            static_cast<const uint16_t*>(table), n_states, eos_id,
                                                            rows);
  DOCQA_CHECK_LAUNCH();
  return 0;
}
