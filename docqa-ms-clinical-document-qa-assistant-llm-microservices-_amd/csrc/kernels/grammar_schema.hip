// grammar_schema.hip -- JSON-schema structured outputs (the Ollama API's format: a schema object)
// on the device.
//
// The automaton is the one ops/json_schema.py compiles: a byte-level DFA with no stack, per
// REQUEST, held in a slot of a table pool.  Rows of one step read different slots.  A slot
// (kSlotBytes bytes, 16-byte aligned) is
//
//     0    int32 n_states, int32 n_classes, 8 bytes of zeros
//     16   cls   uint8 [256]                       byte -> class
//     272  trans uint16 [n_states * n_classes]     entry = next state (bits 0..14) | 0x8000
//
// Entry 0 rejects; a flagged entry is a whitespace byte between tokens and counts against the
// whitespace cap, every other byte resets the run.  State 1 is DONE (nothing but EOS).  The
// host's copy of the walk is ops.json_schema.step and the two must stay the same.
//
//  * schema_mask_kernel    : one workgroup per (row, 4096 tokens), grammar_mask_kernel's shape.
//                            Rows with word 0 / valid 0 leave at once, a DONE row masks
//                            everything but EOS without a table.  Otherwise the workgroup copies
//                            the slot's 256-byte cls into LDS, computes the row's 256-bit "first
//                            byte accepted" set (thread b walks byte b) and walks each token's
//                            bytes from the row's state, 16 tokens a thread: cls from LDS, trans
//                            through L2 -- a table is shared by every workgroup of the step, and
//                            staging tables of <= 60 KiB in LDS instead measured 1.5x to 2.3x
//                            slower at 32 and 256 rows (profiles/format_schema_bench.log: the
//                            copy per workgroup and two workgroups per CU cost more than the
//                            lookups save), so there is one path.  A token that is not allowed
//                            gets -inf in its logit; nothing else is written and no logit is
//                            read.
//  * schema_advance_kernel : one thread per row walks the picked token and stores the new word.
//
// Every index is checked against the slot's header and the header against the slot's size, so a
// word or a pool that the host did not write cannot send a load out of the pool: such a row
// allows nothing.
//
// Per-row state word (int64, 0: the row has no schema): bits 0..15 DFA state, 16..20 whitespace
// run, 21..28 pool slot.
#include "docqa_common.h"
#include <stdint.h>
#include <string.h>

namespace {

constexpr int kWsCap = 16;                 // ops.grammar.WS_CAP
constexpr int kDone = 1;                   // ops.json_schema.DONE
constexpr int kMaxStates = 8192;           // ops.json_schema.MAX_STATES
constexpr int kMaxClasses = 256;           // ops.json_schema.MAX_CLASSES
constexpr int kMaxCells = 1 << 18;         // ops.json_schema.MAX_CELLS
constexpr int kClsOff = 16, kTransOff = 272;
constexpr long kSlotBytes = kTransOff + 2L * kMaxCells;      // ops.json_schema.SLOT_BYTES
constexpr int kTokPerThread = 16;
constexpr int kChunk = 256 * kTokPerThread;

struct Slot {
  const uint8_t* cls;
  const uint16_t* trans;
  int ns, nc;      // 0, 0: no table
};

__device__ __forceinline__ Slot s_slot(const uint8_t* pool, int n_slots, int slot) {
  Slot t{nullptr, nullptr, 0, 0};
  if (slot < 0 || slot >= n_slots) return t;
  const uint8_t* base = pool + (size_t)slot * (size_t)kSlotBytes;
  const int ns = reinterpret_cast<const int*>(base)[0], nc = reinterpret_cast<const int*>(base)[1];
  if (ns < 2 || ns > kMaxStates || nc < 1 || nc > kMaxClasses || ns * nc > kMaxCells) return t;
  t.cls = base + kClsOff;
  t.trans = reinterpret_cast<const uint16_t*>(base + kTransOff);
  t.ns = ns;
  t.nc = nc;
  return t;
}

// one byte of class c from state st (< ns): false: rejected
__device__ __forceinline__ bool s_step(int& st, int& ws, const uint16_t* trans, int ns, int nc, unsigned c) {
  if ((int)c >= nc) return false;
  const unsigned e = trans[st * nc + (int)c];
  const int nxt = (int)(e & 0x7fffu);
  if (e == 0 || nxt >= ns) return false;
  if (e & 0x8000u) {
    if (ws >= kWsCap) return false;
    ws += 1;
  } else {
    ws = 0;
  }
  st = nxt;
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
__global__ __launch_bounds__(256) void schema_mask_kernel(
    T* __restrict__ logits, int n_valid, long ld, const int64_t* __restrict__ sstate,
    const int* __restrict__ valid, const int* __restrict__ tok_off, int n_tok,
    const uint8_t* __restrict__ tok_bytes, int total, const uint8_t* __restrict__ pool, int n_slots,
    int eos_id) {
  __shared__ uint8_t cls[256];
  __shared__ unsigned first[8];
  const int row = blockIdx.y, tid = threadIdx.x;
  if (valid != nullptr && valid[row] == 0) return;     // row-uniform: the whole workgroup leaves
  const int64_t word = sstate[row];
  if (word == 0) return;
  const int st0 = (int)(word & 0xffff), ws0 = (int)(word >> 16) & 0x1f;
  const int lo = blockIdx.x * kChunk, hi = min(n_valid, lo + kChunk);
  T* out = logits + (size_t)row * (size_t)ld;
  const Slot sl = s_slot(pool, n_slots, (int)(word >> 21) & 0xff);
  if (st0 == kDone || st0 >= sl.ns) {
    // DONE: EOS alone (a state or a slot that does not exist allows nothing)
    for (int t = lo + tid; t < hi; t += 256)
      if (!(t == eos_id && st0 == kDone)) out[t] = neg_inf<T>();
    return;
  }
  const int ns = sl.ns, nc = sl.nc;
  cls[tid] = sl.cls[tid];
  const uint16_t* __restrict__ trans = sl.trans;
  __syncthreads();
  {
    int st = st0, ws = ws0;
    const bool ok = s_step(st, ws, trans, ns, nc, cls[tid]);
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
          int st = st0, ws = ws0;
          allowed = true;
          for (int i = 0; i < n8 && allowed; ++i)
            allowed = s_step(st, ws, trans, ns, nc, cls[(unsigned)((w >> (8 * i)) & 0xff)]);
          for (int p = a + 8; p < b && allowed; ++p) allowed = s_step(st, ws, trans, ns, nc, cls[tok_bytes[p]]);
        }
      }
    }
    if (!allowed) out[t] = neg_inf<T>();
  }
}

__global__ __launch_bounds__(256) void schema_advance_kernel(
    int64_t* __restrict__ sstate, const int64_t* __restrict__ nxt, const int* __restrict__ valid,
    const int* __restrict__ tok_off, int n_tok, const uint8_t* __restrict__ tok_bytes, int total,
    const uint8_t* __restrict__ pool, int n_slots, int eos_id, int rows) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= rows) return;
  if (valid != nullptr && valid[r] == 0) return;
  const int64_t word = sstate[r];
  if (word == 0) return;
  int st = (int)(word & 0xffff), ws = (int)(word >> 16) & 0x1f;
  if (st == kDone) return;
  const int64_t t = nxt[r];
  if (t == eos_id || t < 0 || t >= n_tok) return;
  const int a = tok_off[t], b = tok_off[t + 1];
  if (a < 0 || b <= a || b > total) return;
  const Slot sl = s_slot(pool, n_slots, (int)(word >> 21) & 0xff);
  if (st >= sl.ns) return;
  for (int p = a; p < b; ++p)
    if (!s_step(st, ws, sl.trans, sl.ns, sl.nc, sl.cls[tok_bytes[p]])) return;     // rejected: the word stays
  sstate[r] = (word & ~(int64_t)0x1fffff) | (int64_t)st | (int64_t)ws << 16;
}

}  // namespace

long docqa_schema_slot_bytes() { return kSlotBytes; }

// logits [rows, ld] bf16 / fp32; sstate int64 [rows]; valid int32 [rows] or null; tok_off int32
// [n_tok + 1] into tok_bytes [total]; pool uint8 [n_slots, kSlotBytes], 16-byte aligned
int docqa_schema_mask(void* logits, int rows, int n_valid, long ld, int is_bf16, const int64_t* sstate,
                      const int* valid, const int* tok_off, int n_tok, const uint8_t* tok_bytes, int total,
                      const uint8_t* pool, int n_slots, int eos_id, hipStream_t s) {
  if (rows == 0 || n_valid <= 0) return 0;
  if (rows > 65535 || n_slots < 1 || n_slots > 256 || n_tok < 0 || !docqa_aligned16(pool)) return -1;
  dim3 grid((n_valid + kChunk - 1) / kChunk, rows);
  if (is_bf16)
    schema_mask_kernel<uint16_t><<<grid, 256, 0, s>>>(static_cast<uint16_t*>(logits), n_valid, ld, sstate, valid,
                                                      tok_off, n_tok, tok_bytes, total, pool, n_slots, eos_id);
  else
    schema_mask_kernel<uint32_t><<<grid, 256, 0, s>>>(static_cast<uint32_t*>(logits), n_valid, ld, sstate, valid,
                                                      tok_off, n_tok, tok_bytes, total, pool, n_slots, eos_id);
  DOCQA_CHECK_LAUNCH();
  return 0;
}

int docqa_schema_advance(int64_t* sstate, const int64_t* nxt, int rows, const int* valid, const int* tok_off,
                         int n_tok, const uint8_t* tok_bytes, int total, const uint8_t* pool, int n_slots,
                         int eos_id, hipStream_t s) {
  if (rows == 0) return 0;
  if (n_slots < 1 || n_slots > 256 || n_tok < 0 || !docqa_aligned16(pool)) return -1;
  schema_advance_kernel<<<(rows + 255) / 256, 256, 0, s>>>(sstate, nxt, valid, tok_off, n_tok, tok_bytes, total,
                                                           pool, n_slots, eos_id, rows);
  DOCQA_CHECK_LAUNCH();
  return 0;
}
