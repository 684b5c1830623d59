// docqa_kernels.h -- host launchers of the gfx950 kernels (raw pointers + stream).
// Every launcher returns 0 on success, a negative value for an unsupported shape and a
// hipError_t for a failed launch.  They allocate nothing and never synchronise, so they
// can be captured into HIP graphs (cdna_hip_programming.md Guideline 9).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

int docqa_rmsnorm(const void* x, const void* w, void* out, int rows, int H, float eps,
                  hipStream_t s);
int docqa_add_rmsnorm(const void* x, void* residual, const void* w, void* out, int rows, int H,
                      float eps, hipStream_t s);
int docqa_layernorm(const void* x, const void* residual, const void* g, const void* b, void* out,
                    int rows, int H, float eps, hipStream_t s);

int docqa_kv_copy_rows(const uint64_t* caches, int ntensors, const int* tab, int n, int nblocks, int Hkv, int BS,
                       int D, hipStream_t s);
int docqa_rope_cache(void* qkv, const int* positions, const float* cos_sin,
                     const int* slot_mapping, void* k_cache, void* v_cache, int T, int Hq,
                     int Hkv, int D, int row_stride, int BS, hipStream_t s);

// FP8 (OCP e4m3, no scales) paged KV cache: the *8 entry points take caches of 1-byte codes
// in the same [num_blocks, Hkv, BS, D] layout (csrc/kernels/rope_cache.hip, attn_prefill.hip,
// attn_decode.hip)
int docqa_kv_copy_rows8(const uint64_t* caches, int ntensors, const int* tab, int n, int nblocks, int Hkv, int BS,
                        int D, hipStream_t s);
int docqa_rope_cache8(void* qkv, const int* positions, const float* cos_sin, const int* slot_mapping,
                      void* k_cache, void* v_cache, int T, int Hq, int Hkv, int D, int row_stride, int BS,
                      hipStream_t s);
int docqa_rope_cache_splitk8(const void* P, int slab16, int S, void* qkv_out, const int* positions,
                             const float* cos_sin, const int* slot_mapping, void* k_cache, void* v_cache, int T,
                             int Hq, int Hkv, int D, int row_stride, int BS, hipStream_t s);
int docqa_flash_prefill_paged8(const void* qkv, int row_stride, const int* cu_seqlens, void* out,
                               int o_stride, int B, int max_len, int Hq, int Hkv, int head_dim,
                               float scale, const void* k_cache, const void* v_cache,
                               const int* block_tables, int maxb, const int* ctx_start, int BS,
                               hipStream_t s);
int docqa_paged_decode8(const void* q, int q_stride, const void* k_cache, const void* v_cache,
                        const int* block_tables, int maxb, const int* context_lens, void* out,
                        int out_stride, float* tmp_out, float* tmp_ml, int B, int Hq, int Hkv,
                        int D, int BS, int max_parts, float scale, hipStream_t s);
int docqa_paged_decode_group_wave8(const void* q, int q_stride, const void* k_cache, const void* v_cache,
                                   const int* block_tables, int maxb, const int* context_lens, void* out,
                                   int out_stride, int B, int Hq, int Hkv, int BS, float scale, const int* items,
                                   const int* merges, int cap, float* ws_acc, float* ws_ml, hipStream_t s,
                                   int* tick);

int docqa_silu_mul(const void* gu, void* out, int T, int I, int interleaved, hipStream_t s);
int docqa_silu_mul_splitk16(const void* P, void* out, int S, int T, int I, hipStream_t s);
int docqa_silu_mul_splitk(const float* P, void* out, int S, int T, int I, hipStream_t s);
int docqa_bias_act(const void* x, const void* bias, const void* res, void* out, int T, int N,
                   int gelu, hipStream_t s);

int docqa_embedding(const int* ids, const void* table, void* out, int T, int H, int V, hipStream_t s);
int docqa_decode_slots(const int* block_tables, int maxb, const int* positions, const int* valid,
                       int* slots, int B, int BS, hipStream_t s);
int docqa_decode_advance(const int64_t* nxt, int64_t* out, int* tokens, int* positions,
                         int* context_lens, const int* valid, int B, hipStream_t s);
int docqa_bert_embed_ln(const int* ids, const int* pos, const int* tt, const void* wte,
                        const void* wpe, const void* wtt, const void* g, const void* b, void* out,
                        int T, int H, int V, int NP, int NT, float eps, hipStream_t s);
int docqa_argmax(const void* logits, int rows, int V, int ld, int is_bf16, float* ws_v, int* ws_i,
                 int splits, int64_t* out, hipStream_t s);
int docqa_token_cls_argmax(const void* h, int ldh, const void* w, const void* bias, int n_rows,
                           int n_valid, int T, int H, int64_t* out, hipStream_t s);
int docqa_sample(const float* logits, int rows, int V, int ld, const float* inv_temp,
                 const int* top_k, const float* top_p, const float* u, int64_t* out,
                 hipStream_t s);
// sample.hip: Philox4x32-10 uniforms of (seed, index), and the one-read sampler over bf16 /
// fp32 logits (columns < n_valid).  Exactly one of u / (seed, index); min_p, valid may be null.
int docqa_seeded_uniform(const int64_t* seed, const int* index, float* out, int n, hipStream_t s);
int docqa_sample_tokens(const void* logits, int rows, int n_valid, int ld, int is_bf16, const float* inv_temp,
                        const int* top_k, const float* top_p, const float* min_p, const float* u,
                        const int64_t* seed, const int* index, const int* valid, int64_t* out, hipStream_t s);

// repeat / presence / frequency penalties over a per-row token ring hist [rows, W] (W must be
// docqa_penalty_window()), hist_n [rows] tokens appended so far; valid may be null (all rows)
int docqa_penalty_window();
int docqa_apply_penalties(float* logits, int rows, int V, int ld, const int* hist, int W,
                          const int* hist_n, const int* last_n, const float* rep, const float* pres,
                          const float* freq, const int* valid, hipStream_t s);
// argmax over t < n_valid of the penalised logits; CLOBBERS the window tokens' logits
int docqa_penalized_argmax(void* logits, int rows, int V, int ld, int n_valid, int is_bf16,
                           const int* hist, int W, const int* hist_n, const int* last_n,
                           const float* rep, const float* pres, const float* freq, const int* valid,
                           float* ws_v, int* ws_i, int splits, float* pen_v, int* pen_i,
                           int64_t* out, hipStream_t s);
int docqa_decode_advance_hist(const int64_t* nxt, int64_t* out, int* tokens, int* positions,
                              int* context_lens, const int* valid, int* hist, int W, int* hist_n,
                              int B, hipStream_t s);

// per-token log-probabilities (logprobs.hip): lp[r] = logit[r, chosen[r]] - logsumexp(logit[r, :n_valid])
// and the top_n[r] (<= docqa_top_logprobs_max()) most likely tokens; top_n[r] < 0 skips the row.
// Workspaces: pm / ps >= rows * splits, ptv / pti >= rows * splits * docqa_top_logprobs_max(),
// splits = docqa_token_logprobs_splits(rows, n_valid, nullptr) (0: vocabulary too large)
int docqa_top_logprobs_max();
int docqa_token_logprobs_splits(int rows, int V, int* chunk_out);
int docqa_token_logprobs(const void* logits, int rows, int n_valid, int ld, int is_bf16, const int64_t* chosen,
                         const int* top_n, float* pm, float* ps, float* ptv, int* pti, float* lp, int* top_ids,
                         float* top_lp, hipStream_t s);

// grammar-constrained decoding (grammar.hip): per-row automaton state words (0: unconstrained),
// the vocabulary's bytes as tok_off int32 [n_tok + 1] into tok_bytes [total] and the lexer table
// int16 [n_states <= docqa_grammar_max_states(), 256].  mask: -inf into the logits of tokens a
// row's state does not allow (columns < n_valid; EOS only in DONE); advance: the state after the
// picked token.  valid may be null (all rows).
int docqa_grammar_max_states();
int docqa_grammar_mask(void* logits, int rows, int n_valid, long ld, int is_bf16, const int64_t* state,
                       const int* valid, const int* tok_off, int n_tok, const uint8_t* tok_bytes, int total,
                       const void* table, int n_states, int eos_id, hipStream_t s);
int docqa_grammar_advance(int64_t* state, const int64_t* nxt, int rows, const int* valid, const int* tok_off,
                          int n_tok, const uint8_t* tok_bytes, int total, const void* table, int n_states,
                          int eos_id, hipStream_t s);

// JSON-schema structured outputs (grammar_schema.hip): per-row state words (0: no schema; DFA
// state, whitespace run, pool slot) and the table pool uint8 [n_slots, docqa_schema_slot_bytes()],
// one compiled automaton (ops/json_schema.py) per slot.  mask / advance: the contracts of the
// grammar pair, each row walking the tables of its own slot.
long docqa_schema_slot_bytes();
int docqa_schema_mask(void* logits, int rows, int n_valid, long ld, int is_bf16, const int64_t* sstate,
                      const int* valid, const int* tok_off, int n_tok, const uint8_t* tok_bytes, int total,
                      const uint8_t* pool, int n_slots, int eos_id, hipStream_t s);
int docqa_schema_advance(int64_t* sstate, const int64_t* nxt, int rows, const int* valid, const int* tok_off,
                         int n_tok, const uint8_t* tok_bytes, int total, const uint8_t* pool, int n_slots,
                         int eos_id, hipStream_t s);

int docqa_paged_decode(const void* q, int q_stride, const void* k_cache, const void* v_cache,
                       const int* block_tables, int maxb, const int* context_lens, void* out,
                       int out_stride, float* tmp_out, float* tmp_ml, int B, int Hq, int Hkv,
                       int D, int BS, int max_parts, float scale, const int* order, hipStream_t s);
int docqa_decode_splits(int B, int Hkv, int max_context);
int docqa_paged_decode_cascade(const void* q, int q_stride, void* k_cache, void* v_cache,
                               const int* block_tables, int maxb, const int* context_lens, void* out,
                               int out_stride, float* tmp_out, float* tmp_ml, int B, int Hq, int Hkv,
                               int BS, int max_parts, float scale, const int* prefix_table,
                               const int* plen, int nchunk, float* pacc, float* pml, const int* order,
                               hipStream_t s);
int docqa_paged_decode_cascade_grouped(const void* q, int q_stride, void* k_cache, void* v_cache,
                                       const int* block_tables, int maxb, const int* context_lens,
                                       void* out, int out_stride, int B, int Hq, int Hkv, int BS,
                                       float scale, const int* prefix_table, const int* plen, int nchunk,
                                       float* pacc, float* pml, const int* groups, int ngroups,
                                       hipStream_t s);
int docqa_paged_decode_cascade_split(const void* q, int q_stride, void* k_cache, void* v_cache,
                                     const int* block_tables, int maxb, const int* context_lens,
                                     void* out, int out_stride, int B, int Hq, int Hkv, int BS,
                                     float scale, const int* prefix_table, const int* plen, int nchunk,
                                     float* pacc, float* pml, const int* items, const int* merges, int cap,
                                     float* ws_acc, float* ws_ml, int defer,
                                     hipStream_t s, int* tick = nullptr, int inline_prefix = 0,
                                     const float* fP = nullptr, int fS = 0, const int* positions = nullptr,
                                     const float* cos_sin = nullptr, const int* slot_mapping = nullptr);
int docqa_paged_decode_cascade_persist(const void* q, int q_stride, void* k_cache, void* v_cache,
                                       const int* block_tables, int maxb, const int* context_lens,
                                       void* out, int out_stride, int B, int Hq, int Hkv, int BS,
                                       float scale, const int* prefix_table, const int* plen, int nchunk,
                                       float* pacc, float* pml, const int* items, const int* merges,
                                       const int* bins, int cap, float* ws_acc, float* ws_ml, hipStream_t s);
int docqa_group_persist_bins(int cap, int Hkv);
int docqa_set_decode_trace(long long* buf);
int docqa_set_group_wave(int on);   // -1: query only; returns the previous setting
int docqa_paged_decode_cascade_rope(void* qkv, int q_stride, const int* positions,
                                    const float* cos_sin, const int* slot_mapping, void* k_cache,
                                    void* v_cache, const int* block_tables, int maxb,
                                    const int* context_lens, void* out, int out_stride,
                                    float* tmp_out, float* tmp_ml, int B, int Hq, int Hkv, int BS,
                                    int max_parts, float scale, const int* prefix_table,
                                    const int* plen, int nchunk, float* pacc, float* pml,
                                    const int* order, hipStream_t s);

int docqa_flash_prefill(const void* qkv, int row_stride, const int* cu_seqlens, void* out,
                        int o_stride, int B, int max_len, int Hq, int Hkv, int head_dim,
                        float scale, int causal, hipStream_t s);

int docqa_flash_prefill_paged(const void* qkv, int row_stride, const int* cu_seqlens, void* out,
                              int o_stride, int B, int max_len, int Hq, int Hkv, int head_dim,
                              float scale, const void* k_cache, const void* v_cache,
                              const int* block_tables, int maxb, const int* ctx_start, int BS,
                              hipStream_t s);

int docqa_dgemm_partial(const void* X, const void* W, float* P, int M, int N, int K, int S,
                        int tile_rows, hipStream_t s);
int docqa_add_rmsnorm_splitk(const float* P, int S, void* residual, const void* w, void* out,
                             int rows, int H, float eps, hipStream_t s);
int docqa_rope_cache_splitk(const float* P, int S, void* qkv_out, const int* positions,
                            const float* cos_sin, const int* slot_mapping, void* k_cache,
                            void* v_cache, int T, int Hq, int Hkv, int D, int row_stride, int BS,
                            hipStream_t s);
int docqa_add_rmsnorm_splitk16(const void* P, int S, void* residual, const void* w, void* out,
                               int rows, int H, float eps, hipStream_t s);
int docqa_rope_cache_splitk16(const void* P, int S, void* qkv_out, const int* positions,
                              const float* cos_sin, const int* slot_mapping, void* k_cache,
                              void* v_cache, int T, int Hq, int Hkv, int D, int row_stride, int BS,
                              hipStream_t s);
size_t docqa_ar_region_bytes(size_t max_elems);
int docqa_ar_alloc(size_t bytes, void** ptr);
int docqa_ar_free(void* ptr);
int docqa_ar_ipc_handle(void* ptr, void* handle_out);
int docqa_ar_ipc_open(const void* handle, void** ptr);
int docqa_ar_ipc_close(void* ptr);
int docqa_ar_run(const void* in, int S, void* out, void* residual, const void* w, float eps, int M, int H,
                 int rank, int nranks, void* const* regions, size_t max_elems, int mode, unsigned* ctr,
                 unsigned* err, long long timeout_us, hipStream_t s);
int docqa_paged_decode_fused(const float* P, int S, const int* positions, const float* cos_sin,
                             const int* slot_mapping, void* k_cache, void* v_cache,
                             const int* block_tables, int maxb, const int* context_lens, void* out,
                             int out_stride, float* tmp_out, float* tmp_ml, int B, int Hq, int Hkv,
                             int BS, int max_parts, float scale, const int* order, hipStream_t s,
                             int* tick = nullptr);
int docqa_dgemm_splits(int N, int K);
int docqa_dgemm_glu(const void* X, const void* W, void* Y, int M, int N, int K, hipStream_t s);
int docqa_dgemm_add_rmsnorm(const void* X, const void* W, float* P, int M, int N, int K, int S, void* residual,
                            const void* gamma, void* out, float eps, int* tick, hipStream_t s);
int docqa_dgemm_partial_xn(const float* Pin, int Sin, const void* res_in, void* res_out, const void* gamma,
                           float eps, const void* W, float* P, int N, int K, int S, hipStream_t s);
int docqa_dgemm_glu_xn(const float* Pin, int Sin, const void* res_in, void* res_out, const void* gamma, float eps,
                       const void* W, void* Y, int N, int K, hipStream_t s);
// batch-1 GEMV (dgemm.hip gemv_kernel): epi 0 fp32 slabs P [S, 1, N], epi 1 SwiGLU Y [1, N / 2];
// Pin != null: the input row from the previous projection's slabs (XNormIn)
int docqa_gemv(const void* X, const void* W, void* Y, float* P, int N, int K, int S, int R, int epi,
               const float* Pin, int Sin, const void* res_in, void* res_out, const void* gamma, float eps,
               hipStream_t s);
// batch-1 GEMV over FP8 weights (dgemm.hip gemv8_kernel): Wq [N, K] OCP e4m3fn codes, scale [N]
// fp32 powers of two; R rows per workgroup, LB codes per lane per load (8 | 16); otherwise as
// docqa_gemv / docqa_gemv_argmax.  -1 (nothing launched) for a shape without an instantiation.
int docqa_gemv8(const void* X, const void* Wq, const float* scale, void* Y, float* P, int N, int K, int S, int R,
                int LB, int epi, const float* Pin, int Sin, const void* res_in, void* res_out, const void* gamma,
                float eps, hipStream_t s);
int docqa_gemv8_argmax(const void* X, const void* Wq, const float* scale, int64_t* out, float* outv, float* ws_v,
                       int* ws_i, int N, int K, int R, int LB, int n_valid, hipStream_t s);
// batch-1 GEMV over MXFP4 weights (dgemm.hip gemv4_kernel): Wq [N, K / 2] bytes of two OCP e2m1
// codes (element 2j in bits 0..3), E [N, K / 32] e8m0 block scales; R rows per workgroup, LB codes
// per lane per load (16 | 32), KW waves along K (1 | 2 | 4); otherwise as docqa_gemv8 /
// docqa_gemv8_argmax.  -1 (nothing launched) for a shape without an instantiation.
int docqa_gemv4(const void* X, const void* Wq, const void* E, void* Y, float* P, int N, int K, int S, int R, int LB,
                int KW, int epi, const float* Pin, int Sin, const void* res_in, void* res_out, const void* gamma,
                float eps, hipStream_t s);
int docqa_gemv4_argmax(const void* X, const void* Wq, const void* E, int64_t* out, float* outv, float* ws_v,
                       int* ws_i, int N, int K, int R, int LB, int KW, int n_valid, hipStream_t s);
// 2..32-row decode projections over FP8 weights (dgemm.hip dgemm8_kernel: the LDS-DMA ring over
// the codes, K slices of whole 1024-deep ring turns): fp32 slabs P [S, M, N] (tile_rows 64),
// SwiGLU Y [M, N / 2], LM head + greedy pick (ws_v / ws_i: [M, N / 64]).  -1 (nothing launched)
// for a shape without an instantiation.
int docqa_dgemm8_partial(const void* X, const void* Wq, const float* scale, float* P, int M, int N, int K, int S,
                         int tile_rows, hipStream_t s);
int docqa_dgemm8_glu(const void* X, const void* Wq, const float* scale, void* Y, int M, int N, int K, hipStream_t s);
int docqa_dgemm8_argmax(const void* X, const void* Wq, const float* scale, int64_t* out, float* outv, float* ws_v,
                        int* ws_i, int M, int N, int K, int n_valid, hipStream_t s);
// 33..128-row decode projections over FP8 weights (dgemm.hip dgemm8w_kernel: waves own n-tiles of a
// 128-row weight tile, X staged through LDS; K slices of whole 512-deep turns): outputs as
// docqa_dgemm8_* (tile_rows 128; ws_v / ws_i: [M, N / 128]).  -1 (nothing launched) for M outside
// 33..128, N % 128, a K slice that is not whole turns, pointers off 16 B, n_valid outside 1..N.
int docqa_dgemm8w_partial(const void* X, const void* Wq, const float* scale, float* P, int M, int N, int K, int S,
                          int tile_rows, hipStream_t s);
int docqa_dgemm8w_glu(const void* X, const void* Wq, const float* scale, void* Y, int M, int N, int K, hipStream_t s);
int docqa_dgemm8w_argmax(const void* X, const void* Wq, const float* scale, int64_t* out, float* outv, float* ws_v,
                         int* ws_i, int M, int N, int K, int n_valid, hipStream_t s);
// 2..32-row decode projections over MXFP4 weights (dgemm.hip dgemm4_kernel: the same ring over
// Wq [N, K / 2] e2m1 code pairs and E [N, K / 32] e8m0 block scales, K slices of whole 2048-deep
// ring turns): outputs as docqa_dgemm8_*; slab tiles of 64, 32 or 16 weight rows (tile_rows).  -1
// (nothing launched) for a shape without an instantiation.
int docqa_dgemm4_partial(const void* X, const void* Wq, const void* E, float* P, int M, int N, int K, int S,
                         int tile_rows, hipStream_t s);
int docqa_dgemm4_glu(const void* X, const void* Wq, const void* E, void* Y, int M, int N, int K, hipStream_t s);
int docqa_dgemm4_argmax(const void* X, const void* Wq, const void* E, int64_t* out, float* outv, float* ws_v,
                        int* ws_i, int M, int N, int K, int n_valid, hipStream_t s);
int docqa_embed_rmsnorm(const int* ids, const void* table, const void* w, void* h, void* x, int T, int H, int V,
                        float eps, hipStream_t s);
int docqa_fp32_gemm_nt(const float* x, int nq, int d, const float* w, int n, float* out, hipStream_t s);
int docqa_gemv_argmax(const void* X, const void* W, int64_t* out, float* outv, float* ws_v, int* ws_i, int N, int K,
                      int n_valid, hipStream_t s);
int docqa_dgemm_argmax(const void* X, const void* W, int64_t* out, float* outv, float* ws_v, int* ws_i, int M,
                       int N, int K, int n_valid, hipStream_t s);
int docqa_dgemm(const void* X, const void* W, void* Y, float* partial, int M, int N, int K, int S,
                hipStream_t s);
int docqa_gemm(const void* A, const void* W, const void* bias, const void* res, void* C, int M,
               int N, int K, int epi, hipStream_t s);
int docqa_mgemm(const void* X, const void* W, void* Y, float* P, int M, int N, int K, int S, int cfg,
                hipStream_t s);
int docqa_mgemm_slab16(const void* X, const void* W, void* Y, int M, int N, int K, int S, int cfg,
                       hipStream_t s);
int docqa_mgemm_glu(const void* X, const void* W, void* Y, int M, int N, int K, int cfg, hipStream_t s);
int docqa_mgemm_argmax(const void* X, const void* W, int64_t* out, float* outv, float* ws_v, int* ws_i, int M,
                       int N, int K, int n_valid, int cfg, hipStream_t s);
int docqa_mgemm_tile_n(int cfg);
int docqa_mgemm_ld(const void* X, int ldx, const void* W, int ldw, void* Y, float* P, int M, int N, int K, int S,
                   int cfg, int glu, hipStream_t s);
// IVF coarse quantizer for wide probes (coarse.hip): nprobe <= 512 nearest centroids per query
int docqa_coarse_probes(const float* cent, const float* cnorm, int nlist, int d, const float* xq, int nq,
                        int nprobe, float* ws, int64_t* probes, hipStream_t s);
bool docqa_pgemm_ok(int M, int N, int K);
int docqa_pgemm(const void* A, const void* W, void* C, float* P, int M, int N, int K, int S, int epi,
                hipStream_t s);
int docqa_knn_workspace_blocks(int N);
int docqa_knn_kpad(int k);
int docqa_knn(const void* xb, const float* norms, int N, int d, int is_bf16, const float* xq,
              int nq, int k, int metric_ip, float* ws_d, int* ws_i, int nblk, float* out_d,
              int64_t* out_i, int64_t id_offset, hipStream_t s);
// scoped exact search: tags / days int32 [N], scope int32 [nq, 4] = (tag, alt_tag, day_lo,
// day_hi); workspace and outputs as docqa_knn
int docqa_knn_scoped(const void* xb, const float* norms, const int* tags, const int* days, int N,
                     int d, int is_bf16, const float* xq, const int* scope, int nq, int k,
                     int metric_ip, float* ws_d, int* ws_i, int nblk, float* out_d, int64_t* out_i,
                     int64_t id_offset, hipStream_t s);
// BM25 scan over CSR term columns + fused top-k (lexical.hip); ws_d / ws_i [nq,
// docqa_bm25_workspace_blocks(N), docqa_knn_kpad(k)]; tags / days / scope null: unscoped
int docqa_bm25_workspace_blocks(int N);
int docqa_bm25_topk(const int64_t* row_ptr, const int* terms, const uint8_t* tfs, const int* dl, int N,
                    const int* qterms, const float* qweights, int nq, int k, float k1, float b,
                    float one_minus_b, float avgdl, const int* tags, const int* days, const int* scope,
                    float* ws_d, int* ws_i, int nblk, float* out_s, int64_t* out_i, int64_t id_offset,
                    hipStream_t s);
// per query: first k of either ranked id list (mode 0 / 1) or their reciprocal rank fusion (2)
int docqa_rank_fuse(const int64_t* i_dense, int ld, const int64_t* i_lex, int ll, const int* mode, int nq,
                    int k, int c, float* out_f, int64_t* out_i, hipStream_t s);
// maximal marginal relevance re-selection (mmr.hip): per query k picks out of cand [nq, F <= 64]
// (the first ncand[q] entries, ids in [0, N)) by lam * cos(q, c) - (1 - lam) * max cos(c, picked);
// lam < 0: the first k entries pass through.  out_s / out_i / out_p [nq, k]
int docqa_mmr_select(const void* xb, const float* norms, int64_t N, int d, int is_bf16, const float* xq,
                     const int64_t* cand, int F, const int* ncand, const float* lam, int nq, int k,
                     float* out_s, int64_t* out_i, int* out_p, hipStream_t s);

// row compaction for deletes (compact.hip): exact and deterministic, int64 index arithmetic, no
// workgroup waits on another.  masked scan: pos int64 [n+1] = exclusive prefix sum of
// keep[r] ? w[r] : 0 (w null: 1), ws = docqa_masked_scan_workspace(n) int64 words; -1 above
// docqa_compact_scan_tile()^docqa_compact_scan_levels() rows
int docqa_compact_scan_tile();
int docqa_compact_scan_levels();
int64_t docqa_masked_scan_workspace(int64_t n);
int docqa_masked_scan(const uint8_t* keep, const int64_t* w, int64_t n, int64_t* pos, int64_t* ws,
                      hipStream_t s);
// dst[pos[r]] = src[r] for kept rows of W bytes (16-byte, 4-byte or byte lanes by alignment); dst
// holds dst_rows rows and never aliases src; positions outside dst are not written
int docqa_gather_rows(const void* src, void* dst, const uint8_t* keep, const int64_t* pos, int64_t n,
                      int64_t W, int64_t dst_rows, hipStream_t s);
// CSR rows: pos the row scan, epos the scan weighted by row length; new_ptr [ptr_rows], the
// entries of kept rows (terms and / or tfs, either may be null) copied in order into e_cap slots
int docqa_csr_gather(const int64_t* row_ptr, const uint8_t* keep, const int64_t* pos, const int64_t* epos,
                     int64_t n, const int* terms, const uint8_t* tfs, int64_t e_in, int64_t* new_ptr,
                     int64_t ptr_rows, int* new_terms, uint8_t* new_tfs, int64_t e_cap, hipStream_t s);
// out[j] = pos[ids[j]] (ids outside [0, n): -1)
int docqa_remap_ids(const int64_t* ids, int64_t m, const int64_t* pos, int64_t n, int64_t* out, hipStream_t s);

int docqa_ivfpq_search(const float* xq, const float* centroids, const float* pq,
                       const uint8_t* codes, const int64_t* ids, const int64_t* list_off,
                       const int64_t* probes, int nq, int nprobe, int d, int M, int k,
                       float* ws_d, int* ws_i, float* out_d, int64_t* out_i, hipStream_t s);
// precomputed-table scan: norms [N] = ||c_list + r^||^2; lut_ws >= nq*M*256 halves, base_ws >=
// nq*nprobe floats, ws_d / ws_i >= nq*ceil(nprobe/pc)*kpad (kpad = k rounded up to 8/16/32/64)
int docqa_ivfpq_search_pt(const float* xq, const float* centroids, const float* pq, const uint8_t* codes,
                          const float* norms, const int64_t* ids, const int64_t* list_off, const int64_t* probes,
                          int nq, int nprobe, int d, int M, int k, int pc, void* lut_ws, float* base_ws,
                          float* ws_d, int* ws_i, float* out_d, int64_t* out_i, hipStream_t s);
// exact re-rank of <= 64 candidate ids per query against stored vectors (fp32 or bf16 rows)
int docqa_refine_flat(const void* xb, int xb_bf16, int64_t ntotal, const float* xq, const int64_t* cand, int nq,
                      int kc, int d, int k, int ip, float* out_d, int64_t* out_i, hipStream_t s);
int docqa_pq_encode(const float* x, const float* centroids, const int64_t* assign, const float* pq,
                    int n, int d, int M, uint8_t* codes, hipStream_t s);

int docqa_pool_l2(const void* h, const int* cu, int B, int H, int mean, int normalize, float* out,
                  hipStream_t s);
