"""Llama-3 decoder (8B / 70B / test sizes) for the llm-qa generator.

MI355X-first layout:
  * fused projections: one [(Hq + 2*Hkv)*D, H] QKV GEMM and one [2I, H] gate|up GEMM
    per layer, all on the hand-written MFMA GEMMs (prefill: pgemm.hip 256 x 256 with SwiGLU
    in the gate|up epilogue; decode: dgemm.hip <= 192 rows, mgemm.hip 193..512 rows, split-K
    fp32 slabs consumed by the fused RoPE + KV-cache write and residual + RMSNorm kernels;
    the LM head with the greedy argmax fused in at every bucket);
  * the residual stream is updated inside the fused add+RMSNorm kernel, so each layer
    costs 2 GEMM-epilogue-free passes over the hidden state instead of 4;
  * attention reads Q/K/V straight out of the packed QKV buffer (prefill: MFMA flash
    kernel; decode: paged split-K GQA kernel over a [blocks, Hkv, BS, D] cache);
  * tensor parallelism is Megatron-style: column-parallel QKV / gate|up, row-parallel
    O / down followed by one all-reduce each (RCCL over xGMI), vocab-parallel LM head
    whose argmax is resolved with a [B, 2] all-gather instead of gathering logits;
  * with 288 GB of HBM per GPU the 8B model (16 GB bf16) is replicated per GPU (TP=1,
    request-level data parallel) and 70B (140 GB) runs TP=8 (17.6 GB/GPU).

Weights are random-initialised on the device (no checkpoints are reachable offline);
``models/checkpoint.py`` loads Hugging Face Llama checkpoints (safetensors) when one is
available: pass the checkpoint directory wherever a preset name is accepted.

Reference parity: replaces the Ollama/llama.cpp Mistral-7B generator behind
``ChatOllama(model="mistral", temperature=0)`` (llm-qa/main.py:66-69).
"""
from __future__ import annotations

import math
import os
import zlib
from dataclasses import dataclass, field
from typing import NamedTuple

import torch
import torch.nn.functional as F

from .. import ops
from ..parallel import comm

# cascade decode over a library-GEMM QKV: DOCQA_CASCADE_ROPE=1 fuses RoPE + the new
# token's cache write into the cascade kernels (ops.paged_decode_cascade_rope).  Off by
# default: measured 2.5 % slower per decode step at batch 256 than the separate rope_cache
# launch (the ring's fused preamble delays its K/V stream; profiles/r1_cascade_rope_ab.log)
_CASCADE_ROPE = os.environ.get("DOCQA_CASCADE_ROPE", "0") == "1"
# last prefill layer on the logits rows only (forward(): trim)
_PREFILL_TRIM = os.environ.get("DOCQA_PREFILL_TRIM", "1") != "0"
# grouped decode reading the QKV slabs itself (ops.paged_decode_grouped_fused): off -- every
# group workgroup's slab loads + new-token write ahead of its first K/V stage cost more than the
# rope_cache_splitk launch saved (decode 1148-1151 vs 1120-1122 ms per batch same-box,
# profiles/r4_group_fused_ab.log)
_GROUP_FUSED = os.environ.get("DOCQA_GROUP_FUSED", "0") == "1"
# short prefills (<= ops.MID_M_MAX tokens) on the decode projection plans (forward())
_PREFILL_MID = os.environ.get("DOCQA_PREFILL_MID", "1") != "0"


@dataclass
class LlamaConfig:
    name: str = "llama3-8b"
    vocab_size: int = 128256
    hidden: int = 4096
    intermediate: int = 14336
    layers: int = 32
    heads: int = 32
    kv_heads: int = 8
    head_dim: int = 128
    rope_theta: float = 500000.0
    rms_eps: float = 1e-5
    max_position: int = 8192
    bos_token_id: int = 128000
    eos_token_id: int = 128009
    # Hugging Face rope_scaling dict (None, "linear" or "llama3"; ops.reference.rope_inv_freq)
    rope_scaling: dict | None = None
    # Mistral-style sliding-window attention span (None = full causal attention); the
    # engine refuses a context longer than the window since its kernels attend to all of it
    sliding_window: int | None = None

    @staticmethod
    def preset(name: str) -> "LlamaConfig":
        if name in ("llama3-8b", "llama-3-8b", "8b"):
            return LlamaConfig()
        if name in ("llama3-70b", "llama-3-70b", "70b"):
            return LlamaConfig(name="llama3-70b", hidden=8192, intermediate=28672, layers=80,
                               heads=64, kv_heads=8)
        if name in ("mistral-7b", "mistral"):
            # the reference's own generator: ChatOllama(model="mistral") (llm-qa/main.py:69)
            # pulls Mistral-7B-Instruct v0.3 -- the Llama block with a 32768-token vocabulary,
            # rope theta 1e6 and full causal attention (v0.1's 4096-token sliding window is
            # gone); HF checkpoints of either version load through models/checkpoint.py
            return LlamaConfig(name="mistral-7b", vocab_size=32768, rope_theta=1e6, max_position=32768,
                               bos_token_id=1, eos_token_id=2)
        if name == "llama3-1b-test":  # mid-size config for kernel/engine tests on GPU
            return LlamaConfig(name=name, vocab_size=32000, hidden=2048, intermediate=8192,
                               layers=4, heads=16, kv_heads=4, max_position=4096,
                               bos_token_id=1, eos_token_id=2)
        if name == "test-tp8":
            # Llama-3-70B's GQA shape (8 KV heads, 128-d heads) at toy width: every TP degree
            # 1 / 2 / 4 / 8 shards it, so the TP=8 paths run in CPU and one-GPU tests; a vocab
            # that is not a multiple of 8 x 256 exercises the padded last LM-head shard
            return LlamaConfig(name=name, vocab_size=4000, hidden=1024, intermediate=2048,
                               layers=2, heads=32, kv_heads=8, head_dim=128, max_position=2048,
                               bos_token_id=1, eos_token_id=2)
        if name == "tiny":
            return LlamaConfig(name="tiny", vocab_size=4096, hidden=256, intermediate=512,
                               layers=2, heads=4, kv_heads=2, head_dim=128, max_position=2048,
                               bos_token_id=1, eos_token_id=2)
        if name == "tiny-8k":   # tiny with Llama-3's 8192-token window (long-prompt service tests)
            return LlamaConfig(name="tiny-8k", vocab_size=4096, hidden=256, intermediate=512,
                               layers=2, heads=4, kv_heads=2, head_dim=128, max_position=8192,
                               bos_token_id=1, eos_token_id=2)
        raise ValueError(f"unknown llama preset {name}")

    def num_params(self) -> int:
        H, I, D = self.hidden, self.intermediate, self.head_dim
        per_layer = H * (self.heads + 2 * self.kv_heads) * D + self.heads * D * H + 3 * H * I + 2 * H
        return self.layers * per_layer + 2 * self.vocab_size * H + H


@dataclass
class AttnMeta:
    """Per-forward attention metadata (all int32 device tensors)."""
    prefill: bool
    positions: torch.Tensor                 # [T]
    slot_mapping: torch.Tensor              # [T]
    cu_seqlens: torch.Tensor | None = None  # [B+1] (prefill)
    max_len: int = 0                        # (prefill)
    block_tables: torch.Tensor | None = None  # [B, maxb] (decode)
    context_lens: torch.Tensor | None = None  # [B] (decode; includes the new token)
    max_context: int = 0                    # (decode) graph-capture bound
    prefix_lens: torch.Tensor | None = None  # [B] (prefill with prefix-cache hits)
    # (decode, cascade) prompt prefix shared by every row: its block ids [maxb] and its
    # length [1] (multiple of the block size), attended once for the whole batch
    shared_table: torch.Tensor | None = None
    shared_len: torch.Tensor | None = None
    cascade_chunks: int = 8
    # (decode) workgroup dispatch order: int32 permutation of the rows, longest context
    # first (LPT), so short sequences fill the last launch round; None: row order
    seq_order: torch.Tensor | None = None
    # (decode, cascade) rows packed in groups of <= 4 sharing prefix-cache blocks
    # (ops.paged_decode_cascade_grouped); None: per-row suffix attention
    decode_groups: torch.Tensor | None = None
    # decode_groups is a deferred split plan (ops.split_decode_groups(defer=True))
    decode_defer: bool = False
    # ... a split plan whose items start at block 0 (the groups attend the shared prefix)
    decode_inline: bool = False


class Streamed(NamedTuple):
    """A model's streamed weight copy: the format (a key of ops.STREAMED), per layer
    {projection: pair} and the LM head's pair -- (q, s) for FP8, (q, e) for MXFP4."""
    fmt: str
    layers: list
    lm_head: tuple


@dataclass
class StepPlan:
    """Which kernel every projection of one forward runs (LlamaModel._step_plan): plain data.  The
    families "streamed_gemv" / "streamed_ring" / "streamed_wide" read the streamed pair
    (ops.streamed_plan's kinds);
    "gemv", "mgemm", "dgemm", "pgemm" (ops.<family>_partial) and "linear32" the bf16 weights."""
    # "qkv" | "o" | "down" -> (family, split-K count, rows | tile | cfg, bf16 slabs); absent or
    # split-K count 0: the library GEMM with the plain consumer
    proj: dict = field(default_factory=dict)
    glu: tuple = ("prefill_glu",)       # gate|up: ("streamed_" + kind,) | (bf16 ops wrapper, *arguments)
    streamed: dict = field(default_factory=dict)    # projections on the streamed pair -> kind
    nf: dict = field(default_factory=dict)          # "o" | "down" -> splits, add + RMSNorm in-kernel
    xn: bool = False                                # gate|up and QKV build their input row in-kernel

    def splits(self, k: str) -> int:
        return self.proj[k][1] if k in self.proj else 0


class LlamaModel:
    def __init__(self, cfg: LlamaConfig, device="cuda", dtype=torch.bfloat16, seed: int = 0,
                 init: bool = True):
        self.cfg = cfg
        self.device = torch.device(device)
        self.dtype = dtype
        ps = comm.state()
        self.tp = ps.tp_size
        self.tp_rank = ps.tp_rank
        if cfg.heads % self.tp or cfg.kv_heads % self.tp or cfg.intermediate % self.tp:
            raise ValueError("heads / kv_heads / intermediate must divide the TP size")
        self.hq = cfg.heads // self.tp
        self.hkv = cfg.kv_heads // self.tp
        self.inter = cfg.intermediate // self.tp
        self.vocab_shard = (cfg.vocab_size + self.tp - 1) // self.tp
        if self.tp > 1:
            # whole 256-row tiles for the fused LM-head argmax kernel (mgemm.hip); the padded
            # rows (ids >= vocab_size, on the last rank only) are zero and never picked
            self.vocab_shard = (self.vocab_shard + 255) // 256 * 256
        self.vocab_start = self.tp_rank * self.vocab_shard
        # ids this rank's LM-head shard holds
        self.vocab_valid = max(0, min(cfg.vocab_size - self.vocab_start, self.vocab_shard))
        self.scale = 1.0 / math.sqrt(cfg.head_dim)
        self.cos_sin = ops.rope_cos_sin(cfg.max_position, cfg.head_dim, cfg.rope_theta, self.device,
                                        scaling=cfg.rope_scaling)
        self.layers: list[dict] = []
        self._tick = None      # decode attention's last-arriver merge tickets (ops.decode_ticket)
        self._ntick = None     # fused projection + add + RMSNorm ticket word (ops.dgemm_add_rmsnorm)
        # the streamed weight copy (quantize_fp8 / quantize_mxfp4): a model holds one format at most
        self.streamed: Streamed | None = None
        if init:
            self._random_init(seed)

    # ------------------------------------------------------------------ weights
    def _random_init(self, seed: int) -> None:
        """Random weights (no checkpoints offline) that are TP-INVARIANT: every weight is
        generated in fixed global blocks (per head for q / k / v / o, per 64 rows or columns
        of the MLP, per 256 vocab rows of the LM head), each from its own seeded stream, so
        a rank's shard holds exactly the bits the TP = 1 model has at those positions -- TP
        runs and services are then token-exact against TP = 1 by construction."""
        cfg, dev, dt = self.cfg, self.device, self.dtype
        g = torch.Generator(device=dev)
        std = 0.02
        out_std = std / math.sqrt(2 * cfg.layers)
        H, D, r = cfg.hidden, cfg.head_dim, self.tp_rank

        def gen(key, shape, s=std):
            g.manual_seed((seed * 1_000_003 + zlib.crc32(repr(key).encode())) & 0x7FFFFFFFFFFF)
            t = torch.empty(*shape, device=dev, dtype=dt)
            t.normal_(0.0, s, generator=g)
            return t

        def rows(key, lo, hi, width, blk, s=std):       # global rows [lo, hi) in blocks
            return torch.cat([gen(key + (b,), (blk, width), s) for b in range(lo // blk, hi // blk)])

        ib = 64 if self.inter % 64 == 0 else 8            # MLP block (divides every TP shard)
        self.embed = gen(("embed",), (cfg.vocab_size, H))
        self.final_norm = torch.ones(H, device=dev, dtype=dt)
        # vocab block: the same for every TP degree (shards start at multiples of 256)
        vb = next(b for b in (256, 8, 1) if cfg.vocab_size % b == 0)
        self.lm_head = rows(("lm",), self.vocab_start, self.vocab_start + self.vocab_shard, H, vb)
        if self.vocab_valid < self.vocab_shard:
            self.lm_head[self.vocab_valid:] = 0
        i0, i1 = r * self.inter, (r + 1) * self.inter
        for li in range(cfg.layers):
            q = rows((li, "q"), r * self.hq * D, (r + 1) * self.hq * D, H, D)
            k = rows((li, "k"), r * self.hkv * D, (r + 1) * self.hkv * D, H, D)
            v = rows((li, "v"), r * self.hkv * D, (r + 1) * self.hkv * D, H, D)
            o = rows((li, "o"), r * self.hq * D, (r + 1) * self.hq * D, H, D, out_std).t()   # columns
            gt = rows((li, "gate"), i0, i1, H, ib)
            up = rows((li, "up"), i0, i1, H, ib)
            dn = rows((li, "down"), i0, i1, H, ib, out_std).t()
            self.layers.append({
                "in_norm": torch.ones(H, device=dev, dtype=dt),
                "qkv": torch.cat([q, k, v]).contiguous(),
                "o": o.contiguous(),
                "post_norm": torch.ones(H, device=dev, dtype=dt),
                # rows interleaved in blocks of 8 (gate, up): the decode GEMMs' fused SwiGLU
                "gate_up": ops.glu_interleave(gt, up).contiguous(),
                "down": dn.contiguous(),
            })

    def load_state_dict_hf(self, sd: dict) -> None:
        """Map a Hugging Face LlamaForCausalLM state dict (full, un-sharded) onto this
        rank's shards."""
        cfg, D, r, tp = self.cfg, self.cfg.head_dim, self.tp_rank, self.tp
        dev, dt = self.device, self.dtype

        def get(k):
            return sd[k].to(device=dev, dtype=dt)

        self.embed = get("model.embed_tokens.weight")
        self.final_norm = get("model.norm.weight")
        lm = get("lm_head.weight") if "lm_head.weight" in sd else self.embed
        pad = self.vocab_shard * tp - lm.shape[0]
        if pad:
            lm = torch.cat([lm, lm.new_zeros(pad, lm.shape[1])])
        self.lm_head = lm[r * self.vocab_shard:(r + 1) * self.vocab_shard].contiguous()
        self.layers = []
        for i in range(cfg.layers):
            p = f"model.layers.{i}."
            q = get(p + "self_attn.q_proj.weight").view(cfg.heads, D, -1)[r * self.hq:(r + 1) * self.hq]
            k = get(p + "self_attn.k_proj.weight").view(cfg.kv_heads, D, -1)[r * self.hkv:(r + 1) * self.hkv]
            v = get(p + "self_attn.v_proj.weight").view(cfg.kv_heads, D, -1)[r * self.hkv:(r + 1) * self.hkv]
            o = get(p + "self_attn.o_proj.weight")[:, r * self.hq * D:(r + 1) * self.hq * D]
            gt = get(p + "mlp.gate_proj.weight")[r * self.inter:(r + 1) * self.inter]
            up = get(p + "mlp.up_proj.weight")[r * self.inter:(r + 1) * self.inter]
            dn = get(p + "mlp.down_proj.weight")[:, r * self.inter:(r + 1) * self.inter]
            self.layers.append({
                "in_norm": get(p + "input_layernorm.weight"),
                "qkv": torch.cat([q.reshape(-1, cfg.hidden), k.reshape(-1, cfg.hidden),
                                  v.reshape(-1, cfg.hidden)]).contiguous(),
                "o": o.contiguous(),
                "post_norm": get(p + "post_attention_layernorm.weight"),
                # rows interleaved in blocks of 8 (gate, up): the decode GEMM's fused SwiGLU
                # epilogue pairs them inside one MFMA tile (csrc/kernels/dgemm.hip)
                "gate_up": ops.glu_interleave(gt, up).contiguous(),
                "down": dn.contiguous(),
            })

    def export_state_dict_hf(self) -> dict:
        """Inverse of :meth:`load_state_dict_hf` for an un-sharded (TP=1) model."""
        if self.tp != 1:
            raise ValueError("export requires TP=1")
        cfg, D = self.cfg, self.cfg.head_dim
        sd = {"model.embed_tokens.weight": self.embed, "model.norm.weight": self.final_norm,
              "lm_head.weight": self.lm_head[: cfg.vocab_size]}
        for i, L in enumerate(self.layers):
            p = f"model.layers.{i}."
            q, k, v = L["qkv"].split([self.hq * D, self.hkv * D, self.hkv * D])
            g, u = ops.glu_split(L["gate_up"])
            sd.update({p + "self_attn.q_proj.weight": q, p + "self_attn.k_proj.weight": k,
                       p + "self_attn.v_proj.weight": v, p + "self_attn.o_proj.weight": L["o"],
                       p + "mlp.gate_proj.weight": g, p + "mlp.up_proj.weight": u,
                       p + "mlp.down_proj.weight": L["down"],
                       p + "input_layernorm.weight": L["in_norm"],
                       p + "post_attention_layernorm.weight": L["post_norm"]})
        return {k: t.detach().cpu() for k, t in sd.items()}

    STREAMED_WEIGHTS = ("qkv", "o", "gate_up", "down")
    FP8_WEIGHTS = STREAMED_WEIGHTS      # the name the weight tests read

    def quantize_fp8(self) -> None:
        """FP8 weight streaming for decode steps of 1..ops.DGEMM8W_MAX_ROWS rows (TP = 1; one row:
        the GEMV, 2..32 rows: the ring kernel, 33..128 rows: the wide kernel whose waves own
        n-tiles, each where its plan lists the shape): every
        projection and the LM head get a per-row e4m3fn copy (q, s) with power-of-two scales
        (ops.quantize_fp8_rows), and the resident weights are REPLACED by its exact image
        W' = q * s.  Every kernel that reads W' (prefill, batched decode, mixed steps, sampled
        logits, the CPU reference) then computes the same model the FP8 kernels stream from half
        the bytes, so a request sees one model whatever batch it lands in.  Embedding and
        norms stay as they are.  The copies cost memory (about +50 % of the projections)
        and save none.  Call after random init or load_state_dict_hf, before any decode graph
        is captured."""
        self._quantize("fp8-e4m3", "FP8 weights need tp_size == 1: per-row scales of the row-parallel O / down "
                       "shards would depend on the shard's K range and break the TP-invariant weights")

    def quantize_mxfp4(self) -> None:
        """MXFP4 weight streaming for one-row decode steps (TP = 1; the GEMV, where its plan lists
        the shape): every projection and the LM head get an OCP MXFP4 copy (q, e) -- e2m1 codes,
        one e8m0 scale per 32 k (ops.quantize_mxfp4_rows) -- and the resident weights are REPLACED
        by its exact image W' = code * 2^(e - 127).  Every kernel that reads W' (prefill, steps of
        2+ rows, mixed steps, sampled logits, the CPU reference) then computes the same model the
        4-bit kernel streams.  Lossier than FP8: a projection's output moves by roughly 11 % in
        relative L2 norm for Gaussian weights -- an opt-in latency / quality trade.  The copies
        cost memory (about +27 % of the projections) and save none.  Call after random init or
        load_state_dict_hf, before any decode graph is captured."""
        self._quantize("mxfp4", "MXFP4 weights need tp_size == 1: the block scales along K would survive a "
                       "row-parallel split at multiples of 32, but the tensor-parallel path is neither "
                       "built nor tested")

    def _quantize(self, fmt: str, tp_error: str) -> None:
        """Every projection and the LM head get a copy in format ``fmt`` (ops.STREAMED) and are
        replaced by its exact image."""
        if self.tp != 1:
            raise ValueError(tp_error)
        if self.streamed is not None:
            if self.streamed.fmt == fmt:
                return
            entry = {"fp8-e4m3": "quantize_fp8", "mxfp4": "quantize_mxfp4"}[self.streamed.fmt]
            raise ValueError(f"{entry}() was already applied: one model holds one streamed weight format")
        f = ops.STREAMED[fmt]
        layers = []
        for L in self.layers:
            d = {}
            for k in self.STREAMED_WEIGHTS:
                d[k] = f.quantize(L[k])
                L[k] = f.dequantize(*d[k], self.dtype)
            layers.append(d)
        head = f.quantize(self.lm_head)
        self.lm_head = f.dequantize(*head, self.dtype)
        self.streamed = Streamed(fmt, layers, head)
        if fmt == "mxfp4" and self.device.type == "cuda":
            # the quantizer's fp32 temporaries (gigabytes for the LM head) go back to the driver:
            # the engine sizes the KV pool from the HBM that is free after the weights
            torch.cuda.empty_cache()

    def _held(self, fmt: str, part: str):
        s = self.streamed
        return getattr(s, part) if s is not None and s.fmt == fmt else None

    # the copies by format (None unless the model streams that format), as tests and probes read them
    fp8 = property(lambda self: self._held("fp8-e4m3", "layers"))
    lm_head_fp8 = property(lambda self: self._held("fp8-e4m3", "lm_head"))
    mx4 = property(lambda self: self._held("mxfp4", "layers"))
    lm_head_mx4 = property(lambda self: self._held("mxfp4", "lm_head"))

    @property
    def weight_format(self) -> str:
        return self.streamed.fmt if self.streamed is not None else "bf16"

    def weight_bytes(self) -> int:
        n = self.embed.numel() + self.lm_head.numel() + self.final_norm.numel()
        for L in self.layers:
            n += sum(t.numel() for t in L.values())
        n *= self.embed.element_size()
        if self.streamed is not None:   # the copies (codes + scales) are held next to the bf16 image
            for pair in [self.streamed.lm_head] + [p for d in self.streamed.layers for p in d.values()]:
                n += sum(t.numel() * t.element_size() for t in pair)
        return n

    # ------------------------------------------------------------------ step plan
    def _step_plan(self, M: int, meta: AttnMeta, on_gpu: bool, kv8: bool, fused_attn: bool = False) -> StepPlan:
        """The kernels of a forward over M rows, from shapes, ``meta`` fields, ``self.tp`` and the
        module flags alone (no tensor data).  ``on_gpu``: the step's tensors are device tensors;
        ``kv8``: FP8 KV cache; ``fused_attn``: the per-row decode attention reads the QKV slabs
        itself (ops.fused_decode_ok of the cache).  Decode steps stream every weight once: per
        projection a split-K kernel emits slabs straight into the fused consumers (RoPE + KV write
        for QKV, (TP all-reduce +) residual add + RMSNorm for O / down); steps of 1..max_rows rows
        (FP8: 128, MXFP4: 32) of a quantized model read its streamed copy where the format's plans list a kernel
        (ops.streamed_plan / streamed_glu_kind), everything else the bf16 image W'."""
        plan = StepPlan()
        decode = not meta.prefill
        shape = {k: tuple(self.layers[0][k].shape) for k in self.STREAMED_WEIGHTS}
        s = self.streamed
        fmt = s.fmt if (decode and s is not None and on_gpu and 1 <= M <= ops.STREAMED[s.fmt].max_rows) else ""
        # a short prefill (<= ops.MID_M_MAX prompt tokens: batch-1 serving) has the decode
        # step's shape -- too few rows for the 256 x 256 prefill GEMM's tiles -- so it takes
        # the same split-K projection plans and fused consumers (RoPE + KV write, add + norm)
        # (ops.prefill_route mirrors the prefill plan choices below for the GEMM probes and
        # tests/test_pgemm_gpu.py::test_prefill_route_products -- keep the two in step)
        small = not decode and on_gpu and _PREFILL_MID and M <= ops.MID_M_MAX
        if decode or small:
            # bf16 split-K slabs (ops.SLAB_BF16) where the consumer is the RoPE + cache-write
            # kernel (QKV) or the TP = 1 add + RMSNorm (O / down); the fused attention kernels
            # that read QKV slabs themselves take fp32 only
            s16 = on_gpu and self.tp == 1 and ops.SLAB_BF16
            if decode and meta.shared_len is not None:      # cascade: the grouped kernel reading the slabs
                qkv_rope = not (meta.decode_groups is not None and meta.decode_inline and _GROUP_FUSED
                                and not kv8 and meta.slot_mapping is not None)
            else:
                qkv_rope = not (decode and fused_attn)
            b16 = {"qkv": s16 and qkv_rope, "o": s16, "down": s16}
            for k in ("qkv", "o", "down"):
                N, K = shape[k]
                kind, S, R = ops.streamed_plan(fmt, M, N, K) if fmt else ("", 0, 0)
                if kind:
                    # the GEMV, the ring kernel or the wide kernel over the streamed pair
                    plan.streamed[k] = kind
                    plan.proj[k] = ("streamed_" + kind, S, R, False)
                    continue
                S, R = ops.gemv_plan(M, N, K) if on_gpu else (0, 0)
                if S:
                    # one row: the register-streaming GEMV (no LDS ring) -- QKV / O
                    plan.proj[k] = ("gemv", S, R, False)
                    continue
                S, c = ops.mid_plan(M, N, K)
                if S:
                    plan.proj[k] = ("mgemm", S, c, bool(b16[k] and S > 1))
                else:
                    S, t = ops.decode_plan(M, N, K)
                    plan.proj[k] = ("dgemm", S, t, False)
            if small and M > 256:
                # a 257..512-token prefill's down projection (decode buckets keep their plan):
                # the 256 x 256 kernel's S=8 slabs where K is long -- 8B: 66.1 vs the mid-M
                # kernel's S=4 77.5 and hipBLASLt's 97.4 us at 512 rows
                # (profiles/r6_prefill_mid_plans.log); the 70B TP-8 shard keeps mid_plan's
                Sd = ops.down_small_split(M, *shape["down"])
                if Sd:
                    plan.proj["down"] = ("pgemm", Sd, 0, False)
            N, K = shape["gate_up"]
            kind = ops.streamed_glu_kind(fmt, M, N, K) if fmt else ""
            if kind:
                plan.streamed["gate_up"] = kind
                plan.glu = ("streamed_" + kind,)
            elif decode and on_gpu and ops.gemv_glu_ok(M, N, K):
                plan.glu = ("gemv_glu",)      # one row: the register-streaming GEMV with SwiGLU
            elif small and (ops.pgemm_ok(M, N, K) or ops.prefill_split_plan(M, N, K, glu=True)):
                # 256 x 256 tiles with SwiGLU (104 vs 141 us at M = 512), or their split-K
                # slabs into the SwiGLU consumer where too few tiles (the 70B TP-8 shard)
                plan.glu = ("prefill_glu",)
            elif decode and s16 and ops.glu_split16_plan(M, N, K)[0]:
                plan.glu = ("glu_split16", *ops.glu_split16_plan(M, N, K))
            else:
                Sg, cg = ops.mid_plan(M, N, K, glu=True)
                plan.glu = ("mgemm_glu", cg) if Sg else ("glu_linear",)
        elif on_gpu:
            # 513..2048-token prefills: split-K slab plans where they win with the consumer
            s16 = self.tp == 1 and ops.SLAB_BF16      # bf16 slabs: see the decode plans above
            for k in ("qkv", "o", "down"):
                S, c = ops.prefill_plan(M, *shape[k])
                if S >= 2:
                    plan.proj[k] = ("mgemm", S, c, bool(s16))
                elif not S:
                    # narrow tensor-parallel shards: the 256 x 256 tiles split over K
                    Sp = ops.prefill_split_plan(M, *shape[k])
                    if Sp:
                        plan.proj[k] = ("pgemm", Sp, 0, False)
        if self.tp > 1 and not on_gpu:
            # CPU TP rehearsal: row-parallel partials as fp32 slabs, all-reduced before the one
            # bf16 rounding (comm.tp_add_rmsnorm), so TP = N tracks TP = 1's rounding
            for k in ("o", "down"):
                if not plan.splits(k):
                    plan.proj[k] = ("linear32", 1, 0, False)
        # batch 1 (<= ops.NORM_FUSE_ROWS rows, TP = 1): O / down with the residual add + RMSNorm
        # in the projection's own last workgroup -- no add_rmsnorm_splitk launch
        if decode and self.tp == 1 and on_gpu and not plan.streamed:
            for k in ("o", "down"):
                S = ops.dgemm_norm_plan(M, *shape[k])
                if S:
                    plan.nf[k] = S
        # batch 1 (one row, TP = 1, skinny-kernel plans): the gate|up and the next layer's QKV
        # projection build their input row themselves -- residual add + RMSNorm of the previous
        # projection's slabs, in LDS, under their first weight stages (dgemm.hip XNormIn) --
        # so no add_rmsnorm launch runs between projections; the residual ping-pongs between
        # two buffers (one workgroup writes the new one while the others read the old)
        plan.xn = bool(decode and self.tp == 1 and not plan.nf and on_gpu
                       and plan.splits("qkv") and plan.splits("o") and plan.splits("down")
                       and ops.xn_ok(M, self.cfg.hidden) and not ops.mid_plan(M, *shape["gate_up"], glu=True)[0])
        return plan

    def _partial(self, p: tuple, a, w):
        """Split-K slabs of one StepPlan.proj entry: ``a`` times the weight (or streamed pair) ``w``."""
        fam, S, r, b16 = p
        if fam.startswith("streamed_"):
            return ops.streamed_partial(self.streamed.fmt, fam[9:], a, w, S, r)
        if fam == "gemv":
            return ops.gemv_partial(a, w, S, r)
        if fam == "mgemm" and S == 1:
            return ops.mgemm_partial(a, w, 1, r).float()[None]
        if fam == "mgemm":
            return ops.mgemm_partial(a, w, S, r, bf16=b16)
        if fam == "dgemm":
            return ops.dgemm_partial(a, w, S, r)
        if fam == "pgemm":
            return ops.pgemm_partial(a, w, S)
        if fam == "linear32":
            return F.linear(a.float(), w.float())[None]
        raise ValueError(f"no kernel family {fam!r}")

    def _glu(self, plan: StepPlan, a, w):
        """silu(a Wg^T) * (a Wu^T) on the kernel of StepPlan.glu: the streamed pair's, or the bf16
        ops wrapper the plan names (gemv_glu, prefill_glu, glu_split16, mgemm_glu, glu_linear)."""
        fam, *args = plan.glu
        if fam.startswith("streamed_"):
            return ops.streamed_glu(self.streamed.fmt, fam[9:], a, w)
        return getattr(ops, fam)(a, w, *args)

    # ------------------------------------------------------------------ forward
    def forward(self, input_ids: torch.Tensor, meta: AttnMeta, kv_caches: list,
                logits_index: torch.Tensor | None = None, greedy_ids: bool = False) -> torch.Tensor:
        """input_ids [T] int32 -> logits [R, vocab_shard] for the rows selected by
        ``logits_index`` (all rows if None).  kv_caches: list of (k_cache, v_cache).
        ``greedy_ids``: return the greedy token ids int64 [R] instead (the LM head's argmax
        is fused into its GEMM where :func:`ops.lm_head_argmax_ok`)."""
        cfg = self.cfg
        D, hq, hkv, eps = cfg.head_dim, self.hq, self.hkv, cfg.rms_eps
        h, x = ops.embed_rmsnorm(input_ids, self.embed, self.layers[0]["in_norm"], eps)
        residual = h
        nl = len(self.layers)
        decode = not meta.prefill
        # an FP8 KV cache is written by rope_cache / rope_cache_splitk only: the attention
        # kernels that fuse RoPE and the new token's cache write store bf16
        kv8 = bool(kv_caches) and ops.kv_is_fp8(kv_caches[0][0])
        group_fused, cascade_rope = _GROUP_FUSED and not kv8, _CASCADE_ROPE and not kv8
        lin = ops.decode_linear if decode else ops.prefill_linear
        M = x.shape[0]
        cascade = decode and meta.shared_len is not None
        # which kernel every projection runs (split 0 = library GEMM + plain consumer)
        plan = self._step_plan(M, meta, x.is_cuda, kv8,
                               fused_attn=(decode and not cascade and meta.block_tables is not None
                                           and bool(kv_caches)
                                           and ops.fused_decode_ok(kv_caches[0][0], meta.block_tables)))
        sq, so, sd = plan.splits("qkv"), plan.splits("o"), plan.splits("down")
        nf, xn = plan.nf, plan.xn
        fmt = self.streamed.fmt if plan.streamed else ""
        if nf and self._ntick is None:
            self._ntick = torch.zeros(1, dtype=torch.int32, device=self.device)
        trim = (not decode and _PREFILL_TRIM and x.is_cuda and logits_index is not None and self.layers
                and meta.block_tables is not None and meta.prefix_lens is not None
                and logits_index.numel() == meta.block_tables.shape[0] and M > logits_index.numel())
        res2 = torch.empty_like(residual) if xn else None
        pd = None   # XN: the previous layer's down-projection slabs
        for i, L in enumerate(self.layers):
            kc, vc = kv_caches[i]
            if plan.streamed:   # this layer's weights: the streamed pairs where the plan reads them
                L = {**L, **{k: self.streamed.layers[i][k] for k in plan.streamed}}
            if sq:
                if xn and pd is not None:
                    Sg, R = ops.gemv_plan(M, *self.layers[i]["qkv"].shape)
                    if "qkv" in plan.streamed:
                        qkv_slabs = ops.streamed_partial_xn(fmt, plan.streamed["qkv"], pd, residual, res2,
                                                            L["in_norm"], eps, L["qkv"], sq, plan.proj["qkv"][2])
                    elif Sg == sq:
                        qkv_slabs = ops.gemv_partial_xn(pd, residual, res2, L["in_norm"], eps, L["qkv"], sq, R)
                    else:
                        qkv_slabs = ops.dgemm_partial_xn(pd, residual, res2, L["in_norm"], eps, L["qkv"], sq)
                    residual, res2 = res2, residual
                else:
                    qkv_slabs = self._partial(plan.proj["qkv"], x, L["qkv"])
            if cascade:
                # shared-prefix decode: RoPE + cache write, then prefix-once + suffix attention
                if (sq and meta.decode_groups is not None and meta.decode_inline and x.is_cuda
                        and group_fused and meta.slot_mapping is not None):
                    # the group kernel reads the QKV slabs itself (RoPE + new-token cache write)
                    a = ops.paged_decode_grouped_fused(qkv_slabs, meta.positions, self.cos_sin, meta.slot_mapping,
                                                       kc, vc, meta.block_tables, meta.context_lens, hq,
                                                       self.scale, meta.shared_table, meta.shared_len,
                                                       meta.cascade_chunks, meta.decode_groups, self._decode_tick(M))
                elif sq:
                    qkv = ops.rope_cache_splitk(qkv_slabs, meta.positions,
                                                self.cos_sin, meta.slot_mapping, kc, vc, hq, hkv, D)
                    if meta.decode_groups is not None:
                        a = ops.paged_decode_cascade_grouped(qkv, kc, vc, meta.block_tables, meta.context_lens,
                                                             hq, self.scale, meta.shared_table, meta.shared_len,
                                                             meta.cascade_chunks, meta.decode_groups,
                                                             meta.decode_defer,
                                                             self._decode_tick(M) if x.is_cuda else None,
                                                             meta.decode_inline)
                    else:
                        a = ops.paged_decode_cascade(qkv, kc, vc, meta.block_tables, meta.context_lens, hq,
                                                     meta.max_context, self.scale, meta.shared_table,
                                                     meta.shared_len, meta.cascade_chunks, meta.seq_order)
                elif not cascade_rope:
                    qkv = lin(x, L["qkv"])
                    ops.rope_cache(qkv, meta.positions, self.cos_sin, meta.slot_mapping, kc, vc, hq, hkv, D)
                    if meta.decode_groups is not None:
                        a = ops.paged_decode_cascade_grouped(qkv, kc, vc, meta.block_tables, meta.context_lens,
                                                             hq, self.scale, meta.shared_table, meta.shared_len,
                                                             meta.cascade_chunks, meta.decode_groups,
                                                             meta.decode_defer,
                                                             self._decode_tick(M) if x.is_cuda else None,
                                                             meta.decode_inline)
                    else:
                        a = ops.paged_decode_cascade(qkv, kc, vc, meta.block_tables, meta.context_lens, hq,
                                                     meta.max_context, self.scale, meta.shared_table,
                                                     meta.shared_len, meta.cascade_chunks, meta.seq_order)
                else:
                    # library-GEMM QKV: RoPE + new-token cache write fused into the cascade kernels
                    a = ops.paged_decode_cascade_rope(lin(x, L["qkv"]), meta.positions, self.cos_sin,
                                                      meta.slot_mapping, kc, vc, meta.block_tables,
                                                      meta.context_lens, hq, meta.max_context, self.scale,
                                                      meta.shared_table, meta.shared_len,
                                                      meta.cascade_chunks, meta.seq_order)
                qkv = None
            elif decode and sq and ops.fused_decode_ok(kc, meta.block_tables):
                # QKV partials -> RoPE + new-token cache write + attention, one launch
                a = ops.paged_decode_fused(qkv_slabs, meta.positions, self.cos_sin,
                                           meta.slot_mapping, kc, vc, meta.block_tables, meta.context_lens,
                                           hq, meta.max_context, self.scale, meta.seq_order,
                                           self._decode_tick(M) if x.is_cuda else None)
                qkv = None
            elif sq:
                qkv = ops.rope_cache_splitk(qkv_slabs, meta.positions, self.cos_sin,
                                            meta.slot_mapping, kc, vc, hq, hkv, D)
            else:
                qkv = lin(x, L["qkv"])
                ops.rope_cache(qkv, meta.positions, self.cos_sin, meta.slot_mapping, kc, vc, hq, hkv, D)
            if trim and i == nl - 1 and qkv is not None:
                # last layer of a prefill whose logits are wanted for a few rows only: every
                # token's K/V is in the cache now; only the selected rows go on through
                # attention, O and the MLP (their outputs are the only ones anything reads)
                # -- each selected row is its sequence's last token, so its attention over
                # the paged cache is exactly the decode attention at that context length
                ctx = meta.prefix_lens + (meta.cu_seqlens[1:] - meta.cu_seqlens[:-1])
                a = ops.paged_decode(qkv.index_select(0, logits_index).contiguous(), kc, vc, meta.block_tables,
                                     ctx, hq, meta.block_tables.shape[1] * kc.shape[2], self.scale)
                residual = residual.index_select(0, logits_index)
                logits_index = None
                qkv = None
            if qkv is None:
                pass
            elif meta.prefill and meta.prefix_lens is not None:
                # prompt prefix already in the paged cache: attend over cache (prefix + new)
                a = ops.flash_prefill_paged(qkv, meta.cu_seqlens, meta.max_len, hq, hkv, D, self.scale,
                                            kc, vc, meta.block_tables, meta.prefix_lens)
            elif meta.prefill:
                a = ops.flash_prefill(qkv, meta.cu_seqlens, meta.max_len, hq, hkv, D, self.scale, True)
            else:
                a = ops.paged_decode(qkv, kc, vc, meta.block_tables, meta.context_lens, hq,
                                     meta.max_context, self.scale, meta.seq_order)
            nxt = self.layers[i + 1]["in_norm"] if i + 1 < nl else self.final_norm
            if xn:
                po = self._partial(plan.proj["o"], a, L["o"])
                if "gate_up" in plan.streamed:
                    g = ops.streamed_glu_xn(fmt, plan.streamed["gate_up"], po, residual, res2, L["post_norm"], eps,
                                            L["gate_up"])
                elif ops.gemv_glu_ok(M, *L["gate_up"].shape):
                    g = ops.gemv_glu_xn(po, residual, res2, L["post_norm"], eps, L["gate_up"])
                else:
                    g = ops.dgemm_glu_xn(po, residual, res2, L["post_norm"], eps, L["gate_up"])
                residual, res2 = res2, residual
                pd = self._partial(plan.proj["down"], g, L["down"])
                if i + 1 == nl:
                    x = ops.add_rmsnorm_splitk(pd, residual, nxt, eps)
                continue
            # row-parallel O: (TP all-reduce +) residual add + RMSNorm in one consumer
            if "o" in nf:
                x = ops.dgemm_add_rmsnorm(a, L["o"], nf["o"], residual, L["post_norm"], eps, self._ntick)
            else:
                x = comm.tp_add_rmsnorm(self._partial(plan.proj["o"], a, L["o"]) if so else lin(a, L["o"]),
                                        residual, L["post_norm"], eps)
            g = self._glu(plan, x, L["gate_up"])
            if "down" in nf:
                x = ops.dgemm_add_rmsnorm(g, L["down"], nf["down"], residual, nxt, eps, self._ntick)
            else:
                x = comm.tp_add_rmsnorm(self._partial(plan.proj["down"], g, L["down"]) if sd else lin(g, L["down"]),
                                        residual, nxt, eps)
        if logits_index is not None:
            x = x.index_select(0, logits_index)
        if greedy_ids:
            return self.greedy_ids(x)
        return ops.lm_head_logits(x, self.lm_head)

    def forward_mixed(self, input_ids: torch.Tensor, n_dec: int, dmeta: AttnMeta, pmeta: AttnMeta,
                      kv_caches: list, logits_index: torch.Tensor, return_logits: bool = False) -> torch.Tensor:
        """One forward over decode rows AND a prefill chunk (continuous batching without the
        prefill stall): rows [0, n_dec) are decode slots (one new token each, paged decode
        attention over their cache -- ``dmeta``, the decode step's metadata), rows
        [n_dec, T) are prompt-chunk tokens (``pmeta``: positions / slots / cu_seqlens /
        block_tables / prefix_lens of the chunk; attention over cached prefix + chunk).
        Every projection runs ONCE over all T rows -- the decode rows ride in the prefill
        GEMMs' weight pass -- and only attention is split by row kind.  Returns the greedy
        ids of the rows in ``logits_index``.
        Reference parity: the service loop the reference runs one request at a time
        (llm-qa/main.py:111-117)."""
        cfg = self.cfg
        D, hq, hkv, eps = cfg.head_dim, self.hq, self.hkv, cfg.rms_eps
        h, x = ops.embed_rmsnorm(input_ids, self.embed, self.layers[0]["in_norm"], eps)
        residual = h
        positions = torch.cat([dmeta.positions, pmeta.positions]) if n_dec else pmeta.positions
        slots = torch.cat([dmeta.slot_mapping, pmeta.slot_mapping]) if n_dec else pmeta.slot_mapping
        nl = len(self.layers)
        M = x.shape[0]
        for i, L in enumerate(self.layers):
            kc, vc = kv_caches[i]
            qkv = ops.prefill_linear(x, L["qkv"])
            ops.rope_cache(qkv, positions, self.cos_sin, slots, kc, vc, hq, hkv, D)
            parts = []
            if n_dec:
                parts.append(self._attend_decode(qkv[:n_dec], dmeta, kc, vc, n_dec))
            parts.append(ops.flash_prefill_paged(qkv[n_dec:], pmeta.cu_seqlens, pmeta.max_len, hq, hkv, D,
                                                 self.scale, kc, vc, pmeta.block_tables, pmeta.prefix_lens))
            a = torch.cat(parts) if len(parts) > 1 else parts[0]
            nxt = self.layers[i + 1]["in_norm"] if i + 1 < nl else self.final_norm
            x = comm.tp_add_rmsnorm(ops.prefill_linear(a, L["o"]), residual, L["post_norm"], eps)
            g = ops.prefill_glu(x, L["gate_up"])
            x = comm.tp_add_rmsnorm(ops.prefill_linear(g, L["down"]), residual, nxt, eps)
        assert x.shape[0] == M
        if return_logits:          # tests: the selected rows' logits instead of their greedy ids
            return ops.lm_head_logits(x.index_select(0, logits_index).contiguous(), self.lm_head)
        return self.greedy_ids(x.index_select(0, logits_index))

    def _attend_decode(self, qkv: torch.Tensor, meta: AttnMeta, kc, vc, M: int) -> torch.Tensor:
        """Decode attention of post-RoPE bf16 QKV rows whose new K/V are already in the
        cache: the grouped / plain cascade kernels when the step attends a shared prefix,
        else per-row paged decode (the same dispatch as :meth:`forward`'s library-GEMM
        branch)."""
        hq = self.hq
        if meta.shared_len is not None:
            if meta.decode_groups is not None:
                return ops.paged_decode_cascade_grouped(qkv, kc, vc, meta.block_tables, meta.context_lens, hq,
                                                        self.scale, meta.shared_table, meta.shared_len,
                                                        meta.cascade_chunks, meta.decode_groups, meta.decode_defer,
                                                        self._decode_tick(M) if qkv.is_cuda else None,
                                                        meta.decode_inline)
            return ops.paged_decode_cascade(qkv, kc, vc, meta.block_tables, meta.context_lens, hq,
                                            meta.max_context, self.scale, meta.shared_table, meta.shared_len,
                                            meta.cascade_chunks, meta.seq_order)
        return ops.paged_decode(qkv, kc, vc, meta.block_tables, meta.context_lens, hq, meta.max_context,
                                self.scale, meta.seq_order)

    def _decode_tick(self, B: int):
        """Ticket words for the fused decode attention's in-kernel partition merge, shared
        by every layer (the launches are stream-ordered and each re-arms its words).  The
        grouped kernel indexes them by plan row, and a plan holds up to
        bucket x DOCQA_GROUP_CAP_MULT rows (engine/llm_engine.py), so the buffer is sized for
        the largest bucket x that multiple ONCE, before any graph is captured, and never
        reallocated: a captured graph keeps pointing at it."""
        import os

        mult = max(1, int(os.environ.get("DOCQA_GROUP_CAP_MULT", "1")))
        need = max(B, 1) * mult * self.hkv
        if self._tick is None:
            self._tick = ops.decode_ticket(max(B, 4096) * mult * self.hkv, self.device)
        if self._tick.numel() < need:
            raise RuntimeError(f"decode ticket buffer holds {self._tick.numel()} words, a {B}-row bucket "
                               f"needs {need}: raise the first bucket size (buffers are never regrown)")
        return self._tick

    def greedy_ids(self, x: torch.Tensor) -> torch.Tensor:
        """Greedy token ids int64 [R] of the final normed hidden rows ``x``: the LM-head GEMM
        with its argmax fused (mgemm.hip EPI_ARGMAX, no [R, vocab] logits) where the shape
        allows, the vocab-parallel pick resolved by one packed-key MAX all-reduce at TP > 1."""
        R = x.shape[0]
        N, K = self.lm_head.shape
        fused = ops.lm_head_argmax_ok(R, N, K) or (self.tp > 1 and 0 < R <= ops.MID_M_MAX
                                                   and ops.lm_head_argmax_shape_ok(N, K))
        if self.tp == 1:
            if fused:
                s = self.streamed
                return ops.lm_head_argmax(x, self.lm_head, self.cfg.vocab_size,
                                          streamed=(s.fmt, s.lm_head) if s is not None else None)
            return self.greedy(ops.lm_head_logits(x, self.lm_head))
        if fused and self.vocab_valid > 0:
            ids, vals = ops.lm_head_argmax(x, self.lm_head, self.vocab_valid, with_values=True)
        else:
            logits = ops.lm_head_logits(x, self.lm_head)[:, : max(1, self.vocab_valid)]
            ids = ops.argmax(logits)
            vals = logits.gather(1, ids[:, None])[:, 0].float()
        if self.vocab_valid == 0:
            vals = torch.full_like(vals, float("-inf"))
        return comm.tp_argmax(vals, ids + self.vocab_start)

    def greedy(self, logits: torch.Tensor) -> torch.Tensor:
        """argmax over the (possibly vocab-parallel) logits -> int64 [R]."""
        if self.tp == 1:
            return ops.argmax(logits)
        valid = logits[:, : max(1, self.vocab_valid)]
        idx = ops.argmax(valid)
        val = valid.gather(1, idx[:, None])[:, 0].float()
        if self.vocab_valid == 0:
            val = torch.full_like(val, float("-inf"))
        return comm.tp_argmax(val, idx + self.vocab_start)

    def full_logits(self, logits: torch.Tensor) -> torch.Tensor:
        full = comm.tp_all_gather_last(logits)
        return full[:, : self.cfg.vocab_size]
