"""FP8 (OCP e4m3, no scales) paged KV cache on the reference path: pool accounting, the
DOCQA_KV_CACHE option, the cache write (codes = the e4m3 image of what the bf16 path stores,
their exact image written back to the packed QKV row) and a CPU engine end to end with the
block prefix cache and the token-granular tail cache on an FP8 pool."""
import pytest
import torch

from docqa_amd import ops
from docqa_amd.engine.kv_cache import KVCache, resolve_kv_dtype
from docqa_amd.engine.llm_engine import LLMEngine, SamplingParams
from docqa_amd.models.llama import LlamaConfig, LlamaModel
from docqa_amd.ops import reference as R

FP8 = torch.float8_e4m3fn


def test_bytes_per_block_halves_and_budget_doubles():
    b16 = KVCache.bytes_per_block(4, 2, 128, 64, torch.bfloat16)
    b8 = KVCache.bytes_per_block(4, 2, 128, 64, FP8)
    assert b16 == KVCache.bytes_per_block(4, 2, 128, 64) == 2 * 4 * 2 * 128 * 64 * 2
    assert 2 * b8 == b16
    budget = 10 * b16 + 3
    kv16 = KVCache.for_budget(4, 2, 128, budget, 64, "cpu", torch.bfloat16)
    kv8 = KVCache.for_budget(4, 2, 128, budget, 64, "cpu", FP8)
    assert kv16.num_blocks == 10 and kv8.num_blocks == 20
    k, v = kv8.caches[0]
    assert k.dtype == v.dtype == FP8 and k.shape == (20, 2, 64, 128)
    assert int(k.view(torch.uint8).max()) == 0 and int(v.view(torch.uint8).max()) == 0   # zero-initialised


def test_kv_cache_option_validation(monkeypatch):
    monkeypatch.delenv("DOCQA_KV_CACHE", raising=False)
    assert resolve_kv_dtype(None, torch.bfloat16) == torch.bfloat16
    assert resolve_kv_dtype("fp8", torch.bfloat16) == FP8
    assert resolve_kv_dtype("bf16", torch.float32) == torch.float32
    monkeypatch.setenv("DOCQA_KV_CACHE", "fp8")
    assert resolve_kv_dtype(None, torch.bfloat16) == FP8
    m = LlamaModel(LlamaConfig.preset("tiny"), device="cpu", dtype=torch.float32, seed=1)
    eng = LLMEngine(m, max_batch=2, max_context=64, block_size=16, use_graphs=False)
    assert eng.kv_fp8 and eng.kv.caches[0][0].dtype == FP8
    assert not LLMEngine(m, max_batch=2, max_context=64, block_size=16, use_graphs=False, kv_dtype="bf16").kv_fp8
    monkeypatch.setenv("DOCQA_KV_CACHE", "int4")
    with pytest.raises(ValueError):
        LLMEngine(m, max_batch=2, max_context=64, block_size=16, use_graphs=False)
    with pytest.raises(ValueError):
        LLMEngine(m, max_batch=2, max_context=64, block_size=16, use_graphs=False, kv_dtype="fp4")
    with pytest.raises(ValueError):          # a torch dtype: the model's or e4m3, nothing else
        resolve_kv_dtype(torch.float16, torch.bfloat16)
    assert resolve_kv_dtype(FP8, torch.bfloat16) == FP8 and resolve_kv_dtype(torch.float32, torch.float32) == torch.float32
    from docqa_amd.config import Settings

    monkeypatch.setenv("DOCQA_KV_CACHE", "fp8")
    assert Settings().kv_cache == "fp8"


def _write_inputs(T=5, Hq=8, Hkv=2, D=128, seed=0):
    g = torch.Generator().manual_seed(seed)
    qkv = (torch.randn(T, (Hq + 2 * Hkv) * D, generator=g) * 2).to(torch.bfloat16)
    x = qkv.view(T, Hq + 2 * Hkv, D)
    x[4, Hq + 1, :8] = torch.tensor([1000.0, -1000.0, 449.0, -460.0, 3e4, -3e4, 500.0, -448.0]).to(torch.bfloat16)
    x[2, Hq + Hkv, :8] = torch.tensor([2e3, -2e3, 2.0 ** -10, -(2.0 ** -10), 2.0 ** -11, 1.5 * 2.0 ** -10,
                                       2.0 ** -9, -(2.0 ** -12)]).to(torch.bfloat16)
    x[3, Hq + Hkv + 1, 8:12] = torch.tensor([1e-3, -7e-4, 1e-5, 0.0]).to(torch.bfloat16)
    pos = torch.tensor([0, 7, 63, 64, 130], dtype=torch.int32)
    cs = R.rope_cos_sin(256, D, 500000.0)
    return qkv, pos, cs


def test_reference_write_codes_and_image():
    Hq, Hkv, D, BS, NB = 8, 2, 128, 64, 3
    qkv, pos, cs = _write_inputs()
    slots = torch.tensor([5, -1, 63, 2 * BS, 70], dtype=torch.int32)     # -1, offset 63, offset 0 of block 2
    k16 = torch.zeros(NB, Hkv, BS, D, dtype=torch.bfloat16)
    v16 = torch.zeros_like(k16)
    q16 = qkv.clone()
    R.rope_cache(q16, pos, cs, slots, k16, v16, Hq, Hkv, D)
    sentinel = 0x55
    k8 = torch.full((NB, Hkv, BS, D), sentinel, dtype=torch.uint8).view(FP8)
    v8 = torch.full((NB, Hkv, BS, D), sentinel, dtype=torch.uint8).view(FP8)
    q8 = qkv.clone()
    R.rope_cache(q8, pos, cs, slots, k8, v8, Hq, Hkv, D)
    written = torch.zeros(NB, BS, dtype=torch.bool)
    for s in slots.tolist():
        if s >= 0:
            written[s // BS, s % BS] = True
    for c8, c16 in ((k8, k16), (v8, v16)):
        want = c16.float().clamp(-448, 448).to(FP8).view(torch.uint8)
        got = c8.view(torch.uint8)
        w = written[:, None, :, None].expand_as(got)
        assert torch.equal(got[w], want[w])
        assert bool((got[~w] == sentinel).all())                # untouched slots keep their bytes
        assert not bool(((got == 0x7F) | (got == 0xFF)).any())  # never a NaN code
    # beyond +-448 saturates to 0x7e / 0xfe (V is not rotated: the planted values survive)
    sat = v8.view(torch.uint8)[0, 0, 63, :8].tolist()           # token 2 -> slot 63, V head 0
    assert sat[0] == 0x7E and sat[1] == 0xFE
    assert sat[2] == 0x00 and sat[3] == 0x80                    # +-2^-10: ties to even -> +-0
    assert sat[4] == 0x00 and sat[5] == 0x01 and sat[6] == 0x01 and sat[7] == 0x80   # 2^-11, 1.5 * 2^-10, 2^-9, -2^-12
    # the K/V part of qkv is the dequantised codes, bitwise; Q is the bf16 path's
    x8, x16 = q8.view(5, Hq + 2 * Hkv, D), q16.view(5, Hq + 2 * Hkv, D)
    assert torch.equal(x8[:, :Hq], x16[:, :Hq])
    img = x16[:, Hq:].float().clamp(-448, 448).to(FP8).to(torch.bfloat16)
    assert torch.equal(x8[:, Hq:].view(torch.int16), img.view(torch.int16))
    for t, s in enumerate(slots.tolist()):
        if s >= 0:
            assert torch.equal(k8[s // BS, :, s % BS].to(torch.bfloat16).view(torch.int16),
                               x8[t, Hq:Hq + Hkv].view(torch.int16))
            assert torch.equal(v8[s // BS, :, s % BS].to(torch.bfloat16).view(torch.int16),
                               x8[t, Hq + Hkv:].view(torch.int16))


def test_reference_codes_of_nan_and_inf():
    c = R.kv_fp8_codes(torch.tensor([float("nan"), float("inf"), float("-inf"), 448.0, -449.0]))
    assert c.view(torch.uint8).tolist() == [0xFE, 0x7E, 0xFE, 0x7E, 0xFE]


def test_reference_attention_reads_fp8_caches():
    """paged_decode / cascade / paged prefill on an FP8 cache == the same op on the codes'
    bf16 image (the reference reads ``.float()`` of either)."""
    Hq, Hkv, D, BS, NB, B = 8, 2, 128, 16, 12, 3
    g = torch.Generator().manual_seed(3)
    k8 = R.kv_fp8_codes(torch.randn(NB, Hkv, BS, D, generator=g))
    v8 = R.kv_fp8_codes(torch.randn(NB, Hkv, BS, D, generator=g))
    k16, v16 = k8.to(torch.bfloat16), v8.to(torch.bfloat16)
    bt = torch.randperm(NB, generator=g).view(B, 4).int()
    cl = torch.tensor([1, 17, 64], dtype=torch.int32)
    q = torch.randn(B, (Hq + 2 * Hkv) * D, generator=g).to(torch.bfloat16)
    a = R.paged_decode(q, k8, v8, bt, cl, Hq, 64, 0.088)
    b = R.paged_decode(q, k16, v16, bt, cl, Hq, 64, 0.088)
    assert torch.equal(a, b)
    bt2 = bt.clone()
    bt2[:, 0] = bt[0, 0]
    pt, plen = bt2[0].clone(), torch.tensor([16], dtype=torch.int32)
    cl2 = torch.tensor([17, 40, 64], dtype=torch.int32)
    assert torch.equal(R.paged_decode_cascade(q, k8, v8, bt2, cl2, Hq, 64, 0.088, pt, plen),
                       R.paged_decode_cascade(q, k16, v16, bt2, cl2, Hq, 64, 0.088, pt, plen))
    cu = torch.tensor([0, 1, 4, 9], dtype=torch.int32)
    qq = torch.randn(9, (Hq + 2 * Hkv) * D, generator=g).to(torch.bfloat16)
    ctx = torch.tensor([0, 13, 32], dtype=torch.int32)
    assert torch.equal(R.flash_prefill_paged(qq, cu, 5, Hq, Hkv, D, 0.088, k8, v8, bt, ctx),
                       R.flash_prefill_paged(qq, cu, 5, Hq, Hkv, D, 0.088, k16, v16, bt, ctx))


def test_copy_rows_bitwise_on_fp8_pools():
    g = torch.Generator().manual_seed(4)
    pools = [(torch.randint(0, 256, (6, 2, 16, 32), generator=g, dtype=torch.uint8).view(FP8),
              torch.randint(0, 256, (6, 2, 16, 32), generator=g, dtype=torch.uint8).view(FP8)) for _ in range(2)]
    before = [(k.view(torch.uint8).clone(), v.view(torch.uint8).clone()) for k, v in pools]
    ops.kv_copy_rows(pools, [(0, 3, 1), (1, 4, 15), (2, 5, 16)])
    for (k, v), (k0, v0) in zip(pools, before):
        for t, t0 in ((k.view(torch.uint8), k0), (v.view(torch.uint8), v0)):
            for src, dst, m in ((0, 3, 1), (1, 4, 15), (2, 5, 16)):
                assert torch.equal(t[dst, :, :m], t0[src, :, :m])       # NaN codes included: bytes
                assert torch.equal(t[dst, :, m:], t0[dst, :, m:])
            assert torch.equal(t[:3], t0[:3])


def test_cpu_engine_fp8_prefix_and_tail_cache_exact():
    """One model whatever the cache state: with an FP8 pool the second batch -- served from the
    block prefix cache and the tail cache -- and an engine without the prefix cache generate
    the first batch's tokens exactly (the un-paged prefill attends the codes' image)."""
    m = LlamaModel(LlamaConfig.preset("tiny"), device="cpu", dtype=torch.float32, seed=3)
    eng = LLMEngine(m, max_batch=4, max_context=512, block_size=16, use_graphs=False, kv_dtype="fp8")
    assert eng.kv.caches[0][0].dtype == FP8
    assert hasattr(eng.kv.allocator, "match_alloc_batch"), "native block manager not loaded"
    pre = list(range(100, 180))
    ps = [pre + [1, 2, 3], pre + [9, 8, 7, 6, 5], pre[:32]]
    sp = SamplingParams(max_new_tokens=5, stop_on_eos=False)
    first = eng.generate(ps, sp)
    assert all(len(o) == 5 for o in first) and eng.stats.cached_tokens == 0
    second = eng.generate(ps, sp)
    assert eng.stats.cached_tokens == sum(len(p) - 1 for p in ps)
    assert eng.tail.hit_tokens == 2 + 4 + 15
    ref = LLMEngine(m, max_batch=4, max_context=512, block_size=16, use_graphs=False, prefix_cache=False,
                    kv_dtype="fp8").generate(ps, sp)
    assert first == second == ref
    for k, v in eng.kv.caches:
        for t in (k.view(torch.uint8), v.view(torch.uint8)):
            assert not bool(((t == 0x7F) | (t == 0xFF)).any())
