"""FP8 (OCP e4m3, no scales) paged KV cache on the GPU: the cache write (rope_cache /
rope_cache_splitk), the 1-byte row copy, the paged prefill gather, the per-row decode
kernel and the wave-parallel grouped decode kernel over codes, the engine routing and the
model end to end.

Attention outputs are compared with the fp32 reference ON THE SAME CODES and with the bf16
kernel on the codes' exact bf16 image.  The FP8 kernels widen the codes in registers and
then run the bf16 kernels' arithmetic, so the bounds are the bf16 kernels' own
(tests/test_group_decode_gpu.py): 3e-2 absolute against fp32, 2e-2 against the bf16 kernel."""
import math
import random

import pytest
import torch

pytestmark = pytest.mark.gpu

FP8 = torch.float8_e4m3fn
D, BS = 128, 64


@pytest.fixture(scope="module", autouse=True)
def native():
    from docqa_amd import ops

    assert ops.load_native(build_if_missing=True)
    torch.manual_seed(0)
    return ops


def _codes(*shape, seed=0):
    """Random finite e4m3 codes (every slot filled: whatever lies past a row's length is
    stale finite K/V) and their exact bf16 image."""
    g = torch.Generator().manual_seed(seed)
    c = torch.randn(*shape, generator=g).clamp(-448, 448).to(FP8).cuda()
    return c, c.to(torch.bfloat16)


def _err(a, b):
    return (a.float() - b.float()).abs().max().item()


# ------------------------------------------------------------------------------ write
@pytest.mark.parametrize("splitk", [False, True])
def test_write_codes_sentinel_and_image(native, splitk):
    Hq, Hkv, NB, T = 8, 2, 3, 5
    W = (Hq + 2 * Hkv) * D
    g = torch.Generator().manual_seed(1)
    x = torch.randn(T, Hq + 2 * Hkv, D, generator=g) * 2
    x[4, Hq + 1, :8] = torch.tensor([1000.0, -1000.0, 449.0, -460.0, 3e4, -3e4, 500.0, -448.0])   # a K head
    x[2, Hq + Hkv, :8] = torch.tensor([2e3, -2e3, 2.0 ** -10, -(2.0 ** -10), 2.0 ** -11, 1.5 * 2.0 ** -10,
                                       2.0 ** -9, -(2.0 ** -12)])                                  # a V head
    x[3, Hq + Hkv + 1, 8:12] = torch.tensor([1e-3, -7e-4, 1e-5, 0.0])
    x[3, Hq + Hkv, 100] = float("nan")     # a NaN V: stored as -448 (code 0xfe), never as a NaN code
    x[0, Hq, 64:72] = torch.tensor([600.0, -700.0, 1e-3, 2e-3, 1e-4, -1e-3, 3e-3, 1.7e-3])         # K at position 0
    pos = torch.tensor([0, 7, 63, 64, 130], dtype=torch.int32, device="cuda")
    slots = torch.tensor([5, -1, 63, 2 * BS, 70], dtype=torch.int32, device="cuda")   # -1, offset 63, offset 0
    cs = native.reference.rope_cos_sin(256, D, 500000.0, "cuda")
    sentinel = 0x55
    k16 = torch.zeros(NB, Hkv, BS, D, dtype=torch.bfloat16, device="cuda")
    v16 = torch.zeros_like(k16)
    k8 = torch.full((NB, Hkv, BS, D), sentinel, dtype=torch.uint8, device="cuda").view(FP8)
    v8 = torch.full((NB, Hkv, BS, D), sentinel, dtype=torch.uint8, device="cuda").view(FP8)
    if splitk:    # two fp32 slabs whose bf16-rounded sum is the row
        xb = x.view(T, W).to(torch.bfloat16).float()
        s0 = (xb * 0.25).to(torch.bfloat16).float()
        P = torch.stack([s0, xb - s0]).cuda().contiguous()
        q16 = native.rope_cache_splitk(P, pos, cs, slots, k16, v16, Hq, Hkv, D)
        q8 = native.rope_cache_splitk(P, pos, cs, slots, k8, v8, Hq, Hkv, D)
    else:
        q16 = x.view(T, W).to(torch.bfloat16).cuda()
        q8 = q16.clone()
        native.rope_cache(q16, pos, cs, slots, k16, v16, Hq, Hkv, D)
        native.rope_cache(q8, pos, cs, slots, k8, v8, Hq, Hkv, D)
    torch.cuda.synchronize()
    written = torch.zeros(NB, BS, dtype=torch.bool)
    for s in slots.tolist():
        if s >= 0:
            written[s // BS, s % BS] = True
    for c8, c16 in ((k8, k16), (v8, v16)):
        # the bf16 kernel's cache as e4m3: clamp(+-448).to(float8_e4m3fn), NaN -> -448 (ops.kv_fp8_codes)
        want = native.kv_fp8_codes(c16.cpu()).view(torch.uint8)
        finite = torch.isfinite(c16.cpu().float())
        assert torch.equal(want[finite], c16.cpu().float().clamp(-448, 448).to(FP8).view(torch.uint8)[finite])
        got = c8.cpu().view(torch.uint8)
        w = written[:, None, :, None].expand_as(got)
        assert torch.equal(got[w], want[w])
        assert bool((got[~w] == sentinel).all())
        assert not bool(((got == 0x7F) | (got == 0xFF)).any())
    sat = v8.cpu().view(torch.uint8)[0, 0, 63, :8].tolist()       # token 2 -> slot 63, V head 0 (not rotated)
    assert sat == [0x7E, 0xFE, 0x00, 0x80, 0x00, 0x01, 0x01, 0x80]
    assert bool(torch.isnan(v16[2, 0, 0, 100])) and int(v8.cpu().view(torch.uint8)[2, 0, 0, 100]) == 0xFE
    assert bool((k16.float().abs() > 448).any()) and bool(((k16.float().abs() < 2.0 ** -9) & (k16 != 0)).any())
    # the packed row: Q as the bf16 kernel leaves it, K / V the codes' exact image
    a8, a16 = q8.cpu().view(T, Hq + 2 * Hkv, D), q16.cpu().view(T, Hq + 2 * Hkv, D)
    assert torch.equal(a8[:, :Hq].view(torch.int16), a16[:, :Hq].view(torch.int16))
    img = native.kv_fp8_codes(a16[:, Hq:]).to(torch.bfloat16)
    assert torch.equal(a8[:, Hq:].view(torch.int16), img.view(torch.int16))


# ------------------------------------------------------------------------------- copy
@pytest.mark.parametrize("m", [1, 63, 64])
def test_copy_rows_bitwise(native, m):
    g = torch.Generator().manual_seed(m)
    pools = [(torch.randint(0, 256, (6, 2, BS, D), generator=g, dtype=torch.uint8).cuda().view(FP8),
              torch.randint(0, 256, (6, 2, BS, D), generator=g, dtype=torch.uint8).cuda().view(FP8)) for _ in range(2)]
    before = [(k.view(torch.uint8).clone(), v.view(torch.uint8).clone()) for k, v in pools]
    native.kv_copy_rows(pools, [(1, 4, m), (0, 5, m)])
    torch.cuda.synchronize()
    for (k, v), (k0, v0) in zip(pools, before):
        for t, t0 in ((k.view(torch.uint8), k0), (v.view(torch.uint8), v0)):
            for src, dst in ((1, 4), (0, 5)):
                assert torch.equal(t[dst, :, :m], t0[src, :, :m])
                assert torch.equal(t[dst, :, m:], t0[dst, :, m:])
            assert torch.equal(t[:4], t0[:4])


# ---------------------------------------------------------------------- per-row decode
@pytest.mark.parametrize("G", [4, 8])
@pytest.mark.parametrize("lens,maxb", [((1, 64, 65, 200), 4), ((1, 64, 33, 0), 1)])
def test_per_row_decode(native, G, lens, maxb):
    """Split-K partitions + merge (maxb 4: 256-token window) and the single-partition direct
    form (maxb 1); a shuffled block table; stale finite codes past each length; a padded row."""
    Hkv, B = 2, len(lens)
    Hq = G * Hkv
    NB = 20
    k8, k16 = _codes(NB, Hkv, BS, D, seed=2)
    v8, v16 = _codes(NB, Hkv, BS, D, seed=3)
    rnd = random.Random(5)
    bt = torch.tensor(rnd.sample(range(NB), B * maxb), dtype=torch.int32, device="cuda").view(B, maxb)
    cl = torch.tensor(lens, dtype=torch.int32, device="cuda")
    q = torch.randn(B, (Hq + 2 * Hkv) * D, device="cuda", dtype=torch.bfloat16)
    scale = 1 / math.sqrt(D)
    out = native.paged_decode(q, k8, v8, bt, cl, Hq, maxb * BS, scale)
    bf = native.paged_decode(q, k16, v16, bt, cl, Hq, maxb * BS, scale)
    live = [i for i, L in enumerate(lens) if L > 0]
    with native.use_reference():
        ref32 = native.paged_decode(q[live], k8, v8, bt[live], cl[live], Hq, maxb * BS, scale)
    e32, e16 = _err(out[live], ref32), _err(out, bf)
    print(f"per-row G={G} lens={lens}: vs fp32 {e32:.3g}, vs bf16 kernel {e16:.3g}")
    assert torch.isfinite(out.float()).all()
    assert e32 < 3e-2, e32
    assert e16 < 2e-2, e16
    for i, L in enumerate(lens):
        if L == 0:
            assert bool((out[i] == 0).all())


# ----------------------------------------------------------------------- paged prefill
@pytest.mark.parametrize("G", [4, 8])
def test_paged_prefill(native, G):
    Hkv = 2
    Hq = G * Hkv
    prefix = [0, 17, 64, 130]
    new = [1, 40, 7, 33]
    B, maxb, NB = 4, 3, 16
    k8, k16 = _codes(NB, Hkv, BS, D, seed=4)
    v8, v16 = _codes(NB, Hkv, BS, D, seed=5)
    rnd = random.Random(6)
    bt = torch.tensor(rnd.sample(range(NB), B * maxb), dtype=torch.int32, device="cuda").view(B, maxb)
    cu = torch.tensor([0, 1, 41, 48, 81], dtype=torch.int32, device="cuda")
    ctx = torch.tensor(prefix, dtype=torch.int32, device="cuda")
    qkv = torch.randn(sum(new), (Hq + 2 * Hkv) * D, device="cuda", dtype=torch.bfloat16)
    scale = 1 / math.sqrt(D)
    out = native.flash_prefill_paged(qkv, cu, max(new), Hq, Hkv, D, scale, k8, v8, bt, ctx)
    bf = native.flash_prefill_paged(qkv, cu, max(new), Hq, Hkv, D, scale, k16, v16, bt, ctx)
    with native.use_reference():
        ref32 = native.flash_prefill_paged(qkv, cu, max(new), Hq, Hkv, D, scale, k8, v8, bt, ctx)
    e32, e16 = _err(out, ref32), _err(out, bf)
    print(f"paged prefill G={G}: vs fp32 {e32:.3g}, vs bf16 kernel {e16:.3g}")
    assert e32 < 3e-2, e32
    assert e16 < 2e-2, e16


# ------------------------------------------------------------------------ grouped wave
def _trie_batch(B, P_blocks, maxb, seed):
    """Block tables with a common prefix of P_blocks and clusters of rows sharing 1-4 more
    blocks (a prefix-cache trie), then unique blocks; context lengths past the prefix.
    (The generator of tests/test_group_decode_gpu.py.)"""
    rnd = random.Random(seed)
    nxt = P_blocks
    prefix = list(range(P_blocks))
    tables, lens = [], []
    while len(tables) < B:
        csize = rnd.choice([1, 1, 2, 3, 5])
        depth = rnd.randint(0, 4)
        shared = list(range(nxt, nxt + depth))
        nxt += depth
        for _ in range(min(csize, B - len(tables))):
            own = list(range(nxt, nxt + maxb - P_blocks - depth))
            nxt += len(own)
            tables.append(prefix + shared + own)
            lens.append(64 * (P_blocks + depth) + rnd.randint(1, 64 * 3))
    return tables, lens, nxt


_WAVE_REF = {}


def _wave_case(native, B, Hkv, seed):
    """Inputs, the fp32 reference on the codes and the bf16 wave kernel on their image --
    computed once per (B, Hkv) and shared by the tile budgets."""
    key = (B, Hkv)
    if key not in _WAVE_REF:
        Hq, Pb, maxb = 4 * Hkv, 3, 12
        tables, lens, nblk = _trie_batch(B, Pb, maxb, seed)
        lens[1] = 0                                         # a padded row
        lens[0] = 64 * Pb + 16                              # ends exactly on a 16-token quarter
        lens[B - 1] = 64 * Pb + 17                          # ... and one token into the next
        k8, k16 = _codes(nblk, Hkv, BS, D, seed=seed + 10)
        v8, v16 = _codes(nblk, Hkv, BS, D, seed=seed + 11)
        bt = torch.tensor(tables, dtype=torch.int32, device="cuda")
        cl = torch.tensor(lens, dtype=torch.int32, device="cuda")
        q = torch.randn(B, (Hq + 2 * Hkv) * D, device="cuda", dtype=torch.bfloat16)
        live = [i for i, L in enumerate(lens) if L > 0]
        with native.use_reference():
            ref32 = native.paged_decode(q[live], k8, v8, bt[live], cl[live], Hq, maxb * BS, 1 / math.sqrt(D))
        _WAVE_REF[key] = (tables, lens, k8, v8, k16, v16, bt, cl, q, live, ref32)
    return _WAVE_REF[key]


@pytest.mark.parametrize("B,Hkv,seed", [(5, 2, 2), (5, 8, 3), (37, 2, 1), (37, 8, 0)])
@pytest.mark.parametrize("tiles", [1, 3, 1000])
def test_grouped_wave(native, B, Hkv, seed, tiles):
    """Split plans from block 0 (inline prefix) on the FP8 wave kernel: groups split over
    several items and merged by ticket and by the merge kernel, unsplit groups, lengths
    crossing 16-token quarters, a padded row."""
    Hq, Pb, maxb = 4 * Hkv, 3, 12
    tables, lens, k8, v8, k16, v16, bt, cl, q, live, ref32 = _wave_case(native, B, Hkv, seed)
    scale = 1 / math.sqrt(D)
    end_lens = [min(max(L, 1) + 128, maxb * BS) for L in lens]
    quads = native.pack_decode_groups(tables, end_lens, Pb, BS, (B + 1) // 2)
    plan = native.split_decode_groups(quads, tables, end_lens, 0, BS, max(B, 16), tiles).cuda()
    if tiles == 1:
        assert (plan[1, :, 5] > 1).any()   # some group really is split
    pt = torch.zeros(maxb, dtype=torch.int32, device="cuda")
    plen = torch.zeros(1, dtype=torch.int32, device="cuda")
    tick = torch.zeros(plan.shape[1] * Hkv, dtype=torch.int32, device="cuda")
    bf = native.paged_decode_cascade_grouped(q, k16, v16, bt, cl, Hq, scale, pt, plen, 4, plan, False, tick, True)
    merged = native.paged_decode_cascade_grouped(q, k8, v8, bt, cl, Hq, scale, pt, plen, 4, plan, False, None, True)
    for _ in range(2):                      # ticket merge, re-armed after every launch
        out = native.paged_decode_cascade_grouped(q, k8, v8, bt, cl, Hq, scale, pt, plen, 4, plan, False, tick, True)
        torch.cuda.synchronize()
        assert int(tick.abs().sum()) == 0
        e32, e16 = _err(out[live], ref32), _err(out, bf)
        print(f"wave B={B} Hkv={Hkv} tiles={tiles}: vs fp32 {e32:.3g}, vs bf16 kernel {e16:.3g}")
        assert torch.isfinite(out.float()).all()
        assert e32 < 3e-2, e32
        assert e16 < 2e-2, e16
        assert bool((out[1] == 0).all())    # the padded row
    assert _err(merged[live], ref32) < 3e-2 and _err(merged, bf) < 2e-2
    assert bool((merged[1] == 0).all())


# ------------------------------------------------------------- unsupported entry points
def test_unsupported_entry_points_raise(native):
    """A native entry point handed an FP8 cache it does not implement fails its dtype check
    (it never reinterprets the bytes), and the routing predicates say so up front."""
    Hkv, Hq, B, maxb = 2, 8, 4, 4
    k8, _ = _codes(8, Hkv, BS, D, seed=7)
    v8, k16 = _codes(8, Hkv, BS, D, seed=8)
    bt = torch.arange(B * maxb, dtype=torch.int32, device="cuda").view(B, maxb) % 8
    cl = torch.tensor([70, 80, 90, 100], dtype=torch.int32, device="cuda")
    q = torch.randn(B, (Hq + 2 * Hkv) * D, device="cuda", dtype=torch.bfloat16)
    pt, plen = bt[0].clone(), torch.tensor([64], dtype=torch.int32, device="cuda")
    scale = 1 / math.sqrt(D)
    with pytest.raises(RuntimeError):
        native.paged_decode_cascade(q, k8, v8, bt, cl, Hq, maxb * BS, scale, pt, plen, 4)
    groups = torch.tensor([0, 1, 2, 3], dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError):
        native.paged_decode_cascade_grouped(q, k8, v8, bt, cl, Hq, scale, pt, plen, 4, groups)
    plan = native.split_decode_groups([[0, 1, 2, 3]], bt.tolist(), [200] * 4, 1, BS, 4, 12).cuda()
    with pytest.raises(RuntimeError):        # a split plan behind a prefix kernel: bf16 only
        native.paged_decode_cascade_grouped(q, k8, v8, bt, cl, Hq, scale, pt, plen, 4, plan)
    with pytest.raises(RuntimeError):        # mixed pair
        native.paged_decode(q, k8, k16, bt, cl, Hq, maxb * BS, scale)
    assert not native.cascade_ok(k8, bt, Hq) and not native.fused_decode_ok(k8, bt)
    assert native.cascade_ok(k16, bt, Hq) and native.fused_decode_ok(k16, bt)
    assert native.grouped_decode_ok(k8, bt, Hq)


def test_engine_rejects_unsupported_shapes(native):
    from docqa_amd.engine.llm_engine import LLMEngine
    from docqa_amd.models.llama import LlamaConfig, LlamaModel

    m = LlamaModel(LlamaConfig.preset("tiny"), device="cuda", seed=1)      # 4 / 2 heads: G = 2
    with pytest.raises(ValueError):
        LLMEngine(m, max_batch=2, max_context=128, use_graphs=False, kv_dtype="fp8")
    LLMEngine(m, max_batch=2, max_context=128, use_graphs=False, kv_dtype="bf16")


# ------------------------------------------------------------------------------- model
def test_model_prefill_and_decode_vs_reference(native):
    """llama3-1b-test with an FP8 cache: one prefill and one decode step, native kernels
    against the reference ops, at the bound tests/test_models_gpu.py sets for the same
    comparison in bf16 (0.03 of the largest logit)."""
    from tests.test_models_gpu import _decode_logits, _prefill_logits, _rel

    from docqa_amd.engine.kv_cache import KVCache
    from docqa_amd.models.llama import LlamaConfig, LlamaModel

    m = LlamaModel(LlamaConfig.preset("llama3-1b-test"), device="cuda")
    g = torch.Generator().manual_seed(1)
    prompts = [torch.randint(0, 32000, (n,), generator=g).tolist() for n in (9, 130, 300)]
    nxt = [5, 6, 7]
    kv1 = KVCache(m.cfg.layers, 64, m.hkv, m.cfg.head_dim, BS, dtype=FP8).caches
    kv2 = KVCache(m.cfg.layers, 64, m.hkv, m.cfg.head_dim, BS, dtype=FP8).caches
    p1, tables = _prefill_logits(m, kv1, prompts, BS)
    d1 = _decode_logits(m, kv1, prompts, tables, nxt, BS)
    with native.use_reference():
        p2, _ = _prefill_logits(m, kv2, prompts, BS)
        d2 = _decode_logits(m, kv2, prompts, tables, nxt, BS)
    rp, rd = _rel(p1, p2), _rel(d1, d2)
    print(f"model fp8 kv: prefill rel {rp:.3g}, decode rel {rd:.3g}")
    assert rp < 0.03 and rd < 0.03
    used = kv1[0][0].view(torch.uint8)
    assert bool((used != 0).any()) and not bool(((used == 0x7F) | (used == 0xFF)).any())


# ------------------------------------------------------------------------------ engine
def test_engine_on_nan_garbage_memory_matches_clean():
    """tests/test_kv_garbage_gpu.py with kv_dtype="fp8": the poison is 0x7f bytes, the e4m3
    NaN code."""
    from docqa_amd import ops
    from docqa_amd.engine.llm_engine import LLMEngine, SamplingParams
    from docqa_amd.models.llama import LlamaConfig, LlamaModel

    assert ops.load_native()
    m = LlamaModel(LlamaConfig.preset("llama3-1b-test"), device="cuda", seed=5)
    g = torch.Generator().manual_seed(2)
    prompts = [torch.randint(3, 30000, (n,), generator=g).tolist() for n in (5, 33, 70, 100, 129, 200)]
    params = SamplingParams(max_new_tokens=10, stop_on_eos=False)
    clean = LLMEngine(m, max_batch=8, max_context=512, use_graphs=True, kv_dtype="fp8")
    assert clean.kv.caches[0][0].dtype == FP8
    ref = clean.generate(prompts, params)
    assert all(len(o) == 10 for o in ref)
    nkv = sum(k.numel() + v.numel() for k, v in clean.kv.caches)
    del clean
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    junk = torch.full((4 * nkv,), 0x7F, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    del junk
    eng = LLMEngine(m, max_batch=8, max_context=512, use_graphs=True, kv_dtype="fp8")
    assert all(int(k.view(torch.uint8).max()) == 0 and int(v.view(torch.uint8).max()) == 0 for k, v in eng.kv.caches)
    assert eng.generate(prompts, params) == ref
    second = eng.generate(prompts, params)       # served from the prefix and tail caches (paged prefill, row copy)
    assert eng.stats.cached_tokens > 0 and all(len(o) == 10 for o in second)


def test_engine_routes_large_batches_to_the_wave_kernel(native):
    """From 32 rows an FP8 engine takes the grouped wave kernel with the plan built from block
    0, below that the per-row kernel: same generations up to summation-order near-ties (the
    criterion of tests/test_models_gpu.py::test_grouped_decode_without_common_prefix)."""
    from docqa_amd.engine.llm_engine import LLMEngine, SamplingParams
    from docqa_amd.models.llama import LlamaConfig, LlamaModel

    m = LlamaModel(LlamaConfig.preset("llama3-1b-test"), device="cuda", seed=31)
    g = torch.Generator().manual_seed(8)
    shared = [torch.randint(3, 32000, (int(n),), generator=g).tolist() for n in (70, 150)]
    prompts = []
    for i in range(40):
        head = torch.randint(3, 32000, (5 + i % 7,), generator=g).tolist()
        prompts.append(head + shared[i % 2] + torch.randint(3, 32000, (20 + 3 * i,), generator=g).tolist())
    sp = SamplingParams(max_new_tokens=4, stop_on_eos=False)
    outs = {}
    for flag in (False, True):
        eng = LLMEngine(m, max_batch=64, max_context=512, use_graphs=True, kv_dtype="fp8")
        eng.group_without_prefix = (lambda B, fit=True, f=flag, e=eng, orig=LLMEngine.group_without_prefix:
                                    f and orig(e, B, fit))
        assert LLMEngine.group_without_prefix(eng, 40)
        assert eng._shared_prefix_blocks([[0, 1, 2]] * 8, [192] * 8) == 0     # no shared-prefix kernel
        outs[flag] = eng.generate(prompts, sp)
        assert any(k[2] for k in eng._graphs) == flag
    first = sum(a[1] == b[1] for a, b in zip(outs[False], outs[True]))
    assert first >= 0.9 * len(prompts), first
    assert [o[0] for o in outs[True]] == [o[0] for o in outs[False]]
    assert all(len(o) == 4 for o in outs[True])
