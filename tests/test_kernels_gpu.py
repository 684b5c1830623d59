"""Numerics of every hand-written gfx950 kernel against the fp32 PyTorch reference of the
same op (docqa_amd.ops.reference).  GPU only; the native extension must be loaded (no
silent fallback)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def native():
    from docqa_amd import ops

    assert ops.load_native(build_if_missing=True), "native extension failed to load"
    assert ops.native_loaded()
    torch.manual_seed(0)
    return ops


def _close(a, b, atol, rtol=0.0):
    a, b = a.float(), b.float()
    err = (a - b).abs().max().item()
    tol = atol + rtol * b.abs().max().item()
    assert err <= tol, f"max err {err} > {tol}"


@pytest.mark.parametrize("rows,H", [(1, 4096), (37, 4096), (128, 384), (5, 8192), (64, 768)])
def test_rmsnorm(native, rows, H):
    from docqa_amd.ops import reference as R

    x = torch.randn(rows, H, device="cuda", dtype=torch.bfloat16)
    w = (torch.rand(H, device="cuda") + 0.5).bfloat16()
    _close(native.rmsnorm(x, w, 1e-5), R.rmsnorm(x, w, 1e-5), 2e-2, 1e-2)


def test_add_rmsnorm(native):
    from docqa_amd.ops import reference as R

    x = torch.randn(33, 4096, device="cuda", dtype=torch.bfloat16)
    r = torch.randn(33, 4096, device="cuda", dtype=torch.bfloat16)
    w = (torch.rand(4096, device="cuda") + 0.5).bfloat16()
    r1, r2 = r.clone(), r.clone()
    o1 = native.add_rmsnorm(x, r1, w, 1e-5)
    o2 = R.add_rmsnorm(x, r2, w, 1e-5)
    _close(r1, r2, 1e-2, 1e-2)
    _close(o1, o2, 3e-2, 1e-2)


@pytest.mark.parametrize("H,res", [(384, True), (768, False), (1024, True)])
def test_layernorm(native, H, res):
    from docqa_amd.ops import reference as R

    x = torch.randn(77, H, device="cuda", dtype=torch.bfloat16)
    rr = torch.randn(77, H, device="cuda", dtype=torch.bfloat16) if res else None
    g = torch.randn(H, device="cuda").bfloat16()
    b = torch.randn(H, device="cuda").bfloat16()
    _close(native.layernorm(x, rr, g, b, 1e-12), R.layernorm(x, rr, g, b, 1e-12), 5e-2, 1e-2)


def test_rope_cache(native):
    from docqa_amd.ops import reference as R

    Hq, Hkv, D, BS, T = 8, 2, 128, 16, 50
    cs = R.rope_cos_sin(1024, D, 500000.0, "cuda")
    qkv = torch.randn(T, (Hq + 2 * Hkv) * D, device="cuda", dtype=torch.bfloat16)
    pos = torch.randint(0, 1000, (T,), device="cuda", dtype=torch.int32)
    slots = torch.randperm(8 * BS, device="cuda")[:T].int()
    slots[3] = -1
    kc1 = torch.zeros(8, Hkv, BS, D, device="cuda", dtype=torch.bfloat16)
    vc1 = torch.zeros_like(kc1)
    kc2, vc2 = kc1.clone(), vc1.clone()
    q1, q2 = qkv.clone(), qkv.clone()
    native.rope_cache(q1, pos, cs, slots, kc1, vc1, Hq, Hkv, D)
    R.rope_cache(q2, pos, cs, slots, kc2, vc2, Hq, Hkv, D)
    _close(q1, q2, 2e-2, 1e-2)
    _close(kc1, kc2, 2e-2, 1e-2)
    _close(vc1, vc2, 0.0)


def test_silu_mul_bias_act(native):
    from docqa_amd.ops import reference as R

    gu = torch.randn(19, 2 * 1536, device="cuda", dtype=torch.bfloat16)
    _close(native.silu_mul(gu), R.silu_mul(gu), 2e-2, 1e-2)
    x = torch.randn(19, 1536, device="cuda", dtype=torch.bfloat16)
    b = torch.randn(1536, device="cuda", dtype=torch.bfloat16)
    r = torch.randn(19, 1536, device="cuda", dtype=torch.bfloat16)
    _close(native.bias_act(x, b, None, True), R.bias_act(x, b, None, True), 2e-2, 1e-2)
    _close(native.bias_act(x, b, r, False), R.bias_act(x, b, r, False), 2e-2, 1e-2)


def test_embedding_and_bert_embed(native):
    from docqa_amd.ops import reference as R

    table = torch.randn(1000, 4096, device="cuda", dtype=torch.bfloat16)
    ids = torch.randint(0, 1000, (45,), device="cuda", dtype=torch.int32)
    _close(native.embedding(ids, table), R.embedding(ids, table), 0.0)
    H = 384
    wte = torch.randn(3000, H, device="cuda", dtype=torch.bfloat16)
    wpe = torch.randn(512, H, device="cuda", dtype=torch.bfloat16)
    wtt = torch.randn(2, H, device="cuda", dtype=torch.bfloat16)
    g = torch.randn(H, device="cuda").bfloat16()
    bb = torch.randn(H, device="cuda").bfloat16()
    ids = torch.randint(0, 3000, (99,), device="cuda", dtype=torch.int32)
    pos = torch.randint(0, 512, (99,), device="cuda", dtype=torch.int32)
    _close(native.bert_embed_ln(ids, pos, None, wte, wpe, wtt, g, bb, 1e-12),
           R.bert_embed_ln(ids, pos, None, wte, wpe, wtt, g, bb, 1e-12), 6e-2, 1e-2)


@pytest.mark.parametrize("T,H", [(1, 4096), (7, 2048), (300, 4096), (3, 8192), (2, 256)])
def test_embed_rmsnorm(native, T, H):
    """Fused Llama input (embedding gather + first RMSNorm) == embedding + rmsnorm, bit for
    bit; out-of-range ids read row 0 like the plain gather."""
    table = torch.randn(1000, H, device="cuda", dtype=torch.bfloat16)
    w = (torch.rand(H, device="cuda") + 0.5).bfloat16()
    ids = torch.randint(0, 1000, (T,), device="cuda", dtype=torch.int32)
    ids[0] = 5000 if T > 1 else ids[0]
    h, x = torch.ops.docqa.embed_rmsnorm(ids, table, w, 1e-5)
    h2 = native.embedding(ids, table)
    assert torch.equal(h, h2)
    assert torch.equal(x, native.rmsnorm(h2, w, 1e-5))


@pytest.mark.parametrize("parts", [1, 63, 2004, 4100])
def test_argmax_merge_partials(native, parts):
    """LM-head argmax partial merge (256-thread rounds) picks the best (value, lowest id)."""
    M, K = 3, 512
    N = parts * 64
    x = torch.randn(M, K, device="cuda", dtype=torch.bfloat16)
    w = (torch.randn(N, K, device="cuda") / K ** 0.5).bfloat16()
    ids, vals = torch.ops.docqa.dgemm_argmax_val(x, w, N)
    logits = (x.float() @ w.float().T).bfloat16().float()
    best = logits.max(1).values
    assert torch.equal(vals.cpu(), best.cpu())
    assert torch.equal(logits.gather(1, ids[:, None])[:, 0].cpu(), best.cpu())


@pytest.mark.parametrize("V,dtype", [(128256, torch.bfloat16), (32000, torch.float32), (1000, torch.bfloat16)])
def test_argmax(native, V, dtype):
    x = torch.randn(13, V, device="cuda").to(dtype)
    assert torch.equal(native.argmax(x).cpu(), x.float().argmax(-1).cpu())


@pytest.mark.parametrize("T,H,NL,nv", [(1, 384, 8, 5), (257, 768, 16, 9), (5000, 768, 16, 9),
                                        (64, 1024, 32, 31)])
def test_token_cls_argmax(native, T, H, NL, nv):
    # fused NER head + argmax vs the fp32 reference of the same op; h has a padded row
    # stride like a slice of a wider activation buffer
    g = torch.Generator(device="cuda").manual_seed(T + NL)
    hbuf = torch.randn(T, H + 64, device="cuda", generator=g).bfloat16()
    h = hbuf[:, :H]
    w = torch.zeros(NL, H, device="cuda", dtype=torch.bfloat16)
    w[:nv] = (torch.randn(nv, H, device="cuda", generator=g) * 0.05).bfloat16()
    b = torch.full((NL,), -1e4, device="cuda").bfloat16()
    b[:nv] = (torch.randn(nv, device="cuda", generator=g) * 0.1).bfloat16()
    got = native.token_cls_argmax(h, w, b, nv).cpu()
    logits = (h.float() @ w[:nv].float().t() + b[:nv].float()).cpu()
    want = logits.argmax(-1)
    top2 = logits.topk(2, dim=-1).values
    ambiguous = (top2[:, 0] - top2[:, 1]) < 1e-4
    assert got.shape == (T,) and got.dtype == torch.int64
    assert int(got.max()) < nv
    assert torch.equal(got[~ambiguous], want[~ambiguous])


def test_vector_load_kernels_refuse_misaligned_views(native):
    """uint4-loading launchers reject views whose storage offset breaks 16-byte alignment
     instead of faulting on the GPU."""
    H, NL = 256, 16
    hbuf = torch.randn(8 * (H + 8) + 1, device="cuda").bfloat16()
    h = hbuf[1:1 + 8 * (H + 8)].view(8, H + 8)[:, :H]          # offset of one element
    w = torch.zeros(NL, H, device="cuda", dtype=torch.bfloat16)
    b = torch.zeros(NL, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(RuntimeError):
        native.token_cls_argmax(h, w, b, 4)
    wbuf = torch.zeros(NL * H + 1, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(RuntimeError):
        native.token_cls_argmax(hbuf[:8 * H].view(8, H), wbuf[1:].view(NL, H), b, 4)
    logits = torch.randn(4 * 1024 + 1, device="cuda").bfloat16()[1:].view(4, 1024)
    with pytest.raises(RuntimeError):
        native.argmax(logits)


def test_sample_greedy_limit(native):
    # top_k=1 must reproduce argmax whatever u is
    x = torch.randn(8, 5000, device="cuda")
    it = torch.ones(8, device="cuda")
    tk = torch.ones(8, device="cuda", dtype=torch.int32)
    tp = torch.ones(8, device="cuda")
    u = torch.rand(8, device="cuda")
    assert torch.equal(native.sample(x, it, tk, tp, u).cpu(), x.argmax(-1).cpu())


def test_sample_distribution(native):
    # two-token distribution: frequencies follow softmax
    x = torch.full((4096, 16), -30.0, device="cuda")
    x[:, 3] = 0.0
    x[:, 7] = math.log(3.0)
    it = torch.ones(4096, device="cuda")
    tk = torch.zeros(4096, device="cuda", dtype=torch.int32)
    tp = torch.ones(4096, device="cuda")
    u = torch.rand(4096, device="cuda")
    s = native.sample(x, it, tk, tp, u).cpu()
    frac7 = (s == 7).float().mean().item()
    assert set(s.unique().tolist()) <= {3, 7}
    assert abs(frac7 - 0.75) < 0.04


@pytest.mark.parametrize("G", [1, 4, 8])
@pytest.mark.parametrize("lens", [[1, 17, 300, 1000], [64], [513, 2], [2000], [65] * 24])
def test_paged_decode(native, G, lens):
    from docqa_amd.ops import reference as R

    Hkv, D, BS = 2, 128, 64
    Hq = Hkv * G
    B = len(lens)
    maxb = 32
    nb = B * maxb
    kc = torch.randn(nb, Hkv, BS, D, device="cuda", dtype=torch.bfloat16)
    vc = torch.randn(nb, Hkv, BS, D, device="cuda", dtype=torch.bfloat16)
    bt = torch.randperm(nb, device="cuda").int().view(B, maxb)
    cl = torch.tensor(lens, device="cuda", dtype=torch.int32)
    q = torch.randn(B, (Hq + 2 * Hkv) * D, device="cuda", dtype=torch.bfloat16)
    scale = 1 / math.sqrt(D)
    o1 = native.paged_decode(q, kc, vc, bt, cl, Hq, 2048, scale)
    o2 = R.paged_decode(q, kc, vc, bt, cl, Hq, 2048, scale)
    _close(o1, o2, 2e-2, 1e-2)


def test_paged_decode_single_partition(native):
    """Batch 64 x 8 KV heads fills the chip with one partition per sequence: the kernel
    writes the normalised output directly (no merge launch)."""
    from docqa_amd.ops import reference as R

    B, Hkv, G, D, BS = 64, 8, 4, 128, 64
    Hq = Hkv * G
    lens = torch.randint(1, 700, (B,)).tolist()
    maxb = 12
    kc = torch.randn(B * maxb, Hkv, BS, D, device="cuda", dtype=torch.bfloat16)
    vc = torch.randn_like(kc)
    bt = torch.randperm(B * maxb, device="cuda").int().view(B, maxb)
    cl = torch.tensor(lens, device="cuda", dtype=torch.int32)
    q = torch.randn(B, (Hq + 2 * Hkv) * D, device="cuda", dtype=torch.bfloat16)
    o1 = native.paged_decode(q, kc, vc, bt, cl, Hq, maxb * BS, 1 / math.sqrt(D))
    o2 = R.paged_decode(q, kc, vc, bt, cl, Hq, maxb * BS, 1 / math.sqrt(D))
    _close(o1, o2, 2e-2, 1e-2)


@pytest.mark.parametrize("D", [128, 64, 32])
@pytest.mark.parametrize("causal", [True, False])
def test_flash_prefill(native, D, causal):
    from docqa_amd.ops import reference as R

    Hq, Hkv = (8, 2) if D == 128 else (6, 6)
    lens = [1, 130, 257, 64, 500]
    cu = torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), device="cuda", dtype=torch.int32)
    T = sum(lens)
    qkv = torch.randn(T, (Hq + 2 * Hkv) * D, device="cuda", dtype=torch.bfloat16)
    scale = 1 / math.sqrt(D)
    o1 = native.flash_prefill(qkv, cu, max(lens), Hq, Hkv, D, scale, causal)
    o2 = R.flash_prefill(qkv, cu, max(lens), Hq, Hkv, D, scale, causal)
    _close(o1, o2, 3e-2, 1e-2)


@pytest.mark.parametrize("Hq,Hkv", [(16, 2), (8, 1)])
@pytest.mark.parametrize("causal", [True, False])
def test_flash_prefill_gqa8(native, Hq, Hkv, causal):
    """8 query heads per KV head (Llama-3-70B and its TP-8 shard): one 8-wave workgroup per
    (32 rows, KV head) sharing every K/V tile -- plain and prefix-cached (paged) prefill."""
    from docqa_amd.ops import reference as R

    D, BS = 128, 64
    lens = [1, 130, 257, 64, 500]
    cu = torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), device="cuda", dtype=torch.int32)
    qkv = torch.randn(sum(lens), (Hq + 2 * Hkv) * D, device="cuda", dtype=torch.bfloat16)
    scale = 1 / math.sqrt(D)
    o1 = native.flash_prefill(qkv, cu, max(lens), Hq, Hkv, D, scale, causal)
    o2 = R.flash_prefill(qkv, cu, max(lens), Hq, Hkv, D, scale, causal)
    _close(o1, o2, 3e-2, 1e-2)
    if causal:
        B, maxb = len(lens), 16
        kc = torch.randn(B * maxb, Hkv, BS, D, device="cuda", dtype=torch.bfloat16)
        vc = torch.randn_like(kc)
        bt = torch.randperm(B * maxb, device="cuda").int().view(B, maxb)
        cs = torch.tensor([0, 64, 320, 128, 448], device="cuda", dtype=torch.int32)
        o1 = native.flash_prefill_paged(qkv, cu, max(lens), Hq, Hkv, D, scale, kc, vc, bt, cs)
        o2 = R.flash_prefill_paged(qkv, cu, max(lens), Hq, Hkv, D, scale, kc, vc, bt, cs)
        _close(o1, o2, 3e-2, 1e-2)


@pytest.mark.parametrize("prefix", [[0, 64, 128, 320], [256, 0, 64, 1000]])
def test_flash_prefill_paged(native, prefix):
    """Prefix-cached prefill: keys = cached prefix + new tokens, read via block tables."""
    from docqa_amd.ops import reference as R

    Hq, Hkv, D, BS = 8, 2, 128, 64
    new = [5, 130, 64, 200]
    B = len(new)
    maxb = 32
    kc = torch.randn(B * maxb, Hkv, BS, D, device="cuda", dtype=torch.bfloat16)
    vc = torch.randn(B * maxb, Hkv, BS, D, device="cuda", dtype=torch.bfloat16)
    bt = torch.randperm(B * maxb, device="cuda").int().view(B, maxb)
    cu = torch.tensor([0] + list(torch.tensor(new).cumsum(0)), device="cuda", dtype=torch.int32)
    qkv = torch.randn(sum(new), (Hq + 2 * Hkv) * D, device="cuda", dtype=torch.bfloat16)
    cs = torch.tensor(prefix, device="cuda", dtype=torch.int32)
    o1 = native.flash_prefill_paged(qkv, cu, max(new), Hq, Hkv, D, 1 / math.sqrt(D), kc, vc, bt, cs)
    o2 = R.flash_prefill_paged(qkv, cu, max(new), Hq, Hkv, D, 1 / math.sqrt(D), kc, vc, bt, cs)
    _close(o1, o2, 3e-2, 1e-2)


@pytest.mark.parametrize("M,N,K", [(1, 128, 64), (77, 384, 384), (300, 1536, 384), (1000, 384, 1536),
                                   (2048, 3072, 768), (129, 1152, 384)])
@pytest.mark.parametrize("epi", [0, 1, 2, 3])
def test_gemm_fused(native, M, N, K, epi):
    from docqa_amd.ops import reference as R

    a = torch.randn(M, K, device="cuda", dtype=torch.bfloat16)
    w = (torch.randn(N, K, device="cuda") / K ** 0.5).bfloat16()
    b = torch.randn(N, device="cuda", dtype=torch.bfloat16)
    r = torch.randn(M, N, device="cuda", dtype=torch.bfloat16)
    bias = b if epi else None
    res = r if epi == 3 else None
    o1 = torch.ops.docqa.gemm(a, w, bias, res, epi)
    o2 = R.linear_fused(a, w, bias, res, epi)
    _close(o1, o2, 3e-2, 1e-2)


def test_gemm_asymmetric_identity(native):
    """A = I with an asymmetric W catches a transposed C write (guide §3)."""
    n = 128
    a = torch.eye(n, device="cuda", dtype=torch.bfloat16)
    w = (torch.arange(n * 64, device="cuda").view(n, 64) % 97).bfloat16()
    a64 = torch.zeros(n, 64, device="cuda", dtype=torch.bfloat16)
    a64[:, :64] = a[:, :64]
    o = torch.ops.docqa.gemm(a64, w, None, None, 0).float()
    assert torch.equal(o[:64, :], w.float()[:, :64].T[:64, :])


@pytest.mark.parametrize("M", [1, 5, 16, 31, 64, 65, 100, 128, 129, 192, 193, 230, 256])
@pytest.mark.parametrize("N,K,S", [(6144, 4096, 0), (4096, 4096, 0), (4096, 14336, 0), (28672, 4096, 0),
                                   (512, 1024, 1), (512, 1024, 2), (640, 3584, 7)])
def test_dgemm(native, M, N, K, S):
    """Skinny decode projection (split-K / direct) vs the fp32 reference."""
    x = torch.randn(M, K, device="cuda", dtype=torch.bfloat16)
    w = (torch.randn(N, K, device="cuda") / K ** 0.5).bfloat16()
    o2 = (x.float() @ w.float().T)
    for _ in range(3):   # a ring-pipeline race shows up intermittently, not on every call
        o1 = torch.ops.docqa.dgemm(x, w, S)
        _close(o1, o2, 2e-2, 1e-2)


@pytest.mark.parametrize("S,M,tile", [(1, 37, 64), (4, 37, 64), (4, 100, 128), (8, 128, 128), (2, 128, 64),
                                     (4, 160, 64), (4, 192, 64), (4, 256, 64), (2, 200, 64), (8, 256, 128),
                                     (4, 241, 128)])
def test_splitk_fused_consumers(native, S, M, tile):
    """dgemm_partial + add_rmsnorm_splitk / rope_cache_splitk == reference on bf16(sum P)."""
    from docqa_amd.ops import reference as R

    H = 4096
    x = torch.randn(M, 4096, device="cuda", dtype=torch.bfloat16)
    w = (torch.randn(H, 4096, device="cuda") / 64).bfloat16()
    P = torch.ops.docqa.dgemm_partial(x, w, S, tile)
    assert P.shape == (S, M, H)
    _close(P.sum(0), x.float() @ w.float().T, 2e-2, 1e-2)
    r1 = torch.randn(M, H, device="cuda", dtype=torch.bfloat16)
    r2 = r1.clone()
    g = (torch.rand(H, device="cuda") + 0.5).bfloat16()
    o1 = torch.ops.docqa.add_rmsnorm_splitk(P, r1, g, 1e-5)
    o2 = R.add_rmsnorm(P.sum(0).bfloat16(), r2, g, 1e-5)
    _close(r1, r2, 1e-2, 1e-2)
    _close(o1, o2, 3e-2, 1e-2)
    # packed QKV: 8 q + 2 k + 2 v heads of 128
    Hq, Hkv, D, BS, T = 8, 2, 128, 16, M
    Pq = torch.randn(S, T, (Hq + 2 * Hkv) * D, device="cuda")
    cs = R.rope_cos_sin(1024, D, 500000.0, "cuda")
    pos = torch.randint(0, 1000, (T,), device="cuda", dtype=torch.int32)
    nblk = max(8, (T + BS - 1) // BS + 1)
    slots = torch.randperm(nblk * BS, device="cuda")[:T].int()
    slots[3] = -1
    kc1 = torch.zeros(nblk, Hkv, BS, D, device="cuda", dtype=torch.bfloat16)
    vc1 = torch.zeros_like(kc1)
    kc2, vc2 = kc1.clone(), vc1.clone()
    q1 = torch.ops.docqa.rope_cache_splitk(Pq, pos, cs, slots, kc1, vc1, Hq, Hkv, D)
    q2 = Pq.sum(0).bfloat16()
    R.rope_cache(q2, pos, cs, slots, kc2, vc2, Hq, Hkv, D)
    _close(q1, q2, 2e-2, 1e-2)
    _close(kc1, kc2, 2e-2, 1e-2)
    _close(vc1, vc2, 1e-2)


@pytest.mark.parametrize("S", [1, 3, 5, 8, 9, 12])
def test_splitk_consumers_slab_counts(native, S):
    """The consumers' compile-time slab counts (1..8) and the runtime-S fallback (>8)."""
    from docqa_amd.ops import reference as R

    M, H = 70, 4096
    P = torch.randn(S, M, H, device="cuda") / S
    r1 = torch.randn(M, H, device="cuda", dtype=torch.bfloat16)
    r2 = r1.clone()
    g = (torch.rand(H, device="cuda") + 0.5).bfloat16()
    o1 = torch.ops.docqa.add_rmsnorm_splitk(P, r1, g, 1e-5)
    o2 = R.add_rmsnorm(P.sum(0).bfloat16(), r2, g, 1e-5)
    _close(r1, r2, 1e-2, 1e-2)
    _close(o1, o2, 3e-2, 1e-2)
    Hq, Hkv, D, BS, T = 32, 8, 128, 16, M
    Pq = torch.randn(S, T, (Hq + 2 * Hkv) * D, device="cuda")
    cs = R.rope_cos_sin(1024, D, 500000.0, "cuda")
    pos = torch.randint(0, 1000, (T,), device="cuda", dtype=torch.int32)
    slots = torch.randperm(8 * BS, device="cuda")[:T].int()
    slots[5] = -1
    kc1 = torch.zeros(8, Hkv, BS, D, device="cuda", dtype=torch.bfloat16)
    vc1 = torch.zeros_like(kc1)
    kc2, vc2 = kc1.clone(), vc1.clone()
    q1 = torch.ops.docqa.rope_cache_splitk(Pq, pos, cs, slots, kc1, vc1, Hq, Hkv, D)
    q2 = Pq.sum(0).bfloat16()
    R.rope_cache(q2, pos, cs, slots, kc2, vc2, Hq, Hkv, D)
    _close(q1, q2, 2e-2, 1e-2)
    _close(kc1, kc2, 2e-2, 1e-2)
    _close(vc1, vc2, 2e-2, 1e-2)   # fp32 sum order differs from torch's -> 1 bf16 ulp


@pytest.mark.parametrize("M", [1, 16, 33, 64, 97, 128, 129, 200, 256])
@pytest.mark.parametrize("N,K", [(28672, 4096), (1024, 512)])
def test_dgemm_glu(native, M, N, K):
    """Fused SwiGLU decode GEMM (8-interleaved gate|up) vs fp32 GEMM + reference SwiGLU."""
    from docqa_amd.ops import reference as R

    x = torch.randn(M, K, device="cuda", dtype=torch.bfloat16)
    w = (torch.randn(N, K, device="cuda") / K ** 0.5).bfloat16()
    ref = R.silu_mul((x.float() @ w.float().T).bfloat16(), interleaved=True)
    for _ in range(3):
        _close(torch.ops.docqa.dgemm_glu(x, w), ref, 2e-2, 1e-2)
    # interleaved silu_mul kernel (prefill path) on the same GEMM output
    gu = (x.float() @ w.float().T).bfloat16()
    _close(native.silu_mul(gu, interleaved=True), R.silu_mul(gu, interleaved=True), 2e-2, 1e-2)


@pytest.mark.parametrize("B,Hkv,S", [(64, 8, 2), (5, 8, 1), (3, 2, 4), (128, 8, 4)])
def test_paged_decode_fused(native, B, Hkv, S):
    """RoPE + new-token cache write + attention from QKV split-K partials == the unfused
    rope_cache_splitk + paged_decode (outputs and cache contents)."""
    from docqa_amd.ops import reference as R

    G, D, BS, maxb = 4, 128, 64, 16
    Hq = G * Hkv
    W = (Hq + 2 * Hkv) * D
    P = torch.randn(S, B, W, device="cuda") * 0.5
    pos = torch.randint(0, maxb * BS - 1, (B,), device="cuda", dtype=torch.int32)
    bt = torch.randperm(B * maxb, device="cuda").int().view(B, maxb)
    slots = (bt.gather(1, (pos // BS).long()[:, None])[:, 0] * BS + pos % BS).int()
    slots[B // 2] = -1 if B > 2 else slots[B // 2]
    cl = pos + 1
    kc1 = torch.randn(B * maxb, Hkv, BS, D, device="cuda", dtype=torch.bfloat16)
    vc1 = torch.randn_like(kc1)
    kc2, vc2 = kc1.clone(), vc1.clone()
    cs = R.rope_cos_sin(maxb * BS, D, 500000.0, "cuda")
    scale = 1 / math.sqrt(D)
    o1 = native.paged_decode_fused(P, pos, cs, slots, kc1, vc1, bt, cl, Hq, maxb * BS, scale)
    qkv = native.rope_cache_splitk(P, pos, cs, slots, kc2, vc2, Hq, Hkv, D)
    o2 = native.paged_decode(qkv, kc2, vc2, bt, cl, Hq, maxb * BS, scale)
    _close(kc1, kc2, 0.0)
    _close(vc1, vc2, 0.0)
    # a slot of -1 marks a padded batch row: the unfused path then attends to the stale
    # cache row, the fused one to the computed token -- only valid rows are compared
    valid = slots >= 0
    _close(o1[valid], o2[valid], 2e-2, 1e-2)


@pytest.mark.parametrize("B,S,max_context", [(1, 2, 2048), (1, 4, 8192), (3, 1, 1024), (64, 2, 2048)])
def test_paged_decode_fused_last_merge(native, B, S, max_context):
    """In-kernel last-arriver partition merge (tick buffer) == the separate reduce launch (to
    bf16 rounding), over repeated launches (the kernel re-arms its tickets), a padded row
    (context 0) included; and both == the fp32 reference attention."""
    from docqa_amd.ops import reference as R

    G, Hkv, D, BS = 4, 8, 128, 64
    maxb = max_context // BS
    Hq = G * Hkv
    W = (Hq + 2 * Hkv) * D
    torch.manual_seed(B * 7 + S)
    P = torch.randn(S, B, W, device="cuda") * 0.5
    pos = torch.randint(0, max_context - 1, (B,), device="cuda", dtype=torch.int32)
    pos[0] = min(830, max_context - 2)                  # the batch-1 bench's context length
    bt = torch.randperm(B * maxb, device="cuda").int().view(B, maxb)
    slots = (bt.gather(1, (pos // BS).long()[:, None])[:, 0] * BS + pos % BS).int()
    cl = pos + 1
    if B > 2:
        cl[B // 2] = 0                                  # padded decode slot
        slots[B // 2] = -1
    kc = torch.randn(B * maxb, Hkv, BS, D, device="cuda", dtype=torch.bfloat16)
    vc = torch.randn_like(kc)
    cs = R.rope_cos_sin(max_context, D, 500000.0, "cuda")
    scale = 1 / math.sqrt(D)
    tick = torch.zeros(B * Hkv, device="cuda", dtype=torch.int32)
    kc0, vc0 = kc.clone(), vc.clone()
    base = native.paged_decode_fused(P, pos, cs, slots, kc0, vc0, bt, cl, Hq, max_context, scale)
    for _ in range(3):
        kc1, vc1 = kc.clone(), vc.clone()
        o = native.paged_decode_fused(P, pos, cs, slots, kc1, vc1, bt, cl, Hq, max_context, scale, None, tick)
        torch.cuda.synchronize()
        # same arithmetic as the reduce launch; the two kernel instantiations may contract a
        # multiply-add differently, so allow bf16 rounding-level differences only
        d = (o.float() - base.float()).abs().max().item()
        print(f"last-merge vs reduce max |diff| {d:.3g}, bit-equal {torch.equal(o, base)}")
        _close(o, base, 8e-3, 8e-3)
        assert int(tick.abs().sum()) == 0
        assert torch.equal(kc1, kc0) and torch.equal(vc1, vc0)
    ref = R.paged_decode(native.rope_cache_splitk(P, pos, cs, slots, kc.clone(), vc.clone(), Hq, Hkv, D).float(),
                         kc0.float(), vc0.float(), bt, cl, Hq, max_context, scale)
    valid = cl > 0
    _close(base[valid], ref.to(base.dtype)[valid], 2e-2, 1e-2)
    if B > 2:
        assert int(base[B // 2].abs().sum()) == 0


@pytest.mark.parametrize("M", [1, 2, 4])
@pytest.mark.parametrize("N,K,S", [(4096, 4096, 4), (4096, 14336, 4), (8192, 1024, 2), (1024, 2048, 1)])
def test_dgemm_add_rmsnorm_fused(native, M, N, K, S):
    """Projection + residual add + RMSNorm in one launch (last-workgroup epilogue) == the
    split-K projection + add_rmsnorm_splitk, bit for bit (outputs and residual), over
    repeated launches with one ticket word (re-armed by the kernel); and == fp32 reference."""
    from docqa_amd.ops import reference as R

    x = torch.randn(M, K, device="cuda", dtype=torch.bfloat16)
    w = (torch.randn(N, K, device="cuda") / K ** 0.5).bfloat16()
    g = (1 + 0.1 * torch.randn(N, device="cuda")).bfloat16()
    r0 = torch.randn(M, N, device="cuda", dtype=torch.bfloat16)
    r_ref = r0.clone()
    o_ref = native.add_rmsnorm_splitk(native.dgemm_partial(x, w, S, 64), r_ref, g, 1e-5)
    tick = torch.zeros(1, device="cuda", dtype=torch.int32)
    for _ in range(3):
        r = r0.clone()
        o = native.dgemm_add_rmsnorm(x, w, S, r, g, 1e-5, tick)
        torch.cuda.synchronize()
        assert torch.equal(o, o_ref) and torch.equal(r, r_ref)
        assert int(tick.item()) == 0
    r32 = r0.clone()
    o32 = R.add_rmsnorm((x.float() @ w.float().T).bfloat16(), r32, g, 1e-5)
    _close(o, o32, 3e-2, 3e-2)


@pytest.mark.parametrize("K,N,Sin,S", [(4096, 6144, 4, 2), (4096, 28672, 4, 0), (2048, 1024, 2, 1),
                                       (1024, 4096, 1, 0), (4096, 4096, 3, 4)])
def test_dgemm_xn_input_row(native, K, N, Sin, S):
    """Batch-1 projection building its own input row (XNormIn: residual add + RMSNorm of the
    previous projection's slabs in LDS) == add_rmsnorm_splitk + the plain projection, bit for
    bit -- split-K slabs (S > 0) or fused SwiGLU (S == 0); res_out == the updated residual,
    res_in untouched."""
    Pin = torch.randn(Sin, 1, K, device="cuda")
    r0 = torch.randn(1, K, device="cuda", dtype=torch.bfloat16)
    gam = (1 + 0.1 * torch.randn(K, device="cuda")).bfloat16()
    w = (torch.randn(N, K, device="cuda") / K ** 0.5).bfloat16()
    r_ref = r0.clone()
    x = native.add_rmsnorm_splitk(Pin, r_ref, gam, 1e-5)
    ref = native.dgemm_partial(x, w, S, 64) if S else torch.ops.docqa.dgemm_glu(x, w)
    for _ in range(2):
        r_in, r_out = r0.clone(), torch.empty_like(r0)
        if S:
            got = native.dgemm_partial_xn(Pin, r_in, r_out, gam, 1e-5, w, S)
        else:
            got = native.dgemm_glu_xn(Pin, r_in, r_out, gam, 1e-5, w)
        torch.cuda.synchronize()
        assert torch.equal(r_in, r0) and torch.equal(r_out, r_ref)
        assert torch.equal(got, ref), (got.float() - ref.float()).abs().max().item()


@pytest.mark.parametrize("M", [48, 256])
def test_dgemm_asymmetric_identity(native, M):
    """X = I rows against an asymmetric W: Y must be W's columns, catches transposed writes
    (M=256: the 8-wave layout, every wave's rows distinct)."""
    N, K = 128, 1024
    x = torch.zeros(M, K, device="cuda", dtype=torch.bfloat16)
    x[torch.arange(M), torch.arange(M) * 3] = 1
    w = (torch.arange(N * K, device="cuda").view(N, K) % 97).bfloat16()
    for S in (1, 0):
        o = torch.ops.docqa.dgemm(x, w, S).float()
        assert torch.equal(o, w.float()[:, torch.arange(M, device="cuda") * 3].T)


def test_flash_prefill_spike(native):
    """Force the online-softmax rescale branch: one huge key late in the sequence."""
    from docqa_amd.ops import reference as R

    Hq, Hkv, D, L = 2, 1, 128, 300
    qkv = torch.randn(L, (Hq + 2 * Hkv) * D, device="cuda", dtype=torch.bfloat16) * 0.5
    x = qkv.view(L, Hq + 2 * Hkv, D)
    x[200, Hq] = x[250, 0] * 4  # key 200 aligned with query 250
    cu = torch.tensor([0, L], device="cuda", dtype=torch.int32)
    o1 = native.flash_prefill(qkv, cu, L, Hq, Hkv, D, 1 / math.sqrt(D), True)
    o2 = R.flash_prefill(qkv, cu, L, Hq, Hkv, D, 1 / math.sqrt(D), True)
    _close(o1, o2, 3e-2, 1e-2)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("N,d,nq,k", [(649, 384, 1, 3), (5000, 384, 40, 10), (100000, 768, 7, 32), (10, 128, 3, 16),
                                      (20000, 768, 33, 64), (1024, 768, 256, 40)])
@pytest.mark.parametrize("ip", [False, True])
def test_knn(native, dtype, N, d, nq, k, ip):
    from docqa_amd.ops import reference as R

    xb = torch.randn(N, d, device="cuda")
    xb = torch.nn.functional.normalize(xb, dim=1).to(dtype)
    norms = (xb.float() ** 2).sum(1)
    xq = torch.nn.functional.normalize(torch.randn(nq, d, device="cuda"), dim=1)
    D1, I1 = native.knn(xb, norms, xq, k, ip, 0)
    D2, I2 = R.knn(xb, norms, xq, k, ip, 0)
    kk = min(k, N)
    _close(D1[:, :kk], D2[:, :kk], 1e-4 if dtype == torch.float32 else 1e-2)
    if dtype == torch.float32:
        # exact fp32: ids agree except at near-ties
        agree = (I1[:, :kk] == I2[:, :kk]).float().mean().item()
        assert agree > 0.98
    if k > N:
        assert (I1[:, N:] == -1).all()


def test_knn_self_query_shipped_index(native):
    """Self-queries against the reference's shipped 649x384 index return themselves at ~0."""
    from docqa_amd.index.faiss_io import read_index
    from tests.helpers import REFERENCE_FAISS

    idx = read_index(REFERENCE_FAISS)
    xb = torch.from_numpy(idx.xb).cuda()
    norms = (xb ** 2).sum(1)
    D, I = native.knn(xb, norms, xb[:64].clone(), 1, False, 0)
    assert (D[:, 0].abs() < 1e-4).all()


@pytest.mark.parametrize("mean", [True, False])
def test_pool_l2(native, mean):
    from docqa_amd.ops import reference as R

    lens = [1, 7, 256, 33]
    cu = torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), device="cuda", dtype=torch.int32)
    h = torch.randn(sum(lens), 768, device="cuda", dtype=torch.bfloat16)
    _close(native.pool_l2(h, cu, mean, True), R.pool_l2(h, cu, mean, True), 1e-4)


@pytest.mark.parametrize("B", [37, 256])
def test_paged_decode_cascade_rope_matches_unfused(native, B):
    """Fused RoPE + new-token cache write inside the cascade kernels == rope_cache followed
    by the cascade decode (outputs and the written cache rows; a padded row stays zero)."""
    Hkv, G, D, BS, maxb, Lp = 8, 4, 128, 64, 16, 192
    Hq = G * Hkv
    npb = Lp // BS
    NB = npb + B * (maxb - npb) + 1
    kc = torch.randn(NB, Hkv, BS, D, device="cuda", dtype=torch.bfloat16)
    vc = torch.randn_like(kc)
    bt = torch.zeros(B, maxb, dtype=torch.int32, device="cuda")
    bt[:, :npb] = torch.arange(npb, dtype=torch.int32, device="cuda")
    bt[:, npb:] = (npb + torch.arange(B * (maxb - npb), dtype=torch.int32, device="cuda")).view(B, -1)
    cl = (Lp + 1 + torch.randint(0, maxb * BS - Lp - 1, (B,), device="cuda")).int()
    pos = cl - 1
    slots = (torch.gather(bt, 1, (pos // BS).long()[:, None])[:, 0] * BS + pos % BS).int()
    cl[3], slots[3] = 0, -1                                   # padded row
    qkv = (torch.randn(B, (Hq + 2 * Hkv) * D, device="cuda") * 0.5).bfloat16()
    from docqa_amd.ops import reference as R
    cs = R.rope_cos_sin(4096, D, 500000.0, "cuda")
    st = torch.arange(maxb, dtype=torch.int32, device="cuda")
    pl = torch.tensor([Lp], dtype=torch.int32, device="cuda")
    scale = 1 / math.sqrt(D)
    q1, kc1, vc1 = qkv.clone(), kc.clone(), vc.clone()
    native.rope_cache(q1, pos, cs, slots, kc1, vc1, Hq, Hkv, D)
    o1 = torch.ops.docqa.paged_decode_cascade(q1, kc1, vc1, bt, cl, Hq, maxb * BS, scale, st, pl, 3)
    q2, kc2, vc2 = qkv.clone(), kc.clone(), vc.clone()
    o2 = torch.ops.docqa.paged_decode_cascade_rope(q2, pos, cs, slots, kc2, vc2, bt, cl, Hq, maxb * BS,
                                                   scale, st, pl, 3)
    _close(o2, o1, 2e-2, 1e-2)
    _close(kc2, kc1, 2e-2, 1e-2)
    _close(vc2, vc1, 0.0)
    assert o2[3].abs().max().item() == 0


@pytest.mark.parametrize("B,Lp,nchunk", [(5, 448, 4), (64, 448, 16), (128, 448, 16), (128, 960, 8),
                                         (200, 192, 1), (64, 0, 8)])
def test_paged_decode_cascade(native, B, Lp, nchunk):
    """Shared-prefix (cascade) decode attention == plain paged decode over the same tables:
    MFMA prefix partials in key chunks + ring suffix kernel + LSE merge, in the direct
    (one partition) and the split (merge kernel) regimes."""
    from docqa_amd.ops import reference as R

    Hkv, G, D, BS, maxb = 8, 4, 128, 64, 40
    Hq = G * Hkv
    npb = Lp // BS
    NB = npb + B * (maxb - npb) + 1
    kc = torch.randn(NB, Hkv, BS, D, device="cuda", dtype=torch.bfloat16)
    vc = torch.randn_like(kc)
    shared = torch.randperm(NB, device="cuda")[:npb].int()
    rest = torch.tensor([i for i in range(NB) if i not in set(shared.tolist())], device="cuda").int()
    bt = torch.zeros(B, maxb, dtype=torch.int32, device="cuda")
    for b in range(B):
        bt[b, :npb] = shared
        bt[b, npb:] = rest[b * (maxb - npb):(b + 1) * (maxb - npb)]
    cl = (Lp + 1 + torch.randint(0, maxb * BS - Lp - 1, (B,), device="cuda")).int()
    cl[0] = Lp + 1                                   # suffix of exactly the new token
    q = (torch.randn(B, (Hq + 2 * Hkv) * D, device="cuda") * 0.5).bfloat16()
    st = torch.zeros(maxb, dtype=torch.int32, device="cuda")
    st[:npb] = shared
    pl = torch.tensor([Lp], dtype=torch.int32, device="cuda")
    scale = 1 / math.sqrt(D)
    o1 = native.paged_decode_cascade(q, kc, vc, bt, cl, Hq, maxb * BS, scale, st, pl, nchunk)
    o2 = native.paged_decode(q, kc, vc, bt, cl, Hq, maxb * BS, scale)
    _close(o1, o2, 2e-2, 1e-2)
    sel = torch.arange(0, B, max(1, B // 6), device="cuda")
    o3 = R.paged_decode_cascade(q[sel], kc, vc, bt[sel], cl[sel], Hq, maxb * BS, scale, st, pl)
    _close(o1[sel], o3, 2e-2, 1e-2)


@pytest.mark.parametrize("B", [3, 96])
def test_padded_slots_get_defined_outputs(native, B):
    """Padded decode slots (context length 0) produce zero attention output in the split
    (B=3) and direct (B=96) regimes and with cascade; an all-NaN logits row argmaxes to a
    valid id; an out-of-range token id embeds as row 0 -- so a stale slot can never feed
    an out-of-bounds id into the next graph replay."""
    Hkv, G, D, BS, maxb = 8, 4, 128, 64, 8
    Hq = G * Hkv
    kc = torch.randn(B * maxb, Hkv, BS, D, device="cuda", dtype=torch.bfloat16)
    vc = torch.randn_like(kc)
    bt = torch.arange(B * maxb, device="cuda", dtype=torch.int32).view(B, maxb)
    cl = torch.full((B,), 100, device="cuda", dtype=torch.int32)
    cl[1] = 0
    q = torch.randn(B, (Hq + 2 * Hkv) * D, device="cuda").bfloat16()
    for _ in range(2):   # the output buffer may come back from the allocator dirty
        o = native.paged_decode(q, kc, vc, bt, cl, Hq, maxb * BS, 0.1)
        assert torch.isfinite(o.float()).all() and (o[1] == 0).all()
        st = bt[0].clone()
        oc = native.paged_decode_cascade(q, kc, vc, bt, cl, Hq, maxb * BS, 0.1, st,
                                         torch.tensor([64], device="cuda", dtype=torch.int32), 4)
        assert (oc[1] == 0).all()
    lg = torch.randn(2, 1000, device="cuda")
    lg[0] = float("nan")
    assert 0 <= int(native.argmax(lg)[0]) < 1000
    tab = torch.randn(50, 64, device="cuda").bfloat16()
    e = native.embedding(torch.tensor([3, 2 ** 31 - 1, -5], device="cuda", dtype=torch.int32), tab)
    assert torch.equal(e[1], tab[0]) and torch.equal(e[2], tab[0]) and torch.equal(e[0], tab[3])


def test_decode_state_kernels(native):
    """decode_slots / decode_advance (one launch each per decode step) vs the reference."""
    from docqa_amd.ops import reference as R

    B, maxb, BS = 77, 32, 64
    bt = torch.randperm(B * maxb, device="cuda").int().view(B, maxb)
    pos = torch.randint(0, maxb * BS, (B,), device="cuda", dtype=torch.int32)
    valid = (torch.rand(B, device="cuda") > 0.3).int()
    assert torch.equal(torch.ops.docqa.decode_slots(bt, pos, valid, BS), R.decode_slots(bt, pos, valid, BS))
    nxt = torch.randint(0, 128256, (B,), device="cuda", dtype=torch.long)
    st1 = [torch.zeros(B, device="cuda", dtype=torch.long), torch.zeros(B, device="cuda", dtype=torch.int32),
           pos.clone(), pos.clone() + 1]
    st2 = [t.clone() for t in st1]
    torch.ops.docqa.decode_advance(nxt, *st1, valid)
    R.decode_advance(nxt, *st2, valid)
    for a, b in zip(st1, st2):
        assert torch.equal(a, b)


@pytest.mark.parametrize("G", [4, 8])
def test_decode_dispatch_order_is_result_invariant(native, G):
    """An LPT dispatch order (grid row y -> sequence order[y]) changes only scheduling:
    plain (G=4: VALU ring kernel, G=8: MFMA kernel) and cascade decode give the same rows
    with and without it."""
    B, Hkv, D, BS, maxb = 37, 8, 128, 64, 16
    Hq = Hkv * G
    lens = torch.randint(200, maxb * BS, (B,)).int()
    kc = torch.randn(B * maxb + 8, Hkv, BS, D, device="cuda", dtype=torch.bfloat16)
    vc = torch.randn_like(kc)
    bt = (torch.randperm(B * maxb, device="cuda").int() + 8).view(B, maxb)
    bt[:, :3] = torch.arange(3, device="cuda", dtype=torch.int32)     # shared 192-token prefix
    cl = lens.cuda()
    q = torch.randn(B, (Hq + 2 * Hkv) * D, device="cuda", dtype=torch.bfloat16)
    order = torch.argsort(lens, descending=True).int().cuda()
    s = 1 / math.sqrt(D)
    a = torch.ops.docqa.paged_decode(q, kc, vc, bt, cl, Hq, maxb * BS, s)
    b = torch.ops.docqa.paged_decode(q, kc, vc, bt, cl, Hq, maxb * BS, s, order)
    assert torch.equal(a, b)
    if G != 4:
        return
    st = torch.arange(maxb, device="cuda", dtype=torch.int32)
    pl = torch.tensor([192], device="cuda", dtype=torch.int32)
    a = torch.ops.docqa.paged_decode_cascade(q, kc, vc, bt, cl, Hq, maxb * BS, s, st, pl, 3)
    b = torch.ops.docqa.paged_decode_cascade(q, kc, vc, bt, cl, Hq, maxb * BS, s, st, pl, 3, order)
    assert torch.equal(a, b)


def test_kernel_debug_mode_syncs_outside_capture_only(tmp_path):
    """DOCQA_KERNEL_DEBUG=1 (synchronous fault checking per op) runs eager ops and leaves
    HIP-graph capture alone (a sync inside a capture would invalidate it)."""
    import os
    import subprocess
    import sys

    code = """
import torch
from docqa_amd import ops
assert ops.load_native()
x = torch.randn(64, 4096, device='cuda', dtype=torch.bfloat16)
w = (torch.rand(4096, device='cuda') + 0.5).bfloat16()
y = ops.rmsnorm(x, w, 1e-5)
torch.cuda.synchronize()
g = torch.cuda.CUDAGraph()
s = torch.cuda.Stream()
with torch.cuda.stream(s):
    ops.rmsnorm(x, w, 1e-5)
torch.cuda.synchronize()
with torch.cuda.graph(g):
    z = ops.rmsnorm(x, w, 1e-5)
g.replay()
torch.cuda.synchronize()
assert torch.equal(y, z)
print('debug-ok')
"""
    env = dict(os.environ, DOCQA_KERNEL_DEBUG="1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "debug-ok" in r.stdout, r.stderr[-2000:]
