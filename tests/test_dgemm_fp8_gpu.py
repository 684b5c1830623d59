"""2..32-row decode projections over FP8 weights (dgemm.hip dgemm8_kernel) against fp32 on the
dequantized weights W': split-K slabs with rows carrying different scale exponents and pairwise
different X rows, the SwiGLU epilogue, the LM-head argmax with per-row planted winners that
differ from their rivals by the scale only, the shapes the kernel must refuse, and a few-row
decode step of the quantized Llama test preset: eager, graph-captured and through the engine."""
import pytest
import torch

from docqa_amd import ops
from docqa_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

K0 = 1024     # the kernel's K granule: one whole ring turn (4 stages x 256 codes per row)


@pytest.fixture(scope="module")
def native():
    assert ops.load_native(build_if_missing=True)
    assert ops.DGEMM8_K == K0
    return ops


def _wq(N, K, seed):
    """(q, s, W') of random rows whose scales differ: row i is multiplied by 2^(i % 7 - 3), so a
    dropped or mis-indexed scale shows."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    w = (torch.rand(N, K, device="cuda", generator=g) * 2 - 1) / K ** 0.5
    w = w * torch.exp2((torch.arange(N, device="cuda") % 7 - 3).float())[:, None]
    q, s = ops.quantize_fp8_rows(w.to(torch.bfloat16))
    assert s.unique().numel() >= min(N, 7) - 1
    return q, s, ops.dequantize_fp8_rows(q, s, torch.bfloat16)


def _x(M, K, seed=0):
    """Pairwise different random bf16 rows (a row mix-up shows)."""
    g = torch.Generator(device="cuda").manual_seed(100 + seed)
    x = (torch.rand(M, K, device="cuda", generator=g) * 2 - 1).to(torch.bfloat16)
    assert torch.unique(x, dim=0).shape[0] == M
    return x


def _close(a, r, rel=1e-3, abs_=1e-4):
    err, bound = (a - r).abs().max().item(), rel * r.abs().max().item() + abs_
    print(f"max err {err:.3e} bound {bound:.3e}")
    return err <= bound


@pytest.mark.parametrize("K,S", [(K0, 1), (2 * K0, 2)])
@pytest.mark.parametrize("M", [2, 5, 16, 17, 32])
def test_dgemm8_slabs_match_fp32(native, M, K, S):
    N = 128                                    # two 64-row tiles
    x = _x(M, K)
    q, s, wd = _wq(N, K, 1)
    P = torch.ops.docqa.dgemm8_partial(x, q, s, S, 64)
    assert P.shape == (S, M, N) and P.dtype == torch.float32
    r = x.float() @ wd.float().t()
    assert _close(P.sum(0), r)
    # uint8 codes are the same weights
    assert torch.equal(P, torch.ops.docqa.dgemm8_partial(x, q.view(torch.uint8), s, S, 64))
    # and the bf16 kernel on the image W' computes the same products
    assert _close(P.sum(0), ops.dgemm_partial(x, wd, S).sum(0))


def test_dgemm8_real_shape_on_its_plan(native):
    N = K = 4096
    M = 8
    S, t = ops.dgemm8_plan(M, N, K)
    x = _x(M, K, 1)
    q, s, wd = _wq(N, K, 2)
    if S:
        P = ops.dgemm8_partial(x, q, s, S, t)
    else:   # the probe kept this pair on bf16: the kernel itself at decode_plan's split
        S = ops.decode_plan(M, N, K)[0]
        P = torch.ops.docqa.dgemm8_partial(x, q, s, S, 64)
    assert P.shape == (S, M, N)
    assert _close(P.sum(0), x.float() @ wd.float().t())


@pytest.mark.parametrize("M,N", [(2, 128), (17, 128), (32, 128), (2, 112 * 192), (17, 112 * 192), (32, 112 * 192)])
def test_dgemm8_glu_matches_fp32(native, M, N):
    """64-row tiles, and the 112-row (7 n-tile) variant at the fewest tiles that select it, each
    at one and at two m-tiles (separate instantiations)."""
    x = _x(M, K0, 2)
    q, s, wd = _wq(N, K0, 4)
    y = ops.dgemm8_glu(x, q, s)
    r = ref.silu_mul((x.float() @ wd.float().t()).bfloat16(), interleaved=True).float()
    assert y.shape == (M, N // 2) and y.dtype == torch.bfloat16
    assert _close(y.float(), r, 2e-2, 1e-3)


@pytest.mark.parametrize("M", [2, 32])
def test_dgemm8_argmax_matches_bf16_logits(native, M):
    """LM head + greedy pick over FP8 weights == argmax of the bf16-rounded fp32 logits of W'
    over the valid vocabulary, a different winner per X row.  The planted rows are written as
    codes and scales: X row m's winner (row 0's at the last valid id), a rival at a low id with
    the SAME codes and half the scale (the winner wins by its scale only), and a row with twice
    the scale just past n_valid that must be ignored."""
    N, K, n_valid = 4096, K0, 4000
    x = _x(M, K, 3)
    q, s, _ = _wq(N, K, 8)
    q, s = q.clone(), s.clone()
    win = [n_valid - 1] + [1000 + 65 * m for m in range(1, M)]
    rival = [5 + 3 * m for m in range(M)]
    for m in range(M):
        codes = (torch.sign(x.float()[m]) * 64).to(torch.float8_e4m3fn)
        for row, sc in ((win[m], 2.0 ** -8), (rival[m], 2.0 ** -9), (n_valid + m, 2.0 ** -7)):
            q[row] = codes
            s[row] = sc
    wd = ops.dequantize_fp8_rows(q, s, torch.bfloat16)
    logits = (x.float() @ wd[:n_valid].float().t()).bfloat16().float()
    assert logits.argmax(1).tolist() == win
    ids, vals = torch.ops.docqa.dgemm8_argmax_val(x, q, s, n_valid)
    assert ids.dtype == torch.int64 and ids.tolist() == win
    top = logits.max(1).values
    assert ((vals - top).abs() <= 1e-2 * top.abs()).all()
    # ties go to the lowest id: with equal scales every row's rival is picked
    for m in range(M):
        s[rival[m]] = s[win[m]]
    ids2, _ = torch.ops.docqa.dgemm8_argmax_val(x, q, s, n_valid)
    assert ids2.tolist() == rival


def test_dgemm8_refuses_shapes_without_a_kernel(native):
    op = torch.ops.docqa.dgemm8_partial
    q, s, _ = _wq(128, 2 * K0, 3)
    with pytest.raises(RuntimeError, match="dgemm8_partial"):
        op(_x(ops.DGEMM8_MAX_ROWS + 1, 2 * K0), q, s, 1, 64)          # rows
    with pytest.raises(RuntimeError, match="dgemm8_partial"):
        op(_x(4, 2 * K0), q[:96].contiguous(), s[:96].contiguous(), 1, 64)   # N % 64
    with pytest.raises(RuntimeError, match="dgemm8_partial"):
        op(_x(4, 2 * K0), q, s, 3, 64)                                # S does not divide K
    q2, s2, _ = _wq(128, K0 + 128, 3)
    with pytest.raises(RuntimeError, match="dgemm8_partial"):
        op(_x(4, K0 + 128), q2, s2, 1, 64)                            # not whole ring turns
    with pytest.raises(RuntimeError, match="dgemm8_glu"):
        torch.ops.docqa.dgemm8_glu(_x(4, K0 + 128), q2, s2)
    with pytest.raises(RuntimeError, match="dgemm8_argmax_val"):
        torch.ops.docqa.dgemm8_argmax_val(_x(4, 2 * K0), q, s, 129)   # n_valid > N
    with pytest.raises(RuntimeError, match="dgemm8_glu"):
        torch.ops.docqa.dgemm8_glu(_x(4, 2 * K0), q, s[:64].contiguous())   # scale length
    with pytest.raises(RuntimeError, match="dgemm8_argmax_val"):
        torch.ops.docqa.dgemm8_argmax_val(_x(4, 2 * K0), q.view(torch.int8), s, 128)   # code dtype


# ----------------------------------------------------------------------------- model
@pytest.fixture(scope="module")
def qmodel(native):
    from docqa_amd.models.llama import LlamaConfig, LlamaModel

    m = LlamaModel(LlamaConfig.preset("llama3-1b-test"), device="cuda", seed=17)
    m.quantize_fp8()
    return m


def _planned(m, M):
    """(slab projections, gate|up, LM head) of an M-row step of ``m`` that the plans put on the
    FP8 ring kernel."""
    L0 = m.layers[0]
    slabs = [k for k in ("qkv", "o", "down") if ops.dgemm8_plan(M, *L0[k].shape)[0]]
    return slabs, ops.dgemm8_glu_ok(M, *L0["gate_up"].shape), ops.dgemm8_argmax_ok(M, *m.lm_head.shape)


def _spy(monkeypatch, name, calls):
    orig = getattr(ops, name)
    monkeypatch.setattr(ops, name, lambda *a, **k: (calls.append(name), orig(*a, **k))[1])


def _spy_native(monkeypatch, name, calls):
    """Count calls of the torch op ``name`` made through the ops wrappers."""
    real = ops._native()

    class Proxy:
        def __getattr__(self, attr):
            fn = getattr(real, attr)
            if attr != name:
                return fn
            return lambda *a, **k: (calls.append(name), fn(*a, **k))[1]

    monkeypatch.setattr(ops, "_native", lambda: Proxy())


def test_llama_few_row_decode_on_fp8_plans(native, qmodel, monkeypatch):
    """A 3-row decode step of the quantized preset runs the planned projections on the FP8 ring
    kernel, tracks the reference forward of the same model (its bf16 image), and every row
    tracks the same sequence decoded alone through the one-row FP8 path: one model whatever
    batch."""
    from docqa_amd.engine.kv_cache import KVCache
    from tests.test_models_gpu import _decode_logits, _prefill_logits, _rel

    m = qmodel
    g = torch.Generator().manual_seed(5)
    prompts = [torch.randint(0, 32000, (n,), generator=g).tolist() for n in (77, 130, 9)]
    nxt = [4, 5, 6]
    BS = 64
    slabs, glu, lm = _planned(m, 3)
    for k in ("qkv", "o", "down"):     # the plan functions agree with themselves at every row count of the bucket
        assert bool(ops.dgemm8_plan(3, *m.layers[0][k].shape)[0]) == bool(ops.dgemm8_plan(4, *m.layers[0][k].shape)[0])
    kv1 = KVCache(m.cfg.layers, 16, m.hkv, m.cfg.head_dim, BS).caches
    kv2 = KVCache(m.cfg.layers, 16, m.hkv, m.cfg.head_dim, BS).caches
    _, tables = _prefill_logits(m, kv1, prompts, BS)
    calls = []
    with monkeypatch.context() as mp:
        _spy(mp, "dgemm8_glu", calls)
        _spy(mp, "dgemm8_partial", calls)
        d1 = _decode_logits(m, kv1, prompts, tables, nxt, BS)
        # the greedy pick of the same rows goes through the FP8 LM head where it is planned
        _spy_native(mp, "dgemm8_argmax_val", calls)
        ids = m.greedy_ids(torch.randn(3, m.cfg.hidden, device="cuda").to(m.dtype))
    assert calls.count("dgemm8_glu") == (m.cfg.layers if glu else 0)
    assert calls.count("dgemm8_partial") == m.cfg.layers * len(slabs)
    assert calls.count("dgemm8_argmax_val") == (1 if lm else 0) and ids.shape == (3,)
    assert slabs and glu and lm       # this preset has every kind of projection on the FP8 kernel
    with native.use_reference():
        _prefill_logits(m, kv2, prompts, BS)
        d2 = _decode_logits(m, kv2, prompts, tables, nxt, BS)
    assert _rel(d1, d2) < 0.03
    for i, p in enumerate(prompts):
        kv = KVCache(m.cfg.layers, 16, m.hkv, m.cfg.head_dim, BS).caches
        _, t1 = _prefill_logits(m, kv, [p], BS)
        alone = _decode_logits(m, kv, [p], t1, [nxt[i]], BS)
        assert _rel(d1[i:i + 1], alone) < 0.03, i


def test_llama_few_row_fp8_step_in_a_graph_equals_eager(native, qmodel, monkeypatch):
    """A 4-row decode step captured into a graph and replayed gives the eager logits, and the
    fused LM-head pick lands on a maximal logit of each row."""
    from docqa_amd.engine.kv_cache import KVCache
    from docqa_amd.models.llama import AttnMeta
    from tests.test_models_gpu import _prefill_logits

    m = qmodel
    g = torch.Generator().manual_seed(6)
    lens = [77, 20, 130, 9]
    prompts = [torch.randint(0, 32000, (n,), generator=g).tolist() for n in lens]
    BS = 64
    kv = KVCache(m.cfg.layers, 24, m.hkv, m.cfg.head_dim, BS).caches
    _, tables = _prefill_logits(m, kv, prompts, BS)
    maxb = max(len(t) for t in tables)
    bt = torch.zeros(len(lens), maxb, dtype=torch.int32)
    for i, t in enumerate(tables):
        bt[i, :len(t)] = torch.tensor(t)
    slots = [tables[i][n // BS] * BS + n % BS for i, n in enumerate(lens)]
    meta = AttnMeta(prefill=False, positions=torch.tensor(lens, dtype=torch.int32, device="cuda"),
                    slot_mapping=torch.tensor(slots, dtype=torch.int32, device="cuda"), block_tables=bt.cuda(),
                    context_lens=torch.tensor([n + 1 for n in lens], dtype=torch.int32, device="cuda"),
                    max_context=maxb * BS)
    tok = torch.tensor([4, 5, 6, 7], dtype=torch.int32, device="cuda")
    eager = m.forward(tok, meta, kv).clone()
    calls = []
    with monkeypatch.context() as mp:
        _spy_native(mp, "dgemm8_argmax_val", calls)
        ids = m.forward(tok, meta, kv, greedy_ids=True)
    torch.cuda.synchronize()
    assert ids.shape == (4,)
    assert len(calls) == (1 if _planned(m, 4)[2] else 0)   # the pick came from the FP8 LM head
    for r in range(4):
        row = eager[r].float()
        assert float(row[int(ids[r])]) >= float(row.max()) - 2e-2 * float(row.abs().max())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        m.forward(tok, meta, kv)                 # warm-up on the capture stream
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            out = m.forward(tok, meta, kv)
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)


def test_engine_bucket4_fp8_graphs_equal_eager(native, qmodel, monkeypatch):
    """Three greedy prompts at max_batch 4 (bucket 4, one padding row): the same token ids with
    and without decode graphs, all inside the vocabulary."""
    monkeypatch.setenv("DOCQA_TUNE_DECODE", "0")  # same GEMM kernels on both paths
    from docqa_amd.engine.llm_engine import LLMEngine, SamplingParams

    m = qmodel
    g = torch.Generator().manual_seed(2)
    prompts = [torch.randint(0, 32000, (n,), generator=g).tolist() for n in (40, 77, 5)]
    sp = SamplingParams(max_new_tokens=8, stop_on_eos=False)
    a = LLMEngine(m, max_batch=4, max_context=256, use_graphs=True).generate(prompts, sp)
    b = LLMEngine(m, max_batch=4, max_context=256, use_graphs=False).generate(prompts, sp)
    assert a == b
    assert all(len(o) == 8 and all(0 <= t < m.cfg.vocab_size for t in o) for o in a)
