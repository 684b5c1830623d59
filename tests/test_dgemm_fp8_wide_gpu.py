"""33..128-row decode projections over FP8 weights (dgemm.hip dgemm8w_kernel: waves own n-tiles,
X through LDS) against fp32 on the dequantized weights W': split-K slabs with rows carrying
different scale exponents and pairwise different X rows at the first and last row of both
instantiations and a ragged last m-tile in each, the SwiGLU epilogue, the LM-head argmax with
per-row planted winners that differ from their rivals by the scale only, the shapes the kernel
must refuse, and a 40-row decode step of the quantized Llama test preset with the plan tables
patched to list its shapes: eager, graph-captured and through the engine.  Tolerances are
tests/test_dgemm_fp8_gpu.py's: the arithmetic is the same (exact widening, fp32 accumulation)."""
import pytest
import torch

from docqa_amd import ops
from docqa_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

K0 = 512      # the kernel's K granule: four 128-deep stages
TILE = 128    # weight rows per workgroup
ROWS = [33, 48, 64, 65, 100, 128]


@pytest.fixture(scope="module")
def native():
    assert ops.load_native(build_if_missing=True)
    assert ops.DGEMM8W_K == K0 and ops.DGEMM8W_MAX_ROWS == 128 and ops.DGEMM8W_TILE == TILE
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


@pytest.fixture(scope="module")
def slab_weights(native):
    """(q, s, W') per K of the slab cases, built once and left unchanged."""
    return {K: _wq(2 * TILE, K, 1) for K in (K0, 2 * K0)}


@pytest.mark.parametrize("K,S", [(K0, 1), (2 * K0, 2)])
@pytest.mark.parametrize("M", ROWS)
def test_dgemm8w_slabs_match_fp32(native, slab_weights, M, K, S):
    N = 2 * TILE
    x = _x(M, K)
    q, s, wd = slab_weights[K]
    P = torch.ops.docqa.dgemm8w_partial(x, q, s, S, TILE)
    assert P.shape == (S, M, N) and P.dtype == torch.float32
    r = x.float() @ wd.float().t()
    assert _close(P.sum(0), r)
    # uint8 codes are the same weights
    assert torch.equal(P, torch.ops.docqa.dgemm8w_partial(x, q.view(torch.uint8), s, S, TILE))
    # and the bf16 kernel on the image W' computes the same products
    assert _close(P.sum(0), ops.dgemm_partial(x, wd, S).sum(0))


def test_dgemm8w_real_shape_on_its_plan(native):
    N = K = 4096
    M = 64
    S, t = ops.dgemm8w_plan(M, N, K)
    x = _x(M, K, 1)
    q, s, wd = _wq(N, K, 2)
    if S:
        P = ops.dgemm8w_partial(x, q, s, S, t)
    else:   # the probe kept this pair on bf16: the kernel itself at decode_plan's split, whole turns
        S = max(ops.decode_plan(M, N, K)[0], 1)
        while K % S or (K // S) % K0:
            S -= 1
        P = torch.ops.docqa.dgemm8w_partial(x, q, s, S, TILE)
    assert P.shape == (S, M, N)
    assert _close(P.sum(0), x.float() @ wd.float().t())


@pytest.mark.parametrize("N", [TILE, 3 * TILE])
@pytest.mark.parametrize("M", [33, 64, 65, 128])
def test_dgemm8w_glu_matches_fp32(native, M, N):
    """The one tile variant (128 weight rows) at the fewest tiles that select it (one) and at three,
    at the first and last row of both m-tile instantiations."""
    x = _x(M, K0, 2)
    q, s, wd = _wq(N, K0, 4)
    y = ops.dgemm8w_glu(x, q, s)
    r = ref.silu_mul((x.float() @ wd.float().t()).bfloat16(), interleaved=True).float()
    assert y.shape == (M, N // 2) and y.dtype == torch.bfloat16
    assert _close(y.float(), r, 2e-2, 1e-3)


@pytest.mark.parametrize("M", [33, 128])
def test_dgemm8w_argmax_matches_bf16_logits(native, M):
    """LM head + greedy pick over FP8 weights == argmax of the bf16-rounded fp32 logits of W'
    over the valid vocabulary, a different winner per X row.  The planted rows are written as
    codes and scales: X row m's winner (row 0's at the last valid id), a rival at a low id with
    the SAME codes and half the scale (the winner wins by its scale only), and a row with twice
    the scale just past n_valid that must be ignored (N - n_valid = 96 rows lie past n_valid, so
    of 128 X rows the first 96 have such a row of their own)."""
    N, K, n_valid = 4096, K0, 4000
    x = _x(M, K, 3)
    q, s, _ = _wq(N, K, 8)
    q, s = q.clone(), s.clone()
    win = [n_valid - 1] + [400 + 28 * m for m in range(1, M)]
    rival = [5 + 3 * m for m in range(M)]
    assert len(set(win)) == M and max(win) < n_valid and not set(win) & set(rival)
    assert len({w // TILE for w in win}) > 1          # winners spread over more than one tile
    for m in range(M):
        codes = (torch.sign(x.float()[m]) * 64).to(torch.float8_e4m3fn)
        rows = [(win[m], 2.0 ** -8), (rival[m], 2.0 ** -9)] + ([(n_valid + m, 2.0 ** -7)] if n_valid + m < N else [])
        for row, sc in rows:
            q[row] = codes
            s[row] = sc
    wd = ops.dequantize_fp8_rows(q, s, torch.bfloat16)
    logits = (x.float() @ wd[:n_valid].float().t()).bfloat16().float()
    assert logits.argmax(1).tolist() == win
    assert (x.float() @ wd.float().t()).argmax(1)[: min(M, N - n_valid)].ge(n_valid).all()   # the decoys would win
    ids, vals = torch.ops.docqa.dgemm8w_argmax_val(x, q, s, n_valid)
    assert ids.dtype == torch.int64 and ids.tolist() == win
    top = logits.max(1).values
    assert ((vals - top).abs() <= 1e-2 * top.abs()).all()
    # ties go to the lowest id: with equal scales every row's rival is picked
    for m in range(M):
        s[rival[m]] = s[win[m]]
    ids2, _ = torch.ops.docqa.dgemm8w_argmax_val(x, q, s, n_valid)
    assert ids2.tolist() == rival


def test_dgemm8w_refuses_shapes_without_a_kernel(native):
    op = torch.ops.docqa.dgemm8w_partial
    q, s, _ = _wq(2 * TILE, 2 * K0, 3)
    for M in (32, 129):                                                 # rows
        with pytest.raises(RuntimeError, match="dgemm8w_partial"):
            op(_x(M, 2 * K0), q, s, 1, TILE)
        with pytest.raises(RuntimeError, match="dgemm8w_glu"):
            torch.ops.docqa.dgemm8w_glu(_x(M, 2 * K0), q, s)
        with pytest.raises(RuntimeError, match="dgemm8w_argmax_val"):
            torch.ops.docqa.dgemm8w_argmax_val(_x(M, 2 * K0), q, s, 2 * TILE)
    with pytest.raises(RuntimeError, match="dgemm8w_partial"):
        op(_x(40, 2 * K0), q[:192].contiguous(), s[:192].contiguous(), 1, TILE)   # N % 128
    with pytest.raises(RuntimeError, match="dgemm8w_partial"):
        op(_x(40, 2 * K0), q, s, 3, TILE)                              # S does not divide K
    with pytest.raises(RuntimeError, match="dgemm8w_partial"):
        op(_x(40, 2 * K0), q, s, 4, TILE)                              # slices of half a turn
    q2, s2, _ = _wq(2 * TILE, K0 + 128, 3)
    with pytest.raises(RuntimeError, match="dgemm8w_partial"):
        op(_x(40, K0 + 128), q2, s2, 1, TILE)                          # not whole ring turns
    with pytest.raises(RuntimeError, match="dgemm8w_glu"):
        torch.ops.docqa.dgemm8w_glu(_x(40, K0 + 128), q2, s2)
    with pytest.raises(RuntimeError, match="dgemm8w_argmax_val"):
        torch.ops.docqa.dgemm8w_argmax_val(_x(40, 2 * K0), q, s, 2 * TILE + 1)   # n_valid > N
    with pytest.raises(RuntimeError, match="dgemm8w_argmax_val"):
        torch.ops.docqa.dgemm8w_argmax_val(_x(40, 2 * K0), q, s, 0)   # n_valid < 1
    with pytest.raises(RuntimeError, match="dgemm8w_glu"):
        torch.ops.docqa.dgemm8w_glu(_x(40, 2 * K0), q, s[:TILE].contiguous())   # scale length
    with pytest.raises(RuntimeError, match="dgemm8w_argmax_val"):
        torch.ops.docqa.dgemm8w_argmax_val(_x(40, 2 * K0), q.view(torch.int8), s, TILE)   # code dtype


# ----------------------------------------------------------------------------- model
LENS40 = [77, 130, 9, 63, 64, 127, 20, 40] * 5      # mixed; 63 / 64 / 127: the new token crosses a block


@pytest.fixture(scope="module")
def qmodel(native):
    from docqa_amd.models.llama import LlamaConfig, LlamaModel

    m = LlamaModel(LlamaConfig.preset("llama3-1b-test"), device="cuda", seed=17)
    m.quantize_fp8()
    return m


@pytest.fixture
def wide_tables(qmodel, monkeypatch):
    """The shipped tables list served-model shapes only: list the preset's four projections and
    its LM head at both buckets.  Returns the projections that are whole turns of the granule."""
    L0 = qmodel.layers[0]
    b = (64, 128)
    slab = {}
    for k in ("qkv", "o", "down"):
        N, K = L0[k].shape
        S = next(S for S in (4, 2, 1) if K % S == 0 and (K // S) % K0 == 0)
        slab[(N, K)] = {bk: (S, TILE) for bk in b}
    monkeypatch.setattr(ops, "_DGEMM8W", True)
    monkeypatch.setattr(ops, "_DGEMM8W_SLAB", slab)
    monkeypatch.setattr(ops, "_DGEMM8W_GLU", {tuple(L0["gate_up"].shape): b})
    monkeypatch.setattr(ops, "_DGEMM8W_LM", {tuple(qmodel.lm_head.shape): b})
    slabs = [k for k in ("qkv", "o", "down") if ops.dgemm8w_plan(40, *L0[k].shape)[0]]
    glu = ops.dgemm8w_glu_ok(40, *L0["gate_up"].shape)
    lm = ops.dgemm8w_argmax_ok(40, *qmodel.lm_head.shape)
    # every projection of this preset is whole turns: the tests below exercise all of them
    assert slabs == ["qkv", "o", "down"] and glu and lm
    return slabs


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


def _prompts(seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 32000, (n,), generator=g).tolist() for n in LENS40]


def test_llama_40_row_decode_on_wide_fp8_plans(native, qmodel, wide_tables, monkeypatch):
    """A 40-row decode step of the quantized preset runs every projection on the wide FP8 kernel,
    tracks the reference forward of the same model (its bf16 image), and rows 0, 17 and 39 track
    the same sequence decoded alone through the one-row FP8 path: one model whatever batch."""
    from docqa_amd.engine.kv_cache import KVCache
    from tests.test_models_gpu import _decode_logits, _prefill_logits, _rel

    m = qmodel
    prompts = _prompts(5)
    nxt = [4 + i for i in range(40)]
    BS = 64
    plan = m._step_plan(40, _decode_meta_stub(), True, False)
    assert plan.glu == ("streamed_wide",) and all(plan.proj[k][0] == "streamed_wide" for k in wide_tables)
    kv1 = KVCache(m.cfg.layers, 160, m.hkv, m.cfg.head_dim, BS).caches
    kv2 = KVCache(m.cfg.layers, 160, m.hkv, m.cfg.head_dim, BS).caches
    _, tables = _prefill_logits(m, kv1, prompts, BS)
    calls = []
    with monkeypatch.context() as mp:
        _spy(mp, "dgemm8w_glu", calls)
        _spy(mp, "dgemm8w_partial", calls)
        d1 = _decode_logits(m, kv1, prompts, tables, nxt, BS)
        _spy_native(mp, "dgemm8w_argmax_val", calls)
        ids = m.greedy_ids(torch.randn(40, m.cfg.hidden, device="cuda").to(m.dtype))
    assert calls.count("dgemm8w_glu") == m.cfg.layers
    assert calls.count("dgemm8w_partial") == m.cfg.layers * 3
    assert calls.count("dgemm8w_argmax_val") == 1 and ids.shape == (40,)
    with native.use_reference():
        _prefill_logits(m, kv2, prompts, BS)
        d2 = _decode_logits(m, kv2, prompts, tables, nxt, BS)
    r = _rel(d1, d2)
    print(f"40-row step vs reference: rel {r:.4f}")
    assert r < 0.03
    for i in (0, 17, 39):
        kv = KVCache(m.cfg.layers, 16, m.hkv, m.cfg.head_dim, BS).caches
        _, t1 = _prefill_logits(m, kv, [prompts[i]], BS)
        alone = _decode_logits(m, kv, [prompts[i]], t1, [nxt[i]], BS)
        r = _rel(d1[i:i + 1], alone)
        print(f"row {i} vs alone: rel {r:.4f}")
        assert r < 0.03, i


def _decode_meta_stub():
    from docqa_amd.models.llama import AttnMeta

    return AttnMeta(prefill=False, positions=None, slot_mapping=None)


def test_llama_40_row_wide_fp8_step_in_a_graph_equals_eager(native, qmodel, wide_tables, monkeypatch):
    """The 40-row decode step captured into a graph and replayed twice gives the eager logits bit
    for bit, and the fused LM-head pick lands on a maximal logit of each row."""
    from docqa_amd.engine.kv_cache import KVCache
    from docqa_amd.models.llama import AttnMeta
    from tests.test_models_gpu import _prefill_logits

    m = qmodel
    lens = LENS40
    prompts = _prompts(6)
    BS = 64
    kv = KVCache(m.cfg.layers, 160, m.hkv, m.cfg.head_dim, BS).caches
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
    tok = torch.arange(4, 44, dtype=torch.int32, device="cuda")
    calls = []
    with monkeypatch.context() as mp:
        _spy(mp, "dgemm8w_glu", calls)
        _spy(mp, "dgemm8w_partial", calls)
        eager = m.forward(tok, meta, kv).clone()
        _spy_native(mp, "dgemm8w_argmax_val", calls)
        ids = m.forward(tok, meta, kv, greedy_ids=True)
    torch.cuda.synchronize()
    assert calls.count("dgemm8w_glu") == 2 * m.cfg.layers and calls.count("dgemm8w_partial") == 6 * m.cfg.layers
    assert calls.count("dgemm8w_argmax_val") == 1 and ids.shape == (40,)
    for r in range(40):
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


def test_engine_bucket64_wide_fp8_graphs_equal_eager(native, qmodel, wide_tables, monkeypatch):
    """40 greedy prompts at max_batch 64 (bucket 64, 24 padding rows): the same token ids with and
    without decode graphs, all inside the vocabulary, the decode steps on the wide FP8 kernel."""
    monkeypatch.setenv("DOCQA_TUNE_DECODE", "0")  # same GEMM kernels on both paths
    from docqa_amd.engine.llm_engine import LLMEngine, SamplingParams

    m = qmodel
    g = torch.Generator().manual_seed(2)
    prompts = [torch.randint(0, 32000, (n,), generator=g).tolist() for n in [40, 77, 5, 61, 12] * 8]
    sp = SamplingParams(max_new_tokens=8, stop_on_eos=False)
    calls = []
    _spy(monkeypatch, "dgemm8w_glu", calls)
    b = LLMEngine(m, max_batch=64, max_context=256, use_graphs=False).generate(prompts, sp)
    assert calls                                   # the eager engine's decode steps took the wide kernel
    a = LLMEngine(m, max_batch=64, max_context=256, use_graphs=True).generate(prompts, sp)
    assert a == b
    assert len(a) == 40 and all(len(o) == 8 and all(0 <= t < m.cfg.vocab_size for t in o) for o in a)
