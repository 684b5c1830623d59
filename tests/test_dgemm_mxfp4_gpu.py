"""2..32-row decode projections over MXFP4 weights (dgemm.hip dgemm4_kernel) against fp32 on the
dequantized weights W': split-K slabs with scales that differ across rows AND across the blocks of
a row and pairwise different X rows, a one-hot code written by hand (nibble order, scale indexing,
ring turn, slice and tile on the device, independent of the Python dequantizer), the SwiGLU
epilogue, the LM-head argmax with per-row planted winners that differ from their rivals by the
block scales only, the shapes the kernel must refuse, and a few-row decode step of the quantized
Llama test preset: eager, graph-captured and through the engine."""
import pytest
import torch

from docqa_amd import ops
from docqa_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

K0 = 2048     # the kernel's K granule: one whole ring turn (4 stages x 512 codes per row)


@pytest.fixture(scope="module")
def native():
    assert ops.load_native(build_if_missing=True)
    assert ops.DGEMM4_K == K0
    return ops


_WQ = {}


def _wq(N, K, seed):
    """(q, e, W') of random rows whose block (n, b) is multiplied by 2^((n + 3 b) % 7 - 3): scales
    differ across rows and across the blocks of one row, so a dropped, shared or mis-indexed
    scale shows.  Built once per (N, K, seed) and never modified."""
    if (N, K, seed) not in _WQ:
        g = torch.Generator(device="cuda").manual_seed(seed)
        w = (torch.rand(N, K, device="cuda", generator=g) * 2 - 1) / K ** 0.5
        n, b = torch.arange(N, device="cuda")[:, None], torch.arange(K // 32, device="cuda")[None, :]
        w = (w.view(N, K // 32, 32) * torch.exp2(((n + 3 * b) % 7 - 3).float())[:, :, None]).view(N, K)
        q, e = ops.quantize_mxfp4_rows(w.to(torch.bfloat16))
        assert e.unique().numel() >= 6
        _WQ[(N, K, seed)] = (q, e, ops.dequantize_mxfp4_rows(q, e, torch.bfloat16))
    return _WQ[(N, K, seed)]


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
def test_dgemm4_slabs_match_fp32(native, M, K, S):
    N = 128                                    # two 64-row tiles
    x = _x(M, K)
    q, e, wd = _wq(N, K, 1)
    P = torch.ops.docqa.dgemm4_partial(x, q, e, S, 64)
    assert P.shape == (S, M, N) and P.dtype == torch.float32
    r = x.float() @ wd.float().t()
    assert _close(P.sum(0), r)
    # and the bf16 kernel on the image W' computes the same products
    assert _close(P.sum(0), ops.dgemm_partial(x, wd, S).sum(0))


@pytest.mark.parametrize("tile", [32, 16])
@pytest.mark.parametrize("M", [5, 17])
def test_dgemm4_slabs_narrow_tiles(native, M, tile):
    """The 32- and 16-row tiles of the narrow projections (2 and 1 n-tiles per workgroup): the same
    slabs, bit for bit, as the 64-row tiles -- the k order of a product does not depend on the tile."""
    N, K, S = 128, 2 * K0, 2
    x = _x(M, K)
    q, e, wd = _wq(N, K, 1)
    P = torch.ops.docqa.dgemm4_partial(x, q, e, S, tile)
    assert P.shape == (S, M, N)
    assert _close(P.sum(0), x.float() @ wd.float().t())
    assert torch.equal(P, torch.ops.docqa.dgemm4_partial(x, q, e, S, 64))
    with pytest.raises(RuntimeError, match="dgemm4_partial"):
        torch.ops.docqa.dgemm4_partial(x, q[:80].contiguous(), e[:80].contiguous(), S, 32)   # N % 32


# (n*, k*): an odd nibble in the last stage of the second ring turn of the second slice, second
# tile; an even nibble in the first stage of the first slice, first tile; the last code of the
# first turn's third stage (block 15 of the stage, the last k-group's last lane group)
@pytest.mark.parametrize("n_s,k_s", [(101, 4096 + 2048 + 3 * 512 + 13 * 32 + 21), (5, 2), (64, 3 * 512 - 1)])
@pytest.mark.parametrize("M", [3, 17])
def test_dgemm4_one_hot_code_by_hand(native, M, n_s, k_s):
    """Every code is zero except one -3 (code 0b1101) at (n*, k*), whose block has the scale byte
    130 (2^3) among neighbours of 2^-7 .. 2^-1: the slab sum is x[m, k*] * -24 in column n*,
    exactly, and 0 everywhere else."""
    N, K, S = 128, 4 * K0, 2
    g = torch.Generator(device="cuda").manual_seed(9)
    q = torch.zeros(N, K // 2, device="cuda", dtype=torch.uint8)
    e = torch.randint(120, 127, (N, K // 32), device="cuda", generator=g, dtype=torch.uint8)
    e[n_s, k_s // 32] = 130
    q[n_s, k_s // 2] = 0xD << (4 * (k_s & 1))
    x = _x(M, K, 4)
    P = torch.ops.docqa.dgemm4_partial(x, q, e, S, 64)
    assert P.shape == (S, M, N)
    want = torch.zeros(M, N, device="cuda")
    want[:, n_s] = x[:, k_s].float() * -24.0
    assert (want[:, n_s] != 0).all()
    assert torch.equal(P.sum(0), want)
    assert torch.equal(P[1 - k_s // (K // S)], torch.zeros(M, N, device="cuda"))   # the other slice: nothing


def test_dgemm4_real_shape_on_its_plan(native):
    N = K = 4096
    M = 8
    S, t = ops.dgemm4_plan(M, N, K)
    x = _x(M, K, 1)
    q, e, wd = _wq(N, K, 2)
    if S:
        P = ops.dgemm4_partial(x, q, e, S, t)
    else:   # the probe kept this pair on bf16: the kernel itself at the split rule's count
        S = ops.dgemm4_splits(N, K)
        P = torch.ops.docqa.dgemm4_partial(x, q, e, S, 64)
    assert S >= 1 and P.shape == (S, M, N)
    assert _close(P.sum(0), x.float() @ wd.float().t())


@pytest.mark.parametrize("M,N", [(2, 128), (17, 128), (32, 128), (2, 112 * 192), (17, 112 * 192), (32, 112 * 192)])
def test_dgemm4_glu_matches_fp32(native, M, N):
    """64-row tiles, and the 112-row (7 n-tile) variant at the fewest tiles that select it, each
    at one and at two m-tiles (separate instantiations)."""
    x = _x(M, K0, 2)
    q, e, wd = _wq(N, K0, 4)
    y = ops.dgemm4_glu(x, q, e)
    r = ref.silu_mul((x.float() @ wd.float().t()).bfloat16(), interleaved=True).float()
    assert y.shape == (M, N // 2) and y.dtype == torch.bfloat16
    assert _close(y.float(), r, 2e-2, 1e-3)


@pytest.mark.parametrize("M", [2, 32])
def test_dgemm4_argmax_matches_bf16_logits(native, M):
    """LM head + greedy pick over MXFP4 weights == argmax of the bf16-rounded fp32 logits of W'
    over the valid vocabulary, a different winner per X row.  The planted rows are written as
    codes and scales: X row m's winner (row 0's at the last valid id), a rival at a low id with
    the SAME codes and every block scale one exponent lower (the winner wins by its scales only),
    and a row with every scale one exponent higher just past n_valid that must be ignored."""
    N, K, n_valid = 4096, K0, 4000
    x = _x(M, K, 3)
    q0, e0, _ = _wq(N, K, 8)
    q, e = q0.clone(), e0.clone()
    win = [n_valid - 1] + [1000 + 65 * m for m in range(1, M)]
    rival = [5 + 3 * m for m in range(M)]
    for m in range(M):
        # magnitude 0.5 (code 1), sign of x[m] (bit 3), two codes per byte: the planted logits are
        # 0.5 * 2^(e - 127) * sum |x[m]|, about 32 / 16 / 64 against |.| < 8 for the random rows
        c = (1 | ((x[m] < 0).to(torch.uint8) << 3)).view(K // 2, 2)
        codes = c[:, 0] | (c[:, 1] << 4)
        for row, eb in ((win[m], 123), (rival[m], 122), (n_valid + m, 124)):
            q[row] = codes
            e[row] = eb
    wd = ops.dequantize_mxfp4_rows(q, e, torch.bfloat16)
    logits = (x.float() @ wd[:n_valid].float().t()).bfloat16().float()
    assert logits.argmax(1).tolist() == win
    ids, vals = torch.ops.docqa.dgemm4_argmax_val(x, q, e, n_valid)
    assert ids.dtype == torch.int64 and ids.tolist() == win
    top = logits.max(1).values
    assert _close(vals, top)
    # ties go to the lowest id: with equal scales every row's rival is picked
    for m in range(M):
        e[rival[m]] = 123
    ids2, _ = torch.ops.docqa.dgemm4_argmax_val(x, q, e, n_valid)
    assert ids2.tolist() == rival


def test_dgemm4_refuses_shapes_without_a_kernel(native):
    op = torch.ops.docqa.dgemm4_partial
    q, e, _ = _wq(128, 2 * K0, 3)
    with pytest.raises(RuntimeError, match="dgemm4_partial"):
        op(_x(ops.DGEMM4_MAX_ROWS + 1, 2 * K0), q, e, 1, 64)          # rows
    with pytest.raises(RuntimeError, match="dgemm4_partial"):
        op(_x(4, 2 * K0), q[:96].contiguous(), e[:96].contiguous(), 1, 64)   # N % 64
    with pytest.raises(RuntimeError, match="dgemm4_partial"):
        op(_x(4, 2 * K0), q, e, 3, 64)                                # S does not divide K
    q2, e2, _ = _wq(128, K0 + 1024, 3)
    with pytest.raises(RuntimeError, match="dgemm4_partial"):
        op(_x(4, K0 + 1024), q2, e2, 1, 64)                           # not whole ring turns
    with pytest.raises(RuntimeError, match="dgemm4_partial"):
        op(_x(4, 2 * K0), q, e, 2, 64 + 64)                           # tile rows: 64, 32 or 16
    with pytest.raises(RuntimeError, match="dgemm4_glu"):
        torch.ops.docqa.dgemm4_glu(_x(4, K0 + 1024), q2, e2)
    with pytest.raises(RuntimeError, match="dgemm4_argmax_val"):
        torch.ops.docqa.dgemm4_argmax_val(_x(4, 2 * K0), q, e, 129)   # n_valid > N
    with pytest.raises(RuntimeError, match="dgemm4_glu"):
        torch.ops.docqa.dgemm4_glu(_x(4, 2 * K0), q, e[:, :-1].contiguous())   # e is not [N, K / 32]
    with pytest.raises(RuntimeError, match="dgemm4_glu"):
        torch.ops.docqa.dgemm4_glu(_x(4, 2 * K0), q, e[:64].contiguous())
    with pytest.raises(RuntimeError, match="dgemm4_argmax_val"):
        torch.ops.docqa.dgemm4_argmax_val(_x(4, 2 * K0), q.view(torch.int8), e, 128)   # code dtype


# ----------------------------------------------------------------------------- model
@pytest.fixture(scope="module")
def qmodel(native):
    from docqa_amd.models.llama import LlamaConfig, LlamaModel

    m = LlamaModel(LlamaConfig.preset("llama3-1b-test"), device="cuda", seed=17)
    m.quantize_mxfp4()
    return m


@pytest.fixture()
def all_listed(qmodel, monkeypatch):
    """The three plan tables list every preset shape the kernel takes, at every bucket: the model
    tests do not depend on what the probe shipped."""
    L0 = qmodel.layers[0]
    b = (2, 4, 8, 16, 32)
    monkeypatch.setattr(ops, "_DGEMM4_SLAB", {tuple(L0[k].shape): b for k in ("qkv", "o", "down")})
    monkeypatch.setattr(ops, "_DGEMM4_GLU", {tuple(L0["gate_up"].shape): b})
    monkeypatch.setattr(ops, "_DGEMM4_LM", {tuple(qmodel.lm_head.shape): b})
    for k in ("qkv", "o", "down"):
        assert ops.dgemm4_plan(3, *L0[k].shape)[0] == ops.dgemm4_splits(*L0[k].shape) >= 1
    assert ops.dgemm4_glu_ok(3, *L0["gate_up"].shape) and ops.dgemm4_argmax_ok(3, *qmodel.lm_head.shape)
    return qmodel


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


def test_llama_few_row_decode_on_mxfp4_plans(native, all_listed, monkeypatch):
    """A 3-row decode step of the quantized preset runs every projection on the MXFP4 ring kernel,
    tracks the reference forward of the same model (its bf16 image), and every row tracks the same
    sequence decoded alone through the one-row path: one model whatever batch."""
    from docqa_amd.engine.kv_cache import KVCache
    from tests.test_models_gpu import _decode_logits, _prefill_logits, _rel

    m = all_listed
    g = torch.Generator().manual_seed(5)
    prompts = [torch.randint(0, 32000, (n,), generator=g).tolist() for n in (77, 130, 9)]
    nxt = [4, 5, 6]
    BS = 64
    kv1 = KVCache(m.cfg.layers, 16, m.hkv, m.cfg.head_dim, BS).caches
    kv2 = KVCache(m.cfg.layers, 16, m.hkv, m.cfg.head_dim, BS).caches
    _, tables = _prefill_logits(m, kv1, prompts, BS)
    calls = []
    with monkeypatch.context() as mp:
        _spy(mp, "dgemm4_glu", calls)
        _spy(mp, "dgemm4_partial", calls)
        d1 = _decode_logits(m, kv1, prompts, tables, nxt, BS)
        # the greedy pick of the same rows goes through the MXFP4 LM head
        _spy_native(mp, "dgemm4_argmax_val", calls)
        ids = m.greedy_ids(torch.randn(3, m.cfg.hidden, device="cuda").to(m.dtype))
    assert calls.count("dgemm4_glu") == m.cfg.layers
    assert calls.count("dgemm4_partial") == m.cfg.layers * 3      # QKV, O and down
    assert calls.count("dgemm4_argmax_val") == 1 and ids.shape == (3,)
    with native.use_reference():
        _prefill_logits(m, kv2, prompts, BS)
        d2 = _decode_logits(m, kv2, prompts, tables, nxt, BS)
    print(f"rel to the reference forward {_rel(d1, d2):.4f}")
    assert _rel(d1, d2) < 0.03
    for i, p in enumerate(prompts):
        kv = KVCache(m.cfg.layers, 16, m.hkv, m.cfg.head_dim, BS).caches
        _, t1 = _prefill_logits(m, kv, [p], BS)
        alone = _decode_logits(m, kv, [p], t1, [nxt[i]], BS)
        print(f"row {i} rel to its one-row decode {_rel(d1[i:i + 1], alone):.4f}")
        assert _rel(d1[i:i + 1], alone) < 0.03, i


def test_llama_few_row_mxfp4_step_in_a_graph_equals_eager(native, all_listed, monkeypatch):
    """A 4-row decode step captured into a graph and replayed gives the eager logits, and the
    fused LM-head pick lands on a maximal logit of each row."""
    from docqa_amd.engine.kv_cache import KVCache
    from docqa_amd.models.llama import AttnMeta
    from tests.test_models_gpu import _prefill_logits

    m = all_listed
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
    calls = []
    with monkeypatch.context() as mp:
        _spy(mp, "dgemm4_partial", calls)
        eager = m.forward(tok, meta, kv).clone()
        _spy_native(mp, "dgemm4_argmax_val", calls)
        ids = m.forward(tok, meta, kv, greedy_ids=True)
    torch.cuda.synchronize()
    assert ids.shape == (4,)
    assert calls.count("dgemm4_partial") == 2 * 3 * m.cfg.layers and calls.count("dgemm4_argmax_val") == 1
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


def test_engine_bucket4_mxfp4_graphs_equal_eager(native, all_listed, monkeypatch):
    """Three greedy prompts at max_batch 4 (bucket 4, one padding row): the same token ids with
    and without decode graphs, all inside the vocabulary, the steps on the MXFP4 ring kernel."""
    monkeypatch.setenv("DOCQA_TUNE_DECODE", "0")  # same GEMM kernels on both paths
    from docqa_amd.engine.llm_engine import LLMEngine, SamplingParams

    m = all_listed
    g = torch.Generator().manual_seed(2)
    prompts = [torch.randint(0, 32000, (n,), generator=g).tolist() for n in (40, 77, 5)]
    sp = SamplingParams(max_new_tokens=8, stop_on_eos=False)
    a = LLMEngine(m, max_batch=4, max_context=256, use_graphs=True).generate(prompts, sp)
    calls = []
    with monkeypatch.context() as mp:
        _spy(mp, "dgemm4_glu", calls)
        b = LLMEngine(m, max_batch=4, max_context=256, use_graphs=False).generate(prompts, sp)
    assert calls
    assert a == b
    assert all(len(o) == 8 and all(0 <= t < m.cfg.vocab_size for t in o) for o in a)
