"""Batch-1 GEMV over FP8 weights (dgemm.hip gemv8_kernel) against fp32 on the dequantized
weights: split-K slabs at every (rows, chunks, codes per load) it is instantiated for, rows
carrying different scale exponents; the SwiGLU epilogue; the in-kernel input row against the
bf16 GEMV's identical prologue; the LM-head argmax with planted winners that differ by their
scale only; and a batch-1 decode of the quantized Llama test preset, eager and graph-captured."""
import pytest
import torch

from docqa_amd import ops
from docqa_amd.ops import reference as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def native():
    assert ops.load_native(build_if_missing=True)
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


def _x(K, seed=0):
    g = torch.Generator(device="cuda").manual_seed(100 + seed)
    return (torch.rand(1, K, device="cuda", generator=g) * 2 - 1).to(torch.bfloat16)


# the issue's shapes (N, K, S, rows, codes per load), then every instantiation at N = 2 R
_SLABS = [(64, 2048, 1, 16, 8), (64, 4096, 1, 16, 16), (48, 8192, 2, 8, 16), (32, 14336, 1, 4, 8)]
_SLABS += [(2 * R, C * 256 * lb, 1, R, lb) for (R, C, lb) in ops.GEMV8_CASES]
_SLABS += [(2 * R, 2 * C * 256 * lb, 2, R, lb) for (R, C, lb) in ops.GEMV8_CASES[:2]]


@pytest.mark.parametrize("N,K,S,R,lb", _SLABS)
def test_gemv8_slabs_match_fp32(native, N, K, S, R, lb):
    x = _x(K)
    q, s, wd = _wq(N, K, 1)
    P = torch.ops.docqa.gemv8(x, q, s, S, R, lb, False)
    assert P.shape == (S, 1, N) and P.dtype == torch.float32
    r = x.float() @ wd.float().t()
    assert (P.sum(0) - r).abs().max().item() <= 1e-3 * r.abs().max().item() + 1e-4
    # uint8 codes are the same weights
    P2 = torch.ops.docqa.gemv8(x, q.view(torch.uint8), s, S, R, lb, False)
    assert torch.equal(P, P2)


def test_gemv8_real_shape_on_its_plan(native):
    N = K = 4096
    S, R = ops.gemv8_plan(1, N, K)
    assert S and R
    x = _x(K)
    q, s, wd = _wq(N, K, 2)
    P = ops.gemv8_partial(x, q, s, S, R)
    r = x.float() @ wd.float().t()
    assert P.shape == (S, 1, N)
    assert (P.sum(0) - r).abs().max().item() <= 1e-3 * r.abs().max().item() + 1e-4


def test_gemv8_refuses_shapes_without_a_kernel(native):
    x = _x(4096)
    q, s, _ = _wq(64, 4096, 3)
    with pytest.raises(RuntimeError, match="gemv8"):
        torch.ops.docqa.gemv8(x, q, s, 1, 4, 8, False)      # (4, 2, 8) is not instantiated
    with pytest.raises(RuntimeError, match="gemv8"):
        torch.ops.docqa.gemv8(x, q, s, 1, 16, 12, False)    # codes per load: 8 or 16
    with pytest.raises(RuntimeError, match="gemv8"):
        torch.ops.docqa.gemv8(x, q, s, 3, 16, 8, False)     # K % S


@pytest.mark.parametrize("N,K,R,lb", [(32, 2048, 0, 0), (64, 4096, 0, 0), (28672, 4096, 0, 0)]
                         + [(2 * R, C * 256 * lb, R, lb) for (R, C, lb) in ops.GEMV8_EPI_CASES])
def test_gemv8_glu_matches_fp32(native, N, K, R, lb):
    x = _x(K, 1)
    q, s, wd = _wq(N, K, 4)
    y = ops.gemv8_glu(x, q, s, R, lb)
    r = ref.silu_mul((x.float() @ wd.float().t()).bfloat16(), interleaved=True).float()
    assert y.shape == (1, N // 2) and y.dtype == torch.bfloat16
    assert (y.float() - r).abs().max().item() <= 2e-2 * r.abs().max().item() + 1e-3


def _xn_inputs(H, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    Pin = torch.randn(3, 1, H, device="cuda", generator=g)
    res = torch.randn(1, H, device="cuda", generator=g).to(torch.bfloat16)
    gamma = (1 + 0.1 * torch.randn(H, device="cuda", generator=g)).to(torch.bfloat16)
    return Pin, res, gamma


@pytest.mark.parametrize("N,R,C,lb", [(6144, 16, 1, 16)] + [(2 * R, R, C, lb) for (R, C, lb) in ops.GEMV8_XN_CASES])
def test_gemv8_xn_slabs_match_bf16_gemv_prologue(native, N, R, C, lb):
    """Same input-row arithmetic as the bf16 gemv_partial_xn: the same residual out, products
    equal up to the dot-product order."""
    H = C * 256 * lb
    Pin, res, gamma = _xn_inputs(H, 3)
    q, s, wd = _wq(N, H, 5)
    r1, r2 = torch.empty_like(res), torch.empty_like(res)
    a = ops.gemv8_partial_xn(Pin, res, r1, gamma, 1e-5, q, s, 1, R, lb).sum(0)
    b = ops.gemv_partial_xn(Pin, res, r2, gamma, 1e-5, wd, 1, 8).sum(0)
    assert torch.equal(r1, r2)
    assert (a.float() - b.float()).abs().max().item() <= 1e-2 * b.float().abs().max().item() + 1e-3


@pytest.mark.parametrize("N,H,R,lb", [(28672, 4096, 0, 0), (64, 2048, 0, 0)]
                         + [(2 * R, C * 256 * lb, R, lb) for (R, C, lb) in ops.GEMV8_EPI_CASES])
def test_gemv8_xn_glu_matches_bf16_gemv_prologue(native, N, H, R, lb):
    Pin, res, gamma = _xn_inputs(H, 6)
    q, s, wd = _wq(N, H, 7)
    r1, r2 = torch.empty_like(res), torch.empty_like(res)
    a = ops.gemv8_glu_xn(Pin, res, r1, gamma, 1e-5, q, s, R, lb)
    b = ops.gemv_glu_xn(Pin, res, r2, gamma, 1e-5, wd)
    assert torch.equal(r1, r2)
    assert (a.float() - b.float()).abs().max().item() <= 1e-2 * b.float().abs().max().item() + 1e-3


@pytest.mark.parametrize("N,K,n_valid,R,lb", [(4096, 4096, 1000, 0, 0), (32000, 2048, 31990, 0, 0),
                                              (4096, 4096, 1000, 32, 16), (32000, 2048, 31990, 32, 8),
                                              (4096, 4096, 1000, 16, 8)])
def test_gemv8_argmax_matches_bf16_logits(native, N, K, n_valid, R, lb):
    """LM head + greedy pick over FP8 weights == argmax of the bf16 fp32-accumulated logits of
    the dequantized weights over the valid vocabulary.  The planted rows are written as codes
    and scales (so they survive quantization by construction): the winner at the last valid id,
    a rival at id 5 with the SAME codes and half the scale (the winner wins by its scale only,
    and a dropped scale would tie towards the lower id), and a row with twice the scale just
    past n_valid that must be ignored."""
    x = _x(K, 2)
    q, s, _ = _wq(N, K, 8)
    codes = (torch.sign(x.float()[0]) * 64).to(torch.float8_e4m3fn)
    q, s = q.clone(), s.clone()
    for row, sc in ((n_valid - 1, 2.0 ** -8), (5, 2.0 ** -9), (n_valid, 2.0 ** -7)):
        q[row] = codes
        s[row] = sc
    wd = ops.dequantize_fp8_rows(q, s, torch.bfloat16)
    logits = (x.float() @ wd[:n_valid].float().t()).bfloat16().float()
    assert int(logits.argmax(1)[0]) == n_valid - 1
    if R:
        ids, vals = torch.ops.docqa.gemv8_argmax_val(x, q, s, n_valid, R, lb)
    else:
        assert ops.gemv8_argmax_ok(1, N, K)
        ids, vals = ops.lm_head_argmax(x, wd, n_valid, with_values=True, fp8=(q, s))
    assert int(ids[0]) == n_valid - 1
    assert abs(float(vals[0]) - float(logits.max())) <= 1e-2 * abs(float(logits.max()))
    # ties go to the lowest id: with equal scales the rival at id 5 is picked
    s[5] = s[n_valid - 1]
    ids2, _ = torch.ops.docqa.gemv8_argmax_val(x, q, s, n_valid, R or 16, lb or ops.gemv8_lb(K))
    assert int(ids2[0]) == 5


# ----------------------------------------------------------------------------- model
@pytest.fixture(scope="module")
def qmodel(native):
    from docqa_amd.models.llama import LlamaConfig, LlamaModel

    m = LlamaModel(LlamaConfig.preset("llama3-1b-test"), device="cuda", seed=17)
    m.quantize_fp8()
    return m


def test_quantized_model_has_fp8_plans_everywhere(qmodel):
    L0 = qmodel.layers[0]
    for k in ("qkv", "o", "down"):
        assert ops.gemv8_plan(1, *L0[k].shape)[0], k
    assert ops.gemv8_glu_ok(1, *L0["gate_up"].shape)
    assert ops.gemv8_argmax_ok(1, *qmodel.lm_head.shape)
    assert qmodel.weight_format == "fp8-e4m3"
    q, s = qmodel.fp8[0]["down"]
    assert q.is_cuda and q.dtype == torch.float8_e4m3fn and s.dtype == torch.float32
    assert torch.equal(ops.dequantize_fp8_rows(q, s, torch.bfloat16), L0["down"])


def test_llama_batch1_decode_on_fp8_plans(native, qmodel):
    """One-row decode steps of the quantized Llama test preset stream the FP8 copies and track
    the fp32 reference forward of the same model (its bf16 image)."""
    from docqa_amd.engine.kv_cache import KVCache
    from tests.test_models_gpu import _decode_logits, _prefill_logits, _rel

    m = qmodel
    prompts = [torch.randint(0, 32000, (77,), generator=torch.Generator().manual_seed(5)).tolist()]
    BS = 64
    kv1 = KVCache(m.cfg.layers, 16, m.hkv, m.cfg.head_dim, BS).caches
    kv2 = KVCache(m.cfg.layers, 16, m.hkv, m.cfg.head_dim, BS).caches
    _, tables = _prefill_logits(m, kv1, prompts, BS)
    called = []
    orig = ops.gemv8_glu_xn
    try:
        ops.gemv8_glu_xn = lambda *a, **k: (called.append(1), orig(*a, **k))[1]
        d1 = _decode_logits(m, kv1, prompts, tables, [4], BS)
    finally:
        ops.gemv8_glu_xn = orig
    assert len(called) == m.cfg.layers          # the step really ran on the FP8 chain
    with native.use_reference():
        _prefill_logits(m, kv2, prompts, BS)
        d2 = _decode_logits(m, kv2, prompts, tables, [4], BS)
    assert _rel(d1, d2) < 0.03


def test_llama_batch1_fp8_step_in_a_graph_equals_eager(native, qmodel):
    """The same decode step captured into a graph and replayed gives the eager logits, and the
    fused FP8 LM-head pick lands on a maximal logit."""
    from docqa_amd.engine.kv_cache import KVCache
    from docqa_amd.models.llama import AttnMeta
    from tests.test_models_gpu import _prefill_logits

    m = qmodel
    n = 77
    prompts = [torch.randint(0, 32000, (n,), generator=torch.Generator().manual_seed(6)).tolist()]
    BS = 64
    kv = KVCache(m.cfg.layers, 16, m.hkv, m.cfg.head_dim, BS).caches
    _, tables = _prefill_logits(m, kv, prompts, BS)
    t = tables[0]
    meta = AttnMeta(prefill=False, positions=torch.tensor([n], dtype=torch.int32, device="cuda"),
                    slot_mapping=torch.tensor([t[n // BS] * BS + n % BS], dtype=torch.int32, device="cuda"),
                    block_tables=torch.tensor([t], dtype=torch.int32, device="cuda"),
                    context_lens=torch.tensor([n + 1], dtype=torch.int32, device="cuda"),
                    max_context=len(t) * BS)
    tok = torch.tensor([4], dtype=torch.int32, device="cuda")
    eager = m.forward(tok, meta, kv).clone()
    ids = m.forward(tok, meta, kv, greedy_ids=True)
    torch.cuda.synchronize()
    assert float(eager[0, int(ids[0])]) >= float(eager.float().max()) - 2e-2 * float(eager.float().abs().max())
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
