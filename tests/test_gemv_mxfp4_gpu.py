"""Batch-1 GEMV over MXFP4 weights (dgemm.hip gemv4_kernel) against fp32 on the dequantized
weights: split-K slabs at every (rows, chunks, codes per load, waves along K) it is instantiated
for, with scales that differ across rows AND across the blocks of a row; a one-hot block with
hand-made codes (nibble order and scale indexing on the device, independent of the Python
dequantizer); the SwiGLU epilogue; the in-kernel input row against the bf16 GEMV's identical
prologue; the LM-head argmax with planted winners that differ by one block scale only; and a
batch-1 decode of the quantized Llama test preset, eager and graph-captured."""
import pytest
import torch

from docqa_amd import ops
from docqa_amd.ops import reference as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def native():
    assert ops.load_native(build_if_missing=True)
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


def _x(K, seed=0):
    g = torch.Generator(device="cuda").manual_seed(100 + seed)
    return (torch.rand(1, K, device="cuda", generator=g) * 2 - 1).to(torch.bfloat16)


def _kmin(C, lb, kw):
    return C * 64 * lb * kw


# fixed shapes at each real K (N, K, S, rows, codes per load, waves along K), then every
# instantiation at N = 2 R with the smallest K it accepts, the first two again at S = 2
_SLABS = [(64, 2048, 1, 16, 32, 1), (64, 4096, 1, 16, 32, 2), (48, 8192, 2, 8, 16, 4), (32, 14336, 1, 4, 32, 1)]
_SLABS += [(2 * R, _kmin(C, lb, kw), 1, R, lb, kw) for (R, C, lb, kw) in ops.GEMV4_CASES]
_SLABS += [(2 * R, 2 * _kmin(C, lb, kw), 2, R, lb, kw) for (R, C, lb, kw) in ops.GEMV4_CASES[:2]]


@pytest.mark.parametrize("N,K,S,R,lb,kw", _SLABS)
def test_gemv4_slabs_match_fp32(native, N, K, S, R, lb, kw):
    x = _x(K)
    q, e, wd = _wq(N, K, 1)
    P = torch.ops.docqa.gemv4(x, q, e, S, R, lb, kw, False)
    assert P.shape == (S, 1, N) and P.dtype == torch.float32
    r = x.float() @ wd.float().t()
    assert (P.sum(0) - r).abs().max().item() <= 1e-3 * r.abs().max().item() + 1e-4


def test_gemv4_real_shapes_on_their_plans(native):
    """Every planned slab shape through the public wrapper (ops.gemv4_plan picks the kernel)."""
    ran = 0
    for N, K in [(3072, 2048), (6144, 4096), (4096, 4096), (2048, 8192), (4096, 14336)]:
        S, R = ops.gemv4_plan(1, N, K)
        if not S:
            continue
        ran += 1
        x = _x(K)
        q, e, wd = _wq(N, K, 2)
        P = ops.gemv4_partial(x, q, e, S, R)
        r = x.float() @ wd.float().t()
        assert P.shape == (S, 1, N)
        assert (P.sum(0) - r).abs().max().item() <= 1e-3 * r.abs().max().item() + 1e-4
    assert ran or not ops._GEMV4_PLAN


@pytest.mark.parametrize("N,K,S,R,lb,kw,blk", [(32, 4096, 1, 16, 32, 2, 77), (16, 4096, 1, 8, 16, 4, 77),
                                               (16, 4096, 1, 8, 16, 4, 78), (8, 14336, 1, 4, 32, 1, 447),
                                               (8, 14336, 1, 4, 16, 2, 129), (32, 2048, 1, 16, 32, 1, 0)])
def test_gemv4_one_hot_block_by_hand(native, N, K, S, R, lb, kw, blk):
    """x is zero outside block ``blk``; every row's codes there are written by hand with a known
    scale byte (every other block holds other codes and scales, which must not contribute)."""
    g = torch.Generator(device="cuda").manual_seed(9)
    q = torch.randint(0, 256, (N, K // 2), device="cuda", generator=g, dtype=torch.uint8)
    e = torch.randint(120, 134, (N, K // 32), device="cuda", generator=g, dtype=torch.uint8)
    eb = (124 + torch.arange(N, device="cuda") % 6).to(torch.uint8)       # 2^-3 .. 2^2 by row
    e[:, blk] = eb
    scale = torch.exp2(eb.float() - 127)
    x = torch.zeros(1, K, device="cuda", dtype=torch.bfloat16)
    xb = (torch.arange(32, device="cuda") % 5 - 1).float()                # -1 .. 3, small integers
    x[0, blk * 32:(blk + 1) * 32] = xb.to(torch.bfloat16)
    # all code 7 = +6: 6 * scale * sum(x)
    q[:, blk * 16:(blk + 1) * 16] = 0x77
    P = torch.ops.docqa.gemv4(x, q, e, S, R, lb, kw, False).sum(0)[0]
    assert torch.equal(P, 6 * scale * xb.sum())
    # element 2j = +1 (code 2, bits 0..3), element 2j + 1 = -6 (code 15, bits 4..7)
    q[:, blk * 16:(blk + 1) * 16] = 0xF2
    P = torch.ops.docqa.gemv4(x, q, e, S, R, lb, kw, False).sum(0)[0]
    assert torch.equal(P, scale * (xb[0::2].sum() - 6 * xb[1::2].sum()))
    # one element alone: k = 32 blk + 13 (odd: the high nibble of byte 6) = +1.5 (code 3)
    q[:, blk * 16:(blk + 1) * 16] = 0
    q[:, blk * 16 + 6] = 3 << 4
    P = torch.ops.docqa.gemv4(x, q, e, S, R, lb, kw, False).sum(0)[0]
    assert torch.equal(P, scale * 1.5 * xb[13])


def test_gemv4_refuses_shapes_without_a_kernel(native):
    x = _x(4096)
    q, e, _ = _wq(64, 4096, 3)
    with pytest.raises(RuntimeError, match="gemv4"):
        torch.ops.docqa.gemv4(x, q, e, 1, 4, 32, 2, False)      # (4, 1, 32, 2) is not instantiated
    with pytest.raises(RuntimeError, match="gemv4"):
        torch.ops.docqa.gemv4(x, q, e, 1, 16, 24, 2, False)     # codes per load: 16 or 32
    with pytest.raises(RuntimeError, match="gemv4"):
        torch.ops.docqa.gemv4(x, q, e, 3, 16, 32, 2, False)     # K % S
    with pytest.raises(RuntimeError, match="gemv4"):            # K = 2064: K % 32 == 16
        torch.ops.docqa.gemv4(_x(2064), q[:, :1032].contiguous(), e[:, :64].contiguous(), 1, 16, 32, 1, False)


@pytest.mark.parametrize("N,K,R,lb,kw", [(32, 2048, 0, 0, 0), (64, 4096, 0, 0, 0), (28672, 4096, 16, 32, 2)]
                         + [(2 * R, _kmin(C, lb, kw), R, lb, kw) for (R, C, lb, kw) in ops.GEMV4_EPI_CASES])
def test_gemv4_glu_matches_fp32(native, N, K, R, lb, kw):
    x = _x(K, 1)
    q, e, wd = _wq(N, K, 4)
    y = ops.gemv4_glu(x, q, e, R, lb, kw)
    r = ref.silu_mul((x.float() @ wd.float().t()).bfloat16(), interleaved=True).float()
    assert y.shape == (1, N // 2) and y.dtype == torch.bfloat16
    assert (y.float() - r).abs().max().item() <= 2e-2 * r.abs().max().item() + 1e-3


def _xn_inputs(H, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    Pin = torch.randn(3, 1, H, device="cuda", generator=g)
    res = torch.randn(1, H, device="cuda", generator=g).to(torch.bfloat16)
    gamma = (1 + 0.1 * torch.randn(H, device="cuda", generator=g)).to(torch.bfloat16)
    return Pin, res, gamma


@pytest.mark.parametrize("N,R,C,lb,kw", [(6144, 16, 1, 32, 2)]
                         + [(2 * R, R, C, lb, kw) for (R, C, lb, kw) in ops.GEMV4_XN_CASES])
def test_gemv4_xn_slabs_match_bf16_gemv_prologue(native, N, R, C, lb, kw):
    """Same input-row arithmetic as the bf16 gemv_partial_xn: the same residual out, products
    equal up to the dot-product order."""
    H = _kmin(C, lb, kw)
    Pin, res, gamma = _xn_inputs(H, 3)
    q, e, wd = _wq(N, H, 5)
    r1, r2 = torch.empty_like(res), torch.empty_like(res)
    a = ops.gemv4_partial_xn(Pin, res, r1, gamma, 1e-5, q, e, 1, R, lb, kw).sum(0)
    b = ops.gemv_partial_xn(Pin, res, r2, gamma, 1e-5, wd, 1, 8).sum(0)
    assert torch.equal(r1, r2)
    assert (a.float() - b.float()).abs().max().item() <= 1e-2 * b.float().abs().max().item() + 1e-3


@pytest.mark.parametrize("N,H,R,lb,kw", [(28672, 4096, 16, 32, 2), (64, 2048, 16, 32, 1)]
                         + [(2 * R, _kmin(C, lb, kw), R, lb, kw) for (R, C, lb, kw) in ops.GEMV4_EPI_CASES])
def test_gemv4_xn_glu_matches_bf16_gemv_prologue(native, N, H, R, lb, kw):
    Pin, res, gamma = _xn_inputs(H, 6)
    q, e, wd = _wq(N, H, 7)
    r1, r2 = torch.empty_like(res), torch.empty_like(res)
    a = ops.gemv4_glu_xn(Pin, res, r1, gamma, 1e-5, q, e, R, lb, kw)
    b = ops.gemv_glu_xn(Pin, res, r2, gamma, 1e-5, wd)
    assert torch.equal(r1, r2)
    assert (a.float() - b.float()).abs().max().item() <= 1e-2 * b.float().abs().max().item() + 1e-3


@pytest.mark.parametrize("N,K,n_valid,R,lb,kw", [(4096, 4096, 1000, 16, 32, 2), (32000, 2048, 31990, 16, 32, 1),
                                                 (4096, 4096, 1000, 32, 32, 2), (32000, 2048, 31990, 32, 32, 1),
                                                 (4096, 4096, 1000, 16, 16, 4), (4096, 4096, 1000, 0, 0, 0)])
def test_gemv4_argmax_matches_bf16_logits(native, N, K, n_valid, R, lb, kw):
    """LM head + greedy pick over MXFP4 weights == argmax of the bf16 fp32-accumulated logits of
    the dequantized weights over the valid vocabulary.  The planted rows are written as codes
    and scales: the winner at the last valid id, a rival at id 5 with the SAME codes and ONE
    block's scale halved (the winner wins by that block scale only, and a dropped scale would
    tie towards the lower id), and a row with every scale doubled just past n_valid that must be
    ignored."""
    x = _x(K, 2)
    q0, e0, _ = _wq(N, K, 8)
    q, e = q0.clone(), e0.clone()
    # magnitude 0.5 (code 1) everywhere but block 17, which holds 6 (code 7) and so carries
    # 4 .. 9 % of the logit -- well above the bf16 rounding of the logits (2^-8 relative) when its
    # scale is halved; signs follow x (bit 3), packed two per byte
    mag = torch.ones(K, device="cuda", dtype=torch.uint8)
    mag[17 * 32:18 * 32] = 7
    c = (mag | ((x[0] < 0).to(torch.uint8) << 3)).view(K // 2, 2)
    codes = c[:, 0] | (c[:, 1] << 4)
    # 2^-4: the planted logits (about 19 and 35) stand clear of the random rows' (|.| < 8)
    for row, eb in ((n_valid - 1, 123), (5, 123), (n_valid, 124)):
        q[row] = codes
        e[row] = eb
    e[5, 17] = 122                        # the rival: one block's scale halved
    wd = ops.dequantize_mxfp4_rows(q, e, torch.bfloat16)
    logits = (x.float() @ wd[:n_valid].float().t()).bfloat16().float()
    assert int(logits.argmax(1)[0]) == n_valid - 1
    assert float(logits[0, n_valid - 1]) > float(logits[0, 5])        # survives the bf16 rounding
    if R:
        ids, vals = torch.ops.docqa.gemv4_argmax_val(x, q, e, n_valid, R, lb, kw)
    else:   # the public wrapper: the MXFP4 kernel where the shape is planned, else W' on the bf16 GEMV
        ids, vals = ops.lm_head_argmax(x, wd, n_valid, with_values=True, mxfp4=(q, e))
    assert int(ids[0]) == n_valid - 1
    assert abs(float(vals[0]) - float(logits.max())) <= 1e-2 * abs(float(logits.max()))
    # ties go to the lowest id: with equal scales the rival at id 5 is picked
    e[5, 17] = 123
    R2, lb2, kw2 = (R, lb, kw) if R else (16, 32, 2)
    ids2, _ = torch.ops.docqa.gemv4_argmax_val(x, q, e, n_valid, R2, lb2, kw2)
    assert int(ids2[0]) == 5


# ----------------------------------------------------------------------------- model
@pytest.fixture(scope="module")
def qmodel(native):
    from docqa_amd.models.llama import LlamaConfig, LlamaModel

    m = LlamaModel(LlamaConfig.preset("llama3-1b-test"), device="cuda", seed=17)
    m.quantize_mxfp4()
    return m


def test_quantized_model_holds_mxfp4_copies(qmodel):
    L0 = qmodel.layers[0]
    assert qmodel.weight_format == "mxfp4"
    q, e = qmodel.mx4[0]["down"]
    assert q.is_cuda and q.dtype == torch.uint8 and e.dtype == torch.uint8
    assert torch.equal(ops.dequantize_mxfp4_rows(q, e, torch.bfloat16), L0["down"])
    assert ops.gemv4_glu_ok(1, *L0["gate_up"].shape)          # the chain the decode tests count


def test_llama_batch1_decode_on_mxfp4_plans(native, qmodel):
    """One-row decode steps of the quantized Llama test preset stream the MXFP4 copies and track
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
    orig = ops.gemv4_glu_xn
    try:
        ops.gemv4_glu_xn = lambda *a, **k: (called.append(1), orig(*a, **k))[1]
        d1 = _decode_logits(m, kv1, prompts, tables, [4], BS)
    finally:
        ops.gemv4_glu_xn = orig
    assert len(called) == m.cfg.layers          # the step really ran on the MXFP4 chain
    with native.use_reference():
        _prefill_logits(m, kv2, prompts, BS)
        d2 = _decode_logits(m, kv2, prompts, tables, [4], BS)
    assert _rel(d1, d2) < 0.03


def test_llama_batch1_mxfp4_step_in_a_graph_equals_eager(native, qmodel):
    """The same decode step captured into a graph and replayed gives the eager logits, and the
    fused LM-head pick lands on a maximal logit."""
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
