"""FP8 weight format (per-row OCP e4m3fn codes + power-of-two scales) on the CPU: the
quantizer's invariants, the quantized model against a plain model loaded with its exported
bf16 image, the FP8 ops wrappers' CPU dispatch, and the option's way through resolve_llama,
tensor parallelism and the Ollama /api/tags endpoint."""
import math

import pytest
import torch
import torch.nn.functional as F

from docqa_amd import ops
from docqa_amd.models.llama import AttnMeta, LlamaConfig, LlamaModel
from docqa_amd.ops import reference as ref


def _codes(q):
    return q.view(torch.uint8)


def _rows(n=64, k=512, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, k, generator=g) * 0.02


def test_scales_are_powers_of_two_and_codes_finite():
    w = _rows()
    q, s = ops.quantize_fp8_rows(w)
    assert q.dtype == torch.float8_e4m3fn and q.shape == w.shape
    assert s.dtype == torch.float32 and s.shape == (w.shape[0],)
    m, _ = torch.frexp(s)
    assert torch.all(m == 0.5)                       # exact powers of two
    c = _codes(q)
    assert not torch.any((c == 0x7F) | (c == 0xFF))  # never a NaN code
    # the row maximum uses the top binade of the format
    amax = w.abs().amax(1)
    assert torch.all(amax / s > 232) and torch.all(amax / s <= 464)
    top = q.float().abs().amax(1)
    assert torch.all(top >= 240) and torch.all(top <= 448)
    # round to nearest: every element within half a code step (relative 2^-4 for normals)
    err = (q.float() * s[:, None] - w).abs()
    assert torch.all(err <= w.abs() / 16 + s[:, None] * 2.0 ** -10)


def test_scale_formula_on_known_rows():
    w = torch.zeros(6, 16)
    w[0, 3] = 448.0                 # amax exactly 448 * 2^0
    w[1, 3] = -448.0 * 2.0 ** -7    # exactly 448 * 2^-7
    w[2, 3] = 449.0 * 4             # just above 448 * 2^2: rounds to the top code, same scale
    w[3, 3] = 470.0                 # past the rounding boundary 464: next scale
    w[4, 3] = 0.02
    # row 5 stays all zero
    q, s = ops.quantize_fp8_rows(w)
    assert s.tolist() == [1.0, 2.0 ** -7, 4.0, 2.0, 2.0 ** math.ceil(math.log2(0.02 / 448)), 1.0]
    assert q.float()[0, 3] == 448 and q.float()[1, 3] == -448 and q.float()[2, 3] == 448
    assert q.float()[3, 3] == 240   # 470 / 2 = 235 -> 240
    assert torch.all(_codes(q)[5] == 0) and torch.all(ops.dequantize_fp8_rows(q, s)[5] == 0)


def test_outlier_row_saturates_without_nan():
    w = _rows(4, 256, seed=1)
    w[0, 7] = 3.0e30
    w[1, 9] = -3.0e30
    w[2, 0] = 463.9               # rounds / saturates to +448 at scale 1
    q, s = ops.quantize_fp8_rows(w)
    c = _codes(q)
    assert not torch.any((c == 0x7F) | (c == 0xFF))
    d = ops.dequantize_fp8_rows(q, s, torch.float32)
    assert torch.isfinite(d).all()
    assert d[0, 7] <= 448 * s[0] and d[0, 7] >= 240 * s[0]
    assert d[1, 9] >= -448 * s[1] and d[1, 9] <= -240 * s[1]
    assert s[2] == 1.0 and d[2, 0] == 448.0
    # everything else in the outlier rows underflows to zero instead of turning into garbage
    assert torch.count_nonzero(d[0]) == 1 and torch.count_nonzero(d[1]) == 1


def test_bf16_image_is_exact_and_requantizes_to_itself():
    w = _rows(64, 4096, seed=2)
    w[5] *= 2.0 ** -3
    w[6] *= 2.0 ** 5
    q, s = ops.quantize_fp8_rows(w)
    exact = q.float() * s[:, None]
    img = ops.dequantize_fp8_rows(q, s, torch.bfloat16)
    assert img.dtype == torch.bfloat16 and torch.equal(img.float(), exact)
    assert torch.equal(exact.bfloat16().float(), exact)
    assert torch.equal(ops.dequantize_fp8_rows(_codes(q), s, torch.float32), exact)   # uint8 codes
    q2, s2 = ops.quantize_fp8_rows(img)
    assert torch.equal(s2, s) and torch.equal(_codes(q2), _codes(q))
    # ... including a row whose maximum lands just above a binade edge (amax / s in (224, 232])
    e = torch.zeros(1, 16)
    e[0, 0], e[0, 1] = 0.9 * 2.0 ** -4, 0.01       # 0.9 * 2^-4 / 448 -> s0 = 2^-12, amax / s0 = 230.4
    qe, se = ops.quantize_fp8_rows(e)
    qe2, se2 = ops.quantize_fp8_rows(ops.dequantize_fp8_rows(qe, se))
    assert torch.equal(se2, se) and torch.equal(_codes(qe2), _codes(qe))


# ----------------------------------------------------------------------------- model
def _meta(n):
    pos = torch.arange(n, dtype=torch.int32)
    return AttnMeta(prefill=True, positions=pos, slot_mapping=pos.clone(),
                    cu_seqlens=torch.tensor([0, n], dtype=torch.int32), max_len=n)


def _kv(m, blocks=4, bs=16):
    from docqa_amd.engine.kv_cache import KVCache

    return KVCache(m.cfg.layers, blocks, m.hkv, m.cfg.head_dim, bs, device="cpu", dtype=m.dtype).caches


def _forward(m, ids):
    return m.forward(torch.tensor(ids, dtype=torch.int32), _meta(len(ids)), _kv(m))


def test_quantized_model_equals_plain_model_on_exported_image():
    cfg = LlamaConfig.preset("tiny")
    m = LlamaModel(cfg, device="cpu", seed=3)
    plain_bytes = m.weight_bytes()
    assert m.weight_format == "bf16" and m.fp8 is None
    before = m.layers[0]["qkv"].clone()
    m.quantize_fp8()
    assert m.weight_format == "fp8-e4m3" and len(m.fp8) == cfg.layers
    assert not torch.equal(m.layers[0]["qkv"], before)          # the resident weights are W' now
    for L, d in zip(m.layers, m.fp8):
        for k in LlamaModel.FP8_WEIGHTS:
            q, s = d[k]
            assert q.shape == L[k].shape and torch.equal(ops.dequantize_fp8_rows(q, s, m.dtype), L[k])
    assert torch.equal(ops.dequantize_fp8_rows(*m.lm_head_fp8, m.dtype), m.lm_head)
    # the FP8 copies cost memory on top of the bf16 image: one byte per projection weight + scales
    proj = sum(L[k].numel() for L in m.layers for k in LlamaModel.FP8_WEIGHTS) + m.lm_head.numel()
    nscale = sum(L[k].shape[0] for L in m.layers for k in LlamaModel.FP8_WEIGHTS) + m.lm_head.shape[0]
    assert m.weight_bytes() == plain_bytes + proj + 4 * nscale
    ids = torch.randint(0, cfg.vocab_size, (23,), generator=torch.Generator().manual_seed(4)).tolist()
    a = _forward(m, ids)
    p = LlamaModel(cfg, device="cpu", init=False)
    p.load_state_dict_hf(m.export_state_dict_hf())
    assert p.weight_format == "bf16"
    assert torch.equal(a, _forward(p, ids))
    # quantizing the plain copy gives the same codes (the image re-quantizes to itself)
    p.quantize_fp8()
    assert all(torch.equal(_codes(p.fp8[i][k][0]), _codes(m.fp8[i][k][0])) and torch.equal(p.fp8[i][k][1], m.fp8[i][k][1])
               for i in range(cfg.layers) for k in LlamaModel.FP8_WEIGHTS)
    assert torch.equal(a, _forward(p, ids))
    m.quantize_fp8()                                           # idempotent
    assert torch.equal(a, _forward(m, ids))


def test_ops_wrappers_on_cpu_use_dequantized_weights():
    g = torch.Generator().manual_seed(5)
    K, N = 2048, 64
    w = (torch.randn(N, K, generator=g) * 0.02).bfloat16()
    q, s = ops.quantize_fp8_rows(w)
    wd = ops.dequantize_fp8_rows(q, s, torch.bfloat16)
    x = torch.randn(1, K, generator=g).bfloat16()
    r = F.linear(x.float(), wd.float())
    P = ops.gemv8_partial(x, q, s, 1, 16)
    assert P.shape[1:] == (1, N) and torch.allclose(P.float().sum(0), r, rtol=1e-2, atol=1e-3)
    y = ops.gemv8_glu(x, q, s)
    assert torch.equal(y, ref.silu_mul(F.linear(x, wd), interleaved=True))
    Pin = torch.randn(2, 1, K, generator=g)
    res = torch.randn(1, K, generator=g).bfloat16()
    gamma = (1 + 0.1 * torch.randn(K, generator=g)).bfloat16()
    r1, r2 = torch.empty_like(res), torch.empty_like(res)
    a = ops.gemv8_partial_xn(Pin, res, r1, gamma, 1e-5, q, s, 1, 16)
    b = ops.gemv_partial_xn(Pin, res, r2, gamma, 1e-5, wd, 1, 16)
    assert torch.equal(r1, r2) and torch.equal(a.sum(0), b.sum(0))
    a = ops.gemv8_glu_xn(Pin, res, r1, gamma, 1e-5, q, s)
    b = ops.gemv_glu_xn(Pin, res, r2, gamma, 1e-5, wd)
    assert torch.equal(r1, r2) and torch.equal(a, b)
    ids = ops.lm_head_argmax(x, wd, N - 3, fp8=(q, s))
    assert int(ids[0]) == int(F.linear(x, wd[: N - 3]).float().argmax())


def test_plans_name_instantiated_kernels_only():
    for (N, K) in [(6144, 4096), (4096, 4096), (4096, 14336), (3072, 2048), (2048, 2048), (2048, 8192)]:
        S, R = ops.gemv8_plan(1, N, K)
        if S:
            lb = ops.gemv8_lb(K, S)
            assert N % R == 0 and (K // S) % (256 * lb) == 0
            assert (R, K // S // (256 * lb), lb) in ops.GEMV8_CASES
            if K <= 4096:   # these projections also run with the in-kernel input row
                assert (R, K // S // (256 * lb), lb) in ops.GEMV8_XN_CASES
    assert ops.gemv8_plan(2, 4096, 4096) == (0, 0)        # one row only
    assert ops.gemv8_plan(1, 4096, 4096 + 512) == (0, 0)  # no kernel: the caller keeps the bf16 GEMV
    assert ops.gemv8_plan(1, 4100, 4096) == (0, 0)
    assert not ops.gemv8_glu_ok(1, 28672, 3072) and not ops.gemv8_glu_ok(4, 28672, 4096)


def test_tp_refuses_fp8(monkeypatch):
    from docqa_amd.parallel import comm

    m = LlamaModel(LlamaConfig.preset("test-tp8"), device="cpu", init=False)
    m.tp = 2
    with pytest.raises(ValueError, match="tp_size"):
        m.quantize_fp8()
    ps = comm.state()
    monkeypatch.setattr(ps, "tp_size", 2)
    monkeypatch.setenv("DOCQA_LLM_WEIGHTS", "fp8")
    from docqa_amd.models import checkpoint as ck

    with pytest.raises(ValueError, match="tp_size"):
        ck.resolve_llama("test-tp8", device="cpu")


def test_resolve_llama_honours_weights_variable(monkeypatch):
    from docqa_amd.models import checkpoint as ck

    monkeypatch.delenv("DOCQA_LLM_WEIGHTS", raising=False)
    a = ck.resolve_llama("tiny", device="cpu", seed=7)
    assert a.weight_format == "bf16" and a.fp8 is None
    monkeypatch.setenv("DOCQA_LLM_WEIGHTS", "fp8")
    b = ck.resolve_llama("tiny", device="cpu", seed=7)
    assert b.weight_format == "fp8-e4m3"
    q, s = ops.quantize_fp8_rows(a.layers[1]["down"])
    assert torch.equal(b.layers[1]["down"], ops.dequantize_fp8_rows(q, s, torch.bfloat16))
    assert torch.equal(b.embed, a.embed)                     # embedding and norms untouched
    # float32 models are quantized too: the same model on the reference path
    monkeypatch.setenv("DOCQA_LLM_DTYPE", "float32")
    c = ck.resolve_llama("tiny", device="cpu", seed=7)
    assert c.weight_format == "fp8-e4m3" and c.layers[0]["o"].dtype == torch.float32
    q, s = c.fp8[0]["o"]
    assert torch.equal(c.layers[0]["o"], q.float() * s[:, None])
    monkeypatch.setenv("DOCQA_LLM_WEIGHTS", "int3")
    with pytest.raises(ValueError, match="DOCQA_LLM_WEIGHTS"):
        ck.resolve_llama("tiny", device="cpu")


def test_launcher_exposes_llm_weights_flag():
    from docqa_amd.services.launch import build_parser

    assert build_parser().parse_args([]).llm_weights is None
    assert build_parser().parse_args(["--llm-weights", "fp8"]).llm_weights == "fp8"
    with pytest.raises(SystemExit):
        build_parser().parse_args(["--llm-weights", "int4"])


@pytest.mark.parametrize("weights,level", [("fp8", "F8_E4M3"), (None, "BF16")])
def test_api_tags_reports_weight_format(tmp_path, monkeypatch, weights, level):
    from fastapi.testclient import TestClient

    from docqa_amd.config import Settings
    from docqa_amd.services.stack import DocQAStack, StackOptions

    if weights:
        monkeypatch.setenv("DOCQA_LLM_WEIGHTS", weights)
    else:
        monkeypatch.delenv("DOCQA_LLM_WEIGHTS", raising=False)
    st = Settings()
    assert st.llm_weights == (weights or "bf16")
    st.index_dir = str(tmp_path)
    st.default_data_dir = str(tmp_path / "nodata")
    st.database_url = "sqlite://"
    st.max_new_tokens = 3
    s = DocQAStack(StackOptions(llm="tiny", embed="tiny-bert", ner="tiny-bert", device="cpu",
                                max_batch=2, max_context=512, use_graphs=False), st)
    try:
        qa = TestClient(s.qa_app)
        tags = qa.get("/api/tags").json()["models"]
        assert len(tags) == 1 and tags[0]["details"]["quantization_level"] == level
        m = s.pipeline.engine.model
        assert tags[0]["size"] == m.weight_bytes()
        if weights:
            assert m.weight_format == "fp8-e4m3" and tags[0]["size"] > m.cfg.num_params() * 2
        else:
            assert m.weight_format == "bf16" and m.fp8 is None
        # the service answers on the quantized model
        r = qa.post("/api/generate", json={"prompt": "abc", "raw": True, "stream": False,
                                           "options": {"num_predict": 2}})
        assert r.status_code == 200 and r.json()["done"] is True
    finally:
        s.close()
