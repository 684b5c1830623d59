"""FP8 weight streaming at 33..128 decode rows, the parts that need no GPU: the plan functions of
the wide kernel family (row range, K granule, the DOCQA_DGEMM8W knob), the shipped tables (served
shapes only), LlamaModel._step_plan naming the "streamed_wide" family, the CPU fallbacks of the
wrappers, and a quantized model's 40-row CPU decode against a plain model loaded with the image W'."""
import os
import subprocess
import sys
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

from docqa_amd import ops
from docqa_amd.models.llama import AttnMeta, LlamaConfig, LlamaModel, Streamed

ROOT = Path(__file__).resolve().parent.parent
BUCKETS = (64, 128)
PROJ = ("qkv", "o", "down")


@pytest.fixture
def listed(monkeypatch):
    """Plan tables listing a few shapes, whatever the probe shipped."""
    monkeypatch.setattr(ops, "_DGEMM8W", True)
    monkeypatch.setattr(ops, "_DGEMM8W_SLAB", {(4096, 4096): {64: (8, 128), 128: (4, 128)},
                                               (4096, 14336): {64: (7, 128)},
                                               (4096, 4352): {64: (1, 128), 128: (1, 128)},     # K = 8.5 granules
                                               (6144, 4096): {64: (16, 128), 128: (4, 64)}})     # bad split / tile
    monkeypatch.setattr(ops, "_DGEMM8W_GLU", {(28672, 4096): (64,), (28672, 4352): BUCKETS, (28704, 4096): BUCKETS})
    monkeypatch.setattr(ops, "_DGEMM8W_LM", {(128256, 4096): BUCKETS})


def test_plan_functions_row_range_and_granule(listed):
    assert ops.DGEMM8W_MAX_ROWS == 128 and ops.DGEMM8W_K == 512 and ops.DGEMM8W_TILE == 128
    assert ops.DGEMM8_MAX_ROWS == 32                                  # the ring kernel's range is untouched
    off = (0, 128)
    assert ops.dgemm8w_plan(32, 4096, 4096) == off                    # the ring kernel's rows
    assert ops.dgemm8w_plan(33, 4096, 4096) == (8, 128)               # bucket 64
    assert ops.dgemm8w_plan(64, 4096, 4096) == (8, 128)
    assert ops.dgemm8w_plan(65, 4096, 4096) == (4, 128)               # bucket 128
    assert ops.dgemm8w_plan(128, 4096, 4096) == (4, 128)
    assert ops.dgemm8w_plan(129, 4096, 4096) == off
    assert ops.dgemm8w_plan(1, 4096, 4096) == off and ops.dgemm8w_plan(2, 4096, 4096) == off
    assert ops.dgemm8w_plan(40, 4096, 14336) == (7, 128)
    assert ops.dgemm8w_plan(100, 4096, 14336) == off                  # bucket 128 is not listed
    assert ops.dgemm8w_plan(40, 4096, 4352) == off                    # listed, but K is not whole turns
    assert ops.dgemm8w_plan(40, 6144, 4096) == off                    # listed split leaves half a turn per slice
    assert ops.dgemm8w_plan(100, 6144, 4096) == off                   # a tile the kernel does not have
    assert ops.dgemm8w_plan(40, 2048, 4096) == off                    # not listed: stays on W'
    assert not ops.dgemm8w_glu_ok(32, 28672, 4096) and ops.dgemm8w_glu_ok(33, 28672, 4096)
    assert ops.dgemm8w_glu_ok(64, 28672, 4096) and not ops.dgemm8w_glu_ok(65, 28672, 4096)   # bucket 128 not listed
    assert not ops.dgemm8w_glu_ok(40, 28672, 4352)                    # K not whole turns
    assert not ops.dgemm8w_glu_ok(40, 28704, 4096)                    # N not whole 128-row tiles
    assert not ops.dgemm8w_glu_ok(40, 14336, 4096)                    # not listed
    assert not ops.dgemm8w_argmax_ok(32, 128256, 4096) and not ops.dgemm8w_argmax_ok(129, 128256, 4096)
    assert ops.dgemm8w_argmax_ok(33, 128256, 4096) and ops.dgemm8w_argmax_ok(128, 128256, 4096)
    assert not ops.dgemm8w_argmax_ok(40, 32768, 4096)                 # not listed
    # the dispatch: "wide" is tried last and only FP8 has it
    assert ops._KINDS == ("gemv", "ring", "wide")
    assert ops.STREAMED["fp8-e4m3"].wide == "dgemm8w" and ops.STREAMED["mxfp4"].wide == ""
    assert ops.STREAMED["fp8-e4m3"].max_rows == 128 and ops.STREAMED["mxfp4"].max_rows == 32
    assert ops.streamed_plan("fp8-e4m3", 40, 4096, 4096) == ("wide", 8, 128)
    assert ops.streamed_plan("fp8-e4m3", 129, 4096, 4096) == ("", 0, 0)
    assert ops.streamed_plan("mxfp4", 40, 4096, 4096) == ("", 0, 0)
    assert ops.streamed_glu_kind("fp8-e4m3", 40, 28672, 4096) == "wide"
    assert ops.streamed_glu_kind("mxfp4", 40, 28672, 4096) == ""


def test_knob_disables_every_plan():
    code = ("from docqa_amd import ops\n"
            "ops._DGEMM8W_SLAB[(4096, 4096)] = {64: (8, 128)}\nops._DGEMM8W_GLU[(128, 1024)] = (64,)\n"
            "ops._DGEMM8W_LM[(128, 1024)] = (64,)\nops._DGEMM8_SLAB[(4096, 4096)] = (2,)\n"
            "print(ops.dgemm8w_plan(40, 4096, 4096)[0], int(ops.dgemm8w_glu_ok(40, 128, 1024)), "
            "int(ops.dgemm8w_argmax_ok(40, 128, 1024)), ops.dgemm8_plan(2, 4096, 4096)[0])")
    out = {}
    for knob in ("0", "1"):
        env = {**os.environ, "DOCQA_DGEMM8W": knob, "PYTHONPATH": str(ROOT)}
        out[knob] = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True,
                                   check=True).stdout.split()
    assert out["0"] == ["0", "0", "0", "4"] and out["1"] == ["8", "1", "1", "4"]


def _preset_shapes(preset):
    cfg = LlamaConfig.preset(preset)
    H, D = cfg.hidden, cfg.head_dim
    return {"qkv": ((cfg.heads + 2 * cfg.kv_heads) * D, H), "o": (H, cfg.heads * D),
            "gate_up": (2 * cfg.intermediate, H), "down": (H, cfg.intermediate), "lm_head": (cfg.vocab_size, H)}


def test_shipped_tables_list_only_served_shapes_the_kernel_takes():
    test_shapes = {s for p in ("tiny", "llama3-1b-test") for s in _preset_shapes(p).values()}
    for table in (ops._DGEMM8W_SLAB, ops._DGEMM8W_GLU, ops._DGEMM8W_LM):
        for (N, K), buckets in table.items():
            assert N % ops.DGEMM8W_TILE == 0 and K % ops.DGEMM8W_K == 0
            assert set(buckets) <= set(BUCKETS) and buckets
            assert (N, K) not in test_shapes
    for (N, K), entry in ops._DGEMM8W_SLAB.items():
        for b, (S, t) in entry.items():
            assert t == ops.DGEMM8W_TILE and S >= 1 and K % S == 0 and (K // S) % ops.DGEMM8W_K == 0
            assert ops.dgemm8w_plan(b, N, K) == (S, t) or not ops._DGEMM8W


# ----------------------------------------------------------------------------- _step_plan
def _shape_model(fmt: str) -> LlamaModel:
    """``llama3-1b-test`` shapes only (meta tensors), as tests/test_step_plan_cpu.py."""
    cfg = LlamaConfig.preset("llama3-1b-test")
    m = LlamaModel(cfg, device="cpu", init=False)
    sh = _preset_shapes("llama3-1b-test")
    m.layers = [{k: torch.empty(sh[k], device="meta") for k in PROJ + ("gate_up",)}]
    if fmt != "bf16":
        m.streamed = Streamed(fmt, [], ())
    return m


def _meta() -> AttnMeta:
    return AttnMeta(prefill=False, positions=None, slot_mapping=None)


@pytest.fixture
def preset_listed(monkeypatch):
    sh = _preset_shapes("llama3-1b-test")
    monkeypatch.setattr(ops, "_DGEMM8W", True)
    monkeypatch.setattr(ops, "_DGEMM8W_SLAB", {sh[k]: {b: (2, 128) for b in BUCKETS} for k in PROJ})
    monkeypatch.setattr(ops, "_DGEMM8W_GLU", {sh["gate_up"]: BUCKETS})
    monkeypatch.setattr(ops, "_DGEMM8W_LM", {sh["lm_head"]: BUCKETS})
    return sh


def test_step_plan_names_the_wide_family(preset_listed):
    m = _shape_model("fp8-e4m3")
    for M in (33, 64, 100, 128):
        plan = m._step_plan(M, _meta(), True, False)
        for k in PROJ:
            assert plan.proj[k] == ("streamed_wide", 2, 128, False), (M, k)
            assert plan.streamed[k] == "wide"
        assert plan.glu == ("streamed_wide",) and plan.streamed["gate_up"] == "wide"
        assert not plan.xn and not plan.nf
    plan = m._step_plan(129, _meta(), True, False)
    fams = [p[0] for p in plan.proj.values()] + [plan.glu[0]]
    assert not plan.streamed and not any(f.startswith("streamed_") for f in fams)
    for fmt in ("mxfp4", "bf16"):
        o = _shape_model(fmt)
        for M in (33, 64, 100, 128, 129):
            plan = o._step_plan(M, _meta(), True, False)
            fams = [p[0] for p in plan.proj.values()] + [plan.glu[0]]
            assert not plan.streamed and not any(f.startswith("streamed_") for f in fams), (fmt, M)


def test_knob_flag_off_gives_the_plain_models_plan(preset_listed, monkeypatch):
    m, plain = _shape_model("fp8-e4m3"), _shape_model("bf16")
    assert m._step_plan(40, _meta(), True, False).streamed
    monkeypatch.setattr(ops, "_DGEMM8W", False)
    for M in (33, 64, 100, 128, 129):
        assert m._step_plan(M, _meta(), True, False) == plain._step_plan(M, _meta(), True, False)


def test_shipped_tables_leave_the_test_presets_on_the_image():
    m = _shape_model("fp8-e4m3")
    for M in (33, 64, 100, 128):
        assert not m._step_plan(M, _meta(), True, False).streamed
    assert not ops.dgemm8w_argmax_ok(40, *_preset_shapes("llama3-1b-test")["lm_head"])


# ----------------------------------------------------------------------------- CPU wrappers
def test_wrappers_on_cpu_use_dequantized_weights(listed):
    g = torch.Generator().manual_seed(5)
    K, N, M = 1024, 128, 40
    w = (torch.randn(N, K, generator=g) * 0.02).bfloat16()
    q, s = ops.quantize_fp8_rows(w)
    wd = ops.dequantize_fp8_rows(q, s, torch.bfloat16)
    x = torch.randn(M, K, generator=g).bfloat16()
    P = ops.dgemm8w_partial(x, q, s, 2)
    assert P.shape == (2, M, N) and torch.equal(P, ops.dgemm_partial(x, wd, 2))
    assert torch.equal(ops.dgemm8w_glu(x, q, s), ops.glu_linear(x, wd))
    ids = ops.lm_head_argmax(x, wd, N - 3, fp8=(q, s))
    assert ids.shape == (M,) and torch.equal(ids, F.linear(x, wd[: N - 3]).float().argmax(1))


def _decode40(m):
    """Prefill 40 prompts, then one 40-row decode step on the CPU; the step's logits."""
    from docqa_amd.engine.kv_cache import KVCache

    BS = 16
    lens = [23, 9, 30, 15, 16, 5, 31, 12] * 5
    kv = KVCache(m.cfg.layers, 120, m.hkv, m.cfg.head_dim, BS, device="cpu", dtype=m.dtype).caches
    g = torch.Generator().manual_seed(4)
    tables, nb = [], 0
    for n in lens:
        p = torch.randint(0, m.cfg.vocab_size, (n,), generator=g).tolist()
        blocks = list(range(nb, nb + n // BS + 1))
        nb += len(blocks)
        tables.append(blocks)
        meta = AttnMeta(prefill=True, positions=torch.arange(n, dtype=torch.int32),
                        slot_mapping=torch.tensor([blocks[t // BS] * BS + t % BS for t in range(n)], dtype=torch.int32),
                        cu_seqlens=torch.tensor([0, n], dtype=torch.int32), max_len=n)
        m.forward(torch.tensor(p, dtype=torch.int32), meta, kv)
    maxb = max(len(t) for t in tables)
    bt = torch.zeros(len(lens), maxb, dtype=torch.int32)
    for i, t in enumerate(tables):
        bt[i, :len(t)] = torch.tensor(t)
    meta = AttnMeta(prefill=False, positions=torch.tensor(lens, dtype=torch.int32),
                    slot_mapping=torch.tensor([tables[i][n // BS] * BS + n % BS for i, n in enumerate(lens)],
                                              dtype=torch.int32),
                    block_tables=bt, context_lens=torch.tensor([n + 1 for n in lens], dtype=torch.int32),
                    max_context=maxb * BS)
    return m.forward(torch.arange(4, 44, dtype=torch.int32), meta, kv)


def test_quantized_cpu_model_40_row_decode_equals_plain_model_on_the_image(monkeypatch):
    cfg = LlamaConfig.preset("tiny")
    m = LlamaModel(cfg, device="cpu", seed=3)
    m.quantize_fp8()
    p = LlamaModel(cfg, device="cpu", init=False)
    p.load_state_dict_hf(m.export_state_dict_hf())
    assert p.fp8 is None
    sh = _preset_shapes("tiny")       # even with its shapes listed the CPU never streams
    monkeypatch.setattr(ops, "_DGEMM8W_SLAB", {sh[k]: {b: (1, 128) for b in BUCKETS} for k in PROJ})
    monkeypatch.setattr(ops, "_DGEMM8W_GLU", {sh["gate_up"]: BUCKETS})
    calls = []
    for name in ("dgemm8w_partial", "dgemm8w_glu"):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **k: calls.append(_n))
    a = _decode40(m)
    assert a.shape == (40, cfg.vocab_size) and not calls
    assert torch.equal(a, _decode40(p))
