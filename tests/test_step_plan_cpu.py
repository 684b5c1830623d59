"""LlamaModel._step_plan on the CPU: which kernel family every projection of a step takes, checked
against the public per-format plan functions in their priority order (FP8 / MXFP4 GEMV, then ring,
then the bf16 GEMV, the mid-M GEMM, the skinny kernel), for the step matrix of
tests/native_trace.py -- on ``tiny`` models built per format and shape-only on the
``llama3-1b-test`` shapes, with the shipped ring tables and with every shape listed."""
import pytest
import torch

from docqa_amd import ops
from docqa_amd.models.llama import AttnMeta, LlamaConfig, LlamaModel, Streamed

FORMATS = ("bf16", "fp8-e4m3", "mxfp4")
DECODE_ROWS = (1, 2, 3, 8, 16, 32, 33)
PREFILLS = (100, 600)
PROJ = ("qkv", "o", "down")
_MODELS = {}


def _model(preset: str, fmt: str) -> LlamaModel:
    """``tiny``: a real CPU model, quantized; ``llama3-1b-test``: its shapes only (meta tensors)."""
    if (preset, fmt) not in _MODELS:
        cfg = LlamaConfig.preset(preset)
        if preset == "tiny":
            m = LlamaModel(cfg, device="cpu", seed=3)
            {"bf16": lambda: None, "fp8-e4m3": m.quantize_fp8, "mxfp4": m.quantize_mxfp4}[fmt]()
        else:
            m = LlamaModel(cfg, device="cpu", init=False)
            H, D = cfg.hidden, cfg.head_dim
            shapes = {"qkv": ((m.hq + 2 * m.hkv) * D, H), "o": (H, m.hq * D), "gate_up": (2 * m.inter, H),
                      "down": (H, m.inter)}
            m.layers = [{k: torch.empty(s, device="meta") for k, s in shapes.items()}]
            if fmt != "bf16":
                m.streamed = Streamed(fmt, [], ())
        assert m.weight_format == fmt
        _MODELS[(preset, fmt)] = m
    return _MODELS[(preset, fmt)]


def _meta(prefill: bool) -> AttnMeta:
    return AttnMeta(prefill=prefill, positions=None, slot_mapping=None)


def _list_all(monkeypatch, m):
    b = (2, 4, 8, 16, 32)
    L0 = m.layers[0]
    for d in "84":
        monkeypatch.setattr(ops, f"_DGEMM{d}_SLAB", {tuple(L0[k].shape): b for k in PROJ})
        monkeypatch.setattr(ops, f"_DGEMM{d}_GLU", {tuple(L0["gate_up"].shape): b})


def _expected_proj(fmt, M, N, K):
    """(family, S, rows | tile | cfg) from the public plan functions, today's priority order."""
    gemv, ring = {"fp8-e4m3": (ops.gemv8_plan, ops.dgemm8_plan), "mxfp4": (ops.gemv4_plan, ops.dgemm4_plan),
                  "bf16": (None, None)}[fmt]
    if gemv is not None and 1 <= M <= 32:
        for fam, fn in (("streamed_gemv", gemv), ("streamed_ring", ring)):
            S, r = fn(M, N, K)
            if S:
                return fam, S, r
    for fam, fn in (("gemv", ops.gemv_plan), ("mgemm", ops.mid_plan), ("dgemm", ops.decode_plan)):
        S, r = fn(M, N, K)
        if S or fam == "dgemm":
            return fam, S, r


def _expected_glu(fmt, M, N, K):
    ok = {"fp8-e4m3": (ops.gemv8_glu_ok, ops.dgemm8_glu_ok), "mxfp4": (ops.gemv4_glu_ok, ops.dgemm4_glu_ok)}.get(fmt)
    if ok and ok[0](M, N, K):
        return "streamed_gemv"
    if ok and ok[1](M, N, K):
        return "streamed_ring"
    return None


@pytest.mark.parametrize("tables", ["shipped", "listed"])
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("preset", ["tiny", "llama3-1b-test"])
def test_decode_plans_follow_the_public_plan_functions(monkeypatch, preset, fmt, tables):
    m = _model(preset, fmt)
    if tables == "listed":
        _list_all(monkeypatch, m)
    L0 = m.layers[0]
    streamed_seen = 0
    for M in DECODE_ROWS:
        plan = m._step_plan(M, _meta(False), True, False)
        for k in PROJ:
            assert plan.proj[k][:3] == _expected_proj(fmt, M, *L0[k].shape), (M, k, plan.proj[k])
            assert (k in plan.streamed) == plan.proj[k][0].startswith("streamed_")
        want = _expected_glu(fmt, M, *L0["gate_up"].shape)
        if want:
            assert plan.glu == (want,) and plan.streamed["gate_up"] == want[9:]
        else:
            assert not plan.glu[0].startswith("streamed_") and "gate_up" not in plan.streamed
        streamed_seen += len(plan.streamed)
        if M > 32 or fmt == "bf16":
            assert not plan.streamed
        assert not (plan.xn and M != 1)
    if preset == "llama3-1b-test" and fmt != "bf16" and tables == "listed":
        assert streamed_seen >= 4 * 5        # every projection of every 2..32-row step at least


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("preset", ["tiny", "llama3-1b-test"])
def test_prefills_never_stream(preset, fmt):
    m = _model(preset, fmt)
    L0 = m.layers[0]
    for M in PREFILLS:
        plan = m._step_plan(M, _meta(True), True, False)
        assert not plan.streamed and not plan.xn and not plan.nf
        fams = [p[0] for p in plan.proj.values()] + [plan.glu[0]]
        assert not any(f.startswith("streamed_") for f in fams)
    small = m._step_plan(100, _meta(True), True, False)
    for k in PROJ:       # a short prefill takes the decode projection plans on the bf16 image
        assert small.proj[k][:3] == _expected_proj("bf16", 100, *L0[k].shape)
    mid = m._step_plan(600, _meta(True), True, False)
    for k in PROJ:
        S, c = ops.prefill_plan(600, *L0[k].shape)
        Sp = ops.prefill_split_plan(600, *L0[k].shape)
        want = ("mgemm", S, c) if S >= 2 else ("pgemm", Sp, 0) if not S and Sp else None
        assert (mid.proj[k][:3] if k in mid.proj else None) == want


@pytest.mark.parametrize("fmt", ["fp8-e4m3", "mxfp4"])
def test_knobs_off_send_every_projection_back_to_bf16(monkeypatch, fmt):
    m, plain = _model("llama3-1b-test", fmt), _model("llama3-1b-test", "bf16")
    _list_all(monkeypatch, m)
    assert any(m._step_plan(M, _meta(False), True, False).streamed for M in DECODE_ROWS)
    for flag in ("_GEMV8", "_GEMV4", "_DGEMM8", "_DGEMM4"):
        monkeypatch.setattr(ops, flag, False)
    for M in DECODE_ROWS:
        assert m._step_plan(M, _meta(False), True, False) == plain._step_plan(M, _meta(False), True, False)
        assert not m._step_plan(M, _meta(False), True, False).streamed


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("preset", ["tiny", "llama3-1b-test"])
def test_cpu_steps_and_plain_models_never_name_a_streamed_family(monkeypatch, preset, fmt):
    m = _model(preset, fmt)
    _list_all(monkeypatch, m)
    for M in DECODE_ROWS + PREFILLS:
        for prefill in (False, True):
            for on_gpu in ((False,) if fmt != "bf16" else (False, True)):
                plan = m._step_plan(M, _meta(prefill), on_gpu, False)
                fams = [p[0] for p in plan.proj.values()] + [plan.glu[0]]
                assert not plan.streamed and not any(f.startswith("streamed_") for f in fams), (M, prefill, on_gpu)
