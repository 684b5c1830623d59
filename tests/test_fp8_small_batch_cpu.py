"""FP8 weight streaming at 2..32 decode rows, the parts that need no GPU: the plan functions
(row range, K granule, the DOCQA_DGEMM8 knob), the CPU fallbacks of the wrappers, and a
quantized model's few-row CPU decode against a plain model loaded with the image W'."""
import os
import subprocess
import sys
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

from docqa_amd import ops
from docqa_amd.models.llama import AttnMeta, LlamaConfig, LlamaModel

ROOT = Path(__file__).resolve().parent.parent
BUCKETS = (2, 4, 8, 16, 32)


@pytest.fixture
def listed(monkeypatch):
    """Plan tables listing one shape at every bucket, whatever the probe shipped."""
    monkeypatch.setattr(ops, "_DGEMM8", True)
    monkeypatch.setattr(ops, "_DGEMM8_SLAB", {(4096, 4096): BUCKETS, (4096, 14336): BUCKETS, (4096, 4608): BUCKETS})
    monkeypatch.setattr(ops, "_DGEMM8_GLU", {(28672, 4096): (2, 8)})
    monkeypatch.setattr(ops, "_DGEMM8_LM", {(128256, 4096): BUCKETS})


def test_plan_functions_row_range_and_granule(listed):
    top = ops.DGEMM8_MAX_ROWS
    assert top == 32 and ops.DGEMM8_K == 1024
    assert ops.dgemm8_plan(1, 4096, 4096) == (0, 64)              # one row: the GEMV's
    assert ops.dgemm8_plan(2, 4096, 4096) == (4, 64)              # 64 tiles x 4 slices of one ring turn
    assert ops.dgemm8_plan(top, 4096, 4096) == (4, 64)
    assert ops.dgemm8_plan(top + 1, 4096, 4096) == (0, 64)
    assert ops.dgemm8_plan(5, 4096, 14336) == (7, 64)             # 14 turns: 2 slices give 128 workgroups, 7 give 448
    assert ops.dgemm8_plan(2, 4096, 4608) == (0, 64)              # listed, but K is not whole ring turns
    assert ops.dgemm8_plan(2, 6144, 4096) == (0, 64)              # not listed: stays on W'
    assert not ops.dgemm8_glu_ok(1, 28672, 4096) and ops.dgemm8_glu_ok(2, 28672, 4096)
    assert not ops.dgemm8_glu_ok(3, 28672, 4096)                  # bucket 4 is not listed
    assert ops.dgemm8_glu_ok(5, 28672, 4096) and not ops.dgemm8_glu_ok(9, 28672, 4096)
    assert not ops.dgemm8_argmax_ok(1, 128256, 4096) and not ops.dgemm8_argmax_ok(top + 1, 128256, 4096)
    assert ops.dgemm8_argmax_ok(2, 128256, 4096) and ops.dgemm8_argmax_ok(top, 128256, 4096)
    # the split rule alone: smallest S of whole ring turns with >= 192 workgroups, else all turns
    assert ops.dgemm8_splits(6144, 4096) == 2 and ops.dgemm8_splits(2048, 2048) == 2
    assert ops.dgemm8_splits(28672, 4096) == 1 and ops.dgemm8_splits(4096, 4096 + 512) == 0
    assert ops.dgemm8_splits(4100, 4096) == 0


def test_shipped_tables_list_only_shapes_the_kernel_takes():
    for table in (ops._DGEMM8_SLAB, ops._DGEMM8_GLU, ops._DGEMM8_LM):
        for (N, K), buckets in table.items():
            assert N % 64 == 0 and K % ops.DGEMM8_K == 0 and ops.dgemm8_splits(N, K) >= 1
            assert set(buckets) <= set(BUCKETS)


def test_knob_disables_every_plan():
    code = ("from docqa_amd import ops\n"
            "ops._DGEMM8_SLAB[(4096, 4096)] = (2,)\nops._DGEMM8_GLU[(128, 1024)] = (2,)\n"
            "ops._DGEMM8_LM[(128, 1024)] = (2,)\n"
            "print(ops.dgemm8_plan(2, 4096, 4096)[0], int(ops.dgemm8_glu_ok(2, 128, 1024)), "
            "int(ops.dgemm8_argmax_ok(2, 128, 1024)))")
    out = {}
    for knob in ("0", "1"):
        env = {**os.environ, "DOCQA_DGEMM8": knob, "PYTHONPATH": str(ROOT)}
        out[knob] = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True,
                                   check=True).stdout.split()
    assert out["0"] == ["0", "0", "0"] and out["1"] == ["4", "1", "1"]


def test_wrappers_on_cpu_use_dequantized_weights(listed):
    g = torch.Generator().manual_seed(5)
    K, N, M = 2048, 64, 3
    w = (torch.randn(N, K, generator=g) * 0.02).bfloat16()
    q, s = ops.quantize_fp8_rows(w)
    wd = ops.dequantize_fp8_rows(q, s, torch.bfloat16)
    x = torch.randn(M, K, generator=g).bfloat16()
    P = ops.dgemm8_partial(x, q, s, 2)
    assert P.shape == (2, M, N) and torch.equal(P, ops.dgemm_partial(x, wd, 2))
    assert torch.equal(ops.dgemm8_glu(x, q, s), ops.glu_linear(x, wd))
    ids = ops.lm_head_argmax(x, wd, N - 3, fp8=(q, s))
    assert torch.equal(ids, F.linear(x, wd[: N - 3]).float().argmax(1))


def _decode3(m):
    """Prefill three prompts, then one 3-row decode step on the CPU; the step's logits."""
    from docqa_amd.engine.kv_cache import KVCache

    BS = 16
    kv = KVCache(m.cfg.layers, 12, m.hkv, m.cfg.head_dim, BS, device="cpu", dtype=m.dtype).caches
    g = torch.Generator().manual_seed(4)
    lens = [23, 9, 30]
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
    bt = torch.zeros(3, maxb, dtype=torch.int32)
    for i, t in enumerate(tables):
        bt[i, :len(t)] = torch.tensor(t)
    meta = AttnMeta(prefill=False, positions=torch.tensor(lens, dtype=torch.int32),
                    slot_mapping=torch.tensor([tables[i][n // BS] * BS + n % BS for i, n in enumerate(lens)],
                                              dtype=torch.int32),
                    block_tables=bt, context_lens=torch.tensor([n + 1 for n in lens], dtype=torch.int32),
                    max_context=maxb * BS)
    return m.forward(torch.tensor([4, 5, 6], dtype=torch.int32), meta, kv)


def test_quantized_cpu_model_three_row_decode_equals_plain_model_on_the_image(monkeypatch):
    cfg = LlamaConfig.preset("tiny")
    m = LlamaModel(cfg, device="cpu", seed=3)
    m.quantize_fp8()
    p = LlamaModel(cfg, device="cpu", init=False)
    p.load_state_dict_hf(m.export_state_dict_hf())
    assert p.fp8 is None
    calls = []
    for name in ("dgemm8_partial", "dgemm8_glu"):    # the CPU never takes use8
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **k: calls.append(_n))
    a = _decode3(m)
    assert a.shape == (3, cfg.vocab_size) and not calls
    assert torch.equal(a, _decode3(p))
