"""MXFP4 weight streaming at 2..32 decode rows, the parts that need no GPU: the plan functions
(row range, K granule, the DOCQA_DGEMM4 knob), the CPU fallbacks of the wrappers, and a
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
    monkeypatch.setattr(ops, "_DGEMM4", True)
    monkeypatch.setattr(ops, "_DGEMM4_SLAB", {(4096, 4096): BUCKETS, (4096, 14336): BUCKETS, (4096, 5120): BUCKETS})
    monkeypatch.setattr(ops, "_DGEMM4_GLU", {(28672, 4096): (2, 8)})
    monkeypatch.setattr(ops, "_DGEMM4_LM", {(128256, 4096): BUCKETS})


def test_plan_functions_row_range_and_granule(listed):
    top = ops.DGEMM4_MAX_ROWS
    assert top == 32 and ops.DGEMM4_K == 2048
    assert ops.dgemm4_plan(1, 4096, 4096) == (0, 64)              # one row: the GEMV's
    assert ops.dgemm4_plan(2, 4096, 4096) == (2, 64)              # 2 ring turns: at most 2 slices (128 workgroups)
    assert ops.dgemm4_plan(top, 4096, 4096) == (2, 64)
    assert ops.dgemm4_plan(top + 1, 4096, 4096) == (0, 64)
    assert ops.dgemm4_plan(5, 4096, 14336) == (7, 64)             # 7 turns: 1 slice gives 64 workgroups, 7 give 448
    assert ops.dgemm4_plan(2, 4096, 5120) == (0, 64)              # listed, but K is 2.5 ring turns
    assert ops.dgemm4_plan(2, 6144, 4096) == (0, 64)              # not listed: stays on W'
    assert not ops.dgemm4_glu_ok(1, 28672, 4096) and ops.dgemm4_glu_ok(2, 28672, 4096)
    assert not ops.dgemm4_glu_ok(3, 28672, 4096)                  # bucket 4 is not listed
    assert ops.dgemm4_glu_ok(5, 28672, 4096) and not ops.dgemm4_glu_ok(9, 28672, 4096)
    assert not ops.dgemm4_argmax_ok(1, 128256, 4096) and not ops.dgemm4_argmax_ok(top + 1, 128256, 4096)
    assert ops.dgemm4_argmax_ok(2, 128256, 4096) and ops.dgemm4_argmax_ok(top, 128256, 4096)
    # the split rule alone: smallest S of whole ring turns with >= 192 workgroups, else all turns
    assert ops.dgemm4_splits(6144, 4096) == 2                     # 96 tiles x 2
    assert ops.dgemm4_splits(2048, 2048) == 1                     # one turn
    assert ops.dgemm4_splits(2048, 8192) == 4                     # 32 tiles x 4 = 128 < 192: every turn
    assert ops.dgemm4_splits(4096, 14336) == 7                    # 7 is prime: 1 or 7
    assert ops.dgemm4_splits(28672, 4096) == 1                    # 448 tiles
    assert ops.dgemm4_splits(4096, 4096 + 1024) == 0 and ops.dgemm4_splits(4100, 4096) == 0
    assert ops.dgemm4_splits(4096, 1024) == 0                     # less than one turn


def test_shipped_tables_list_only_shapes_the_kernel_takes():
    for table in (ops._DGEMM4_SLAB, ops._DGEMM4_GLU, ops._DGEMM4_LM):
        for (N, K), buckets in table.items():
            assert N % 64 == 0 and K % ops.DGEMM4_K == 0 and ops.dgemm4_splits(N, K) >= 1
            assert set(buckets) <= set(BUCKETS)


def test_knob_disables_every_plan():
    code = ("from docqa_amd import ops\n"
            "ops._DGEMM4_SLAB[(4096, 4096)] = (2,)\nops._DGEMM4_GLU[(128, 2048)] = (2,)\n"
            "ops._DGEMM4_LM[(128, 2048)] = (2,)\n"
            "print(ops.dgemm4_plan(2, 4096, 4096)[0], int(ops.dgemm4_glu_ok(2, 128, 2048)), "
            "int(ops.dgemm4_argmax_ok(2, 128, 2048)))")
    out = {}
    for knob in ("0", "1"):
        env = {**os.environ, "DOCQA_DGEMM4": knob, "PYTHONPATH": str(ROOT)}
        out[knob] = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True,
                                   check=True).stdout.split()
    assert out["0"] == ["0", "0", "0"] and out["1"] == ["2", "1", "1"]


def test_wrappers_on_cpu_use_dequantized_weights(listed):
    g = torch.Generator().manual_seed(5)
    K, N, M = 4096, 64, 3
    w = (torch.randn(N, K, generator=g) * 0.02).bfloat16()
    q, e = ops.quantize_mxfp4_rows(w)
    wd = ops.dequantize_mxfp4_rows(q, e, torch.bfloat16)
    x = torch.randn(M, K, generator=g).bfloat16()
    P = ops.dgemm4_partial(x, q, e, 2)
    assert P.shape == (2, M, N) and torch.equal(P, ops.dgemm_partial(x, wd, 2))
    assert torch.equal(ops.dgemm4_glu(x, q, e), ops.glu_linear(x, wd))
    ids = ops.lm_head_argmax(x, wd, N - 3, mxfp4=(q, e))
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
    m.quantize_mxfp4()
    p = LlamaModel(cfg, device="cpu", init=False)
    p.load_state_dict_hf(m.export_state_dict_hf())
    assert p.mx4 is None
    # list the model's own shapes: even then the CPU never takes use4
    L0 = m.layers[0]
    monkeypatch.setattr(ops, "_DGEMM4_SLAB", {tuple(L0[k].shape): BUCKETS for k in ("qkv", "o", "down")})
    monkeypatch.setattr(ops, "_DGEMM4_GLU", {tuple(L0["gate_up"].shape): BUCKETS})
    calls = []
    for name in ("dgemm4_partial", "dgemm4_glu"):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **k: calls.append(_n))
    a = _decode3(m)
    assert a.shape == (3, cfg.vocab_size) and not calls
    assert torch.equal(a, _decode3(p))
